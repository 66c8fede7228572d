"""Sessions in the cached generator, host side (no GPU): the schedule ``plan_sessions`` deals, every
refusal of lbwn_gen_begin that needs no device (EINVAL before any launch, the message naming the
argument), the "sessions" tensor, and the Python layer's own argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

from lbwn import _lib
from lbwn.imodel import WaveNetGen, plan_sessions
from tests.conftest import ROOT
from tests.test_gen_lc import SMALL_LC, c_arch, make_plan, tensor

sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

SMALL_GC = dict(SMALL_LC, n_gc_embed=8, n_gc_category=5)


# ---- plan_sessions ----------------------------------------------------------------------------
def brute_force_total(lengths, B, chunk):
    """Step by step: at every chunk boundary a slot whose utterance is covered takes the next waiting one;
    the run ends at the first step at which nothing waits and everything is covered."""
    left, nxt, t = [0] * B, 0, 0
    while True:
        if t % chunk == 0:
            for s in range(B):
                if left[s] <= 0 and nxt < len(lengths):
                    left[s] = lengths[nxt]
                    nxt += 1
        if nxt == len(lengths) and max(left) <= 0:
            return t
        left = [r - 1 for r in left]
        t += 1


CASES = [([5], 1, 4), ([5], 3, 4), ([3, 9, 2, 7, 7, 1, 12], 3, 4), ([1, 1, 1, 1], 2, 8), ([2, 3], 4, 16),
         ([16, 40, 72, 24, 8, 64, 56], 3, 10), ([7] * 9, 1, 7), ([100, 1, 1, 1, 1, 1], 2, 5)]


@pytest.mark.parametrize('lengths,B,chunk', CASES)
def test_plan_sessions_properties(lengths, B, chunk):
    rounds, total = plan_sessions(lengths, B, chunk)
    assert total == sum(st for st, _ in rounds) == brute_force_total(lengths, B, chunk)
    dealt, t = [], 0
    busy_until = [0] * B                  # the step at which the slot's current session is covered
    for steps, begins in rounds:
        assert 1 <= steps <= chunk
        assert len(set(s for s, _ in begins)) == len(begins)          # no slot twice in a round
        for slot, u in begins:
            assert 0 <= slot < B
            assert busy_until[slot] <= t, 'slot %d replaced before its session was covered' % slot
            busy_until[slot] = t + lengths[u]
            dealt.append(u)
        t += steps
    assert dealt == list(range(len(lengths)))                         # each exactly once, first in first out
    assert max(busy_until) <= total                                   # the run covers every session
    # only the rounds after the last begin may be shorter than a chunk
    last = max(i for i, (_, b) in enumerate(rounds) if b)
    assert all(st == chunk for st, _ in rounds[:last])


def test_plan_sessions_random_against_brute_force():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, B, chunk = int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.integers(1, 20))
        lengths = [int(v) for v in rng.integers(1, 60, n)]
        assert plan_sessions(lengths, B, chunk)[1] == brute_force_total(lengths, B, chunk)


def test_plan_sessions_edges_and_errors():
    assert plan_sessions([], 3, 4) == ([], 0)
    assert plan_sessions([5], 1, 4) == ([(4, [(0, 0)]), (1, [])], 5)                 # B = 1, one utterance
    assert plan_sessions([2, 3], 2, 16) == ([(3, [(0, 0), (1, 1)])], 3)             # lengths below one chunk
    assert plan_sessions([2, 3, 1], 2, 16) == ([(16, [(0, 0), (1, 1)]), (1, [(0, 2)])], 17)
    for bad in (([0], 2, 4), ([3], 0, 4), ([3], 2, 0), ([3], True, 4)):
        with pytest.raises(ValueError, match='plan_sessions'):
            plan_sessions(*bad)


# ---- lbwn_gen_begin: refusals that need no device ---------------------------------------------
def fake_params():
    P = _lib.Params()
    for f, _ in _lib.Params._fields_:
        if f != 'lc_up':
            setattr(P, f, 0x1000)
    for i in range(8):
        P.lc_up[i] = 0x1000
    return P


def sessions(*entries):
    arr = (_lib.GenSession * max(1, len(entries)))()
    for i, (slot, gc, key, mel, fr) in enumerate(entries):
        arr[i].slot, arr[i].gc_id, arr[i].key, arr[i].mel, arr[i].n_frames = slot, gc, key, mel, fr
    return arr


SZ = ctypes.sizeof(_lib.GenSession)
FAKE = 0x1000       # never dereferenced: every call below returns before a launch


def refused(lib, h, P, arr, n, needle, ws=FAKE, size=SZ):
    assert lib.lbwn_gen_begin(h, ctypes.byref(P) if P is not None else None, ws, arr, n, size, None) == 22
    msg = lib.lbwn_last_error()
    assert needle in msg, msg


def test_gen_begin_is_exported_and_struct_matches_header():
    import re
    lib = _lib.load()
    assert hasattr(lib, 'lbwn_gen_begin') and 'lbwn_gen_begin' in _lib.EXPORTED
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_gen_session \{(.*?)\} lbwn_gen_session;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [re.findall(r'\w+', d)[-1] for d in body.split(';') if d.strip()]
    assert fields == [n for n, _ in _lib.GenSession._fields_]
    assert SZ == 32


def test_gen_begin_refusals_lc_plan():
    lib = _lib.load()
    P = fake_params()
    h = make_plan(lib, c_arch(SMALL_LC), 3, 65)                # hop 8: 9 frames reserved
    ok = (0, 0, 0, FAKE, 8)
    refused(lib, None, P, sessions(ok), 1, b'plan is null')
    refused(lib, h, None, sessions(ok), 1, b'params is null')
    refused(lib, h, P, sessions(ok), 1, b'workspace is null', ws=None)
    refused(lib, h, P, None, 1, b's (the session array) is null')
    for bad in (0, SZ - 8, SZ + 8):
        refused(lib, h, P, sessions(ok), 1, b'struct_size %d != %d' % (bad, SZ), size=bad)
    for n in (0, -1, 4):
        refused(lib, h, P, sessions(ok, ok, ok, ok), n, b'n = %d' % n)
    refused(lib, h, P, sessions((3, 0, 0, FAKE, 8)), 1, b's[0].slot = 3')
    refused(lib, h, P, sessions((-1, 0, 0, FAKE, 8)), 1, b's[0].slot = -1')
    refused(lib, h, P, sessions(ok, (1, 0, 1, FAKE, 8), (0, 0, 2, FAKE, 8)), 3, b's[2].slot = 0 is listed twice')
    refused(lib, h, P, sessions((0, 0, -1, FAKE, 8)), 1, b's[0].key = -1')
    refused(lib, h, P, sessions(ok, (1, 0, 2 ** 31, FAKE, 8)), 2, b's[1].key = 2147483648')
    refused(lib, h, P, sessions((0, 0, 0, None, 8)), 1, b's[0].mel is null')
    refused(lib, h, P, sessions((0, 0, 0, FAKE + 4, 8)), 1, b's[0].mel 0x1004 is not 16-byte aligned')
    refused(lib, h, P, sessions((0, 0, 0, FAKE, 0)), 1, b's[0].n_frames = 0')
    refused(lib, h, P, sessions(ok, (1, 0, 1, FAKE, 10)), 2, b's[1].n_frames = 10')
    refused(lib, h, P, sessions((0, 0, 0, FAKE, 2 ** 62)), 1, b'n_frames')
    # gc_id is ignored on an arch without GC: the next check speaks
    refused(lib, h, P, sessions((0, 99, 0, None, 8)), 1, b'mel is null')
    # nothing above changed the mode: an LC plan still has no mel
    assert lib.lbwn_gen_run(h, ctypes.byref(P), FAKE, 4, None) == 22
    assert b'without a mel' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)


def test_gen_begin_refusals_gc_and_no_lc():
    lib = _lib.load()
    P = fake_params()
    h = make_plan(lib, c_arch(SMALL_GC, lc=False), 3, 65)      # GC, no LC
    refused(lib, h, P, sessions((0, 0, 0, FAKE, 0)), 1, b's[0].mel is given, but the arch has no local conditioning')
    refused(lib, h, P, sessions((0, 6, 0, None, 0)), 1, b's[0].gc_id = 6')
    refused(lib, h, P, sessions((0, 5, 0, None, 0), (1, -1, 1, None, 0)), 2, b's[1].gc_id = -1')
    lib.lbwn_gen_plan_destroy(h)


@pytest.mark.parametrize('B', [3, 10, 80])
def test_sessions_tensor_is_reported_and_costs_no_workspace(B, monkeypatch):
    """"sessions" is int64 [B][4] at the very end of the workspace, 256-byte aligned, on every plan; it
    lies over the prefill scratch, so the workspace is no larger than its parts were."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    lib = _lib.load()
    for a in (c_arch(SMALL_LC), c_arch(SMALL_LC, lc=False)):
        h = make_plan(lib, a, B, 65)
        ret, off, nb = tensor(lib, h, 'sessions')
        ws = lib.lbwn_gen_workspace_bytes(h)
        assert ret == 0 and nb == 32 * B and off % 256 == 0
        assert off + (nb + 255) // 256 * 256 == ws
        for other in ('samples', 'wav', 'logits', 'rings', 'step') + (('lc', 'lccond') if a.n_lc_out else ()):
            _, o2, n2 = tensor(lib, h, other)
            assert o2 + n2 <= off, other
        lib.lbwn_gen_plan_destroy(h)


def test_sessions_tensor_with_the_smallest_prefill_scratch(monkeypatch):
    """A prefill slice of one position, one narrow layer and many streams: the words (16000 bytes) still
    end the workspace and lie behind every tensor a session run uses."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '1')
    lib = _lib.load()
    a = c_arch(dict(SMALL_LC, n_blocks=1, n_block_layers=1, n_res=4, n_dil=4), lc=False)
    h = make_plan(lib, a, 500, 8)
    ret, off, nb = tensor(lib, h, 'sessions')
    assert ret == 0 and nb == 32 * 500 and off + 16128 == lib.lbwn_gen_workspace_bytes(h)
    for other in ('samples', 'wav', 'logits', 'rings', 'step'):
        _, o2, n2 = tensor(lib, h, other)
        assert o2 + n2 <= off, other
    lib.lbwn_gen_plan_destroy(h)


# ---- the Python layer's own checks -------------------------------------------------------------
def _cpu_gen(B=3, gc=0, lc=True):
    a = SMALL_LC
    return WaveNetGen(a['n_blocks'], a['n_block_layers'], a['n_quant'], a['n_res'], a['n_dil'], a['n_skip'],
                      a['n_post'], 8 if gc else 0, gc, True, B, 10, None, device='cpu',
                      n_lc_in=12 if lc else 0, n_lc_out=16 if lc else 0, lc_upsample=[2, 4] if lc else ())


def test_begin_validates_before_the_library():
    g = _cpu_gen()
    m = np.zeros((4, 12), np.float32)
    for slots, mels, match in (([], [], 'slots'), ([0, 1, 2, 0], [m] * 4, 'slots'), ([3], [m], r'slots\[0\]'),
                               ([0, 0], [m, m], 'twice'), ([True], [m], r'slots\[0\]'),
                               ([0], None, 'mels'), ([0, 1], [m], 'mels has 1'),
                               ([0], [np.zeros((4, 11), np.float32)], r'mels\[0\]'),
                               ([0], [np.zeros((0, 12), np.float32)], r'mels\[0\]')):
        with pytest.raises(ValueError, match=match):
            g.begin(slots, mels)
    with pytest.raises(ValueError, match=r'keys\[0\]'):
        g.begin([0], [m], keys=[-1])
    with pytest.raises(ValueError, match=r'keys\[0\]'):
        g.begin([0], [m], keys=[2 ** 31])
    with pytest.raises(ValueError, match='keys has 2'):
        g.begin([0], [m], keys=[1, 2])
    with pytest.raises(RuntimeError, match='no run'):
        g.begin([0], [m])
    with pytest.raises(ValueError, match=r'mels\[0\] has shape'):
        g.begin([0], [[[0.0] * 11] * 4])                       # a nested list is converted, then checked
    with pytest.raises(ValueError, match=r'mels\[0\] is not an array'):
        g.begin([0], [[[0.0] * 12, [0.0] * 11]])                # ragged
    with pytest.raises(RuntimeError, match='no run'):
        g.begin([0], [[[0.0] * 12] * 4])                       # a good nested list passes the checks
    g = _cpu_gen(gc=5)
    with pytest.raises(ValueError, match='gc_ids'):
        g.begin([0], [m])
    with pytest.raises(ValueError, match=r'gc_ids\[0\]'):
        g.begin([0], [m], gc_ids=[6])
    g = _cpu_gen(lc=False)
    with pytest.raises(ValueError, match='no local conditioning'):
        g.begin([0], [m])
    with pytest.raises(ValueError, match='no local conditioning'):
        g.vocode([m])
    with pytest.raises(ValueError, match='begun no session'):
        g.take(0, 4)


def test_vocode_validates_before_the_library():
    g = _cpu_gen()
    assert g.vocode([]) == []
    with pytest.raises(ValueError, match=r'mels\[1\]'):
        g.vocode([np.zeros((4, 12), np.float32), np.zeros((4, 13), np.float32)])
    with pytest.raises(ValueError, match=r'mels\[0\]'):
        g.vocode([[[0.0] * 13] * 4])
    with pytest.raises(ValueError, match='keys'):
        g.vocode([np.zeros((4, 12), np.float32)], keys=[1, 2])
    with pytest.raises(ValueError, match='gc_ids'):
        _cpu_gen(gc=5).vocode([np.zeros((4, 12), np.float32)])


def test_generate_cli_mel_list_errors(tmp_path, capsys):
    """--mel-list: an arch without LC is refused with a message; so are a missing list, a malformed line
    and a mel of the wrong width, all before any device work."""
    import json
    import generate
    from lbwn.ckpt import ckpt_file
    a = generate.get_args(['--mel-list', 'l.txt', 'arch.json', 'ckpt', 'out'])
    assert a.mel_list == 'l.txt' and generate.get_args(['arch.json', 'ckpt', 'out']).mel_list is None
    open(ckpt_file(str(tmp_path / 'ck')), 'wb').close()
    no_lc = {k: v for k, v in SMALL_LC.items() if not k.startswith(('n_lc', 'lc_'))}
    af0, af = tmp_path / 'arch0.json', tmp_path / 'arch.json'
    af0.write_text(json.dumps(dict(no_lc, wav_input_type='mu_law_quant')))
    af.write_text(json.dumps(dict(SMALL_LC, wav_input_type='mu_law_quant')))
    np.save(tmp_path / 'm.npy', np.zeros((4, 12), np.float32))
    np.save(tmp_path / 'bad.npy', np.zeros((4, 11), np.float32))
    lst = tmp_path / 'list.txt'
    lst.write_text('0\t%s\tfirst\n' % (tmp_path / 'm.npy'))

    def fails(argv, needle):
        with pytest.raises(SystemExit) as e:
            generate.main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 1 and needle in err, err

    tail = [str(tmp_path / 'ck'), str(tmp_path / 'out')]
    fails(['--mel-list', str(lst), str(af0)] + tail, 'no local conditioning')
    fails(['--mel-list', str(tmp_path / 'none.txt'), str(af)] + tail, "Couldn't find")
    fails(['--mel-list', str(lst), '--mel-npy', str(tmp_path / 'm.npy'), str(af)] + tail, '--mel-list')
    lst.write_text('0\n')
    fails(['--mel-list', str(lst), str(af)] + tail, 'line 1')
    lst.write_text('x\t%s\n' % (tmp_path / 'm.npy'))
    fails(['--mel-list', str(lst), str(af)] + tail, 'line 1')
    lst.write_text('0\t%s\n0\t%s\n' % (tmp_path / 'm.npy', tmp_path / 'bad.npy'))
    fails(['--mel-list', str(lst), str(af)] + tail, 'line 2')
    lst.write_text('0\t%s\tsame\n0\t%s\tsame\n' % (tmp_path / 'm.npy', tmp_path / 'm.npy'))
    fails(['--mel-list', str(lst), str(af)] + tail, 'same')


def test_mel_list_groups():
    """The byte budget splits a list into consecutive groups, each within the budget unless a single
    utterance alone exceeds it (then it is a group of its own)."""
    import generate
    lengths = [800, 1600, 400, 2400, 800, 800]
    # batch_sz x (samples + wav + an lc row + a quarter row of the first stage's scratch) bytes per step
    per_step = 3 * (8 + 4 * 16 + 16)
    assert generate.mel_list_bytes(800, 3, 16, [2, 4]) == per_step * 800
    assert generate.mel_list_bytes(801, 3, 16, [2, 4]) == 3 * (8 * 801 + 64 * 808 + 64 * 202)
    assert generate.mel_list_bytes(800, 2, 16, [8]) == 2 * (8 + 64) * 800       # one stage: no scratch
    g = generate.mel_list_groups(lengths, 3, 100, 16, [2, 4], 10 ** 12)
    assert g == [list(range(6))]
    budget = per_step * 2500
    g = generate.mel_list_groups(lengths, 3, 100, 16, [2, 4], budget)
    assert [u for grp in g for u in grp] == list(range(6)) and len(g) > 1
    for grp in g:
        total = plan_sessions([lengths[u] for u in grp], 3, 100)[1]
        assert len(grp) == 1 or generate.mel_list_bytes(total, 3, 16, [2, 4]) <= budget
    assert generate.mel_list_groups(lengths, 3, 100, 16, [2, 4], 1) == [[u] for u in range(6)]
