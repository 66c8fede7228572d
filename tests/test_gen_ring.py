"""Ring plans of the cached generator, host side (no GPU): every refusal of lbwn_gen_plan_create_ex,
lbwn_gen_extend and lbwn_gen_collect that needs no device (EINVAL before any launch, the message naming the
argument), what a ring plan refuses elsewhere, the workspace arithmetic, the scheduler ``plan_ring`` against
a plain simulation of its rounds, and the Python layer's own checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from lbwn import _lib
from lbwn.imodel import WaveNetGen, plan_ring, plan_sessions, ring_rounds
from tests.conftest import ROOT
from tests.test_gen_lc import SMALL_LC, c_arch, make_plan, tensor
from tests.test_gen_sessions import FAKE, fake_params, sessions

TENSORS = ('rings', 'logits', 'step', 'status', 'teacher', 'samples', 'wav', 'trace', 'sessions')
LC_TENSORS = ('lc', 'lccond', 'pfcond')


def make_ex(lib, a, B, max_steps, ring, max_teacher=0, expect=0, size=None):
    args = _lib.GenPlanArgs(batch_sz=B, max_steps=max_steps, max_teacher=max_teacher, ring_steps=ring)
    if size is not None:
        args.struct_size = size
    h = ctypes.c_void_p()
    assert lib.lbwn_gen_plan_create_ex(ctypes.byref(a), ctypes.byref(args), ctypes.byref(h)) == expect, \
        lib.lbwn_last_error()
    return h


def entries(*es):
    arr = (_lib.GenExtendEntry * max(1, len(es)))()
    for i, (slot, mel, fr) in enumerate(es):
        arr[i].slot, arr[i].mel, arr[i].n_frames = slot, mel, fr
    return arr


ESZ = ctypes.sizeof(_lib.GenExtendEntry)


def ext_refused(lib, h, P, arr, n, needle, ws=FAKE, size=ESZ):
    assert lib.lbwn_gen_extend(h, ctypes.byref(P) if P is not None else None, ws, arr, n, size, None) == 22
    assert needle in lib.lbwn_last_error(), lib.lbwn_last_error()


def col_refused(lib, h, needle, ws=FAKE, slot=0, i0=0, n=4, wav=FAKE, smp=FAKE):
    assert lib.lbwn_gen_collect(h, ws, slot, i0, n, wav, smp, None) == 22
    assert needle in lib.lbwn_last_error(), lib.lbwn_last_error()


# ---- 9. exports and structs ------------------------------------------------------------------------
def test_ring_entry_points_are_exported_and_structs_match_the_header():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    for name in ('lbwn_gen_plan_create_ex', 'lbwn_gen_extend', 'lbwn_gen_collect'):
        assert hasattr(lib, name) and name in _lib.EXPORTED
    for cname, cls, size in (('lbwn_gen_plan_args', _lib.GenPlanArgs, 40), ('lbwn_gen_extend_entry', _lib.GenExtendEntry, 24)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), txt, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.findall(r'\w+', d)[-1] for d in body.split(';') if d.strip()]
        assert fields == [n for n, _ in cls._fields_]
        assert ctypes.sizeof(cls) == size
    assert lib.lbwn_abi_version() == 5


# ---- 6. the EINVAL table ---------------------------------------------------------------------------
def test_plan_create_ex_refusals():
    lib = _lib.load()
    a = c_arch(SMALL_LC)
    h = ctypes.c_void_p()
    args = _lib.GenPlanArgs(batch_sz=3, max_steps=65, max_teacher=0, ring_steps=64)
    for arch_p, args_p, out_p, needle in ((None, ctypes.byref(args), ctypes.byref(h), b'arch is null'),
                                          (ctypes.byref(a), None, ctypes.byref(h), b'args is null'),
                                          (ctypes.byref(a), ctypes.byref(args), None, b'out is null')):
        assert lib.lbwn_gen_plan_create_ex(arch_p, args_p, out_p) == 22
        assert needle in lib.lbwn_last_error(), lib.lbwn_last_error()
    size = ctypes.sizeof(_lib.GenPlanArgs)
    for bad in (0, size - 8, size + 8):
        make_ex(lib, a, 3, 65, 64, expect=22, size=bad)
        assert b'struct_size %d != %d' % (bad, size) in lib.lbwn_last_error()
    make_ex(lib, a, 3, 65, -1, expect=22)
    assert b'ring_steps = -1' in lib.lbwn_last_error()
    make_ex(lib, a, 3, 65, 2 ** 31, expect=22)
    assert b'ring_steps' in lib.lbwn_last_error()
    make_ex(lib, a, 3, 65, 2 ** 31 - 4, expect=22)               # Rlc = 2^31 rows
    assert b'ring_steps too large' in lib.lbwn_last_error()
    make_ex(lib, a, 0, 65, 64, expect=22)                        # lbwn_gen_plan_create's own refusals
    make_ex(lib, a, 3, 0, 64, expect=22)


def test_ring_plan_refuses_prefill_score_teacher_and_long_begins():
    lib = _lib.load()
    P = fake_params()
    h = make_ex(lib, c_arch(SMALL_LC), 3, 1, 60, max_teacher=8)   # hop 8: Rlc = 64 rows, 8 frames
    assert lib.lbwn_gen_prefill(h, ctypes.byref(P), FAKE, FAKE, 0, 4, None) == 22
    assert b'prefill: not supported on a ring plan' in lib.lbwn_last_error()
    assert lib.lbwn_gen_score(h, ctypes.byref(P), FAKE, FAKE, 0, 4, FAKE, 4, FAKE, None) == 22
    assert b'score: not supported on a ring plan' in lib.lbwn_last_error()
    assert lib.lbwn_gen_start(h, ctypes.byref(P), FAKE, None, FAKE, 4, 0, 1, None) == 22
    assert b'n_teacher = 4 on a ring plan' in lib.lbwn_last_error()
    SZ = ctypes.sizeof(_lib.GenSession)
    assert lib.lbwn_gen_begin(h, ctypes.byref(P), FAKE, sessions((0, 0, 0, FAKE, 9)), 1, SZ, None) == 22
    assert b's[0].n_frames = 9 must be in 1..8' in lib.lbwn_last_error()
    assert lib.lbwn_gen_set_mel(h, ctypes.byref(P), FAKE, FAKE, 9, None) == 22      # n_frames·hop <= Rlc there too
    assert b'9 frames' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)


@pytest.mark.parametrize('ring', [0, 64])
def test_gen_extend_refusals(ring):
    lib = _lib.load()
    P = fake_params()
    h = make_ex(lib, c_arch(SMALL_LC), 3, 65, ring)
    ok = (0, FAKE, 2)
    ext_refused(lib, None, P, entries(ok), 1, b'plan is null')
    ext_refused(lib, h, None, entries(ok), 1, b'params is null')
    ext_refused(lib, h, P, entries(ok), 1, b'workspace is null', ws=None)
    ext_refused(lib, h, P, None, 1, b'e (the entry array) is null')
    for bad in (0, ESZ - 8, ESZ + 8):
        ext_refused(lib, h, P, entries(ok), 1, b'struct_size %d != %d' % (bad, ESZ), size=bad)
    for n in (0, -1, 4):
        ext_refused(lib, h, P, entries(ok, ok, ok, ok), n, b'n = %d' % n)
    ext_refused(lib, h, P, entries((3, FAKE, 2)), 1, b'e[0].slot = 3')
    ext_refused(lib, h, P, entries((-1, FAKE, 2)), 1, b'e[0].slot = -1')
    # what the entries alone decide comes first, for every entry
    ext_refused(lib, h, P, entries(ok, (1, FAKE, 2), (0, FAKE, 2)), 3, b'e[2].slot = 0 is listed twice')
    ext_refused(lib, h, P, entries((0, None, 2)), 1, b'e[0].mel is null')
    ext_refused(lib, h, P, entries(ok, (1, None, 2)), 2, b'e[1].mel is null')
    ext_refused(lib, h, P, entries((0, FAKE + 4, 2)), 1, b'e[0].mel 0x1004 is not 16-byte aligned')
    most = 8 if ring else 9                    # hop 8: Rlc = 64 rows; without a ring ceil(65 / 8) frames reserved
    for fr in (0, -3, most + 1, 2 ** 62):
        ext_refused(lib, h, P, entries(ok, (2, FAKE, fr)), 2, b'e[1].n_frames = %d must be in 1..%d' % (fr, most))
    # then the run: no stream has begun a session (no lbwn_gen_begin since plan creation)
    ext_refused(lib, h, P, entries(ok), 1, b'e[0].slot = 0 has begun no session')
    ext_refused(lib, h, P, entries((1, FAKE, most)), 1, b'e[0].slot = 1 has begun no session')
    lib.lbwn_gen_plan_destroy(h)
    h = make_ex(lib, c_arch(SMALL_LC, lc=False), 3, 65, ring)
    ext_refused(lib, h, P, entries(ok), 1, b'the arch has no local conditioning')
    lib.lbwn_gen_plan_destroy(h)


@pytest.mark.parametrize('ring', [0, 64])
def test_gen_collect_refusals(ring):
    lib = _lib.load()
    h = make_ex(lib, c_arch(SMALL_LC), 3, 65, ring)
    col_refused(lib, None, b'plan is null')
    col_refused(lib, h, b'workspace is null', ws=None)
    col_refused(lib, h, b'slot = 3', slot=3)
    col_refused(lib, h, b'slot = -1', slot=-1)
    col_refused(lib, h, b'i0 = -1', i0=-1)
    col_refused(lib, h, b'n = -2', n=-2)
    col_refused(lib, h, b'n = %d' % (2 ** 63 - 1), i0=1, n=2 ** 63 - 1)
    col_refused(lib, h, b'wav_out and samples_out are both null', wav=None, smp=None)
    assert lib.lbwn_gen_collect(h, FAKE, 0, 0, 0, FAKE, None, None) == 0        # n = 0: nothing is launched
    lib.lbwn_gen_plan_destroy(h)


# ---- 7. workspace arithmetic -----------------------------------------------------------------------
@pytest.mark.parametrize('lc', [True, False])
def test_ring_zero_is_the_plain_plan(lc, monkeypatch):
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    lib = _lib.load()
    a = c_arch(SMALL_LC, lc=lc)
    for B, steps, teach in ((3, 65, 0), (10, 1000, 17), (80, 77, 0)):
        h0 = ctypes.c_void_p()
        assert lib.lbwn_gen_plan_create(ctypes.byref(a), B, steps, teach, ctypes.byref(h0)) == 0
        h1 = make_ex(lib, a, B, steps, 0, max_teacher=teach)
        assert lib.lbwn_gen_workspace_bytes(h0) == lib.lbwn_gen_workspace_bytes(h1) > 0
        for name in TENSORS + (LC_TENSORS if lc else ()):
            assert tensor(lib, h0, name) == tensor(lib, h1, name), name
            assert tensor(lib, h0, name)[0] == 0, name
        lib.lbwn_gen_plan_destroy(h0)
        lib.lbwn_gen_plan_destroy(h1)


@pytest.mark.parametrize('lc', [True, False])
@pytest.mark.parametrize('B,R', [(3, 64), (3, 60), (10, 1), (80, 129)])
def test_ring_plan_sizes_do_not_depend_on_max_steps(lc, B, R, monkeypatch):
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    lib = _lib.load()
    a = c_arch(SMALL_LC, lc=lc)
    hop, Lo = 8, 16
    Rlc = -(-R // hop) * hop
    seen = set()
    for steps in (1, 65, 10 ** 6, 2 ** 40):
        h = make_ex(lib, a, B, steps, R)
        seen.add(lib.lbwn_gen_workspace_bytes(h))
        assert tensor(lib, h, 'samples')[2] == tensor(lib, h, 'wav')[2] == 4 * B * R
        if lc:
            assert tensor(lib, h, 'lc')[2] == 4 * B * Rlc * Lo
        else:
            assert tensor(lib, h, 'lc')[0] == 22
        lib.lbwn_gen_plan_destroy(h)
    assert len(seen) == 1
    # and it is the plain plan of max_steps = R: the rings replace the schedule-sized tensors one for one
    h = make_plan(lib, a, B, R)
    assert seen == {lib.lbwn_gen_workspace_bytes(h)}
    lib.lbwn_gen_plan_destroy(h)
    # a plain plan for a schedule of 100 rings is larger by the outputs (and the lc rows) of 99 of them
    h = make_plan(lib, a, B, 100 * R)
    assert lib.lbwn_gen_workspace_bytes(h) > max(seen)
    lib.lbwn_gen_plan_destroy(h)


# ---- 8. the scheduler ------------------------------------------------------------------------------
def simulate(lengths, B, chunk, R, hop, rounds):
    """Run the rounds in plain Python; returns the total.  Asserts every invariant of plan_ring's docstring."""
    Rlc = -(-R // hop) * hop
    sess = [None] * B                   # per slot: utterance, local step, rows fed, frames fed
    got = {u: 0 for u in range(len(lengths))}
    dealt, total = [], 0
    for steps, begins, extends, collects in rounds:
        assert 1 <= steps <= R and steps <= chunk
        for slot, u, nf in begins:
            s = sess[slot]
            assert s is None or s['i'] >= lengths[s['u']], 'slot %d replaced before its utterance was covered' % slot
            assert 1 <= nf <= Rlc // hop and nf <= -(-lengths[u] // hop)
            sess[slot] = dict(u=u, i=0, rows=nf * hop)
            dealt.append(u)
        for slot, u, f0, nf in extends:
            s = sess[slot]
            assert s is not None and s['u'] == u and f0 * hop == s['rows'] and nf >= 1
            assert (f0 + nf) * hop <= -(-lengths[u] // hop) * hop
            s['rows'] += nf * hop
            read = min(max(s['i'] - 1, 0), s['rows'])
            assert s['rows'] - read <= Rlc, 'slot %d holds %d unread rows' % (slot, s['rows'] - read)
        for slot, s in enumerate(sess):
            if s is None:
                continue
            for j in range(s['i'], min(s['i'] + steps, lengths[s['u']])):      # past the end: the clamp is the rule
                assert max(j - 1, 0) < s['rows'], 'slot %d runs step %d with %d rows' % (slot, j, s['rows'])
            s['i'] += steps
        for slot, u, i0, n in collects:
            s = sess[slot]
            assert s['u'] == u and n >= 1 and i0 == got[u], 'utterance %d collected out of order' % u
            assert i0 + n <= min(s['i'], lengths[u]) and i0 >= s['i'] - R
            got[u] += n
        for s in sess:                     # nothing drawn in this round may wait for a later one
            assert s is None or got[s['u']] == min(s['i'], lengths[s['u']])
        total += steps
    assert dealt == list(range(len(lengths)))
    assert got == {u: n for u, n in enumerate(lengths)}
    return total


def test_plan_ring_on_seeded_lists():
    rng = np.random.default_rng(19)
    cut = 0
    for case in range(50):
        B, chunk, R = (1, 3, 10)[case % 3], (7, 10, 64)[(case // 3) % 3], (64, 128)[(case // 9) % 2]
        lengths = [int(v) for v in rng.integers(1, 401, int(rng.integers(1, 25)))]
        rounds, total = plan_ring(lengths, B, chunk, R, 8)
        ref_rounds, ref_total = plan_sessions(lengths, B, chunk)
        assert total == sum(r[0] for r in rounds) == ref_total
        assert simulate(lengths, B, chunk, R, 8, rounds) == total
        # plan_sessions' round structure: the same begins at the same steps
        at, t = [], 0
        for steps, begins, _, _ in rounds:
            at += [(t, slot, u) for slot, u, _ in begins]
            t += steps
        ref_at, t = [], 0
        for steps, begins in ref_rounds:
            ref_at += [(t, slot, u) for slot, u in begins]
            t += steps
        assert at == ref_at
        cut += len(rounds) > len(ref_rounds)
    assert cut > 0          # some case had to cut a round (chunk 64 in a ring of 64 rows)


def test_plan_ring_edges_and_errors():
    assert plan_ring([], 3, 4, 64, 8) == ([], 0)
    # one utterance of 20 frames through a ring of 64: begun with 8 frames, extended as rows are read
    rounds, total = plan_ring([160], 1, 10, 64, 8)
    assert total == 160 and rounds[0] == (10, [(0, 0, 8)], [], [(0, 0, 0, 10)])
    assert rounds[1][2] == [(0, 0, 8, 1)] and sum(nf for r in rounds for _, _, _, nf in r[2]) == 12
    for bad, name in ((([5], 3, 65, 64, 8), 'chunk'), (([5], 0, 4, 64, 8), 'batch_sz'), (([5], 3, 0, 64, 8), 'chunk'),
                      (([5], 3, 4, 0, 8), 'ring_steps'), (([5], 3, 4, 64, 0), 'hop'), (([5], True, 4, 64, 8), 'batch_sz'),
                      (([0], 3, 4, 64, 8), r'lengths\[0\]')):
        with pytest.raises(ValueError, match='plan_ring: ' + name):
            plan_ring(*bad)


def test_ring_rounds_takes_an_endless_iterator():
    def forever():
        while True:
            yield 24
    it = ring_rounds(forever(), 2, 10, 64, 8)
    seen = [next(it) for _ in range(40)]
    assert all(steps == 10 for steps, _, _, _ in seen)
    assert [u for _, b, _, _ in seen for _, u, _ in b] == list(range(sum(len(b) for _, b, _, _ in seen)))


# ---- the Python layer's own checks -----------------------------------------------------------------
def _cpu_gen(B=3, lc=True, **kw):
    a = SMALL_LC
    return WaveNetGen(a['n_blocks'], a['n_block_layers'], a['n_quant'], a['n_res'], a['n_dil'], a['n_skip'],
                      a['n_post'], 0, 0, True, B, 10, None, device='cpu', n_lc_in=12 if lc else 0,
                      n_lc_out=16 if lc else 0, lc_upsample=[2, 4] if lc else (), **kw)


def test_python_layer_validates_before_the_library():
    for bad in (-1, True, 2.5):
        with pytest.raises(ValueError, match='ring_steps'):
            _cpu_gen(ring_steps=bad)
    g = _cpu_gen(ring_steps=64)
    m = np.zeros((2, 12), np.float32)
    for slots, mels, match in (([], [], 'slots'), ([3], [m], r'slots\[0\]'), ([0], [m, m], 'mels has 2'),
                               ([0], [m], 'begun no session')):
        with pytest.raises(ValueError, match=match):
            g.extend(slots, mels)
    with pytest.raises(ValueError, match='slot'):
        g.collect(0, 0, 4)                                   # no plan
    with pytest.raises(ValueError, match='no local conditioning'):
        _cpu_gen(lc=False, ring_steps=64).extend([0], [m])
    with pytest.raises(ValueError, match='ring plan'):
        next(_cpu_gen().vocode_iter([m]))
    with pytest.raises(ValueError, match='chunk'):
        next(_cpu_gen(ring_steps=8).vocode_iter([m]))          # chunk_sz 10 > ring_steps 8
    with pytest.raises(ValueError, match='exceeds ring_steps'):
        g.run(100, mel=np.zeros((20, 12), np.float32))


def test_generate_cli_mel_list_ring_flag(tmp_path, capsys):
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import generate
    from lbwn.ckpt import ckpt_file
    a = generate.get_args(['--mel-list', 'l.txt', '--mel-list-ring', '4096', 'arch.json', 'ckpt', 'out'])
    assert a.mel_list_ring == 4096
    assert generate.get_args(['--mel-list', 'l.txt', 'arch.json', 'ckpt', 'out']).mel_list_ring == 0
    open(ckpt_file(str(tmp_path / 'ck')), 'wb').close()
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(dict(SMALL_LC, wav_input_type='mu_law_quant')))
    np.save(tmp_path / 'm.npy', np.zeros((4, 12), np.float32))
    lst = tmp_path / 'list.txt'
    lst.write_text('0\t%s\tfirst\n' % (tmp_path / 'm.npy'))
    for ring in ('-1', '5'):                                  # negative, or below --chunk-size
        with pytest.raises(SystemExit) as e:
            generate.main(['--mel-list', str(lst), '--mel-list-ring', ring, '--chunk-size', '10', str(af),
                           str(tmp_path / 'ck'), str(tmp_path / 'out')])
        assert e.value.code == 1 and '--mel-list-ring' in capsys.readouterr().err
