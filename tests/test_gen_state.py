"""State save / load of the cached generator, host side (no GPU): the snapshot's size, the refusals
lbwn_gen_state_save / _load make before any launch (there is no device here), the documented layout's
numpy restatement (tests/state_ref.py), GenState's file format and the argument checks of
WaveNetGen.save_state / load_state / fork / prefill='fanout' and generate.py --prefill-fanout."""
import ctypes
import os
import re

import numpy as np
import pytest

from lbwn import _lib
from lbwn.arch import load_arch, normalize_arch
from tests import state_ref as S
from tests.conftest import ROOT
from tests.test_gen_prefill import SMALL, WS, c_arch, make_plan

STATE = ctypes.c_void_p(8192)    # a non-null, 16-byte aligned snapshot address: a refused call never touches it


def formula(arch, n):
    D = arch['n_blocks'] * (2 ** arch['n_block_layers'] - 1)
    return 256 + n * ((16 + 4 * D * arch['n_res'] + 15) // 16 * 16)


def test_state_entries_are_exported_and_abi_stays_5():
    lib = _lib.load()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lbwn.h')).read(), flags=re.S)
    for name, res in (('lbwn_gen_state_bytes', 'size_t'), ('lbwn_gen_state_save', 'int'), ('lbwn_gen_state_load', 'int')):
        assert hasattr(lib, name) and name in _lib.EXPORTED
        assert re.search(r'\b%s %s\s*\(' % (res, name), hdr), name
    assert lib.lbwn_abi_version() == 5 == _lib.ABI_VERSION


def test_state_bytes_against_the_formula():
    lib = _lib.load()
    arch3 = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    odd = dict(SMALL, n_res=3, n_dil=4, n_skip=8, n_post=6)       # 16 + 4·30·3 = 376 -> 384: the rounding
    for arch, B in ((SMALL, 3), (arch3, 10), (odd, 2)):
        h = make_plan(lib, c_arch(arch), B=B)
        for n in (1, B, 80):
            assert lib.lbwn_gen_state_bytes(h, n) == formula(arch, n) == S.state_bytes(normalize_arch(dict(arch)), n)
        assert lib.lbwn_gen_state_bytes(h, 0) == 0
        assert lib.lbwn_gen_state_bytes(h, -3) == 0
        lib.lbwn_gen_plan_destroy(h)
    assert lib.lbwn_gen_state_bytes(None, 4) == 0
    assert formula(SMALL, 1) == 256 + 16 + 4 * 30 * 32
    assert formula(odd, 1) == 256 + 384
    assert formula(arch3, 10) == 256 + 10 * (16 + 4 * 5115 * 32)     # ~6.5 MB of rings


def test_state_refusals_before_any_launch():
    """EINVAL (22) naming the argument, with no device work."""
    lib = _lib.load()
    B = 3
    h = make_plan(lib, c_arch(), B=B)
    src = ctypes.c_void_p(12288)

    def load(plan=h, ws=WS, state=STATE, n=B, m=None):
        return lib.lbwn_gen_state_load(plan, ws, state, n, m, None)

    def save(plan=h, ws=WS, state=STATE):
        return lib.lbwn_gen_state_save(plan, ws, state, None)

    err = lib.lbwn_last_error
    assert load(plan=None) == 22 and b'gen_state_load: plan is null' in err()
    assert load(ws=None) == 22 and b'gen_state_load: workspace is null' in err()
    assert load(state=None) == 22 and b'gen_state_load: state is null' in err()
    assert load(n=0, m=src) == 22 and b'state_streams must be >= 1' in err()
    assert load(n=-2, m=src) == 22 and b'state_streams must be >= 1' in err()
    assert load(n=B + 1) == 22 and b'src_stream is null' in err() and b'state_streams 4 != batch_sz 3' in err()
    assert load(n=B - 1) == 22 and b'src_stream is null' in err()
    assert load(state=ctypes.c_void_p(8192 + 8)) == 22 and b'state' in err() and b'16-byte aligned' in err()
    assert load(state=ctypes.c_void_p(8192 + 4), n=2, m=src) == 22 and b'16-byte aligned' in err()
    assert save(plan=None) == 22 and b'gen_state_save: plan is null' in err()
    assert save(ws=None) == 22 and b'gen_state_save: workspace is null' in err()
    assert save(state=None) == 22 and b'gen_state_save: state is null' in err()
    assert save(state=ctypes.c_void_p(8192 + 8)) == 22 and b'16-byte aligned' in err()
    lib.lbwn_gen_plan_destroy(h)


@pytest.mark.parametrize('n_res', [32, 3])
def test_pack_unpack_round_trip(n_res):
    arch = normalize_arch(dict(SMALL, n_res=n_res))
    B = 3
    rng = np.random.default_rng(5)
    rings = rng.standard_normal(B * 30 * n_res).astype(np.float32)
    codes = np.array([-1, 0, 255], np.int32)
    blob = S.pack(rings, codes, 21, arch, B)
    assert blob.dtype == np.uint8 and blob.size == formula(arch, B)
    r2, c2, step, B2 = S.unpack(blob, arch)
    assert (step, B2) == (21, B)
    np.testing.assert_array_equal(c2, codes)
    assert r2.tobytes() == rings.tobytes()
    # the layout, spelled out: stream 1's record starts with its code, then layer 0 (d = 1), layer 1 (d = 2) ...
    rb = S.record_bytes(arch)
    rec = blob[256 + rb:256 + 2 * rb]
    assert rec[:4].view('<i4')[0] == 0 and not rec[4:16].any()
    l0 = rings[:B * n_res].reshape(B, 1, n_res)
    l1 = rings[B * n_res:B * n_res + B * 2 * n_res].reshape(B, 2, n_res)
    got = rec[16:16 + 4 * 3 * n_res].view(np.float32)
    np.testing.assert_array_equal(got, np.concatenate([l0[1].ravel(), l1[1].ravel()]))
    assert not rec[16 + 4 * 30 * n_res:].any()
    # block 1's first layer (d = 1) follows block 0's 15 rows
    off = B * 15 * n_res
    np.testing.assert_array_equal(rec[16 + 4 * 15 * n_res:16 + 4 * 16 * n_res].view(np.float32),
                                  rings[off:off + B * n_res].reshape(B, n_res)[1])


def make_state(B=3, arch=SMALL, step=21, seed=6):
    import torch
    from lbwn.imodel import GenState
    a = normalize_arch(dict(arch))
    rng = np.random.default_rng(seed)
    D = sum(S.dilations(a))
    blob = S.pack(rng.standard_normal(B * D * a['n_res']).astype(np.float32),
                  rng.integers(0, a['n_quant'], B).astype(np.int32), step, a, B)
    return GenState(torch.from_numpy(blob), B, a['n_blocks'], a['n_block_layers'], a['n_res'], a['n_quant']), blob


def test_genstate_file_round_trip_and_header(tmp_path):
    import torch
    from lbwn.imodel import GenState, parse_state_header
    st, blob = make_state(step=(1 << 33) + 21)
    assert st.step() == (1 << 33) + 21
    assert st.header() == dict(n_streams=3, n_blocks=2, n_block_layers=4, n_res=32, n_quant=256,
                               record_bytes=16 + 4 * 30 * 32, step=(1 << 33) + 21)
    path = str(tmp_path / 'state.npy')
    st.save(path)
    raw = np.load(path, allow_pickle=False)
    assert raw.dtype == np.uint8 and raw.tobytes() == blob.tobytes()
    back = GenState.load(path, 'cpu')
    assert back.n_streams == 3 and back.dims == st.dims and back.step() == st.step()
    assert torch.equal(back.blob, st.blob)
    # refused: a wrong magic, another version, a truncated file, a size the header does not explain
    for edit, msg in ((lambda b: b[:4].view('<i4').__setitem__(0, 7), 'magic'),
                      (lambda b: b[4:8].view('<i4').__setitem__(0, 2), 'version'),
                      (lambda b: b[28:32].view('<i4').__setitem__(0, 64), 'inconsistent')):
        bad = blob.copy()
        edit(bad)
        with pytest.raises(ValueError, match=msg):
            parse_state_header(bad)
        np.save(path, bad)
        with pytest.raises(ValueError, match=msg):
            GenState.load(path, 'cpu')
    np.save(path, blob[:100])
    with pytest.raises(ValueError, match='header'):
        GenState.load(path, 'cpu')
    np.save(path, blob[:-16])
    with pytest.raises(ValueError, match='the header says'):
        GenState.load(path, 'cpu')
    np.save(path, blob.view(np.float32))
    with pytest.raises(ValueError, match='uint8'):
        GenState.load(path, 'cpu')
    with pytest.raises(ValueError, match='blob must be uint8'):
        GenState(torch.from_numpy(blob[:-16].copy()), 3, 2, 4, 32, 256)


def host_gen(B=3, plan=True, **kw):
    from lbwn.imodel import WaveNetGen
    g = WaveNetGen(2, 4, 256, 32, 32, 64, 32, 0, 0, True, B, 8, None, device='cpu', **kw)
    if plan:
        g.build_graph(64)
    return g


def no_lib(g, monkeypatch):
    called = []
    monkeypatch.setattr(g, 'lib', type('NoLib', (), {'__getattr__': lambda s, n: called.append(n)})())
    return called


def test_wavenetgen_state_methods_validate_before_the_library(monkeypatch):
    st, _ = make_state(B=3)
    g0 = host_gen(plan=False)
    called = no_lib(g0, monkeypatch)
    with pytest.raises(ValueError, match='save_state: no plan'):
        g0.save_state()
    with pytest.raises(ValueError, match='load_state: no plan'):
        g0.load_state(st)
    with pytest.raises(ValueError, match='fork: no plan'):
        g0.fork(0)
    assert not called
    g = host_gen()
    called = no_lib(g, monkeypatch)
    other, _ = make_state(B=3, arch=dict(SMALL, n_res=16))
    with pytest.raises(ValueError, match='another arch'):
        g.load_state(other)
    with pytest.raises(ValueError, match='another arch'):
        g.load_state(make_state(B=3, arch=dict(SMALL, n_quant=128))[0])
    with pytest.raises(ValueError, match='GenState'):
        g.load_state(st.blob)
    for m in ([0, 1], [0, 1, 2, 0], []):                           # a wrong map length
        with pytest.raises(ValueError, match=r'streams has %d entries, batch_sz is 3' % len(m)):
            g.load_state(st, m)
    for m in ([0, 1, 3], [-1, 0, 0], [0, 1.0, 2], [0, True, 2]):   # an entry out of range (or no integer)
        with pytest.raises(ValueError, match=r'streams\[\d\] = .* is not an integer in \[0, 3\)'):
            g.load_state(st, m)
    st2, _ = make_state(B=2)
    with pytest.raises(ValueError, match='identity'):             # None needs batch_sz records
        g.load_state(st2)
    with pytest.raises(ValueError, match=r'in \[0, 2\)'):
        g.load_state(st2, [0, 1, 2])
    for src in (3, -1, [0, 1], [0, 1, 5], None, 1.5):
        with pytest.raises(ValueError, match='fork'):
            g.fork(src)
    # a valid call passes every check and then needs init_buffers on the plan
    with pytest.raises(RuntimeError, match='init_buffers first'):
        g.load_state(st2, [0, 1, 1])
    with pytest.raises(RuntimeError, match='init_buffers first'):
        g.load_state(st, np.array([2, 1, 0]))
    assert not called


def test_fanout_prefill_argument_checks(monkeypatch):
    kw = dict(n_lc_in=12, n_lc_out=16, lc_upsample=[2, 4])
    import torch
    g = host_gen(**kw)
    g.teacher_mu = torch.zeros(20, dtype=torch.int32)
    called = no_lib(g, monkeypatch)
    mel3 = np.zeros((3, 8, 12), np.float32)
    with pytest.raises(ValueError, match="prefill='fanout' takes a shared mel"):
        g.init_buffers(mel=mel3, prefill='fanout')
    with pytest.raises(ValueError, match="prefill='fanout' takes a shared mel"):
        g.run(40, mel=mel3, prefill='fanout')
    for bad in ('fan', 'yes', 2):
        with pytest.raises(ValueError, match='prefill must be'):
            g.init_buffers(mel=mel3[0], prefill=bad)
    assert not called


def test_generate_cli_prefill_fanout_flag(capsys, tmp_path):
    import generate
    assert generate.get_args(['a', 'b', 'c']).prefill_fanout is False
    a = generate.get_args(['--prefill-fanout', '--teacher-wav', 't.wav', 'a', 'b', 'c'])
    assert a.prefill_fanout is True and a.teacher_prefill is False
    with pytest.raises(SystemExit) as e:
        generate.main(['--prefill-fanout', 'no_arch.json', 'no_ckpt', str(tmp_path / 'out')])
    assert e.value.code == 1
    assert '--prefill-fanout needs --teacher-wav' in capsys.readouterr().err
