"""Teacher-forced scoring of the cached generator, host side (no GPU): lbwn_gen_score and
lbwn_gen_score_scratch_bytes are added to ABI 5, refuse bad calls before any launch (there is no device
here), the scratch follows the prefill slice and not max_steps, the plan's workspace is what it was
before the two symbols existed, and WaveNetGen.score / generate.py --score-teacher validate their
arguments before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

from lbwn import _lib
from tests.conftest import ROOT
from tests.test_gen_prefill import SMALL, WS, c_arch, make_host_gen, make_plan

CODES = ctypes.c_void_p(8192)       # non-null addresses: a refused call never touches them
LOGP = ctypes.c_void_p(16384)
SCRATCH = ctypes.c_void_p(32768)
ARCH3 = dict(SMALL, n_blocks=5, n_block_layers=10, n_skip=512, n_post=512)


def test_score_symbols_are_exported_and_declared_abi5():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('lbwn_gen_score', 'int'), ('lbwn_gen_score_scratch_bytes', 'size_t')):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED
        assert re.search(r'\b%s %s\s*\(' % (ret, name), code)
    assert re.search(r'#define LBWN_ABI_VERSION 5\b', hdr)
    assert lib.lbwn_abi_version() == 5 == _lib.ABI_VERSION
    assert 'lbwn_gen_state_save / lbwn_gen_state_load' in hdr.split('lbwn_gen_score_scratch_bytes')[0].split(
        'Teacher-forced scoring')[1]      # the header says how to score without advancing


def test_score_refusals_before_any_launch(monkeypatch):
    """EINVAL (22) with its message and no device work: every refusal of lbwn_gen_prefill, then logp or
    scratch NULL, a scratch that is not 16-byte aligned, ld_logp < n."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    lib = _lib.load()
    P = _lib.Params()
    h = make_plan(lib, c_arch())
    n = 10

    def call(plan=h, params=ctypes.byref(P), ws=WS, c=CODES, ld=n, nn=n, logp=LOGP, ldl=n, scratch=SCRATCH):
        return lib.lbwn_gen_score(plan, params, ws, c, ld, nn, logp, ldl, scratch, None)

    for kw in (dict(c=None), dict(plan=None), dict(params=None), dict(ws=None)):
        assert call(**kw) == 22 and b'score: null' in lib.lbwn_last_error(), kw
    assert call(nn=0, ld=0, ldl=0) == 22 and b'score: n must be >= 1' in lib.lbwn_last_error()
    assert call(nn=-4, ld=0) == 22 and b'n must be >= 1' in lib.lbwn_last_error()
    assert call(ld=n - 1) == 22 and b'score: ld_codes' in lib.lbwn_last_error()
    assert call(ld=-1) == 22 and b'ld_codes' in lib.lbwn_last_error()
    assert call(logp=None) == 22 and b'score: logp is null' in lib.lbwn_last_error()
    assert call(scratch=None) == 22 and b'score: scratch is null' in lib.lbwn_last_error()
    assert call(scratch=ctypes.c_void_p(32768 + 8)) == 22 and b'not 16-byte aligned' in lib.lbwn_last_error()
    assert call(ldl=n - 1) == 22 and b'score: ld_logp' in lib.lbwn_last_error()
    assert call(ldl=0) == 22 and b'ld_logp' in lib.lbwn_last_error()
    # prefill's refusals come first: n < 1 speaks before the NULL logp
    assert call(nn=0, ld=0, logp=None) == 22 and b'n must be >= 1' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    h = make_plan(lib, c_arch(lc=True))
    assert call(plan=h) == 22
    assert b'score: local conditioning is not supported' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    # B·T_s·Cr >= 2^31: 1100 streams x 65536 positions x 32 channels
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '65536')
    h = make_plan(lib, c_arch(), B=1100)
    assert call(plan=h) == 22 and b'2^31' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    # the scratch's own rows: 130 streams x 65536 positions x 256 (L·n_dil) columns pass prefill's bound, not this one
    h = make_plan(lib, c_arch(), B=130)
    assert call(plan=h) == 22 and b'columns >= 2^31' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    # a width the GEMMs do not take
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE')
    h = make_plan(lib, c_arch(dict(SMALL, n_post=30)))
    assert call(plan=h) == 22 and b'multiples of 4' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)


def scratch_bytes(lib, B, T, arch):
    rows = B * T
    L = arch['n_blocks'] * arch['n_block_layers']
    return sum((4 * rows * c + 255) // 256 * 256
               for c in (L * arch['n_dil'], arch['n_skip'], arch['n_post'], arch['n_quant']))


def test_score_scratch_size(monkeypatch):
    """0 for NULL; Zcat | S | H | LG over B·T_s rows, each part rounded to 256 bytes: it grows with
    LBWN_GEN_PREFILL_SLICE and does not depend on max_steps."""
    lib = _lib.load()
    assert lib.lbwn_gen_score_scratch_bytes(None) == 0
    size = {}
    for v in ('5', '4096'):
        monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', v)
        h = make_plan(lib, c_arch())
        size[v] = lib.lbwn_gen_score_scratch_bytes(h)
        lib.lbwn_gen_plan_destroy(h)
        assert size[v] == scratch_bytes(lib, 3, int(v), SMALL)
    assert size['4096'] > size['5']
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE')
    h1, h2 = make_plan(lib, c_arch(), max_steps=64), make_plan(lib, c_arch(), max_steps=64 + 1000)
    s1, s2 = lib.lbwn_gen_score_scratch_bytes(h1), lib.lbwn_gen_score_scratch_bytes(h2)
    lib.lbwn_gen_plan_destroy(h1)
    lib.lbwn_gen_plan_destroy(h2)
    assert s1 == s2 == scratch_bytes(lib, 3, 10880, SMALL)       # the default slice of B = 3
    # arch3 at 10 voices, the default slice of 3200 positions: 32000 rows x (1600 + 512 + 512 + 256) floats
    h = make_plan(lib, c_arch(ARCH3), B=10, max_steps=48000)
    assert lib.lbwn_gen_score_scratch_bytes(h) == 32000 * 2880 * 4 == scratch_bytes(lib, 10, 3200, ARCH3)
    lib.lbwn_gen_plan_destroy(h)


def test_workspace_size_is_the_parents(monkeypatch):
    """lbwn_gen_workspace_bytes as recorded on the commit before lbwn_gen_score existed (no device:
    B <= 16 keeps the size independent of the execution form): the scratch is the caller's."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    monkeypatch.delenv('LBWN_GEN_PREFILL_LC_GROUP', raising=False)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    lib = _lib.load()
    for a, B, steps, want in ((c_arch(), 3, 64, 13128704),
                              (c_arch(lc=True), 3, 64, 80384000),
                              (c_arch(ARCH3), 10, 48000, 28204032)):
        h = make_plan(lib, a, B=B, max_steps=steps)
        assert lib.lbwn_gen_workspace_bytes(h) == want
        lib.lbwn_gen_plan_destroy(h)


def test_wavenetgen_score_validates_before_the_library(monkeypatch):
    import torch
    g = make_host_gen()
    called = []
    monkeypatch.setattr(g, 'lib', type('NoLib', (), {'__getattr__': lambda s, n: called.append(n)})())
    for bad in (np.zeros((2, 5), np.int32),            # batch mismatch
                np.zeros((3, 5, 1), np.int32),         # rank
                np.zeros((), np.int32),
                np.zeros((3, 0), np.int32),            # n < 1
                np.zeros(0, np.int64),
                np.zeros((3, 5), np.float32),          # dtype
                torch.zeros(5, dtype=torch.float32),
                torch.zeros(4, 5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            g.score(bad)
    with pytest.raises(ValueError, match='local conditioning is not supported'):
        make_host_gen(lc=True).score(np.zeros((3, 5), np.int32))
    for ok in (np.zeros(5, np.int64), np.zeros((3, 5), np.int32), torch.zeros(3, 5, dtype=torch.int64), [1, 2, 3]):
        with pytest.raises(RuntimeError, match='score: no plan'):
            g.score(ok)
    with pytest.raises(ValueError, match="'score'"):
        g._check_prefill('scores', None)
    g._check_prefill('score', None)
    assert not called


def test_generate_cli_score_teacher_flags(capsys):
    import generate
    a = generate.get_args(['a', 'b', 'c'])
    assert a.score_teacher is False and a.score_npy is None
    a = generate.get_args(['--score-teacher', '--score-npy', 'x.npy', '-w', 't.wav', 'a', 'b', 'c'])
    assert a.score_teacher is True and a.score_npy == 'x.npy'
    for argv, msg in ((['--score-teacher', 'a', 'b', 'c'], '--score-teacher needs --teacher-wav'),
                      (['--score-teacher', '--prefill-fanout', '-w', 't.wav', 'a', 'b', 'c'],
                       'cannot be combined with --prefill-fanout'),
                      (['--score-npy', 'x.npy', 'a', 'b', 'c'], '--score-npy needs --score-teacher')):
        with pytest.raises(SystemExit) as e:
            generate.main(argv)
        assert e.value.code == 1
        assert msg in capsys.readouterr().err
