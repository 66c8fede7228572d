"""Parallel prompt prefill of the cached generator, host side (no GPU): lbwn_gen_prefill is part of
ABI 5, refuses bad calls before any launch (there is no device here), LBWN_GEN_PREFILL_SLICE is
validated at plan creation, and WaveNetGen.prefill validates its argument before the library is
called."""
import ctypes
import os
import re

import numpy as np
import pytest

from lbwn import _lib
from tests.conftest import ROOT

SMALL = dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
             n_gc_embed=0, n_gc_category=0, use_bias=True)
WS = ctypes.c_void_p(4096)      # a non-null workspace address: a refused call never touches it


def c_arch(arch=SMALL, lc=False):
    a = _lib.Arch()
    for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post', 'n_gc_embed',
              'n_gc_category'):
        setattr(a, k, int(arch[k]))
    a.use_bias = 1
    if lc:
        a.n_lc_in, a.n_lc_out, a.n_lc_upsample = 12, 16, 2
        a.lc_upsample[0], a.lc_upsample[1] = 2, 4
    return a


def make_plan(lib, a, B=3, max_steps=64, expect=0):
    h = ctypes.c_void_p()
    assert lib.lbwn_gen_plan_create(ctypes.byref(a), B, max_steps, 0, ctypes.byref(h)) == expect, \
        lib.lbwn_last_error()
    return h


def test_prefill_is_exported_and_declared_abi5():
    lib = _lib.load()
    assert hasattr(lib, 'lbwn_gen_prefill')
    assert 'lbwn_gen_prefill' in _lib.EXPORTED
    hdr = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    assert re.search(r'\bint lbwn_gen_prefill\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))
    assert re.search(r'#define LBWN_ABI_VERSION 5\b', hdr)
    assert lib.lbwn_abi_version() == 5 == _lib.ABI_VERSION


def test_prefill_refusals_before_any_launch(monkeypatch):
    """EINVAL (22) with its message and no device work: null pointers, n < 1, a row stride shorter
    than n, an arch with local conditioning, a slice too large for 32-bit indexing."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    lib = _lib.load()
    P = _lib.Params()
    codes = ctypes.c_void_p(8192)
    h = make_plan(lib, c_arch())
    n = 10

    def call(plan=h, params=ctypes.byref(P), ws=WS, c=codes, ld=n, nn=n):
        return lib.lbwn_gen_prefill(plan, params, ws, c, ld, nn, None)

    assert call(c=None) == 22 and b'prefill: null' in lib.lbwn_last_error()
    assert call(plan=None) == 22 and b'prefill: null' in lib.lbwn_last_error()
    assert call(params=None) == 22 and b'prefill: null' in lib.lbwn_last_error()
    assert call(ws=None) == 22 and b'prefill: null' in lib.lbwn_last_error()
    assert call(nn=0, ld=0) == 22 and b'n must be >= 1' in lib.lbwn_last_error()
    assert call(nn=-4, ld=0) == 22 and b'n must be >= 1' in lib.lbwn_last_error()
    assert call(ld=n - 1) == 22 and b'ld_codes' in lib.lbwn_last_error()
    assert call(ld=-1) == 22 and b'ld_codes' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    h = make_plan(lib, c_arch(lc=True))
    assert call(plan=h) == 22
    assert b'prefill: local conditioning is not supported' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    # B·T_s·Cr >= 2^31: 1100 streams x 65536 positions x 32 channels
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '65536')
    h = make_plan(lib, c_arch(), B=1100)
    assert call(plan=h) == 22 and b'2^31' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)


def test_prefill_slice_env_values(monkeypatch):
    """LBWN_GEN_PREFILL_SLICE: an integer in 1..65536 at plan creation; anything else is EINVAL
    naming the variable.  The prefill scratch follows the slice length, not max_steps."""
    lib = _lib.load()
    lib.lbwn_gen_workspace_bytes.restype = ctypes.c_size_t
    size = {}
    for v in ('5', '4096'):
        monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', v)
        h = make_plan(lib, c_arch())
        size[v] = lib.lbwn_gen_workspace_bytes(h)
        lib.lbwn_gen_plan_destroy(h)
    B, Cr, Cd = 3, 32, 32
    grow = (4096 - 5) * B * (2 * Cr + Cd) * 4       # two halo buffers and z, per position
    assert abs(size['4096'] - size['5'] - grow) <= 4 * 256, (size, grow)     # each carve rounds to 256 B
    for v in ('0', 'x', '70000', '', '-5', '12k'):
        monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', v)
        make_plan(lib, c_arch(), expect=22)
        assert b'LBWN_GEN_PREFILL_SLICE' in lib.lbwn_last_error()
    # the default: the largest multiple of 128 with B·T_s <= 32768 (B = 3: 10880), whatever max_steps is
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    h1, h2 = make_plan(lib, c_arch(), max_steps=64), make_plan(lib, c_arch(), max_steps=64 + 1000)
    s1, s2 = lib.lbwn_gen_workspace_bytes(h1), lib.lbwn_gen_workspace_bytes(h2)
    lib.lbwn_gen_plan_destroy(h1)
    lib.lbwn_gen_plan_destroy(h2)
    assert abs(s2 - s1 - 2 * 4 * B * 1000) <= 2 * 256              # only samples and wav grow with max_steps
    grow = (10880 - 5) * B * (2 * Cr + Cd) * 4
    assert abs(s1 - size['5'] - grow) <= 4 * 256, (s1, size, grow)


def make_host_gen(B=3, lc=False):
    from lbwn.imodel import WaveNetGen
    kw = dict(n_lc_in=12, n_lc_out=16, lc_upsample=[2, 4]) if lc else {}
    return WaveNetGen(2, 4, 256, 32, 32, 64, 32, 0, 0, True, B, 8, None, device='cpu', **kw)


def test_wavenetgen_prefill_validates_before_the_library(monkeypatch):
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
        with pytest.raises(ValueError, match='prefill'):
            g.prefill(bad)
    with pytest.raises(ValueError, match='local conditioning is not supported'):
        make_host_gen(lc=True).prefill(np.zeros((3, 5), np.int32))
    # a valid prompt passes validation and then needs a plan
    for ok in (np.zeros(5, np.int64), np.zeros((3, 5), np.int32), torch.zeros(3, 5, dtype=torch.int64), [1, 2, 3]):
        with pytest.raises(RuntimeError, match='no plan'):
            g.prefill(ok)
    assert not called


def test_generate_cli_has_teacher_prefill_flag():
    import generate
    assert generate.get_args(['a', 'b', 'c']).teacher_prefill is False
    assert generate.get_args(['--teacher-prefill', 'a', 'b', 'c']).teacher_prefill is True
