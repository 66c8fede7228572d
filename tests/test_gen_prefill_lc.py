"""Prompt prefill on plans with local conditioning, host side (no GPU, no launch): the refusal is
now "no mel loaded", LC plans carve and report the "pfcond" scratch of B·T_s·G·2·n_dil floats, G
comes from LBWN_GEN_PREFILL_LC_GROUP (validated at plan creation, LC plans only), plans without LC
keep their workspace, and WaveNetGen validates before the library is called."""
import ctypes

import numpy as np
import pytest

from lbwn import _lib
from tests.test_gen_prefill import WS, c_arch, make_host_gen, make_plan

B, L, CD = 3, 8, 32          # make_plan's batch, the layers and n_dil of test_gen_prefill.SMALL


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    monkeypatch.delenv('LBWN_GEN_PREFILL_LC_GROUP', raising=False)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    lib = _lib.load()
    lib.lbwn_gen_workspace_bytes.restype = ctypes.c_size_t
    return lib


def tensor(lib, h, name):
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.lbwn_gen_tensor(h, name, ctypes.byref(off), ctypes.byref(nb))
    return rc, off.value, nb.value


def test_lc_plan_without_a_mel_refuses_prefill(lib):
    h = make_plan(lib, c_arch(lc=True))
    P = _lib.Params()
    assert lib.lbwn_gen_prefill(h, ctypes.byref(P), WS, ctypes.c_void_p(8192), 10, 10, None) == 22
    msg = lib.lbwn_last_error()
    assert b'prefill: local conditioning is not supported before lbwn_gen_set_mel (no mel loaded)' in msg, msg
    lib.lbwn_gen_plan_destroy(h)


def test_pfcond_follows_slice_and_group(lib, monkeypatch):
    """B·T_s·G·2Cd·4 bytes, at a 256-byte offset inside the workspace; default T_s = 10880 at B = 3
    and default G = 8."""
    for sl, grp, T, G in ((None, None, 10880, 8), ('5', None, 5, 8), ('300', '3', 300, 3), ('16', '1', 16, 1),
                          (None, str(L), 10880, L)):
        for name, v in (('LBWN_GEN_PREFILL_SLICE', sl), ('LBWN_GEN_PREFILL_LC_GROUP', grp)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        h = make_plan(lib, c_arch(lc=True))
        rc, off, nb = tensor(lib, h, b'pfcond')
        assert rc == 0, lib.lbwn_last_error()
        assert nb == B * T * G * 2 * CD * 4, (sl, grp, nb)
        assert off % 256 == 0 and off + nb <= lib.lbwn_gen_workspace_bytes(h)
        lib.lbwn_gen_plan_destroy(h)


def test_pfcond_is_einval_without_lc(lib):
    h = make_plan(lib, c_arch())
    rc, _, _ = tensor(lib, h, b'pfcond')
    assert rc == 22 and b'pfcond' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)


def test_lc_group_env_values(lib, monkeypatch):
    """An integer in 1..L on LC plans, anything else EINVAL naming the variable; a plan without LC
    does not read it and keeps its workspace to the byte."""
    h = make_plan(lib, c_arch())
    plain = lib.lbwn_gen_workspace_bytes(h)
    lib.lbwn_gen_plan_destroy(h)
    for v in ('0', 'x', str(L + 1), '', '-2'):
        monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', v)
        make_plan(lib, c_arch(lc=True), expect=22)
        assert b'LBWN_GEN_PREFILL_LC_GROUP' in lib.lbwn_last_error()
        h = make_plan(lib, c_arch())
        assert lib.lbwn_gen_workspace_bytes(h) == plain
        lib.lbwn_gen_plan_destroy(h)
    for v in ('1', '4', str(L)):
        monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', v)
        h = make_plan(lib, c_arch())
        assert lib.lbwn_gen_workspace_bytes(h) == plain
        lib.lbwn_gen_plan_destroy(h)


def test_lc_workspace_is_the_plain_one_plus_the_lc_tensors(lib, monkeypatch):
    """"pfcond" is the only thing G changes: the LC plan's workspace grows by its bytes."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '128')
    size = {}
    for g in ('1', '5'):
        monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', g)
        h = make_plan(lib, c_arch(lc=True))
        size[g] = lib.lbwn_gen_workspace_bytes(h)
        lib.lbwn_gen_plan_destroy(h)
    assert size['5'] - size['1'] == 4 * B * 128 * 2 * CD * 4       # a multiple of 256: no rounding


def test_wavenetgen_lc_prefill_validates_before_the_library(monkeypatch):
    g = make_host_gen(lc=True)
    called = []
    monkeypatch.setattr(g, 'lib', type('NoLib', (), {'__getattr__': lambda s, n: called.append(n)})())
    assert g._mel is None
    codes = np.zeros((3, 5), np.int32)
    with pytest.raises(ValueError, match='local conditioning is not supported before a mel is loaded'):
        g.prefill(codes)
    g.teacher_mu = np.zeros(5, np.int32)
    with pytest.raises(ValueError, match='local conditioning is not supported before a mel is loaded'):
        g.init_buffers(prefill=True)         # no mel in the same call either
    g._mel = np.zeros((3, 2, 12), np.float32)
    with pytest.raises(RuntimeError, match='no plan'):
        g.prefill(codes)
    with pytest.raises(ValueError, match='prefill: codes must be integers'):
        g.prefill(codes.astype(np.float32))
    assert not called
