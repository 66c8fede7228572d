"""Cached generation with local conditioning, host side (no GPU): the generation plan accepts LC
archs and carves the upsampled mel and the cond ring, lbwn_gen_set_mel refuses bad calls before
any launch, and the Python / CLI layers validate the mel."""
import ctypes
import os
import sys

import numpy as np
import pytest

from lbwn import _lib
from lbwn.arch import load_arch
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

SMALL_LC = dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
                n_gc_embed=0, n_gc_category=0, n_lc_in=12, n_lc_out=16, lc_upsample=[2, 4], use_bias=True)


def c_arch(arch, lc=True):
    a = _lib.Arch()
    for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post', 'n_gc_embed',
              'n_gc_category'):
        setattr(a, k, int(arch[k]))
    a.use_bias = 1
    if lc:
        a.n_lc_in, a.n_lc_out = int(arch['n_lc_in']), int(arch['n_lc_out'])
        a.n_lc_upsample = len(arch['lc_upsample'])
        for i, s in enumerate(arch['lc_upsample']):
            a.lc_upsample[i] = int(s)
    return a


def make_plan(lib, a, B, max_steps, expect=0):
    h = ctypes.c_void_p()
    assert lib.lbwn_gen_plan_create(ctypes.byref(a), B, max_steps, 0, ctypes.byref(h)) == expect, \
        lib.lbwn_last_error()
    return h


def tensor(lib, h, name):
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    ret = lib.lbwn_gen_tensor(h, name.encode(), ctypes.byref(off), ctypes.byref(nb))
    return ret, off.value, nb.value


@pytest.mark.parametrize('which', ['arch5', 'small'])
def test_gen_plan_accepts_lc_and_carves(which, monkeypatch):
    lib = _lib.load()
    arch = load_arch(os.path.join(ROOT, 'par', 'arch5.json')) if which == 'arch5' else SMALL_LC
    B, max_steps = (10, 1000) if which == 'arch5' else (3, 65)
    L = arch['n_blocks'] * arch['n_block_layers']
    hop = int(np.prod(arch['lc_upsample']))
    rows = -(-max_steps // hop) * hop
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    h = make_plan(lib, c_arch(arch), B, max_steps)
    h0 = make_plan(lib, c_arch(arch, lc=False), B, max_steps)
    ws, ws0 = lib.lbwn_gen_workspace_bytes(h), lib.lbwn_gen_workspace_bytes(h0)
    ret, off, nb = tensor(lib, h, 'lc')
    assert ret == 0 and nb == 4 * B * rows * arch['n_lc_out'] and off % 256 == 0 and off + nb <= ws
    ret, off_c, nb_c = tensor(lib, h, 'lccond')
    assert ret == 0 and nb_c == 64 * L * B * 64 * 4 and off_c + nb_c <= ws      # default NC = 64 steps
    assert off_c >= off + nb or off >= off_c + nb_c
    assert ws >= ws0 + nb + nb_c
    assert tensor(lib, h0, 'lc')[0] == 22 and tensor(lib, h0, 'lccond')[0] == 22   # not on plans without LC
    lib.lbwn_gen_plan_destroy(h)
    lib.lbwn_gen_plan_destroy(h0)
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    h = make_plan(lib, c_arch(arch), B, max_steps)
    assert tensor(lib, h, 'lccond')[2] == 4 * L * B * 64 * 4
    lib.lbwn_gen_plan_destroy(h)


def test_gen_lc_chunk_env_values(monkeypatch):
    """LBWN_GEN_LC_CHUNK: an integer in 1..4096; anything else is refused at plan creation.  Plans
    without LC do not read it."""
    lib = _lib.load()
    for v in ('1', '64', '4096'):
        monkeypatch.setenv('LBWN_GEN_LC_CHUNK', v)
        lib.lbwn_gen_plan_destroy(make_plan(lib, c_arch(SMALL_LC), 2, 40))
    for v in ('0', '-3', '4097', '', '8x', 'auto'):
        monkeypatch.setenv('LBWN_GEN_LC_CHUNK', v)
        make_plan(lib, c_arch(SMALL_LC), 2, 40, expect=22)
        assert b'LBWN_GEN_LC_CHUNK' in lib.lbwn_last_error()
        lib.lbwn_gen_plan_destroy(make_plan(lib, c_arch(SMALL_LC, lc=False), 2, 40))


def test_gen_plan_refuses_bad_lc_arch():
    lib = _lib.load()
    bad = dict(SMALL_LC, n_lc_in=10)
    make_plan(lib, c_arch(bad), 2, 40, expect=22)
    assert b'multiples of 4' in lib.lbwn_last_error()
    bad = dict(SMALL_LC, n_lc_out=18)
    make_plan(lib, c_arch(bad), 2, 40, expect=22)
    a = c_arch(SMALL_LC)
    a.n_lc_upsample = 9
    make_plan(lib, a, 2, 40, expect=22)
    assert b'upsample stages' in lib.lbwn_last_error()
    a = c_arch(SMALL_LC)
    a.n_lc_upsample = 0
    make_plan(lib, a, 2, 40, expect=22)
    a = c_arch(SMALL_LC)
    a.lc_upsample[1] = 0
    make_plan(lib, a, 2, 40, expect=22)
    assert b'stride' in lib.lbwn_last_error()


def test_gen_set_mel_refusals_before_any_launch():
    """EINVAL with a message and no device work (there is no device here): a null mel, a plan
    without LC, more frames than the plan holds, no frames; and lbwn_gen_run on an LC plan that
    has no mel loaded."""
    lib = _lib.load()
    P = _lib.Params()
    for f, _ in _lib.Params._fields_:
        if f != 'lc_up':
            setattr(P, f, 0x1000)
    for i in range(8):
        P.lc_up[i] = 0x1000
    fake = 0x1000   # never dereferenced: every call below returns before a launch
    h = make_plan(lib, c_arch(SMALL_LC), 3, 65)                # hop 8: ceil(65 / 8) = 9 frames
    assert lib.lbwn_gen_set_mel(h, ctypes.byref(P), fake, None, 8, None) == 22
    assert b'mel is null' in lib.lbwn_last_error()
    assert lib.lbwn_gen_set_mel(h, ctypes.byref(P), fake, fake, 10, None) == 22
    assert b'exceed' in lib.lbwn_last_error()
    assert lib.lbwn_gen_set_mel(h, ctypes.byref(P), fake, fake, 2 ** 62, None) == 22
    assert lib.lbwn_gen_set_mel(h, ctypes.byref(P), fake, fake, 0, None) == 22
    assert b'n_frames' in lib.lbwn_last_error()
    assert lib.lbwn_gen_run(h, ctypes.byref(P), fake, 4, None) == 22
    assert b'mel' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h)
    h0 = make_plan(lib, c_arch(SMALL_LC, lc=False), 3, 65)
    assert lib.lbwn_gen_set_mel(h0, ctypes.byref(P), fake, fake, 8, None) == 22
    assert b'no local conditioning' in lib.lbwn_last_error()
    lib.lbwn_gen_plan_destroy(h0)


def test_generate_cli_parses_mel_npy():
    import generate
    a = generate.get_args(['--mel-npy', 'm.npy', '-g', '1', '-b', '2', 'arch.json', 'ckpt', 'out'])
    assert a.mel_npy == 'm.npy' and a.gen_seconds == 1 and a.batch_size == 2
    assert generate.get_args(['arch.json', 'ckpt', 'out']).mel_npy is None


def test_generate_cli_mel_errors(tmp_path, capsys):
    """LC arch: --mel-npy is required, and a mel too short for gen_seconds + teacher seconds is
    refused, both on stderr with exit(1) before any device work."""
    import json
    import generate
    from lbwn.ckpt import ckpt_file
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(dict(SMALL_LC, wav_input_type='mu_law_quant')))
    open(ckpt_file(str(tmp_path / 'ck')), 'wb').close()
    base = ['-g', '0.01', '-b', '2', str(af), str(tmp_path / 'ck'), str(tmp_path / 'out')]
    with pytest.raises(SystemExit) as e:
        generate.main(base)
    assert e.value.code == 1 and '--mel-npy is required' in capsys.readouterr().err
    np.save(tmp_path / 'm.npy', np.zeros((19, 12), np.float32))       # 160 steps need 20 frames of hop 8
    with pytest.raises(SystemExit) as e:
        generate.main(['--mel-npy', str(tmp_path / 'm.npy')] + base)
    assert e.value.code == 1 and 'too short' in capsys.readouterr().err


def _cpu_gen(B=3):
    from lbwn.imodel import WaveNetGen
    a = SMALL_LC
    return WaveNetGen(a['n_blocks'], a['n_block_layers'], a['n_quant'], a['n_res'], a['n_dil'], a['n_skip'],
                      a['n_post'], 0, 0, True, B, 10, None, device='cpu', n_lc_in=12, n_lc_out=16,
                      lc_upsample=[2, 4])


def test_wavenetgen_mel_value_errors():
    """run() validates the mel before it touches a device."""
    import torch
    g = _cpu_gen()
    assert g.arch['n_lc_out'] == 16 and g.hop == 8 and 'LC_UPSAMPLE_1' in g.vars and 'LC_GATE_1_3' in g.vars
    with pytest.raises(ValueError, match='mel'):
        g.run(65)
    with pytest.raises(ValueError, match='shape'):
        g.run(65, mel=np.zeros((3, 8, 11), np.float32))
    with pytest.raises(ValueError, match='shape'):
        g.run(65, mel=np.zeros((2, 8, 12), np.float32))
    with pytest.raises(ValueError, match='shape'):
        g.run(65, mel=torch.zeros(8, 12, 1, 1))
    with pytest.raises(ValueError, match='gen_sz 66'):
        g.run(66, mel=np.zeros((3, 8, 12), np.float32))            # 8 frames x hop 8 cover 65 steps
    with pytest.raises(ValueError, match='gen_sz 66'):
        g.run(66, mel=torch.zeros(8, 12))                          # [frames, n_lc_in], broadcast
    m = g._check_mel(np.ones((8, 12)), 65)
    assert m.shape == (3, 8, 12) and m.dtype == np.float32


def test_wavenetgen_no_lc_unchanged():
    """Without the LC keywords the constructor is the reference's, and a mel is refused."""
    from lbwn.imodel import WaveNetGen
    g = WaveNetGen(2, 4, 256, 32, 32, 64, 32, 0, 0, True, 2, 10, None, device='cpu')
    assert g.arch['n_lc_out'] == 0 and not any(n.startswith('LC_') for n in g.vars)
    with pytest.raises(ValueError, match='no local conditioning'):
        g.run(20, mel=np.zeros((2, 4, 12), np.float32))
