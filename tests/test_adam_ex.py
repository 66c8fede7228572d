"""Host side of the extended Adam step (lbwn_adam_ex), without a GPU: the struct and its
exports, every refusal (the checks precede any launch), AdamOptimizer's argument validation, the
checkpoint keys of the EMA shadows and the skip count, WaveNetGen.load_params(..., ema=True) and
train.py's flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.ckpt import load_tensors
from lbwn.optim import AdamOptimizer
from lbwn.tmodel import WaveNetTrain
from tests.conftest import ROOT
from tests.test_capi import header_functions
from tests.test_dropin import small_arch

EMA = '/ExponentialMovingAverage'
EINVAL = 22


# ---- struct and exports -------------------------------------------------------------------------

def test_struct_mirrors_header_and_library(lib):
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_adam_ex_args \{(.*?)\} lbwn_adam_ex_args;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [re.findall(r'\w+', piece)[-1] for decl in body.split(';') for piece in decl.split(',') if piece.strip()]
    assert fields == [n for n, _ in _lib.AdamExArgs._fields_], fields
    a = _lib.AdamExArgs()
    assert a.struct_size == ctypes.sizeof(_lib.AdamExArgs)
    a.struct_size += 8
    assert lib.lbwn_adam_ex(ctypes.byref(a), None) == EINVAL
    msg = lib.lbwn_last_error().decode()
    # the library names its own sizeof when it refuses another
    assert 'struct_size' in msg and '!= %d' % ctypes.sizeof(_lib.AdamExArgs) in msg, msg


def test_exports_and_workspace_size(lib):
    names = header_functions()
    assert 'lbwn_adam_ex' in names and 'lbwn_adam_ex_ws_floats' in names
    assert set(names) == set(_lib.EXPORTED)
    assert lib.lbwn_abi_version() == 5
    assert lib.lbwn_adam_ex_ws_floats(0) == 0 and lib.lbwn_adam_ex_ws_floats(-3) == 0
    sizes = [lib.lbwn_adam_ex_ws_floats(n) for n in (1, 2, 7, 1003, 4096, 100_000, 2_100_003, 50_000_000)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert sizes[-1] == sizes[-2]                   # capped: the partial count stops growing


# ---- refusals -------------------------------------------------------------------------------------

def good_args(**kw):
    """Arguments that pass every check (aligned fake pointers: nothing is launched in these tests)."""
    base = dict(params=0x1000, grads=0x2000, m=0x3000, v=0x4000, n_weights=4, n_total=8, lr=1e-3, beta1=0.9,
                beta2=0.999, eps=1e-8, l2_factor=0.0, stats=0x5000, counters=0x6000, lr_decay_rate=1.0, ws=0x7000,
                ema=0x8000, info=0x9000)
    base.update(kw)
    return _lib.AdamExArgs(**base)


@pytest.mark.parametrize('kw,word', [
    (dict(params=0), 'null argument'),
    (dict(grads=0), 'null argument'),
    (dict(m=0), 'null argument'),
    (dict(v=0), 'null argument'),
    (dict(counters=0), 'null argument'),
    (dict(n_weights=9), 'bad sizes'),
    (dict(n_weights=-1), 'bad sizes'),
    (dict(params=0x1004, clip_norm=1.0), '16-byte aligned'),
    (dict(m=0x3008, ema_decay=0.5), '16-byte aligned'),
    (dict(clip_norm=-1.0), 'clip_norm'),
    (dict(clip_norm=float('inf')), 'clip_norm'),
    (dict(clip_norm=float('nan')), 'clip_norm'),
    (dict(ema_decay=1.0), 'ema_decay'),
    (dict(ema_decay=-0.1), 'ema_decay'),
    (dict(ema_decay=float('nan')), 'ema_decay'),
    (dict(ema_decay=0.9, ema=0), 'ema must'),
    (dict(ema_decay=0.9, ema=0x8004), 'ema must'),
    (dict(clip_norm=1.0, ws=0, info=0), 'ws must'),
    (dict(skip_nonfinite=1, ws=0, info=0), 'ws must'),
    (dict(ws=0), 'ws must'),                                  # info alone asks for the norm
    (dict(clip_norm=1.0, ws=0x7008), 'ws must'),
    (dict(lr_warmup_steps=-1), 'lr_warmup_steps'),
    (dict(lr_decay_steps=-1), 'lr_decay_steps'),
    (dict(lr_decay_steps=4, lr_decay_rate=0.0), 'lr_decay_rate'),
    (dict(lr_decay_steps=4, lr_decay_rate=1.5), 'lr_decay_rate'),
    (dict(lr_decay_steps=4, lr_decay_rate=float('nan')), 'lr_decay_rate'),
])
def test_refusals_name_the_argument(lib, kw, word):
    a = good_args(**kw)
    assert lib.lbwn_adam_ex(ctypes.byref(a), None) == EINVAL
    msg = lib.lbwn_last_error().decode()
    assert msg.startswith('adam') and word in msg, msg


def test_null_struct_is_refused(lib):
    assert lib.lbwn_adam_ex(None, None) == EINVAL
    assert 'null argument struct' in lib.lbwn_last_error().decode()


# ---- AdamOptimizer ------------------------------------------------------------------------------

@pytest.mark.parametrize('kw,name', [
    (dict(clip_norm=-1.0), 'clip_norm'),
    (dict(clip_norm=float('inf')), 'clip_norm'),
    (dict(clip_norm=float('nan')), 'clip_norm'),
    (dict(ema_decay=1.0), 'ema_decay'),
    (dict(ema_decay=-0.5), 'ema_decay'),
    (dict(warmup_steps=-1), 'warmup_steps'),
    (dict(decay_steps=-2), 'decay_steps'),
    (dict(decay_steps=10, decay_rate=0.0), 'decay_rate'),
    (dict(decay_steps=10, decay_rate=1.01), 'decay_rate'),
])
def test_optimizer_rejects_bad_arguments(kw, name):
    with pytest.raises(ValueError, match=name):
        AdamOptimizer(1e-3, **kw)


def test_optimizer_picks_the_call():
    assert not AdamOptimizer().extended and not AdamOptimizer(clip_norm=None, ema_decay=None).extended
    for kw in (dict(clip_norm=1.0), dict(skip_nonfinite=True), dict(ema_decay=0.99), dict(warmup_steps=5),
               dict(decay_steps=5, decay_rate=0.5), dict(log_norm=True)):
        assert AdamOptimizer(**kw).extended, kw
    assert AdamOptimizer(clip_norm=1.0).norm_pass and AdamOptimizer(log_norm=True).norm_pass
    assert not AdamOptimizer(ema_decay=0.9).norm_pass
    with pytest.raises(ValueError, match='grad_info'):
        AdamOptimizer(ema_decay=0.9).grad_info(_net())
    with pytest.raises(ValueError, match='ema_decay'):
        AdamOptimizer(clip_norm=1.0).ema_tensors(_net())


def _net(tmp_path=None, step=0, seed=3):
    net = WaveNetTrain(**small_arch(), batch_sz=2, l2_factor=1e-3, device='cpu', seed=seed, resume_step=step,
                       ckpt_path=str(tmp_path / 'run.net') if tmp_path is not None else None)
    net.init_vars(seed, bias_scale=0.1)
    return net


def _default_keys(net):
    names = net.layout.names()
    return (set(names) | set(net.save_vars) | {'GLOBAL_STEP', 'VALID_SAMPLES', 'Adam/step'}
            | {n + sfx for n in names for sfx in ('/Adam', '/Adam_1')})


def test_checkpoint_keys_and_shadow_roundtrip(tmp_path):
    a = _net(tmp_path)
    names = a.layout.names()
    # defaults: exactly today's set
    assert set(load_tensors(a.save(1, AdamOptimizer()))) == _default_keys(a)
    opt = AdamOptimizer(ema_decay=0.99)
    ema = opt.ema_tensors(a)
    assert list(ema) == list(names) and all(torch.equal(ema[n], a.vars[n]) for n in names)   # a clone at creation
    opt.ex_slots(a)['ema'].uniform_(-1, 1)
    opt.ex_slots(a)['skips'].fill_(3)
    m, v = opt.slots(a)
    m.uniform_(-1, 1)
    v.uniform_(0, 1)
    a.counters[:3] = torch.tensor([17, 12345, 16])
    t = load_tensors(a.save(17, opt))
    assert set(t) == _default_keys(a) | {n + EMA for n in names} | {'Adam/nonfinite_skips'}
    b = _net(tmp_path, step=17, seed=9)
    opt2 = AdamOptimizer(ema_decay=0.99)
    b.restore(opt2)
    assert torch.equal(opt2.ex_slots(b)['ema'], opt.ex_slots(a)['ema'])        # bitwise
    assert not torch.equal(opt2.ex_slots(b)['ema'], b.flat)
    assert opt2.nonfinite_skips(b) == 3
    assert all(torch.equal(x, y) for x, y in zip(opt.slots(a), opt2.slots(b)))
    # a default optimizer reads the same file and ignores the shadows
    c = _net(tmp_path, step=17, seed=5)
    c.restore(AdamOptimizer())
    assert torch.equal(c.flat, a.flat)


def test_checkpoint_without_shadows_seeds_them_from_the_parameters(tmp_path):
    a = _net(tmp_path)
    a.save(4, AdamOptimizer())
    b = _net(tmp_path, step=4, seed=11)
    opt = AdamOptimizer(ema_decay=0.999, clip_norm=1.0)
    opt.ex_slots(b)['ema'].fill_(7.0)
    opt.ex_slots(b)['skips'].fill_(2)
    b.restore(opt)
    assert torch.equal(b.flat, a.flat)
    assert torch.equal(opt.ex_slots(b)['ema'], a.flat)
    assert opt.nonfinite_skips(b) == 0


# ---- WaveNetGen.load_params(..., ema=True) ------------------------------------------------------

def _gen():
    from lbwn.imodel import WaveNetGen
    a = small_arch()
    return WaveNetGen(a['n_blocks'], a['n_block_layers'], a['n_quant'], a['n_res'], a['n_dil'], a['n_skip'],
                      a['n_post'], a['n_gc_embed'], a['n_gc_category'], a['use_bias'], 2, 16, device='cpu')


def test_gen_load_params_takes_the_shadows(tmp_path):
    a = _net(tmp_path)
    opt = AdamOptimizer(ema_decay=0.99)
    opt.ex_slots(a)['ema'].uniform_(-1, 1)
    pfx = a.save(5, opt)
    g = _gen()
    g.restore(pfx, ema=True)
    assert torch.equal(g.flat, opt.ex_slots(a)['ema'])
    g.restore(pfx)
    assert torch.equal(g.flat, a.flat)
    t = dict(load_tensors(pfx))
    first = a.layout.names()[0]
    del t[a.layout.names()[2] + EMA]
    del t[first + EMA]
    with pytest.raises(ValueError, match=re.escape(first + EMA)):
        g.load_params(t, ema=True)
    with pytest.raises(ValueError, match='flat tensor'):
        g.load_params(a.flat, ema=True)


def test_generate_cli_ema_without_shadows_exits_1(tmp_path, capsys, monkeypatch):
    """generate.py --ema on a checkpoint without shadows: a message on stderr and exit 1, before any
    device work (the net is built on the CPU here, so the test needs no GPU)."""
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import json
    import generate
    import lbwn.imodel

    class CpuGen(lbwn.imodel.WaveNetGen):
        def __init__(self, *a, **kw):
            super().__init__(*a, device='cpu', **kw)

    monkeypatch.setattr(lbwn.imodel, 'WaveNetGen', CpuGen)
    a = _net(tmp_path)
    pfx = a.save(5, AdamOptimizer())
    arch = tmp_path / 'arch.json'
    arch.write_text(json.dumps(small_arch()))
    assert generate.get_args(['--ema', 'a', 'c', 'w']).ema and not generate.get_args(['a', 'c', 'w']).ema
    with pytest.raises(SystemExit) as e:
        generate.main(['--ema', '-b', '2', str(arch), pfx, str(tmp_path / 'wav')])
    assert e.value.code == 1
    assert 'ExponentialMovingAverage' in capsys.readouterr().err


# ---- train.py -----------------------------------------------------------------------------------

def test_train_flags_override_par():
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import train
    pos = ['p', 'a', 'b', 'c']
    args = train.get_args(['--clip-norm', '2.5', '--skip-nonfinite', '--ema-decay', '0.999', '--lr-warmup-steps', '100',
                           '--lr-decay-steps', '5000', '--lr-decay-rate', '0.5', '--log-grad-norm'] + pos)
    assert (args.clip_norm, args.skip_nonfinite, args.ema_decay, args.lr_warmup_steps, args.lr_decay_steps,
            args.lr_decay_rate, args.log_grad_norm) == (2.5, True, 0.999, 100, 5000, 0.5, True)
    par = dict(learning_rate=1e-3, batch_sz=8, slice_sz=4096, l2_factor=0.0, clip_norm=9.0, ema_decay=0.5,
               lr_warmup_steps=7, lr_decay_steps=8, lr_decay_rate=0.9, skip_nonfinite=False, log_grad_norm=False)
    train.override_par(args, par)
    assert [par[k] for k in train.OPT_KEYS] == [2.5, True, 0.999, 100, 5000, 0.5, True]
    assert par['batch_sz'] == 8 and par['learning_rate'] == 1e-3
    opt = AdamOptimizer(**train.optimizer_kwargs(par))
    assert (opt.clip_norm, opt.skip_nonfinite, opt.ema_decay, opt.warmup_steps, opt.decay_steps, opt.decay_rate,
            opt.log_norm) == (2.5, True, 0.999, 100, 5000, 0.5, True)
    # no flag given: the par keys stand, and a par file without them gives the plain optimizer
    none = train.get_args(pos)
    par2 = dict(learning_rate=2e-3, clip_norm=9.0)
    train.override_par(none, par2)
    assert par2 == dict(learning_rate=2e-3, clip_norm=9.0)
    assert AdamOptimizer(**train.optimizer_kwargs(par2)).clip_norm == 9.0
    plain = AdamOptimizer(**train.optimizer_kwargs(dict(learning_rate=2e-3)))
    assert not plain.extended and plain.lr == 2e-3
