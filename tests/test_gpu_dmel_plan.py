"""dmel through the whole step: lbwn_train_forward, then lbwn_train_backward_ex with a dmel buffer
(csrc/engine.cpp lc_upsample_bwd: the fused kernel, or one more GEMM after the per-stage products), on
rows of LC_TABLE / TILE_TABLE of tests/test_gpu_cond_plan.py that take each side of each branch the new
output meets, and through lbwn.torch_ops.wavenet_loss under torch autograd.

Base: 1 block x 4 layers, C = 32, B = 2, T = 256 unless the row says otherwise.  Inputs: cond_batch with
stream 0 masked from position T - 2·hop - 5 on (tests/dmel_ref.py tail_mask), so that whole frames lie
after a stream's last scored position.

Per case: dmel / n_valid against tests/dmel_ref.py (float64, from the oracle's public pieces, after the
oracle has taken the GPU forward's sign for the few relu inputs within the forward bars of zero, as
every gradient test here does) within GRAD_REL = 2e-4 of its own max (grad_close, the project's bar for
every gradient); the frames wholly after a stream's last scored position exactly zero, the frame holding
it not; dmel allocated NaN-filled between NaN canaries: canaries intact, every element written;
lbwn_plan_info "dmel_fused" as in the table; every tensor of grad_flat (NaN-filled before each backward)
bitwise equal to a plain lbwn_train_backward on the same forward and inputs; a second run bitwise the same
dmel.

One exception to "bitwise", found when this file first ran: the GC table gradient of a tile that holds more
than one voice is summed with float atomicAdd (chain_bwd.hip, layer_common.h; cond_batch changes the voice
inside tiles), so GC_EMBED, GC_SIGNAL_* and GC_GATE_* differ in their last bits between two plain
lbwn_train_backward calls on the same forward, with or without this call in the library.  No bitwise
comparison of those three groups can pass; they are held to the float64 oracle at GRAD_REL instead, in
every run, and every other tensor (the LC ones among them) bitwise.  dmel does not depend on them.

Max err / own max of dmel measured on the MI355X, in units of 1e-6 (the bar is 200; printed per case with -s),
and the frames held to exact zero:

    row                          dmel_fused   dmel     zero frames
    8->24 [8,8,4] T=512              1        0.73     2 of 4      (stream 0 wholly masked: hop 256)
    4->4 [8]                         1        0.37     2 of 64
    12->16 [2,4] 2 blocks            1        0.59     2 of 64
    8->16 [2] B=3                    0        0.49     5 of 384
    24->16 [2,4]                     0        0.46     2 of 64
    8->16 [2,2,2,2,2]                0        0.37     2 of 16
    8->16 [8,8,8] T=512              0        0.48     1 of 2      (stream 0 wholly masked: hop 512)
    24->16 [2,4] T=2048              0        0.48     2 of 512
    20->68 [2,4]                     1        0.60     2 of 64
    12->16 [2,4] GC, chain           1        0.45     2 of 64
    12->16 [2,4] GC, LBWN_NO_CHAIN   1        0.50     2 of 64
    12->16 [2,4] GC, f32 MFMA        1        0.39     2 of 64
    wavenet_loss through Linear(20, 12): enc.weight.grad 0.37, enc.bias.grad 0.54, lc_input.grad 0.41

Every branch sits where float32 arithmetic sits, 300x inside the bar; none stands out.
"""
import ctypes

import numpy as np
import pytest
import torch

from lbwn import _lib
from tests.dmel_ref import check_zero_frames, dmel_ref, hop_of, tail_mask
from tests.gradcheck import GRAD_REL, adopt_relu_signs, adoption_capped, cond_arch, cond_batch, grad_close, oracle_run
from tests.test_gpu_cond_kernels import Out
from tests.test_gpu_cond_plan import LC_TABLE, TILE_TABLE

gpu = pytest.mark.gpu
DEV = 'cuda'

# row of LC_TABLE / TILE_TABLE (its name up to the colon) -> "dmel_fused" after the backward
ROWS = {
    '8->24 [8,8,4] T=512': 1,       # fused, hop 256, four frames
    '4->4 [8]': 1,                  # fused, one stage
    '12->16 [2,4] 2 blocks': 1,     # fused, dlc as two deferred partials
    '8->16 [2] B=3': 0,             # 384 frames, one stage: the dmel product reads the reduced dlc
    '24->16 [2,4]': 0,              # Li > Lo: dmel wider than the stack
    '8->16 [2,2,2,2,2]': 0,         # five stages
    '8->16 [8,8,8] T=512': 0,       # two frames in all: a product of M = 2 rows, below the bf16-split forms' four
    '24->16 [2,4] T=2048': 0,       # split-K stage gradient beside it
    '20->68 [2,4]': 1,              # in-chain LC
}
TABLE = {c['name'].split(':')[0]: c for c in LC_TABLE + TILE_TABLE}
assert set(ROWS) <= set(TABLE), set(ROWS) - set(TABLE)


def i32(t):
    return t.view(torch.int32)


class Step:
    """One net, one slice: every run starts from the same SAVE, so the forwards are the same bits."""

    def __init__(self, arch, B, T, seed=0, l2=1e-3, mel=None):
        from tests.test_gpu_parity import make_net, oracle_params
        self.arch, self.B, self.T, self.hop = arch, B, T, hop_of(arch)
        self.net = make_net(arch, B, seed=seed, l2=l2)
        self.q, self.ids, m = cond_batch(arch, B, T)
        self.mel = m if mel is None else mel
        self.ids = tail_mask(self.ids, self.hop)
        self.P, self.S = oracle_params(self.net)
        self.save0 = self.net.save_flat.clone()
        self.frames = T // self.hop

    def forward(self):
        net = self.net
        net.save_flat.copy_(self.save0)
        net.grad_flat.fill_(float('nan'))
        net.forward(self.q, self.mel, self.ids, backward=False)
        return net._plan(self.T), net._last

    def backward(self, dmel=None, ex=True):
        """Forward, then lbwn_train_backward_ex (dmel: an Out, or None) or lbwn_train_backward; returns
        the gradients' bits."""
        net, lib = self.net, self.net.lib
        h, (q, ids, mel) = self.forward()
        P, G, ws, sp = ctypes.byref(net._params_c), ctypes.byref(net._grads_c), net._ws.data_ptr(), _lib.stream_ptr()
        if ex:
            a = _lib.BackwardArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=mel.data_ptr(),
                                  dmel=dmel.ptr() if dmel is not None else None)
            _lib.check(lib.lbwn_train_backward_ex(h, P, G, ws, ctypes.byref(a), sp))
        else:
            _lib.check(lib.lbwn_train_backward(h, P, G, ws, q.data_ptr(), ids.data_ptr(), mel.data_ptr(), sp))
        torch.cuda.synchronize()
        assert int(net.plan_tensor(self.T, 'status').view(torch.int32)[0]) == 0, 'chain hand-off timed out'
        return i32(net.grad_flat).clone()

    def reference(self):
        """(dmel of the mean loss in float64, every parameter gradient, the loss statistics)"""
        cache, _, st, dlog = oracle_run(self.arch, self.P, self.S, self.q, self.ids, self.mel)
        self.forward()
        torch.cuda.synchronize()
        M = self.B * self.T
        s = self.net.plan_tensor(self.T, 's').view(M, -1).cpu().numpy()
        r2 = self.net.plan_tensor(self.T, 'r2').view(M, -1).cpu().numpy()
        adoption_capped(cache, adopt_relu_signs(cache, s, r2))
        ref, G = dmel_ref(self.arch, self.P, cache, dlog)
        return ref, G, st


def check_dmel_step(arch, B, T, name, fused, seed=0):
    stp = Step(arch, B, T, seed=seed)
    net, Li = stp.net, arch['n_lc_in']
    assert net.plan_info(T, 'dmel_fused') == -1
    ref, G, st = stp.reference()
    plain = stp.backward(ex=False)
    assert net.plan_info(T, 'dmel_fused') == -1
    null = stp.backward(dmel=None)
    assert net.plan_info(T, 'dmel_fused') == -1
    outs = [Out(B * stp.frames * Li) for _ in range(2)]
    with_dmel = [stp.backward(dmel=o) for o in outs]
    assert net.plan_info(T, 'dmel_fused') == fused, (name, net.plan_info(T, 'dmel_fused'))
    d = [o.read('dmel ' + name, (B, stp.frames, Li)) for o in outs]      # canaries; every element written
    assert int(net.stats[1]) == st['n_valid']
    ratio = grad_close(d[0].astype(np.float64) / st['n_valid'], ref, 'dmel ' + name)
    nz = check_zero_frames(d[0], stp.ids, stp.hop, name)
    print('dmel plan   %-34s max err / own max %.3g (bar %.3g)   frames held to exact zero: %d of %d'
          % (name, ratio, GRAD_REL, nz, B * stp.frames))
    assert np.array_equal(d[0].view(np.int32), d[1].view(np.int32)), name + ': two runs, two dmel'
    pv = net.layout.views(plain.view(torch.float32))
    if arch['n_gc_embed'] > 0:      # printed, not asserted: what two plain backwards on one forward disagree on
        p2 = net.layout.views(stp.backward(ex=False).view(torch.float32))
        print('dmel plan   %-34s two plain lbwn_train_backward calls differ in: %s'
              % (name, [n for n in net.layout.names() if not torch.equal(i32(p2[n]), i32(pv[n]))] or 'nothing'))
    for what, g in (('dmel NULL', null), ('dmel', with_dmel[0]), ('dmel, second run', with_dmel[1])):
        assert not torch.isnan(g.view(torch.float32)).any(), '%s (%s): part of a gradient not written' % (name, what)
        gv = net.layout.views(g.view(torch.float32))
        bad = [n for n in net.layout.names() if not n.startswith('GC_') and not torch.equal(i32(gv[n]), i32(pv[n]))]
        assert not bad, '%s (%s): gradients differ from lbwn_train_backward: %s' % (name, what, bad)
        # GC_EMBED / GC_SIGNAL / GC_GATE: see the docstring (float atomics, two plain runs differ too)
        for n in net.layout.names():
            if n.startswith('GC_'):
                grad_close(gv[n].cpu().double().numpy() / st['n_valid'], G[n], '%s (%s) %s' % (name, what, n))
    return stp


@gpu
@pytest.mark.parametrize('row', list(ROWS), ids=lambda r: r.replace(' ', '_'))
def test_dmel_branch(row, monkeypatch):
    for v in ('LBWN_CHAIN_TILE', 'LBWN_NO_CHAIN'):
        monkeypatch.delenv(v, raising=False)
    c = TABLE[row]
    check_dmel_step(c['arch'], c['B'], c['T'], row, ROWS[row], seed=c['seed'])


@gpu
@pytest.mark.parametrize('variant', ['chain', 'no_chain', 'f32_mfma'])
def test_dmel_with_gc(variant, monkeypatch, lib):
    """12->16 [2,4] with GC: the chain plan, the per-layer path (LBWN_NO_CHAIN=1: the third call site
    of lc_upsample_bwd) and the f32-MFMA GEMM mode."""
    monkeypatch.delenv('LBWN_CHAIN_TILE', raising=False)
    monkeypatch.setenv('LBWN_NO_CHAIN', '1' if variant == 'no_chain' else '0')
    mode = lib.lbwn_gemm_get_mode()
    try:
        if variant == 'f32_mfma':
            _lib.check(lib.lbwn_gemm_set_mode(0))
        check_dmel_step(cond_arch(1, 1), 2, 256, '12->16 [2,4] GC ' + variant, 1)
    finally:
        _lib.check(lib.lbwn_gemm_set_mode(mode))


@gpu
def test_wavenet_loss_autograd(monkeypatch):
    """enc = torch.nn.Linear(20, 12) feeds wavenet_loss on 12->16 [2,4]: after loss.backward() its
    gradients are the float64 chain rule through the reference dmel (within GRAD_REL of their own max),
    the loss is net.total_loss() at l2_factor = 0, and net.grad_flat is bitwise that of build()."""
    from lbwn.torch_ops import wavenet_loss
    for v in ('LBWN_CHAIN_TILE', 'LBWN_NO_CHAIN'):
        monkeypatch.delenv(v, raising=False)
    arch, B, T = cond_arch(0, 1), 2, 256
    torch.manual_seed(4)
    enc = torch.nn.Linear(20, 12).to(DEV)
    x = torch.randn(B, T // hop_of(arch), 20, device=DEV)
    with torch.no_grad():
        mel = enc(x).cpu().numpy()                # the f32 values the engine reads
    stp = Step(arch, B, T, l2=0.0, mel=mel)
    net = stp.net
    ref, _, st = stp.reference()
    net.save_flat.copy_(stp.save0)
    net.grad_flat.fill_(float('nan'))
    _, built_loss = net.build(stp.q, mel, stp.ids)
    built = i32(net.grad_flat).clone()
    built_loss = built_loss.clone()
    net.save_flat.copy_(stp.save0)
    net.grad_flat.fill_(float('nan'))
    lc = enc(x)
    lc.retain_grad()
    loss = wavenet_loss(net, stp.q, lc, stp.ids)
    assert loss.dim() == 0 and loss.requires_grad
    assert torch.equal(loss.detach(), net.total_loss()) and torch.equal(loss.detach(), built_loss)
    np.testing.assert_allclose(float(loss.detach()), st['mean_xent'], rtol=1e-5)
    assert torch.equal(i32(net.grad_flat), built), 'grad_flat differs from build() on the same inputs'
    assert net.plan_info(T, 'dmel_fused') == 1 and tuple(net.dmel.shape) == mel.shape
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    x64, W64 = x.cpu().double().numpy(), enc.weight.detach().cpu().double().numpy()
    np.testing.assert_allclose(mel, x64 @ W64.T + enc.bias.detach().cpu().double().numpy(), rtol=0, atol=1e-5)
    rw = grad_close(enc.weight.grad.cpu().double().numpy(), 2.0 * np.einsum('bto,bti->oi', ref, x64), 'enc.weight.grad')
    rb = grad_close(enc.bias.grad.cpu().double().numpy(), 2.0 * ref.sum(axis=(0, 1)), 'enc.bias.grad')
    rl = grad_close(lc.grad.cpu().double().numpy(), 2.0 * ref, 'lc_input.grad')
    print('wavenet_loss: max err / own max  enc.weight %.3g  enc.bias %.3g  lc_input %.3g (bar %.3g)'
          % (rw, rb, rl, GRAD_REL))
    check_zero_frames(lc.grad.cpu().numpy(), stp.ids, stp.hop, 'lc_input.grad')
