"""lbwn_adam_ex on the GPU through the raw C ABI, and end to end through lbwn.optim.AdamOptimizer:
global-norm clipping, the non-finite skip, the weight EMA and the learning-rate schedule
(include/lbwn.h) against float64 numpy written here.

The inputs are test_adam_kernel_ragged's (tests/test_gpu_parity.py): seeded p, g, m normal, v uniform,
stats[1] = 7, counters = [4, 0, 4, 0] (so t = 5), l2 = 1e-3, at (n, n_weights) = (1, 0), (7, 3), (1003, 501),
(4096, 4096) and (2_100_003, 1_000_001).  At the last one the norm pass has 512 blocks of 256 threads over
525000 vectors: every block walks 4 full grid-stride turns (asserted from lbwn_adam_ex_ws_floats), and
the weight boundary 1_000_001 falls inside a vector.

Bounds.  Norm: relative 1e-6 against float64 on the same f32 g (each g carries at most 2 roundings, so
Σ g² about 2.4e-7 and its root 1.2e-7; 4x margin; an f32-accumulated sum over 2.1 M terms does not meet
it).  p, m, v and the shadow: test_adam_kernel_ragged's rtol 1e-6, atol 1e-7 (the scale adds under 3e-7
relative to g, which enters m as at most 0.1·|g|·3e-7, inside atol).  Bitwise where the arithmetic is
the same: the neutral call against lbwn_adam_tf1, skipped steps, two runs of one call, graph replay.

The non-finite cases: the partial sums are doubles (squares formed in double), so two finite gradients
of 1e25, whose squares overflow f32 but not double, do NOT skip: the norm is finite (about 2e24) and the
step is applied; +Inf and NaN skip."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.optim import AdamOptimizer
from oracle import wavenet_ref as R
from tests.test_gpu_parity import make_net, oracle_params, rand_batch, small_arch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LR, B1, B2, EPS, L2 = 1e-3, 0.9, 0.999, 1e-8, 1e-3
SHAPES = [(1, 0), (7, 3), (1003, 501), (4096, 4096), (2_100_003, 1_000_001)]
BIG = SHAPES[-1]


@functools.lru_cache(maxsize=None)
def inputs(n, seed=None):
    """(p0, g0, m0, v0) float32, read-only: test_adam_kernel_ragged's draw (seed n)."""
    rng = np.random.default_rng(n if seed is None else seed)
    p0, g0, m0 = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v0 = rng.random(n).astype(np.float32)
    for a in (p0, g0, m0, v0):
        a.setflags(write=False)
    return p0, g0, m0, v0


class State:
    """Device copies of one set of inputs plus every buffer lbwn_adam_ex takes."""

    def __init__(self, lib, n, nw, g0=None, status=None, t_prev=4):
        self.lib, self.n, self.nw = lib, n, nw
        p0, g_in, m0, v0 = inputs(n)
        self.p, self.g, self.m, self.v = (torch.tensor(a, device=DEV) for a in (p0, g_in if g0 is None else g0, m0, v0))
        self.stats = torch.tensor([0.0, 7.0, 0.0, 0.0], device=DEV)
        self.counters = torch.tensor([4, 0, t_prev, 0], dtype=torch.int64, device=DEV)
        self.ema = self.p.clone()
        self.ws = torch.zeros(max(4, int(lib.lbwn_adam_ex_ws_floats(n))), device=DEV)
        self.info = torch.full((4,), -1.0, device=DEV)
        self.skips = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.status = None if status is None else torch.tensor([status], dtype=torch.int32, device=DEV)

    def ex(self, info=True, ema=False, **kw):
        kw.setdefault('lr_decay_rate', 1.0)
        a = _lib.AdamExArgs(params=self.p.data_ptr(), grads=self.g.data_ptr(), m=self.m.data_ptr(),
                            v=self.v.data_ptr(), n_weights=self.nw, n_total=self.n, lr=LR, beta1=B1, beta2=B2, eps=EPS,
                            l2_factor=L2, stats=self.stats.data_ptr(), counters=self.counters.data_ptr(),
                            step_status=_lib.ptr(self.status), ws=self.ws.data_ptr(),
                            info=self.info.data_ptr() if info else None, nonfinite_skips=self.skips.data_ptr(),
                            ema=self.ema.data_ptr() if ema else None, **kw)
        _lib.check(self.lib.lbwn_adam_ex(ctypes.byref(a), torch.cuda.current_stream().cuda_stream))

    def tf1(self):
        _lib.check(self.lib.lbwn_adam_tf1(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                          self.nw, self.n, LR, B1, B2, EPS, L2, self.stats.data_ptr(),
                                          self.counters.data_ptr(), _lib.ptr(self.status), None))

    def snap(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).clone() for k in ('p', 'm', 'v', 'ema', 'counters', 'info', 'skips')}


def same_bits(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def g_f32(p0, g0, nw):
    """g as the kernel forms it: f32 raw·inv, then + l2·θ in f32."""
    inv = np.float32(1.0) / np.float32(7.0)
    g = (g0 * inv).astype(np.float32)
    g[:nw] = g[:nw] + np.float32(L2) * p0[:nw]
    return g


def norm64(p0, g0, nw):
    g = g_f32(p0, g0, nw).astype(np.float64)
    return float(np.sqrt(np.sum(g * g)))


def f32(x):
    """The value a float argument of the C ABI carries."""
    return float(np.float32(x))


def adam64(p, g_raw, m, v, nw, t, scale=1.0, lr=None):
    """One float64 TF1 Adam step on g·scale (test_adam_kernel_ragged's reference); returns p, m, v.
    The hyperparameters enter at the float32 values the ABI carries, like every other input: with the
    Python doubles, 1 - 0.999 differs from the kernel's exact 1 - fl(0.999) by 1.3e-5 relative, which
    reaches p where (1-β2)·g² dominates v (measured at n = 2_100_003 with the doubles: 6 elements of
    lbwn_adam_tf1 itself, 7 of the clipped call, miss rtol 1e-6 / atol 1e-7 by up to 3.3e-7, each at
    6e-6 of its step; m and v miss nowhere)."""
    b1, b2, eps, l2 = f32(B1), f32(B2), f32(EPS), f32(L2)
    gd = np.asarray(g_raw, np.float64) / 7.0
    gd[:nw] += l2 * p[:nw]
    gd *= scale
    md = b1 * m + (1 - b1) * gd
    vd = b2 * v + (1 - b2) * gd * gd
    lr_t = (f32(LR) if lr is None else lr) * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return p - lr_t * md / (np.sqrt(vd) + eps), md, vd


def close(got, want, name):
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=1e-7, err_msg=name)


def test_big_shape_takes_more_than_two_turns(lib):
    n = BIG[0]
    nparts = (int(lib.lbwn_adam_ex_ws_floats(n)) - 4) // 2
    assert nparts == 512
    assert (n // 4) // (nparts * 256) > 2          # full grid-stride turns of every block of the norm pass
    assert BIG[1] % 4 != 0                          # the weight boundary inside a vector


@pytest.mark.parametrize('n,nw', SHAPES)
def test_neutral_is_bitwise_adam_tf1_and_norm_is_accurate(lib, n, nw):
    """clip_norm = 1e30 (scale exactly 1) with info: p, m, v and the counters bitwise lbwn_adam_tf1's;
    info[0] within 1e-6 relative of the float64 norm."""
    a, b = State(lib, n, nw), State(lib, n, nw)
    a.ex(clip_norm=1e30)
    b.tf1()
    sa, sb = a.snap(), b.snap()
    same_bits(sa, sb, ('p', 'm', 'v', 'counters'))
    assert sa['counters'].tolist() == [5, 7, 5, 0] and int(sa['skips']) == 0
    p0, g0, _, _ = inputs(n)
    want = norm64(p0, g0, nw)
    info = sa['info'].tolist()
    print('n %d: norm %.9g ref %.9g rel %.3g' % (n, info[0], want, abs(info[0] - want) / want))
    assert abs(info[0] - want) <= 1e-6 * want
    assert info[1] == 1.0 and info[2] == 0.0 and abs(info[3] - LR) <= 1e-6 * LR


@pytest.mark.parametrize('n,nw', SHAPES)
def test_clipping_matches_float64(lib, n, nw):
    p0, g0, m0, v0 = inputs(n)
    nrm = norm64(p0, g0, nw)
    clip = float(np.float32(0.5 * nrm))
    scale = clip / max(nrm, clip)
    assert scale < 1.0
    s = State(lib, n, nw)
    s.ex(clip_norm=clip)
    out = s.snap()
    pd, md, vd = adam64(p0.astype(np.float64), g0, m0.astype(np.float64), v0.astype(np.float64), nw, 5, scale)
    close(out['m'], md, 'm')
    close(out['v'], vd, 'v')
    close(out['p'], pd, 'p')
    info = out['info'].tolist()
    assert abs(info[1] - scale) <= 1e-6 * scale and info[2] == 0.0
    assert abs(info[0] - nrm) <= 1e-6 * nrm


def _poisoned(n, kind):
    g = inputs(n)[1].copy()
    if kind == 'inf':
        g[n // 2] = np.inf
    elif kind == 'nan':
        g[n // 3] = np.nan
    else:                                   # squares overflow f32 (1e50 / 49), not double
        g[n // 2] = 1e25
        g[n // 3] = -1e25
    return g


@pytest.mark.parametrize('kind', ['inf', 'nan', 'f32_overflow'])
@pytest.mark.parametrize('how', ['skip_nonfinite', 'clip_norm'])
def test_nonfinite_skip(lib, kind, how):
    n, nw = 1003, 501
    g = _poisoned(n, kind)
    s = State(lib, n, nw, g0=g)
    s.ema.mul_(1.5)                         # a shadow that an update would move
    before = s.snap()
    kw = dict(skip_nonfinite=1) if how == 'skip_nonfinite' else dict(clip_norm=1e30)
    s.ex(ema=True, ema_decay=0.999, ema_num_updates=1, **kw)
    after = s.snap()
    if kind == 'f32_overflow':              # double partials: a finite norm, so the step is applied
        want = norm64(inputs(n)[0], g, nw)
        assert np.isfinite(want) and abs(after['info'][0].item() - want) <= 1e-6 * want
        assert after['info'][2].item() == 0.0 and int(after['skips']) == 0
        assert after['counters'].tolist() == [5, 7, 5, 0]
        assert not torch.equal(after['p'], before['p'])
        return
    same_bits(after, before, ('p', 'm', 'v', 'ema', 'counters'))
    assert int(after['skips']) == 1 and after['info'][2].item() == 1.0
    assert not np.isfinite(after['info'][0].item())
    s.ex(ema=True, ema_decay=0.999, ema_num_updates=1, **kw)      # the count is cumulative
    assert int(s.snap()['skips']) == 2


def test_inf_without_guard_updates_as_adam_tf1(lib):
    n, nw = 1003, 501
    g = _poisoned(n, 'inf')
    a, b = State(lib, n, nw, g0=g), State(lib, n, nw, g0=g)
    a.ex(info=False, skip_nonfinite=0, clip_norm=0.0, lr_warmup_steps=1)   # a schedule of factor 1: the ex kernel
    b.tf1()
    sa, sb = a.snap(), b.snap()
    same_bits(sa, sb, ('p', 'm', 'v', 'counters'))
    assert int(sa['skips']) == 0
    c = State(lib, n, nw, g0=g)
    c.ex(info=True)                          # the norm is reported, nothing acts on it
    sc = c.snap()
    same_bits(sc, sb, ('p', 'm', 'v', 'counters'))
    assert np.isinf(sc['info'][0].item()) and sc['info'][1].item() == 1.0 and sc['info'][2].item() == 0.0


def test_status_skip(lib):
    n, nw = 1003, 501
    s = State(lib, n, nw, status=2)
    before = s.snap()
    s.ex(ema=True, ema_decay=0.999, clip_norm=1.0)
    after = s.snap()
    same_bits(after, before, ('p', 'm', 'v', 'ema'))
    assert after['counters'].tolist() == [4, 0, 4, 2]
    assert int(after['skips']) == 0
    assert after['info'][:3].tolist() == [0.0, 0.0, 0.0] and abs(after['info'][3].item() - LR) <= 1e-6 * LR


@pytest.mark.parametrize('num_updates', [1, 0])
@pytest.mark.parametrize('n,nw', [(7, 3), (1003, 501)])
def test_ema_three_steps(lib, n, nw, num_updates):
    p0, _, m0, v0 = inputs(n)
    s = State(lib, n, nw)
    p, m, v = (a.astype(np.float64) for a in (p0, m0, v0))
    sh = p.copy()
    for k in range(3):
        g = inputs(n, seed=1000 + 7 * n + k)[1]
        s.g.copy_(torch.tensor(g))
        s.ex(ema=True, ema_decay=0.999, ema_num_updates=num_updates)
        t = 5 + k
        p, m, v = adam64(p, g, m, v, nw, t)
        d = min(0.999, (1.0 + t) / (10.0 + t)) if num_updates else 0.999
        sh = sh - (1.0 - d) * (sh - p)
    out = s.snap()
    assert out['counters'].tolist() == [7, 21, 7, 0]
    close(out['ema'], sh, 'ema')
    close(out['p'], p, 'p')


def test_ema_unchanged_by_a_skipped_middle_step(lib):
    n, nw = 1003, 501
    s = State(lib, n, nw)
    s.ex(ema=True, ema_decay=0.999, skip_nonfinite=1)
    one = s.snap()
    assert not torch.equal(one['ema'], one['p']) and one['counters'].tolist() == [5, 7, 5, 0]
    s.g.copy_(torch.tensor(_poisoned(n, 'nan')))
    s.ex(ema=True, ema_decay=0.999, skip_nonfinite=1)
    two = s.snap()
    same_bits(two, one, ('p', 'm', 'v', 'ema', 'counters'))
    assert int(two['skips']) == 1
    s.g.copy_(torch.tensor(inputs(n)[1]))
    s.ex(ema=True, ema_decay=0.999, skip_nonfinite=1)
    three = s.snap()
    assert three['counters'].tolist() == [6, 14, 6, 0] and not torch.equal(three['ema'], one['ema'])


@pytest.mark.parametrize('kw,factor', [
    (dict(lr_warmup_steps=10), 0.5),
    (dict(lr_decay_steps=4, lr_decay_rate=0.5), 0.5 ** 1.25),
    (dict(lr_decay_steps=4, lr_decay_rate=0.5, lr_decay_staircase=1), 0.5),
    (dict(lr_warmup_steps=10, lr_decay_steps=4, lr_decay_rate=0.5), 0.5 * 0.5 ** 1.25),
])
def test_lr_schedule(lib, kw, factor):
    n, nw = 1003, 501
    p0, g0, m0, v0 = inputs(n)
    s = State(lib, n, nw)
    s.ex(**kw)
    out = s.snap()
    lr_eff = f32(LR) * factor
    assert abs(out['info'][3].item() - lr_eff) <= 1e-6 * lr_eff
    pd, md, vd = adam64(p0.astype(np.float64), g0, m0.astype(np.float64), v0.astype(np.float64), nw, 5, lr=lr_eff)
    close(out['p'], pd, 'p')
    close(out['m'], md, 'm')


def test_deterministic_bits_at_2m(lib):
    n, nw = BIG
    p0, g0, _, _ = inputs(n)
    clip = float(np.float32(0.5 * norm64(p0, g0, nw)))
    runs = []
    for k in range(3):
        s = State(lib, n, nw)
        torch.cuda.synchronize()
        if k == 2:      # right behind an unrelated kernel that holds part of the device
            side = torch.cuda.Stream()
            big = torch.empty(1 << 28, device=DEV)      # 1 GiB fill
            with torch.cuda.stream(side):
                big.fill_(1.0)
        s.ex(clip_norm=clip)
        runs.append(s.snap())
    for r in runs[1:]:
        same_bits(r, runs[0], ('p', 'm', 'v', 'info', 'counters'))


def test_graph_capture_replays_bitwise(lib):
    n, nw = 1003, 501
    p0, g0, _, _ = inputs(n)
    clip = float(np.float32(0.5 * norm64(p0, g0, nw)))
    kw = dict(ema=True, ema_decay=0.999, ema_num_updates=1, clip_norm=clip, lr_warmup_steps=10)
    eager, cap = State(lib, n, nw), State(lib, n, nw)
    for _ in range(3):
        eager.ex(**kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.ex(**kw)
    for _ in range(3):
        graph.replay()
    a, b = eager.snap(), cap.snap()
    assert a['counters'].tolist() == [7, 21, 7, 0]
    same_bits(b, a, ('p', 'm', 'v', 'ema', 'counters', 'info', 'skips'))
    assert abs(a['info'][3].item() - LR * 0.7) <= 1e-6 * LR        # t = 7 of the last replay: the schedule moved


def test_end_to_end_clip_and_ema_match_oracle():
    """check_adam_step's setup (tests/test_gpu_parity.py) with clip_norm = half the oracle's step-0 norm and
    ema_decay 0.99: parameters and shadow to check_adam_step's bounds, each step's norm to 2e-4 relative."""
    arch = small_arch(nb=1, nbl=3)
    B, T, lr = 2, 128, 1e-3
    net = make_net(arch, B, l2=1e-3)
    q, ids = rand_batch(arch, B, T)
    P, S = oracle_params(net)
    shadow = {k: v.copy() for k, v in P.items()}
    opt_o = R.AdamTF1(lr)
    opt = None
    norms, c = [], None
    for step in range(3):
        lg, cache, S = R.forward(arch, P, q, ids, S)
        st, dlog = R.loss_fcn(arch, P, lg, q, ids, 1e-3)
        G = R.backward(arch, P, cache, dlog, 1e-3)
        nrm = float(np.sqrt(sum(float(np.sum(np.square(G[k]))) for k in P)))
        if c is None:
            c = 0.5 * nrm
            opt = AdamOptimizer(lr, clip_norm=c, ema_decay=0.99)
        scale = c / max(nrm, c)
        assert scale < 1.0, (step, nrm, c)
        opt_o.step(P, {k: G[k] * scale for k in P})
        t = step + 1
        d = min(0.99, (1.0 + t) / (10.0 + t))
        for k in P:
            shadow[k] = shadow[k] - (1.0 - d) * (shadow[k] - P[k])
        gv, loss = net.build(q, None, ids)
        opt.apply_gradients(gv)
        norms.append((opt.grad_info(net).clone(), nrm, scale))
    torch.cuda.synchronize()
    for info, nrm, scale in norms:
        info = info.tolist()
        print('norm %.7g oracle %.7g scale %.6g' % (info[0], nrm, info[1]))
        assert abs(info[0] - nrm) <= 2e-4 * nrm
        assert info[2] == 0.0
    assert opt.nonfinite_skips(net) == 0
    ema = opt.ema_tensors(net)
    for name in net.layout.names():
        for got, want, what in ((net.vars[name], P[name], 'param'), (ema[name], shadow[name], 'ema')):
            dlt = np.abs(got.cpu().double().numpy() - want)
            assert dlt.max() <= 2 * 3 * lr + 1e-6, (what, name)
            assert np.mean(dlt) <= 2e-6, (what, name, np.mean(dlt))
    assert net.counters[0].item() == 3 and net.counters[2].item() == 3
