"""The optimizer step's forms at arch3's parameter count: lbwn_adam_tf1, lbwn_adam_ex neutral,
with clipping, with clipping + EMA + schedule, interleaved in one process (device events around 10
back-to-back calls, 200 samples per form after 20 warm-up rounds; median [p10, p90]), then the whole C2
step (arch3, B = 8, T = 4096) through AdamOptimizer with and without clip_norm, blocks of 5 steps
alternating.  Prints the figures and writes them to --out (profiles/r13_adam_ex.md quotes them).  No test
asserts these times."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
from lbwn import _lib                      # noqa: E402
from lbwn.arch import ParamLayout, load_arch   # noqa: E402
from lbwn.optim import AdamOptimizer       # noqa: E402
from lbwn.tmodel import WaveNetTrain       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.devnull)
out = open(ap.parse_args().out, 'w')


def say(*a):
    s = ' '.join(str(x) for x in a)
    print(s, flush=True)
    out.write(s + '\n')
    out.flush()


lib = _lib.load()
arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
lay = ParamLayout(arch)
n, nw = lay.n_total, lay.n_weights
say('device', torch.cuda.get_device_name(0), 'n_total', n, 'n_weights', nw)
dev = 'cuda'
g = torch.Generator(device=dev).manual_seed(0)


class St:
    def __init__(self):
        self.p = torch.randn(n, device=dev, generator=g)
        self.g = torch.randn(n, device=dev, generator=g)
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.ema = self.p.clone()
        self.stats = torch.tensor([0.0, 32000.0, 0.0, 0.0], device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws = torch.zeros(int(lib.lbwn_adam_ex_ws_floats(n)), device=dev)
        self.info = torch.zeros(4, device=dev)
        self.skips = torch.zeros(1, dtype=torch.int64, device=dev)

    def args(self, **kw):
        kw.setdefault('lr_decay_rate', 1.0)
        return _lib.AdamExArgs(params=self.p.data_ptr(), grads=self.g.data_ptr(), m=self.m.data_ptr(),
                               v=self.v.data_ptr(), n_weights=nw, n_total=n, lr=1e-3, beta1=0.9, beta2=0.999,
                               eps=1e-8, l2_factor=1e-3, stats=self.stats.data_ptr(),
                               counters=self.counters.data_ptr(), nonfinite_skips=self.skips.data_ptr(), **kw)


sts = [St() for _ in range(4)]
stream = torch.cuda.current_stream().cuda_stream
a1 = sts[1].args()
a2 = sts[2].args(clip_norm=1.0, ws=sts[2].ws.data_ptr(), info=sts[2].info.data_ptr())
a3 = sts[3].args(clip_norm=1.0, ws=sts[3].ws.data_ptr(), info=sts[3].info.data_ptr(), ema=sts[3].ema.data_ptr(),
                 ema_decay=0.999, ema_num_updates=1, lr_warmup_steps=1000, lr_decay_steps=10000, lr_decay_rate=0.5)


def f0():
    s = sts[0]
    _lib.check(lib.lbwn_adam_tf1(s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), nw, n, 1e-3, 0.9,
                                 0.999, 1e-8, 1e-3, s.stats.data_ptr(), s.counters.data_ptr(), None, stream))


forms = [('adam_tf1', f0),
         ('adam_ex neutral', lambda: _lib.check(lib.lbwn_adam_ex(ctypes.byref(a1), stream))),
         ('adam_ex clip', lambda: _lib.check(lib.lbwn_adam_ex(ctypes.byref(a2), stream))),
         ('adam_ex clip+ema+schedule', lambda: _lib.check(lib.lbwn_adam_ex(ctypes.byref(a3), stream)))]
K, REPS, WARM = 10, 200, 20
times = [[] for _ in forms]
for r in range(WARM + REPS):
    for i, (_, f) in enumerate(forms):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(K):
            f()
        e1.record()
        e1.synchronize()
        if r >= WARM:
            times[i].append(e0.elapsed_time(e1) * 1000.0 / K)
say('per call (update + counters launches), us: median [p10, p90] over %d samples of %d back-to-back calls' % (REPS, K))
for (name, _), t in zip(forms, times):
    t = np.array(t)
    say('  %-28s %7.2f  [%6.2f, %6.2f]' % (name, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
say('skips', [int(s.skips) for s in sts], 'info clip', sts[2].info.tolist())

# ---- the whole C2 step (arch3, B = 8, T = 4096), with and without clip_norm ----
B, T = 8, 4096
rng = np.random.default_rng(0)
q = rng.integers(0, arch['n_quant'], size=(B, T)).astype(np.int32)
ids = np.ones((B, T), np.int32)
nets, opts = [], [AdamOptimizer(1e-3), AdamOptimizer(1e-3, clip_norm=1.0)]
for _ in opts:
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=1e-3, print_interval=0, seed=0)
    net.init_vars(0, bias_scale=0.1)
    nets.append(net)
qd, idd = torch.tensor(q, device=dev), torch.tensor(ids, device=dev)
KS, BLOCKS, WB = 5, 16, 3
st = [[], []]
for r in range(WB + BLOCKS):
    for i in (0, 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(KS):
            nets[i].forward(qd, None, idd, backward=True)
            opts[i].apply(nets[i])
        e1.record()
        e1.synchronize()
        if r >= WB:
            st[i].append(e0.elapsed_time(e1) / KS)
for name, t, net in zip(('plain', 'clip_norm=1'), st, nets):
    t = np.array(t)
    net.check_status()
    say('C2 step %-12s %7.4f ms median [%7.4f, %7.4f] over %d blocks of %d steps' % (
        name, np.median(t), np.percentile(t, 10), np.percentile(t, 90), BLOCKS, KS))
say('clip info', opts[1].grad_info(nets[1]).tolist(), 'skips', opts[1].nonfinite_skips(nets[1]))
