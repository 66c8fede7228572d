"""The cost of dmel (lbwn_train_backward_ex): the backward of one arch at T = 4096 with and
without the gradient into the mel input, at B = 8 (128 mel frames for arch5: the fused upsample backward
writes dmel) and B = 32 (512 frames: one more GEMM after the per-stage products).  Three forms on one
plan and workspace in one process, alternating in one loop: (a) lbwn_train_backward, (b)
lbwn_train_backward_ex with dmel NULL, (c) lbwn_train_backward_ex with dmel.  Every backward follows its
own lbwn_train_forward (not timed); a sample is the sum of device events around --launches backwards of
one form, divided by their number; after one warm-up round the median of --reps samples is reported
with min and max, and the spread (max - min) / median of each form is the box's repeat spread the forms
are compared against.  --plain-only: form (a) alone, for a library from before the call existed (under
tools/with_lib.py: same-box A/B against a tools/build_variant.sh build of the parent commit).  Prints a
markdown table and one JSON line per batch size; --out also writes the table.  No test asserts these
times."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--arch', default='arch5')
ap.add_argument('-B', type=int, nargs='+', default=[8, 32])
ap.add_argument('-T', type=int, default=4096)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--plain-only', action='store_true')
ap.add_argument('--tag', default='')
ap.add_argument('--out', default=None, help='also write the table to this file (it is overwritten)')
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn import _lib  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('dmel_bench: no GPU found (needs an MI355X)')

rows = []
for B in a.B:
    arch = load_arch(os.path.join(ROOT, 'par', a.arch + '.json'))
    T = a.T
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=0.0, print_interval=0, seed=0)
    net.init_vars(0, bias_scale=0.1)
    rng = np.random.default_rng(0)
    q = torch.as_tensor(rng.integers(0, arch['n_quant'], (B, T)).astype(np.int32), device='cuda')
    nvoice = max(1, arch['n_gc_category'])
    ids = np.repeat(rng.integers(1, nvoice + 1, (B, T // 512)), 512, axis=1).astype(np.int32)
    ids[:, :T // 4] = 0                       # the invalid windows at a stream's start
    ids = torch.as_tensor(ids, device='cuda')
    frames = T // mel_hop_sz(arch)
    mel = torch.randn(B, frames, arch['n_lc_in'], generator=torch.Generator().manual_seed(0)).cuda()
    dmel = torch.empty_like(mel)
    h, lib = net._plan(T), net.lib
    P, G, ws = ctypes.byref(net._params_c), ctypes.byref(net._grads_c), net._ws.data_ptr()
    sp = _lib.stream_ptr()

    def plain():
        _lib.check(lib.lbwn_train_backward(h, P, G, ws, q.data_ptr(), ids.data_ptr(), mel.data_ptr(), sp))

    def ex(out):
        args = _lib.BackwardArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=mel.data_ptr(),
                                 dmel=out.data_ptr() if out is not None else None)
        _lib.check(lib.lbwn_train_backward_ex(h, P, G, ws, ctypes.byref(args), sp))

    forms = [('lbwn_train_backward', plain)]
    if not a.plain_only:
        forms += [('lbwn_train_backward_ex, dmel NULL', lambda: ex(None)),
                  ('lbwn_train_backward_ex, dmel', lambda: ex(dmel))]

    def sample_ms(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        torch.cuda.synchronize()
        for e0, e1 in ev:
            net.forward(q, mel, ids, backward=False)
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.launches

    ms = [[] for _ in forms]
    for r in range(a.reps + 1):
        for i, (_, fn) in enumerate(forms):
            t = sample_ms(fn)
            if r:
                ms[i].append(t)
    assert net.status(T) == 0
    fused = -2 if a.plain_only else net.plan_info(T, 'dmel_fused')
    assert a.plain_only or bool(torch.isfinite(dmel).all())
    res = {}
    for i, (form, _) in enumerate(forms):
        med = statistics.median(ms[i])
        rows.append((B, B * frames, fused, form, med, min(ms[i]), max(ms[i]), (max(ms[i]) - min(ms[i])) / med,
                     med - statistics.median(ms[0])))
        res[form] = dict(median_us=med * 1e3, min_us=min(ms[i]) * 1e3, max_us=max(ms[i]) * 1e3)
    print(json.dumps(dict(tag=a.tag, arch=a.arch, B=B, T=T, frames=B * frames, dmel_fused=fused, forms=res)), flush=True)
    del net

md = ['# The backward with and without dmel (%s, T = %d)' % (a.arch, a.T), '',
      'Device events around each backward (its forward before it, not timed), %d per sample; one warm-up round, then' % a.launches,
      'the median of %d samples (min .. max); the forms alternate in one loop on one plan and workspace.  spread =' % a.reps,
      '(max - min) / median of the form\'s own samples.  dmel_fused: 1 = the fused upsample backward wrote dmel, 0 = a GEMM.', '',
      '| B | mel frames | dmel_fused | form | us per backward | spread | minus lbwn_train_backward us |',
      '|---:|---:|---:|---|---:|---:|---:|']
for B, fr, fused, form, med, lo, hi, spread, diff in rows:
    md.append('| %d | %d | %s | %s | %.1f (%.1f .. %.1f) | %.2f %% | %+.1f |' % (
        B, fr, '' if fused == -2 else '%d' % fused, form, med * 1e3, lo * 1e3, hi * 1e3, 100 * spread, diff * 1e3))
print('\n'.join(md), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(md) + '\n')
    print('wrote', a.out)
