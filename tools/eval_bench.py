"""Held-out evaluation (lbwn_train_eval) against the training forward of the same plan.
Per arch at B x T: (a) lbwn_train_forward, (b) lbwn_train_eval with only acc, (c) lbwn_train_eval with
nll and by_voice (--bins bins), in one process on one plan and workspace, the three forms alternating in
one loop.  Each sample is device events around --launches consecutive launches of one form, divided by
their number; after one warm-up round the median of --reps samples is reported with min and max, and
the spread (max - min) / median of each form is the box's repeat spread the forms are compared
against.  Prints a markdown table (the one in profiles/r15_eval.md) and, with --out, also writes it to
that file.  No test asserts these times."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--arch', nargs='+', default=['arch3', 'arch5'])
ap.add_argument('-B', type=int, default=8)
ap.add_argument('-T', type=int, default=4096)
ap.add_argument('--bins', type=int, default=377)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None, help='also write the table to this file (it is overwritten)')
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('eval_bench: no GPU found (needs an MI355X)')


def sample_ms(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.launches


rows = []
for name in a.arch:
    arch = load_arch(os.path.join(ROOT, 'par', name + '.json'))
    B, T = a.B, a.T
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=0.0, print_interval=0, seed=0)
    net.init_vars(0, bias_scale=0.1)
    rng = np.random.default_rng(0)
    q = torch.as_tensor(rng.integers(0, arch['n_quant'], (B, T)).astype(np.int32), device='cuda')
    nvoice = max(1, min(arch['n_gc_category'] or a.bins - 1, a.bins - 1))
    ids = np.repeat(rng.integers(1, nvoice + 1, (B, T // 512)), 512, axis=1).astype(np.int32)
    ids[:, :T // 4] = 0                       # the invalid windows at a stream's start
    ids = torch.as_tensor(ids, device='cuda')
    mel = None
    if arch['n_lc_out'] > 0:
        mel = torch.randn(B, T // mel_hop_sz(arch), arch['n_lc_in'], generator=torch.Generator().manual_seed(0)).cuda()
    lean, full = net.eval_state(), net.eval_state(a.bins)
    nll = torch.zeros(B, T, device='cuda')
    forms = [('lbwn_train_forward', lambda: net.forward(q, mel, ids, backward=False)),
             ('lbwn_train_eval, acc only', lambda: net.eval_slice(lean, q, mel, ids)),
             ('lbwn_train_eval, nll + by_voice (%d bins)' % a.bins, lambda: net.eval_slice(full, q, mel, ids, nll=nll))]
    ms = [[] for _ in forms]
    for r in range(a.reps + 1):
        for i, (_, fn) in enumerate(forms):
            t = sample_ms(fn)
            lean['keep'].clear()
            full['keep'].clear()
            if r:
                ms[i].append(t)
    assert int(lean['status'].item()) == 0 and int(full['status'].item()) == 0 and net.status(T) == 0
    n = (a.reps + 1) * a.launches
    assert lean['acc'][1].item() == full['acc'][1].item() == n * net.stats[1].item()
    assert full['by_voice'][:, 1].sum().item() == full['acc'][1].item()
    scratch = [net.lib.lbwn_train_eval_scratch_bytes(net._plan(T), k) for k in (0, a.bins)]
    for i, (form, _) in enumerate(forms):
        med = statistics.median(ms[i])
        rows.append((name, form, med, min(ms[i]), max(ms[i]), (max(ms[i]) - min(ms[i])) / med,
                     med - statistics.median(ms[0]), None if i == 0 else scratch[i - 1]))
        print('%s %-44s %.1f us (%.1f .. %.1f)' % (name, form, med * 1e3, min(ms[i]) * 1e3, max(ms[i]) * 1e3), flush=True)
    del net

md = ['# Held-out evaluation against the training forward (B = %d, T = %d)' % (a.B, a.T), '',
      'Device events around %d consecutive launches of one form, per launch; one warm-up round, then the median of' % a.launches,
      '%d samples (min .. max); the three forms alternate in one loop on one plan and workspace.  spread =' % a.reps,
      '(max - min) / median of the form\'s own samples.', '',
      '| arch | form | us per launch | spread | minus train_forward us | scratch bytes |', '|---|---|---:|---:|---:|---:|']
for name, form, med, lo, hi, spread, diff, sb in rows:
    md.append('| %s | %s | %.1f (%.1f .. %.1f) | %.2f %% | %+.1f | %s |' % (
        name, form, med * 1e3, lo * 1e3, hi * 1e3, 100 * spread, diff * 1e3, '' if sb is None else '%d' % sb))
print('\n'.join(md), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(md) + '\n')
    print('wrote', a.out)
