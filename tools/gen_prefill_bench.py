"""Prompt prefill against the sequential teacher path: arch3, B = 10 and 80, prompts
of 4,096 and 48,000 codes.  Both paths bring the generator from lbwn_gen_start to step n with the same
shared prompt; each is timed with device events around the call alone (the reset is outside), after
one warm-up, as the median of --reps runs.  Writes a markdown table (both times and the ratio) to
--out; with --kernel-stats (the *kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this
tool with --prefill-only) the prefill's kernel time is split into the layer launches and the
embed / copy / finish kernels (LC archs: and the LC projection launches).  Archs with local
conditioning get a random mel covering the prompt; --strip-lc runs the same arch without
its n_lc_* keys, as tools/arch5_nogc.json does for GC.  No test asserts these times."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--arch', default=os.path.join(ROOT, 'par', 'arch3.json'))
ap.add_argument('--batch', type=int, nargs='+', default=[10, 80])
ap.add_argument('--n', type=int, nargs='+', default=[4096, 48000])
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--chunk', type=int, default=1000, help='graph-replay chunk of the sequential path')
ap.add_argument('--prefill-only', action='store_true', help='no sequential runs (for a profiler run)')
ap.add_argument('--kernel-stats', default=None, metavar='CSV')
ap.add_argument('--strip-lc', action='store_true', help='run the arch without its local conditioning')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_gen_prefill.md'))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz, normalize_arch  # noqa: E402
from lbwn.imodel import WaveNetGen  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

assert torch.cuda.is_available(), 'needs an MI355X'
arch = load_arch(a.arch)
if a.strip_lc:
    arch = normalize_arch({k: v for k, v in arch.items() if k not in ('n_lc_in', 'n_lc_out', 'lc_upsample')})
lc = arch['n_lc_out'] > 0
net = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)


def timed(fn, reset):
    """median, min, max in ms of fn() between device events; reset() before each, one warm-up"""
    ms = []
    for r in range(a.reps + 1):
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


rows = []
for B in a.batch:
    for n in a.n:
        codes = torch.as_tensor(np.random.default_rng(n).integers(0, arch['n_quant'], n).astype(np.int32), device='cuda')
        g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                       arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                       B, a.chunk, None, seed=1, n_lc_in=arch['n_lc_in'], n_lc_out=arch['n_lc_out'],
                       lc_upsample=arch['lc_upsample'])
        g.load_params(net)
        g.build_graph(n)
        gc = list(range(1, B + 1)) if arch['n_gc_embed'] else None
        mel = None
        if lc:   # the rows of steps 0 .. n-1
            mel = torch.randn(B, -(-n // mel_hop_sz(arch)), arch['n_lc_in'], generator=torch.Generator().manual_seed(n))
            mel = mel.to('cuda')
        pf = timed(lambda: g.prefill(codes), lambda: g.init_buffers(gc, mel=mel))
        assert int(g.tensor('step', torch.int64).item()) == n
        seq = None
        if not a.prefill_only:
            g.teacher_mu = codes
            g.build_graph(n)        # a plan with room for the teacher vector
            seq = timed(lambda: g.step(n), lambda: g.init_buffers(gc, mel=mel))
            assert int(g.tensor('step', torch.int64).item()) == n
            g.check_status()
        rows.append((B, n, g.persistent, pf, seq))
        print('B=%d n=%d prefill %.3f ms%s' % (B, n, pf[0], '' if seq is None else
                                              ', sequential %.1f ms, ratio %.0fx' % (seq[0], seq[0] / pf[0])), flush=True)

out = ['# Prompt prefill against the sequential teacher path (%s%s)' % (
    os.path.basename(a.arch), ', local conditioning stripped' if a.strip_lc else ''), '',
       'Device events around the call, one warm-up, median of %d (min .. max); the sequential path steps' % a.reps,
       'through graph replays of %d steps.' % a.chunk, '',
       '| B | prompt n | form | prefill ms | sequential ms | ratio | prefill us per code |', '|---:|---:|---|---:|---:|---:|---:|']
for B, n, pers, pf, seq in rows:
    out.append('| %d | %d | %s | %.3f (%.3f .. %.3f) | %s | %s | %.3f |' % (
        B, n, 'persistent' if pers else 'per step', pf[0], pf[1], pf[2],
        'not measured' if seq is None else '%.1f (%.1f .. %.1f)' % seq,
        'not measured' if seq is None else '%.0fx' % (seq[0] / pf[0]), 1e3 * pf[0] / n))
if a.kernel_stats:
    ks = list(csv.DictReader(open(a.kernel_stats)))
    groups = {}
    for r in ks:
        nm = r['Name']
        key = ('layer launches (layer_fwd_kernel)' if 'layer_fwd_kernel' in nm else
               'LC projection (gen_prefill_lcproj_kernel)' if 'gen_prefill_lcproj' in nm else
               'ring <-> halo copies (gen_prefill_xfer_kernel)' if 'gen_prefill_xfer' in nm else
               'embed (gen_prefill_embed_kernel)' if 'gen_prefill_embed' in nm else
               'pack / GC table / outputs / finish' if ('gen_prefill' in nm or 'pack_layers_kernel' in nm) else None)
        if key:
            c, t = groups.get(key, (0, 0.0))
            groups[key] = (c + int(r['Calls']), t + float(r['TotalDurationNs']))
    tot = sum(t for _, t in groups.values())
    out += ['', '## Kernel time of the prefill calls (rocprofv3 --kernel-trace --stats, a run of its own)', '',
            '| kernels | launches | total us | avg us | % |', '|---|---:|---:|---:|---:|']
    for k, (c, t) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        out.append('| %s | %d | %.1f | %.2f | %.1f |' % (k, c, t / 1e3, t / 1e3 / c, 100 * t / tot))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, 'w').write('\n'.join(out) + '\n')
print('wrote', a.out)
