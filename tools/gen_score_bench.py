"""Teacher-forced scoring (lbwn_gen_score) against the prefill of the same plan and against
the sequential teacher path it replaces.  Per (arch, B): the generator is brought from lbwn_gen_start to
step n with one shared prompt by (a) WaveNetGen.prefill, (b) WaveNetGen.score, (c) n teacher-forced steps
through graph replays; each is timed with device events around the call alone (the reset is outside),
after one warm-up, as the median of --reps runs, (a) and (b) alternating in one loop.  Archs with local
conditioning get a random mel covering the prompt.  Writes a markdown table to --out: the three times, the
ratio score / prefill, the head's work (2·rows·(L·n_dil·n_skip + n_skip·n_post + n_post·n_quant) FLOP) and,
with --kernel-stats (the *kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool with
--score-only and ONE (arch, B)), the kernel time of the score calls by kernel family and the three GEMMs'
achieved TFLOP/s.  No test asserts these times."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--case', nargs='+', default=['arch3:10', 'arch3:80', 'arch5:10'], metavar='ARCH:B',
                help='par/<ARCH>.json at B voices')
ap.add_argument('--n', type=int, default=48000)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--chunk', type=int, default=1000, help='graph-replay chunk of the sequential path')
ap.add_argument('--score-only', action='store_true', help='only the score calls (for a profiler run)')
ap.add_argument('--kernel-stats', default=None, metavar='CSV')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_gen_score.md'))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz  # noqa: E402
from lbwn.imodel import WaveNetGen  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

assert torch.cuda.is_available(), 'needs an MI355X'


def event_ms(fn, reset):
    reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fns, reset):
    """[(median, min, max) in ms] of each fn between device events, the fns alternating; reset() before
    each, one warm-up round"""
    ms = [[] for _ in fns]
    for r in range(a.reps + 1):
        for i, fn in enumerate(fns):
            t = event_ms(fn, reset)
            if r:
                ms[i].append(t)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def head_flop(arch, rows):
    L = arch['n_blocks'] * arch['n_block_layers']
    return 2.0 * rows * (L * arch['n_dil'] * arch['n_skip'] + arch['n_skip'] * arch['n_post']
                         + arch['n_post'] * arch['n_quant'])


n = a.n
rows = []
nets = {}
for case in a.case:
    name, B = case.split(':')
    B = int(B)
    arch = load_arch(os.path.join(ROOT, 'par', name + '.json'))
    if name not in nets:
        nets[name] = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)
    lc = arch['n_lc_out'] > 0
    codes = torch.as_tensor(np.random.default_rng(n).integers(0, arch['n_quant'], n).astype(np.int32), device='cuda')
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, a.chunk, None, seed=1, n_lc_in=arch['n_lc_in'], n_lc_out=arch['n_lc_out'],
                   lc_upsample=arch['lc_upsample'])
    g.load_params(nets[name])
    g.build_graph(n)
    gc = list(range(1, B + 1)) if arch['n_gc_embed'] else None
    mel = None
    if lc:   # the rows of steps 0 .. n-1
        mel = torch.randn(B, -(-n // mel_hop_sz(arch)), arch['n_lc_in'], generator=torch.Generator().manual_seed(n))
        mel = mel.to('cuda')

    def reset():
        g.init_buffers(gc, mel=mel)

    out = {}

    def do_score():
        out['logp'] = g.score(codes)

    if a.score_only:
        pf, (sc,) = None, timed([do_score], reset)
    else:
        pf, sc = timed([lambda: g.prefill(codes), do_score], reset)
    assert int(g.tensor('step', torch.int64).item()) == n
    logp = out['logp']
    assert bool(torch.isfinite(logp).all()) and float(logp.max()) <= 0.0
    nats = -float(logp.double().mean())
    scratch_mb = g.lib.lbwn_gen_score_scratch_bytes(g._plan) / 1e6
    seq = None
    if not a.score_only:
        g.teacher_mu = codes
        g.build_graph(n)        # a plan with room for the teacher vector
        (seq,) = timed([lambda: g.step(n)], reset)
        assert int(g.tensor('step', torch.int64).item()) == n
        g.check_status()
    rows.append((name, B, g.persistent, pf, sc, seq, head_flop(arch, B * n), scratch_mb, nats))
    print('%s B=%d n=%d score %.3f ms%s, mean -logp %.4f nats' % (
        name, B, n, sc[0], '' if pf is None else ', prefill %.3f ms (x%.2f), sequential %.1f ms (%.0fx score)' % (
            pf[0], sc[0] / pf[0], seq[0], seq[0] / sc[0]), nats), flush=True)
    del g

fmt = lambda t: 'not measured' if t is None else '%.3f (%.3f .. %.3f)' % t   # noqa: E731
md = ['# Teacher-forced scoring against prefill and the sequential teacher path (n = %d codes)' % n, '',
      'Device events around the call, one warm-up, median of %d (min .. max); prefill and score alternate in one' % a.reps,
      'loop on one plan; the sequential path steps through graph replays of %d steps.' % a.chunk, '',
      '| arch | B | form | prefill ms | score ms | score / prefill | sequential ms | sequential / score | head GFLOP | '
      '(score - prefill) ms | scratch MB | mean -logp nats |',
      '|---|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|']
for name, B, pers, pf, sc, seq, fl, smb, nats in rows:
    md.append('| %s | %d | %s | %s | %s | %s | %s | %s | %.1f | %s | %.0f | %.4f |' % (
        name, B, 'persistent' if pers else 'per step', fmt(pf), fmt(sc),
        'not measured' if pf is None else '%.2f' % (sc[0] / pf[0]), fmt(seq),
        'not measured' if seq is None else '%.0fx' % (seq[0] / sc[0]), fl / 1e9,
        'not measured' if pf is None else '%.3f' % (sc[0] - pf[0]), smb, nats))
if a.kernel_stats:
    assert len(rows) == 1, '--kernel-stats describes a run of one case'
    name, B, _, _, _, _, fl, _, _ = rows[0]
    calls = a.reps + 1
    groups = {}
    for r in csv.DictReader(open(a.kernel_stats)):
        nm = r['Name']
        key = ('head GEMMs (gemm_x3*)' if 'gemm_' in nm else
               'log-softmax gather (gen_score_logp_kernel)' if 'gen_score_logp' in nm else
               'layer launches (layer_fwd_kernel)' if 'layer_fwd_kernel' in nm else
               'LC projection (gen_prefill_lcproj_kernel)' if 'gen_prefill_lcproj' in nm else
               'ring <-> halo copies (gen_prefill_xfer_kernel)' if 'gen_prefill_xfer' in nm else
               'embed (gen_prefill_embed_kernel)' if 'gen_prefill_embed' in nm else
               'pack / GC table / outputs / finish' if ('gen_prefill' in nm or 'pack_layers_kernel' in nm) else None)
        if key:
            c, t = groups.get(key, (0, 0.0))
            groups[key] = (c + int(r['Calls']), t + float(r['TotalDurationNs']))
    tot = sum(t for _, t in groups.values())
    md += ['', '## Kernel time of the score calls (%s, B = %d; rocprofv3 --kernel-trace --stats, a run of its own, '
               '%d calls)' % (name, B, calls), '',
           '| kernels | launches | total us | avg us | % |', '|---|---:|---:|---:|---:|']
    for k, (c, t) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        md.append('| %s | %d | %.1f | %.2f | %.1f |' % (k, c, t / 1e3, t / 1e3 / c, 100 * t / tot))
    gt = groups.get('head GEMMs (gemm_x3*)', (0, 0.0))[1]
    if gt:
        md += ['', 'The three GEMMs: %.3f ms per call for %.1f GFLOP = %.1f TFLOP/s.' % (
            gt / 1e6 / calls, fl / 1e9, fl * calls / gt / 1e3)]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, 'w').write('\n'.join(md) + '\n')
print('wrote', a.out)
