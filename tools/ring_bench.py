"""Ring plans of the cached generator (lbwn_gen_plan_create_ex): three measurements, one
process, the forms interleaved inside every repetition, the median of --reps with min .. max beside it.

1. Per-step cost of the ring addressing for each --arch and --batch: microseconds per step of a run of --steps
   steps in session mode (every stream begun at step 0; on an LC arch with a mel of --ring steps, clamped
   after it) on a ring plan of --ring steps and on the plan without a ring of the same library, and, with
   --parent-lib, the plan without a ring of that other build of liblbwn.so (the parent commit's).
2. What the ring buys on a list (the first LC arch of --arch): a seeded list of --utts utterances, lengths
   uniform in [1, 4] s at --rate Hz, vocoded in the groups generate.py --mel-list cuts at --budget-mb
   (mel_list_groups, one plan_sessions schedule per group) against one ring schedule for the whole list.
   The expected ratio is arithmetic on the lengths (the groups' totals over plan_ring's total).
3. One lbwn_gen_extend call of --extend-frames frames for 1 stream and for all streams of the largest
   --batch, and one lbwn_gen_collect of --collect steps against a device-to-device copy of the same bytes.

Writes a markdown report to --out.  No test asserts these times."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--arch', nargs='+', default=[os.path.join(ROOT, 'par', 'arch3.json'), os.path.join(ROOT, 'par', 'arch5.json')])
ap.add_argument('--batch', type=int, nargs='+', default=[10, 80])
ap.add_argument('--steps', type=int, default=2048)
ap.add_argument('--ring', type=int, default=1024)
ap.add_argument('--utts', type=int, default=60)
ap.add_argument('--list-batch', type=int, default=10)
ap.add_argument('--list-ring', type=int, default=16000)
ap.add_argument('--budget-mb', type=float, default=256.0)
ap.add_argument('--rate', type=int, default=16000)
ap.add_argument('--chunk', type=int, default=1000)
ap.add_argument('--extend-frames', type=int, default=16)
ap.add_argument('--collect', type=int, default=1000)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--list-reps', type=int, default=2)
ap.add_argument('--parent-lib', default=None, help="another build's liblbwn.so for part 1")
ap.add_argument('--only-step-cost', action='store_true', help='part 1 alone')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_gen_ring.md'))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import generate  # noqa: E402
from lbwn import _lib  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz  # noqa: E402
from lbwn.imodel import WaveNetGen, plan_ring, plan_sessions  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

assert torch.cuda.is_available(), 'needs an MI355X'


def other_build(path):
    """A second liblbwn.so beside the product's, with the signatures a session run without a ring needs."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ('lbwn_gen_plan_create', 'lbwn_gen_plan_destroy', 'lbwn_gen_workspace_bytes', 'lbwn_gen_tensor',
                 'lbwn_gen_start', 'lbwn_gen_begin', 'lbwn_gen_run', 'lbwn_gen_is_persistent',
                 'lbwn_gen_set_sampling', 'lbwn_last_error'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    return lib


def make_gen(arch, net, B, max_steps, ring=0, lib=None, chunk=None):
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, chunk or a.chunk, None, seed=1, n_lc_in=arch['n_lc_in'], n_lc_out=arch['n_lc_out'],
                   lc_upsample=arch['lc_upsample'] if arch['n_lc_out'] else (), ring_steps=ring)
    if lib is not None:
        g.lib = lib
    g.load_params(net)
    g.build_graph(max_steps)
    return g


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(v):
    return statistics.median(v), min(v), max(v)


rng = np.random.default_rng(19)
parent = other_build(a.parent_lib) if a.parent_lib else None
out = ['# Ring plans of the cached generator', '',
       'One process; the forms alternate inside every repetition; median (min .. max).', '',
       '## Per-step cost: %d steps in session mode, ring of %d steps, device events around the run' % (a.steps, a.ring),
       '', '| arch | B | form | no ring us/step | ring us/step | ring - no ring | %sspread of no ring (max - min) |'
       % ('parent us/step | no ring - parent | spread of parent | ' if parent else ''),
       '|---|---:|---|---:|---:|---:|%s---:|' % ('---:|---:|---:|' if parent else '')]
nets = {}
for path in a.arch:
    arch = load_arch(path)
    net = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)
    net.init_vars(3, bias_scale=0.2)
    nets[path] = (arch, net)
    lc = arch['n_lc_out'] > 0
    hop = mel_hop_sz(arch) if lc else 1
    for B in a.batch:
        gc = [1 + (37 * b) % arch['n_gc_category'] for b in range(B)] if arch['n_gc_embed'] else None
        mel = list(rng.standard_normal((B, max(1, a.ring // hop), arch['n_lc_in'])).astype(np.float32)) if lc else None
        gens = {'plain': make_gen(arch, net, B, a.steps), 'ring': make_gen(arch, net, B, a.steps, ring=a.ring)}
        if parent is not None:
            gens['parent'] = make_gen(arch, net, B, a.steps, lib=parent)
        t = {k: [] for k in gens}
        for g in gens.values():
            g.use_graph = False          # one lbwn_gen_run call: the launches themselves
        for r in range(a.reps + 1):
            for name, g in gens.items():
                g.init_sessions()
                g.begin(list(range(B)), mel, gc_ids=gc, keys=list(range(B)))
                ms = events(lambda: g.step(a.steps))
                g.check_status()
                if r:
                    t[name].append(1e3 * ms / a.steps)
        # the same run: the ring holds the last --ring samples of the plain plan's
        n = min(a.ring, a.steps)
        ring_tail = gens['ring'].collect(0, a.steps - n, n)[1]
        assert torch.equal(ring_tail, gens['plain'].samples()[0, a.steps - n:a.steps])
        d, s = med(t['plain']), med(t['ring'])
        row = '| %s | %d | %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %+.2f |' % (
            (os.path.basename(path), B, 'persistent' if gens['plain'].persistent else 'per step') + d + s + (s[0] - d[0],))
        if parent is not None:
            p = med(t['parent'])
            row += ' %.2f (%.2f .. %.2f) | %+.2f | %.2f |' % (p + (d[0] - p[0], p[2] - p[1]))
        out.append(row + ' %.2f |' % (d[2] - d[1]))
        print(row, flush=True)
        del gens

if a.only_step_cost:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(out) + '\n')
    print('wrote', a.out)
    sys.exit(0)

# ---- 2. a list larger than its budget ----------------------------------------------------------
path = next(p for p in a.arch if nets[p][0]['n_lc_out'] > 0)
arch, net = nets[path]
hop, Li, B = mel_hop_sz(arch), arch['n_lc_in'], a.list_batch
secs = rng.uniform(1.0, 4.0, a.utts)
fr = [max(1, int(round(s * a.rate / hop))) for s in secs]
lengths = [f * hop for f in fr]
mels = [rng.standard_normal((f, Li)).astype(np.float32) for f in fr]
voices = [1 + (37 * u) % arch['n_gc_category'] for u in range(a.utts)] if arch['n_gc_embed'] else None
budget = int(a.budget_mb * 2 ** 20)
groups = generate.mel_list_groups(lengths, B, a.chunk, arch['n_lc_out'], arch['lc_upsample'], budget)
totals = [plan_sessions([lengths[u] for u in grp], B, a.chunk)[1] for grp in groups]
ring_rounds, ring_total = plan_ring(lengths, B, a.chunk, a.list_ring, hop)
gg = make_gen(arch, net, B, max(totals))
gr = make_gen(arch, net, B, 1, ring=a.list_ring)


def run_groups():
    return [w for grp in groups for w in gg.vocode([mels[u] for u in grp], gc_ids=[voices[u] for u in grp] if voices
                                                  else None, keys=grp, chunk=a.chunk)]


def run_ring():
    return gr.vocode(mels, gc_ids=voices, chunk=a.chunk)


tg, tr = [], []
for r in range(a.list_reps + 1):
    wg = []
    x = wall(lambda: wg.extend(run_groups()))
    wr = []
    y = wall(lambda: wr.extend(run_ring()))
    assert all(torch.equal(p, q) for p, q in zip(wg, wr))        # the same wavs, bit for bit
    if r:
        tg.append(x)
        tr.append(y)
g_, r_ = med(tg), med(tr)
out += ['', '## A list larger than its budget: %s, %d utterances, lengths U[1, 4] s at %d Hz (hop %d), B = %d, chunk %d'
        % (os.path.basename(path), a.utts, a.rate, hop, B, a.chunk), '',
        'Wall clock around the whole list, host work included; graph replay of whole chunks in both; the wavs are',
        'compared bit for bit.  Grouped: generate.py --mel-list at --mel-list-budget-mb %g, %d groups.  Ring: one'
        % (a.budget_mb, len(groups)), 'schedule, ring of %d steps, %d rounds.' % (a.list_ring, len(ring_rounds)), '',
        '| | steps | seconds | audio s per s | workspace bytes |', '|---|---:|---:|---:|---:|',
        '| grouped (%d plans\' worth, the largest shown) | %d | %.3f (%.3f .. %.3f) | %.1f | %d |' % (
            (len(groups), sum(totals)) + g_ + (sum(lengths) / a.rate / g_[0], gg._ws.numel())),
        '| one ring schedule | %d | %.3f (%.3f .. %.3f) | %.1f | %d |' % (
            (ring_total,) + r_ + (sum(lengths) / a.rate / r_[0], gr._ws.numel())),
        '', 'Expected ratio (steps, arithmetic on the lengths): %.3f.  Measured ratio (seconds): %.3f.' % (
            sum(totals) / ring_total, g_[0] / r_[0]),
        'A plan without a ring for the whole list in one schedule would hold %d steps per stream: %d bytes of outputs,'
        % (plan_sessions(lengths, B, a.chunk)[1], generate.mel_list_bytes(plan_sessions(lengths, B, a.chunk)[1], B,
                                                                         arch['n_lc_out'], arch['lc_upsample'])),
        'upsampled mels and stage scratch.']
print('\n'.join(out[-9:]), flush=True)
del gg, gr

# ---- 3. one extend, one collect ----------------------------------------------------------------
B = max(a.batch)
R = max(a.collect, 4 * a.extend_frames * hop)
g = make_gen(arch, net, B, 1, ring=R, chunk=a.collect)
g.use_graph = False
first = [rng.standard_normal((a.extend_frames, Li)).astype(np.float32) for _ in range(B)]
more = [torch.as_tensor(rng.standard_normal((a.extend_frames, Li)).astype(np.float32), device='cuda') for _ in range(B)]
gc = [1 + (37 * b) % arch['n_gc_category'] for b in range(B)] if arch['n_gc_embed'] else None
out += ['', '## One lbwn_gen_extend call (%d frames per stream) and one lbwn_gen_collect (%d steps), B = %d, ring %d'
        % (a.extend_frames, a.collect, B, R), '', 'Device events around the call.', '',
        '| call | streams | microseconds |', '|---|---:|---:|']
for n in (1, B):
    ts = []
    for r in range(a.reps + 1):
        g.init_sessions()
        g.begin(list(range(B)), first, gc_ids=gc, keys=list(range(B)))
        ms = events(lambda: g.extend(list(range(n)), more[:n]))
        g.check_status()
        if r:
            ts.append(1e3 * ms)
    out.append('| extend | %d | %.1f (%.1f .. %.1f) |' % ((n,) + med(ts)))
    print(out[-1], flush=True)
g.step(a.collect)
src = torch.empty(a.collect, dtype=torch.float32, device='cuda')
dst = torch.empty_like(src)
tc, tm, tb = [], [], []
for r in range(a.reps + 1):
    x = events(lambda: g.collect(0, 0, a.collect))
    y = events(lambda: [g.collect(b, 0, a.collect) for b in range(B)])
    z = events(lambda: (dst.copy_(src), dst.copy_(src)))       # wav and samples: two copies of 4·n bytes
    if r:
        tc.append(1e3 * x)
        tb.append(1e3 * y)
        tm.append(1e3 * z)
g.check_status()
out += ['| collect (wav and samples, allocation included) | 1 | %.1f (%.1f .. %.1f) |' % med(tc),
        '| collect | %d | %.1f (%.1f .. %.1f) |' % ((B,) + med(tb)),
        '| two device-to-device copies of %d bytes | 1 | %.1f (%.1f .. %.1f) |' % ((4 * a.collect,) + med(tm))]
print('\n'.join(out[-3:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, 'w').write('\n'.join(out) + '\n')
print('wrote', a.out)
