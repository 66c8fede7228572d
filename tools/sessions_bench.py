"""Sessions in the cached generator (lbwn_gen_begin): three measurements, one process, the
forms interleaved inside every repetition, the median of --reps with min .. max beside it.

1. Per-step cost at --arch (arch5) for each --batch: microseconds per step of a run of --steps steps on the
   dense lbwn_gen_set_mel path and in session mode (every stream begun at step 0), and, with --parent-lib, the
   dense path of that other build of liblbwn.so (the parent commit's) loaded beside this one.
2. List throughput: a synthetic list of --utts utterances, lengths uniform in [1, 4] s at --rate Hz (seeded),
   vocoded by WaveNetGen.vocode at --list-batch streams against the same list as padded static batches of
   consecutive utterances on the lbwn_gen_set_mel path.  The expected ratio is arithmetic on the lengths
   alone (sum of the padded batches' steps over plan_sessions' total) and is printed beside the measured one.
3. The cost of one lbwn_gen_begin call for 1 stream and for all streams of the largest --batch.

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
ap.add_argument('--arch', default=os.path.join(ROOT, 'par', 'arch5.json'))
ap.add_argument('--batch', type=int, nargs='+', default=[10, 80])
ap.add_argument('--steps', type=int, default=2048)
ap.add_argument('--utts', type=int, default=30)
ap.add_argument('--list-batch', type=int, default=10)
ap.add_argument('--rate', type=int, default=16000)
ap.add_argument('--chunk', type=int, default=1000)
ap.add_argument('--begin-frames', type=int, default=100)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--list-reps', type=int, default=3)
ap.add_argument('--parent-lib', default=None, help="another build's liblbwn.so for the dense path of part 1")
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_gen_sessions.md'))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn import _lib  # noqa: E402
from lbwn.arch import load_arch, mel_hop_sz  # noqa: E402
from lbwn.imodel import WaveNetGen, plan_sessions  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

assert torch.cuda.is_available(), 'needs an MI355X'
arch = load_arch(a.arch)
assert arch['n_lc_out'] > 0, 'an arch with local conditioning, please'
hop, Li = mel_hop_sz(arch), arch['n_lc_in']
net = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)
net.init_vars(3, bias_scale=0.2)


def other_build(path):
    """A second liblbwn.so beside the product's, with the signatures the dense path needs."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ('lbwn_gen_plan_create', 'lbwn_gen_plan_destroy', 'lbwn_gen_workspace_bytes', 'lbwn_gen_tensor',
                 'lbwn_gen_start', 'lbwn_gen_set_mel', 'lbwn_gen_run', 'lbwn_gen_is_persistent',
                 'lbwn_gen_set_sampling', 'lbwn_last_error'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    return lib


def make_gen(B, max_steps, lib=None):
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, a.chunk, None, seed=1, n_lc_in=Li, n_lc_out=arch['n_lc_out'], lc_upsample=arch['lc_upsample'])
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


def med(v):
    return statistics.median(v), min(v), max(v)


rng = np.random.default_rng(16)
out = ['# Sessions in the cached generator (%s)' % os.path.basename(a.arch), '',
       'One process; the forms alternate inside every repetition; median (min .. max).', '']

# ---- 1. per-step cost --------------------------------------------------------------------------
parent = other_build(a.parent_lib) if a.parent_lib else None
out += ['## Per-step cost: %d steps, device events around the run' % a.steps, '',
        '| B | form | dense us/step | sessions us/step | sessions - dense | %sspread of dense (max - min) |'
        % ('parent dense us/step | dense - parent | ' if parent else ''),
        '|---:|---|---:|---:|---:|%s---:|' % ('---:|---:|' if parent else '')]
frames = -(-a.steps // hop)
for B in a.batch:
    gc = [1 + (37 * b) % arch['n_gc_category'] for b in range(B)] if arch['n_gc_embed'] else None
    mel = rng.standard_normal((B, frames, Li)).astype(np.float32)
    gens = {'dense': make_gen(B, a.steps), 'sessions': make_gen(B, a.steps)}
    if parent is not None:
        gens['parent'] = make_gen(B, a.steps, parent)
    for g in gens.values():
        g.use_graph = False          # one lbwn_gen_run call: the launches themselves

    def start(name):
        g = gens[name]
        if name == 'sessions':
            g.init_sessions()
            g.begin(list(range(B)), list(mel), gc_ids=gc, keys=list(range(B)))
        else:
            g.init_buffers(gc, mel)

    t = {k: [] for k in gens}
    for r in range(a.reps + 1):
        for name in gens:
            start(name)
            ms = events(lambda: gens[name].step(a.steps))
            gens[name].check_status()
            if r:
                t[name].append(1e3 * ms / a.steps)
    assert torch.equal(gens['dense'].samples(), gens['sessions'].samples())      # neutral sessions: the same run
    d, s = med(t['dense']), med(t['sessions'])
    row = '| %d | %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %+.2f |' % (
        (B, 'persistent' if gens['dense'].persistent else 'per step') + d + s + (s[0] - d[0],))
    if parent is not None:
        p = med(t['parent'])
        row += ' %.2f (%.2f .. %.2f) | %+.2f |' % (p + (d[0] - p[0],))
    out.append(row + ' %.2f |' % (d[2] - d[1]))
    print(row, flush=True)
    del gens

# ---- 2. list throughput ------------------------------------------------------------------------
B = a.list_batch
secs = rng.uniform(1.0, 4.0, a.utts)
fr = [max(1, int(round(s * a.rate / hop))) for s in secs]
lengths = [f * hop for f in fr]
mels = [rng.standard_normal((f, Li)).astype(np.float32) for f in fr]
voices = [1 + (37 * u) % arch['n_gc_category'] for u in range(a.utts)] if arch['n_gc_embed'] else None
rounds, total = plan_sessions(lengths, B, a.chunk)
batches = [list(range(i, min(i + B, a.utts))) for i in range(0, a.utts, B)]
padded = sum(max(lengths[u] for u in bt) for bt in batches)
order = sorted(range(a.utts), key=lambda u: lengths[u])
padded_sorted = sum(max(lengths[u] for u in order[i:i + B]) for i in range(0, a.utts, B))
gs = make_gen(B, total)
gd = make_gen(B, max(lengths))


def run_static():
    for bt in batches:
        n = max(lengths[u] for u in bt)
        m = np.zeros((B, n // hop, Li), np.float32)
        for i, u in enumerate(bt):
            m[i, :fr[u]] = mels[u]
        ids = [voices[bt[i % len(bt)]] for i in range(B)] if voices else None
        gd.init_buffers(ids, m)
        gd.step(n)
    gd.check_status()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


tv, tst = [], []
for r in range(a.list_reps + 1):
    x = wall(lambda: gs.vocode(mels, gc_ids=voices, chunk=a.chunk))
    y = wall(run_static)
    if r:
        tv.append(x)
        tst.append(y)
v, st = med(tv), med(tst)
n_begin = sum(1 for _, b in rounds if b)
out += ['', '## List throughput: %d utterances, lengths U[1, 4] s at %d Hz (hop %d), B = %d, chunk %d' % (
            a.utts, a.rate, hop, B, a.chunk), '',
        'Wall clock around the whole list, host work included (mel upload, lbwn_gen_start, the begins); graph',
        'replay of whole chunks in both.  Static: consecutive utterances in list order, %d batches, each run to its'
        % len(batches), 'longest member.', '',
        '| | steps | seconds | audio s per s |', '|---|---:|---:|---:|',
        '| padded static batches | %d | %.3f (%.3f .. %.3f) | %.1f |' % ((padded,) + st + (sum(lengths) / a.rate / st[0],)),
        '| vocode (sessions) | %d | %.3f (%.3f .. %.3f) | %.1f |' % ((total,) + v + (sum(lengths) / a.rate / v[0],)),
        '', 'Expected ratio (steps, arithmetic on the lengths): %.3f.  Measured ratio (seconds): %.3f.' % (
            padded / total, st[0] / v[0]),
        'The schedule makes %d begin calls in %d rounds.  Sorting the list by length first would bring the static'
        % (n_begin, len(rounds)),
        'batches to %d steps (ratio %.3f against the same schedule total).' % (padded_sorted, padded_sorted / total)]
print('\n'.join(out[-9:]), flush=True)
del gs, gd

# ---- 3. the cost of one begin ------------------------------------------------------------------
B = max(a.batch)
g = make_gen(B, a.begin_frames * hop)
mel = [torch.as_tensor(rng.standard_normal((a.begin_frames, Li)).astype(np.float32), device='cuda') for _ in range(B)]
gc = [1 + (37 * b) % arch['n_gc_category'] for b in range(B)] if arch['n_gc_embed'] else None
out += ['', '## One lbwn_gen_begin call: B = %d, mels of %d frames, device events around the call' % (B, a.begin_frames),
        '', '| streams begun | launches | microseconds |', '|---:|---:|---:|']
g.init_sessions()
up = 1 if g.lib.lbwn_lc_upsample_fused_ok(len(arch['lc_upsample']), (ctypes.c_int * 8)(*arch['lc_upsample']), Li,
                                          arch['n_lc_out']) else len(arch['lc_upsample'])
for n in (1, B):
    slots = list(range(n))
    ts = []
    for r in range(a.reps + 1):
        ms = events(lambda: g.begin(slots, mel[:n], gc_ids=gc[:n] if gc else None, keys=slots))
        if r:
            ts.append(1e3 * ms)
    m = med(ts)
    out.append('| %d | %d | %.1f (%.1f .. %.1f) |' % ((n, 1 + n * up) + m))
    print(out[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, 'w').write('\n'.join(out) + '\n')
print('wrote', a.out)
