"""State save / load / fan-out prefill of the cached generator, timed with device events
around the call alone, after one warm-up, as the median of --reps runs.

Copy rate: lbwn_gen_state_save and lbwn_gen_state_load (identity map) at --arch (arch3) for each --batch,
beside a hipMemcpyAsync device-to-device of the snapshot's byte count in the same run -- the yardstick;
there is no pass bar.  A save reads the rings and writes the snapshot, a load reads the snapshot and
writes the rings and zeroes the hand-off granules, the memcpy reads and writes the same bytes once each;
the rate column counts the snapshot's bytes once (copied bytes per second), for all three alike.

Fan-out prefill: --n codes at --fan-batch streams, init_buffers(prefill='fanout') against
init_buffers(prefill=True) of the same generator (both include lbwn_gen_start): the arch as shipped (no
GC: one voice), and the arch with a GC embedding added (--gc-embed / --gc-category) with one and with two
distinct voice ids.  Writes a markdown report to --out.  No test asserts these times."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--arch', default=os.path.join(ROOT, 'par', 'arch3.json'))
ap.add_argument('--batch', type=int, nargs='+', default=[10, 80])
ap.add_argument('--n', type=int, default=48000, help='prompt length of the fan-out part')
ap.add_argument('--fan-batch', type=int, default=80)
ap.add_argument('--gc-embed', type=int, default=32)
ap.add_argument('--gc-category', type=int, default=8)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--no-fanout', action='store_true', help='the copy rates only')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_gen_state.md'))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn import _lib  # noqa: E402
from lbwn.arch import load_arch, normalize_arch  # noqa: E402
from lbwn.imodel import WaveNetGen  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

assert torch.cuda.is_available(), 'needs an MI355X'


def hip_runtime():
    """The HIP runtime this process already has (torch's), not a second copy: by its mapped path."""
    for line in open('/proc/self/maps'):
        path = line.split()[-1]
        if 'libamdhip64' in os.path.basename(path):
            return ctypes.CDLL(path)
    return None


hip = hip_runtime()
if hip is not None:
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]


def memcpy_d2d(dst, src):
    if hip is None:
        dst.copy_(src)          # torch's contiguous same-dtype device copy is the same call
        return
    err = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, _lib.stream_ptr())   # 3: device to device
    assert err == 0, err


def timed(fn, reset=lambda: None):
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


def make_gen(arch, net, B, max_steps, teacher=None):
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, 1000, None, seed=1)
    g.load_params(net)
    g.teacher_mu = teacher
    g.build_graph(max_steps)
    return g


arch = load_arch(a.arch)
assert arch['n_lc_out'] == 0, 'an arch without local conditioning, please'
net = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)
fmt = lambda t: '%.3f (%.3f .. %.3f)' % t   # noqa: E731
out = ['# State save / load and fan-out prefill of the cached generator (%s)' % os.path.basename(a.arch), '',
       'Device events around the call, one warm-up, median of %d (min .. max).  The repetitions copy the same' % a.reps,
       'buffers, so from the second one on the bytes may be served by the 256 MB last-level cache; the memcpy',
       'beside them runs under the same condition.', '',
       '## Copy rate', '',
       'GB/s = the snapshot\'s bytes once over the median time (each call reads and writes them once).  memcpy = %s'
       % ('hipMemcpyAsync, device to device, of the same byte count' if hip is not None else 'torch copy_ (device to device)'),
       '', '| B | snapshot MB | form | save us | GB/s | load us | GB/s | memcpy us | GB/s | save / memcpy | load / memcpy | granules zeroed by a load MB |',
       '|---:|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|']
for B in a.batch:
    gc = list(range(1, B + 1)) if arch['n_gc_embed'] else None
    g = make_gen(arch, net, B, 64)
    g.init_buffers(gc)
    g.step(8)
    nb = g.lib.lbwn_gen_state_bytes(g._plan, B)
    blob, blob2 = (torch.empty(nb, dtype=torch.uint8, device='cuda') for _ in range(2))
    ws, st = g._ws.data_ptr(), _lib.stream_ptr()
    sv = timed(lambda: _lib.check(g.lib.lbwn_gen_state_save(g._plan, ws, blob.data_ptr(), st)))
    ld = timed(lambda: _lib.check(g.lib.lbwn_gen_state_load(g._plan, ws, blob.data_ptr(), B, None, st)))
    mc = timed(lambda: memcpy_d2d(blob2, blob))
    g.check_status()
    assert torch.equal(blob, blob2)
    L, Cs, Q = arch['n_blocks'] * arch['n_block_layers'], arch['n_skip'], arch['n_quant']
    gran = 8 * (B * L * 32 + B * Cs + 32 * B * Q)
    rate = lambda t: nb / (t[0] * 1e-3) / 1e9   # noqa: E731
    us = lambda t: '%.1f (%.1f .. %.1f)' % tuple(1e3 * v for v in t)   # noqa: E731
    out.append('| %d | %.2f | %s | %s | %.0f | %s | %.0f | %s | %.0f | %.2f | %.2f | %.2f |' % (
        B, nb / 1e6, 'persistent' if g.persistent else 'per step', us(sv), rate(sv), us(ld), rate(ld), us(mc),
        rate(mc), sv[0] / mc[0], ld[0] / mc[0], gran / 1e6))
    print('B=%d %.2f MB: save %.4f ms, load %.4f ms, memcpy %.4f ms' % (B, nb / 1e6, sv[0], ld[0], mc[0]), flush=True)
    del g, blob, blob2

if not a.no_fanout:
    B, n = a.fan_batch, a.n
    codes = torch.as_tensor(np.random.default_rng(n).integers(0, arch['n_quant'], n).astype(np.int32), device='cuda')
    out += ['', '## Fan-out prefill: %d codes, %d streams' % (n, B), '',
            "init_buffers(prefill=...) whole: lbwn_gen_start, then the prefill of all streams (True) or of the distinct",
            "voices in the private generator, its save and the load into the %d streams ('fanout')." % B, '',
            "| arch | distinct voice ids | prefill=True ms | prefill='fanout' ms | ratio |", '|---|---:|---:|---:|---:|']
    arch_gc = normalize_arch(dict(arch, n_gc_embed=a.gc_embed, n_gc_category=a.gc_category))
    net_gc = WaveNetTrain(**arch_gc, batch_sz=1, l2_factor=0.0, print_interval=0, seed=0)
    cases = [('as shipped (no GC)', arch, net, None, 1),
             ('GC %d / %d' % (a.gc_embed, a.gc_category), arch_gc, net_gc, [1] * B, 1),
             ('GC %d / %d' % (a.gc_embed, a.gc_category), arch_gc, net_gc, [1 + b % 2 for b in range(B)], 2)]
    for name, ar, nt, ids, nv in cases:
        g = make_gen(ar, nt, B, n, teacher=codes)
        full = timed(lambda: g.init_buffers(ids, prefill=True))
        fan = timed(lambda: g.init_buffers(ids, prefill='fanout'))
        assert int(g.tensor('step', torch.int64).item()) == n
        g.check_status()
        out.append('| %s | %d | %s | %s | %.1fx |' % (name, nv, fmt(full), fmt(fan), full[0] / fan[0]))
        print("%s, %d voice(s): prefill=True %.2f ms, 'fanout' %.2f ms" % (name, nv, full[0], fan[0]), flush=True)
        del g
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, 'w').write('\n'.join(out) + '\n')
print('wrote', a.out)
