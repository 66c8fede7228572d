"""The cost of distillation and label smoothing (lbwn_train_forward_ex) at B x T, per
student arch (default: arch3, and the 2 x 10-layer arch3_student) with an arch3 teacher, in one process:

  head    the "head" probe (lbwn_plan_probe) of the plain head, the smoothing-only head and the distilling
          head at tau = 1 and tau = 2, each beside the bytes it moves over its time (the logits read and
          written, the teacher's rows read: 2·M·Q·4, or about 3·M·Q·4 with a teacher);
  step    forward + backward: plain, against teacher logits that are already there, and Distiller.step
          (the teacher's eval_slice included);
  neutral lbwn_train_forward_ex with no option active against lbwn_train_forward (forward only).

The forms of a group alternate in one loop; each sample is device events around --launches calls of one
form (the head: one probe per call); after a warm-up round the median of --reps samples is reported with
min .. max and the spread (max - min) / median.  --plain-only times lbwn_train_forward alone: run it under
tools/with_lib.py with the parent revision's library for the same-box comparison.  Prints a markdown table
and, with --out, appends it to that file.  No test asserts these times."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--student', nargs='+', default=['arch3', 'arch3_student'])
ap.add_argument('--teacher', default='arch3')
ap.add_argument('-B', type=int, default=8)
ap.add_argument('-T', type=int, default=4096)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--plain-only', action='store_true')
ap.add_argument('--out', default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbwn import _lib  # noqa: E402
from lbwn.arch import load_arch  # noqa: E402
from lbwn.tmodel import WaveNetTrain  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('distill_bench: no GPU found (needs an MI355X)')
B, T = a.B, a.T


def make(name):
    arch = load_arch(os.path.join(ROOT, 'par', name + '.json'))
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=0.0, print_interval=0, seed=0)
    net.init_vars(0, bias_scale=0.1)
    return net


def sample_ms(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def head_ms(net, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    e.record()
    _lib.check(net.lib.lbwn_plan_probe(net._plan(T), b'head', s.cuda_event, e.cuda_event))
    fn()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def group(forms, sampler):
    """forms: [(label, fn)]; alternating, one warm-up round; returns [(label, median, min, max)]."""
    ms = [[] for _ in forms]
    for r in range(a.reps + 1):
        for i, (_, fn) in enumerate(forms):
            t = sampler(fn)
            if r:
                ms[i].append(t)
    return [(forms[i][0], statistics.median(m), min(m), max(m)) for i, m in enumerate(ms)]


rng = np.random.default_rng(0)
q = torch.as_tensor(rng.integers(0, 256, (B, T)).astype(np.int32), device='cuda')
ids = np.ones((B, T), np.int32)
ids[:, :T // 4] = 0                           # the invalid windows at a stream's start
ids = torch.as_tensor(ids, device='cuda')
md = []
for name in a.student:
    net = make(name)
    Q, M = net.n_quant, B * T
    plain = lambda bw=False: net.forward(q, None, ids, backward=bw)   # noqa: E731
    if a.plain_only:
        (r,) = group([('lbwn_train_forward', plain)], lambda fn: sample_ms(fn, a.launches))
        print('%s lbwn_train_forward %.1f us (%.1f .. %.1f), spread %.2f %%' % (
            name, r[1] * 1e3, r[2] * 1e3, r[3] * 1e3, 100 * (r[3] - r[2]) / r[1]), flush=True)
        del net
        continue
    from lbwn.distill import Distiller
    teacher = make(a.teacher)
    teacher.init_vars(1, bias_scale=0.1)
    st = teacher.eval_state()
    teacher.eval_slice(st, q, None, ids)
    tl = teacher.logits_view(T).clone()          # teacher logits that are already there
    dist = Distiller(net, teacher, 0.5, 2.0)

    def ex(alpha, temp, eps, bw=False):
        return lambda: net.forward(q, None, ids, backward=bw, teacher_logits=tl if alpha else None,
                                   distill_alpha=alpha, distill_temp=temp, label_smoothing=eps)

    def neutral():
        arg = _lib.ForwardArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=None, save=net.save_flat.data_ptr(),
                               stats=net.stats.data_ptr(), stats_ex=None, teacher_logits=None, ld_teacher=0,
                               distill_alpha=0.0, distill_temp=1.0, label_smoothing=0.0)
        _lib.check(net.lib.lbwn_train_forward_ex(net._plan(T), ctypes.byref(net._params_c), net._ws.data_ptr(),
                                                 ctypes.byref(arg), _lib.stream_ptr()))

    def dstep():
        dist.step(q, None, ids, backward=True)

    heads = group([('plain head', plain), ('smoothing only (0, 1, 0.1)', ex(0.0, 1.0, 0.1)),
                   ('distilling, tau = 1 (0.5, 1, 0)', ex(0.5, 1.0, 0.0)), ('distilling, tau = 2 (0.5, 2, 0.1)', ex(0.5, 2.0, 0.1))],
                  lambda fn: head_ms(net, fn))
    steps = group([('step, plain', lambda: plain(True)), ('step, teacher logits given (0.5, 2, 0)', ex(0.5, 2.0, 0.0, True)),
                   ('step, Distiller.step (teacher eval_slice included)', dstep)], lambda fn: sample_ms(fn, a.launches))
    neut = group([('lbwn_train_forward', plain), ('lbwn_train_forward_ex, no option active', neutral)],
                 lambda fn: sample_ms(fn, a.launches))
    assert net.status(T) == 0 and dist.teacher_status() == 0
    md += ['', '## student %s, teacher %s (B = %d, T = %d)' % (name, a.teacher, B, T), '',
           '| form | us | min .. max | spread | GB/s |', '|---|---:|---:|---:|---:|']
    for k, (label, med, lo, hi) in enumerate(heads + steps + neut):
        nbytes = (2 + (1 if 'distilling' in label else 0)) * M * Q * 4 if k < len(heads) else None
        md.append('| %s | %.1f | %.1f .. %.1f | %.2f %% | %s |' % (
            label, med * 1e3, lo * 1e3, hi * 1e3, 100 * (hi - lo) / med, '%.0f' % (nbytes / med / 1e6) if nbytes else ''))
        print(md[-1], flush=True)
    del dist, teacher, net

if md:
    md = ['# Distillation and label smoothing: head, step and neutral path', '',
          'Median of %d samples after one warm-up round, forms of a group alternating; head rows: one "head" probe per' % a.reps,
          'sample; the other rows: device events around %d calls.' % a.launches] + md
    print('\n'.join(md), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(md) + '\n')
        print('wrote', a.out)
