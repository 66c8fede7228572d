"""Time the log-mel front end (lbwn_mel_forward) on one hour of 16 kHz audio at the defaults
(n_fft 1024, hop 256, 80 mels: 225,000 frames), in one process.

GPU: hipEvents around `--launches` back-to-back launches after `--warmup`, repeated `--repeats` times;
the figure is the median repeat divided by the launches.  CPU (for scale only): the float32 numpy rfft
restatement of the same transform on this box's host, one pass over `--cpu-seconds` of audio scaled to
the hour.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))


def numpy_mel(x, fb, n_fft, hop, log_floor):
    """float32 numpy restatement with rfft (reflect padding, periodic Hann, power 2, ln floor)."""
    F = len(x) // hop
    pad = np.pad(x, n_fft // 2, mode='reflect')
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
    spec = np.fft.rfft(pad[idx] * w, axis=1)
    p = (spec.real.astype(np.float32) ** 2 + spec.imag.astype(np.float32) ** 2)
    return np.log(np.maximum(p @ fb, np.float32(log_floor)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cpu-seconds', type=float, default=60.0)
    args = ap.parse_args()
    import torch
    from lbwn.mel import MelSpectrogram
    sr, hop, n_mels, n_fft = 16000, 256, 80, 1024
    n = int(args.seconds * sr)
    ms = MelSpectrogram(sr, hop, n_mels)
    F = ms.frames(n)
    rng = np.random.default_rng(0)
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    wav = torch.from_numpy(x).cuda()[None].contiguous()
    out = torch.empty(1, F * n_mels, device='cuda')
    for _ in range(args.warmup):
        ms.forward_into(wav, out)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            ms.forward_into(wav, out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / args.launches)
    us = float(np.median(times))
    nbins = n_fft // 2 + 1
    flop = 2.0 * F * n_fft * 2 * nbins + 2.0 * F * nbins * n_mels          # DFT (re and im) + filterbank
    res = dict(what='lbwn_mel_forward', seconds=args.seconds, frames=F, us=us, us_min=float(min(times)),
               us_max=float(max(times)), launches=args.launches, repeats=args.repeats,
               tflops=flop / us * 1e-6, frac_of_157_tflops=flop / us * 1e-6 / 157.0,
               device=torch.cuda.get_device_name(0))
    # the first frames against the numpy restatement, as a sanity check of what was timed
    m = min(n, int(args.cpu_seconds * sr))
    fb = ms.filterbank()
    t0 = time.perf_counter()
    ref = numpy_mel(x[:m], fb, n_fft, hop, 1e-5)
    cpu_s = time.perf_counter() - t0
    got = out.view(F, n_mels)[:ref.shape[0] - 4].cpu().numpy()
    res['max_abs_log_diff_vs_numpy_f32'] = float(np.abs(got - ref[:got.shape[0]]).max())
    res['cpu_numpy_rfft_us_scaled'] = cpu_s * 1e6 * (n / m)
    res['cpu_numpy_seconds_measured'] = m / sr
    print(json.dumps(res))


if __name__ == '__main__':
    main()
