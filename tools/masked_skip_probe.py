"""Per-launch times of the six products the masked-position skip touches (dh, ds, dz, dpost2,
dpost1, dskip; lbwn_plan_probe event pairs) at C2 (arch3, B=8 x T=4096) on chosen entries of the
benchmark's slice ring, with each entry's share of valid rows and live 256-row tiles / 32-row
k-steps.  One JSON line.  A/B: run it under tools/with_lib.py with a variant build, or with
LBWN_SKIP_MASKED=0.

    python tools/masked_skip_probe.py [--entries 0,1,2,3] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
sys.path.insert(0, ROOT)

NAMES = ['dh', 'ds', 'dz', 'dpost2', 'dpost1', 'dskip']


def live_shares(ids):
    B, T = ids.shape
    M = B * T
    flat = ids.reshape(-1)
    m = np.arange(M)
    valid = (m % T != T - 1) & (flat[np.minimum(m + 1, M - 1)] != 0)
    return {'valid_rows': float(valid.mean()), 'live_tiles_256': float(valid.reshape(-1, 256).any(axis=1).mean()),
            'live_ksteps_32': float(valid.reshape(-1, 32).any(axis=1).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--entries', default='0,1,2,3')
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    from lbwn import dist as lbdist
    from lbwn.arch import load_arch
    arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    tb = bench.TrainBench(arch, 8, 4096, lbdist.init())
    for i in range(8):
        tb.step(i)
    torch.cuda.synchronize()
    out = {'skip_masked_env': os.environ.get('LBWN_SKIP_MASKED'), 'entries': {}, 'us': {}}
    for e in (int(x) for x in args.entries.split(',')):
        out['entries'][e] = live_shares(tb.ring[e][2].cpu().numpy())
        for name in NAMES:
            ts = []
            for _ in range(args.reps):
                s, t = tb.probe(name)
                tb.step(e)
                torch.cuda.synchronize()
                ts.append(round(s.elapsed_time(t) * 1e3, 1))
            out['us'].setdefault(name, {})[e] = ts
    tb.net.check_status(tb.T)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
