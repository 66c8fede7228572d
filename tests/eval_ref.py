"""Float64 reference of the held-out evaluation (lbwn_train_eval) and the inputs its tests share.

``score`` takes logits (oracle.wavenet_ref.forward's, or any [B, T, Q] array) and forms, in numpy,
what include/lbwn.h defines: per position the log-softmax gather in nats (0 where not scored), the
first-max argmax, the four totals and the per-voice sums.  ``run`` chains oracle forwards over
consecutive slices with SAVE carried.  ``case`` builds the configurations of tests/test_gpu_eval.py
(tests/test_eval.py checks on the CPU, with the oracle alone, the property their argmax comparison
rests on: the share of rows whose top-2 logit gap is below 1e-3)."""
import numpy as np

from lbwn.arch import normalize_arch
from oracle import wavenet_ref as R

N_BINS = 4      # voice ids run 1..5: 4 and 5 are >= N_BINS and must land in bin 0


def score(logits, wav_q, ids, n_bins=None):
    """dict(nll [B,T], scored [B,T] bool, argmax [B,T], gap [B,T] (top-2 logit gap), acc float64[4],
    by_voice float64 [n_bins, 2] or None).  Row t is scored against wav_q[:, t+1] iff ids[:, t+1] != 0."""
    lg = np.asarray(logits, np.float64)
    B, T, Q = lg.shape
    tgt = np.zeros((B, T), np.int64)
    tgt[:, :-1] = wav_q[:, 1:]
    scored = np.zeros((B, T), bool)
    scored[:, :-1] = ids[:, 1:] != 0
    m = lg.max(axis=2)
    lse = m + np.log(np.exp(lg - m[..., None]).sum(axis=2))
    picked = np.take_along_axis(lg, tgt[..., None], axis=2)[..., 0]
    nll = np.where(scored, lse - picked, 0.0)
    am = np.argmax(lg, axis=2)                  # numpy returns the first maximum
    top2 = np.sort(lg, axis=2)[..., -2:]
    gap = top2[..., 1] - top2[..., 0]
    acc = np.array([nll.sum(), scored.sum(), np.abs(tgt - am)[scored].sum(), (tgt == am)[scored].sum()], np.float64)
    bv = None
    if n_bins is not None:
        vid = np.zeros((B, T), np.int64)
        vid[:, :-1] = ids[:, 1:]
        bins = np.where((vid >= 0) & (vid < n_bins), vid, 0)
        bv = np.zeros((n_bins, 2), np.float64)
        np.add.at(bv[:, 0], bins[scored], nll[scored])
        np.add.at(bv[:, 1], bins[scored], 1.0)
    return dict(nll=nll, scored=scored, argmax=am, gap=gap, tgt=tgt, acc=acc, by_voice=bv)


def run(arch, P, slices, save, n_bins=None):
    """Oracle forwards over consecutive (q, ids, mel) slices with SAVE carried; returns the list of
    per-slice ``score`` dicts (each with its 'logits') and the final SAVE."""
    out = []
    for q, ids, mel in slices:
        lg, _, save = R.forward(arch, P, q, ids, save, mel=mel)
        s = score(lg, q, ids, n_bins)
        s['logits'] = lg
        out.append(s)
    return out, save


def totals(scores):
    acc = sum(s['acc'] for s in scores)
    bv = sum(s['by_voice'] for s in scores) if scores[0]['by_voice'] is not None else None
    return acc, bv


# ---- the configurations (2 blocks x 3 layers) -------------------------------------------------------
def _arch(Cr=32, Cd=32, Cs=64, Cp=32, Q=256, use_bias=True, cond=False):
    a = dict(n_blocks=2, n_block_layers=3, n_quant=Q, n_res=Cr, n_dil=Cd, n_skip=Cs, n_post=Cp, n_gc_embed=0,
             n_gc_category=0, use_bias=use_bias)
    if cond:
        a.update(n_gc_embed=4, n_gc_category=5, n_lc_in=4, n_lc_out=4, lc_upsample=[2, 2])
    return normalize_arch(a)


ARCHS = {
    'chain': lambda: _arch(),
    'per_layer': lambda: _arch(Cr=3, Cd=4, Cs=6, Cp=5),        # the padded head
    'cond': lambda: _arch(cond=True),
    'no_bias': lambda: _arch(use_bias=False),
    'q64': lambda: _arch(Q=64),
    'q260': lambda: _arch(Q=260),                             # a partial last 64-column group
    'q1028': lambda: _arch(Q=1028),                           # the generic row kernel (n_quant > 512)
}


# The data seed of each configuration.  The argmax totals are compared on rows whose float64 top-2 logit
# gap exceeds 1e-3, and at most 5 % of the scored rows may fall below it: a condition on the case, not
# on the kernels (tests/test_eval.py::test_top2_gap_shares holds it on the CPU), so a configuration
# whose logits are small takes the seed that meets it: without biases the logits stay within 0.16 and
# one seed in forty does.
DATA_SEED = {'per_layer': 4, 'no_bias': 62}


def case(name, B=2, T=64, n_slices=1, invalid=13, pseed=0):
    """(arch, P, S, slices): parameters R.init_params(default_rng(pseed), bias_scale=0.5), SAVE
    R.init_save, uniform codes, ids masked over the first ``invalid`` columns of the deal and runs of
    voice ids 1..5 after (with one masked run inside), mel N(0, 1) for the LC arch."""
    arch = ARCHS[name]()
    P = R.init_params(arch, np.random.default_rng(pseed), bias_scale=0.5)
    S = R.init_save(arch, B, np.random.default_rng(1))
    rng = np.random.default_rng(DATA_SEED.get(name, 2))
    n = T * n_slices
    q = rng.integers(0, arch['n_quant'], size=(B, n)).astype(np.int32)
    ids = np.zeros((B, n), np.int32)
    for b in range(B):
        t = invalid
        while t < n:
            run_len = int(rng.integers(1, 12))
            ids[b, t:t + run_len] = int(rng.integers(1, 6))
            t += run_len
        if n >= 40:
            ids[b, 30 + b:30 + b + 5] = 0
    mel = None
    if arch['n_lc_out'] > 0:
        hop = int(np.prod(arch['lc_upsample']))
        mel = rng.standard_normal((B, n // hop, arch['n_lc_in'])).astype(np.float32)
    slices = []
    for k in range(n_slices):
        hop = int(np.prod(arch['lc_upsample'])) if mel is not None else 1
        slices.append((q[:, k * T:(k + 1) * T], ids[:, k * T:(k + 1) * T],
                       mel[:, k * T // hop:(k + 1) * T // hop] if mel is not None else None))
    return arch, P, S, slices
