"""Numpy reference of the distilling / label-smoothing head (lbwn_train_forward_ex, include/lbwn.h).

``head`` follows the header's formulas with the ``score`` conventions of tests/eval_ref.py: row t is
scored against wav_q[:, t+1] iff ids[:, t+1] != 0, t = T-1 never.  In float64 it is the reference; with
``dtype=np.float32`` every operation runs in float32 (the "twin"): what the formulas give in the
kernel's number format, with numpy's summation order and exp.  The GPU tests hold the kernel to 8x the
twin's own error against float64 (the margin tests/test_gpu_mel.py gives a kernel over its numpy twin).
Archs and data come from eval_ref.case."""
import numpy as np

from tests import eval_ref as E


def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    d = x - m
    return d - np.log(np.exp(d).sum(axis=-1, keepdims=True))


def head(logits, teacher, wav_q, ids, alpha, temp, eps, dtype=np.float64):
    """(value [B, T], dlogits [B, T, Q], stats [4], stats_ex [4]) in ``dtype``; see ``_head``."""
    return _head(logits, teacher, wav_q, ids, alpha, temp, eps, dtype)[:4]


def _sum_orders(x, f):
    """A sum of the 1-d array x formed in ``f`` in three orders: numpy's own (pairwise), first to last,
    last to first."""
    fwd = f(0)
    for v in x:
        fwd = f(fwd + v)
    rev = f(0)
    for v in x[::-1]:
        rev = f(rev + v)
    return np.array([x.sum(dtype=f), fwd, rev], np.float64)


def _head(logits, teacher, wav_q, ids, alpha, temp, eps, dtype):
    """``head``'s (value [B, T], dlogits [B, T, Q], stats [4], stats_ex [4]) in ``dtype``.  ``teacher`` may be None
    when alpha == 0.  stats = (Σ value, count, Σ|argmax - c|, 1/count); stats_ex = (Σ plain xent, Σ kl, 0, 0);
    the sums over the scored rows are formed in ``dtype`` like everything else; a fifth item holds the
    three sums in three summation orders (see ``twin``)."""
    f = dtype
    l = np.asarray(logits, f)
    B, T, Q = l.shape
    alpha, temp, eps = f(alpha), f(temp), f(eps)
    one = f(1)
    tgt = np.zeros((B, T), np.int64)
    tgt[:, :-1] = wav_q[:, 1:]
    scored = np.zeros((B, T), bool)
    scored[:, :-1] = ids[:, 1:] != 0
    q = np.full((B, T, Q), eps / f(Q), f)
    np.put_along_axis(q, tgt[..., None], np.take_along_axis(q, tgt[..., None], axis=2) + (one - eps), axis=2)
    logp = _log_softmax(l)
    p = np.exp(logp)
    onehot = np.zeros((B, T, Q), f)
    np.put_along_axis(onehot, tgt[..., None], one, axis=2)
    xent = -(onehot * logp).sum(axis=2)
    hard = -(q * logp).sum(axis=2)               # lse(l) - Σ q·l, as Σ q = 1
    value = (one - alpha) * hard
    dl = (one - alpha) * (p - q)
    kl = np.zeros((B, T), f)
    if alpha != 0:
        u = np.asarray(teacher, f)
        logps, logpt = _log_softmax(l / temp), _log_softmax(u / temp)
        ps, pt = np.exp(logps), np.exp(logpt)
        terms = np.where(pt > 0, pt * (logpt - logps), f(0))       # pT_k = 0 contributes 0
        kl = terms.sum(axis=2).astype(f)
        value = value + alpha * temp * temp * kl
        dl = dl + alpha * temp * (ps - pt)
    value = np.where(scored, value, f(0)).astype(f)
    dl = np.where(scored[..., None], dl, f(0)).astype(f)
    am = np.argmax(l, axis=2)
    n = float(scored.sum())
    stats = np.array([value[scored].sum(dtype=f), n, np.abs(tgt - am)[scored].sum(), 1.0 / n if n else 0.0], np.float64)
    stats_ex = np.array([xent[scored].sum(dtype=f), kl[scored].sum(dtype=f), 0.0, 0.0], np.float64)
    orders = dict(stats0=_sum_orders(value[scored], f), ex0=_sum_orders(xent[scored], f), ex1=_sum_orders(kl[scored], f))
    return value, dl, stats, stats_ex, orders


def twin(logits, teacher, wav_q, ids, alpha, temp, eps):
    """``head`` evaluated in float32 on the float32 roundings of the same inputs, and a fifth item: the
    three sums (stats[0], stats_ex[0], stats_ex[1]) each formed in float32 in three orders (dict stats0,
    ex0, ex1 of float64 [3]).  A single float32 sum can land within a tenth of an ulp of the true value by
    the accident of its roundings; the order of a sum is what the kernel's margin over the twin is for, so
    the twin's error on a sum is the largest over its orders."""
    return _head(np.asarray(logits, np.float32), None if teacher is None else np.asarray(teacher, np.float32),
                 wav_q, ids, alpha, temp, eps, np.float32)


def q516_arch():
    """The generic head just past the register forms, inside the backward's n_quant <= 1024."""
    return E._arch(Q=516)


def f32_params(P):
    """The float64 parameters rounded to what the device holds."""
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in P.items()}


def kernel_case(Q, B=2, T=9, seed=0):
    """Inputs of the kernel-alone test: logits and teacher N(0, 3²) [B, T, Q] as float32, targets that
    include code 0 and code Q-1, ids with a masked run, and one scored row whose teacher has a logit 200
    below the row maximum (its probability underflows to 0 in float32)."""
    rng = np.random.default_rng(1000 + Q + seed)
    lg = (3.0 * rng.standard_normal((B, T, Q))).astype(np.float32)
    te = (3.0 * rng.standard_normal((B, T, Q))).astype(np.float32)
    q = rng.integers(0, Q, size=(B, T)).astype(np.int32)
    q[0, 2], q[1, 3] = 0, Q - 1
    ids = np.ones((B, T), np.int32)
    ids[0, 4:6] = 0            # a masked run: rows t = 3, 4 of stream 0 are not scored
    ids[1, 0] = 0              # (row scoring looks at ids[:, t+1]: column 0 never matters)
    ids[1, T - 2] = 0
    te[0, 1, (Q // 2) % Q] = te[0, 1].max() - 200.0     # row (0, 1) is scored
    return lg, te, q, ids
