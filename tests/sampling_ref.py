"""Float64 reference of the generator's filtered draw (lbwn_gen_set_sampling, include/lbwn.h) and the
inputs the sampling tests share.  A helper module, not a test.

The definition, restated with sort and cumsum.  With l a stream's logits at a step:
  1. top_k (0 = off, >= Q = off): keep the codes whose logit is >= the k-th largest; ties kept.
  2. temperature T: e_c = exp((l_c - max l) / T) for kept codes, 0 otherwise.
  3. top_p (1 = off), after top-k: order the kept codes by e, descending; keep the shortest prefix whose
     mass is >= p·Σe plus every code whose e equals that prefix's last member; all others get e = 0.
  4. the draw: the first code, in code order, with cumsum(e) > u·Σe.
"""
import numpy as np

from oracle import wavenet_ref as R

K_TOL = 1e-4      # x max|lg|: the atol the generator's logits are held to (tests/test_gpu_gen.py)
CDF_TOL = 5e-5    # x Σe: _near_tie of tests/test_gpu_gen.py

S_ALL = [(0.7, 0, 1.0), (1.5, 0, 1.0), (1.0, 8, 1.0), (1.0, 1, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95)]
S_SUB = [(1.0, 8, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95)]
POST2_SCALE = {256: 30.0, 100: 10.0, 300: 30.0}
SEED = 7


def small(Q=256, gc=0, use_bias=True):
    """The small arch of tests/test_gpu_gen.py with n_quant = Q."""
    from lbwn.arch import normalize_arch
    return normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=Q, n_res=32, n_dil=32, n_skip=64,
                               n_post=32, n_gc_embed=8 if gc else 0, n_gc_category=gc, use_bias=use_bias))


_PARAMS = {}


def host_params(arch, scale):
    """({name: float32 array} for load_params, the same values as float64 for the oracle): R.init_params
    with default_rng(3) and bias_scale 0.2, rounded to float32, POST2 multiplied (in float32) by scale.
    Computed once per (arch, scale) and shared; callers must not modify them."""
    key = (repr(sorted((k, repr(v)) for k, v in arch.items())), float(scale))
    if key not in _PARAMS:
        P = R.init_params(arch, np.random.default_rng(3), bias_scale=0.2)
        P32 = {n: np.asarray(v, np.float32) for n, v in P.items()}
        P32['POST2'] = P32['POST2'] * np.float32(scale)
        _PARAMS[key] = (P32, {n: v.astype(np.float64) for n, v in P32.items()})
    return _PARAMS[key]


def _norm_k(k, Q):
    return 0 if k >= Q else int(k)


def _topk_keep(lg, k):
    k = _norm_k(k, len(lg))
    if k == 0:
        return np.ones(len(lg), bool)
    kth = np.sort(lg)[::-1][k - 1]
    return lg >= kth


def _e_before_top_p(lg, T, k):
    keep = _topk_keep(lg, k)
    return keep, np.where(keep, np.exp((lg - lg.max()) / T), 0.0)


def keep_and_e(lg, T, k, p):
    """(keep bool[Q], e float64[Q]) of one logits row after top-k, temperature and top-p."""
    lg = np.asarray(lg, np.float64)
    keep, e = _e_before_top_p(lg, T, k)
    if p < 1:
        order = np.argsort(-e, kind='stable')
        order = order[keep[order]]
        cs = np.cumsum(e[order])
        m = int(np.argmax(cs >= p * cs[-1]))          # the shortest prefix: its last member is order[m]
        keep = keep & (e >= e[order[m]])
        e = np.where(keep, e, 0.0)
    return keep, e


def ref_draw(lg, u, T, k, p):
    """The filtered draw of one row: the first code with cumsum(e) > u·Σe ((1, 0, 1): exactly
    R.sample_from_logits)."""
    _, e = keep_and_e(lg, T, k, p)
    c = np.cumsum(e)
    return min(int(np.searchsorted(c, u * c[-1], side='right')), len(e) - 1)


def flags(lg, u, T, k, p):
    """The near-tie predicates of one draw, a set of:
    'k'  the k-th and (k+1)-th largest logits differ by <= 1e-4·max|lg|: fp32 logits may order them
         the other way, so the top-k set may gain or lose a code;
    'p'  some descending-prefix mass lies within 5e-5·Σe of p·Σe: the nucleus may end one code
         earlier or later;
    'c'  u·Σe lies within 5e-5·Σe of a boundary of the filtered CDF (_near_tie of test_gpu_gen.py
         applied to the filtered e)."""
    lg = np.asarray(lg, np.float64)
    out = set()
    kk = _norm_k(k, len(lg))
    if kk > 0:
        s = np.sort(lg)[::-1]
        if s[kk - 1] - s[kk] <= K_TOL * np.abs(lg).max():
            out.add('k')
    if p < 1:
        _, e0 = _e_before_top_p(lg, T, k)
        cs = np.cumsum(np.sort(e0)[::-1])
        if np.min(np.abs(cs - p * cs[-1])) <= CDF_TOL * cs[-1]:
            out.add('p')
    _, e = keep_and_e(lg, T, k, p)
    c = np.cumsum(e)
    if np.min(np.abs(c - u * c[-1])) <= CDF_TOL * c[-1]:
        out.add('c')
    return out


def filtered_generate(monkeypatch, arch, P, B, n, setting, **kw):
    """R.generate(..., return_logits=True) whose every draw is the filtered reference."""
    T, k, p = setting
    with monkeypatch.context() as m:
        m.setattr(R, 'sample_from_logits', lambda row, u: ref_draw(row, u, T, k, p))
        return R.generate(arch, P, B, n, seed=SEED, return_logits=True, **kw)


def check_draws(got, lg, setting, seed=SEED, t0=0, label=''):
    """The common check of the GPU tests: got int[B, n] against the float64 logits lg [B, n, Q] each
    draw was taken from.  Returns the number of differing draws after asserting that
      - every differing draw carries a flag, and at most 2 differ;
      - every draw, with no exception, lies in the reference's kept set up to the logits' tolerance:
        its float64 logit is >= the smallest kept logit - 1e-4·max|lg| (where the draw is flagged
        'k' or 'p': >= the next logit below the kept set, same tolerance)."""
    T, k, p = setting
    B, n = got.shape
    bad, unflagged = [], []
    for b in range(B):
        for i in range(n):
            row, u = lg[b, i], R.philox_uniform(seed, b, t0 + i)
            keep, _ = keep_and_e(row, T, k, p)
            f = flags(row, u, T, k, p)
            tol = K_TOL * np.abs(row).max()
            floor = row[keep].min()
            if f & {'k', 'p'}:
                below = row[row < floor]
                if below.size:
                    floor = below.max()
            assert row[got[b, i]] >= floor - tol, \
                '%s draw (%d, %d) = %d has logit %.6f below the kept set (floor %.6f, flags %s)' % (
                    label, b, i, got[b, i], row[got[b, i]], floor, sorted(f))
            if got[b, i] != ref_draw(row, u, T, k, p):
                bad.append((b, i))
                if not f:
                    unflagged.append((b, i))
    print('%s setting %s: draws %d, differing %d, max |logit| %.3f' % (label, setting, got.size, len(bad),
                                                                     np.abs(lg).max()))
    assert not unflagged, '%s draws differ away from any near tie at (stream, step) %s' % (label, unflagged[:8])
    assert len(bad) <= 2, (label, bad)
    return len(bad)
