"""One comparison for every gradient in the suite: against the reference tensor's OWN max, no floor.

The gradients compared are those of the mean loss; none comes near 1, so a bar scaled by
max(1, max|ref|) is an absolute bar, and at 2e-4 it is 2 % .. 300 % of the small tensors' own
scale (tests/test_gradcheck.py shows what that lets through).  grad_close applies the project's
2e-4 to each tensor's own scale; adopt_relu_signs takes the one property of the function that
would otherwise break such a bar -- a relu mask that flips on fp32 noise -- out of the comparison,
counted and capped.  The cases (archs, batches) the CPU proof and the GPU tests share live here too."""
import numpy as np

from lbwn.arch import normalize_arch
from oracle import wavenet_ref as R

GRAD_REL = 2e-4          # the project's gradient bar, of each tensor's own max
S_TIE, H1_TIE = 1e-5, 2e-5   # the forward bars the suite asserts on the skip sum s and on r2
ADOPT_CAP = 5e-4         # at most 0.05 % of the elements of S, and of h1, may be relu ties


def err_stats(ours, ref):
    """(max|ours - ref|, max|ref|, relative L2 error) in float64."""
    a = np.asarray(ours, np.float64)
    b = np.asarray(ref, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if not a.size:
        return 0.0, 0.0, 0.0
    err = float(np.max(np.abs(a - b)))
    own = float(np.max(np.abs(b)))
    nb = float(np.linalg.norm(b))
    l2 = float(np.linalg.norm(a - b)) / nb if nb else float(np.linalg.norm(a - b))
    return err, own, l2


def grad_close(ours, ref, name='', rel=GRAD_REL):
    """max|ours - ref| <= rel * max|ref|; a reference of exactly zero wants exactly zero.
    Returns max|ours - ref| / max|ref| (0 for a zero reference)."""
    err, own, l2 = err_stats(ours, ref)
    if own == 0.0:
        assert err == 0.0, '%s: reference is exactly zero, got max |value| %.3g' % (name, err)
        return 0.0
    assert np.all(np.isfinite(np.asarray(ours, np.float64))), '%s: not finite' % name
    assert err <= rel * own, ('%s: max err / own max %.3g > %.3g (max err %.3g, own max %.3g, rel L2 %.3g)'
                              % (name, err / own, rel, err, own, l2))
    return err / own


def old_close_accepts(ours, ref, rel=GRAD_REL):
    """The rule this module replaces: max|ours - ref| <= rel * max(1, max|ref|)."""
    err, own, _ = err_stats(ours, ref)
    return err <= rel * max(1.0, own)


def zero_where_ref_zero(ours, ref, name=''):
    """Masked rows and relu-off elements: exact zeros of the reference are exact zeros."""
    a, b = np.asarray(ours), np.asarray(ref)
    bad = (b == 0) & (a != 0)
    assert not bad.any(), '%s: %d elements non-zero where the reference is exactly zero (max %.3g)' % (
        name, int(bad.sum()), float(np.abs(a[bad]).max()))


def relu_ties(cache):
    """Boolean masks of the ambiguous elements of the oracle's S and h1: within the forward bars
    of zero, so the forward check does not pin their sign."""
    S, h1 = cache['S'], cache['h1']
    ts = S_TIE * max(1.0, float(np.abs(S).max()))
    th = H1_TIE * max(1.0, float(np.abs(h1).max()))
    return np.abs(S) <= ts, np.abs(h1) <= th, ts, th


def adopt_relu_signs(cache, gpu_s, gpu_r2):
    """For the ambiguous elements only, give the oracle's cache the relu signs of the path under
    test (its s and r2, any shape with the elements in [B][T][C] order): S takes that path's
    value, h1 +-its threshold by whether r2 > 0.  Every other element has the same sign on both
    sides whenever the forward check (s at 1e-5, r2 at 2e-5 of scale) passes.  Call before
    R.backward.  Returns the numbers adopted, (of S, of h1); cap them with adoption_capped."""
    aS, aH, ts, th = relu_ties(cache)
    s = np.asarray(gpu_s, np.float64).reshape(cache['S'].shape)
    r2 = np.asarray(gpu_r2, np.float64).reshape(cache['h1'].shape)
    S = cache['S'].copy()
    S[aS] = s[aS]
    h1 = cache['h1'].copy()
    h1[aH] = np.where(r2[aH] > 0, th, -th)
    cache['S'], cache['h1'] = S, h1
    return int(aS.sum()), int(aH.sum())


def adoption_capped(cache, adopted):
    """A condition, not a measurement: relu ties are rare, or the case needs another seed."""
    nS, nH = adopted
    assert nS <= ADOPT_CAP * cache['S'].size, 'relu ties in S: %d of %d' % (nS, cache['S'].size)
    assert nH <= ADOPT_CAP * cache['h1'].size, 'relu ties in h1: %d of %d' % (nH, cache['h1'].size)


# ---- the shared cases -------------------------------------------------------------------

def small_arch(nb=2, nbl=4, Cr=32, Cd=32, Cs=64, Cp=32, Q=256, use_bias=True):
    return normalize_arch(dict(n_blocks=nb, n_block_layers=nbl, n_quant=Q, n_res=Cr, n_dil=Cd, n_skip=Cs,
                               n_post=Cp, n_gc_embed=0, n_gc_category=0, use_bias=use_bias))


def cond_arch(gc, lc, C=32, Li=12, Lo=16, strides=(2, 4), n_blocks=1, n_block_layers=4, Ge=8, ncat=5,
              use_bias=True):
    a = dict(n_blocks=n_blocks, n_block_layers=n_block_layers, n_quant=256, n_res=C, n_dil=C, n_skip=64, n_post=32,
             n_gc_embed=Ge if gc else 0, n_gc_category=ncat if gc else 0, use_bias=use_bias)
    if lc:
        a.update(n_lc_in=Li, n_lc_out=Lo, lc_upsample=list(strides))
    return normalize_arch(a)


def arch3_no_bias():
    import os
    from lbwn.arch import load_arch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return normalize_arch(dict(load_arch(os.path.join(root, 'par', 'arch3.json')), use_bias=False))


def _nb(**kw):
    return lambda: small_arch(use_bias=False, **kw)


def _nbc(C):
    return lambda: cond_arch(1, 1, C, use_bias=False)


# The use_bias=False plans that tests/test_gpu_no_bias.py holds against float64, by name:
# (arch, B, T, masked head positions, parameter seed, conditioned).  tests/test_no_bias.py counts
# each one's relu ties on the CPU (adoption_capped is a condition on the case, not on the kernels): a
# case that passes the cap takes another seed here, never a wider cap.
NO_BIAS_CASES = {
    'small_2x256': (_nb(), 2, 256, 37, 0, False),
    'small_1x129': (_nb(), 1, 129, 37, 0, False),
    'small_5x333': (_nb(), 5, 333, 37, 0, False),
    'small_live_halo_2x256': (_nb(), 2, 256, 3, 0, False),
    'arch3_2x512': (arch3_no_bias, 2, 512, 37, 0, False),
    'arch3_2x96': (arch3_no_bias, 2, 96, 37, 0, False),
    'tall_2x4096': (_nb(nb=1, nbl=4), 2, 4096, 37, 0, False),
    'layers16_2x256': (_nb(Cr=16, Cd=16), 2, 256, 37, 0, False),
    # seed 7, not 0: with n_skip = 8 and no bias, seed 0 has 6 positions whose S is all <= 0, so their
    # h1 rows are exactly 0 (36 of 2400 elements count as ties; the cap is 1); seed 7 has none
    'arch2_widths_2x200': (_nb(Cr=3, Cd=4, Cs=8, Cp=6), 2, 200, 37, 7, False),
    'head_200_100_100': (_nb(nb=1, nbl=4, Cs=200, Cp=100, Q=100), 2, 200, 37, 0, False),
    'head_136_72_260': (_nb(nb=1, nbl=4, Cs=136, Cp=72, Q=260), 2, 200, 37, 0, False),
    'head_64_32_520': (_nb(nb=1, nbl=4, Cs=64, Cp=32, Q=520), 2, 200, 37, 0, False),
    'cond32_2x256': (_nbc(32), 2, 256, 37, 0, True),
    'cond32_3x136': (_nbc(32), 3, 136, 37, 0, True),
    'cond16_2x256': (_nbc(16), 2, 256, 37, 0, True),
}


def arch3_arch():
    import os
    from lbwn.arch import load_arch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return load_arch(os.path.join(root, 'par', 'arch3.json'))


def _sa(**kw):
    return lambda: small_arch(**kw)


def _ca(C, **kw):
    return lambda: cond_arch(1, 1, C, **kw)


def edge_invalid(T):
    """Masked head positions of an edge case: 37 as elsewhere, 1 where the slice is not longer than
    that, 0 at T < 4 so that n_valid >= 1."""
    return 37 if T > 37 else 1 if T >= 4 else 0


def _edge(prefix, mk, shapes, cond=False, seed=0):
    return {'%s_%dx%d' % (prefix, B, T): (mk, B, T, edge_invalid(T), seed, cond) for B, T in shapes}


# The ends of the depth and slice ranges lbwn_plan_create accepts (n_blocks >= 1, n_block_layers in
# 1..16, slice_sz >= 2, at least 4 positions) that tests/test_gpu_edge_shapes.py holds against
# float64, in the shape of NO_BIAS_CASES: (arch, B, T, masked head positions, parameter seed, conditioned).
# tests/test_edge_shapes.py counts each one's relu ties on the CPU; a case that passes the cap takes
# another seed here, never a wider cap.  L1*: one layer (the first is the last), H = 1.  L2*: two
# layers (the chains' min(l + 2, L - 1) prefetches).  tiny*: M = 4 .. 360, T below 4 / 16 / 32.
# deep*: n_block_layers 12 and 16 (d and H up to 32768).
EDGE_CASES = {}
EDGE_CASES.update(_edge('L1', _sa(nb=1, nbl=1), [(2, 256)]))
# seed 1, not 0: seed 0 has 4 of 8256 elements of S within the forward bar of zero, and the cap is 4.1
EDGE_CASES.update(_edge('L1', _sa(nb=1, nbl=1), [(1, 129)], seed=1))
EDGE_CASES.update(_edge('L2_d1', _sa(nb=2, nbl=1), [(2, 256)]))
EDGE_CASES.update(_edge('L2', _sa(nb=1, nbl=2), [(3, 200)]))
EDGE_CASES.update(_edge('L1_c16', _sa(nb=1, nbl=1, Cr=16, Cd=16), [(2, 256)]))
EDGE_CASES.update(_edge('L1_cond32', _ca(32, n_blocks=1, n_block_layers=1), [(2, 136)], cond=True))
EDGE_CASES.update(_edge('L2_cond32', _ca(32, n_blocks=2, n_block_layers=1), [(2, 136)], cond=True))
EDGE_CASES.update(_edge('L1_cond16', _ca(16, n_blocks=1, n_block_layers=1), [(2, 136)], cond=True))
# (2, 2) and (2, 3), not (1, 2) and (1, 3): lbwn_plan_create refuses fewer than 4 positions (include/lbwn.h)
EDGE_CASES.update(_edge('tiny', _sa(), [(2, 2), (2, 3), (3, 5), (2, 17), (7, 31), (40, 9)]))
EDGE_CASES.update(_edge('tiny_arch3', arch3_arch, [(2, 8)]))
EDGE_CASES.update(_edge('tiny_arch2w', _sa(Cr=3, Cd=4, Cs=8, Cp=6), [(3, 5)]))
EDGE_CASES.update(_edge('tiny_cond32', _ca(32), [(2, 8), (5, 16)], cond=True))
EDGE_CASES.update(_edge('tiny_cond16', _ca(16), [(3, 8)], cond=True))
EDGE_CASES.update(_edge('deep12', _sa(nb=1, nbl=12), [(2, 2200)]))
EDGE_CASES.update(_edge('deep12_c16', _sa(nb=1, nbl=12, Cr=16, Cd=16), [(2, 2200)]))
EDGE_CASES.update(_edge('deep16', _sa(nb=1, nbl=16), [(2, 300)]))


def rand_batch(arch, B, T, seed=0, invalid=37):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, arch['n_quant'], size=(B, T)).astype(np.int32)
    ids = np.ones((B, T), np.int32)
    ids[:, :invalid] = 0
    if B > 1:
        ids[1, T // 2:T // 2 + 11] = 0
    return q, ids


def cond_batch(arch, B, T, invalid=37):
    """rand_batch with, for GC archs, voice ids that change at "file" boundaries (0 = masked)
    and, for LC archs, a mel input of T / hop frames."""
    q, ids = rand_batch(arch, B, T, invalid=invalid)
    rng = np.random.default_rng(3)
    if arch['n_gc_embed'] > 0:
        for b in range(B):
            cuts = np.sort(rng.choice(np.arange(40, T), 3, replace=False))
            v = rng.integers(1, arch['n_gc_category'] + 1, 4)
            ids[b] = np.repeat(v, np.diff(np.r_[0, cuts, T]))
            ids[b, cuts[1]:cuts[1] + 20] = 0
    mel = None
    if arch['n_lc_out'] > 0:
        hop = int(np.prod(arch['lc_upsample']))
        mel = rng.standard_normal((B, T // hop, arch['n_lc_in'])).astype(np.float32)
    return q, ids, mel


def edge_cond_batch(arch, B, T, invalid=1):
    """cond_batch for slices of any length >= 2 (cond_batch needs T >= 43 for its three cuts):
    rand_batch with, for GC archs, one voice change per stream at a random position in [1, T)
    (masked positions stay 0, ids[:, 0] = 0) and, for LC archs, a mel input of T / hop frames."""
    q, ids = rand_batch(arch, B, T, invalid=max(invalid, 1))
    rng = np.random.default_rng(3)
    if arch['n_gc_embed'] > 0:
        for b in range(B):
            cut = int(rng.integers(1, T))
            v = rng.choice(np.arange(1, arch['n_gc_category'] + 1), 2, replace=False)
            ids[b] = np.where(ids[b] != 0, np.repeat(v, [cut, T - cut]), 0)
    ids[:, 0] = 0
    mel = None
    if arch['n_lc_out'] > 0:
        hop = int(np.prod(arch['lc_upsample']))
        assert T % hop == 0
        mel = rng.standard_normal((B, T // hop, arch['n_lc_in'])).astype(np.float32)
    return q, ids, mel


def oracle_run(arch, P, S, q, ids, mel=None):
    """Forward and loss of the oracle in P's precision: (cache, new_save, stats, dlogits)."""
    lg, cache, new_save = R.forward(arch, P, q, ids, S, mel=mel)
    st, dlog = R.loss_fcn(arch, P, lg, q, ids, 0.0)
    return cache, new_save, st, dlog


def group_of(name):
    """Parameter group of a serial name: SIGNAL_1_3 -> SIGNAL, LC_UPSAMPLE_0 -> LC_UPSAMPLE."""
    parts = name.split('_')
    while parts and parts[-1].isdigit():
        parts.pop()
    return '_'.join(parts)


class Worst:
    """The worst max-err / own-max per group, for the written record (printed, never asserted)."""

    def __init__(self):
        self.w = {}

    def add(self, group, ratio):
        self.w[group] = max(self.w.get(group, 0.0), float(ratio))

    def report(self, title):
        print('gradcheck %s: ' % title + '  '.join('%s %.2g' % kv for kv in sorted(self.w.items())))
