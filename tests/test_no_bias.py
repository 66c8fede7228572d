"""use_bias = false on the CPU: what tests/test_gpu_no_bias.py expects of the GPU, proved on the
oracle and the host code alone.

  - the parameter layout of a no-bias arch has no bias region (n_weights == n_total), no *_BIAS
    name and no bias kind, the lbwn_params struct WaveNetTrain fills has its seven bias pointers
    null ("Bias pointers are NULL when !use_bias", include/lbwn.h), and the all-reduce buckets of
    lbwn.dist still tile the gradient buffer;
  - the bars of the GPU module see a stray bias: the float64 gradients of a with-bias twin whose
    every bias is BIAS_MUTANT = 1e-3 (same weights, same batch) are rejected by grad_close against
    the no-bias gradients on at least one tensor of every group -- PRE, SIGNAL / GATE, RESIDUAL,
    SKIP, POST1, POST2 all reject at 1e-3, so no group needed a larger power of ten (measured worst
    err / own max per group at 1e-3, the bar being 2e-4: PRE 0.35, SIGNAL 0.38, GATE 0.36,
    RESIDUAL 0.31, SKIP 0.37, POST1 0.29, POST2 0.074; the eight SKIP biases alone move S by 8e-3
    of its 0.6, and relu masks flip with it);
  - every (arch, B, T, seed) the GPU module compares with float64 (tests/gradcheck.py NO_BIAS_CASES)
    keeps its relu ties inside adoption_capped's 0.05 % of S and of h1, counted on the oracle in
    float32 against itself in float64.  One case changed its seed: the arch2 widths at (2, 200),
    seed 0 -> 7 (36 of 2400 h1 elements at seed 0, from 6 positions whose whole S is <= 0 so that
    h1 is exactly 0 without a bias; 0 of 2400 at seed 7)."""
import numpy as np
import pytest
import torch

from lbwn.arch import ParamLayout
from lbwn.dist import _Buckets
from lbwn.tmodel import WaveNetTrain
from oracle import wavenet_ref as R
from tests import gradcheck as gc

BIAS_KINDS = ('pre_b', 'sig_b', 'gate_b', 'res_b', 'skip_b', 'post1_b', 'post2_b')
BIAS_MUTANT = 1e-3
ARCHS = {'plain': lambda: gc.small_arch(use_bias=False), 'gc': lambda: gc.cond_arch(1, 0, use_bias=False),
         'lc': lambda: gc.cond_arch(0, 1, use_bias=False), 'gc_lc': lambda: gc.cond_arch(1, 1, use_bias=False),
         'arch3': gc.arch3_no_bias}


def host_net(arch, B, seed=0):
    """tests/test_gpu_parity.py make_net on the host: the same parameters and SAVE (init_vars draws
    them from a CPU generator)."""
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=1e-3, print_interval=0, seed=seed, device='cpu')
    net.init_vars(seed, bias_scale=0.1)
    return net


# ---- layout, struct, buckets -------------------------------------------------------------------

@pytest.mark.parametrize('key', sorted(ARCHS))
def test_layout_has_no_bias_region(key):
    arch = ARCHS[key]()
    lay = ParamLayout(arch)
    assert lay.n_weights == lay.n_total
    assert not any('BIAS' in n for n in lay.names())
    assert not any(e.is_bias for e in lay.entries.values())
    assert not any(k in lay.kind_base for k in BIAS_KINDS)
    assert set(lay.names()) == set(R.param_shapes(arch))
    twin = ParamLayout(dict(arch, use_bias=True))
    assert [n for n in twin.names() if 'BIAS' not in n] == lay.names()
    assert twin.n_weights == lay.n_weights and all(k in twin.kind_base for k in BIAS_KINDS)


@pytest.mark.parametrize('key', sorted(ARCHS))
def test_params_struct_bias_pointers_null(key):
    """Both structs the plan is called with (parameters and gradients)."""
    arch = ARCHS[key]()
    net = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, device='cpu')
    assert net._arch_c.use_bias == 0
    for st, flat in ((net._params_c, net.flat), (net._grads_c, net.grad_flat)):
        for f in BIAS_KINDS:
            assert getattr(st, f) is None, f
        for f in ('pre', 'sig', 'gate', 'res', 'skip', 'post1', 'post2'):
            assert getattr(st, f) == flat.data_ptr() + 4 * net.layout.kind_base[f], f
    twin = WaveNetTrain(**dict(arch, use_bias=True), batch_sz=1, l2_factor=0.0, print_interval=0, device='cpu')
    assert twin._arch_c.use_bias == 1 and all(getattr(twin._params_c, f) for f in BIAS_KINDS)


class _Stub:
    def __init__(self, layout):
        self.layout = layout
        self.grad_flat = torch.zeros(layout.n_total)
        self.stats = torch.zeros(4)


@pytest.mark.parametrize('key', sorted(ARCHS))
def test_dist_buckets_tile_a_no_bias_layout(key):
    """_Buckets' own tiling assert holds, every element has one owner, and the owners are the
    with-bias layout's (head: POST1 / POST2, side: PRE .. RESIDUAL and GC, rest: SKIP and LC)."""
    lay = ParamLayout(ARCHS[key]())
    stub = _Stub(lay)
    bk = _Buckets(stub)
    owner = np.full(lay.n_total, -1)
    for k, rs in enumerate(bk.ranges):
        for a, b in rs:
            assert 0 <= a < b <= lay.n_total and (owner[a:b] == -1).all()
            owner[a:b] = k
    assert (owner >= 0).all()
    want = {'POST1': 0, 'POST2': 0, 'PRE': 1, 'SIGNAL': 1, 'GATE': 1, 'RESIDUAL': 1, 'GC_EMBED': 1, 'GC_SIGNAL': 1,
            'GC_GATE': 1, 'SKIP': 2, 'LC_UPSAMPLE': 2, 'LC_SIGNAL': 2, 'LC_GATE': 2}
    for n, e in lay.entries.items():
        assert (owner[e.offset:e.offset + e.numel] == want[gc.group_of(n)]).all(), n
    assert sum(t.numel() for k in range(3) for t in bk.tensors(k, stub)) == lay.n_total + 3     # + the stats


# ---- the bars see a stray bias ---------------------------------------------------------------------

def _rejects(ours, ref, name):
    try:
        gc.grad_close(ours, ref, name)
    except AssertionError:
        return True
    return False


def test_mutant_stray_bias_rejected_in_every_group():
    arch = gc.small_arch(use_bias=False)
    twin = gc.small_arch(use_bias=True)
    B, T = 2, 256
    rng = np.random.default_rng(0)
    P = R.init_params(arch, rng)
    S = R.init_save(arch, B, rng)
    Pt = dict(P)
    for n, (shape, _, is_bias) in R.param_shapes(twin).items():
        if is_bias:
            Pt[n] = np.full(shape, BIAS_MUTANT)
    assert set(Pt) - set(P) and all('BIAS' in n for n in set(Pt) - set(P))
    q, ids = gc.rand_batch(arch, B, T)
    G = {}
    for key, a, p in (('none', arch, P), ('twin', twin, Pt)):
        cache, _, _, dlog = gc.oracle_run(a, p, S, q, ids)
        G[key] = R.backward(a, p, cache, dlog, 0.0)
    assert set(G['none']) == set(P)
    worst = gc.Worst()
    for n in P:
        err, own, _ = gc.err_stats(G['twin'][n], G['none'][n])
        if own:
            worst.add(gc.group_of(n) if _rejects(G['twin'][n], G['none'][n], n) else 'accepted', err / own)
    worst.report('bias = %g twin vs no bias (rejected tensors)' % BIAS_MUTANT)
    for group in ('PRE', 'SIGNAL', 'GATE', 'RESIDUAL', 'SKIP', 'POST1', 'POST2'):
        assert group in worst.w, '%s: no tensor rejects a stray bias of %g' % (group, BIAS_MUTANT)


# ---- relu ties of the GPU module's cases ----------------------------------------------------------------

@pytest.mark.parametrize('key', sorted(gc.NO_BIAS_CASES))
def test_relu_ties_within_cap(key):
    mk, B, T, invalid, seed, cond = gc.NO_BIAS_CASES[key]
    arch = mk()
    assert arch['use_bias'] is False
    net = host_net(arch, B, seed)
    P = {n: v.double().numpy() for n, v in net.vars.items()}
    S = {n: v.double().numpy() for n, v in net.save_vars.items()}
    if cond:
        q, ids, mel = gc.cond_batch(arch, B, T, invalid)
    else:
        q, ids = gc.rand_batch(arch, B, T, invalid=invalid)
        mel = None
    P32 = {k: v.astype(np.float32) for k, v in P.items()}
    S32 = {k: v.astype(np.float32) for k, v in S.items()}
    cache32, _, st32, _ = gc.oracle_run(arch, P32, S32, q, ids, mel)
    cache, _, st, _ = gc.oracle_run(arch, P, S, q, ids, mel)
    assert st32['n_valid'] == st['n_valid'] > 0
    adopted = gc.adopt_relu_signs(cache, cache32['S'], cache32['r2'])
    print('%s: relu ties %d of %d in S, %d of %d in h1' % (key, adopted[0], cache['S'].size, adopted[1],
                                                           cache['h1'].size))
    gc.adoption_capped(cache, adopted)
