"""The gradient bar bites (tests/gradcheck.py), proved on the CPU with the oracle alone.

grad_close asks max|ours - ref| <= 2e-4 of the tensor's OWN max.  Here: the oracle run in
float32 meets that against float64 with more than 10x to spare, so correct fp32 arithmetic can
reach it; five plausible kernel mistakes all miss it; and the rule it replaces,
2e-4 * max(1, max|ref|), accepts the first three of them -- the reason this file exists.
Relu-tie adoption (adopt_relu_signs) stays under its cap on every case and is the identity on the
oracle's own signs."""
import numpy as np
import pytest

from oracle import wavenet_ref as R
from tests import gradcheck as gc

CASES = {'small_2x256': (lambda: gc.small_arch(), 2, 256), 'small_3x200': (lambda: gc.small_arch(), 3, 200),
         'cond_2x256': (lambda: gc.cond_arch(1, 1), 2, 256)}


class Case:
    def __init__(self, key, invalid=37):
        mk, B, T = CASES[key]
        self.arch, self.B, self.T = mk(), B, T
        rng = np.random.default_rng(0)
        self.P = R.init_params(self.arch, rng, bias_scale=0.1)
        self.S = R.init_save(self.arch, B, rng)
        self.q, self.ids, self.mel = gc.cond_batch(self.arch, B, T, invalid)
        self.cache, _, self.st, self.dlog = gc.oracle_run(self.arch, self.P, self.S, self.q, self.ids, self.mel)
        self.G = R.backward(self.arch, self.P, self.cache, self.dlog, 0.0, intermediates=True)
        for v in self.G.values():
            v.setflags(write=False)
        self.L = R.n_layers(self.arch)

    def last(self, name):
        b, bl, _ = R.layer_index(self.arch, self.L - 1)
        return '%s_%d_%d' % (name, b, bl)


_cases = {}


@pytest.fixture(params=sorted(CASES))
def case(request):
    """Each case's float64 reference is computed once and shared, read-only."""
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def rejects(ours, ref, name):
    try:
        gc.grad_close(ours, ref, name)
    except AssertionError:
        return True
    return False


def test_float32_oracle_passes_with_room(case):
    """The same oracle in float32 against float64: every tensor within 2e-5 of its own max (a
    tenth of the bar; measured worst 1.7e-6), zero references exactly zero."""
    c = case
    P32 = {k: v.astype(np.float32) for k, v in c.P.items()}
    S32 = {k: v.astype(np.float32) for k, v in c.S.items()}
    cache32, _, st32, dlog32 = gc.oracle_run(c.arch, P32, S32, c.q, c.ids, c.mel)
    assert dlog32.dtype == np.float32 and st32['n_valid'] == c.st['n_valid']
    G32 = R.backward(c.arch, P32, cache32, dlog32, 0.0)
    cache64, _, _, dlog = gc.oracle_run(c.arch, c.P, c.S, c.q, c.ids, c.mel)
    adopted = gc.adopt_relu_signs(cache64, cache32['S'], cache32['r2'])
    gc.adoption_capped(cache64, adopted)
    G = R.backward(c.arch, c.P, cache64, dlog, 0.0)
    worst = gc.Worst()
    for name, ref in G.items():
        assert G32[name].dtype == np.float32
        worst.add(gc.group_of(name), gc.grad_close(G32[name], ref, name, rel=gc.GRAD_REL / 10))
    worst.report('float32 oracle vs float64')
    for name in (c.last('RESIDUAL'), c.last('RESIDUAL_BIAS')):
        assert not G[name].any() and not G32[name].any()


def test_mutant_zeroed_gate(case):
    """One layer's GATE gradient replaced by zeros (the smallest of them: 2e-4 is more than its
    whole scale)."""
    c = case
    name = min((n for n in c.G if n.startswith('GATE_') and 'BIAS' not in n), key=lambda n: np.abs(c.G[n]).max())
    assert np.abs(c.G[name]).max() > 0
    mut = np.zeros_like(c.G[name])
    assert rejects(mut, c.G[name], name)
    assert gc.old_close_accepts(mut, c.G[name])


def test_mutant_signal_scaled(case):
    """Every SIGNAL gradient off by 1 %."""
    c = case
    names = [n for n in c.G if n.startswith('SIGNAL_')]
    assert len(names) == 2 * c.L
    for name in names:
        assert rejects(0.99 * c.G[name], c.G[name], name)
        assert gc.old_close_accepts(0.99 * c.G[name], c.G[name])


def test_mutant_noise_in_dead_residual(case):
    """The last layer's RESIDUAL feeds nothing: its reference is exactly zero, and 1e-4 of noise
    there is garbage, not rounding."""
    c = case
    for name in (c.last('RESIDUAL'), c.last('RESIDUAL_BIAS')):
        assert not c.G[name].any()
        mut = 1e-4 * np.random.default_rng(1).uniform(-1, 1, c.G[name].shape)
        assert rejects(mut, c.G[name], name)
        assert gc.old_close_accepts(mut, c.G[name])
        gc.grad_close(np.zeros_like(c.G[name]), c.G[name], name)


def test_mutant_dropped_dlogits_row(case):
    """One valid position's dlogits row lost (a tile edge, a masked-skip list off by one): every
    tensor's gradient moves by about 1 / n_valid of its scale."""
    c = case
    b, t = c.B - 1, c.T - 2
    assert c.ids[b, t + 1] != 0 and np.abs(c.dlog[b, t]).max() > 0
    dlog = c.dlog.copy()
    dlog[b, t] = 0
    cache, _, _, _ = gc.oracle_run(c.arch, c.P, c.S, c.q, c.ids, c.mel)
    Gm = R.backward(c.arch, c.P, cache, dlog, 0.0, intermediates=True)
    for name in ('POST2_BIAS', 'POST2', 'POST1', 'POST1_BIAS', c.last('SKIP'), 'PRE_BIAS'):
        assert rejects(Gm[name], c.G[name], name), name
    gc.grad_close(cache['bwd']['dh1'][:, :t], c.cache['bwd']['dh1'][:, :t], 'dh1 before the dropped row')
    assert rejects(cache['bwd']['dh1'], c.cache['bwd']['dh1'], 'dh1')


@pytest.mark.parametrize('key', sorted(CASES))
def test_mutant_tap0_without_save_rows(key):
    """One layer's tap-0 weight gradient summed without the positions t < d, whose dilated tap
    x[t - d] is a SAVE row (a halo the backward forgot).  With the usual 37 masked positions at
    the head of every stream -- more than these archs' receptive fields of 30 and 15 -- no
    gradient reaches a position t < d and the mutant computes the right answer: the first
    block's d = 8 layer of a batch that masks 3 positions is where it shows."""
    c = Case(key, invalid=3)
    l = c.arch['n_block_layers'] - 1
    b, bl, d = R.layer_index(c.arch, l)
    assert d == 2 ** (c.arch['n_block_layers'] - 1)
    Cd = c.arch['n_dil']
    prev, dv = c.cache['prev'][l], c.cache['bwd']['dv'][l]
    for h, nm in enumerate(('SIGNAL', 'GATE')):
        name = '%s_%d_%d' % (nm, b, bl)
        dvh = dv[..., h * Cd:(h + 1) * Cd]
        full = np.einsum('btr,btc->rc', prev, dvh)
        np.testing.assert_allclose(full, c.G[name][0], rtol=1e-12, atol=1e-18)
        mut = c.G[name].copy()
        mut[0] = np.einsum('btr,btc->rc', prev[:, d:], dvh[:, d:])
        assert rejects(mut, c.G[name], name)


def test_adoption_is_rare_and_identity_on_own_signs(case):
    """The ambiguous elements (within the forward bars of zero) stay under the 0.05 % cap, and
    adopting the oracle's own signs changes no gradient bit."""
    c = case
    cache, _, _, dlog = gc.oracle_run(c.arch, c.P, c.S, c.q, c.ids, c.mel)
    adopted = gc.adopt_relu_signs(cache, c.cache['S'], c.cache['r2'])
    gc.adoption_capped(cache, adopted)
    print('relu ties: %d of %d in S, %d of %d in h1' % (adopted[0], cache['S'].size, adopted[1], cache['h1'].size))
    G = R.backward(c.arch, c.P, cache, dlog, 0.0)
    for name, ref in c.G.items():
        assert np.array_equal(G[name], ref), name


def test_adoption_moves_only_ambiguous_signs():
    """A sign handed over for an ambiguous element is taken; one for a clear element is not."""
    cache = {'S': np.array([[[0.5, 1e-7, -3e-6, -2.0]]]), 'h1': np.array([[[1.0, -1e-6, 1e-5, -0.3]]])}
    s = np.array([-0.5, -2e-7, 4e-6, 2.0])
    r2 = np.array([0.0, 3e-6, 0.0, 0.7])
    assert gc.adopt_relu_signs(cache, s, r2) == (2, 2)
    assert np.array_equal(cache['S'] > 0, [[[True, False, True, False]]])
    assert np.array_equal(cache['h1'] > 0, [[[True, True, False, False]]])
    with pytest.raises(AssertionError):
        gc.adoption_capped(cache, (2, 2))


def test_grad_close_rule():
    ref = np.array([1e-4, -2e-4, 0.0])
    assert gc.grad_close(ref + 3e-8, ref, 'x') == pytest.approx(1.5e-4)
    assert rejects(ref + 5e-8, ref, 'x') and gc.old_close_accepts(ref + 5e-8, ref)
    assert rejects(np.array([np.nan, 0, 0]), ref, 'x')
    gc.grad_close(np.zeros(3), np.zeros(3), 'zero')
    assert rejects(np.array([0, 1e-30, 0]), np.zeros(3), 'zero')
    with pytest.raises(AssertionError, match='rel L2'):
        gc.grad_close(2 * ref, ref, 'x')
