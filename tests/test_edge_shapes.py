"""The ends of the depth and slice ranges on the CPU: what tests/test_gpu_edge_shapes.py expects of
the GPU at one and two layers, at slices of 2 .. 31 positions (4 positions in all at the least) and
at n_block_layers 12 and 16, proved on the oracle and the host code alone.

  - every (arch, B, T, seed) of tests/gradcheck.py EDGE_CASES keeps its relu ties inside
    adoption_capped's 0.05 % of S and of h1, counted on the oracle in float32 against itself in
    float64 with the net's own initialiser (host_net).  The cap is a condition on the case.  Where it
    is below one element (the 32-wide cases of up to 34 positions and the arch2 widths) the seed
    must give no tie at all.  Counted (of S, of h1; printed by every run with -s):
        tiny_2x2, tiny_2x3, tiny_3x5, tiny_2x17, tiny_arch2w_3x5, tiny_cond16_3x8, tiny_cond32_2x8,
        tiny_cond32_5x16, L1_cond32_2x136                                      0, 0
        tiny_7x31 0, 1 of 6944 (cap 3.5)      tiny_40x9 3 of 23040 (cap 11.5), 0
        tiny_arch3_2x8 0, 2 of 8192 (cap 4.1)
        L1_2x256 8 of 32768, 2 of 16384 (caps 16.4 / 8.2)     L1_c16_2x256 2, 3     L1_cond16_2x136 0, 2 (cap 4.4)
        L2_d1_2x256 2, 0     L2_3x200 1, 3 of 19200 (cap 9.6)     L2_cond32_2x136 2, 0
        deep12_2x2200 8 of 281600, 3 of 140800 (caps 140.8 / 70.4)     deep12_c16_2x2200 9, 10
        deep16_2x300 3 of 38400, 1 of 19200
    One case changed its seed: L1_1x129, seed 0 -> 1 (4 of 8256 elements of S at seed 0 with a cap of
    4.1: at its cap by luck; 1 of 8256 and 0 of 4128 at seed 1);
  - the reference itself is proved at these shapes by tests/test_oracle.py
    test_backward_finite_difference (L1, L2-d1, 2x2, 1x3, nbl12-T40);
  - the bars see the mistake that belongs to one layer: a backward whose only layer takes a dx_out
    from a next layer that does not exist (an unguarded l + 1 < L) is rejected by grad_close on PRE,
    and its RESIDUAL gradients are no longer exactly zero."""
import numpy as np
import pytest

from oracle import wavenet_ref as R
from tests import gradcheck as gc
from tests.test_no_bias import host_net


def edge_batch(key):
    mk, B, T, invalid, seed, cond = gc.EDGE_CASES[key]
    arch = mk()
    if cond:
        q, ids, mel = gc.edge_cond_batch(arch, B, T, invalid)
    else:
        q, ids = gc.rand_batch(arch, B, T, invalid=invalid)
        mel = None
    return arch, B, T, seed, q, ids, mel


def test_edge_table():
    """Every case is a shape lbwn_plan_create accepts, the tiny ones have a scored position, and the
    conditioned batches have what edge_cond_batch promises."""
    assert len(gc.EDGE_CASES) == 22
    for key, (mk, B, T, invalid, seed, cond) in gc.EDGE_CASES.items():
        arch, B, T, seed, q, ids, mel = edge_batch(key)
        assert arch['n_blocks'] >= 1 and 1 <= arch['n_block_layers'] <= 16 and T >= 2, key
        assert invalid == gc.edge_invalid(T) and q.shape == ids.shape == (B, T)
        assert (ids[:, 1:] != 0).any(), key
        if cond:
            hop = int(np.prod(arch['lc_upsample']))
            assert mel.shape == (B, T // hop, arch['n_lc_in']) and not ids[:, 0].any()
            for b in range(B):
                assert 1 <= len(set(ids[b][ids[b] != 0])) <= 2
            assert any(len(set(ids[b][ids[b] != 0])) == 2 for b in range(B)), key
    assert gc.edge_invalid(2) == gc.edge_invalid(3) == 0 and gc.edge_invalid(4) == gc.edge_invalid(37) == 1
    assert gc.edge_invalid(38) == 37


@pytest.mark.parametrize('key', sorted(gc.EDGE_CASES))
def test_relu_ties_within_cap(key):
    arch, B, T, seed, q, ids, mel = edge_batch(key)
    net = host_net(arch, B, seed)
    P = {n: v.double().numpy() for n, v in net.vars.items()}
    S = {n: v.double().numpy() for n, v in net.save_vars.items()}
    P32 = {k: v.astype(np.float32) for k, v in P.items()}
    S32 = {k: v.astype(np.float32) for k, v in S.items()}
    cache32, _, st32, _ = gc.oracle_run(arch, P32, S32, q, ids, mel)
    cache, _, st, _ = gc.oracle_run(arch, P, S, q, ids, mel)
    assert st32['n_valid'] == st['n_valid'] > 0
    adopted = gc.adopt_relu_signs(cache, cache32['S'], cache32['r2'])
    print('%s: relu ties %d of %d in S, %d of %d in h1' % (key, adopted[0], cache['S'].size, adopted[1],
                                                           cache['h1'].size))
    gc.adoption_capped(cache, adopted)


# ---- the mutant that belongs to L = 1 -------------------------------------------------------------

def one_layer_backward(arch, P, cache, dlog, dx_out):
    """R.backward for a stack of one layer (use_bias, no conditioning), with the gradient dx_out that
    a next layer would hand down given from outside: zeros for the function's true gradient."""
    assert R.n_layers(arch) == 1 and arch['use_bias'] and cache['emb'] is None and cache['lc'] is None
    g = {}
    r2, h1, S = cache['r2'], cache['h1'], cache['S']
    g['POST2'] = np.einsum('btp,btq->pq', r2, dlog)
    g['POST2_BIAS'] = dlog.sum(axis=(0, 1))
    dh1 = (dlog @ P['POST2'].T) * (h1 > 0)
    g['POST1'] = np.einsum('bts,btp->sp', np.maximum(S, 0), dh1)
    g['POST1_BIAS'] = dh1.sum(axis=(0, 1))
    dS = (dh1 @ P['POST1'].T) * (S > 0)
    z, th, sg, x, prev = (cache[k][0] for k in ('z', 'th', 'sg', 'x', 'prev'))
    g['SKIP_0_0'] = np.einsum('btc,bts->cs', z, dS)
    g['SKIP_BIAS_0_0'] = dS.sum(axis=(0, 1))
    g['RESIDUAL_0_0'] = np.einsum('btc,btr->cr', z, dx_out)
    g['RESIDUAL_BIAS_0_0'] = dx_out.sum(axis=(0, 1))
    dz = dS @ P['SKIP_0_0'].T + dx_out @ P['RESIDUAL_0_0'].T
    dv = {'SIGNAL': dz * sg * (1 - th * th), 'GATE': dz * th * sg * (1 - sg)}
    dx = dx_out.copy()
    for nm in ('SIGNAL', 'GATE'):
        W = P[nm + '_0_0']
        g[nm + '_0_0'] = np.stack([np.einsum('btr,btc->rc', prev, dv[nm]), np.einsum('btr,btc->rc', x, dv[nm])])
        g[nm + '_BIAS_0_0'] = dv[nm].sum(axis=(0, 1))
        dx += dv[nm] @ W[1].T
        dx[:, :-1] += (dv[nm] @ W[0].T)[:, 1:]
    g['PRE'] = np.zeros_like(P['PRE'])
    np.add.at(g['PRE'], cache['wav_q'], dx)
    g['PRE_BIAS'] = dx.sum(axis=(0, 1))
    return g, dx


def _rejects(ours, ref, name):
    try:
        gc.grad_close(ours, ref, name)
    except AssertionError:
        return True
    return False


def test_mutant_phantom_next_layer_rejected_at_one_layer():
    """At L = 1 the first layer is the last: dx_out is zero by definition.  A chain that formed
    dn = dx_out of layer l + 1 without the l + 1 < L guard would read whatever the hand-off rows of a
    layer 1 hold -- here the rows this layer itself hands down (what the slot holds after a step of a
    deeper plan on the same workspace).  With zeros the restatement is R.backward bit for bit; with
    the phantom rows PRE misses the bar and RESIDUAL / RESIDUAL_BIAS are no longer exactly zero."""
    arch, B, T, seed, q, ids, mel = edge_batch('L1_2x256')
    rng = np.random.default_rng(0)
    P = R.init_params(arch, rng, bias_scale=0.1)
    S = R.init_save(arch, B, rng)
    cache, _, st, dlog = gc.oracle_run(arch, P, S, q, ids)
    G = R.backward(arch, P, cache, dlog, 0.0, intermediates=True)
    true, dx0 = one_layer_backward(arch, P, cache, dlog, np.zeros_like(cache['x_out']))
    assert set(true) == set(G)
    for name in G:
        np.testing.assert_allclose(true[name], G[name], rtol=1e-13, atol=1e-18, err_msg=name)
    np.testing.assert_allclose(dx0, cache['bwd']['dx0'], rtol=1e-13, atol=1e-18)
    assert not G['RESIDUAL_0_0'].any() and not G['RESIDUAL_BIAS_0_0'].any()
    mut, _ = one_layer_backward(arch, P, cache, dlog, dx0)
    err, own, _ = gc.err_stats(mut['PRE'], G['PRE'])
    print('phantom next layer at L = 1: PRE max err / own max %.3g (the bar is %.3g)' % (err / own, gc.GRAD_REL))
    for name in ('PRE', 'PRE_BIAS', 'SIGNAL_0_0', 'GATE_0_0', 'RESIDUAL_0_0', 'RESIDUAL_BIAS_0_0'):
        assert _rejects(mut[name], G[name], name), name
    for name in ('POST2', 'POST1', 'SKIP_0_0'):       # upstream of the layer: untouched
        gc.grad_close(mut[name], G[name], name)
