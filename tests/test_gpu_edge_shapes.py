"""The plans at the ends of the depth and slice ranges they accept, on the GPU against float64.

lbwn_plan_create takes n_blocks >= 1, n_block_layers in 1..16, slice_sz >= 2 and at least 4
positions; the generator any stack up to 256 layers.  The cases are tests/gradcheck.py EDGE_CASES
(tests/test_edge_shapes.py holds their relu ties to adoption_capped on the CPU, tests/test_oracle.py
proves the reference at these shapes), through check_plan / check_conditioning of
tests/test_gpu_parity.py with its bars unchanged: z at 1e-5 on identical inputs and 5e-5 end to end,
SAVE layer 0 bit-exact and deeper layers at 1e-5, s / r2 at 1e-5 / 2e-5, every gradient and backward
intermediate at 2e-4 of its own max (grad_close), exact zeros where the reference is zero,
status == 0.  Every backward starts from gradients filled with NaN.

  L1*     one layer: the first layer is the last (the dead residual output, the layer-0 dx0 export and
          the PRE gradient meet in one loop pass), H = 1
  L2*     two layers: the chains' min(l + 2, L - 1) prefetches and l + 2 < L guards
  tiny*   M = B.T = 4 .. 360 with T below 4 / 16 / 32: a tile with fewer rows than one 32-row block of
          the chain-order layouts, 16-position waves with no valid row, one colsum part, weight-gradient
          GEMMs with K = M < 32, the head with one scored row per stream
  deep*   n_block_layers 12 and 16: taps at d = 1024 .. 32768, H up to 32768
and the generator at one layer, two layers of dilation 1, and a d = 2048 ring that wraps.

The one defect these cases found: (B, T) = (1, 2) and (1, 3) were accepted by lbwn_plan_create, ran
their forward, and were refused by the first GEMM of lbwn_train_backward (EINVAL: below 4 rows
lbwn_gemm_launch leaves the bf16-split form, the only one with the column-partial and chain-order
epilogues the backward asks for).  lbwn_plan_create now refuses batch_sz * slice_sz < 4
(include/lbwn.h, tests/test_capi.py); the two cases became (2, 2) and (2, 3).

Worst max-err / own-max measured on the MI355X (printed by every run with -s; the bar is 2e-4 =
200e-6), in units of 1e-6, over every case and chain form of a column; "small" is the small_arch
(2, 256) value of tests/test_gpu_parity.py's table that the row is to be read against, "tiny*" the
tiny cases but arch3's, "f32" GEMM mode 0:

    group          small   L1*    L2*    tiny*  tiny_arch3  deep12  deep12_c16  deep16  L1 f32  tiny f32
    PRE            0.66    0.43   0.46   0.81   2.5         0.67    0.43        0.67    0.56    0.65
    PRE_BIAS       2.1     0.74   0.75   0.94   2.6         4.3     2.2         1.1     0.28    0.70
    SIGNAL         1.3     0.50   0.75   1.5    3.1         3.1     2.1         1.2     0.30    0.59
    SIGNAL_BIAS    1.7     0.96   0.99   1.4    3.1         3.6     2.1         1.6     0.29    0.90
    GATE           1.3     0.45   0.75   1.6    4.1         3.2     2.4         1.8     0.47    0.91
    GATE_BIAS      1.3     0.86   1.0    1.5    3.8         5.3     2.7         1.9     0.41    0.97
    RESIDUAL       1.5     0      0.86   1.4    3.1         3.6     2.6         1.6     0       1.0
    RESIDUAL_BIAS  1.4     0      1.1    1.4    3.0         4.1     2.4         1.6     0       0.88
    SKIP           1.1     0.95   0.89   1.3    2.3         2.8     2.2         1.0     0.48    0.70
    SKIP_BIAS      0.70    0.84   0.79   0.75   0.68        2.2     2.0         0.58    0.29    0.49
    POST1          1.2     0.97   1.3    1.3    0.53        2.6     1.1         1.3     0.58    0.76
    POST1_BIAS     0.89    0.66   1.1    0.73   0.29        2.6     1.2         1.1     0.32    0.46
    POST2          0.36    0.53   0.58   0.38   1.0         0.42    0.38        0.86    0.82    0.30
    POST2_BIAS     0.22    0.15   0.17   0.11   0.06        0.14    0.11        0.12    0.11    0.07
    dlogits        0.03    0.03   0.03   0.03   0.03        0.03    0.03        0.03    0.03    0.03
    dh             0.85    0.85   0.90   1.1    0.70        1.1     1.1         0.90    1.4     0.77
    ds             0.38    0.36   0.30   0.43   0.66        0.43    0.35        0.32    0.53    0.56
    dz             0.42    0.39   0.47   0.54   0.74        0.43    0.37        0.36    0.53    0.37

Conditioning (L1* / L2* / tiny*, beside tests/test_gpu_parity.py's cond_arch figures in brackets):
GC_EMBED 0.72 / 0.64 / 1.2 (0.96), GC_SIGNAL 0.49 / 0.72 / 0.56 (0.79), GC_GATE 0.62 / 0.66 / 0.56
(0.92), LC_SIGNAL 0.45 / 0.47 / 0.47 (0.74), LC_GATE 0.44 / 0.43 / 0.64 (0.87), LC_UPSAMPLE 0.49 /
0.43 / 0.47 (0.62), dvall 0.33 / 0.36 / 0.42 (0.47), gcd 0.52 / 0.66 / 0.43 (0.86).  L1 (2, 256)
under LBWN_NO_CHAIN=1: at most 0.91 (POST1).

L1*, L2* and tiny* sit within 2x of the small figures in every group.  POST2 is the one group above
2x in L1 f32 (0.82) and deep16 (0.86): the float64 oracle run in float32 has POST2 at 0.64 and 0.81
on those two cases, so that is float32's own level.  The columns more than 2x above "small" are the ones
that are another depth or length, not another arithmetic.  tiny_arch3 is par/arch3.json: its column
is to be read against that table's arch3 (2, 512) one, 2.8 .. 12, and is below it throughout.  deep12
(2, 2200) sums 4400 positions through 12 layers where small sums 512 through 8: the float64 oracle
run in float32 is at 2.8 there (GATE_BIAS; 1.4 for small, 3.7 for arch3), so the kernels sit at 2x
float32 arithmetic as they do for small and arch3 (12 / 3.7); deep12_c16 (the per-layer kernels, f32
oracle 3.4) and deep16 (300 positions, f32 oracle 1.7) likewise.
"""
import functools

import numpy as np
import pytest
import torch

from lbwn import _lib
from oracle import wavenet_ref as R
from tests.gradcheck import EDGE_CASES, edge_cond_batch, rand_batch, small_arch
from tests.test_gpu_gen import form, make_gen  # noqa: F401  (form is a fixture)
from tests.test_gpu_gen_prefill import SEED, check_free_steps, prefill_from_zero
from tests.test_gpu_gen_score import score_from_zero
from tests.test_gpu_parity import (DEV, check_adam_step, check_conditioning, check_plan, gemm_mode,  # noqa: F401
                                   make_net)

pytestmark = pytest.mark.gpu

SHALLOW_TINY = sorted(k for k in EDGE_CASES if not k.startswith('deep'))
DEEP = sorted(k for k in EDGE_CASES if k.startswith('deep'))


def run_case(key, form=''):
    """The case through check_plan / check_conditioning from NaN gradients; returns the net after its
    backward."""
    mk, B, T, invalid, seed, cond = EDGE_CASES[key]
    arch = mk()
    if cond:
        return check_conditioning(1, 1, arch['n_res'], B, T, '%s %s' % (key, form), arch=arch, seed=seed,
                                  poison_grads=True, batch=functools.partial(edge_cond_batch, invalid=invalid))
    return check_plan(arch, B, T, invalid=invalid, seed=seed, poison_grads=True, title='edge %s %s' % (key, form))


def one_chain_form(monkeypatch, tile='w32'):
    monkeypatch.setenv('LBWN_CHAIN_TILE', tile)
    monkeypatch.setenv('LBWN_BWD_WGRAD', '0')


# ---- depth and slice cases -----------------------------------------------------------------------

@pytest.mark.parametrize('key', SHALLOW_TINY)
def test_shallow_and_tiny(lib, key, chain_tile):
    """One and two layers, and slices of 2 .. 31 positions, over the five chain forms (the widths the
    chains do not take run the per-layer kernels under each)."""
    run_case(key, chain_tile)


@pytest.mark.parametrize('tile', ['w32', '128'])
@pytest.mark.parametrize('key', DEEP)
def test_deep(lib, monkeypatch, key, tile):
    """n_block_layers = 12 at T = 2200 (real taps at d = 1024 and 2048, 17 tiles per stream whose
    producer tile is 8 and 16 tiles back) and 16 at T = 300 (every tap of d >= 512 a SAVE row, a SAVE
    of 65535 rows per stream)."""
    one_chain_form(monkeypatch, tile)
    run_case(key, tile)


@pytest.mark.parametrize('key', ['L1_2x256', 'tiny_3x5'])
def test_f32_mfma_mode(lib, gemm_mode, monkeypatch, key):
    """GEMM mode 0: the f32 chains (row-major dZ / DV) and f32 MFMA GEMMs."""
    one_chain_form(monkeypatch)
    gemm_mode(0)
    run_case(key, 'f32 MFMA')


def test_one_layer_per_layer_kernels(lib, monkeypatch):
    """LBWN_NO_CHAIN=1: lbwn_layer_fwd / bwd_launch as the only, first and last layer at 32 channels."""
    one_chain_form(monkeypatch)
    monkeypatch.setenv('LBWN_NO_CHAIN', '1')
    run_case('L1_2x256', 'no chain')


@pytest.mark.parametrize('tile', ['w32', '128'])
def test_deep12_staged_equals_unstaged_bitwise(lib, monkeypatch, tile):
    """tests/test_gpu_parity.py test_staged_equals_unstaged_arch3_bitwise at n_block_layers = 12: one
    slice of 2200 against stages 1000 + 1200, both shorter than d = 2048 (rows [T, d) of the new SAVE
    are old SAVE rows): every layer's z, SAVE and r2, bit for bit."""
    one_chain_form(monkeypatch, tile)
    mk, B, T, invalid, seed, _ = EDGE_CASES['deep12_2x2200']
    arch = mk()
    L, Cd = R.n_layers(arch), arch['n_dil']
    q, ids = rand_batch(arch, B, T, invalid=invalid)
    a = make_net(arch, B, seed=seed)
    a.forward(q, None, ids, backward=False)
    assert int(a.plan_tensor(T, 'status').view(torch.int32)[0]) == 0
    full_z = a.plan_tensor(T, 'z').view(B, T, L * Cd).clone()
    full_r2 = a.plan_tensor(T, 'r2').view(B, T, -1).clone()
    save_full = a.save_flat.clone()
    b = make_net(arch, B, seed=seed)
    zs, r2s = [], []
    for lo, hi in ((0, 1000), (1000, 2200)):
        b.forward(q[:, lo:hi], None, ids[:, lo:hi], backward=False)
        assert int(b.plan_tensor(hi - lo, 'status').view(torch.int32)[0]) == 0
        zs.append(b.plan_tensor(hi - lo, 'z').view(B, hi - lo, L * Cd).clone())
        r2s.append(b.plan_tensor(hi - lo, 'r2').view(B, hi - lo, -1).clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(zs, 1), full_z)
    assert torch.equal(b.save_flat, save_full)
    assert torch.equal(torch.cat(r2s, 1), full_r2)


# ---- L = 1 and tiny (1, 2) by name ---------------------------------------------------------------

def test_one_layer_dead_residual_exactly_zero(lib, chain_tile):
    """The single layer's x_out feeds nothing: RESIDUAL_0_0 / RESIDUAL_BIAS_0_0 are exactly zero,
    starting from NaN."""
    net = run_case('L1_2x256', chain_tile)
    assert net.layout.names().count('RESIDUAL_0_0') == 1
    for name in ('RESIDUAL_0_0', 'RESIDUAL_BIAS_0_0'):
        g = net.grads[name]
        assert bool(torch.isfinite(g).all()) and not bool(g.any()), name


def test_one_layer_adam_steps(lib):
    check_adam_step(small_arch(nb=1, nbl=1))


def test_two_positions_one_scored_row(lib, chain_tile):
    """(B, T) = (2, 2), the smallest plan there is (lbwn_plan_create refuses (1, 2): fewer than 4
    positions): stream 1's only target is masked, so one row is scored, 1 / n_valid = 1, and the rows
    with no target -- each stream's second, and stream 1's masked first -- get no gradient."""
    net = run_case('tiny_2x2', chain_tile)
    stats = net.stats.cpu().numpy()
    assert stats[1] == 1 and stats[3] == 1
    dlog = net.plan_tensor(2, 'logits').view(4, -1)
    assert bool(dlog[0].any()) and not bool(dlog[1:].any())


# ---- the head at T = 2 and 3 ---------------------------------------------------------------------

def _head_problem(B, T, Q):
    rng = np.random.default_rng(5 + T)
    lg = rng.normal(size=(B, T, Q)) * 3
    q, ids = rand_batch(dict(n_quant=Q), B, T, invalid=0)
    st, dlog = R.loss_fcn(dict(n_quant=Q), {}, lg, q, ids, 0.0)
    assert st['n_valid'] >= 1
    return lg, q, ids, st, dlog


def _head_call(lib, lg, q, ids, B, T, Q, write_grad):
    lgd = torch.tensor(lg, dtype=torch.float32, device=DEV).contiguous()
    qd = torch.tensor(q, device=DEV)
    idd = torch.tensor(ids, device=DEV)
    stats = torch.zeros(4, device=DEV)
    ws = torch.zeros(3 * 2048, device=DEV)
    before = lgd.clone()
    _lib.check(lib.lbwn_head_xent(lgd.data_ptr(), qd.data_ptr(), idd.data_ptr(), B, T, Q, write_grad,
                                  stats.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    return lgd, before, stats.cpu().numpy()


def _head_stats(s, st, B, T):
    assert int(s[1]) == st['n_valid']
    np.testing.assert_allclose(s[0], st['sum_xent'], rtol=1e-5)
    assert int(s[2]) // (B * (T - 1)) == st['avg_diff']
    assert int(s[2]) == st['sum_absdiff']


@pytest.mark.parametrize('Q', [256, 512, 520])
@pytest.mark.parametrize('B,T', [(1, 2), (5, 3)])
def test_head_xent_short_streams(lib, B, T, Q):
    """lbwn_head_xent against R.loss_fcn with one or two scored rows per stream (stream 1 of (5, 3) has
    none): both register-resident kernels and the generic one, the asserts of
    tests/test_gpu_parity.py::test_head_xent; with write_grad = 0 the same stats and the logits
    bitwise untouched."""
    lg, q, ids, st, dlog = _head_problem(B, T, Q)
    lgd, _, s = _head_call(lib, lg, q, ids, B, T, Q, 1)
    _head_stats(s, st, B, T)
    np.testing.assert_allclose(lgd.cpu().numpy(), dlog * st['n_valid'], rtol=0, atol=1e-6)
    assert not bool(lgd[:, -1].any()), 'the last row of a stream has no target'
    lgd0, before, s0 = _head_call(lib, lg, q, ids, B, T, Q, 0)
    _head_stats(s0, st, B, T)
    np.testing.assert_array_equal(s0[:3], s[:3])
    assert torch.equal(lgd0.view(torch.int32), before.view(torch.int32))


# ---- the generator -------------------------------------------------------------------------------

GEN = {'L1': (1, 1, 40), 'L2_d1': (2, 1, 40), 'deep12': (1, 12, 2100)}     # nb, nbl, steps
GEN_B = 3


def _gen_case(key):
    nb, nbl, n = GEN[key]
    return small_arch(nb=nb, nbl=nbl), n, key == 'deep12'


@pytest.mark.parametrize('key', sorted(GEN))
def test_gen_teacher_forced(key, form):
    """tests/test_gpu_gen.py test_gen_teacher_forced_and_gc on these stacks: 25 teacher codes, then
    free running; the samples equal the oracle's and the last logits agree at 2e-4 of max|logit|.
    The 2100 steps of deep12 (its d = 2048 ring wraps) are evaluated along the GPU's own trajectory
    as test_gen_arch3_full_ring_depth does (check_free_steps: a draw may differ at a near CDF tie only,
    last logits at 1e-4)."""
    arch, n, deep = _gen_case(key)
    teacher_q = np.random.default_rng(1).integers(0, 256, 25).astype(np.int32)
    g, P = make_gen(arch, GEN_B, chunk=1000 if deep else 10)
    g.teacher_mu = torch.as_tensor(teacher_q, device='cuda')
    g.build_graph(n)
    g.run(n)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    if deep:
        assert len(np.unique(g.samples().cpu().numpy()[:, :n])) > 16
        check_free_steps(g, lambda fq: R.generate(arch, P, GEN_B, n, seed=SEED, teacher_q=teacher_q, forced_q=fq,
                                                  return_logits=True), 0, n)
        return
    s_ref, _, lg_ref = R.generate(arch, P, GEN_B, n, seed=SEED, teacher_q=teacher_q, return_logits=True)
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], s_ref)
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg_ref[:, -1], rtol=0, atol=2e-4 * np.abs(lg_ref).max())


@pytest.mark.parametrize('key', sorted(GEN))
def test_gen_prefill_then_run(key, form, monkeypatch):
    """tests/test_gpu_gen_prefill.py prefill_from_zero: per-stream prompts, rings at 5e-5, then free
    steps.  Shallow: 25 codes in slices of 5 and 15 free steps.  deep12: 2060 codes in slices of 1000
    (shorter than d = 1024 and 2048) and 40 free steps that read the wrapped d = 2048 ring."""
    arch, n, deep = _gen_case(key)
    k = 40 if deep else 15
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '1000' if deep else '5')
    prompt = np.random.default_rng(41).integers(0, 256, (GEN_B, n - k)).astype(np.int32)
    prefill_from_zero('edge_%s' % key, form, arch, GEN_B, prompt, k, chunk=1000 if deep else 16, yardstick=not deep)


@pytest.mark.parametrize('key', sorted(GEN))
def test_gen_score(key, form, monkeypatch):
    """tests/test_gpu_gen_score.py score_from_zero over the whole length: logp at 2e-4 of max|logit|,
    the last step's logits at 1e-4."""
    arch, n, deep = _gen_case(key)
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '1000' if deep else '5')
    prompt = np.random.default_rng(42).integers(0, 256, (GEN_B, n)).astype(np.int32)
    score_from_zero('edge_%s' % key, form, arch, GEN_B, prompt, seq_streams=[0] if deep else None)
