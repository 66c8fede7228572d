"""Parallel prompt prefill (lbwn_gen_prefill) on the GPU against the oracle.

Two bars throughout:
  rings         after the prefill every layer's ring equals the oracle's rings after the same n
                teacher-forced steps (generate(forced_q=prompt, return_state=True)) within
                5e-5 · max|oracle ring of that layer| (the end-to-end activation bar).  Where
                the prompt starts at step 0 the sequential teacher path's error on the same prompt is
                measured and printed beside it: the parent's code is the yardstick.
  continuation  the free steps after the prefill are evaluated by the oracle along the GPU's own
                trajectory, resumed from the ORACLE's state after the prompt: every draw equals the
                oracle's except at a near CDF tie (tol 5e-5, at most 2 per test), the last step's
                logits agree within 1e-4 · max|logits|, status is 0 and "step" is n + k.
The oracle's state after a prompt is computed once per case and shared by both execution forms."""
import copy
import os

import numpy as np
import pytest
import torch

from lbwn.arch import load_arch, normalize_arch
from oracle import wavenet_ref as R
from tests.conftest import ROOT
from tests.test_gpu_gen import _near_tie, form, make_gen, small  # noqa: F401  (form is a fixture)

pytestmark = pytest.mark.gpu

RING_BAR = 5e-5
SEED = 7            # make_gen's default
_ORACLE = {}        # case -> the oracle's rings after the prompt (never modified: generate copies init_rings)


def oracle_state(case, arch, P, B, prompt, gc=None, pre_bias=True):
    if case not in _ORACLE:
        p2 = np.broadcast_to(prompt, (B, prompt.shape[-1]))
        _ORACLE[case] = R.generate(arch, P, B, p2.shape[1], seed=SEED, forced_q=p2, gc_ids=gc, pre_bias=pre_bias,
                                   return_state=True)[-1]
    return _ORACLE[case]


def ring_error(g, rings_ref, streams=None):
    """max over layers of max|GPU ring - oracle ring| / max|oracle ring of the layer| (over `streams`)."""
    flat = g.tensor('rings').cpu().numpy().astype(np.float64)
    B, Cr = g.batch_sz, g.arch['n_res']
    worst, off = 0.0, 0
    for r in rings_ref:
        d = r.shape[1]
        got = flat[off:off + B * d * Cr].reshape(B, d, Cr)
        off += B * d * Cr
        sel = slice(None) if streams is None else streams
        worst = max(worst, float(np.abs(got[sel] - r[sel]).max() / np.abs(r).max()))
    assert off == flat.size
    return worst


def sequential_ring_error(arch, B, prompt, rings_ref, gc=None, pre_bias=True):
    """The parent's teacher path (one step at a time, shared teacher vector) on the same prompt: a
    shared prompt is one run; per-stream prompts take one run per stream, of which stream b is read
    (streams are independent)."""
    n = prompt.shape[-1]
    worst = 0.0
    for b in ([None] if prompt.ndim == 1 else range(B)):
        g, _ = make_gen(arch, B, chunk=n, graph=False, pre_bias=pre_bias)
        g.teacher_mu = torch.as_tensor(prompt if b is None else prompt[b], device='cuda')
        g.build_graph(n)
        g.run(n, gc_ids=gc)
        torch.cuda.synchronize()
        g.check_status()
        worst = max(worst, ring_error(g, rings_ref, None if b is None else [b]))
    return worst


def check_free_steps(g, ref_call, t_first, k):
    """Draws of steps t_first .. t_first+k-1 against ref_call(forced_q) -> (samples, wav, logits) over
    exactly those steps."""
    got = g.samples().cpu().numpy()[:, t_first:t_first + k]
    ref, _, lg = ref_call(got)
    bad = np.argwhere(got != ref)
    ties = [(int(b), int(i)) for b, i in bad if _near_tie(lg[b, i], R.philox_uniform(SEED, int(b), t_first + int(i)))]
    assert len(ties) == len(bad), 'draws differ away from a CDF tie at (stream, step) %s' % (
        [(int(b), t_first + int(i)) for b, i in bad[:8]],)
    assert len(bad) <= 2, bad.tolist()
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())
    return len(bad)


def prefill_from_zero(case, form, arch, B, prompt, k, gc=None, pre_bias=True, chunk=16, graph=False, yardstick=True):
    """gen_start, prefill(prompt) at step 0, k free steps; both bars.  Returns the generator."""
    n = prompt.shape[-1]
    g, P = make_gen(arch, B, chunk=chunk, pre_bias=pre_bias, graph=graph)
    g.build_graph(n + k)
    g.init_buffers(gc)
    assert g.prefill(prompt) == n
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n
    rings_ref = oracle_state(case, arch, P, B, prompt, gc, pre_bias)
    err = ring_error(g, rings_ref)
    print('%s [%s]: prefill ring error %.3g' % (case, form, err))
    if yardstick:
        seq = sequential_ring_error(arch, B, prompt, rings_ref, gc, pre_bias)
        print('%s [%s]: sequential teacher path ring error %.3g' % (case, form, seq))
        assert seq <= RING_BAR, 'the sequential path itself is outside the bar: %g' % seq
    assert err <= RING_BAR, err
    p2 = np.broadcast_to(prompt, (B, n))
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], p2)
    if k:
        g.step(k)
        torch.cuda.synchronize()
        g.check_status()
        assert int(g.tensor('step', torch.int64).item()) == n + k
        check_free_steps(g, lambda fq: R.generate(
            arch, P, B, k, seed=SEED, return_logits=True, forced_q=fq, start=n, init_rings=copy.deepcopy(rings_ref),
            init_q=p2[:, -1], gc_ids=gc, pre_bias=pre_bias), n, k)
    return g


@pytest.mark.parametrize('pre_bias', [True, False])
def test_prefill_sub_dilation_slices(pre_bias, form, monkeypatch):
    """Slices of 5 positions: ragged (37 = 7 x 5 + 2), T_s < d for d = 8 (the ring write aliases the
    slots the halo copy reads), several ring wraps, -1 as the pending input, per-stream prompts."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    B, n, k = 3, 37, 27
    prompt = np.random.default_rng(11).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('sub_dilation_%d' % pre_bias, form, small(), B, prompt, k, pre_bias=pre_bias)


def test_prefill_default_slice_shared_prompt(form, monkeypatch):
    """One slice of the default length, one prompt shared by the streams (ld_codes = 0); the outputs
    of the prefilled steps are the prompt and its µ-law decode."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    B, n, k = 3, 37, 27
    prompt = np.random.default_rng(12).integers(0, 256, n).astype(np.int32)
    g = prefill_from_zero('default_shared', form, small(), B, prompt, k)
    wav = g.tensor('wav').view(B, g.max_steps).cpu().numpy()[:, :n]
    want = np.broadcast_to(R.mu_decode_tf32(prompt, 256), (B, n))
    np.testing.assert_allclose(wav, want, rtol=1e-6, atol=1e-6)


def test_prefill_global_conditioning(form, monkeypatch):
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '16')
    B, n, k = 2, 37, 27
    prompt = np.random.default_rng(13).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('gc', form, small(gc=5), B, prompt, k, gc=[2, 5])


def test_prefill_arch2_widths_gc(form, monkeypatch):
    """par/arch2.json's widths (n_res 3, n_dil 4, n_skip 8, n_post 6) with GC: the scalar row copies
    and the per-stream GC table of 2·n_dil columns; the rings against the oracle."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '16')
    arch = normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=3, n_dil=4, n_skip=8, n_post=6,
                               n_gc_embed=8, n_gc_category=5, use_bias=True))
    B, n = 2, 37
    prompt = np.random.default_rng(14).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('arch2_gc', form, arch, B, prompt, 0, gc=[2, 5], yardstick=False)


def test_prefill_mid_run_two_groups(form, monkeypatch):
    """B = 20 (two persistent stream groups): 20 free steps, 30 prefilled per-stream codes in slices
    of 16, 20 more free steps, against the oracle along the composed trajectory (the samples tensor
    IS the composed forced_q: the prefilled steps store the prompt).  A missed group step counter, a
    wrong pending input at t0 > 0 or a wrong RNG step shows as a draw the oracle does not explain."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '16')
    arch = small()
    B, n0, n, k = 20, 20, 30, 20
    total = n0 + n + k
    prompt = np.random.default_rng(15).integers(0, 256, (B, n)).astype(np.int32)
    g, P = make_gen(arch, B, chunk=10, graph=False)
    g.build_graph(total)
    g.init_buffers()
    g.step(n0)
    g.prefill(prompt)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n0 + n
    traj = g.samples().cpu().numpy()[:, :n0 + n].copy()
    np.testing.assert_array_equal(traj[:, n0:], prompt)
    out = R.generate(arch, P, B, n0 + n, seed=SEED, return_logits=True, forced_q=traj, return_state=True)
    rings_gpu_err = ring_error(g, out[-1])
    print('mid_run [%s]: ring error after free + prefill %.3g' % (form, rings_gpu_err))
    assert rings_gpu_err <= RING_BAR
    g.step(k)
    torch.cuda.synchronize()
    g.check_status()
    assert int(g.tensor('step', torch.int64).item()) == total
    full = g.samples().cpu().numpy()[:, :total]
    ref, _, lg = R.generate(arch, P, B, total, seed=SEED, return_logits=True, forced_q=full)
    free = np.r_[0:n0, n0 + n:total]
    bad = [(b, i) for b in range(B) for i in free if full[b, i] != ref[b, i]]
    ties = [(b, i) for b, i in bad if _near_tie(lg[b, i], R.philox_uniform(SEED, b, int(i)))]
    assert len(ties) == len(bad), 'draws differ away from a CDF tie at (stream, step) %s' % bad[:8]
    assert len(bad) <= 2, bad
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())


def test_prefill_arch3_depth_and_slicing(form, monkeypatch):
    """arch3, all 50 layers: d = 512 > T_s = 300, three slices (300, 300, 100), more than one
    128-position tile per stream."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '300')
    arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    B, n, k = 2, 700, 40
    prompt = np.random.default_rng(16).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('arch3', form, arch, B, prompt, k, chunk=100)


def test_prefill_equals_sequential_teacher(form, monkeypatch):
    """WaveNetGen.run(prefill=True) against the sequential teacher run of the same generator: the
    same samples at steps 25..39 (near ties excepted: each run is checked against the oracle along its
    own trajectory) and, the draws being equal, final rings within the ring bar of each other."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    arch = small()
    B, nt, n = 3, 25, 40
    teacher = np.random.default_rng(17).integers(0, 256, nt).astype(np.int32)
    runs = []
    for pf in (False, True):
        g, P = make_gen(arch, B, chunk=10, graph=False)
        g.teacher_mu = torch.as_tensor(teacher, device='cuda')
        g.build_graph(n)
        g.run(n, prefill=pf)
        torch.cuda.synchronize()
        assert int(g.tensor('step', torch.int64).item()) == n
        s = g.samples().cpu().numpy()[:, :n].copy()
        if pf:
            np.testing.assert_array_equal(s[:, :nt], np.broadcast_to(teacher, (B, nt)))
        fq = np.concatenate([np.broadcast_to(teacher, (B, nt)), s[:, nt:]], axis=1)
        ref, _, lg = R.generate(arch, P, B, n, seed=SEED, return_logits=True, forced_q=fq)
        bad = [(b, i) for b in range(B) for i in range(nt, n) if s[b, i] != ref[b, i]]
        assert all(_near_tie(lg[b, i], R.philox_uniform(SEED, b, i)) for b, i in bad), bad
        assert len(bad) <= 2, bad
        runs.append((s, g.tensor('rings').cpu().numpy().astype(np.float64), len(bad)))
    (s0, r0, f0), (s1, r1, f1) = runs
    if f0 == 0 and f1 == 0:
        np.testing.assert_array_equal(s0[:, nt:], s1[:, nt:])
    if np.array_equal(s0[:, nt:], s1[:, nt:]):
        off, Cr = 0, arch['n_res']
        for l in range(R.n_layers(arch)):
            sz = B * R.layer_index(arch, l)[2] * Cr
            a, b = r0[off:off + sz], r1[off:off + sz]
            off += sz
            assert np.abs(a - b).max() <= RING_BAR * np.abs(a).max(), l


def test_prefill_then_graph_replay(form, monkeypatch):
    """After a prefill, step() through chunk-sized graph replays (chunk 10: capture + 2 replays + a
    7-step tail) continues from the prefilled state."""
    monkeypatch.delenv('LBWN_GEN_PREFILL_SLICE', raising=False)
    B, n, k = 3, 37, 37
    prompt = np.random.default_rng(18).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('replay', form, small(), B, prompt, k, chunk=10, graph=True, yardstick=False)
