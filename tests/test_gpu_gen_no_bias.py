"""The cached generator on an arch with use_bias = false, both execution forms, with the helpers
and the bars of the with-bias modules: samples equal to R.generate, wav at 1e-6, logits at
2e-4 · max|ref|, status 0.  Without biases the GEMV chain runs with in_bias = nullptr, the persistent
kernel with bsum / post1_b / draw.bias null, the MFMA head GEMMs (B > 16 per step) with
bias = nullptr, the filtered draw adds no b2, and the prefill's embed has no PRE_BIAS to add whatever
pre_bias says."""
import numpy as np
import pytest
import torch

from oracle import wavenet_ref as R
from tests import sampling_ref as S
from tests import test_gpu_gen_lc as LC
from tests import test_gpu_gen_prefill_lc as PLC
from tests.test_gpu_gen import form, make_gen, small  # noqa: F401  (form is a fixture)
from tests.test_gpu_gen_prefill import prefill_from_zero
from tests.test_gpu_gen_sampling import check_against_reference, finish, make_gen as make_gen_sampling

pytestmark = pytest.mark.gpu


def _no_bias(P):
    assert P and not any('BIAS' in n for n in P)


def test_free_running_and_pre_bias_flag(form):
    """B = 3, n = 48: the oracle's samples and wav; pre_bias True and False are bit-identical (there is
    no PRE_BIAS for the flag to add)."""
    arch = small(use_bias=False)
    B, n = 3, 48
    out = []
    for pre_bias in (True, False):
        g, P = make_gen(arch, B, chunk=16, pre_bias=pre_bias)
        _no_bias(P)
        _, wav, _ = g.run(n)
        torch.cuda.synchronize()
        assert g.persistent == (form == 'persistent')
        assert int(g.tensor('status', torch.int32).item()) == 0
        out.append((g.samples().cpu().numpy()[:, :n].copy(), wav.cpu().numpy().copy()))
    s_ref, w_ref = R.generate(arch, P, B, n, seed=7)
    np.testing.assert_array_equal(out[0][0], s_ref)
    np.testing.assert_allclose(out[0][1], w_ref[:, :out[0][1].shape[1]], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1].view(np.uint32), out[0][1].view(np.uint32))


def test_teacher_forced_with_gc(form):
    arch = small(gc=5, use_bias=False)
    B, n = 2, 40
    teacher_q = np.random.default_rng(1).integers(0, 256, 25).astype(np.int32)
    g, P = make_gen(arch, B, chunk=10)
    _no_bias(P)
    g.teacher_mu = torch.as_tensor(teacher_q, device='cuda')
    g.build_graph(n)
    gc = [2, 5]
    g.run(n, gc_ids=gc)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('status', torch.int32).item()) == 0
    s_ref, _, lg_ref = R.generate(arch, P, B, n, seed=7, teacher_q=teacher_q, gc_ids=gc, return_logits=True)
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], s_ref)
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg_ref[:, -1], rtol=0, atol=2e-4 * np.abs(lg_ref).max())


def test_large_batch(form):
    """B = 20: two persistent stream groups; per step the skip / post1 / post2 MFMA GEMMs instead of
    the GEMVs."""
    arch = small(use_bias=False)
    B, n = 20, 24
    g, P = make_gen(arch, B, chunk=8)
    _, wav, _ = g.run(n)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    s_ref, w_ref, lg_ref = R.generate(arch, P, B, n, seed=7, return_logits=True)
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], s_ref)
    np.testing.assert_allclose(wav.cpu().numpy(), w_ref[:, :wav.shape[1]], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg_ref[:, -1], rtol=0, atol=2e-4 * np.abs(lg_ref).max())


def test_local_conditioning_free_running(monkeypatch):
    """The small LC arch of tests/test_gpu_gen_lc.py (strides [2, 4]) without biases, B = 3, both
    forms (that module's own form fixture also clears LBWN_GEN_LC_CHUNK)."""
    arch = LC.small(use_bias=False)
    B, n = 3, 65
    mel = np.random.default_rng(11).standard_normal((B, 8, 12)).astype(np.float32)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    for per_step in (False, True):
        if per_step:
            monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
        else:
            monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
        g, P = LC.make_gen(arch, B, chunk=10)
        _no_bias(P)
        g.run(n, mel=mel)
        torch.cuda.synchronize()
        assert g.persistent == (not per_step)
        got = g.samples().cpu().numpy()[:, :n]
        assert len(np.unique(got)) > 16
        LC.check_run(g, LC.oracle_logits(arch, P, got, mel), n)


def test_prefill_sub_dilation_slices(form, monkeypatch):
    """Slices of 5 positions (below d = 8): a prompt of 40 codes, then 16 free steps, against the oracle
    and beside the sequential teacher path (the yardstick of tests/test_gpu_gen_prefill.py)."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    B, n, k = 3, 40, 16
    prompt = np.random.default_rng(41).integers(0, 256, (B, n)).astype(np.int32)
    prefill_from_zero('no_bias_sub_dilation', form, small(use_bias=False), B, prompt, k)


def test_prefill_local_conditioning(monkeypatch):
    """The same with a mel: 40 prefilled steps in slices of 5, free steps up to 65, both forms."""
    for v in ('LBWN_GEN_PREFILL_LC_GROUP', 'LBWN_GEN_LC_CHUNK'):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    B, n, N = 3, 40, 65
    mel = np.random.default_rng(42).standard_normal((B, 8, 12)).astype(np.float32)
    prompt = np.random.default_rng(43).integers(0, 256, (B, n)).astype(np.int32)
    for name in ('persistent', 'per_step'):
        if name == 'per_step':
            monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
        else:
            monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
        PLC.prefill_case('no_bias_lc', name, LC.small(use_bias=False), B, mel, prompt, N, monkeypatch)


@pytest.mark.parametrize('Q', [256, 100])
def test_filtered_draw(Q, form):
    """(temperature, top_k, top_p) = (0.8, 40, 0.95) at Q = 256 and at Q = 100 with two codes per lane:
    the filtered kernels add b2 themselves through draw.bias, here null."""
    setting = (0.8, 40, 0.95)
    arch = S.small(Q, use_bias=False)
    B, n = 3, 64
    g, P = make_gen_sampling(arch, S.POST2_SCALE[Q], B, 16, setting)
    _no_bias(P)
    g.run(n)
    got = finish(g, n, form == 'persistent')
    check_against_reference(g, arch, P, got, setting, 'no bias Q=%d %s' % (Q, form))
