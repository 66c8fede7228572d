"""Teacher-forced scoring (lbwn_gen_score) on the GPU against the oracle.

Reference: the oracle's float64 logits l along the prompt (R.generate(forced_q=prompt, return_logits=True);
LC archs: oracle_logits of tests/test_gpu_gen_lc.py), ref = l[c] - logsumexp(l).
Bar: |logp - ref| <= 2e-4 · max|l_ref|.  Derived, not measured: the project holds GPU logits to
1e-4 · max|logits| in the max norm; logp is one logit (error <= 1e-4 · max) minus a logsumexp, which is
1-Lipschitz in the max norm (error <= 1e-4 · max).  The last scored step's "logits" are held to the
project's own 1e-4 · max.  Beside the observed error every case prints the error of the sequential teacher
path's logits() at the last step, the code this call replaces.
The oracle's logits are computed once per case and shared by both execution forms."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.arch import load_arch, normalize_arch
from oracle import wavenet_ref as R
from tests import test_gpu_gen_lc as LC
from tests.conftest import ROOT
from tests.test_gpu_gen import form, make_gen, small  # noqa: F401  (form is a fixture)
from tests.test_gpu_gen_prefill import SEED, check_free_steps

pytestmark = pytest.mark.gpu

LOGP_BAR = 2e-4
LOGIT_BAR = 1e-4
_ORACLE = {}        # case -> float64 logits (and state) along the prompt; never modified


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for v in ('LBWN_GEN_PREFILL_SLICE', 'LBWN_GEN_PREFILL_LC_GROUP', 'LBWN_GEN_LC_CHUNK'):
        monkeypatch.delenv(v, raising=False)


def cached(case, fn):
    if case not in _ORACLE:
        _ORACLE[case] = fn()
    return _ORACLE[case]


def ref_logp(lg, codes):
    """l[c] - logsumexp(l) in float64; lg [B, n, Q], codes int [B, n] inside [0, Q)."""
    m = lg.max(axis=-1)
    lse = m + np.log(np.exp(lg - m[..., None]).sum(axis=-1))
    return np.take_along_axis(lg, np.asarray(codes, np.int64)[..., None], axis=-1)[..., 0] - lse


def check_logp(case, form, logp, lg, codes, g=None, seq=None):
    """The logp bar (and, given the generator, the last step's logits at the project's bar); prints the
    observed error and the sequential teacher path's last-step logits error beside it."""
    got = logp.detach().cpu().numpy().astype(np.float64)
    B, n = lg.shape[:2]
    codes = np.broadcast_to(np.clip(codes, 0, lg.shape[2] - 1), (B, n))
    assert got.shape == (B, n)
    scale = np.abs(lg).max()
    err = np.abs(got - ref_logp(lg, codes)).max()
    print('%s [%s]: logp error %.3g (bar %.3g, max|l| %.3g)' % (case, form, err, LOGP_BAR * scale, scale))
    if seq is not None:
        print('%s [%s]: sequential teacher path last-step logits error %.3g' % (case, form, seq))
    if g is not None:
        lerr = np.abs(g.logits().cpu().numpy() - lg[:, -1]).max()
        print('%s [%s]: last-step logits error %.3g (bar %.3g)' % (case, form, lerr, LOGIT_BAR * scale))
        assert lerr <= LOGIT_BAR * scale, lerr
    assert np.isfinite(got).all()
    assert err <= LOGP_BAR * scale, err


def sequential_last_logits_error(arch, B, prompt, lg, gc=None, pre_bias=True, streams=None):
    """The sequential teacher path (one step per code, one shared teacher vector) on the same prompt:
    max |logits() - l_{n-1}| after its n steps.  Per-stream prompts take one run per stream read."""
    n = prompt.shape[-1]
    worst = 0.0
    for b in ([None] if prompt.ndim == 1 else (range(B) if streams is None else streams)):
        g, _ = make_gen(arch, B, chunk=n, graph=False, pre_bias=pre_bias)
        g.teacher_mu = torch.as_tensor(prompt if b is None else prompt[b], device='cuda')
        g.build_graph(n)
        g.run(n, gc_ids=gc)
        torch.cuda.synchronize()
        g.check_status()
        sel = slice(None) if b is None else [b]
        worst = max(worst, float(np.abs(g.logits().cpu().numpy()[sel] - lg[sel, n - 1]).max()))
    return worst


def oracle_from_zero(case, arch, P, B, prompt, gc=None, pre_bias=True):
    p2 = np.broadcast_to(np.clip(prompt, 0, arch['n_quant'] - 1), (B, prompt.shape[-1]))
    return cached(case, lambda: R.generate(arch, P, B, p2.shape[1], seed=SEED, forced_q=p2, gc_ids=gc,
                                           pre_bias=pre_bias, return_logits=True)[2])


def score_from_zero(case, form, arch, B, prompt, gc=None, pre_bias=True, seq_streams=None, extra=0):
    """gen_start, score(prompt) at step 0 against the oracle.  Returns (generator, P, logp, logits)."""
    n = prompt.shape[-1]
    g, P = make_gen(arch, B, chunk=16, pre_bias=pre_bias, graph=False)
    g.build_graph(n + extra)
    g.init_buffers(gc)
    logp = g.score(prompt)
    torch.cuda.synchronize()
    g.check_status()
    assert g.persistent == (form == 'persistent')
    assert logp.dtype == torch.float32 and tuple(logp.shape) == (B, n) and logp.is_cuda
    assert int(g.tensor('step', torch.int64).item()) == n
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n],
                                  np.broadcast_to(np.clip(prompt, 0, arch['n_quant'] - 1), (B, n)))
    lg = oracle_from_zero(case, arch, P, B, prompt, gc, pre_bias)
    seq = sequential_last_logits_error(arch, B, np.clip(prompt, 0, arch['n_quant'] - 1), lg, gc, pre_bias,
                                       seq_streams)
    check_logp(case, form, logp, lg, prompt, g, seq)
    return g, P, logp, lg


@pytest.mark.parametrize('pre_bias', [True, False])
def test_score_sub_dilation_slices(pre_bias, form, monkeypatch):
    """Slices of 5 positions: 37 = 7 x 5 + 2 (a ragged last slice of B·2 = 6 rows: a partial block of the
    log-softmax kernel), T_s < d for d = 8, per-stream prompts, both pre_bias values."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    B, n = 3, 37
    prompt = np.random.default_rng(21).integers(0, 256, (B, n)).astype(np.int32)
    score_from_zero('sub_dilation_%d' % pre_bias, form, small(), B, prompt, pre_bias=pre_bias)


def test_score_shared_prompt_and_padded_logp(form, monkeypatch):
    """ld_codes = 0 (one prompt for every stream) through the C entry with ld_logp = n + 5: the columns past
    n keep their sentinel."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    B, n, pad = 3, 37, 5
    prompt = np.random.default_rng(22).integers(0, 256, n).astype(np.int32)
    g, P = make_gen(arch, B, chunk=16, graph=False)
    g.build_graph(n)
    g.init_buffers()
    codes = torch.as_tensor(prompt, device='cuda')
    scratch = torch.empty(g.lib.lbwn_gen_score_scratch_bytes(g._plan), dtype=torch.uint8, device='cuda')
    out = torch.full((B, n + pad), 7.5, dtype=torch.float32, device='cuda')
    _lib.check(g.lib.lbwn_gen_score(g._plan, ctypes.byref(g._params_c), g._ws.data_ptr(), codes.data_ptr(), 0, n,
                                    out.data_ptr(), n + pad, scratch.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    g.check_status()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n
    assert bool((out[:, n:] == 7.5).all())
    lg = oracle_from_zero('shared', arch, P, B, prompt)
    seq = sequential_last_logits_error(arch, B, prompt, lg)
    check_logp('shared', form, out[:, :n], lg, prompt, g, seq)
    # the wrapper on the same shared prompt: the same numbers
    g.init_buffers()
    assert torch.equal(g.score(prompt), out[:, :n])


def test_score_gc_two_groups(form, monkeypatch):
    """GC arch, B = 20: two persistent stream groups (their counters advance with the score), or per step
    the GEMM form; 60 rows per slice of 3."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '3')
    B, n, k = 20, 14, 6
    gc = [1 + b % 5 for b in range(B)]
    arch = small(gc=5)
    prompt = np.random.default_rng(23).integers(0, 256, (B, n)).astype(np.int32)
    g, P, _, _ = score_from_zero('gc_groups', form, arch, B, prompt, gc=gc, seq_streams=[0, 19], extra=k)
    st = cached('gc_groups_state', lambda: R.generate(arch, P, B, n, seed=SEED, forced_q=prompt, gc_ids=gc,
                                                      return_state=True)[-1])
    g.step(k)
    torch.cuda.synchronize()
    g.check_status()
    check_free_steps(g, lambda fq: R.generate(arch, P, B, k, seed=SEED, return_logits=True, forced_q=fq, start=n,
                                              init_rings=copy.deepcopy(st), init_q=prompt[:, -1], gc_ids=gc), n, k)


def test_score_mid_run(form, monkeypatch):
    """11 free steps, 23 scored codes in slices of 5, 9 more free steps.  logp against the oracle resumed
    from its own state after the free steps (start, init_rings, init_q); the continuation through
    check_free_steps from the oracle's state after the scored codes."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    B, n0, n, k = 3, 11, 23, 9
    prompt = np.random.default_rng(24).integers(0, 256, (B, n)).astype(np.int32)
    g, P = make_gen(arch, B, chunk=16, graph=False)
    g.build_graph(n0 + n + k)
    g.init_buffers()
    g.step(n0)
    logp = g.score(prompt)
    torch.cuda.synchronize()
    g.check_status()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n0 + n
    traj = g.samples().cpu().numpy()[:, :n0 + n].copy()
    np.testing.assert_array_equal(traj[:, n0:], prompt)
    rings0 = R.generate(arch, P, B, n0, seed=SEED, forced_q=traj[:, :n0], return_state=True)[-1]
    _, _, lg, rings1 = R.generate(arch, P, B, n, seed=SEED, forced_q=prompt, start=n0, init_rings=rings0,
                                  init_q=traj[:, n0 - 1], return_logits=True, return_state=True)
    check_logp('mid_run', form, logp, lg, prompt, g)
    g.step(k)
    torch.cuda.synchronize()
    g.check_status()
    assert int(g.tensor('step', torch.int64).item()) == n0 + n + k
    check_free_steps(g, lambda fq: R.generate(arch, P, B, k, seed=SEED, return_logits=True, forced_q=fq, start=n0 + n,
                                              init_rings=copy.deepcopy(rings1), init_q=prompt[:, -1]), n0 + n, k)


def test_score_local_conditioning(form, monkeypatch):
    """LC + GC: 8 frames x hop 8, n = 65 (step t on lc row max(t - 1, 0)), slices of 5, projection groups of
    3 layers."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', '3')
    arch = LC.small(gc=5)
    B, n = 3, 65
    gc = [2, 5, 1]
    rng = np.random.default_rng(25)
    mel = rng.standard_normal((B, 8, arch['n_lc_in'])).astype(np.float32)
    prompt = rng.integers(0, 256, (B, n)).astype(np.int32)
    g, P = LC.make_gen(arch, B, chunk=10)
    g.build_graph(n)
    g.init_buffers(gc, mel=mel)
    logp = g.score(prompt)
    torch.cuda.synchronize()
    g.check_status()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n
    lg = cached('lc', lambda: LC.oracle_logits(arch, P, prompt, mel, gc=gc))
    worst = 0.0
    for b in range(B):      # the sequential teacher path, stream b of a run on prompt[b]
        s, _ = LC.make_gen(arch, B, chunk=n + 1, teacher_q=prompt[b])
        s.build_graph(n)
        s.init_buffers(gc, mel=mel)
        s.step(n)
        torch.cuda.synchronize()
        s.check_status()
        worst = max(worst, float(np.abs(s.logits().cpu().numpy()[b] - lg[b, n - 1]).max()))
    check_logp('lc', form, logp, lg, prompt, g, worst)


@pytest.mark.parametrize('use_bias', [True, False])
def test_score_n_quant_100(use_bias, form, monkeypatch):
    """n_quant = 100: 25 float4 per row, lanes 25..63 of the log-softmax idle; without biases the GEMMs run
    with null bias pointers and no Σ SKIP_BIAS."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = normalize_arch(dict(small(use_bias=use_bias), n_quant=100))
    B, n = 3, 37
    prompt = np.random.default_rng(26).integers(0, 100, (B, n)).astype(np.int32)
    _, P, _, _ = score_from_zero('q100_%d' % use_bias, form, arch, B, prompt)
    assert use_bias or not any('BIAS' in name for name in P)


@pytest.mark.parametrize('B', [3, 20])
def test_score_leaves_the_state_of_a_prefill(B, form, monkeypatch):
    """Two generators built alike, 5 free steps, then score(prompt) on one and prefill(prompt) on the other:
    the snapshot (rings, pending codes, step), "rings", "step", samples and wav of the prompt are bitwise
    equal, and k free steps after each draw identical samples (B = 20: both groups' counters)."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    n0, n, k = 5, 37, 12
    prompt = np.random.default_rng(27).integers(0, 256, (B, n)).astype(np.int32)
    gens = []
    for how in ('score', 'prefill'):
        g, _ = make_gen(arch, B, chunk=16, graph=False)
        g.build_graph(n0 + n + k)
        g.init_buffers()
        g.step(n0)
        getattr(g, how)(prompt)
        torch.cuda.synchronize()
        g.check_status()
        assert g.persistent == (form == 'persistent')
        gens.append(g)
    a, b = gens
    assert torch.equal(a.save_state().blob, b.save_state().blob)
    assert torch.equal(a.tensor('rings').view(torch.int32), b.tensor('rings').view(torch.int32))
    assert int(a.tensor('step', torch.int64).item()) == int(b.tensor('step', torch.int64).item()) == n0 + n
    assert torch.equal(a.samples()[:, :n0 + n], b.samples()[:, :n0 + n])
    wa, wb = (x.tensor('wav').view(B, x.max_steps)[:, :n0 + n].view(torch.int32) for x in gens)
    assert torch.equal(wa, wb)
    for g in gens:
        g.step(k)
        torch.cuda.synchronize()
        g.check_status()
    assert torch.equal(a.samples(), b.samples())
    assert torch.equal(a.tensor('rings').view(torch.int32), b.tensor('rings').view(torch.int32))


def test_score_graph_capture(form, monkeypatch):
    """A captured score replayed after init_buffers gives the eager call's logp bitwise (t0 is read on the
    device; nothing in the call synchronises or allocates)."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    B, n = 3, 37
    prompt = torch.as_tensor(np.random.default_rng(28).integers(0, 256, (B, n)).astype(np.int32), device='cuda')
    g, _ = make_gen(arch, B, chunk=16, graph=False)
    g.build_graph(n)
    g.init_buffers()
    eager = g.score(prompt).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = g.score(prompt)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        g.init_buffers()
        out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        g.check_status()
        assert int(g.tensor('step', torch.int64).item()) == n
        assert torch.equal(out, eager)


def test_score_without_advancing(form, monkeypatch):
    """save_state, score, load_state, score: the same logp twice, bitwise, with the step counter back where
    it was in between."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    B, n0, n = 3, 7, 23
    prompt = np.random.default_rng(29).integers(0, 256, (B, n)).astype(np.int32)
    g, _ = make_gen(arch, B, chunk=16, graph=False)
    g.build_graph(n0 + n)
    g.init_buffers()
    g.step(n0)
    state = g.save_state()
    first = g.score(prompt)
    assert int(g.tensor('step', torch.int64).item()) == n0 + n
    g.load_state(state)
    assert int(g.tensor('step', torch.int64).item()) == n0
    second = g.score(prompt)
    torch.cuda.synchronize()
    g.check_status()
    assert int(g.tensor('step', torch.int64).item()) == n0 + n
    assert first.data_ptr() != second.data_ptr()
    assert torch.equal(first, second)


def test_score_clamps_codes(form, monkeypatch):
    """Codes outside [0, Q) are clamped into it: logp is that of the clamped prompt, bitwise, and meets the
    oracle's along the clamped prompt."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    arch = small()
    B, n = 3, 21
    prompt = np.random.default_rng(30).integers(0, 256, (B, n)).astype(np.int32)
    prompt[0, 3], prompt[1, 0], prompt[2, n - 1], prompt[1, 9] = -3, 300, 256, -2 ** 31
    g, _, logp, _ = score_from_zero('clamp', form, arch, B, prompt)
    g.init_buffers()
    assert torch.equal(g.score(np.clip(prompt, 0, 255)), logp)


def test_score_default_slice_arch3(form):
    """arch3 at the default slice length (3200 positions at B = 10, one slice of 3000 rows, the default
    scratch of 369 MB): status 0, finite logp, exp(logp) <= 1."""
    arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    B, n = 10, 300
    prompt = np.random.default_rng(31).integers(0, 256, (B, n)).astype(np.int32)
    g, _ = make_gen(arch, B, chunk=100, graph=False)
    g.build_graph(n)
    g.init_buffers()
    assert g.lib.lbwn_gen_score_scratch_bytes(g._plan) == 32000 * 2880 * 4
    logp = g.score(prompt)
    torch.cuda.synchronize()
    g.check_status()
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    got = logp.cpu().numpy()
    assert np.isfinite(got).all()
    assert (np.exp(got.astype(np.float64)) <= 1.0).all()
    print('arch3 default slice [%s]: mean -logp %.4f nats' % (form, -got.mean()))


def test_generate_score_teacher_end_to_end(tmp_path, capsys):
    """generate.py --score-teacher --score-npy: the teacher wav's codes are scored (one stderr line per
    stream, the saved [B, n] array inside the logp bar of the oracle's) and generation continues as under
    --teacher-prefill (the output starts with the µ-law-quantised teacher)."""
    import json
    import generate
    from scipy.io import wavfile
    from lbwn.tmodel import WaveNetTrain
    arch = small()
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(arch))
    tr = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, ckpt_path=str(tmp_path / 'g.net'))
    tr.init_vars(5, bias_scale=0.2)
    with torch.no_grad():
        tr.vars['POST2'].mul_(4.0)
    tr.save(1)
    t = np.arange(160) / 16000.0
    x = 0.6 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 530 * t)
    wavfile.write(str(tmp_path / 'teach.wav'), 16000, (x * 32767).astype(np.int16))
    B, n = 2, 160
    total = (int((0.003 + n / 16000) * 16000) // 100) * 100       # whole chunks, as generate.py returns them
    wav = generate.main(['--teacher-wav', str(tmp_path / 'teach.wav'), '--score-teacher', '--score-npy',
                         str(tmp_path / 'logp.npy'), '--gen-seconds', '0.003', '--batch-size', str(B),
                         '--chunk-size', '100', str(af), str(tmp_path / 'g.net-1'), str(tmp_path / 'out')])
    err = capsys.readouterr().err
    assert wav.shape == (B, total)
    tq = R.mu_encode_tf32(generate.load_teacher(str(tmp_path / 'teach.wav'), 16000), 256)
    np.testing.assert_allclose(wav[:, :n], np.broadcast_to(R.mu_decode_tf32(tq, 256), (B, n)), rtol=1e-6, atol=1e-6)
    logp = np.load(str(tmp_path / 'logp.npy'))
    assert logp.dtype == np.float32 and logp.shape == (B, n)
    P = {k: v.cpu().double().numpy() for k, v in tr.vars.items()}
    lg = R.generate(arch, P, B, n, seed=0, forced_q=np.broadcast_to(tq, (B, n)), return_logits=True)[2]
    check_logp('cli', 'default', torch.from_numpy(logp), lg, tq)
    for i in range(B):
        nats = -float(logp[i].mean())
        assert 'score stream %d: %d codes, mean -logp %.6f nats, %.6f bits per sample' % (
            i, n, nats, nats / np.log(2.0)) in err
