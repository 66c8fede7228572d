"""Prompt prefill with local conditioning (lbwn_gen_prefill on LC plans) on the GPU
against the oracle's float64 TRAINING forward with the mel, as tests/test_gpu_gen_lc.py builds it.

One R.forward(..., mel=) over the final trajectory gives everything: cache['x'][l][:, p] is layer
l's input at training position p = generation step p + 1, step0() gives it for step 0.  After the
counter reaches n, ring l's slot t & (d-1) holds the input of step t for the last min(d, n) steps and
slots never written are 0; the network is causal, so the forward over the whole trajectory also
gives the state after its prefix.  Two bars, both the project's:
  rings         within RING_BAR = 5e-5 · max|oracle ring of the layer| (tests/test_gpu_gen_prefill.py)
  continuation  check_run's: status 0, the step counter, every free draw equal to the oracle's except
                at a near CDF tie (at most 2), the last step's logits within 1e-4 · max.  The prefilled
                steps store the prompt, not a draw, so only the free steps' draws are compared.
Where the prompt starts at step 0 the sequential teacher path's ring error on the same prompt and
mel is printed beside the prefill's and must itself be inside the bar."""
import os

import numpy as np
import pytest
import torch

from lbwn.arch import load_arch, normalize_arch
from oracle import wavenet_ref as R
from tests.conftest import ROOT
from tests.test_gpu_gen_lc import (SEED, _near_tie, check_run, form, make_gen,  # noqa: F401  (form is a fixture)
                                   oracle_logits, small)
from tests.test_gpu_gen_prefill import RING_BAR, ring_error

pytestmark = pytest.mark.gpu

_ORACLE = {}        # (case, trajectory) -> (logits, per-layer inputs): one float64 forward for both forms


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for v in ('LBWN_GEN_PREFILL_SLICE', 'LBWN_GEN_PREFILL_LC_GROUP'):
        monkeypatch.delenv(v, raising=False)


def oracle(case, arch, P, got, mel, monkeypatch, **kw):
    """oracle_logits over the trajectory `got` [B, n], plus X[l] [B, n, Cr] = layer l's input at every
    generation step (step 0 from step0's SAVE rows, step p + 1 from the forward's cache['x'][l][:, p])."""
    key = (case, got.tobytes())
    if key not in _ORACLE:
        seen, fwd = {}, R.forward

        def spy(a, p, wav_q, ids, save, mel=None):
            out = fwd(a, p, wav_q, ids, save, mel=mel)
            seen['x'], seen['save'] = out[1]['x'], save
            return out
        monkeypatch.setattr(R, 'forward', spy)
        lg = oracle_logits(arch, P, got, mel, monkeypatch=monkeypatch, **kw)
        monkeypatch.setattr(R, 'forward', fwd)
        X = []
        for l in range(R.n_layers(arch)):
            b, bl, d = R.layer_index(arch, l)
            X.append(np.concatenate([seen['save']['SAVE_%d_%d_%d' % (d, b, bl)][:, -1:], seen['x'][l]], axis=1))
        _ORACLE[key] = (lg, X)
    return _ORACLE[key]


def rings_at(arch, X, n):
    """The oracle's rings once the step counter is n."""
    out = []
    for l, x in enumerate(X):
        d = R.layer_index(arch, l)[2]
        r = np.zeros((x.shape[0], d, x.shape[2]))
        for t in range(max(0, n - d), n):
            r[:, t & (d - 1)] = x[:, t]
        out.append(r)
    return out


class RingSnapshot:
    """The generator's rings at one moment, for ring_error (the oracle comes after the run)."""

    def __init__(self, g):
        torch.cuda.synchronize()
        self.batch_sz, self.arch, self._r = g.batch_sz, g.arch, g.tensor('rings').clone()

    def tensor(self, name):
        assert name == 'rings'
        return self._r


def check_continuation(g, lg, n, free):
    """check_run with the draws compared at the free steps only."""
    torch.cuda.synchronize()
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    got = g.samples().cpu().numpy()[:, :n]
    bad = [(b, int(i)) for b in range(got.shape[0]) for i in free
           if got[b, i] != R.sample_from_logits(lg[b, i], R.philox_uniform(SEED, b, int(i)))]
    print('free draws %d, differing %d, max |logit| %.3f' % (got.shape[0] * len(free), len(bad), np.abs(lg).max()))
    ties = [(b, i) for b, i in bad if _near_tie(lg[b, i], R.philox_uniform(SEED, b, i))]
    assert len(ties) == len(bad), 'draws differ away from a CDF tie at (stream, step) %s' % (bad[:8],)
    assert len(bad) <= 2, bad
    err = np.abs(g.logits().cpu().numpy() - lg[:, -1]).max()
    print('last-step logits: max err %.3e (bound %.3e)' % (err, 1e-4 * np.abs(lg[:, -1]).max()))
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())
    return len(bad)


def sequential_snapshots(arch, B, prompt, mel, gc=None):
    """The parent's teacher path (one step at a time, one shared teacher vector) on the same prompt
    and mel: a shared prompt is one run, per-stream prompts one run per stream, of which stream b is
    read (streams are independent).  Returns [(snapshot, streams)]."""
    n = prompt.shape[-1]
    out = []
    for b in ([None] if prompt.ndim == 1 else range(B)):
        g, _ = make_gen(arch, B, chunk=n + 1, teacher_q=prompt if b is None else prompt[b])   # chunk > n: no graph
        g.build_graph(n)
        g.init_buffers(gc, mel=mel)
        g.step(n)
        g.check_status()
        out.append((RingSnapshot(g), None if b is None else [b]))
    return out


def prefill_case(case, form, arch, B, mel, prompt, N, monkeypatch, gc=None, clamp_rows=False, yardstick=True,
                 chunk=10, check_form=True):
    """init_buffers(mel), prefill(prompt) at step 0, free steps up to N; both bars.  Returns (g, P, X)."""
    n = prompt.shape[-1]
    g, P = make_gen(arch, B, chunk=chunk)
    g.build_graph(N)
    g.init_buffers(gc, mel=mel)
    assert g.prefill(prompt) == n
    snap = RingSnapshot(g)
    if check_form:
        assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], np.broadcast_to(prompt, (B, n)))
    seq = sequential_snapshots(arch, B, prompt, mel, gc) if yardstick else []
    g.step(N - n)
    torch.cuda.synchronize()
    got = g.samples().cpu().numpy()[:, :N]
    kw = dict(clamp_rows=True) if clamp_rows else {}
    lg, X = oracle(case, arch, P, got, mel, monkeypatch, gc=gc, **kw)
    ref = rings_at(arch, X, n)
    err = ring_error(snap, ref)
    print('%s [%s]: prefill ring error %.3g (bar %.3g)' % (case, form, err, RING_BAR))
    if seq:
        serr = max(ring_error(s, ref, streams) for s, streams in seq)
        print('%s [%s]: sequential teacher path ring error %.3g' % (case, form, serr))
        assert serr <= RING_BAR, 'the sequential path itself is outside the bar: %g' % serr
    assert err <= RING_BAR, err
    check_continuation(g, lg, N, range(n, N))
    return g, P, X


def test_prefill_lc_sub_dilation_slices(form, monkeypatch):
    """Slices of 5 positions (37 = 7 x 5 + 2, T_s < d for d = 8), layer groups 3 + 3 + 2, a cond ring
    of 4 steps for the continuation, per-stream prompts."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '5')
    monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', '3')
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    B, n, N = 3, 37, 65
    mel = np.random.default_rng(21).standard_normal((B, 8, 12)).astype(np.float32)
    prompt = np.random.default_rng(22).integers(0, 256, (B, n)).astype(np.int32)
    g, _, _ = prefill_case('sub_dilation', form, small(), B, mel, prompt, N, monkeypatch)
    assert g.tensor('pfcond').numel() == B * 5 * 3 * 64


def test_prefill_lc_and_gc(form, monkeypatch):
    """LC + GC, the default slice and the default group (all 8 layers in one launch), a shared prompt."""
    B, n, N = 2, 25, 65
    mel = np.random.default_rng(23).standard_normal((B, 8, 12)).astype(np.float32)
    prompt = np.random.default_rng(24).integers(0, 256, n).astype(np.int32)
    prefill_case('lc_gc', form, small(gc=5), B, mel, prompt, N, monkeypatch, gc=[2, 5])


@pytest.mark.parametrize('n_lc_out', [16, 88])
def test_prefill_lc_projection_alone(n_lc_out, form, monkeypatch):
    """"pfcond" after a one-slice prefill with every layer in one group against float64
    lc[b, r] @ [LC_SIGNAL_l | LC_GATE_l], within 1e-5 · max|ref| (the bar the upsampled mel is held to);
    the step path's "lccond" over the same steps is measured against the same reference and the two
    GPU results are compared bit for bit (printed, not asserted).  n_lc_out = 88 takes two k passes."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', '8')
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '64')
    arch = normalize_arch(dict(small(), n_lc_out=n_lc_out))
    B, n, L, Cd = 3, 37, 8, 32
    mel = np.random.default_rng(25).standard_normal((B, 8, 12)).astype(np.float32)
    prompt = np.random.default_rng(26).integers(0, 256, (B, n)).astype(np.int32)
    g, P = make_gen(arch, B, chunk=n + 1)
    g.build_graph(65)
    g.init_buffers(mel=mel)
    g.prefill(prompt)
    torch.cuda.synchronize()
    pf = g.tensor('pfcond')[:B * n * L * 2 * Cd].view(B, n, L, 2 * Cd).cpu().numpy()
    lc, _ = R.lc_upsample_fwd(arch, P, mel.astype(np.float64))
    rows = np.clip(np.arange(n) - 1, 0, lc.shape[1] - 1)
    ref = np.empty((B, n, L, 2 * Cd))
    for l in range(L):
        sfx = '_%d_%d' % R.layer_index(arch, l)[:2]
        ref[:, :, l] = lc[:, rows] @ np.concatenate([P['LC_SIGNAL' + sfx], P['LC_GATE' + sfx]], axis=1)
    bar = 1e-5 * np.abs(ref).max()
    err = np.abs(pf - ref).max()
    g2, _ = make_gen(arch, B, chunk=n + 1)
    g2.build_graph(65)
    g2.init_buffers(mel=mel)
    g2.step(n)                                             # one sub-run: steps 0..n-1 in slots 0..n-1
    torch.cuda.synchronize()
    sp = g2.tensor('lccond').view(64, L, B, 64)[:n].permute(2, 0, 1, 3).cpu().numpy()
    print('projection [%s, n_lc_out %d]: prefill err %.3e, step path err %.3e (bar %.3e), bitwise equal: %s'
          % (form, n_lc_out, err, np.abs(sp - ref).max(), bar, np.array_equal(sp, pf)))
    assert err <= bar, (err, bar)


def test_prefill_lc_mel_matters_and_reload(form, monkeypatch):
    """Streams 0 and 1 share a mel and the prompt: bitwise equal rings; stream 2 has another mel: its
    rings differ.  A second init_buffers with a second mel on the same plan: the rings follow it."""
    arch = small()
    B, n, N = 3, 37, 65
    rng = np.random.default_rng(27)
    m2 = rng.standard_normal((2, 8, 12)).astype(np.float32)
    mel_a = np.stack([m2[0], m2[0], m2[1]])
    mel_b = rng.standard_normal((B, 8, 12)).astype(np.float32)
    prompt = rng.integers(0, 256, n).astype(np.int32)
    traj = np.concatenate([np.broadcast_to(prompt, (B, n)), np.zeros((B, N - n), np.int32)], axis=1)   # causal: any tail
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(N)
    for name, mel in (('a', mel_a), ('b', mel_b)):
        g.init_buffers(mel=mel)
        g.prefill(prompt)
        snap = RingSnapshot(g)
        _, X = oracle('reload_' + name, arch, P, traj, mel, monkeypatch)
        ref = rings_at(arch, X, n)
        err = ring_error(snap, ref)
        print('mel %s [%s]: prefill ring error %.3g' % (name, form, err))
        assert err <= RING_BAR, err
        if name == 'a':
            flat, off = snap.tensor('rings').cpu().numpy(), 0
            differ = 0.0
            for r in ref:
                d = r.shape[1]
                got = flat[off:off + B * d * 32].reshape(B, d, 32)
                off += B * d * 32
                np.testing.assert_array_equal(got[0], got[1])
                differ = max(differ, np.abs(got[0] - got[2]).max() / np.abs(r).max())
            assert differ > 1e-3, differ


def test_prefill_lc_mid_run_two_groups(form, monkeypatch):
    """B = 20 (two persistent stream groups): 20 free steps, 30 prefilled per-stream codes in slices of
    16, 15 free steps, along the composed trajectory.  A mel row taken from `off` instead of
    t0 + off shows here."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '16')
    arch = small()
    B, n0, n, N = 20, 20, 30, 65
    mel = np.random.default_rng(28).standard_normal((B, 8, 12)).astype(np.float32)
    prompt = np.random.default_rng(29).integers(0, 256, (B, n)).astype(np.int32)
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(N)
    g.init_buffers(mel=mel)
    g.step(n0)
    assert g.prefill(prompt) == n
    snap = RingSnapshot(g)
    assert g.persistent == (form == 'persistent')
    assert int(g.tensor('step', torch.int64).item()) == n0 + n
    g.step(N - n0 - n)
    torch.cuda.synchronize()
    got = g.samples().cpu().numpy()[:, :N]
    np.testing.assert_array_equal(got[:, n0:n0 + n], prompt)
    lg, X = oracle('mid_run', arch, P, got, mel, monkeypatch)
    err = ring_error(snap, rings_at(arch, X, n0 + n))
    print('mid_run [%s]: ring error after free + prefill %.3g' % (form, err))
    assert err <= RING_BAR, err
    check_continuation(g, lg, N, np.r_[0:n0, n0 + n:N])


def test_prefill_lc_clamp_past_the_mel(form, monkeypatch):
    """Below the Python length check: 4 frames = 32 rows, 45 prefilled steps and 10 free ones.  Steps
    past row 31 reuse it: a forward whose upsampled mel has its last row repeated."""
    B, n, N = 3, 45, 55
    mel = np.random.default_rng(30).standard_normal((B, 4, 12)).astype(np.float32)
    prompt = np.random.default_rng(31).integers(0, 256, (B, n)).astype(np.int32)
    prefill_case('clamp', form, small(), B, mel, prompt, N, monkeypatch, clamp_rows=True)


def test_prefill_lc_arch5_as_shipped(form, monkeypatch):
    """par/arch5.json (50 layers, LC 80 -> 80, hop 256, GC 16): 450 prefilled steps in slices of 300
    with the default group (6 x 8 + 2 layers), d = 512 > T_s, then 63 free steps."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '300')
    arch = load_arch(os.path.join(ROOT, 'par', 'arch5.json'))
    B, n, N = 2, 450, 513
    mel = np.random.default_rng(32).standard_normal((B, 2, 80)).astype(np.float32)
    prompt = np.random.default_rng(33).integers(0, 256, (B, n)).astype(np.int32)
    g, _, _ = prefill_case('arch5', form, arch, B, mel, prompt, N, monkeypatch, gc=[38, 75], chunk=100)
    assert g.tensor('pfcond').numel() == B * 300 * 8 * 2 * arch['n_dil']


def test_prefill_lc_narrow_widths(form, monkeypatch):
    """n_res 3, n_dil 4, n_skip 8, n_post 6, LC 8 -> 4: the scalar stores of a 2·n_dil = 8 wide row,
    a 4-deep projection, groups of 3 + 3 + 2 layers."""
    monkeypatch.setenv('LBWN_GEN_PREFILL_SLICE', '16')
    monkeypatch.setenv('LBWN_GEN_PREFILL_LC_GROUP', '3')
    arch = normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=3, n_dil=4, n_skip=8, n_post=6,
                               n_gc_embed=0, n_gc_category=0, n_lc_in=8, n_lc_out=4, lc_upsample=[2, 4],
                               use_bias=True))
    B, n, N = 2, 37, 65
    mel = np.random.default_rng(34).standard_normal((B, 8, 8)).astype(np.float32)
    prompt = np.random.default_rng(35).integers(0, 256, (B, n)).astype(np.int32)
    prefill_case('narrow', form, arch, B, mel, prompt, N, monkeypatch, check_form=False)


def test_prefill_lc_run_equals_sequential_teacher(form, monkeypatch):
    """run(N, mel=, prefill=True) against run(N, mel=) of the same generator and a 25-code teacher:
    each run against the oracle along its own trajectory; where neither had a tie the continuations
    are equal and the final rings within the ring bar of each other."""
    arch = small()
    B, nt, N = 3, 25, 65
    teacher = np.random.default_rng(36).integers(0, 256, nt).astype(np.int32)
    mel = np.random.default_rng(37).standard_normal((B, 8, 12)).astype(np.float32)
    g, P = make_gen(arch, B, chunk=10, teacher_q=teacher)
    runs = []
    for pf in (False, True):
        g.run(N, mel=mel, prefill=pf)
        torch.cuda.synchronize()
        s = g.samples().cpu().numpy()[:, :N].copy()
        if pf:
            np.testing.assert_array_equal(s[:, :nt], np.broadcast_to(teacher, (B, nt)))
        lg, _ = oracle('run_%d' % pf, arch, P, s, mel, monkeypatch, teacher_q=teacher)
        if pf:
            bad = check_continuation(g, lg, N, range(nt, N))
        else:
            check_run(g, lg, N)                 # the teacher-forced steps store the model's ignored draws
            ref = np.array([[R.sample_from_logits(lg[b, i], R.philox_uniform(SEED, b, i)) for i in range(N)]
                            for b in range(B)])
            bad = int((s != ref).sum())
        runs.append((s, g.tensor('rings').cpu().numpy().astype(np.float64), bad))
    (s0, r0, f0), (s1, r1, f1) = runs
    if f0 == 0 and f1 == 0:
        np.testing.assert_array_equal(s0[:, nt:], s1[:, nt:])
    if np.array_equal(s0[:, nt:], s1[:, nt:]):
        off = 0
        for l in range(R.n_layers(arch)):
            sz = B * R.layer_index(arch, l)[2] * arch['n_res']
            a, b = r0[off:off + sz], r1[off:off + sz]
            off += sz
            assert np.abs(a - b).max() <= RING_BAR * np.abs(a).max(), l


def test_generate_cli_teacher_prefill_with_mel(tmp_path):
    """generate.py --mel-npy --teacher-wav --teacher-prefill on a small LC arch: the wav starts with
    the µ-law-quantised teacher and continues with the checkpoint's draws for that mel."""
    import json
    import sys

    from scipy.io import wavfile
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import generate
    from lbwn.ckpt import ckpt_file, save_tensors
    from lbwn.ops import mu_encode
    arch = small()
    B, nt = 2, 25
    g, P = make_gen(arch, B, chunk=10)
    pfx = str(tmp_path / 'ck' / 'net')
    save_tensors(ckpt_file(pfx), g.vars)
    (tmp_path / 'arch.json').write_text(json.dumps(dict(arch, wav_input_type='mu_law_quant')))
    rng = np.random.default_rng(38)
    teacher = (0.5 * np.sin(np.arange(nt) * 0.7) + 0.05 * rng.standard_normal(nt)).astype(np.float32)
    wavfile.write(tmp_path / 'teacher.wav', 16000, teacher)
    mel = rng.standard_normal((B, 10, 12)).astype(np.float32)          # 80 rows cover 81 steps
    np.save(tmp_path / 'mel.npy', mel)
    wav = generate.main(['--mel-npy', str(tmp_path / 'mel.npy'), '--teacher-wav', str(tmp_path / 'teacher.wav'),
                         '--teacher-prefill', '--gen-seconds', '0.003', '--batch-size', str(B), '--chunk-size', '5',
                         '--seed', str(SEED), str(tmp_path / 'arch.json'), pfx, str(tmp_path / 'out')])
    assert wav.shape == (B, 70) and np.all(np.abs(wav) <= 1.03)          # 25 + 48 = 73 steps, whole chunks of 5
    for i in range(B):
        assert os.path.exists(tmp_path / 'out' / ('gen.i%d.wav' % i))
    table = R.mu_decode_np(np.arange(256), 256)
    q = np.abs(wav[:, :65, None].astype(np.float64) - table).argmin(axis=2)       # the codes behind the wav
    tq = mu_encode(torch.as_tensor(teacher, device='cuda'), 256).cpu().numpy()
    np.testing.assert_array_equal(q[:, :nt], np.broadcast_to(tq, (B, nt)))
    lg = oracle_logits(arch, P, q, mel[:, :8])
    bad = [(b, i) for b in range(B) for i in range(nt, 65)
           if q[b, i] != R.sample_from_logits(lg[b, i], R.philox_uniform(SEED, b, i))]
    assert all(_near_tie(lg[b, i], R.philox_uniform(SEED, b, i)) for b, i in bad) and len(bad) <= 2, bad
