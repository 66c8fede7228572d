"""Cached generation with local conditioning (a mel) on the GPU, checked against the oracle's
TRAINING forward (oracle.forward(..., mel=)) along the GPU's own trajectory: generation step i
(input: sample i-1) is training position i-1 and is conditioned on row max(i-1, 0) of the
upsampled mel, so forward() over wav_q = the inputs of steps 1..n-1, with SAVE_l = [0 .. 0, g_l]
(g_l = layer l's input at step 0), gives the float64 logits every draw i >= 1 was taken from;
step 0 (zero input, mel row 0) comes from the same helper that builds g_l.  Acceptance as
tests/test_gpu_gen.py::test_gen_arch3_full_ring_depth."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from lbwn.arch import load_arch, normalize_arch
from lbwn.imodel import WaveNetGen
from lbwn.tmodel import WaveNetTrain
from oracle import wavenet_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
SEED = 7


@pytest.fixture(params=['persistent', 'per_step'])
def form(request, monkeypatch):
    """Both execution forms: the persistent one-launch kernel (one launch per sub-run of <= NC
    steps) and the per-step launches (LBWN_GEN_PERSIST=0: vector GEMVs at B <= 16, the head as
    MFMA GEMMs beyond)."""
    if request.param == 'per_step':
        monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
    else:
        monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    return request.param


def small(gc=0, use_bias=True):
    return normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64,
                               n_post=32, n_gc_embed=8 if gc else 0, n_gc_category=gc, n_lc_in=12, n_lc_out=16,
                               lc_upsample=[2, 4], use_bias=use_bias))


_PARAMS = {}


def make_gen(arch, B, chunk, teacher_q=None):
    """WaveNetGen with the parameters of WaveNetTrain.init_vars(3, bias_scale=0.2), POST2 x4 (so
    draws are not uniform noise); the float64 copy is computed once per arch and shared."""
    key = json.dumps(arch, sort_keys=True)
    if key not in _PARAMS:
        tr = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0)
        tr.init_vars(3, bias_scale=0.2)
        with torch.no_grad():
            tr.vars['POST2'].mul_(4.0)
        _PARAMS[key] = ({n: v.detach().clone() for n, v in tr.vars.items()},
                        {n: v.cpu().double().numpy() for n, v in tr.vars.items()})
    dev, P = _PARAMS[key]
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, chunk, None, seed=SEED, n_lc_in=arch['n_lc_in'], n_lc_out=arch['n_lc_out'],
                   lc_upsample=arch['lc_upsample'])
    g.load_params(dev)
    if teacher_q is not None:
        g.teacher_mu = torch.as_tensor(np.asarray(teacher_q, np.int32), device='cuda')
    return g, P


def _near_tie(lg_row, u, tol=5e-5):
    e = np.exp(lg_row - lg_row.max())
    c = np.cumsum(e)
    return float(np.min(np.abs(c - u * c[-1]))) <= tol * c[-1]


def step0(arch, P, B, gc, lc_row):
    """Generation step 0 in float64: zero input (+ PRE_BIAS), zero lookback, LC row lc_row [B, Lo].
    Returns (SAVE with g_l in each layer's last row, logits [B, Q])."""
    bias = (lambda n: P[n]) if arch['use_bias'] else (lambda n: 0.0)      # no-bias archs have no *_BIAS tensor
    x = np.zeros((B, arch['n_res'])) + bias('PRE_BIAS')
    emb = P['GC_EMBED'][np.asarray(gc)] if arch['n_gc_embed'] > 0 else None
    save, S = {}, 0.0
    for l in range(R.n_layers(arch)):
        b, bl, d = R.layer_index(arch, l)
        sfx = '_%d_%d' % (b, bl)
        sv = np.zeros((B, d, arch['n_res']))
        sv[:, -1] = x
        save['SAVE_%d%s' % (d, sfx)] = sv
        v = {nm: x @ P[nm + sfx][1] + bias(nm + '_BIAS' + sfx) + lc_row @ P['LC_' + nm + sfx]
             + (emb @ P['GC_' + nm + sfx] if emb is not None else 0.0) for nm in ('SIGNAL', 'GATE')}
        z = np.tanh(v['SIGNAL']) * R._sigmoid(v['GATE'])
        S = S + z @ P['SKIP' + sfx] + bias('SKIP_BIAS' + sfx)
        x = x + z @ P['RESIDUAL' + sfx] + bias('RESIDUAL_BIAS' + sfx)
    h = np.maximum(np.maximum(S, 0) @ P['POST1'] + bias('POST1_BIAS'), 0)
    return save, h @ P['POST2'] + bias('POST2_BIAS')


def oracle_logits(arch, P, got, mel, gc=None, teacher_q=None, clamp_rows=False, monkeypatch=None):
    """Float64 logits [B, n, Q] of every generation step along the trajectory `got` [B, n] (the
    GPU's draws; the teacher's codes where it forces the input).  clamp_rows: the run is longer
    than the mel, the upsampled mel's last row is repeated (needs monkeypatch)."""
    B, n = got.shape
    mel = np.asarray(mel, np.float64)
    lc, _ = R.lc_upsample_fwd(arch, P, mel)
    save, lg0 = step0(arch, P, B, gc, lc[:, 0])
    wav_q = got[:, :n - 1].copy()
    if teacher_q is not None:
        k = min(len(teacher_q), n - 1)
        wav_q[:, :k] = np.asarray(teacher_q)[:k]
    ids = np.ones((B, n - 1), np.int64) if gc is None else np.repeat(np.asarray(gc)[:, None], n - 1, axis=1)
    if clamp_rows:
        assert n - 1 > lc.shape[1]
        pad = np.concatenate([lc, np.repeat(lc[:, -1:], n - 1 - lc.shape[1], axis=1)], axis=1)
        monkeypatch.setattr(R, 'lc_upsample_fwd', lambda a, p, m: (pad, None))
    else:
        assert n - 1 == lc.shape[1]
    lg, _, _ = R.forward(arch, P, wav_q, ids, save, mel=mel)
    return np.concatenate([lg0[:, None], lg], axis=1)


def check_draws(got, lg, exact=False):
    """Every draw against the float64 logits it was drawn from: differences only at a near tie
    of the inverse CDF, at most 2 (exact: none)."""
    B, n = got.shape
    ref = np.array([[R.sample_from_logits(lg[b, i], R.philox_uniform(SEED, b, i)) for i in range(n)]
                    for b in range(B)])
    bad = np.argwhere(got != ref)
    print('draws %d, differing %d, max |logit| %.3f' % (got.size, len(bad), np.abs(lg).max()))
    if exact:
        assert len(bad) == 0, bad.tolist()
    ties = [(int(b), int(i)) for b, i in bad if _near_tie(lg[b, i], R.philox_uniform(SEED, int(b), int(i)))]
    assert len(ties) == len(bad), 'draws differ away from a CDF tie at (stream, step) %s' % (bad[:8].tolist(),)
    assert len(bad) <= 2, bad.tolist()


def check_run(g, lg, n, exact=False):
    """Status, step counter, the draws, and the last step's logits."""
    torch.cuda.synchronize()
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    check_draws(g.samples().cpu().numpy()[:, :n], lg, exact)
    err = np.abs(g.logits().cpu().numpy() - lg[:, -1]).max()
    print('last-step logits: max err %.3e (bound %.3e)' % (err, 1e-4 * np.abs(lg[:, -1]).max()))
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())


def test_gen_lc_small_free_running_ragged(form, monkeypatch):
    """B = 3, 8 frames x hop 8 -> n = 65 steps, chunk 10 with a cond ring of NC = 4 steps: each
    replayed chunk is 4 + 4 + 2 sub-runs, six replays and a 5-step tail launch, the ring wraps 16
    times.  195 draws, all equal."""
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    arch = small()
    B, n = 3, 65
    mel = np.random.default_rng(11).standard_normal((B, 8, 12)).astype(np.float32)
    g, P = make_gen(arch, B, chunk=10)
    _, wav, rem = g.run(n, mel=mel)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    assert g.tensor('lccond').numel() == 4 * 8 * B * 64
    assert wav.shape == (B, 60) and rem == 5
    got = g.samples().cpu().numpy()[:, :n]
    assert len(np.unique(got)) > 16
    lg = oracle_logits(arch, P, got, mel)
    check_run(g, lg, n, exact=True)
    # the upsampled mel itself (the training plan's stack, run once by lbwn_gen_set_mel)
    lc_ref, _ = R.lc_upsample_fwd(arch, P, mel.astype(np.float64))
    lc = g.tensor('lc')[:B * 64 * 16].view(B, 64, 16).cpu().numpy()
    np.testing.assert_allclose(lc, lc_ref, rtol=0, atol=1e-5 * np.abs(lc_ref).max())


def test_gen_lc_upsample_gemm_fallback(lib, monkeypatch):
    """n_lc_in 24 > n_lc_out 16 is outside the fused upsample's envelope (Li > Lo), so
    lbwn_gen_set_mel runs the upsample as one GEMM per stage: the plan's "lc" against
    lc_upsample_fwd in float64 at 1e-5 of max(1, max), and the 17 steps drawn from it."""
    import ctypes
    monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    arch = normalize_arch(dict(small(), n_lc_in=24))
    assert lib.lbwn_lc_upsample_fused_ok(2, (ctypes.c_int * 2)(2, 4), 24, 16) == 0
    B, frames = 3, 2
    n = frames * 8 + 1
    mel = np.random.default_rng(16).standard_normal((B, frames, 24)).astype(np.float32)
    g, P = make_gen(arch, B, chunk=10)
    g.run(n, mel=mel)
    torch.cuda.synchronize()
    lc_ref, _ = R.lc_upsample_fwd(arch, P, mel.astype(np.float64))
    lc = g.tensor('lc')[:B * frames * 8 * 16].view(B, frames * 8, 16).cpu().numpy()
    err, bar = np.abs(lc - lc_ref).max(), 1e-5 * max(1.0, np.abs(lc_ref).max())
    print('lc (per-stage GEMMs): max err %.3e (bar %.3e)' % (err, bar))
    assert np.isfinite(lc).all() and err <= bar, (err, bar)
    got = g.samples().cpu().numpy()[:, :n]
    check_run(g, oracle_logits(arch, P, got, mel), n)


def test_gen_lc_gc_teacher_forced(form):
    """LC + GC (8 / 5 voices), teacher-forced over the first 25 steps, then free; default NC."""
    arch = small(gc=5)
    B, n = 2, 65
    teacher_q = np.random.default_rng(1).integers(0, 256, 25).astype(np.int32)
    mel = np.random.default_rng(12).standard_normal((B, 8, 12)).astype(np.float32)
    g, P = make_gen(arch, B, chunk=10, teacher_q=teacher_q)
    gc = [2, 5]
    g.run(n, gc_ids=gc, mel=mel)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    got = g.samples().cpu().numpy()[:, :n]
    lg = oracle_logits(arch, P, got, mel, gc=gc, teacher_q=teacher_q)
    check_run(g, lg, n)


def test_gen_lc_mel_matters_per_stream_and_rerun(form, monkeypatch):
    """Every input forced by the teacher: streams 0 and 1 share a mel and get equal logits,
    stream 2 (another mel) does not; a second run of the same plan (and the same captured graph)
    with a second mel follows the second mel (a stale "lc" or cond ring would follow the first)."""
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    arch = small()
    B, n = 3, 65
    teacher_q = np.random.default_rng(2).integers(0, 256, n).astype(np.int32)
    rng = np.random.default_rng(13)
    m2 = rng.standard_normal((2, 8, 12)).astype(np.float32)
    mel_a = np.stack([m2[0], m2[0], m2[1]])
    mel_b = rng.standard_normal((8, 12)).astype(np.float32)        # [frames, n_lc_in]: every stream
    g, P = make_gen(arch, B, chunk=10, teacher_q=teacher_q)
    g.run(n, mel=mel_a)
    torch.cuda.synchronize()
    la = g.logits().cpu().numpy().copy()
    np.testing.assert_array_equal(la[0], la[1])
    assert np.abs(la[0] - la[2]).max() > 1e-3 * np.abs(la).max()
    got = g.samples().cpu().numpy()[:, :n]
    check_run(g, oracle_logits(arch, P, got, mel_a, teacher_q=teacher_q), n)
    g.run(n, mel=torch.as_tensor(mel_b))
    torch.cuda.synchronize()
    lb = g.logits().cpu().numpy().copy()
    np.testing.assert_array_equal(lb[0], lb[2])
    assert np.abs(lb - la).max() > 1e-3 * np.abs(la).max()
    got = g.samples().cpu().numpy()[:, :n]
    check_run(g, oracle_logits(arch, P, got, np.broadcast_to(mel_b, (B, 8, 12)), teacher_q=teacher_q), n)


_ARCH5_LOGITS = {}


@pytest.mark.parametrize('B', [10, 20])
def test_gen_lc_arch5_as_shipped(B, form):
    """par/arch5.json (50 layers, LC 80 -> 80, hop 256, GC 16 / 376): 2 frames -> n = 513, so the
    d = 512 rings wrap and the clamped step 0 is exercised; chunk 100, default NC.  B = 10 is one
    persistent group, B = 20 two (LBWN_GEN_PERSIST=0: the vector GEMVs / the MFMA-GEMM head)."""
    arch = load_arch(os.path.join(ROOT, 'par', 'arch5.json'))
    n = 513
    mel = np.random.default_rng(14).standard_normal((B, 2, 80)).astype(np.float32)
    gc = [1 + (37 * b) % 376 for b in range(B)]
    g, P = make_gen(arch, B, chunk=100)
    g.run(n, gc_ids=gc, mel=mel)
    torch.cuda.synchronize()
    assert g.persistent == (form == 'persistent')
    got = g.samples().cpu().numpy()[:, :n]
    assert len(np.unique(got)) > 16
    key = (B, got.tobytes())        # both forms draw the same trajectory: one float64 forward for the two
    if key not in _ARCH5_LOGITS:
        _ARCH5_LOGITS[key] = oracle_logits(arch, P, got, mel, gc=gc)
    check_run(g, _ARCH5_LOGITS[key], n)


def test_gen_lc_clamp_past_the_mel(form, monkeypatch):
    """Below the Python layer (init_buffers + step, no length check): n = 70 steps on 8 frames x
    hop 8 = 64 rows.  Steps 66..69 reuse the last upsampled row, i.e. they equal a forward whose
    upsampled mel has its last row repeated."""
    arch = small()
    B, n = 3, 70
    mel = np.random.default_rng(15).standard_normal((B, 8, 12)).astype(np.float32)
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(n)
    g.init_buffers(mel=mel)
    g.step(n)
    torch.cuda.synchronize()
    got = g.samples().cpu().numpy()[:, :n]
    lg = oracle_logits(arch, P, got, mel, clamp_rows=True, monkeypatch=monkeypatch)
    check_run(g, lg, n)


def test_train_then_generate_with_mel_end_to_end(tmp_path, capsys):
    """train.py on an LC arch (mel catalog) writes a checkpoint; generate.py --mel-npy samples it."""
    import generate
    import train
    from lbwn.ops import mu_encode_np
    arch = dict(small(), wav_input_type='mu_law_quant')
    par = dict(batch_sz=2, sample_rate=16000, slice_sz=128, l2_factor=1e-3, learning_rate=1e-3, prefetch_sz=4,
               add_summary=False, n_keep_checkpoints=3, n_valid_total=100000)
    af, pf = tmp_path / 'arch.json', tmp_path / 'par.json'
    af.write_text(json.dumps(arch))
    pf.write_text(json.dumps(par))
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        n = 8 * int(rng.integers(80, 170))
        t = np.arange(n) / 16000.0
        x = 0.8 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + rng.normal(0, 0.05, n)
        wp, mp = tmp_path / ('w%d.npy' % i), tmp_path / ('m%d.npy' % i)
        np.save(wp, mu_encode_np(np.clip(x, -1, 1), 256).astype(np.int32))
        np.save(mp, rng.standard_normal((n // 8, 12)).astype(np.float32))
        lines.append('1\t%s\t%s' % (wp, mp))
    cat = tmp_path / 'samples.txt'
    cat.write_text('\n'.join(lines) + '\n')
    pfx = str(tmp_path / 'ck' / 'run')
    net = train.main(['--max-steps', '3', '--save-interval', '2', '--seed', '1', pfx, str(af), str(pf), str(cat)])
    assert int(net.counters[0]) == 2
    mel = rng.standard_normal((2, 100, 12)).astype(np.float32)        # 800 steps of hop 8
    np.save(tmp_path / 'mel.npy', mel)
    wav = generate.main(['--mel-npy', str(tmp_path / 'mel.npy'), '--gen-seconds', '0.05', '--batch-size', '2',
                         '--chunk-size', '200', '--seed', str(SEED), str(af), pfx + '.net-2', str(tmp_path / 'out')])
    assert wav.shape == (2, 800) and np.all(np.abs(wav) <= 1.03)
    for i in range(2):
        assert os.path.exists(tmp_path / 'out' / ('gen.i%d.wav' % i))
    # the wavs are the checkpoint's draws for that mel: the first 65 steps against the oracle
    from lbwn.ckpt import load_tensors
    P = {k: v.double().numpy() for k, v in load_tensors(pfx + '.net-2').items() if k in net.vars}
    a = normalize_arch(arch)
    table = R.mu_decode_np(np.arange(256), 256)
    q = np.abs(wav[:, :65, None].astype(np.float64) - table).argmin(axis=2)       # the codes behind the wav
    np.testing.assert_allclose(table[q], wav[:, :65], rtol=1e-6, atol=1e-6)
    check_draws(q, oracle_logits(a, P, q, mel[:, :8]))
