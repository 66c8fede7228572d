"""The drop-in entry points end to end on the GPU: train.py on a .npy sample catalog
(train.py:12-244: train, checkpoint at --save-interval, resume from --resume-step) and
generate.py from the resulting checkpoint (generate.py:1-120)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from lbwn.ckpt import ckpt_file, load_tensors
from lbwn.ops import mu_encode_np
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))


def _dataset(tmp_path, n_files=6, voices=3):
    rng = np.random.default_rng(0)
    lines = []
    for i in range(n_files):
        n = int(rng.integers(600, 1400))
        t = np.arange(n) / 16000.0
        x = 0.8 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + rng.normal(0, 0.05, n)
        wav = mu_encode_np(np.clip(x, -1, 1), 256).astype(np.int32)
        wp, mp = tmp_path / ('w%d.npy' % i), tmp_path / ('m%d.npy' % i)
        np.save(wp, wav)
        np.save(mp, np.zeros((n, 0), np.float32))
        lines.append('%d\t%s\t%s' % (i % voices + 1, wp, mp))
    cat = tmp_path / 'samples.txt'
    cat.write_text('\n'.join(lines) + '\n')
    return str(cat)


def test_train_resume_generate(tmp_path, capsys):
    _train_resume_generate(tmp_path, capsys, True)


def test_train_resume_generate_no_bias(tmp_path, capsys):
    """The same run on the arch with use_bias = false: no *_BIAS tensor in any checkpoint."""
    _train_resume_generate(tmp_path, capsys, False)


def _train_resume_generate(tmp_path, capsys, use_bias):
    import generate
    import train
    arch = dict(n_blocks=1, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
                n_gc_embed=8, n_gc_category=3, n_lc_in=0, n_lc_out=0, lc_upsample=[], use_bias=use_bias,
                wav_input_type='mu_law_quant')
    par = dict(batch_sz=2, sample_rate=16000, slice_sz=128, l2_factor=1e-3, learning_rate=1e-3, prefetch_sz=4,
               add_summary=False, n_keep_checkpoints=3, n_valid_total=100000)
    af, pf = tmp_path / 'arch.json', tmp_path / 'par.json'
    af.write_text(json.dumps(arch))
    pf.write_text(json.dumps(par))
    cat = _dataset(tmp_path)
    pfx = str(tmp_path / 'ck' / 'run')
    net = train.main(['--max-steps', '5', '--save-interval', '2', '--progress-interval', '1', '--seed', '1',
                      pfx, str(af), str(pf), cat])
    err = capsys.readouterr().err
    assert 'Starting training...' in err and 'Saved checkpoints to' in err
    lines = [l for l in err.splitlines() if l and l.split('\t')[0].strip().isdigit()]
    assert len(lines) >= 4                             # progress columns, tmodel.py:263-267
    assert all(np.isfinite(float(l.split('\t')[1])) for l in lines)
    assert int(net.counters[0]) == 4                   # steps 1..4 (train.py:213 loop)
    for s in (2, 4):
        assert os.path.exists(ckpt_file(pfx + '.net', s)) and os.path.exists(ckpt_file(pfx + '.dset', s))
    t = load_tensors(pfx + '.net-4')
    assert int(t['GLOBAL_STEP'][0]) == 4
    assert any('BIAS' in n for n in t) == use_bias and any('BIAS' in n for n in net.vars) == use_bias
    np.testing.assert_array_equal(t['SIGNAL_0_3'].numpy(), net.vars['SIGNAL_0_3'].cpu().numpy())
    # resume from step 4 and take two more steps
    net2 = train.main(['--max-steps', '7', '--resume-step', '4', '--save-interval', '2', pfx, str(af), str(pf), cat])
    assert int(net2.counters[0]) == 7                  # the reference resumes AT resume_step (train.py:212)
    assert os.path.exists(ckpt_file(pfx + '.net', 6))
    assert 'Restored net and dset from checkpoint' in capsys.readouterr().err
    # generate from the step-6 checkpoint (GC arch: voice ids cycled over the batch)
    wav = generate.main(['--gen-seconds', '0.05', '--batch-size', '3', '--chunk-size', '200', '--gc-ids', '1,3',
                         str(af), pfx + '.net-6', str(tmp_path / 'out')])
    assert wav.shape == (3, 800)
    assert np.all(np.abs(wav) <= 1.03)
    for i in range(3):
        assert os.path.exists(tmp_path / 'out' / ('gen.i%d.wav' % i))


def test_generate_teacher_wav_end_to_end(tmp_path):
    """generate.py --teacher-wav (generate.py:52-59, imodel.py:44-46, :260): a 16-bit 8 kHz
    wav is read, cut (--teacher-start/--teacher-duration), resampled to 16 kHz, µ-law encoded
    on the GPU (TF-fp32 form, ops.py:4-9) and forces the inputs; the draws must equal the
    oracle's generation forced by the oracle's own encoding of the same samples."""
    import generate
    from scipy.io import wavfile
    from lbwn.arch import normalize_arch
    from lbwn.tmodel import WaveNetTrain
    from oracle import wavenet_ref as R
    arch = normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
                               n_gc_embed=0, n_gc_category=0, use_bias=True))
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(arch))
    tr = WaveNetTrain(**arch, batch_sz=1, l2_factor=0.0, print_interval=0, ckpt_path=str(tmp_path / 'g.net'))
    tr.init_vars(5, bias_scale=0.2)
    with torch.no_grad():
        tr.vars['POST2'].mul_(4.0)
    tr.save(1)
    t = np.arange(800) / 8000.0
    x = 0.6 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 530 * t)
    wavfile.write(str(tmp_path / 'teach.wav'), 8000, (x * 32767).astype(np.int16))
    wav = generate.main(['--teacher-wav', str(tmp_path / 'teach.wav'), '--teacher-start', '0.01',
                         '--teacher-duration', '0.05', '--gen-seconds', '0.02', '--batch-size', '2',
                         '--chunk-size', '100', str(af), str(tmp_path / 'g.net-1'), str(tmp_path / 'out')])
    teacher = generate.load_teacher(str(tmp_path / 'teach.wav'), 16000, 0.01, 0.05)
    assert teacher.shape == (800,)                     # 0.05 s at 8 kHz, resampled to 16 kHz
    n = int((0.02 + teacher.shape[0] / 16000) * 16000)
    assert wav.shape == (2, (n // 100) * 100)
    P = {k: v.cpu().double().numpy() for k, v in tr.vars.items()}
    tq = R.mu_encode_tf32(teacher, 256)
    _, w_ref = R.generate(arch, P, 2, n, seed=0, teacher_q=tq)
    np.testing.assert_allclose(wav, w_ref[:, :wav.shape[1]], rtol=1e-6, atol=1e-6)


def _synthetic_catalog(tmp_path, n_files=24):
    from lbwn.data import SyntheticSource
    src = SyntheticSource(seed=7, hop=1, n_mel=0, n_voices=1)
    lines = []
    for i in range(n_files):
        vid, wav, _ = next(src)
        wp, mp = tmp_path / ('s%d.npy' % i), tmp_path / ('s%d.mel.npy' % i)
        np.save(wp, wav.astype(np.int32))
        np.save(mp, np.zeros((len(wav), 0), np.float32))
        lines.append('%d\t%s\t%s' % (vid, wp, mp))
    cat = tmp_path / 'cat.txt'
    cat.write_text('\n'.join(lines) + '\n')
    return str(cat)


def test_train_py_bench_config_runs(tmp_path):
    """The drop-in train.py loop (dealer thread -> pinned buffers -> non-blocking H2D -> plan ->
    DP hook -> TF1 Adam, progress line every 10 steps, train.py:216-252) at the benchmarked
    arch3 B=8 T=4096: every step is applied (GLOBAL_STEP advances once per step of the loop,
    train.py:213) and no chain hand-off timed out."""
    import train
    arch_file = os.path.join(ROOT, 'par', 'arch3.json')
    par = json.load(open(os.path.join(ROOT, 'par', 'par1.json')))
    par.update(batch_sz=8, slice_sz=4096)
    pf = tmp_path / 'par.json'
    pf.write_text(json.dumps(par))
    cat = _synthetic_catalog(tmp_path)
    net = train.main(['--max-steps', '12', '--seed', '3', str(tmp_path / 'ck'), arch_file, str(pf), cat])
    torch.cuda.synchronize()
    assert int(net.counters[0]) == 11
    net.check_status()
    assert net.global_step_host == 11
    assert np.isfinite(float(net.total_loss()))


@pytest.mark.skipif(os.environ.get('LBWN_PERF_TESTS') != '1',
                    reason='wall-clock comparison: opt in with LBWN_PERF_TESTS=1 (depends on the box)')
def test_train_py_runs_at_bench_speed(tmp_path):
    """The drop-in train.py loop (dealer thread -> pinned buffers -> non-blocking H2D -> plan ->
    DP hook -> TF1 Adam, progress line every 10 steps, train.py:216-252) at arch3 B=8 T=4096
    runs within 10 % of bench.py's pre-dealt device ring at the same arch/B/T.  Steady-state
    time per step = (wall(61 steps) - wall(21 steps)) / 40, so setup cancels (after a warm-up
    run, whose one-time costs would otherwise fall into the 21-step wall only)."""
    import time
    import train
    sys.path.insert(0, ROOT)
    import bench
    from lbwn import dist as lbdist
    from lbwn.arch import load_arch
    arch_file = os.path.join(ROOT, 'par', 'arch3.json')
    par = json.load(open(os.path.join(ROOT, 'par', 'par1.json')))
    par.update(batch_sz=8, slice_sz=4096)
    pf = tmp_path / 'par.json'
    pf.write_text(json.dumps(par))
    cat = _synthetic_catalog(tmp_path)
    walls = {}
    for n in (6, 21, 61):   # the first run pays the one-time costs (module loads, first plan): discarded
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net = train.main(['--max-steps', str(n), '--seed', '3', str(tmp_path / ('ck%d' % n)), arch_file, str(pf),
                          cat])
        torch.cuda.synchronize()
        walls[n] = time.perf_counter() - t0
        assert int(net.counters[0]) == n - 1
        del net
        torch.cuda.empty_cache()
    train_ms = (walls[61] - walls[21]) * 1000.0 / 40
    tb = bench.TrainBench(load_arch(arch_file), 8, 4096, lbdist.DPContext())
    bench_ms, _, _, _ = tb.run(40, 5)
    tb.close()
    print('train.py %.3f ms/step, bench %.3f ms/step' % (train_ms, bench_ms))
    assert train_ms <= 1.10 * bench_ms, (train_ms, bench_ms)
