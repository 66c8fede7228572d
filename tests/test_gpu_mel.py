"""The log-mel front end on the GPU (lbwn_mel_forward, lbwn.mel.MelSpectrogram) against
the float64 restatement in tests/mel_ref.py.

Yardstick: the helper's float32 twin (the same direct sums with every array in float32) on the same
input, computed here.  Linear domain (log_floor = 0): per frame, max |kernel - float64| over the bands
divided by the frame's largest float64 band; the kernel may reach 8x the twin's worst frame and never
more than 1e-5.  Log domain (floor 1e-5): max |kernel - float64| over all bands, bounded by 8x the
twin's.  The margin is for another summation order (the kernel sums each dot product in sample order on
the matrix cores and the bands per wave; numpy sums pairwise)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import mel_ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))

SR = 16000
# name: (n_fft, hop, n_mels, n, extra settings)
CASES = {
    'one_tile': (64, 16, 8, 512, {}),                         # 32 frames
    'partial_tail': (64, 16, 8, 16 * 65 + 7, {}),             # 65 frames: a 1-row second tile, dropped tail
    'mid': (256, 64, 20, 64 * 70, {}),                        # 70 frames, 9 column blocks (Nyquist alone)
    'real': (1024, 256, 80, 10240, {}),                       # 40 frames, 17 column blocks, 80 bands
    'no_overlap': (64, 64, 8, 64 * 40, {}),                   # hop = n_fft
    'hop4': (64, 4, 8, 4 * 150 + 3, {}),                      # 150 frames: three tiles
    'win800': (1024, 256, 80, 10240, dict(win_length=800)),
    'power1': (256, 64, 20, 64 * 70, dict(power=1)),
    'htk_nonorm': (256, 64, 20, 64 * 70, dict(htk=True, norm=False)),
    # the kernel's other instantiations: two and four 32-band tiles, and the 32-frame tile a block falls
    # back to when 64 frames do not fit the LDS (n_fft 2048 at hop 512: 40 frames = two tiles)
    'mels40': (256, 64, 40, 64 * 70, {}),
    'mels128': (1024, 256, 128, 10240, {}),
    'rows32': (2048, 512, 80, 512 * 40, {}),
}
_REF = {}


def reference(name, log_floor):
    """(x, float64 mel, float32 twin's mel) of a case; computed once and shared, never written to."""
    key = (name, log_floor)
    if key not in _REF:
        n_fft, hop, n_mels, n, kw = CASES[name]
        x = mel_ref.test_signal(n, SR)
        a = mel_ref.mel(x, SR, n_fft, hop, n_mels, log_floor=log_floor, **kw)
        b = mel_ref.mel(x, SR, n_fft, hop, n_mels, log_floor=log_floor, dtype=np.float32, **kw)
        for v in (x, a, b):
            v.setflags(write=False)
        _REF[key] = (x, a, b)
    return _REF[key]


def spec(name, log_floor):
    from lbwn.mel import MelSpectrogram
    n_fft, hop, n_mels, n, kw = CASES[name]
    return MelSpectrogram(SR, hop, n_mels, n_fft=n_fft, log_floor=log_floor, **kw)


def lin_err(got, ref):
    """Per frame: max |got - ref| over the bands / the frame's largest reference band."""
    return np.abs(np.asarray(got, np.float64) - ref).max(axis=1) / ref.max(axis=1)


@pytest.mark.parametrize('name', list(CASES))
def test_linear_accuracy(name):
    x, ref, twin = reference(name, 0.0)
    got = spec(name, 0.0)(x).cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    e_k, e_t = lin_err(got, ref), lin_err(twin, ref)
    print('%s linear: kernel worst %.3e, twin worst %.3e, ratio %.2f' % (name, e_k.max(), e_t.max(),
                                                                         e_k.max() / e_t.max()))
    assert e_k.max() <= min(8.0 * e_t.max(), 1e-5), (e_k.max(), e_t.max())


@pytest.mark.parametrize('name', list(CASES))
def test_log_accuracy(name):
    x, ref, twin = reference(name, 1e-5)
    got = spec(name, 1e-5)(x).cpu().numpy()
    assert got.shape == ref.shape
    e_k, e_t = np.abs(got.astype(np.float64) - ref).max(), np.abs(twin.astype(np.float64) - ref).max()
    print('%s log: kernel %.3e, twin %.3e, ratio %.2f' % (name, e_k, e_t, e_k / e_t))
    assert e_k <= 8.0 * e_t, (e_k, e_t)


def test_edge_frames_of_the_real_configuration():
    """Frames 0, 1 (left reflection) and F-2, F-1 (right reflection) of the 1024 case on their own."""
    x, ref, twin = reference('real', 0.0)
    got = spec('real', 0.0)(x).cpu().numpy()
    e_k, e_t = lin_err(got, ref), lin_err(twin, ref)
    F = ref.shape[0]
    for t in (0, 1, F - 2, F - 1):
        assert e_k[t] <= min(8.0 * e_t.max(), 1e-5), (t, e_k[t], e_t.max())


@pytest.mark.parametrize('name', ['one_tile', 'real'])
def test_impulses_show_the_reflection(name):
    """One impulse at sample 0 and one at n-1: with the edge repeated (or the reflection off by one) the
    first and last frames would see the impulse twice or at another lag."""
    from lbwn.mel import MelSpectrogram
    n_fft, hop, n_mels, n, kw = CASES[name]
    x = np.zeros(n, np.float32)
    x[0], x[n - 1] = 1.0, -0.75
    ref = mel_ref.mel(x, SR, n_fft, hop, n_mels, log_floor=0.0)
    twin = mel_ref.mel(x, SR, n_fft, hop, n_mels, log_floor=0.0, dtype=np.float32)
    got = MelSpectrogram(SR, hop, n_mels, n_fft=n_fft, log_floor=0.0)(x).cpu().numpy().astype(np.float64)
    live = ref.max(axis=1) > 0                     # frames that reach neither impulse are exactly zero
    assert live[0] and live[-1] and (got[~live] == 0).all()
    e_k = np.abs(got[live] - ref[live]).max(axis=1) / ref[live].max(axis=1)
    e_t = np.abs(twin[live] - ref[live]).max(axis=1) / ref[live].max(axis=1)
    print('%s impulses: kernel %.3e, twin %.3e' % (name, e_k.max(), e_t.max()))
    assert e_k.max() <= min(8.0 * e_t.max(), 1e-5), (e_k.max(), e_t.max())


def test_batch_strides_and_padding():
    """B = 3 with ld_wav > n and ld_out_stream > F*n_mels: the wav padding is NaN and must be unread, the
    out padding holds a sentinel and must be unwritten; stream b is bitwise the single-stream result."""
    from lbwn.mel import MelSpectrogram
    n_fft, hop, n_mels, B = 256, 64, 20, 3
    n = 64 * 70 + 9
    F = n // hop
    ms = MelSpectrogram(SR, hop, n_mels, n_fft=n_fft, log_floor=0.0)
    xs = np.stack([mel_ref.test_signal(n, SR, seed=s) for s in range(B)])
    ld_wav, ld_out = n + 3 + 8, F * n_mels + 12       # ld_wav = n + 11 = a multiple of 4
    assert ld_wav % 4 == 0
    wav = torch.full((B, ld_wav), float('nan'), device='cuda')
    wav[:, :n] = torch.from_numpy(xs).cuda()
    out = torch.full((B, ld_out), -777.0, device='cuda')
    ms.forward_into(wav[:, :n], out)
    got = out.cpu().numpy()
    assert (got[:, F * n_mels:] == -777.0).all()
    body = got[:, :F * n_mels].reshape(B, F, n_mels)
    assert np.isfinite(body).all()
    for b in range(B):
        ref = mel_ref.mel(xs[b], SR, n_fft, hop, n_mels, log_floor=0.0)
        twin = mel_ref.mel(xs[b], SR, n_fft, hop, n_mels, log_floor=0.0, dtype=np.float32)
        assert lin_err(body[b], ref).max() <= min(8.0 * lin_err(twin, ref).max(), 1e-5)
        single = ms(xs[b]).cpu().numpy()
        assert np.array_equal(single, body[b]), b
    assert np.array_equal(ms(xs).cpu().numpy(), body)


def test_deterministic_and_graph_replay():
    """Two launches give the same bits; a captured graph replays to the same bits, also on new input."""
    x, _, _ = reference('real', 1e-5)
    ms = spec('real', 1e-5)
    a = ms(x)
    b = ms(x)
    assert torch.equal(a, b)
    n = len(x)
    wav = torch.from_numpy(np.array(x)).cuda()[None].contiguous()
    out = torch.zeros(1, a.numel(), device='cuda')
    ms.forward_into(wav, out)                       # warm: tables and the kernel's LDS attribute are set
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ms.forward_into(wav, out)
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view_as(a), a)
    x2 = mel_ref.test_signal(n, SR, seed=5)
    wav.copy_(torch.from_numpy(x2).cuda()[None])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view_as(a), ms(x2))


def test_tables_are_a_function_of_the_configuration():
    """lbwn_mel_init writes the same bits into two workspaces; the basis is finite and not all zero."""
    a, b = spec('mid', 1e-5), spec('mid', 1e-5)
    wa, wb = a.workspace(), b.workspace()
    torch.cuda.synchronize()
    assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))
    assert torch.isfinite(wa).all() and float(wa.abs().max()) > 0.5


def test_make_mels_train_generate_end_to_end(tmp_path):
    """make_mels.py on two synthetic wavs, train.py for 3 steps on the written catalogue, then generate.py
    --mel-from-wav --mel-config; the same generation with the mel saved and passed as --mel-npy gives
    bitwise the same samples.  The arch is the tiny LC arch of tests/test_gpu_gen_lc.py as it stands
    (mu_law_quant, what normalize_arch defaults to and par/arch5.json says): the audio files are what
    train.py takes them for, int32 mu-law codes of the trimmed wav, and the last training step was fed
    exactly those codes beside the mel rows written for them."""
    import generate
    import make_mels
    import train
    from scipy.io import wavfile
    from lbwn.arch import normalize_arch
    from lbwn.mel import MelSpectrogram
    from lbwn.ops import mu_encode_np
    arch = dict(normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64,
                                    n_post=32, n_gc_embed=0, n_gc_category=0, n_lc_in=12, n_lc_out=16,
                                    lc_upsample=[2, 4], use_bias=True)))
    assert arch['wav_input_type'] == 'mu_law_quant'
    hop, n_mels = 8, 12
    par = dict(batch_sz=2, sample_rate=SR, slice_sz=128, l2_factor=1e-3, learning_rate=1e-3, prefetch_sz=4,
               add_summary=False, n_keep_checkpoints=3, n_valid_total=100000)
    af, pf, cf = tmp_path / 'arch.json', tmp_path / 'par.json', tmp_path / 'cfg_in.json'
    af.write_text(json.dumps(arch))
    pf.write_text(json.dumps(par))
    cfg = dict(sample_rate=SR, n_fft=128, win_length=128, hop=hop, n_mels=n_mels, fmin=0.0, fmax=8000.0, power=2,
               htk=False, norm=True, log_floor=1e-5)
    cf.write_text(json.dumps(cfg))
    lines, sigs = [], []
    for i, n in enumerate((1605, 1203)):
        x = 0.9 * mel_ref.test_signal(n, SR, seed=10 + i)
        sigs.append(x)
        if i == 0:
            wavfile.write(str(tmp_path / 'a.wav'), SR, x)
            lines.append('1\t%s' % (tmp_path / 'a.wav'))
        else:
            np.save(tmp_path / 'b.npy', x)
            lines.append('1\t%s' % (tmp_path / 'b.npy'))
    lines.append('1\t%s' % (tmp_path / 'short.npy'))
    np.save(tmp_path / 'short.npy', np.zeros(64, np.float32))        # n_fft/2 samples: skipped
    (tmp_path / 'in.txt').write_text('\n'.join(lines) + '\n')
    cat = tmp_path / 'samples.txt'
    written = make_mels.main(['--mel-config', str(cf), str(af), str(pf), str(tmp_path / 'in.txt'),
                              str(tmp_path / 'data'), str(cat)])
    assert len(written) == 2
    assert json.loads((tmp_path / 'data' / 'mel_config.json').read_text()) == cfg
    frame_of = {}                                   # mel row bytes -> (the codes of its hop samples)
    for (vid, wp, mp), x in zip(written, sigs):
        w, m = np.load(wp), np.load(mp)
        assert m.dtype == np.float32
        assert len(w) == len(m) * hop and m.shape == (len(x) // hop, n_mels)
        trimmed = x[:len(w)]
        codes = mu_encode_np(np.clip(trimmed.astype(np.float64), -1.0, 1.0), 256).astype(np.int32)
        assert w.dtype == np.int32 and np.array_equal(w, codes)
        assert w.min() >= 0 and w.max() <= 255 and len(np.unique(w)) > 50
        ref = mel_ref.mel(trimmed, SR, 128, hop, n_mels, log_floor=1e-5)
        twin = mel_ref.mel(trimmed, SR, 128, hop, n_mels, log_floor=1e-5, dtype=np.float32)
        assert np.abs(m - ref).max() <= 8.0 * np.abs(twin - ref).max()
        for t in range(len(m)):
            frame_of[m[t].tobytes()] = codes[t * hop:(t + 1) * hop]
    assert [l.split('\t')[1:] for l in cat.read_text().splitlines()] == [[wp, mp] for _, wp, mp in written]

    pfx = str(tmp_path / 'ck' / 'run')
    net = train.main(['--max-steps', '3', '--save-interval', '2', '--seed', '1', pfx, str(af), str(pf), str(cat)])
    assert int(net.counters[0]) == 2
    # what the last step was fed: every mel row is a written one, beside the codes of its own hop samples
    q, ids, fed_mel = (t.cpu().numpy() for t in net._last)
    assert q.shape == (2, 128) and fed_mel.shape == (2, 16, n_mels)
    for b in range(2):
        for j in range(16):
            want = frame_of[fed_mel[b, j].tobytes()]
            got = q[b, j * hop:(j + 1) * hop]
            assert np.array_equal(got, want), (b, j)
    stats = net.stats.cpu().numpy()                  # [sum of masked xent, n_valid, ...] of that step
    assert np.isfinite(stats).all() and stats[1] > 0
    assert 0.0 < stats[0] / stats[1] < 2.0 * np.log(256.0), stats

    base = ['--gen-seconds', '0.05', '--batch-size', '2', '--chunk-size', '200', '--seed', '7', str(af),
            pfx + '.net-2']
    wav = generate.main(['--mel-from-wav', str(tmp_path / 'a.wav'), '--mel-config',
                         str(tmp_path / 'data' / 'mel_config.json')] + base + [str(tmp_path / 'out1')])
    assert wav.shape == (2, 800) and np.isfinite(wav).all()
    mel = MelSpectrogram.from_config(cfg)(generate.load_teacher(str(tmp_path / 'a.wav'), SR)).cpu().numpy()
    np.save(tmp_path / 'mel.npy', mel)
    wav2 = generate.main(['--mel-npy', str(tmp_path / 'mel.npy')] + base + [str(tmp_path / 'out2')])
    assert np.array_equal(wav, wav2)
