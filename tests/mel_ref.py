"""Float64 restatement of the log-mel front end (include/lbwn.h, "log-mel front end"), in
plain numpy: framing by indexing, explicit windowed DFT matrices, the filterbank formula.  ``dtype``
float32 gives the twin: the same direct sums with every array cast to float32.  Uses nothing of the
product (no MelSpectrogram, no make_mels)."""
import numpy as np


def hz_to_mel(f, htk):
    f = np.asarray(f, np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep,
                    f / f_sp)


def mel_to_hz(m, htk):
    m = np.asarray(m, np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def filterbank(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None, htk=False, norm=True):
    """[n_fft/2+1][n_mels] float64."""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    m_lo, m_hi = float(hz_to_mel(fmin, htk)), float(hz_to_mel(fmax, htk))
    pts = mel_to_hz(m_lo + (m_hi - m_lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1), htk)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    lo, ce, hi = pts[:-2][None, :], pts[1:-1][None, :], pts[2:][None, :]
    w = np.maximum(0.0, np.minimum((f[:, None] - lo) / (ce - lo), (hi - f[:, None]) / (hi - ce)))
    if norm:
        w = w * (2.0 / (hi - lo))
    return w


def frames_of(n, n_fft, hop):
    return n // hop if n > n_fft // 2 else 0


def frame_index(n, n_fft, hop):
    """[F][n_fft] sample indices: frame t centred at t*hop, reflect padding without the edge repeated."""
    F = frames_of(n, n_fft, hop)
    i = np.arange(F, dtype=np.int64)[:, None] * hop + np.arange(n_fft, dtype=np.int64)[None, :] - n_fft // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    assert i.min() >= 0 and i.max() < n
    return i


def window(n_fft, win_length):
    w = np.zeros(n_fft, np.float64)
    off = (n_fft - win_length) // 2
    j = np.arange(win_length, dtype=np.float64)
    w[off:off + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win_length)
    return w


def basis(n_fft, win_length):
    """Windowed DFT matrices Cw, Sw [n_fft][n_fft/2+1] in float64, the angle reduced as (j*k) mod n_fft."""
    j = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((j * k) % n_fft).astype(np.float64) / n_fft
    w = window(n_fft, win_length)[:, None]
    return w * np.cos(ang), w * np.sin(ang)


def mel(x, sample_rate, n_fft, hop, n_mels, win_length=None, fmin=0.0, fmax=None, power=2, htk=False, norm=True,
        log_floor=1e-5, dtype=np.float64):
    """x [n] -> [F][n_mels] in ``dtype`` (float64: the reference; float32: the twin)."""
    win_length = n_fft if win_length is None else win_length
    x = np.asarray(x).astype(dtype)
    fr = x[frame_index(len(x), n_fft, hop)]
    cw, sw = (m.astype(dtype) for m in basis(n_fft, win_length))
    fb = filterbank(sample_rate, n_fft, n_mels, fmin, fmax, htk, norm).astype(np.float32).astype(dtype)
    re, im = fr @ cw, fr @ sw
    p = re * re + im * im
    if power == 1:
        p = np.sqrt(p)
    m = p @ fb
    assert m.dtype == dtype
    if log_floor > 0:
        m = np.log(np.maximum(m, dtype(log_floor)))
    return m


def test_signal(n, sample_rate=16000, seed=0):
    """Three harmonics plus Gaussian noise at 0.05 from default_rng(seed), rounded to f32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = 0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.25 * np.sin(2 * np.pi * 440.0 * t + 0.3) \
        + 0.125 * np.sin(2 * np.pi * 660.0 * t + 1.1) + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32)


test_signal.__test__ = False
