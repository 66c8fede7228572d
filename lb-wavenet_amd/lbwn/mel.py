"""Log-mel front end on the device: wav -> the LC conditioning rows (include/lbwn.h, lbwn_mel_*).

The reference made its mels offline with librosa; this is that transform (center=True,
pad_mode='reflect', minus librosa's last frame, so len(wav) == len(mel)·hop as data.py:143 wants) as one
launch of liblbwn.so.  There is no CPU path: ``__call__`` needs the GPU; the configuration, the frame
count and the filterbank are host-only.
"""
import ctypes

import numpy as np
import torch

from . import _lib

CONFIG_KEYS = ('sample_rate', 'n_fft', 'win_length', 'hop', 'n_mels', 'fmin', 'fmax', 'power', 'htk', 'norm',
               'log_floor')


REQUIRED_KEYS = ('sample_rate', 'hop', 'n_mels')


def check_config(cfg):
    """ValueError naming what is wrong with a mel config dict (e.g. a parsed mel_config.json)."""
    if not isinstance(cfg, dict):
        raise ValueError('a mel config is a JSON object of {}, got {}'.format(', '.join(CONFIG_KEYS),
                                                                              type(cfg).__name__))
    missing = [k for k in REQUIRED_KEYS if k not in cfg]
    if missing:
        raise ValueError('mel config lacks {}'.format(', '.join(missing)))
    unknown = sorted(k for k in cfg if k not in CONFIG_KEYS)
    if unknown:
        raise ValueError('mel config has unknown key(s) {} (known: {})'.format(', '.join(map(str, unknown)),
                                                                             ', '.join(CONFIG_KEYS)))


class MelSpectrogram:
    def __init__(self, sample_rate, hop, n_mels, n_fft=1024, win_length=None, fmin=0.0, fmax=None, power=2,
                 htk=False, norm=True, log_floor=1e-5, device='cuda'):
        self.sample_rate, self.hop, self.n_mels, self.n_fft = int(sample_rate), int(hop), int(n_mels), int(n_fft)
        self.win_length = self.n_fft if win_length is None else int(win_length)
        self.fmin = float(fmin)
        self.fmax = self.sample_rate / 2.0 if fmax is None else float(fmax)
        self.power, self.htk, self.norm, self.log_floor = int(power), bool(htk), bool(norm), float(log_floor)
        self.device = device
        self._lib = _lib.load()
        cfg = _lib.MelCfg(sample_rate=self.sample_rate, n_fft=self.n_fft, win_length=self.win_length, hop=self.hop,
                          n_mels=self.n_mels, fmin=self.fmin, fmax=self.fmax, power=self.power, htk=int(self.htk),
                          norm=int(self.norm), log_floor=self.log_floor)
        h = ctypes.c_void_p()
        _lib.check(self._lib.lbwn_mel_plan_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._plan = h
        self._ws = None

    def __del__(self):
        plan, self._plan = getattr(self, '_plan', None), None
        if plan is not None and getattr(self, '_lib', None) is not None:
            if self._ws is not None and torch.cuda.is_available():
                torch.cuda.synchronize()      # the init's filterbank copy reads plan-owned memory
            self._lib.lbwn_mel_plan_destroy(plan)

    def config(self):
        """lbwn_mel_cfg's settings (all but struct_size) as a plain dict: what make_mels.py writes as
        mel_config.json."""
        return {k: getattr(self, k) for k in CONFIG_KEYS}

    @classmethod
    def from_config(cls, cfg, device='cuda'):
        """From a dict of config()'s keys.  sample_rate, hop and n_mels are required, the rest default as in
        the constructor; a missing required key, an unknown key or a non-dict is a ValueError naming it."""
        check_config(cfg)
        return cls(device=device, **cfg)

    def frames(self, n):
        """Frames of a signal of n samples: n // hop, or 0 when the length is refused (n <= n_fft/2)."""
        return int(self._lib.lbwn_mel_frames(self._plan, int(n)))

    def filterbank(self):
        """The [n_fft/2+1, n_mels] float32 filterbank (host-only)."""
        fb = np.empty((self.n_fft // 2 + 1, self.n_mels), np.float32)
        _lib.check(self._lib.lbwn_mel_filterbank(self._plan, fb.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return fb

    def workspace(self):
        """The device tables (basis + filterbank), filled on first use."""
        if self._ws is None:
            nbytes = int(self._lib.lbwn_mel_workspace_bytes(self._plan))
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            _lib.check(self._lib.lbwn_mel_init(self._plan, _lib.ptr(ws), _lib.stream_ptr()))
            self._ws = ws
        return self._ws

    def forward_into(self, wav, out):
        """wav [B][ld_wav-strided rows of n], out [B][>= F*n_mels-strided]: the raw call, for tests and graphs."""
        B, n = wav.shape
        _lib.check(self._lib.lbwn_mel_forward(self._plan, _lib.ptr(self.workspace()), _lib.ptr(wav), wav.stride(0), B,
                                              n, _lib.ptr(out), out.stride(0), _lib.stream_ptr()))
        return out

    def __call__(self, wav):
        if isinstance(wav, np.ndarray):
            wav = torch.from_numpy(np.array(wav, dtype=np.float32))      # a copy: the input may be read-only
        single = wav.dim() == 1
        if wav.dim() not in (1, 2):
            raise ValueError('wav must be [n] or [B][n], got shape %s' % (tuple(wav.shape),))
        x = wav.to(device=self.device, dtype=torch.float32)
        x = x[None] if single else x
        B, n = x.shape
        F = self.frames(n)
        if F < 1:
            raise _lib.LbwnError('a signal of %d samples gives no frame: needs more than n_fft/2 = %d samples and at '
                                 'least hop = %d' % (n, self.n_fft // 2, self.hop))
        ld = (n + 3) // 4 * 4              # rows 16-byte aligned (lbwn_mel_forward: ld_wav a multiple of 4)
        buf = torch.empty(B, ld, dtype=torch.float32, device=self.device)
        buf[:, :n] = x
        out = torch.empty(B, F, self.n_mels, dtype=torch.float32, device=self.device)
        self.forward_into(buf[:, :n], out.view(B, F * self.n_mels))
        return out[0] if single else out
