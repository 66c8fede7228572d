"""Host half of the log-mel front end (include/lbwn.h, lbwn_mel_*), no GPU: the filterbank
against the float64 restatement (tests/mel_ref.py), the frame count, every refusal of the envelope with
the argument's name, the configuration round trip and the CLIs' argument handling."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import mel_ref
from tests.conftest import ROOT


def cfg_of(**kw):
    from lbwn import _lib
    d = dict(sample_rate=16000, n_fft=1024, win_length=None, hop=256, n_mels=80, fmin=0.0, fmax=None, power=2,
             htk=0, norm=1, log_floor=1e-5)
    d.update(kw)
    if d['win_length'] is None:
        d['win_length'] = d['n_fft']
    if d['fmax'] is None:
        d['fmax'] = d['sample_rate'] / 2.0
    return _lib.MelCfg(**d)


def create(lib, cfg):
    h = ctypes.c_void_p()
    ret = lib.lbwn_mel_plan_create(ctypes.byref(cfg), ctypes.byref(h))
    return ret, h


FB_CASES = [
    dict(sample_rate=16000, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0),
    dict(sample_rate=16000, n_fft=64, n_mels=8, hop=16, htk=1),
    dict(sample_rate=16000, n_fft=1024, n_mels=80, norm=0),
    dict(sample_rate=22050, n_fft=512, n_mels=40, fmin=55.0, fmax=7600.0, hop=128),
    dict(sample_rate=16000, n_fft=256, n_mels=20, hop=64, htk=1, norm=0),
]


@pytest.mark.parametrize('case', FB_CASES, ids=lambda c: '-'.join('%s%s' % kv for kv in sorted(c.items())))
def test_filterbank_matches_float64(lib, case):
    """lbwn_mel_filterbank is the float64 formula rounded once to f32: within one f32 rounding, half an
    ulp of the f32 value, plus an absolute 1e-12 of the largest weight for the last-bit freedom of the
    libm log / exp / pow behind the mel points (~1e-15 relative in double, amplified by up to
    p / (p_j+1 - p_j) ~ 1e2 in the triangle's quotient).  Every bin feeds at most two bands and no band is
    empty."""
    cfg = cfg_of(**case)
    ret, h = create(lib, cfg)
    assert ret == 0, lib.lbwn_last_error()
    nb = cfg.n_fft // 2 + 1
    fb = np.empty((nb, cfg.n_mels), np.float32)
    assert lib.lbwn_mel_filterbank(h, fb.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    lib.lbwn_mel_plan_destroy(h)
    ref = mel_ref.filterbank(cfg.sample_rate, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax, bool(cfg.htk), bool(cfg.norm))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(fb.astype(np.float64) - ref)
    assert np.all(err <= 0.5 * ulp + 1e-12 * np.abs(ref).max()), float((err / ulp).max())
    assert ((fb != 0).sum(axis=1) <= 2).all()
    assert ((fb != 0).sum(axis=0) >= 1).all()
    assert (fb >= 0).all()


def test_frame_count(lib):
    for n_fft, hop in ((1024, 256), (64, 16), (64, 64), (256, 4)):
        ret, h = create(lib, cfg_of(n_fft=n_fft, hop=hop, n_mels=8 if n_fft < 1024 else 80))
        assert ret == 0, lib.lbwn_last_error()
        f = lambda n: lib.lbwn_mel_frames(h, n)
        assert f(n_fft // 2) == 0
        assert f(n_fft // 2 + 1) == (n_fft // 2 + 1) // hop
        assert f(hop - 1) == 0
        assert f(0) == 0 and f(-5) == 0
        for k in (3, 7, 100):
            n = k * hop
            want = k if n > n_fft // 2 else 0
            assert f(n) == want == mel_ref.frames_of(n, n_fft, hop)
            n = k * hop + hop - 1
            want = k if n > n_fft // 2 else 0
            assert f(n) == want == mel_ref.frames_of(n, n_fft, hop)
        assert lib.lbwn_mel_workspace_bytes(h) >= 4 * (n_fft * (n_fft // 2 + 1) * 2 + (n_fft // 2 + 1) * 8)
        lib.lbwn_mel_plan_destroy(h)
    assert lib.lbwn_mel_frames(None, 4096) == 0


REFUSALS = [
    (dict(n_fft=48), b'n_fft'), (dict(n_fft=32, hop=16, n_mels=4), b'n_fft'), (dict(n_fft=4096), b'n_fft'),
    (dict(n_fft=1000), b'n_fft'),
    (dict(hop=0), b'hop'), (dict(hop=2), b'hop'), (dict(hop=258), b'hop'), (dict(hop=2048), b'hop'),
    (dict(win_length=1), b'win_length'), (dict(win_length=1025), b'win_length'),
    (dict(n_mels=0), b'n_mels'), (dict(n_mels=82), b'n_mels'), (dict(n_mels=132), b'n_mels'),
    (dict(fmin=-1.0), b'fmin'), (dict(fmin=4000.0, fmax=4000.0), b'fmin'), (dict(fmin=5000.0, fmax=4000.0), b'fmin'),
    (dict(fmax=8000.5), b'fmax'), (dict(fmax=float('nan')), b'fm'),
    (dict(power=0), b'power'), (dict(power=3), b'power'),
    (dict(log_floor=-1e-5), b'log_floor'), (dict(log_floor=float('inf')), b'log_floor'),
    (dict(log_floor=float('nan')), b'log_floor'),
    (dict(n_fft=64, hop=16, n_mels=128), b'empty'),         # 33 bins cannot feed 128 bands
    (dict(n_fft=2048, hop=2048), b'LDS'),                     # 31·2048 + 2048 samples: no tile fits
]


@pytest.mark.parametrize('kw,word', REFUSALS, ids=lambda v: v.decode() if isinstance(v, bytes) else
                         ','.join('%s=%s' % kv for kv in v.items()))
def test_refusals_name_the_argument(lib, kw, word):
    ret, h = create(lib, cfg_of(**kw))
    assert ret == 22, (kw, ret)
    assert word in lib.lbwn_last_error(), lib.lbwn_last_error()


def test_struct_size_and_null(lib):
    from lbwn import _lib
    cfg = cfg_of()
    size = ctypes.sizeof(_lib.MelCfg)
    assert cfg.struct_size == size
    for bad in (0, size - 4, size + 8):
        cfg.struct_size = bad
        ret, h = create(lib, cfg)
        assert ret == 22
        assert b'struct_size %d != %d' % (bad, size) in lib.lbwn_last_error()
    cfg.struct_size = size
    ret, h = create(lib, cfg)
    assert ret == 0
    # the mirror has the header's fields in the header's order
    import re
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_mel_cfg \{(.*?)\} lbwn_mel_cfg;', txt, re.S).group(1)
    fields = [re.findall(r'\w+', piece)[-1] for decl in body.split(';') for piece in decl.split(',') if piece.strip()]
    assert fields == [n for n, _ in _lib.MelCfg._fields_], fields
    # refusals of the launching calls come before any device work
    assert lib.lbwn_mel_forward(h, None, None, 0, 1, 4096, None, 0, None) == 22
    assert b'null' in lib.lbwn_last_error()
    assert lib.lbwn_mel_init(h, None, None) == 22
    assert lib.lbwn_mel_forward(h, 256, 16, 4096, 1, 512, 16, 0, None) == 22       # 512 samples: no frame
    assert b'n_samples' in lib.lbwn_last_error()
    assert lib.lbwn_mel_forward(h, 256, 20, 4096, 1, 4096, 16, 0, None) == 22      # wav not 16-byte aligned
    assert b'aligned' in lib.lbwn_last_error()
    assert lib.lbwn_mel_forward(h, 256, 16, 4098, 2, 4096, 16, 1 << 20, None) == 22
    assert b'ld_wav' in lib.lbwn_last_error()
    assert lib.lbwn_mel_forward(h, 256, 16, 4096, 2, 4096, 16, 100, None) == 22
    assert b'ld_out_stream' in lib.lbwn_last_error()
    assert lib.lbwn_mel_forward(h, 256, 16, 4096, 0, 4096, 16, 1 << 20, None) == 22
    assert b'batch' in lib.lbwn_last_error()
    lib.lbwn_mel_plan_destroy(h)


def test_config_round_trip():
    from lbwn.mel import MelSpectrogram
    ms = MelSpectrogram(22050, 128, 40, n_fft=512, win_length=400, fmin=55.0, fmax=7600.0, power=1, htk=True,
                        norm=False, log_floor=0.0)
    cfg = ms.config()
    assert cfg == dict(sample_rate=22050, n_fft=512, win_length=400, hop=128, n_mels=40, fmin=55.0, fmax=7600.0,
                       power=1, htk=True, norm=False, log_floor=0.0)
    assert json.loads(json.dumps(cfg)) == cfg
    again = MelSpectrogram.from_config(json.loads(json.dumps(cfg)))
    assert again.config() == cfg
    np.testing.assert_array_equal(again.filterbank(), ms.filterbank())
    assert ms.frames(128 * 9 + 5) == 9 and ms.frames(256) == 0
    d = MelSpectrogram(16000, 256, 80)
    assert d.config() == dict(sample_rate=16000, n_fft=1024, win_length=1024, hop=256, n_mels=80, fmin=0.0,
                              fmax=8000.0, power=2, htk=False, norm=True, log_floor=1e-5)
    assert d.filterbank().shape == (513, 80)
    from lbwn import _lib
    with pytest.raises(_lib.LbwnError, match='hop'):
        MelSpectrogram(16000, 250, 80)


def run_generate(argv, capsys):
    """generate.main in this process: (exit code, stderr)."""
    import generate
    with pytest.raises(SystemExit) as e:
        generate.main(argv)
    return e.value.code, capsys.readouterr().err


def test_generate_refuses_both_mel_sources(tmp_path, capsys):
    code, err = run_generate(['--mel-from-wav', 'a.wav', '--mel-npy', 'a.npy', os.path.join(ROOT, 'par', 'arch5.json'),
                              str(tmp_path / 'none'), str(tmp_path / 'out')], capsys)
    assert code == 1
    assert '--mel-from-wav' in err and '--mel-npy' in err


@pytest.mark.parametrize('field,value', [('hop', 128), ('n_mels', 40)])
def test_generate_refuses_mel_config_mismatch(tmp_path, capsys, field, value):
    """par/arch5.json is LC 80 -> 80 at hop 256: a mel_config.json with another hop or n_mels is refused,
    naming both sides, before the checkpoint is even looked for."""
    cfg = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop=256, n_mels=80, fmin=0.0, fmax=8000.0, power=2,
               htk=False, norm=True, log_floor=1e-5)
    cfg[field] = value
    path = tmp_path / 'mel_config.json'
    path.write_text(json.dumps(cfg))
    code, err = run_generate(['--mel-from-wav', 'a.wav', '--mel-config', str(path),
                              os.path.join(ROOT, 'par', 'arch5.json'), str(tmp_path / 'none'), str(tmp_path / 'out')],
                             capsys)
    assert code == 1
    assert 'hop %d' % cfg['hop'] in err and 'n_mels %d' % cfg['n_mels'] in err
    assert 'hop 256' in err and 'n_lc_in 80' in err


def test_generate_mel_config_needs_mel_from_wav(tmp_path, capsys):
    code, err = run_generate(['--mel-config', 'c.json', os.path.join(ROOT, 'par', 'arch5.json'),
                              str(tmp_path / 'none'), str(tmp_path / 'out')], capsys)
    assert code == 1 and '--mel-config needs --mel-from-wav' in err


GOOD_CFG = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop=256, n_mels=80, fmin=0.0, fmax=8000.0, power=2,
                htk=False, norm=True, log_floor=1e-5)


def bad_configs():
    lacking = {k: v for k, v in GOOD_CFG.items() if k != 'hop'}
    return [('lacks', json.dumps(lacking), 'lacks hop'),
            ('unknown', json.dumps(dict(GOOD_CFG, window='hann')), 'window'),
            ('list', json.dumps([1, 2]), 'JSON object'),
            ('not_json', '{"hop": ', '--mel-config')]


@pytest.mark.parametrize('name,text,word', bad_configs(), ids=[c[0] for c in bad_configs()])
def test_clis_report_a_bad_mel_config_by_name(tmp_path, capsys, name, text, word):
    """A mel_config.json with a key missing, an unknown key, or that is no JSON object: generate.py and
    make_mels.py exit(1) with a message naming it, not a traceback; no GPU is touched."""
    import make_mels
    path = tmp_path / 'mel_config.json'
    path.write_text(text)
    arch5 = os.path.join(ROOT, 'par', 'arch5.json')
    code, err = run_generate(['--mel-from-wav', 'a.wav', '--mel-config', str(path), arch5, str(tmp_path / 'none'),
                              str(tmp_path / 'out')], capsys)
    assert code == 1 and word in err and str(path) in err, err
    (tmp_path / 'in.txt').write_text('')
    with pytest.raises(SystemExit) as e:
        make_mels.main(['--mel-config', str(path), arch5, os.path.join(ROOT, 'par', 'par1.json'),
                        str(tmp_path / 'in.txt'), str(tmp_path / 'data'), str(tmp_path / 'cat.txt')])
    err = capsys.readouterr().err
    assert e.value.code == 1 and word in err and str(path) in err, err


def test_make_mels_refuses_a_raw_arch(tmp_path, capsys):
    """train.py's batches carry the audio as int32, so a float catalogue would train on zeros: make_mels.py
    writes mu-law codes and refuses an arch that asks for raw input, naming wav_input_type; no GPU."""
    import make_mels
    arch = json.load(open(os.path.join(ROOT, 'par', 'arch5.json')))
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(dict(arch, wav_input_type='raw')))
    (tmp_path / 'in.txt').write_text('')
    with pytest.raises(SystemExit) as e:
        make_mels.main([str(af), os.path.join(ROOT, 'par', 'par1.json'), str(tmp_path / 'in.txt'),
                        str(tmp_path / 'data'), str(tmp_path / 'cat.txt')])
    assert e.value.code == 1 and 'wav_input_type' in capsys.readouterr().err
    assert not os.path.exists(tmp_path / 'cat.txt') and not os.path.exists(tmp_path / 'data')


def test_from_config_names_what_is_wrong():
    from lbwn.mel import MelSpectrogram
    with pytest.raises(ValueError, match='lacks sample_rate, n_mels'):
        MelSpectrogram.from_config(dict(hop=256))
    with pytest.raises(ValueError, match='unknown key.*center'):
        MelSpectrogram.from_config(dict(sample_rate=16000, hop=256, n_mels=80, center=True))
    ms = MelSpectrogram.from_config(dict(sample_rate=16000, hop=256, n_mels=80))      # the rest defaults
    assert ms.config() == GOOD_CFG
