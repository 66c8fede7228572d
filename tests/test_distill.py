"""Distillation and label smoothing without a GPU: the ctypes mirror of lbwn_forward_args,
lbwn_train_forward_ex's refusals (all made before the device is touched), tests/distill_ref.py against
the oracle's own loss and against central differences of its own value, Distiller's constructor
refusals and train.py's option errors."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from lbwn import _lib
from oracle import wavenet_ref as R
from tests import distill_ref as D
from tests import eval_ref as E
from tests.conftest import ROOT
from tests.test_eval import _plan


# ---- C ABI ------------------------------------------------------------------------------------------
def test_forward_args_mirror_matches_header():
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_forward_args \{(.*?)\} lbwn_forward_args;', txt, re.S).group(1)
    fields = [re.findall(r'\w+', piece)[-1] for decl in body.split(';') for piece in decl.split(',') if piece.strip()]
    assert fields == [n for n, _ in _lib.ForwardArgs._fields_], fields
    assert fields == ['struct_size', 'wav_q', 'ids', 'mel', 'save', 'stats', 'stats_ex', 'teacher_logits',
                      'ld_teacher', 'distill_alpha', 'distill_temp', 'label_smoothing']
    assert {'lbwn_train_forward_ex', 'lbwn_head_xent_ex'} <= set(_lib.EXPORTED)
    assert re.search(r'#define LBWN_ABI_VERSION 5\b', txt)


def test_train_forward_ex_refusals_without_gpu(lib):
    """Every refusal of include/lbwn.h is EINVAL with the argument's name in lbwn_last_error, on a
    host-only plan and with pointers nothing ever dereferences."""
    T = 64
    h = _plan(lib, E.ARCHS['chain'](), 2, T)
    hc = _plan(lib, E.ARCHS['cond'](), 2, T)
    P = _lib.Params()
    WS = 0x10000000
    ok = dict(wav_q=0x1000, ids=0x2000, mel=None, save=0x3000, stats=0x4000, stats_ex=None, teacher_logits=0x100000,
              ld_teacher=256, distill_alpha=0.5, distill_temp=2.0, label_smoothing=0.1)

    def refused(word, plan=h, params=P, ws=WS, args=True, size=None, **kw):
        a = _lib.ForwardArgs(**dict(ok, **kw))
        if size is not None:
            a.struct_size = size
        ret = lib.lbwn_train_forward_ex(plan, ctypes.byref(params) if params is not None else None, ws,
                                        ctypes.byref(a) if args else None, None)
        msg = lib.lbwn_last_error().decode()
        assert ret == 22 and word in msg, (ret, word, msg)

    refused('plan', plan=None)
    refused('params', params=None)
    refused('workspace', ws=None)
    refused('args', args=False)
    refused('struct_size', size=ctypes.sizeof(_lib.ForwardArgs) - 8)
    for name in ('wav_q', 'ids', 'save', 'stats'):
        refused(name, **{name: None})
    refused('mel', plan=hc)
    for bad in (-0.01, 1.01, float('nan')):
        refused('distill_alpha', distill_alpha=bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        refused('distill_temp', distill_temp=bad)
    for bad in (-0.1, 1.0, float('nan')):
        refused('label_smoothing', label_smoothing=bad)
    refused('teacher_logits', teacher_logits=None)                      # alpha > 0 without a teacher
    refused('teacher_logits', teacher_logits=0x100008)                  # not 16-byte aligned
    refused('ld_teacher', ld_teacher=252)                               # < n_quant
    refused('ld_teacher', ld_teacher=258)                               # not a multiple of 4
    nbytes = lib.lbwn_plan_workspace_bytes(h)
    tbytes = 4 * ((2 * T - 1) * 256 + 256)
    for t in (WS, (WS + nbytes - 16) & ~15, WS - tbytes + 16, WS + 4096):      # any overlap with [WS, WS + nbytes)
        refused('overlaps', teacher_logits=t)
    # the other neutral options do not lift a refusal that does not depend on them
    refused('distill_temp', distill_alpha=0.0, label_smoothing=0.0, teacher_logits=None, distill_temp=0.0)
    # lbwn_head_xent_ex checks its scalars too
    for kw, word in ((dict(alpha=1.5), 'alpha'), (dict(temp=0.0), 'temp'), (dict(eps=1.0), 'smoothing'),
                     (dict(teacher=None), 'teacher')):
        v = dict(dict(alpha=0.5, temp=1.0, eps=0.0, teacher=0x100000), **kw)
        ret = lib.lbwn_head_xent_ex(0x1000, 0x2000, 0x3000, 2, 9, 8, v['teacher'], 8, v['alpha'], v['temp'], v['eps'],
                                    0x4000, None, 0x5000, None)
        assert ret == 22 and word in lib.lbwn_last_error().decode(), (kw, lib.lbwn_last_error())
    for p in (h, hc):
        lib.lbwn_plan_destroy(p)


# ---- the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chain', 'cond'])
def test_neutral_head_is_the_oracle_loss(name):
    arch, P, S, slices = E.case(name)
    q, ids, mel = slices[0]
    lg, _, _ = R.forward(arch, P, q, ids, S, mel=mel)
    st, dlog = R.loss_fcn(arch, P, lg, q, ids, 0.0)
    for teacher, temp in ((None, 1.0), (lg[::-1], 3.0)):        # alpha = 0: teacher and temperature without effect
        value, dl, stats, ex = D.head(lg, teacher, q, ids, 0.0, temp, 0.0)
        np.testing.assert_allclose(stats[0], st['sum_xent'], rtol=1e-13)
        np.testing.assert_allclose(ex[0], st['sum_xent'], rtol=1e-13)
        assert stats[1] == st['n_valid'] and stats[2] == st['sum_absdiff'] and ex[1] == 0 and ex[2] == ex[3] == 0
        np.testing.assert_allclose(dl / st['n_valid'], dlog, rtol=0, atol=1e-15)
        assert np.all(dl[:, -1] == 0) and np.all(value[:, -1] == 0)


@pytest.mark.parametrize('alpha,temp,eps', [(0.0, 1.0, 0.1), (0.5, 1.0, 0.0), (0.5, 2.0, 0.1), (1.0, 0.5, 0.0),
                                            (1.0, 2.0, 0.0)])
def test_dlogits_are_the_central_differences_of_the_value(alpha, temp, eps):
    """float64: d(Σ value)/d(logit) by central differences (h = 1e-5 on logits of N(0, 3²): the h² error
    term is ~1e-10) agrees with dlogits within 1e-6 of max|dlogits|, at every element of a Q = 12 case
    with a masked run, code 0 and code Q-1 among the targets and an underflowing teacher probability."""
    Q = 12
    lg, te, q, ids = D.kernel_case(Q, T=6)
    lg, te = lg.astype(np.float64), te.astype(np.float64)
    te[0, 1, 3] = te[0, 1].max() - 2000.0                     # pT = 0 exactly in float64 too
    value, dl, stats, ex = D.head(lg, te, q, ids, alpha, temp, eps)
    assert np.isfinite(value).all() and np.isfinite(dl).all()
    np.testing.assert_allclose(stats[0], value.sum(), rtol=1e-14)
    num = np.zeros_like(dl)
    h = 1e-5
    for idx in np.ndindex(*lg.shape):
        a, b = lg.copy(), lg.copy()
        a[idx] += h
        b[idx] -= h
        num[idx] = (D.head(a, te, q, ids, alpha, temp, eps)[2][0] - D.head(b, te, q, ids, alpha, temp, eps)[2][0]) / (2 * h)
    err = np.max(np.abs(num - dl))
    assert err <= 1e-6 * np.max(np.abs(dl)), (err, np.max(np.abs(dl)))
    scored = np.zeros(q.shape, bool)
    scored[:, :-1] = ids[:, 1:] != 0
    assert np.all(dl[~scored] == 0) and np.all(value[~scored] == 0) and (~scored[:, :-1]).any()
    if alpha > 0:
        assert ex[1] > 0
    if alpha == 1.0:
        np.testing.assert_allclose(stats[0], temp * temp * ex[1], rtol=1e-13)


def test_twin_is_the_reference_in_float32():
    lg, te, q, ids = D.kernel_case(260)
    ref = D.head(lg, te, q, ids, 0.5, 2.0, 0.1)
    tw = D.twin(lg, te, q, ids, 0.5, 2.0, 0.1)
    assert tw[0].dtype == np.float32 and tw[1].dtype == np.float32
    err = np.max(np.abs(tw[1].astype(np.float64) - ref[1]))
    assert 0 < err < 1e-5
    assert np.array_equal(tw[2][1:3], ref[2][1:3])
    np.testing.assert_allclose(tw[2][0], ref[2][0], rtol=1e-5)
    np.testing.assert_allclose(tw[3][:2], ref[3][:2], rtol=1e-5)


# ---- Distiller --------------------------------------------------------------------------------------
def _stub(arch, B=2):
    return SimpleNamespace(arch=arch, batch_sz=B)


def test_distiller_constructor_refusals():
    from lbwn.distill import Distiller, check_pair
    chain, cond = E.ARCHS['chain'](), E.ARCHS['cond']()
    with pytest.raises(ValueError, match='n_quant'):
        Distiller(_stub(E.ARCHS['q64']()), _stub(chain), 0.5, 1.0)
    with pytest.raises(ValueError, match='n_lc_in'):
        Distiller(_stub(dict(cond, n_lc_in=8)), _stub(cond), 0.5, 1.0)
    with pytest.raises(ValueError, match='n_lc_in'):                # an LC teacher, a student without LC
        Distiller(_stub(chain), _stub(cond), 0.5, 1.0)
    with pytest.raises(ValueError, match='hop'):
        Distiller(_stub(dict(cond, lc_upsample=[2, 4])), _stub(cond), 0.5, 1.0)
    with pytest.raises(ValueError, match='n_gc_category'):
        Distiller(_stub(dict(cond, n_gc_category=9)), _stub(cond), 0.5, 1.0)
    with pytest.raises(ValueError, match='batch_sz'):
        Distiller(_stub(chain, 2), _stub(chain, 3), 0.5, 1.0)
    for kw, word in ((dict(alpha=1.5), 'alpha'), (dict(temp=0.0), 'temp'), (dict(label_smoothing=1.0), 'label_smoothing')):
        with pytest.raises(ValueError, match=word):
            Distiller(_stub(chain), _stub(chain), **dict(dict(alpha=0.5, temp=1.0), **kw))
    # pairs that may be trained: a shallower student, a teacher with more voices
    check_pair(dict(chain, n_blocks=1), chain, 2, 2)
    check_pair(cond, dict(cond, n_gc_category=9), 2, 2)


# ---- train.py ---------------------------------------------------------------------------------------
def test_train_distill_option_errors(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import train
    arch, par = os.path.join(ROOT, 'par', 'arch3.json'), os.path.join(ROOT, 'par', 'par1.json')
    tail = [str(tmp_path / 'ck'), arch, par, 'none.txt']
    teacher = ['--teacher-arch', arch, '--teacher-ckpt', 't.safetensors']
    for argv, word in ((['--teacher-ckpt', 't.safetensors'], '--teacher-ckpt needs --teacher-arch'),
                       (['--teacher-arch', arch], '--teacher-arch needs --teacher-ckpt'),
                       (['--distill-alpha', '0.3'], '--distill-alpha needs a teacher'),
                       (['--distill-temp', '2'], '--distill-temp needs a teacher'),
                       (['--teacher-ema'], '--teacher-ema needs a teacher'),
                       (teacher + ['--distill-alpha', '1.5'], '--distill-alpha must be in [0, 1]'),
                       (teacher + ['--distill-alpha', '-0.1'], '--distill-alpha must be in [0, 1]'),
                       (teacher + ['--distill-temp', '0'], '--distill-temp must be finite and > 0'),
                       (teacher + ['--distill-temp', 'inf'], '--distill-temp must be finite and > 0'),
                       (teacher + ['--label-smoothing', '1'], '--label-smoothing must be in [0, 1)'),
                       (['--label-smoothing', '-0.5'], '--label-smoothing must be in [0, 1)'),
                       (teacher + ['--valid-file', 'v.txt', '--eval-only', '--resume-step', '3'],
                        'cannot be combined with --eval-only')):
        with pytest.raises(SystemExit) as e:
            train.main(argv + tail)
        assert e.value.code == 1
        assert word in capsys.readouterr().err, argv
    opt = lambda argv: train.distill_options(train.override_par(train.get_args(argv + ['p', 'a', 'b', 'c']), {}))  # noqa: E731
    assert opt([]) == dict(teacher_arch=None, teacher_ckpt=None, teacher_ema=False, alpha=0.0, temp=1.0, smoothing=0.0)
    assert opt(['--label-smoothing', '0.1', '--distill-alpha', '0'])['smoothing'] == 0.1
    got = opt(teacher + ['--teacher-ema'])
    assert (got['alpha'], got['temp'], got['teacher_ema'], got['teacher_ckpt']) == (0.5, 1.0, True, 't.safetensors')
    assert opt(teacher + ['--distill-alpha', '1', '--distill-temp', '2.5'])['temp'] == 2.5
