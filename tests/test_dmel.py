"""dmel, the gradient with respect to the mel input, without a GPU: the float64 reference
of tests/dmel_ref.py against central differences of the oracle's loss, the exact-zero rule on it, the
kernel test's comparison held to both sides, and the host refusals of lbwn_train_backward_ex and of the
Python surface (no device is touched: these fail on a library without the call because the symbols do
not exist).

Central differences: f = the oracle's mean_xent in float64 as a function of the mel input,
(f(mel + eps·v) - f(mel - eps·v)) / (2·eps) at eps = 1e-5 against <dmel, v> for three standard-normal
directions v per case.  The truncation term is eps²·f'''/6 ~ 1e-10 relative and the cancellation term
2^-53·|f| / eps ~ 1e-11 absolute, against directional derivatives of 1e-3 .. 1e-2: the bar is 1e-5 of
|<dmel, v>|.  Measured on a CPU with these four cases and seeds: worst 4.7e-7 (1.1e-7 with the parameters
the bar was first tried with); the bar leaves more than an order for another BLAS.
The loss is piecewise smooth: a relu input (the skip sum S, h1) that changes sign between mel - eps·v and
mel + eps·v puts a kink inside the difference interval, and the quotient then measures no derivative
(seed 11 on GC + 8->16 [2]: 7 such elements over the three directions, quotient off by 1.7e-3; none at
eps = 1e-6, 5e-8).  That is a property of the case, not of the reference, so the test asserts it away: no
relu input changes sign inside any interval, and a case that fails that takes another parameter seed
(the last column of CASES), never another eps or bar.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from lbwn import _lib
from oracle import wavenet_ref as R
from tests.conftest import ROOT
from tests.dmel_ref import (check_kernel_dmel, check_zero_frames, dmel_ref, hop_of, kernel_dmel_ref,
                            last_scored_frame, tail_mask)
from tests.gradcheck import cond_arch, cond_batch
from tests.test_gpu_cond_kernels import lc_problem
from tests.test_gpu_cond_plan import arch_struct

# (name, GC, Li, Lo, strides, B, T, parameter seed): 1 block x 4 layers, C = 32
CASES = [
    ('12->16 [2,4] B=2', 0, 12, 16, (2, 4), 2, 256, 11),
    ('GC + 8->16 [2] B=3', 1, 8, 16, (2,), 3, 256, 12),        # seed 11: 7 relu kinks inside the intervals
    ('24->16 [2,4] B=2', 0, 24, 16, (2, 4), 2, 256, 12),       # seed 11: 3
    ('GC + 4->4 [8] B=1 T=64', 1, 4, 4, (8,), 1, 64, 11),
]
IDS = [c[0].replace(' ', '_') for c in CASES]
EPS, FD_REL = 1e-5, 1e-5


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case's arch, float64 parameters and SAVE, inputs (cond_batch with stream 0's tail masked) and
    the reference dmel; shared by the tests below and never modified."""
    _, gc, Li, Lo, strides, B, T, seed = next(c for c in CASES if c[0] == name)
    arch = cond_arch(gc, 1, 32, Li=Li, Lo=Lo, strides=strides)
    rng = np.random.default_rng(seed)
    P = R.init_params(arch, rng, bias_scale=0.1)
    S = R.init_save(arch, B, rng)
    q, ids, mel = cond_batch(arch, B, T)
    ids = tail_mask(ids, hop_of(arch))
    mel = mel.astype(np.float64)
    lg, cache, _ = R.forward(arch, P, q, ids, S, mel=mel)
    st, dlog = R.loss_fcn(arch, P, lg, q, ids, 0.0)
    dmel, _ = dmel_ref(arch, P, cache, dlog)
    return dict(arch=arch, P=P, S=S, q=q, ids=ids, mel=mel, dmel=dmel, st=st)


def mean_xent(pb, mel):
    """(the oracle's mean_xent at this mel, the signs of its relu inputs)"""
    lg, cache, _ = R.forward(pb['arch'], pb['P'], pb['q'], pb['ids'], pb['S'], mel=mel)
    signs = np.concatenate([(cache['S'] > 0).ravel(), (cache['h1'] > 0).ravel()])
    return R.loss_fcn(pb['arch'], pb['P'], lg, pb['q'], pb['ids'], 0.0)[0]['mean_xent'], signs


@pytest.mark.parametrize('name', [c[0] for c in CASES], ids=IDS)
def test_reference_matches_central_differences(name):
    pb = problem(name)
    assert pb['dmel'].shape == pb['mel'].shape and pb['dmel'].dtype == np.float64
    assert pb['st']['n_valid'] > 0
    rng = np.random.default_rng(5)
    for k in range(3):
        v = rng.standard_normal(pb['mel'].shape)
        (fp, sp), (fm, sm) = mean_xent(pb, pb['mel'] + EPS * v), mean_xent(pb, pb['mel'] - EPS * v)
        # a condition on the case, not a measurement of the reference
        assert np.array_equal(sp, sm), '%s direction %d: %d relu inputs change sign inside the interval; the ' \
            'case needs another parameter seed' % (name, k, int((sp != sm).sum()))
        fd = (fp - fm) / (2 * EPS)
        an = float(np.sum(pb['dmel'] * v))
        print('%s direction %d: fd %.12g  <dmel, v> %.12g  rel %.3g' % (name, k, fd, an, abs(fd - an) / abs(an)))
        assert abs(fd - an) <= FD_REL * abs(an), (name, k, fd, an)


@pytest.mark.parametrize('name', [c[0] for c in CASES], ids=IDS)
def test_frames_after_the_last_scored_position_are_exactly_zero(name):
    """ids[0, T - 2·hop - 5:] = 0: the last two frames of stream 0 are exactly zero, the frame holding
    its last scored position is not (and so for every stream, by its own last scored position)."""
    pb = problem(name)
    hop, T = hop_of(pb['arch']), pb['q'].shape[1]
    assert not pb['ids'][0, T - 2 * hop - 5:].any() and pb['ids'][0, T - 2 * hop - 6] != 0
    f0 = last_scored_frame(pb['ids'], hop)[0]
    assert 0 <= f0 <= T // hop - 3
    assert not np.any(pb['dmel'][0, -2:] != 0)
    assert np.any(pb['dmel'][0, f0] != 0)
    assert check_zero_frames(pb['dmel'], pb['ids'], hop, name) >= 2
    # the rule's own check: a frame that should be zero and is not, and an all-zero live frame, fail
    bad = pb['dmel'].copy()
    bad[0, -1, 0] = 1e-30
    with pytest.raises(AssertionError):
        check_zero_frames(bad, pb['ids'], hop)
    bad = pb['dmel'].copy()
    bad[0, f0] = 0.0
    with pytest.raises(AssertionError):
        check_zero_frames(bad, pb['ids'], hop)


def test_kernel_check_accepts_rounded_results_and_rejects_wrong_ones():
    """The comparison of tests/test_gpu_dmel_kernel.py itself: the float64 dmel rounded once to f32
    passes; dmel with stage 0's last phase left out, with the neighbouring frame's row, with the last
    split-K partial left out, or with one element unwritten does not."""
    # (the last: the deepest, widest chain of the list, where the bound is loosest against the rounding error)
    for Li, Lo, strides, frames, parts in ((12, 16, (2, 4), 3, 3), (4, 4, (8,), 3, 1), (68, 68, (4, 4, 4), 3, 1)):
        _, F, dlc, _ = lc_problem(Li, Lo, strides, frames, parts)
        ref, bound = kernel_dmel_ref(Li, Lo, strides, frames, F, dlc)
        assert ref.shape == bound.shape == (frames, Li) and np.all(bound > 0)
        good = ref.astype(np.float32)
        assert check_kernel_dmel('rounded', good, ref, bound) < 1.0
        mutants = {'phase': kernel_dmel_ref(Li, Lo, strides, frames, F, dlc, drop='phase')[0].astype(np.float32),
                   'neighbour': np.roll(good, 1, axis=0)}
        if parts > 1:
            mutants['part'] = kernel_dmel_ref(Li, Lo, strides, frames, F, dlc, drop='part')[0].astype(np.float32)
        unwritten = good.copy()
        unwritten[1, Li - 1] = np.nan
        mutants['unwritten'] = unwritten
        for what, bad in mutants.items():
            with pytest.raises(AssertionError):
                check_kernel_dmel(what, bad, ref, bound)


# ---- host refusals (no device) ----------------------------------------------------------------------

FAKE = 1 << 20          # a non-null, 16-byte aligned "device pointer" that no refusal dereferences


def make_plan(lib, arch, B, T):
    h = ctypes.c_void_p()
    _lib.check(lib.lbwn_plan_create(ctypes.byref(arch_struct(arch)), B, T, ctypes.byref(h)))
    return h


def info(lib, h, key):
    v = _lib.c_int64(-7)
    _lib.check(lib.lbwn_plan_info(h, key.encode(), ctypes.byref(v)))
    return v.value


def test_backward_args_mirror_matches_the_header(lib):
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_backward_args \{(.*?)\} lbwn_backward_args;', txt, re.S).group(1)
    fields = [re.findall(r'\w+', decl)[-1] for decl in body.split(';') if decl.strip()]
    assert fields == [n for n, _ in _lib.BackwardArgs._fields_], fields
    size = ctypes.sizeof(_lib.BackwardArgs)
    a = _lib.BackwardArgs()
    assert a.struct_size == size == 5 * ctypes.sizeof(ctypes.c_void_p)
    P = _lib.Params()
    for bad in (0, size - 8, size + 8):      # the library names its own sizeof when it refuses another
        a.struct_size = bad
        assert lib.lbwn_train_backward_ex(None, ctypes.byref(P), ctypes.byref(P), FAKE, ctypes.byref(a), None) == 22
        assert b'struct_size %d != %d' % (bad, size) in lib.lbwn_last_error(), lib.lbwn_last_error()
    assert {'lbwn_train_backward_ex', 'lbwn_lc_upsample_backward_dmel'} <= set(_lib.EXPORTED)


def test_train_backward_ex_refusals_without_a_device(lib):
    """Every EINVAL of the header comment, its argument named, before any launch and before the device
    is touched (this test runs where there is none); the plan's facts around it."""
    lc = cond_arch(0, 1, 32)
    h, h0 = make_plan(lib, lc, 2, 256), make_plan(lib, cond_arch(1, 0, 32), 2, 256)
    P, G = _lib.Params(), _lib.Params()
    try:
        ws_before = lib.lbwn_plan_workspace_bytes(h)
        assert info(lib, h, 'dmel_fused') == -1 and info(lib, h0, 'dmel_fused') == -1

        def call(plan, a, params=P, grads=G, ws=FAKE):
            ret = lib.lbwn_train_backward_ex(plan, ctypes.byref(params) if params is not None else None,
                                             ctypes.byref(grads) if grads is not None else None, ws,
                                             ctypes.byref(a) if a is not None else None, None)
            return ret, lib.lbwn_last_error().decode()

        def args(**kw):
            d = dict(wav_q=FAKE, ids=FAKE + 4096, mel=FAKE + 8192, dmel=FAKE + 16384)
            d.update(kw)
            return _lib.BackwardArgs(**d)
        ws_far = FAKE << 8                                    # the fake workspace, away from the fake tensors
        refused = [
            (call(h, None, ws=ws_far), 'null argument struct'),
            (call(None, args(), ws=ws_far), 'null argument'),
            (call(h, args(), params=None, ws=ws_far), 'null argument'),
            (call(h, args(), grads=None, ws=ws_far), 'null argument'),
            (call(h, args(), ws=None), 'null argument'),
            (call(h, args(wav_q=None), ws=ws_far), 'wav_q'),
            (call(h, args(ids=None), ws=ws_far), 'ids'),
            (call(h, args(mel=None), ws=ws_far), 'mel'),
            (call(h0, args(mel=None), ws=ws_far), 'dmel on an arch without local conditioning'),
            (call(h, args(dmel=FAKE + 16384 + 4), ws=ws_far), 'dmel must be 16-byte aligned'),
            (call(h, args(dmel=FAKE + 8192), ws=ws_far), 'dmel aliases mel'),
            (call(h, args(dmel=ws_far + 64), ws=ws_far), 'dmel aliases mel or the workspace'),
            # a fresh plan has no training forward, as a plan after lbwn_train_eval has none: with and without dmel
            (call(h, args(), ws=ws_far), 'no training forward'),
            (call(h, args(dmel=None), ws=ws_far), 'no training forward'),
            (call(h0, args(mel=None, dmel=None), ws=ws_far), 'no training forward'),
        ]
        for (ret, msg), want in refused:
            assert ret == 22 and want in msg, (ret, msg, want)
        # lbwn_train_backward is the same call with dmel NULL: the same refusal, the same order of checks
        assert lib.lbwn_train_backward(h, ctypes.byref(P), ctypes.byref(G), ws_far, FAKE, FAKE, FAKE, None) == 22
        assert b'no training forward' in lib.lbwn_last_error()
        assert info(lib, h, 'dmel_fused') == -1
        assert lib.lbwn_plan_workspace_bytes(h) == ws_before
    finally:
        lib.lbwn_plan_destroy(h)
        lib.lbwn_plan_destroy(h0)


def test_lc_upsample_backward_dmel_refusals_without_a_device(lib):
    """Same envelope, same refusals as lbwn_lc_upsample_backward, and its own two for dmel."""
    s = (ctypes.c_int * 2)(2, 4)
    ptrs = (_lib.c_fp * 2)(FAKE, FAKE)
    base = (2, s, 12, 16, 3, FAKE, ptrs, ptrs, FAKE, 1, 0, FAKE, ptrs)
    assert lib.lbwn_lc_upsample_backward_dmel(*base, None, None) == 22
    assert b'dmel is null' in lib.lbwn_last_error()
    assert lib.lbwn_lc_upsample_backward_dmel(*base, FAKE + 8, None) == 22
    assert b'dmel must be 16-byte aligned' in lib.lbwn_last_error()
    out = (2, s, 24, 16, 3, FAKE, ptrs, ptrs, FAKE, 1, 0, FAKE, ptrs)      # Li > Lo
    assert lib.lbwn_lc_upsample_backward_dmel(*out, FAKE, None) == 22
    assert b'envelope' in lib.lbwn_last_error()
    assert lib.lbwn_lc_upsample_backward_dmel(*base[:4], 0, *base[5:], FAKE, None) == 22
    assert b'frames' in lib.lbwn_last_error()


def test_python_surface_refusals_without_a_device():
    from lbwn.dist import DPContext
    from lbwn.tmodel import WaveNetTrain
    from lbwn.torch_ops import wavenet_loss
    lc = WaveNetTrain(**cond_arch(0, 1, 32), batch_sz=2, l2_factor=0.0, device='cpu', print_interval=0)
    plain = WaveNetTrain(**cond_arch(1, 0, 32), batch_sz=2, l2_factor=0.0, device='cpu', print_interval=0)
    q, ids, mel = cond_batch(lc.arch, 2, 256)
    assert lc.dmel is None
    with pytest.raises(ValueError, match='no local conditioning'):
        plain.forward(q, None, ids, backward=True, want_dmel=True)
    with pytest.raises(ValueError, match='backward=True'):
        lc.forward(q, mel, ids, backward=False, want_dmel=True)
    melt = torch.from_numpy(mel)
    with pytest.raises(ValueError, match='no local conditioning'):
        wavenet_loss(plain, q, melt, ids)
    with pytest.raises(ValueError, match='device tensors only'):
        wavenet_loss(lc, q, melt, ids)
    with pytest.raises(ValueError, match='float32'):
        wavenet_loss(lc, q, melt.double(), ids)
    lc.dp = DPContext(world=2, rank=0)
    with pytest.raises(ValueError, match='data parallelism'):
        wavenet_loss(lc, q, melt, ids)
    lc.dp = DPContext()       # world 1: not enabled, so the next refusal speaks
    with pytest.raises(ValueError, match='device tensors only'):
        wavenet_loss(lc, q, melt, ids)
