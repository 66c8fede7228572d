"""The conditioning kernels of csrc/cond.hip on their own inputs against float64: the fused LC
upsample (lc_up_fwd_kernel<0 / 4>, lc_up_bwd_kernel, lc_up_sum_kernel) through
lbwn_lc_upsample_forward / _backward, and the GC table and its three gradients (gc_table_kernel,
gc_wgrad_kernel, gc_egrad_part_kernel + gc_egrad_sum_kernel) through lbwn_gc_table / lbwn_gc_grads.

Reference: the einsums of oracle/wavenet_ref.py (lc_upsample_fwd / lc_upsample_bwd) and the three GC
sums of cond.hip's header comment, restated in float64 on the f32 inputs the kernel read (standard
normal, fixed seed).  Every output is allocated NaN-filled between two 64-float NaN canaries inside
one allocation: an element the kernel did not write fails the comparison, a write outside the output
fails the canary check.

Tolerance, derived and not measured: the forward error bound of a dot product, element by element,
    |got - ref| <= gamma_k * sum |a|*|b|,   gamma_k = k*u / (1 - k*u),   u = 2^-24,
the sum taken in float64 over absolute values and k the number of floating-point operations on the
longest path to the element.  It holds for any summation order, so it carries no margin.
  forward, stage i on the GPU's own act[i-1]:  k = I_i (the kernel's explicit fmaf chain)
  forward, end to end:                         k = sum of I_j over stages j <= i, through |F_i|..|F_0|·|mel|
  backward dF_i (din stays in LDS, so the bound runs through the chain):
      gamma_K * (|D_last|·|F_{nup-1}|···|F_{i+1}|)^T |IN_i|,
      K = (dlc_parts - 1) + sum_{k>i} 2·s_k·Lo + 2·R_i + frames   (two per term: no reliance on contraction)
  gc_table k = Ge;  gc_wgrad k = ncat1;  dEMB k = 2·256 + nk (nk = ceil(N / 256) chunk partials).

Worst err / bound measured on the MI355X over every case below (printed per case with -s; the
assertion is err <= bound, that is a ratio below 1):

    lc_up_fwd, stage by stage   0.54   4->4 [8], 257 frames, stage 0
    lc_up_fwd, end to end       0.54   the same element (stage 0 is both); later stages <= 0.12
                                       (stage by stage on identical inputs they reach 0.28, at k = 4)
    lc_up_bwd                   0.37   4->196 [4], 3 frames, dF[0]
    gc_table                    0.99   Ge 1; 0.28 and below for Ge >= 8
    gc_wgrad                    0.56   Ge 1, ncat1 2; 0.42 and below for ncat1 >= 6, 0.008 at ncat1 377
    gc_egrad (dEMB)             0.006

Where the ratio is above about 0.5, k is 1 .. 4 and the bound is nearly attained by construction: one
rounding of a single product can reach u·|a·b|, which is the whole bound at k = 1 (gc_table with Ge = 1),
and the stage-0 sums of a 4-wide mel (k = 4) and the two-term gc_wgrad sums are the maximum over
thousands of elements of a sum of k <= 4 roundings.  The ratio falls as k grows (a few percent from
k ~ 30, under one percent past k ~ 300), as it must for roundings that do not all point one way.
test_checks_accept_rounded_results_and_reject_wrong_ones (no GPU) holds the comparison itself to both
sides: correctly rounded results pass, eight kinds of wrong result do not.
Every case of the list is inside the library's envelope (test_lc_cases_are_inside_the_envelope):
none was replaced.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lbwn import _lib

gpu = pytest.mark.gpu
DEV = 'cuda'
G = 64                      # canary floats on each side of every output
U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# (Li, Lo, strides): what each exercises is in the table of the test below
LC_CASES = [
    (12, 16, (2, 4)),          # baseline
    (16, 16, (4, 4)),          # the SC = 4 template away from arch5
    (16, 16, (4,)),            # ... with one stage
    (4, 4, (8,)),              # narrowest, stride 8
    (8, 8, (1,)),              # stride 1
    (4, 4, (1, 1, 1, 1)),      # ... four times
    (8, 20, (3, 5)),           # odd strides
    (20, 36, (5, 3, 2)),       # three stages
    (8, 24, (8, 8, 4)),        # hop 256
    (4, 80, (4, 4, 4, 4)),     # hop 256 on the SC = 4 template, arch5's width from a narrow mel
    (68, 68, (4, 4, 4)),       # width between the padded sizes
    (4, 72, (2, 7, 1)),        # forward LDS carve-out at 40440 of 40448 floats
    (4, 196, (4,)),            # backward LDS carve-out at 40400
    (4, 44, (3, 8, 8, 1)),     # the second work item per thread of the backward's din loop
]
LONG_CASES = [(12, 16, (2, 4)), (4, 4, (8,))]                        # 257 frames: the sum kernel's grid
PARTS_CASES = [(12, 16, (2, 4)), (8, 20, (3, 5)), (4, 80, (4, 4, 4, 4))]   # dlc as 3 split-K partials
LC_RUNS = ([(c, f, 1) for c in LC_CASES for f in (1, 3)] + [(c, 257, 1) for c in LONG_CASES] +
           [(c, 3, 3) for c in PARTS_CASES])
# outside the envelope: Li > Lo, stride 9, Li % 4 != 0, hop 512, five stages
LC_REFUSED = [(8, 4, (2,)), (4, 4, (9,)), (6, 8, (2,)), (4, 4, (8, 8, 8)), (4, 4, (1, 1, 1, 1, 1))]

# (Ge, ncat1, L, Cd)
GC_CASES = [
    (8, 6, 4, 32),             # baseline
    (1, 2, 4, 32),             # smallest
    (16, 17, 4, 32),           # ep = 16: 16 categories per block, two groups; the 8-batch tail of one
    (17, 9, 4, 32),            # ep = 32: 8 categories per block, two groups; tail of one
    (32, 8, 5, 32),            # Ge at its limit, N = 320: a ragged n chunk
    (16, 33, 3, 16),           # N = 96 < 256
    (16, 377, 4, 32),          # many category groups (arch5's table)
]

WORST = {}


def record(kernel, case, err, bound):
    """err <= bound element by element; prints and keeps the worst ratio."""
    assert np.all(np.isfinite(err)), '%s %s: not finite (an element was not written?)' % (kernel, case)
    ratio = float(np.max(err / bound))
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print('%-14s %-40s worst err / bound %.4f   (worst so far %.4f)' % (kernel, case, ratio, WORST[kernel]))
    assert np.all(err <= bound), '%s %s: err / bound %.3f at %s' % (
        kernel, case, ratio, np.unravel_index(np.argmax(err / bound), err.shape))


class Out:
    """n NaN floats between two runs of G NaN canaries, one device allocation."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * G,), float('nan'), dtype=torch.float32, device=DEV)
        self.bits = self.buf.view(torch.int32).cpu().numpy().copy()

    def ptr(self):
        return self.buf.data_ptr() + 4 * G

    def read(self, what, shape=None, whole=True):
        host = self.buf.cpu()
        bits = host.view(torch.int32).numpy()
        assert np.array_equal(bits[:G], self.bits[:G]), what + ': write in front of the output'
        assert np.array_equal(bits[G + self.n:], self.bits[G + self.n:]), what + ': write behind the output'
        out = host.numpy()[G:G + self.n]
        if whole:
            assert not np.isnan(out).any(), '%s: %d elements not written' % (what, int(np.isnan(out).sum()))
        return out.reshape(shape) if shape is not None else out

    def untouched(self):
        return np.array_equal(self.buf.view(torch.int32).cpu().numpy(), self.bits)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def c_ints(v):
    return (ctypes.c_int * len(v))(*v)


def c_ptrs(v):
    return (_lib.c_fp * len(v))(*v)


def stage_shapes(Li, Lo, strides):
    """[(s, I, R)] per stage: stride, input width, input rows per frame."""
    out, R = [], 1
    for i, s in enumerate(strides):
        out.append((s, Li if i == 0 else Lo, R))
        R *= s
    return out


@functools.lru_cache(maxsize=None)
def lc_problem(Li, Lo, strides, frames, parts):
    """Inputs (f32, standard normal) of one case, shared by its tests and never modified."""
    rng = np.random.default_rng([Li, Lo, frames, parts] + list(strides))
    hop = int(np.prod(strides))
    mel = rng.standard_normal((frames, Li)).astype(np.float32)
    F = [rng.standard_normal((s, Lo, I)).astype(np.float32) for s, I, _ in stage_shapes(Li, Lo, strides)]
    stride = frames * hop * Lo + 68          # partials further apart than their size (a multiple of 4)
    dlc = rng.standard_normal((parts, stride)).astype(np.float32)
    return mel, F, dlc, stride


def stage_fwd(x, F):
    """oracle lc_upsample_fwd, one stage: x [frames][R][I], F [s][O][I] -> [frames][R·s][O]"""
    f, R, _ = x.shape
    return np.einsum('bti,joi->btjo', x, F).reshape(f, R * F.shape[0], F.shape[1])


def gpu_forward(lib, Li, Lo, strides, frames, mel, F):
    shp = stage_shapes(Li, Lo, strides)
    acts = [Out(frames * R * s * Lo) for s, _, R in shp]
    md, Fd = dev(mel), [dev(f) for f in F]
    _lib.check(lib.lbwn_lc_upsample_forward(len(strides), c_ints(strides), Li, Lo, frames, md.data_ptr(),
                                            c_ptrs([f.data_ptr() for f in Fd]), c_ptrs([a.ptr() for a in acts]), None))
    torch.cuda.synchronize()
    return acts, md, Fd


def case_name(Li, Lo, strides, frames, parts=1):
    return '%d->%d %s frames %d%s' % (Li, Lo, list(strides), frames, ' parts %d' % parts if parts > 1 else '')


def test_lc_cases_are_inside_the_envelope(lib):
    """The library's own predicate (no device): every case above is accepted, every refusal case is
    refused, the two LDS-limit shapes sit within a few floats of the 40448-float budget (one stride
    more, or the next width, is refused) and the scratch size is frames·Σ s_i·Lo·I_i."""
    def ok(Li, Lo, s):
        return lib.lbwn_lc_upsample_fused_ok(len(s), c_ints(s), Li, Lo)
    for Li, Lo, s in LC_CASES:
        assert ok(Li, Lo, s) == 1, (Li, Lo, s)
    for Li, Lo, s in LC_REFUSED:
        assert ok(Li, Lo, s) == 0, (Li, Lo, s)
    assert ok(4, 76, (2, 7, 1)) == 0 and ok(4, 200, (4,)) == 0
    assert lib.lbwn_lc_upsample_fused_ok(1, None, 4, 4) == 0
    assert lib.lbwn_lc_upsample_part_floats(2, c_ints((2, 4)), 12, 16, 3) == 3 * (2 * 16 * 12 + 4 * 16 * 16)
    assert lib.lbwn_gc_part_floats_abi(4, 8, 32) == 16 * 8 * 2 * 4 * 32
    # the second work item: 192 input rows of the trailing stride-1 stage, two per item, 11 column groups
    assert (3 * 8 * 8 + 1) // 2 * (44 // 4) == 1056 > 1024


def check_forward(name, Li, Lo, strides, frames, mel, F, outs):
    """outs[i] [frames][R_{i+1}][Lo] f32: stage i on the previous stage as given (identical inputs,
    k = I_i) and against float64 end to end."""
    x_got = mel.astype(np.float64).reshape(frames, 1, Li)
    x_ref = x_got
    x_abs = np.abs(x_got)
    k_e2e = 0
    for i, (s, I, R) in enumerate(stage_shapes(Li, Lo, strides)):
        got = np.asarray(outs[i], np.float64).reshape(frames, R * s, Lo)
        F64 = F[i].astype(np.float64)
        record('lc_up_fwd', name + ' stage %d' % i, np.abs(got - stage_fwd(x_got, F64)),
               gamma(I) * stage_fwd(np.abs(x_got), np.abs(F64)))
        x_ref, x_abs, k_e2e = stage_fwd(x_ref, F64), stage_fwd(x_abs, np.abs(F64)), k_e2e + I
        record('lc_up_fwd_e2e', name + ' stage %d' % i, np.abs(got - x_ref), gamma(k_e2e) * x_abs)
        x_got = got


def backward_ref(Li, Lo, strides, frames, F, dlc, ins, drop=None):
    """oracle lc_upsample_bwd in float64 on the stage inputs `ins` (ins[0] = mel), with the bound's
    abs-value chain and operation count beside it: [(dF_i, bound_i)] by stage.  drop: a mutant for
    the CPU proof below, never a tolerance: 'part' leaves out the last split-K partial, 'frame' the
    last frame of the frame sum, 'item2' the din rows of work items past the first 1024."""
    nup, hop, shp = len(strides), int(np.prod(strides)), stage_shapes(Li, Lo, strides)
    parts = dlc.shape[0]
    d64 = dlc.astype(np.float64)[:, :frames * hop * Lo]
    D = d64[:parts - 1 if drop == 'part' else parts].sum(axis=0).reshape(frames, hop, Lo)   # d(last stage output)
    A = np.abs(d64).sum(axis=0).reshape(frames, hop, Lo)                                    # the bound's leaves
    K, out = parts - 1, [None] * nup
    for i in reversed(range(nup)):
        s, I, R = shp[i]
        F64 = F[i].astype(np.float64)
        D4, A4 = D.reshape(frames, R, s, Lo), A.reshape(frames, R, s, Lo)
        x = np.asarray(ins[i], np.float64).reshape(frames, R, I)
        fr = frames - 1 if drop == 'frame' else frames
        out[i] = (np.einsum('btjo,bti->joi', D4[:fr], x[:fr]),
                  gamma(K + 2 * R + frames) * np.einsum('btjo,bti->joi', A4, np.abs(x)))
        D, A = np.einsum('btjo,joi->bti', D4, F64), np.einsum('btjo,joi->bti', A4, np.abs(F64))
        if drop == 'item2':      # item w = (t / 2)·(I / 4) + c / 4
            t, c = np.meshgrid(np.arange(R), np.arange(I), indexing='ij')
            D = np.where((t // 2) * (I // 4) + c // 4 >= 1024, 0.0, D)
        K += 2 * s * Lo
    return out


def check_backward(name, Li, Lo, strides, frames, F, dlc, ins, dFs):
    ref = backward_ref(Li, Lo, strides, frames, F, dlc, ins)
    for i in reversed(range(len(strides))):
        got = np.asarray(dFs[i], np.float64).reshape(ref[i][0].shape)
        record('lc_up_bwd', name + ' dF[%d]' % i, np.abs(got - ref[i][0]), ref[i][1])


def test_checks_accept_rounded_results_and_reject_wrong_ones(monkeypatch):
    """No GPU: the comparison itself.  The float64 result rounded once to f32 passes (so does it with
    half the bound added to every element: the assertion sits at the bound, not above it); results
    that are wrong the way these kernels can be wrong do not: one k-step of one output missing, a
    neighbouring stride phase, one element not written, an error of twice the bound, the last split-K
    partial or the last frame left out of the sums, and -- the reason 4->44 [3,8,8,1] is in the list --
    the din rows of the second work item per thread left at zero."""
    monkeypatch.setitem(globals(), 'WORST', {})      # the mutants' ratios stay out of the record
    Li, Lo, strides, frames = 12, 16, (2, 4), 3
    mel, F, dlc, _ = lc_problem(Li, Lo, strides, frames, 3)
    x, outs = mel.astype(np.float64).reshape(frames, 1, Li), []
    for f in F:
        x = stage_fwd(x, f.astype(np.float64)).astype(np.float32).astype(np.float64)
        outs.append(x.astype(np.float32))
    check_forward('rounded', Li, Lo, strides, frames, mel, F, outs)
    absb = stage_fwd(np.abs(outs[0].astype(np.float64)), np.abs(F[1].astype(np.float64)))

    def mutant(fn):
        m = [o.copy() for o in outs]
        fn(m)
        with pytest.raises(AssertionError):
            check_forward('mutant', Li, Lo, strides, frames, mel, F, m)

    def drop_k(m):      # the last 4-wide k-step of out[f 1][row 5][o 7]: j = 1, t = 1
        m[1][1, 5, 7] -= np.float32(outs[0][1, 1, Lo - 4:].astype(np.float64) @ F[1][1, 7, Lo - 4:].astype(np.float64))

    def phase(m):
        m[1][2, 4, :] = outs[1][2, 5, :]

    def unwritten(m):
        m[0][0, 1, 3] = np.nan

    def twice(m):
        m[1][0, 0, 0] += np.float32(2 * gamma(Lo) * absb[0, 0, 0])
    for fn in (drop_k, phase, unwritten, twice):
        mutant(fn)
    half = [outs[0], (outs[1].astype(np.float64) + 0.4 * gamma(Lo) * absb).astype(np.float32)]
    check_forward('rounded + 0.4 bound', Li, Lo, strides, frames, mel, F, half)

    ins = [mel] + outs[:-1]
    ref = backward_ref(Li, Lo, strides, frames, F, dlc, ins)
    check_backward('rounded', Li, Lo, strides, frames, F, dlc, ins, [r.astype(np.float32) for r, _ in ref])
    for drop in ('part', 'frame'):
        bad = backward_ref(Li, Lo, strides, frames, F, dlc, ins, drop=drop)
        with pytest.raises(AssertionError):
            check_backward(drop, Li, Lo, strides, frames, F, dlc, ins, [r.astype(np.float32) for r, _ in bad])
    # 'item2' changes nothing here (8 work items), and every dF below the last stage at 4->44 [3,8,8,1]
    same = backward_ref(Li, Lo, strides, frames, F, dlc, ins, drop='item2')
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(ref, same))
    Li, Lo, strides, frames = 4, 44, (3, 8, 8, 1), 1
    mel, F, dlc, _ = lc_problem(Li, Lo, strides, frames, 1)
    x, ins = mel.astype(np.float64).reshape(frames, 1, Li), [mel]
    for f in F[:-1]:
        x = stage_fwd(x, f.astype(np.float64)).astype(np.float32).astype(np.float64)
        ins.append(x)
    bad = backward_ref(Li, Lo, strides, frames, F, dlc, ins, drop='item2')
    with pytest.raises(AssertionError):
        check_backward('item2', Li, Lo, strides, frames, F, dlc, ins, [r.astype(np.float32) for r, _ in bad])


@gpu
@pytest.mark.parametrize('case,frames', [(c, f) for c, f, p in LC_RUNS if p == 1],
                         ids=lambda v: str(v).replace(' ', ''))
def test_lc_upsample_forward(lib, case, frames):
    Li, Lo, strides = case
    mel, F, _, _ = lc_problem(Li, Lo, strides, frames, 1)
    acts, _, _ = gpu_forward(lib, Li, Lo, strides, frames, mel, F)
    name = case_name(Li, Lo, strides, frames)
    check_forward(name, Li, Lo, strides, frames, mel, F,
                  [a.read('act[%d] %s' % (i, name)) for i, a in enumerate(acts)])


@gpu
@pytest.mark.parametrize('case,frames,parts', LC_RUNS, ids=lambda v: str(v).replace(' ', ''))
def test_lc_upsample_backward(lib, case, frames, parts):
    Li, Lo, strides = case
    nup = len(strides)
    mel, F, dlc, stride = lc_problem(Li, Lo, strides, frames, parts)
    acts, md, Fd = gpu_forward(lib, Li, Lo, strides, frames, mel, F)
    name = case_name(Li, Lo, strides, frames, parts)
    shp = stage_shapes(Li, Lo, strides)
    ins = [mel] + [a.read('act[%d]' % i) for i, a in enumerate(acts[:-1])]   # the kernel reads the GPU's own
    nfl = int(lib.lbwn_lc_upsample_part_floats(nup, c_ints(strides), Li, Lo, frames))
    assert nfl == frames * sum(s * Lo * I for s, I, _ in shp)
    dpart = Out(nfl)
    dF = [Out(s * Lo * I) for s, I, _ in shp]
    dd = dev(dlc)
    _lib.check(lib.lbwn_lc_upsample_backward(nup, c_ints(strides), Li, Lo, frames, md.data_ptr(),
                                             c_ptrs([f.data_ptr() for f in Fd]), c_ptrs([a.ptr() for a in acts]),
                                             dd.data_ptr(), parts, stride, dpart.ptr(),
                                             c_ptrs([o.ptr() for o in dF]), None))
    torch.cuda.synchronize()
    dpart.read('dpart ' + name)
    check_backward(name, Li, Lo, strides, frames, F, dlc, ins,
                   [o.read('dF[%d] %s' % (i, name)) for i, o in enumerate(dF)])
    for a in acts:      # the backward only reads them
        a.read('act after the backward')


@gpu
@pytest.mark.parametrize('Li,Lo,strides', LC_REFUSED, ids=lambda v: str(v).replace(' ', ''))
def test_lc_upsample_refused_outside_the_envelope(lib, Li, Lo, strides):
    """Li > Lo, stride 9, Li % 4 != 0, hop 512, five stages: both launches return EINVAL, name the
    envelope and write nothing."""
    nup, frames = len(strides), 2
    hop = int(np.prod(strides))
    w = max(Li, Lo)
    md = dev(np.ones((frames, Li + 4)))
    Fd = [dev(np.ones(s * w * w)) for s in strides]
    outs = [Out(frames * hop * w) for _ in strides] + [Out(frames * sum(strides) * w * w)] + \
           [Out(s * w * w) for s in strides]
    acts, dpart, dF = outs[:nup], outs[nup], outs[nup + 1:]
    dd = dev(np.ones(frames * hop * w))
    args = (nup, c_ints(strides), Li, Lo, frames, md.data_ptr(), c_ptrs([f.data_ptr() for f in Fd]),
            c_ptrs([a.ptr() for a in acts]))
    assert lib.lbwn_lc_upsample_forward(*args, None) == 22
    assert b'envelope' in lib.lbwn_last_error(), lib.lbwn_last_error()
    assert lib.lbwn_lc_upsample_backward(*args, dd.data_ptr(), 1, 0, dpart.ptr(), c_ptrs([o.ptr() for o in dF]),
                                         None) == 22
    assert b'envelope' in lib.lbwn_last_error(), lib.lbwn_last_error()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- GC -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gc_problem(Ge, ncat1, L, Cd):
    rng = np.random.default_rng([Ge, ncat1, L, Cd])
    emb = rng.standard_normal((ncat1, Ge)).astype(np.float32)
    W = rng.standard_normal((L, 2, Ge, Cd)).astype(np.float32)          # [l][signal | gate][e][o]
    gcd = rng.standard_normal((ncat1, L, 2, Cd)).astype(np.float32)     # column n = l·2Cd + s·Cd + o
    return emb, W, gcd


@gpu
@pytest.mark.parametrize('Ge,ncat1,L,Cd', GC_CASES)
def test_gc_table(lib, Ge, ncat1, L, Cd):
    """out[c][n] = sum_e emb[c][e]·W(n)[e]"""
    emb, W, _ = gc_problem(Ge, ncat1, L, Cd)
    N = 2 * L * Cd
    out = Out(ncat1 * N)
    ed, sd, gd = dev(emb), dev(W[:, 0]), dev(W[:, 1])
    _lib.check(lib.lbwn_gc_table(ed.data_ptr(), sd.data_ptr(), gd.data_ptr(), out.ptr(), L, ncat1, Ge, Cd, None))
    torch.cuda.synchronize()
    e64, W64 = emb.astype(np.float64), W.astype(np.float64)
    ref = np.einsum('ce,lseo->clso', e64, W64).reshape(ncat1, N)
    bound = gamma(Ge) * np.einsum('ce,lseo->clso', np.abs(e64), np.abs(W64)).reshape(ncat1, N)
    name = 'Ge %d ncat1 %d L %d Cd %d' % (Ge, ncat1, L, Cd)
    record('gc_table', name, np.abs(out.read('gctab ' + name, (ncat1, N)).astype(np.float64) - ref), bound)


@gpu
@pytest.mark.parametrize('Ge,ncat1,L,Cd', GC_CASES)
def test_gc_grads(lib, Ge, ncat1, L, Cd):
    """dW(n)[e] = sum_c emb[c][e]·gcd[c][n];  dEMB[c][e] = sum_n gcd[c][n]·W(n)[e]"""
    emb, W, gcd = gc_problem(Ge, ncat1, L, Cd)
    N = 2 * L * Cd
    part = Out(lib.lbwn_gc_part_floats_abi(L, Ge, Cd))
    demb, dsig, dgate = Out(ncat1 * Ge), Out(L * Ge * Cd), Out(L * Ge * Cd)
    ed, sd, gd, cd = dev(emb), dev(W[:, 0]), dev(W[:, 1]), dev(gcd)
    _lib.check(lib.lbwn_gc_grads(ed.data_ptr(), sd.data_ptr(), gd.data_ptr(), cd.data_ptr(), part.ptr(), demb.ptr(),
                                 dsig.ptr(), dgate.ptr(), L, ncat1, Ge, Cd, None))
    torch.cuda.synchronize()
    name = 'Ge %d ncat1 %d L %d Cd %d' % (Ge, ncat1, L, Cd)
    part.read('part ' + name, whole=False)      # scratch: the chunk partials fill only its head
    e64, W64, g64 = emb.astype(np.float64), W.astype(np.float64), gcd.astype(np.float64)
    ref = np.einsum('ce,clso->lseo', e64, g64)
    bound = gamma(ncat1) * np.einsum('ce,clso->lseo', np.abs(e64), np.abs(g64))
    for s, o in ((0, dsig), (1, dgate)):
        got = o.read('dW %s' % name, (L, Ge, Cd)).astype(np.float64)
        record('gc_wgrad', name + (' gate' if s else ' signal'), np.abs(got - ref[:, s]), bound[:, s])
    nk = (N + 255) // 256
    ref = np.einsum('clso,lseo->ce', g64, W64)
    bound = gamma(2 * 256 + nk) * np.einsum('clso,lseo->ce', np.abs(g64), np.abs(W64))
    got = demb.read('dEMB ' + name, (ncat1, Ge)).astype(np.float64)
    record('gc_egrad', name, np.abs(got - ref), bound)


@gpu
@pytest.mark.parametrize('Ge', [33, 0])
def test_gc_refused(lib, Ge):
    """n_gc_embed outside [1, 32]: EINVAL from both entries before any launch, nothing written."""
    L, ncat1, Cd = 2, 3, 32
    N = 2 * L * Cd
    src = dev(np.ones(64 * N))
    outs = [Out(ncat1 * N), Out(16 * 33 * N), Out(ncat1 * 33), Out(L * 33 * Cd), Out(L * 33 * Cd)]
    p = src.data_ptr()
    assert lib.lbwn_gc_table(p, p, p, outs[0].ptr(), L, ncat1, Ge, Cd, None) == 22
    assert b'n_gc_embed' in lib.lbwn_last_error()
    assert lib.lbwn_gc_grads(p, p, p, p, outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), outs[4].ptr(), L, ncat1, Ge, Cd,
                             None) == 22
    assert b'n_gc_embed' in lib.lbwn_last_error()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
