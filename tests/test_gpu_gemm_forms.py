"""Every kernel form and epilogue option of the step's GEMM launcher (csrc/gemm.hip
lbwn_gemm_launch), through lbwn_gemm_ex, against float64.

Each case builds A and B in float64 (magnitude ~1, B scaled by 1/sqrt(K) so the outputs are ~1
too), rounds them to f32, lays them out by a numpy restatement of the documented layout (every
padding element of a blocked layout is NaN), runs one launch, asserts the kernel instantiation the
launcher names (lbwn_gemm_last_form) and compares with epi(A32.double() @ B32.double()) at the
GEMM bar of tests/test_gpu_parity.py (close(.., 1e-5)).  C and every auxiliary output (column
partials, mask bits, the split-K slab, the step counter) sit inside guard elements that must come
back untouched, as must every element of C's buffer that is not an output (row padding, the gaps of
the chain order).  Bit-for-bit claims are those csrc/kernels.h makes.

Which form admits which option (what the cases below encode; everything else is a refusal):

  option                         x3q<8>  x3q<10>  x3q<6>  x3q<*,amn*>  x3<..>    x3<kl>  f32<..>
  bias / mask                      y       y        y       - (1)        y         y       y
  relu_a / relu_out / accumulate   y       y        y       y            y         y       y
  split_k, splits_deferred         y       y        y       y            y         y       y
  colpart (split 1)                y       y        y       - (1)        wm4 (2)   -       -
  c_chain_ls                       raw (3) raw (3)  raw (3) - (1)        y         -       -
  mbits_out / mbits                y       -        -       -            -         -       -
  row_live                         y       y        -       -            -         -       -
  k_live / nk_live / k_pre         -       -        -       <8,amn,kl>   -         y       -
  a_kstride                        y       y        y       -            akc,kfull -       -
  b_gstride                        -       -        -       -            bmn       -       -
  a_gstride                        -       -        -       not kl       -         -       -
  step_advance                     y       y        y       y            y         y       -
  xcd2d                            -       y        -       -            -         -       -
  (1) the option sends the product to an x3<..> form instead   (2) colpart selects the wm4 forms
  (3) the raw sums only: bias / relu_out / mbits* with it are refused
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lbwn import _lib
from tests.test_gpu_parity import DEV, check_plan, close, gemm_mode, small_arch  # noqa: F401  (gemm_mode: fixture)

pytestmark = pytest.mark.gpu

G = 64                         # guard elements on each side of every output buffer
SENT = -12345.0                # what outputs hold before a launch (f32)
SENT64 = 0x5A5A5A5A5A5A5A5A    # ... and the 64-bit ones
NAN = np.float32('nan')

X3Q = ['x3q<8>', 'x3q<10>', 'x3q<6>']
AMN = ['x3q<8,amn>', 'x3q<8,amn,kl>', 'x3q<6,amn>']
# the LDS-staged instantiations the dispatch reaches: x3<akc,pre,kfull,wm4> is compiled but never
# launched (that product runs on x3q<..>), and a pre-split B implies kfull
X3 = (['x3<%s,%s,%s,wm2>' % (a, b, k) for k in ('kfull', 'kany') for a in ('akc', 'amn') for b in ('bkc', 'bmn')] +
      ['x3<%s,%s,%s,wm4>' % (a, b, k) for k in ('kfull', 'kany') for a in ('akc', 'amn') for b in ('bkc', 'bmn')] +
      ['x3<akc,pre,kfull,wm2>', 'x3<amn,pre,kfull,wm2>', 'x3<amn,pre,kfull,wm4>'])
F32 = ['f32<%s,%s>' % (a, b) for a in ('akc', 'amn') for b in ('bkc', 'bmn')]
DISPATCHER_FORMS = set(X3Q + AMN + X3 + ['x3<kl>'] + F32)


# ---- problems (shared, never modified) and the float64 reference ------------------------------

@functools.lru_cache(maxsize=None)
def problem(M, N, K, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    P = SimpleNamespace(M=M, N=N, K=K)
    P.A = torch.randn(M, K, generator=g, dtype=torch.float64).float().numpy()
    P.B = (torch.randn(K, N, generator=g, dtype=torch.float64) / K ** 0.5).float().numpy()
    P.bias = torch.randn(N, generator=g, dtype=torch.float64).float().numpy()
    P.mask = (torch.rand(M, N, generator=g) > 0.3).float().numpy()
    P.C0 = torch.randn(M, N, generator=g, dtype=torch.float64).float().numpy()
    P.prod = {}
    return P


def derive(P, M=None, a_zero_rows=None, b_zero_rows=None):
    """P's first M rows, or P with rows of A / B set to exact zeros."""
    M = M or P.M
    Q = SimpleNamespace(M=M, N=P.N, K=P.K, A=P.A[:M].copy(), B=P.B.copy(), bias=P.bias, mask=P.mask[:M],
                        C0=P.C0[:M], prod={})
    if a_zero_rows is not None:
        Q.A[a_zero_rows] = 0.0
    if b_zero_rows is not None:
        Q.B[b_zero_rows] = 0.0
    return Q


def ref(P, bias=0, mask=0, relu_a=0, relu_out=0, acc=0, mask_arr=None, **_):
    if relu_a not in P.prod:
        A = P.A.astype(np.float64)
        P.prod[relu_a] = (np.maximum(A, 0.0) if relu_a else A) @ P.B.astype(np.float64)
    R = P.prod[relu_a]
    if bias:
        R = R + P.bias.astype(np.float64)
    if relu_out:
        R = np.maximum(R, 0.0)
    if mask_arr is not None:
        R = R * (mask_arr > 0)
    elif mask:
        R = R * (P.mask > 0)
    if acc:
        R = R + P.C0.astype(np.float64)
    return R


# ---- buffers ------------------------------------------------------------------------------------

class Guarded:
    """n payload elements between two runs of G sentinel elements, on the device."""

    def __init__(self, n, dtype=np.float32, init=None):
        self.n, self.sent = n, (SENT if dtype == np.float32 else SENT64)
        host = np.full(n + 2 * G, self.sent, dtype)
        if init is not None:
            host[G:G + n] = init
        self.initial = host[G:G + n].copy()
        self.dev = torch.from_numpy(host).to(DEV)

    def ptr(self):
        return self.dev.data_ptr() + G * self.dev.element_size()

    def read(self, what):
        host = self.dev.cpu().numpy()
        assert (host[:G] == self.sent).all() and (host[G + self.n:] == self.sent).all(), what + ': guard overwritten'
        return host[G:G + self.n]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def chain_index(M, N, ls):
    """csrc/kernels.h c_chain_ls: 32-column block j at j·ls, element (m, c) of it at sg_off's order."""
    m, c = np.meshgrid(np.arange(M), np.arange(N), indexing='ij')
    return (c >> 5) * ls + ((((m >> 5) * 4 + ((c >> 3) & 3)) * 32 + (m & 31)) * 8 + (c & 7))


def chain_min(M):
    return (M + 31) // 32 * 32 * 32


def x3_splits(K, split, bk=32):
    kps = -(-K // max(split, 1))
    kps = -(-kps // bk) * bk
    return -(-K // kps)


# ---- one launch ---------------------------------------------------------------------------------

def launch(lib, P, akc=1, bkc=0, pre=0, split=1, bias=0, mask=0, relu_a=0, relu_out=0, acc=0, ldc=None, cp=0,
           chain=0, xcd2d=0, a_kstride=0, b_gstride=0, a_gstride=0, rx=0, mbits_out=0, mbits=None, mask_arr=None,
           row_live=None, kl=None, kl_partial=False, deferred=0, step=None, no_slab=False, refused=False, **_):
    """Run lbwn_gemm_ex on P with the options given and return what it wrote; every guard and every
    non-output element of C's buffer is checked here.  refused: the call must return 22 with a
    message and leave every output as it was."""
    M, N, K = P.M, P.N, P.K
    m, k = np.meshgrid(np.arange(M), np.arange(K), indexing='ij')
    if a_kstride:      # A[m·32 + (k/32)·a_kstride + k%32]
        Ah = np.full((-(-K // 32)) * a_kstride, NAN, np.float32)
        Ah[m * 32 + (k // 32) * a_kstride + k % 32] = P.A
        lda = 32
    elif a_gstride:    # A[k·32 + (m/32)·a_gstride + m%32]
        Ah = np.full((-(-M // 32)) * a_gstride, NAN, np.float32)
        Ah[k * 32 + (m // 32) * a_gstride + m % 32] = P.A
        lda = 32
    else:
        Ah, lda = (P.A, K) if akc else (P.A.T, M)
    kk, n = np.meshgrid(np.arange(K), np.arange(N), indexing='ij')
    if b_gstride:      # B[k·32 + (n/32)·b_gstride + n%32]
        Bh = np.full((-(-N // 32)) * b_gstride, NAN, np.float32)
        Bh[kk * 32 + (n // 32) * b_gstride + n % 32] = P.B
        ldb = 32
    else:
        Bh, ldb = (P.B.T, K) if bkc else (P.B, N)
    Ad, Bd = dev(Ah), dev(Bh)
    keep = [Ad, Bd]
    a = _lib.GemmExArgs(A=Ad.data_ptr(), B=Bd.data_ptr(), lda=lda, ldb=ldb, M=M, N=N, K=K, a_kcontig=akc, b_kcontig=bkc,
                        split_k=split, relu_a=relu_a, relu_out=relu_out, accumulate=acc, xcd2d=xcd2d, c_chain_ls=chain,
                        a_kstride=a_kstride, b_gstride=b_gstride, a_gstride=a_gstride, row_exact=rx)
    if pre:
        b3 = torch.empty(int(lib.lbwn_split_planes_elems_abi(N, K)), dtype=torch.int16, device=DEV)
        _lib.check(lib.lbwn_split_planes(Bd.data_ptr(), ldb, N, K, 0 if bkc else 1, b3.data_ptr(), None))
        a.b3 = b3.data_ptr()
        keep.append(b3)
    # C: rows of ldc, or the chain order; C0 where it accumulates
    ldc = ldc or N
    mm, cc = np.meshgrid(np.arange(M), np.arange(N), indexing='ij')
    cidx = chain_index(M, N, chain) if chain else mm * ldc + cc
    csize = (N // 32) * chain if chain else M * ldc
    c0 = np.full(csize, SENT, np.float32)
    if acc:
        c0[cidx] = P.C0
    Cg = Guarded(csize, init=c0)
    a.C, a.ldc = Cg.ptr(), ldc
    if bias:
        keep.append(dev(P.bias))
        a.bias = keep[-1].data_ptr()
    if mask or mask_arr is not None:
        keep.append(dev(P.mask if mask_arr is None else mask_arr.astype(np.float32)))
        a.mask, a.ldm = keep[-1].data_ptr(), N
    out = {}
    if cp:
        out['colpart'] = Guarded(int(lib.lbwn_colpart_parts_abi(M)) * N)
        a.colpart = out['colpart'].ptr()
    if mbits_out:
        out['mbits'] = Guarded(int(lib.lbwn_gemm_mbits_words_abi(M, N)), np.int64)
        a.mbits_out = out['mbits'].ptr()
    if mbits is not None:
        keep.append(dev(mbits))
        a.mbits = keep[-1].data_ptr()
    if (split > 1 or deferred) and not no_slab:
        out['slab'] = Guarded(max(split, 1) * M * N)
        a.slab_ws = out['slab'].ptr()
    if step is not None:
        a.step_advance = step.ptr()
    if row_live is not None:
        keep.append(dev(np.asarray(row_live, np.int32)))
        a.row_live = keep[-1].data_ptr()
    if kl is not None:   # kernels.h: the ascending live k-steps, their count, and the prefix counts [K/32 + 1]
        nks = K // 32
        lst = np.zeros(max(nks, 1), np.int32)
        lst[:len(kl)] = kl
        pre_cnt = np.array([sum(1 for e in kl if e < i) for i in range(nks + 1)], np.int32)
        keep += [dev(lst), dev(np.array([len(kl)], np.int32)), dev(pre_cnt)]
        a.k_live, a.nk_live = keep[-3].data_ptr(), keep[-2].data_ptr()
        if not kl_partial:
            a.k_pre = keep[-1].data_ptr()
    nsplit = ctypes.c_int(-7)
    if deferred:
        a.splits_deferred = ctypes.pointer(nsplit)
    rc = lib.lbwn_gemm_ex(ctypes.byref(a), None)
    torch.cuda.synchronize()
    r = SimpleNamespace(rc=rc, err=lib.lbwn_last_error().decode() if rc else '', form=lib.lbwn_gemm_last_form().decode(),
                        splits=nsplit.value)
    craw = Cg.read('C')
    res = {kname: g.read(kname) for kname, g in out.items()}
    if refused:
        assert rc == 22 and r.err and r.form == '', (rc, r.err, r.form)
        assert np.array_equal(craw, Cg.initial), 'a refused launch wrote C'
        for kname, g in out.items():
            assert np.array_equal(res[kname], g.initial), 'a refused launch wrote ' + kname
        assert nsplit.value == -7
        return r
    assert rc == 0, r.err
    if deferred and r.splits > 1:
        assert np.array_equal(craw, Cg.initial), 'deferred split-K wrote C'
    else:
        other = np.ones(csize, bool)
        other[cidx] = False
        assert (craw[other] == np.float32(SENT)).all(), 'C buffer written outside the outputs'
        r.C = craw[cidx]
    r.__dict__.update(res)
    return r


def check_colpart(lib, r, M, N):
    """Only the summation is measured: the float64 column sums of the GPU's own C per 256-row
    block, sequential-sum bound 255·2^-24·Σ|C| per column; then lbwn_colsum_final's order on the
    host (csrc/reduce.hip colsum_final_kernel: 16 lanes take every 16th part in order, then the lane
    sums in order) against C's whole column sum."""
    parts = r.colpart.reshape(-1, N)
    assert parts.shape[0] == (M + 255) // 256 == lib.lbwn_colpart_parts_abi(M)
    C = r.C.astype(np.float64)
    for p in range(parts.shape[0]):
        blk = C[256 * p:256 * (p + 1)]
        err, bound = np.abs(parts[p] - blk.sum(0)), 255 * 2.0 ** -24 * np.abs(blk).sum(0)
        assert (err <= bound).all(), 'colpart block %d: %.3g over the bound' % (p, float((err - bound).max()))
    lanes = np.zeros((16, N), np.float32)
    for p in range(parts.shape[0]):
        lanes[p % 16] += parts[p]
    tot = np.zeros(N, np.float32)
    for ln in range(16):
        tot += lanes[ln]
    bound = (255 + parts.shape[0] + 15) * 2.0 ** -24 * np.abs(C).sum(0)
    assert (np.abs(tot - C.sum(0)) <= bound).all(), 'colsum_final of the parts'


# ---- the form matrix ------------------------------------------------------------------------------

def case(form, M, N, K, akc, bkc, **kw):
    return dict(form=form, M=M, N=N, K=K, akc=akc, bkc=bkc, **kw)


ALL8 = list(range(8))
TABLE = [
    # A in registers, pre-split B: 256-row tiles below M = 8192 through row_exact or colpart
    case('x3q<8>', 520, 136, 96, 1, 0, pre=1, rx=1),
    case('x3q<8>', 520, 200, 64, 1, 1, pre=1, rx=1),
    case('x3q<8>', 520, 136, 96, 1, 0, pre=1, cp=1),
    case('x3q<8>', 520, 200, 96, 1, 1, pre=1, rx=1, split=3),
    case('x3q<8>', 8200, 136, 96, 1, 0, pre=1),
    case('x3q<10>', 520, 640, 64, 1, 1, pre=1, rx=1),
    case('x3q<10>', 1000, 640, 64, 1, 1, pre=1, rx=1, xcd2d=1),     # 4 x 4 tiles: xcd2d_tile's own walk
    case('x3q<10>', 520, 640, 64, 1, 0, pre=1, cp=1, xcd2d=1),      # 3 x 4 tiles: its fall-back
    case('x3q<10>', 8200, 640, 64, 1, 1, pre=1),
    case('x3q<6>', 520, 80, 96, 1, 1, pre=1, rx=1),
    case('x3q<6>', 520, 96, 64, 1, 0, pre=1, rx=1),
    case('x3q<6>', 520, 80, 96, 1, 1, pre=1, cp=1),
    case('x3q<6>', 8200, 80, 64, 1, 1, pre=1),
    # the weight-gradient forms (both operands mn-contiguous, >= 8 tiles of 256 x 128)
    case('x3q<8,amn>', 1028, 200, 96, 0, 0),
    case('x3q<8,amn>', 1028, 200, 96, 0, 0, split=3),
    case('x3q<8,amn,kl>', 1028, 200, 256, 0, 0, kl=ALL8),
    case('x3q<8,amn,kl>', 1028, 200, 256, 0, 0, kl=ALL8, split=3),
    case('x3q<6,amn>', 1800, 80, 64, 0, 0),
    case('x3q<6,amn>', 1800, 96, 64, 0, 0, split=2),
    case('x3q<6,amn>', 1800, 80, 64, 0, 0, a_gstride=64 * 32 + 64),
    case('x3<kl>', 260, 136, 256, 0, 0, kl=ALL8),
    case('x3<kl>', 260, 136, 256, 0, 0, kl=ALL8, split=3),
    # LDS-staged, 128-row tiles
    case('x3<akc,pre,kfull,wm2>', 520, 136, 96, 1, 0, pre=1),
    case('x3<amn,pre,kfull,wm2>', 520, 136, 96, 0, 1, pre=1),
    case('x3<akc,bkc,kfull,wm2>', 520, 136, 96, 1, 1),
    case('x3<akc,bmn,kfull,wm2>', 520, 200, 64, 1, 0, split=2),
    case('x3<amn,bkc,kfull,wm2>', 520, 136, 96, 0, 1),
    case('x3<amn,bmn,kfull,wm2>', 520, 136, 96, 0, 0),
    case('x3<akc,bkc,kany,wm2>', 520, 136, 100, 1, 1),
    case('x3<akc,bmn,kany,wm2>', 520, 200, 200, 1, 0),
    case('x3<amn,bkc,kany,wm2>', 520, 136, 100, 0, 1, split=3),
    case('x3<amn,bmn,kany,wm2>', 520, 200, 100, 0, 0),
    # LDS-staged, 256-row tiles: row_exact (k-contiguous A) or colpart
    case('x3<akc,bkc,kfull,wm4>', 520, 136, 96, 1, 1, rx=1),
    case('x3<akc,bmn,kfull,wm4>', 520, 200, 64, 1, 0, rx=1, cp=1),
    case('x3<akc,bmn,kfull,wm4>', 8200, 136, 64, 1, 0),
    case('x3<akc,bkc,kfull,wm4>', 520, 200, 64, 1, 1, cp=1),
    case('x3<akc,bkc,kany,wm4>', 520, 136, 100, 1, 1, cp=1),
    case('x3<akc,bkc,kany,wm4>', 8200, 136, 100, 1, 1),
    case('x3<akc,bmn,kany,wm4>', 520, 136, 100, 1, 0, cp=1),
    case('x3<akc,bmn,kany,wm4>', 520, 200, 200, 1, 0, rx=1, split=3),
    case('x3<amn,pre,kfull,wm4>', 520, 136, 96, 0, 0, pre=1, cp=1),
    case('x3<amn,bkc,kfull,wm4>', 520, 136, 96, 0, 1, cp=1),
    case('x3<amn,bmn,kfull,wm4>', 520, 200, 64, 0, 0, cp=1),
    case('x3<amn,bkc,kany,wm4>', 520, 200, 100, 0, 1, cp=1),
    case('x3<amn,bmn,kany,wm4>', 520, 136, 100, 0, 0, cp=1),
    # mode 0
    case('f32<akc,bkc>', 520, 136, 100, 1, 1, mode=0),
    case('f32<akc,bmn>', 520, 200, 96, 1, 0, mode=0, split=3),
    case('f32<amn,bkc>', 520, 136, 100, 0, 1, mode=0),
    case('f32<amn,bmn>', 1028, 200, 96, 0, 0, mode=0),
]


def case_id(c):
    return '%s-%dx%dx%d%s' % (c['form'], c['M'], c['N'], c['K'], ''.join(
        '-%s%s' % (k, '' if v in (1, True) or isinstance(v, list) else v) for k, v in c.items()
        if k not in ('form', 'M', 'N', 'K', 'akc', 'bkc') and v))


def by_form(*forms, **need):
    return [c for c in TABLE if c['form'] in forms and all(c.get(k, 0) == v for k, v in need.items())]


SEEN = []   # (case id, what lbwn_gemm_last_form said) of every test_form case that ran


def test_table_covers_every_form():
    """A form the dispatcher has (DISPATCHER_FORMS, from gemm_launch_x3 / gemm_launch_t) without a
    case here fails; test_form asserts that each case runs the form it names, and
    test_forms_seen (last in the file) checks the names the launcher really reported."""
    assert {c['form'] for c in TABLE} == DISPATCHER_FORMS


@pytest.mark.parametrize('c', TABLE, ids=case_id)
def test_form(lib, gemm_mode, c):
    """The plain product, then every elementwise option the form admits, together (the float64
    expression of test_gemm_layouts): without accumulate at ldc = N (the x3q forms' 16-byte
    epilogue), with accumulate and at ldc % 4 != 0 (their scalar one).  Column partials wherever
    the case has them.  The shape queries must say what the launcher then did."""
    gemm_mode(c.get('mode', 1))
    P = problem(c['M'], c['N'], c['K'])
    M, N, K, form = c['M'], c['N'], c['K'], c['form']
    q = [lib.lbwn_gemm_form_query(w, M, N, K, c['akc'], c.get('pre', 0), c.get('rx', 0), c.get('cp', 0)) for w in (0, 1, 2)]
    assert q[0] == int(form == 'x3q<8>') and q[1] == int(form in ('x3q<8>', 'x3q<10>')), q
    if form.startswith('f32'):
        assert q[2] == 0
    elif not c['akc'] and not c['bkc'] and not c.get('pre') and not c.get('cp'):
        assert q[2] == int(form in ('x3q<8,amn>', 'x3q<8,amn,kl>', 'x3<kl>', 'x3<amn,bmn,kfull,wm2>')), q
    amn = form in AMN
    epis = [dict()]
    full = dict(relu_a=1, relu_out=1) if amn else dict(bias=1, mask=1, relu_a=1, relu_out=1)
    if form in X3Q + AMN:
        epis += [full, dict(full, acc=1), dict(full, ldc=N + 1)]
    else:
        epis += [dict(full, acc=1, ldc=N + 4)]
    for epi in epis:
        r = launch(lib, P, **dict(c, **epi))
        if not epi:
            SEEN.append((case_id(c), r.form))
        assert r.form == form, (r.form, epi)
        close(r.C, ref(P, **epi), 1e-5, '%s %s' % (form, epi))
        if c.get('cp'):
            check_colpart(lib, r, M, N)
        if c.get('split', 1) > 1:   # the slab past the slices the launcher formed stays untouched
            used = x3_splits(K, c['split'], 16 if form.startswith('f32') else 32) * M * N
            assert (r.slab[used:] == np.float32(SENT)).all()


# ---- options ------------------------------------------------------------------------------------

CHAIN = [case('x3q<10>', 520, 640, 64, 1, 1, pre=1, rx=1, xcd2d=1), case('x3q<8>', 520, 160, 96, 1, 0, pre=1, rx=1),
         case('x3q<8>', 520, 160, 96, 1, 0, pre=1, cp=1), case('x3q<6>', 520, 96, 64, 1, 1, pre=1, rx=1),
         case('x3<akc,pre,kfull,wm2>', 520, 160, 96, 1, 1, pre=1),      # the form dZ takes below M = 8192
         case('x3<akc,bmn,kany,wm4>', 520, 160, 100, 1, 0, cp=1)]


@pytest.mark.parametrize('c', CHAIN, ids=case_id)
def test_chain_order(lib, c):
    """C in the backward chain's order (c_chain_ls at its minimum, M % 32 != 0): the values of the
    row-major run bit for bit, at sg_off's places, nothing else written.  The LDS-staged forms
    apply bias / relu there; the x3q forms store the raw sums, so the launcher refuses those
    options on them (it used to accept them and drop them silently)."""
    P = problem(c['M'], c['N'], c['K'])
    ls = chain_min(P.M)
    rows = launch(lib, P, **c)
    r = launch(lib, P, chain=ls, **c)
    assert r.form == rows.form == c['form']
    assert np.array_equal(r.C, rows.C)
    close(r.C, ref(P), 1e-5, 'chain order')
    if c.get('cp'):
        check_colpart(lib, r, P.M, P.N)
    opts = [dict(bias=1, relu_out=1, relu_a=1), dict(bias=1), dict(relu_out=1)]
    if c['form'] in X3Q:
        for o in opts + ([dict(mbits_out=1)] if c['form'] == 'x3q<8>' else []):
            assert 'chain-order' in launch(lib, P, chain=ls, refused=True, **dict(c, **o)).err
    else:
        for o in opts:
            r = launch(lib, P, chain=ls + 1024, **dict(c, **o))
            assert r.form == c['form']
            close(r.C, ref(P, **o), 1e-5, 'chain order %s' % o)


def mbits_decode(words, M, N):
    """kernels.h mbits: [tile][wave][lane] words, bit 8·nb + e = element (e, nb) of the lane's
    epilogue = row m0 + 32·wave + 16·(e/4) + 4·(lane/16) + e%4, column n0 + 16·nb + lane%16."""
    tn = (N + 127) // 128
    w = words.view(np.uint64).reshape(-1, 8, 64)
    t, wave, lane, nb, e = np.indices((w.shape[0], 8, 64, 8, 8))
    row = (t // tn) * 256 + 32 * wave + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3)
    col = (t % tn) * 128 + 16 * nb + (lane & 15)
    bit = (w[t, wave, lane] >> (8 * nb + e).astype(np.uint64)) & np.uint64(1)
    ok = (row < M) & (col < N)
    out = np.zeros((M, N), bool)
    out[row[ok], col[ok]] = bit[ok] != 0
    return out


@pytest.mark.parametrize('N,K', [(136, 96), (200, 64)])
def test_mask_bits(lib, N, K):
    """mbits_out -> mbits on x3q<8> at ragged M and N: the producer's bits are (C1 > 0) at the
    documented places; a consumer of the same shape masked by them equals, bit for bit, the one
    masked by the f32 mask (C1 > 0), and float64 within the bar."""
    M = 520
    c = dict(akc=1, bkc=0, pre=1, rx=1)
    P1, P2 = problem(M, N, K), problem(M, N, K, seed=1)
    r1 = launch(lib, P1, bias=1, relu_out=1, mbits_out=1, **c)
    assert r1.form == 'x3q<8>' and r1.mbits.size == lib.lbwn_gemm_mbits_words_abi(M, N)
    close(r1.C, ref(P1, bias=1, relu_out=1), 1e-5, 'producer')
    assert np.array_equal(mbits_decode(r1.mbits, M, N), r1.C > 0)
    epi = dict(bias=1, relu_a=1, relu_out=1)
    rb = launch(lib, P2, mbits=r1.mbits, **c, **epi)
    rm = launch(lib, P2, mask_arr=(r1.C > 0), **c, **epi)
    assert rb.form == rm.form == 'x3q<8>'
    assert np.array_equal(rb.C, rm.C)
    close(rb.C, ref(P2, mask_arr=(r1.C > 0), **epi), 1e-5, 'consumer')
    # a consumer that is also a producer, through the scalar epilogue (accumulate)
    rb2 = launch(lib, P2, mbits=r1.mbits, mbits_out=1, acc=1, **c, **epi)
    close(rb2.C, ref(P2, mask_arr=(r1.C > 0), acc=1, **epi), 1e-5, 'consumer + accumulate')
    assert np.array_equal(mbits_decode(rb2.mbits, M, N), rb.C > 0)


@pytest.mark.parametrize('c', by_form('x3q<8>', 'x3q<10>', M=520, split=0), ids=case_id)
@pytest.mark.parametrize('live', [(1, 1, 1), (0, 0, 0), (1, 1, 0), (0, 0, 1)])
def test_row_live(lib, c, live):
    """A dead 256-row tile (every A row exactly zero) runs no k-step: the result equals the run
    without the list bit for bit, and the dead rows hold epi(0) = relu(bias), not zero."""
    P0 = problem(c['M'], c['N'], c['K'])
    dead = np.repeat(np.array(live) == 0, 256)[:P0.M]
    P = derive(P0, a_zero_rows=dead)
    epi = dict(bias=1, relu_out=1)
    r0 = launch(lib, P, **c, **epi)
    r1 = launch(lib, P, row_live=live, **c, **epi)
    assert r0.form == r1.form == c['form']
    assert np.array_equal(r0.C, r1.C)
    close(r1.C, ref(P, **epi), 1e-5, 'row_live')
    assert np.array_equal(r1.C[dead], np.broadcast_to(np.maximum(P.bias, 0), (int(dead.sum()), P.N)))
    if c.get('cp'):
        check_colpart(lib, r1, P.M, P.N)


@pytest.mark.parametrize('c', by_form('x3q<8,amn,kl>', 'x3<kl>'), ids=case_id)
@pytest.mark.parametrize('kl', [[], [5], ALL8, [0, 1, 5, 6, 7]])
def test_k_live(lib, c, kl):
    """B rows exactly zero in the dead k-steps; the lists as kernels.h defines them.  K = 256 is 8
    k-steps; split 3 makes slices of 3, 3 and 2, so the dead run 2..4 straddles a slice boundary
    and the one-entry list leaves two slices empty.  Bit for bit the run without the lists."""
    P0 = problem(c['M'], c['N'], c['K'])
    dead = np.repeat(~np.isin(np.arange(8), kl), 32)
    P = derive(P0, b_zero_rows=dead)
    base = dict(c, kl=None)
    for epi in (dict(), dict(relu_a=1, relu_out=1, acc=1)):
        r0 = launch(lib, P, **dict(base, **epi))
        r1 = launch(lib, P, **dict(c, kl=kl, **epi))
        assert r1.form == c['form'] and r0.form == {'x3q<8,amn,kl>': 'x3q<8,amn>', 'x3<kl>': 'x3<amn,bmn,kfull,wm2>'}[c['form']]
        assert np.array_equal(r0.C, r1.C)
        close(r1.C, ref(P, **epi), 1e-5, 'k_live')
    if c['form'] == 'x3<kl>':   # bias / mask keep the product on the 128-row form
        epi = dict(bias=1, mask=1, relu_out=1)
        r1 = launch(lib, P, **dict(c, kl=kl, **epi))
        assert r1.form == 'x3<kl>'
        assert np.array_equal(r1.C, launch(lib, P, **dict(base, **epi)).C)
        close(r1.C, ref(P, **epi), 1e-5, 'k_live + bias')


KSTRIDE = (by_form('x3q<8>', 'x3q<10>', 'x3q<6>', M=520, rx=1) +
           by_form('x3<akc,pre,kfull,wm2>', 'x3<akc,bkc,kfull,wm2>', 'x3<akc,bmn,kfull,wm2>', 'x3<akc,bkc,kfull,wm4>',
                   'x3<akc,bmn,kfull,wm4>', M=520))
GSTRIDE_B = by_form('x3<akc,bmn,kfull,wm2>', 'x3<amn,bmn,kfull,wm2>', 'x3<akc,bmn,kany,wm2>', 'x3<amn,bmn,kany,wm2>',
                    'x3<akc,bmn,kfull,wm4>', 'x3<akc,bmn,kany,wm4>', 'x3<amn,bmn,kfull,wm4>', 'x3<amn,bmn,kany,wm4>', M=520)
GSTRIDE_A = by_form('x3q<8,amn>', 'x3q<6,amn>', a_gstride=0)


@pytest.mark.parametrize('c,opt', [(c, 'a_kstride') for c in KSTRIDE] + [(c, 'b_gstride') for c in GSTRIDE_B] +
                         [(c, 'a_gstride') for c in GSTRIDE_A], ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_blocked_operands(lib, c, opt):
    """The k-blocked layouts of kernels.h (the backward chain's DV export) at M / N that are no
    whole number of 32-groups and a stride above the minimum: the same form and, bit for bit, the
    product from the plain layout."""
    P = problem(c['M'], c['N'], c['K'])
    stride = {'a_kstride': P.M * 32 + 96, 'b_gstride': P.K * 32 + 64, 'a_gstride': P.K * 32 + 32}[opt]
    epi = dict(relu_a=1, relu_out=1) if opt == 'a_gstride' else dict(bias=1, relu_a=1, relu_out=1, mask=1)
    r0 = launch(lib, P, **c, **epi)
    r1 = launch(lib, P, **{opt: stride}, **c, **epi)
    assert r0.form == r1.form == c['form']
    assert np.array_equal(r0.C, r1.C)
    close(r1.C, ref(P, **epi), 1e-5, opt)


DEFER = [(case('x3q<8,amn>', 1028, 200, 96, 0, 0), 3, 3), (case('x3q<8,amn>', 1028, 200, 96, 0, 0), 4, 3),
         (case('x3q<8>', 520, 136, 96, 1, 0, pre=1, rx=1), 2, 2), (case('x3q<6>', 520, 80, 96, 1, 1, pre=1, rx=1), 4, 3),
         (case('x3<akc,bkc,kfull,wm2>', 520, 136, 96, 1, 1), 4, 3), (case('x3<amn,bmn,kany,wm2>', 520, 200, 100, 0, 0), 5, 4),
         (case('x3<akc,bkc,kfull,wm2>', 520, 136, 96, 1, 1), 1, 1), (case('f32<akc,bmn>', 520, 200, 96, 1, 0, mode=0), 4, 3)]


@pytest.mark.parametrize('c,split,want', DEFER, ids=lambda v: str(v) if isinstance(v, int) else case_id(v))
def test_splits_deferred(lib, gemm_mode, c, split, want):
    """The partials stay unsummed in the [splits][M][N] slab, C is untouched, and the count the
    launcher really formed comes back (K = 96 asked for 4 slices makes 3 of one k-step each; 1: C
    was written as usual).  The float64 sum of the partials is the product."""
    gemm_mode(c.get('mode', 1))
    P = problem(c['M'], c['N'], c['K'])
    r = launch(lib, P, deferred=1, **dict(c, split=split))
    assert r.form == c['form'] and r.splits == want
    if want == 1:
        close(r.C, ref(P), 1e-5, 'deferred, one slice')
        assert (r.slab == np.float32(SENT)).all()
        return
    n = P.M * P.N
    assert (r.slab[want * n:] == np.float32(SENT)).all()
    close(r.slab[:want * n].reshape(want, P.M, P.N).astype(np.float64).sum(0), ref(P), 1e-5, 'sum of the partials')


STEP = [c for f in ('x3q<8>', 'x3q<10>', 'x3q<6>', 'x3q<8,amn>', 'x3q<6,amn>', 'x3q<8,amn,kl>', 'x3<kl>', 'x3<akc,bmn,kfull,wm2>',
                    'x3<amn,bkc,kany,wm2>', 'x3<akc,bkc,kfull,wm4>', 'x3<amn,bmn,kany,wm4>') for c in by_form(f)[:1]]


@pytest.mark.parametrize('c', STEP, ids=case_id)
def test_step_advance(lib, c):
    """+1 per launch (split-K launches included: one block of the whole grid counts)."""
    P = problem(c['M'], c['N'], c['K'])
    step = Guarded(1, np.int64, init=41)
    for want in (42, 43):
        r = launch(lib, P, step=step, **c)
        assert r.form == c['form']
        assert int(step.read('step counter')[0]) == want


def test_xcd2d_is_placement_only(lib):
    """x3q<10>'s 2-D XCD walk of the tiles (4 x 4 tiles: the walk itself, not its fall-back)
    changes which block computes a tile, never a value."""
    c = by_form('x3q<10>', M=1000)[0]
    P = problem(c['M'], c['N'], c['K'])
    epi = dict(bias=1, relu_out=1, mask=1)
    r0 = launch(lib, P, **dict(c, xcd2d=0, **epi))
    r1 = launch(lib, P, **c, **epi)
    assert r0.form == r1.form == 'x3q<10>' and np.array_equal(r0.C, r1.C)


@pytest.mark.parametrize('c', by_form(*(X3Q + X3), M=8200), ids=case_id)
def test_row_exact(lib, c):
    """row_exact below M = 8192 picks the form M >= 8192 gets, and a row's value depends on its own
    A row only: the 520 rows of the short run equal those rows of the M = 8200 run bit for bit
    (what the staged-slice tests rest on)."""
    big = problem(8200, c['N'], c['K'])
    small = derive(big, M=520)
    epi = dict(bias=1, relu_a=1, relu_out=1, mask=1)
    rb = launch(lib, big, **c, **epi)
    rs = launch(lib, small, rx=1, **c, **epi)
    assert rb.form == rs.form == c['form']
    assert np.array_equal(rb.C[:520], rs.C)
    close(rs.C, ref(small, **epi), 1e-5, 'row_exact')


# ---- refusals -----------------------------------------------------------------------------------

Q8 = dict(akc=1, bkc=0, pre=1, rx=1)          # x3q<8> at (520, 136, 96)
WG = dict(akc=0, bkc=0)                       # x3q<8,amn> at (1028, 200, 96)
REFUSED = [
    # (M, N, K), options, mode, a word of the message
    ((520, 640, 64), dict(Q8, mbits_out=1), 1, 'mask bits'),              # x3q<10>
    ((520, 80, 96), dict(Q8, mbits_out=1), 1, 'mask bits'),               # x3q<6>
    ((520, 136, 96), dict(Q8, rx=0, mbits_out=1), 1, 'mask bits'),        # 128-row tiles
    ((520, 136, 96), dict(Q8, pre=0, mbits_out=1), 1, 'mask bits'),       # no pre-split B
    ((520, 136, 96), dict(Q8, split=3, mbits_out=1), 1, 'mask bits'),
    ((520, 136, 96), dict(Q8, split=3, row_live=(1, 1, 1)), 1, 'row_live'),
    ((520, 136, 96), dict(Q8, akc=0, cp=1, row_live=(1, 1, 1)), 1, 'row_live'),
    ((520, 80, 96), dict(Q8, row_live=(1, 1, 1)), 1, 'row_live'),
    ((520, 136, 96), dict(Q8, rx=0, row_live=(1, 1, 1)), 1, 'row_live'),
    ((1028, 200, 96), dict(WG, pre=1, kl=[0, 1, 2]), 1, 'k_live'),
    ((1028, 200, 96), dict(WG, akc=1, kl=[0, 1, 2]), 1, 'k_live'),
    ((1028, 200, 96), dict(WG, bkc=1, kl=[0, 1, 2]), 1, 'k_live'),
    ((1028, 200, 96), dict(WG, cp=1, kl=[0, 1, 2]), 1, 'k_live'),
    ((1028, 200, 96), dict(WG, kl=[0, 1, 2], kl_partial=True), 1, 'k_live'),
    ((1028, 200, 100), dict(WG, kl=[0, 1, 2]), 1, 'k_live'),
    ((1800, 80, 64), dict(WG, kl=[0, 1]), 1, 'k_live'),                    # the 96-column AMN form
    ((1800, 80, 64), dict(WG, a_gstride=2048, bias=1), 1, 'mn-blocked A'),
    ((1800, 80, 64), dict(WG, a_gstride=2048, mask=1), 1, 'mn-blocked A'),
    ((1800, 80, 64), dict(WG, a_gstride=2048, cp=1), 1, 'mn-blocked A'),
    ((1800, 80, 64), dict(WG, a_gstride=2048, pre=1), 1, 'mn-blocked A'),
    ((1800, 80, 64), dict(WG, a_gstride=2048, bkc=1), 1, 'mn-blocked A'),
    ((252, 80, 64), dict(WG, a_gstride=2048), 1, 'mn-blocked A'),
    ((520, 136, 96), dict(Q8, akc=0, a_kstride=520 * 32), 1, 'k-blocked A'),
    ((520, 136, 100), dict(akc=1, bkc=1, a_kstride=520 * 32), 1, 'k-blocked A'),
    ((520, 136, 96), dict(akc=1, bkc=1, b_gstride=96 * 32), 1, 'mn-blocked B'),
    ((520, 136, 96), dict(akc=1, bkc=0, pre=1, b_gstride=96 * 32), 1, 'mn-blocked B'),
    ((520, 136, 96), dict(Q8, cp=1, split=3), 1, 'column partials'),
    ((520, 160, 96), dict(Q8, chain=chain_min(520), acc=1), 1, 'chain-order'),
    ((520, 160, 96), dict(Q8, chain=chain_min(520), mask=1), 1, 'chain-order'),
    ((520, 160, 96), dict(Q8, chain=chain_min(520), split=3), 1, 'chain-order'),
    ((520, 160, 96), dict(Q8, chain=chain_min(520) - 1024), 1, 'chain-order'),
    ((520, 136, 96), dict(Q8, chain=chain_min(520)), 1, 'chain-order'),    # N % 32 != 0
    ((520, 136, 96), dict(akc=1, bkc=1, split=3, deferred=1, bias=1), 1, 'deferred'),
    ((520, 136, 96), dict(akc=1, bkc=1, split=3, no_slab=True), 1, 'slab'),
    ((520, 136, 100), dict(akc=1, bkc=1, pre=1), 1, 'pre-split'),
    ((520, 134, 96), dict(akc=1, bkc=1), 1, 'N %'),
    ((520, 136, 98), dict(akc=1, bkc=0), 1, 'K %'),
    ((522, 136, 96), dict(akc=0, bkc=0), 1, 'M %'),
    # mode 0 has none of the extended options
    ((520, 136, 96), dict(akc=1, bkc=0, cp=1), 0, 'bf16-split'),
    ((520, 136, 96), dict(akc=1, bkc=0, step=True), 0, 'bf16-split'),
    ((520, 160, 96), dict(akc=1, bkc=0, chain=chain_min(520)), 0, 'bf16-split'),
    ((520, 136, 96), dict(Q8, row_live=(1, 1, 1)), 0, 'bf16-split'),
    ((1028, 200, 96), dict(WG, kl=[0, 1, 2]), 0, 'bf16-split'),
    ((520, 136, 96), dict(Q8, mbits_out=1), 0, 'bf16-split'),
    ((520, 136, 96), dict(Q8, mbits=True), 0, 'bf16-split'),
    ((520, 136, 96), dict(akc=1, bkc=1, a_kstride=520 * 32), 0, 'bf16-split'),
    ((520, 136, 96), dict(akc=1, bkc=0, b_gstride=96 * 32), 0, 'bf16-split'),
    ((1800, 80, 64), dict(WG, a_gstride=2048), 0, 'mn-blocked A'),
]


@pytest.mark.parametrize('shape,opts,mode,word', REFUSED, ids=[
    '%dx%dx%d-mode%d-%s' % (s + (m, '+'.join(k for k, v in o.items() if v and k not in ('akc', 'bkc')))) for s, o, m, _ in REFUSED])
def test_refused(lib, gemm_mode, shape, opts, mode, word):
    """What the launcher documents as refused: 22 with a message, nothing launched (no form named)
    and every output as it was."""
    gemm_mode(mode)
    P = problem(*shape)
    o = dict(opts)
    if o.get('step'):
        o['step'] = Guarded(1, np.int64, init=41)
    if o.get('mbits') is True:
        o['mbits'] = np.zeros(int(lib.lbwn_gemm_mbits_words_abi(P.M, P.N)), np.int64)
    r = launch(lib, P, refused=True, **o)
    assert word in r.err, r.err
    if o.get('step'):
        assert int(o['step'].read('step counter')[0]) == 41


def test_refused_struct_size(lib):
    a = _lib.GemmExArgs()
    a.struct_size += 8
    assert lib.lbwn_gemm_ex(ctypes.byref(a), None) == 22 and b'struct_size' in lib.lbwn_last_error()


# ---- head widths that are no multiple of 32, through whole plans ------------------------------

@pytest.mark.parametrize('Cs,Cp,Q,B,T', [(200, 100, 100, 2, 200), (200, 100, 100, 2, 4096), (136, 72, 260, 2, 200),
                                         (640, 96, 256, 2, 200), (64, 32, 520, 2, 200)])
def test_plan_odd_head_widths(lib, Cs, Cp, Q, B, T):
    """lbwn_plan_create takes any n_skip / n_post / n_quant (padded to 4): forward, SAVE, every
    gradient and every layer's z against the float64 oracle at widths that leave ragged column
    tiles in every head GEMM (136 = 128 + 8, 200, 100 and 72 below one tile, 96 and 640 = the
    96- and 160-column forms, 260 past 256); B·T = 8192 runs the tall forms at ragged N; n_quant = 520
    is the generic head kernel and a PRE gradient histogram past 64 KB of LDS."""
    check_plan(small_arch(nb=1, nbl=4, Cs=Cs, Cp=Cp, Q=Q), B, T)


def test_forms_seen():
    """The names lbwn_gemm_last_form reported over the module: nothing the list above does not
    have and, when the whole form matrix ran, all of it."""
    seen = {f for _, f in SEEN}
    assert seen <= DISPATCHER_FORMS, seen - DISPATCHER_FORMS
    if len({i for i, _ in SEEN}) == len({case_id(c) for c in TABLE}):
        assert seen == DISPATCHER_FORMS, DISPATCHER_FORMS - seen
