"""lc_up_bwd_kernel<true> (csrc/cond.hip): the fused LC upsample backward that also forms stage 0's input
gradient (its K spread over the block, the slices combined in a fixed order) and stores the row, d(mel),
through lbwn_lc_upsample_backward_dmel on every entry of LC_RUNS of tests/test_gpu_cond_kernels.py: 14
shapes x 1 and 3 frames, 257 frames, and three split-K partials.
Those shapes hold the places where the new stage can go wrong: one stage, where stage 0 is also the last
and D is dlc itself (4->4 [8], 16->16 [4], 8->8 [1]); stride 1 four times; Li < Lo at the W carve's limit
(4->196 [4]: one column group, 49 K slices); Li = Lo = 68 (17 x 17 threads); widths of 4 (one slice of one
o group); hop 256; the second work item of the stages above (4->44 [3,8,8,1]).

Reference: tests/dmel_ref.py kernel_dmel_ref, the din chain of oracle lc_upsample_bwd in float64 on the
f32 inputs the kernel read.  dmel sits NaN-filled between NaN canaries (Out).

Tolerance, derived as in tests/test_gpu_cond_kernels.py and with no margin: the forward error bound of
the chain of sums, element by element,
    |got - ref| <= gamma_K · (|D|·|F_{nup-1}|···|F_0|),   K = (parts - 1) + Σ_{k=0}^{nup-1} 2·s_k·Lo,
|D| the sum of the partials' absolute values (two operations per term: no reliance on contraction; any
summation order).  tests/test_dmel.py holds the comparison to both sides without a GPU.

Also asserted: dF and dpart are bitwise those of lbwn_lc_upsample_backward on the same inputs; a second
call gives bitwise the same dmel; act is untouched.

Worst err / bound measured on the MI355X per case (printed with -s; the assertion is a ratio <= 1), at
1 frame / 3 frames:

    12->16 [2,4]       7.1e-4 / 1.5e-3      8->20 [3,5]        3.4e-4 / 4.6e-4
    16->16 [4,4]       5.8e-4 / 6.9e-4      20->36 [5,3,2]     2.7e-5 / 2.4e-5
    16->16 [4]         3.0e-3 / 5.4e-3      8->24 [8,8,4]      1.2e-5 / 2.4e-5
    4->4 [8]           3.9e-3 / 1.7e-2      4->80 [4,4,4,4]    7.2e-8 / 1.5e-7
    8->8 [1]           3.2e-2 / 5.6e-2      68->68 [4,4,4]     6.4e-6 / 6.4e-6
    4->4 [1,1,1,1]     9.6e-3 / 2.1e-2      4->72 [2,7,1]      8.7e-6 / 8.6e-6
    4->196 [4]         2.3e-4 / 4.0e-4      4->44 [3,8,8,1]    4.2e-7 / 1.1e-6
    257 frames:        12->16 [2,4] 2.7e-3, 4->4 [8] 4.7e-2
    3 split-K partials, 3 frames: 12->16 [2,4] 8.1e-4, 8->20 [3,5] 4.2e-4, 4->80 [4,4,4,4] 1.7e-7

The worst, 0.056, is 8->8 [1] (K = 16, one stage of stride 1: the bound is at its tightest where the sums are
shortest); the ratio falls as the chain grows because the bound multiplies absolute values through every
stage (|D|·|F|···|F| grows like the width per stage, the rounding error like its square root), as the dF
ratios of tests/test_gpu_cond_kernels.py do.  The bound still tells a wrong kernel from a right one at the
deep end: a missing phase of stage 0 is an error of the order of the value itself (tests/test_dmel.py: 4000x
the bound at 12->16 [2,4], 7x at 68->68 [4,4,4], the deepest and widest chain of the list).
"""
import numpy as np
import pytest
import torch

from lbwn import _lib
from tests.dmel_ref import check_kernel_dmel, kernel_dmel_ref
from tests.test_gpu_cond_kernels import (LC_RUNS, Out, c_ints, c_ptrs, case_name, dev, gpu_forward, lc_problem,
                                         stage_shapes)

gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@gpu
@pytest.mark.parametrize('case,frames,parts', LC_RUNS, ids=lambda v: str(v).replace(' ', ''))
def test_lc_upsample_backward_dmel(lib, case, frames, parts):
    Li, Lo, strides = case
    nup = len(strides)
    mel, F, dlc, stride = lc_problem(Li, Lo, strides, frames, parts)
    acts, md, Fd = gpu_forward(lib, Li, Lo, strides, frames, mel, F)
    acts_before = [a.buf.view(torch.int32).clone() for a in acts]
    name = case_name(Li, Lo, strides, frames, parts)
    shp = stage_shapes(Li, Lo, strides)
    nfl = int(lib.lbwn_lc_upsample_part_floats(nup, c_ints(strides), Li, Lo, frames))
    dd = dev(dlc)
    head = (nup, c_ints(strides), Li, Lo, frames, md.data_ptr(), c_ptrs([f.data_ptr() for f in Fd]),
            c_ptrs([a.ptr() for a in acts]), dd.data_ptr(), parts, stride)

    def run(with_dmel):
        dpart, dF = Out(nfl), [Out(s * Lo * I) for s, I, _ in shp]
        tail = (dpart.ptr(), c_ptrs([o.ptr() for o in dF]))
        dmel = Out(frames * Li) if with_dmel else None
        if with_dmel:
            _lib.check(lib.lbwn_lc_upsample_backward_dmel(*head, *tail, dmel.ptr(), None))
        else:
            _lib.check(lib.lbwn_lc_upsample_backward(*head, *tail, None))
        torch.cuda.synchronize()
        return (dpart.read('dpart ' + name), [o.read('dF[%d] %s' % (i, name)) for i, o in enumerate(dF)],
                dmel.read('dmel ' + name, (frames, Li)) if with_dmel else None)

    dpart0, dF0, _ = run(False)
    dpart1, dF1, dmel1 = run(True)
    _, _, dmel2 = run(True)
    ref, bound = kernel_dmel_ref(Li, Lo, strides, frames, F, dlc)
    check_kernel_dmel(name, dmel1, ref, bound)
    assert np.array_equal(bits(dmel1), bits(dmel2)), name + ': two calls, two dmel'
    assert np.array_equal(bits(dpart0), bits(dpart1)), name + ': dpart differs from lbwn_lc_upsample_backward'
    for i in range(nup):
        assert np.array_equal(bits(dF0[i]), bits(dF1[i])), '%s: dF[%d] differs from lbwn_lc_upsample_backward' % (name, i)
    for i, (a, b) in enumerate(zip(acts, acts_before)):      # the backward only reads them
        assert torch.equal(a.buf.view(torch.int32), b), '%s: act[%d] changed' % (name, i)
