"""Every branch of the conditioning dispatch (csrc/engine.cpp cond_forward, lc_wgrad, lc_dlc,
lc_upsample_bwd, gc_backward; csrc/cond.hip lbwn_lc_up_fused_ok) through the whole plan:
check_conditioning of tests/test_gpu_parity.py (forward, SAVE, loss, every gradient and dvall / gcd
against the float64 oracle at the project's bars: 1e-5 / 2e-5 forward, 2e-4 of each gradient's own
max) on archs chosen so that each side of each shape-selected branch is taken, and the branch taken
is asserted with lbwn_plan_info.  test_table_covers_every_branch (no GPU) creates the same plans
without a device and holds the table to its branches, so a later change to a threshold cannot move
a case to another branch unnoticed.

Base: 1 block of 4 layers, C = 32 (the persistent chains), B = 2, T = 256, the default chain tile.

Worst max-err / own-max of the conditioning gradients measured on the MI355X, in units of 1e-6
(the bar is 200; printed per case by every run with -s):

    case                          LC_UPSAMPLE  LC_SIGNAL  LC_GATE  dvall   worst of any tensor
    8->24 [8,8,4] T=512              0.48        0.61      0.55    0.37    PRE_BIAS 1.4
    4->4 [8]                         0.43        0.55      0.77    0.45    SIGNAL_BIAS 0.92
    4->44 [3,8,8,1] T=384            0.78        0.54      0.65    0.37    POST1 1.2
    8->16 [2] B=3                    0.43        0.47      0.49    0.44    PRE_BIAS 1.0
    24->16 [2,4]                     0.56        0.69      0.43    0.38    dh 0.98
    8->16 [16]                       0.44        0.58      0.52    0.37    SKIP 0.98
    8->16 [2,2,2,2,2]                0.60        0.67      0.63    0.41    SIGNAL_BIAS 1.1
    8->16 [8,8,8] T=512              0.57        0.47      0.45    0.40    dh 0.93
    24->16 [2,4] T=2048              0.62        0.61      0.81    0.37    RESIDUAL_BIAS 2.2
    12->16 [2,4] 2 blocks            0.56        0.92      0.68    0.42    SIGNAL_BIAS 0.99
    12->16 [2,4] 3 layers            0.50        0.85      0.69    0.39    dh 0.97
    20->64 [2,4]                     0.43        0.54      0.63    0.35    PRE_BIAS 1.4
    20->84 [2,4]                     0.64        0.54      0.57    0.34    PRE_BIAS 1.4
    20->68 [2,4] (five tiles)        0.57        0.57      0.59    0.37    PRE_BIAS 0.98
    20->76 [2,4] (five tiles)        0.60        0.53      0.65    0.61    RESIDUAL_BIAS 1.2

    GC only (Ge, ncat, layers)    GC_EMBED  GC_SIGNAL  GC_GATE  gcd     worst of any tensor
    (32, 8, 5)                      0.82      0.72       1.0     0.71    PRE_BIAS 1.4
    (1, 1, 4)                       2.2       1.4        2.0     0.95    GC_EMBED 2.2
    (16, 16, 4)                     0.42      0.66       0.73    0.93    POST1 1.3

Every branch sits where float32 arithmetic sits (the float32 oracle of tests/test_gpu_parity.py: 1.2),
90x inside the bar; no branch stands out.  No case needed another seed for the relu adoption cap.
"""
import ctypes

import pytest

from lbwn import _lib
from tests.gradcheck import cond_arch

gpu = pytest.mark.gpu

GE2 = ('>=', 2)


def case(name, Li=12, Lo=16, strides=(2, 4), B=2, T=256, nb=1, nbl=4, expect=None, after=None, seed=0):
    return dict(name=name, arch=cond_arch(0, 1, 32, Li=Li, Lo=Lo, strides=strides, n_blocks=nb, n_block_layers=nbl),
                B=B, T=T, expect=expect or {}, after=after or {}, seed=seed)


FUSED = dict(up_fused=1, up_fused_bwd=1, lc_in_chain=0)
UNFUSED = dict(up_fused=0, up_fused_bwd=0, lc_in_chain=0)
# expect: lbwn_plan_info at plan creation; after: once a backward has run
LC_TABLE = [
    case('8->24 [8,8,4] T=512: fused both ways, hop 256', 8, 24, (8, 8, 4), T=512, expect=FUSED,
         after=dict(dlc_parts=1)),
    case('4->4 [8]: fused, one stage, cond_project', 4, 4, (8,), expect=FUSED),
    case('4->44 [3,8,8,1] T=384: fused, second work item', 4, 44, (3, 8, 8, 1), T=384, expect=FUSED),
    case('8->16 [2] B=3: fused forward, 384 frames: GEMM backward', 8, 16, (2,), B=3,
         expect=dict(up_fused=1, up_fused_bwd=0, lc_in_chain=0, split_up0=1)),
    case('24->16 [2,4]: unfused (Li > Lo)', 24, 16, (2, 4), expect=dict(UNFUSED, split_up0=1, split_up1=1)),
    case('8->16 [16]: unfused (stride above 8)', 8, 16, (16,), expect=UNFUSED),
    case('8->16 [2,2,2,2,2]: unfused (five stages)', 8, 16, (2, 2, 2, 2, 2), expect=UNFUSED),
    case('8->16 [8,8,8] T=512: unfused (hop 512)', 8, 16, (8, 8, 8), T=512, expect=UNFUSED),
    case('24->16 [2,4] T=2048: unfused, split-K stage gradient', 24, 16, (2, 4), T=2048,
         expect=dict(UNFUSED, split_up0=1, split_up1=GE2)),
    case('12->16 [2,4] 2 blocks: dlc split-K partials summed by the fused backward', nb=2,
         expect=dict(FUSED, split_dlcx=2), after=dict(dlc_parts=2, dv_blk=1)),
    case('12->16 [2,4] 3 layers: ncond 192, the LDS-staged lc_wgrad on the k-blocked DV', nbl=3,
         expect=dict(FUSED, split_dlcx=1), after=dict(dv_blk=1, dlc_parts=1)),
    case('20->64 [2,4]: below the in-chain window', 20, 64, (2, 4), expect=FUSED),
    case('20->84 [2,4]: above the in-chain window', 20, 84, (2, 4), expect=FUSED),
]
IN_CHAIN = dict(up_fused=1, up_fused_bwd=1, lc_in_chain=1)
TILE_TABLE = [      # run at every chain_tile: both LC image layouts
    case('20->68 [2,4]: in-chain LC, narrowest', 20, 68, (2, 4), expect=IN_CHAIN, after=dict(dv_blk=1)),
    case('20->76 [2,4]: in-chain LC, padded to 80', 20, 76, (2, 4), expect=IN_CHAIN, after=dict(dv_blk=1)),
]
# GC only (Ge, ncat, layers): Ge at its limit with a ragged n chunk (N = 320); the smallest; the ep switch
GC_TABLE = [(32, 8, 5), (1, 1, 4), (16, 16, 4)]


def arch_struct(arch):
    a = _lib.Arch()
    for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post', 'n_gc_embed',
              'n_gc_category', 'n_lc_in', 'n_lc_out'):
        setattr(a, k, int(arch[k]))
    ups = arch['lc_upsample'] if arch['n_lc_out'] > 0 else []
    a.n_lc_upsample = len(ups)
    for i, s in enumerate(ups):
        a.lc_upsample[i] = int(s)
    a.use_bias = int(arch['use_bias'])
    return a


def holds(info, expect, name):
    for k, want in expect.items():
        got = info(k)
        if isinstance(want, tuple):
            assert got >= want[1], '%s: %s = %d, wanted >= %d' % (name, k, got, want[1])
        else:
            assert got == want, '%s: %s = %d, wanted %d' % (name, k, got, want)


def test_table_covers_every_branch(lib, monkeypatch):
    """Plans are created without a device.  Each case takes the branch its row names, and over the
    table up_fused, up_fused_bwd, lc_in_chain, split_dlcx > 1, split_up* > 1 and ncond >= 256 each
    take both values."""
    for v in ('LBWN_NO_CHAIN', 'LBWN_CHAIN_TILE'):
        monkeypatch.delenv(v, raising=False)
    seen = {}
    for c in LC_TABLE + TILE_TABLE:
        a, h = c['arch'], ctypes.c_void_p()
        _lib.check(lib.lbwn_plan_create(ctypes.byref(arch_struct(a)), c['B'], c['T'], ctypes.byref(h)))

        def info(key):
            v = _lib.c_int64(-1)
            _lib.check(lib.lbwn_plan_info(h, key.encode(), ctypes.byref(v)))
            return v.value
        try:
            holds(info, c['expect'], c['name'])
            nup = len(a['lc_upsample'])
            facts = dict(up_fused=info('up_fused'), up_fused_bwd=info('up_fused_bwd'), lc_in_chain=info('lc_in_chain'),
                         split_dlcx=int(info('split_dlcx') > 1),
                         split_up=int(any(info('split_up%d' % i) > 1 for i in range(nup))),
                         ncond=int(2 * a['n_blocks'] * a['n_block_layers'] * a['n_dil'] >= 256))
            assert all(info('split_up%d' % i) == 0 for i in range(nup, 8)), c['name']
            assert info('dv_blk') == 0 and info('dlc_parts') == 1, c['name']      # no backward yet
            v = _lib.c_int64(7)
            assert lib.lbwn_plan_info(h, b'no_such_key', ctypes.byref(v)) == 22 and v.value == 7
            assert b"unknown key 'no_such_key'" in lib.lbwn_last_error()
        finally:
            lib.lbwn_plan_destroy(h)
        for k, val in facts.items():
            seen.setdefault(k, set()).add(val)
    assert seen == {k: {0, 1} for k in ('up_fused', 'up_fused_bwd', 'lc_in_chain', 'split_dlcx', 'split_up',
                                        'ncond')}, seen
    v = _lib.c_int64()
    assert lib.lbwn_plan_info(None, b'up_fused', ctypes.byref(v)) == 22


def run_case(c, tile):
    from tests.test_gpu_parity import check_conditioning
    net = check_conditioning(0, 1, 32, c['B'], c['T'], '%s | %s' % (c['name'], tile), arch=c['arch'], seed=c['seed'])
    holds(lambda k: net.plan_info(c['T'], k), dict(c['expect'], **c['after']), c['name'])


@gpu
@pytest.mark.parametrize('c', LC_TABLE, ids=lambda c: c['name'].split(':')[0].replace(' ', '_'))
def test_lc_branch(c, monkeypatch):
    monkeypatch.delenv('LBWN_CHAIN_TILE', raising=False)
    run_case(c, 'default tile')


@gpu
@pytest.mark.parametrize('c', TILE_TABLE, ids=lambda c: c['name'].split(':')[0].replace(' ', '_'))
def test_lc_in_chain_widths(c, chain_tile):
    run_case(c, chain_tile)


@gpu
@pytest.mark.parametrize('Ge,ncat,nbl', GC_TABLE)
def test_gc_edges(Ge, ncat, nbl, monkeypatch):
    """GC only, through gc_tile_sum and the atomics of the mixed-voice tiles."""
    from tests.test_gpu_parity import check_conditioning
    monkeypatch.delenv('LBWN_CHAIN_TILE', raising=False)
    arch = cond_arch(1, 0, 32, n_block_layers=nbl, Ge=Ge, ncat=ncat)
    check_conditioning(1, 0, 32, 2, 256, 'GC only Ge %d ncat %d %d layers' % (Ge, ncat, nbl), arch=arch)
