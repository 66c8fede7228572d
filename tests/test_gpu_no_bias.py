"""use_bias = false on the GPU: every path of the training plan, and the single-layer entries with
null bias pointers, against float64.

The library never reads arch.use_bias; it branches on each bias pointer of lbwn_params being null
("Bias pointers are NULL when !use_bias", include/lbwn.h).  The cases are tests/gradcheck.py
NO_BIAS_CASES (tests/test_no_bias.py holds their relu ties to adoption_capped on the CPU), each the
smallest shape that reaches its branch, through check_plan / check_conditioning of
tests/test_gpu_parity.py with its bars unchanged: z at 1e-5 on identical inputs, SAVE / s / r2 by
close, every gradient and backward intermediate at 2e-4 of its own max (grad_close), exact zeros
where the reference is zero.  Every backward starts from gradients filled with NaN and must leave
them finite ("grads: every pointer of the struct is fully overwritten").

Worst max-err / own-max measured on the MI355X (printed by every run with -s; the bar is 2e-4 =
200e-6), in units of 1e-6; "with" is the with-bias value of tests/test_gpu_parity.py's table that
the row is to be read against:

    group       small (2, 256), 5 forms    arch3 (2, 512), 5 forms    small (2, 256) f32 MFMA
                no bias      with          no bias      with          no bias
    PRE         0.56         0.66          3.2          2.8           0.56
    SIGNAL      0.53         1.3           3.8          8.7           0.72
    GATE        0.73         1.3           4.3          8.6           0.98
    RESIDUAL    0.59         1.5           4.5          6.2           0.93
    SKIP        0.87         1.1           2.5          1.5           0.71
    POST1       0.69         1.2           1.5          0.89          0.54
    POST2       0.59         0.36          0.92         0.75          0.66
    dlogits     0.03         0.03          0.04         0.05          0.03
    dh          0.75         0.85          1.1          1.1           1.3
    ds          0.30         0.38          0.77         0.67          0.40
    dz          0.24         0.42          0.83         0.92          0.38

Every other case sits there too.  (1, 129), (5, 333) and the live-halo batch, every form: at most
1.2 (POST1).  arch3 (2, 96): at most 3.8 (GATE).  The tall forms (2, 4096): 1.3 (POST1).  The
per-layer kernels: n_res = n_dil = 16 at most 1.0 (GATE), the arch2 widths 2.5 (GATE).  The padded
heads (200, 100, 100) / (136, 72, 260) / (64, 32, 520): 0.63 / 0.82 / 0.96.  Conditioning, (2, 256) and
(3, 136), every form, beside tests/test_gpu_parity.py's with-bias figures in brackets: GC_EMBED 0.90
(0.96), GC_SIGNAL / GC_GATE 0.73 / 0.75 (0.79 / 0.92), LC_SIGNAL / LC_GATE 0.77 / 0.89 (0.74 / 0.87),
LC_UPSAMPLE 0.64 (0.62), dvall 0.50 (0.47), gcd 0.82 (0.86).  The single-layer backward: dx_in, dw_sig,
dw_gate, dw_res at most 0.42.  No group is 2x above its with-bias value; the arithmetic is the same, the
bias rows of the images are zeros.

The (64, 32, 520) head found the one defect: the plan took n_quant = 520 but its backward refused it,
with or without biases (the PRE gradient's histogram was limited to 64 KB of LDS, n_quant <= 512);
lbwn_pre_grad_launch now asks for up to 128 KB, n_quant <= 1024."""
import numpy as np
import pytest
import torch

from lbwn import _lib
from oracle import wavenet_ref as R
from tests.gradcheck import NO_BIAS_CASES, arch3_no_bias, grad_close, small_arch
from tests.test_gpu_masked_skip import check_masked_skip
from tests.test_gpu_parity import DEV, check_adam_step, check_conditioning, check_plan, gemm_mode  # noqa: F401
from tests.test_no_bias import BIAS_KINDS

pytestmark = pytest.mark.gpu


def run_case(key, form=''):
    mk, B, T, invalid, seed, cond = NO_BIAS_CASES[key]
    arch = mk()
    assert arch['use_bias'] is False
    if cond:
        net = check_conditioning(1, 1, arch['n_res'], B, T, form, arch=arch, seed=seed, poison_grads=True)
        assert all(getattr(net._params_c, f) is None and getattr(net._grads_c, f) is None for f in BIAS_KINDS)
    else:
        check_plan(arch, B, T, invalid=invalid, seed=seed, poison_grads=True, title='no bias %s %s' % (key, form))


def one_chain_form(monkeypatch):
    monkeypatch.setenv('LBWN_CHAIN_TILE', 'w32')
    monkeypatch.setenv('LBWN_BWD_WGRAD', '0')


# ---- the training plan -------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['small_2x256', 'small_1x129', 'small_5x333', 'small_live_halo_2x256'])
def test_chain_forms(lib, key, chain_tile):
    """The x3 forward and backward chains and the in- and out-of-chain weight gradients, whose images
    hold zero bias rows and whose slab bias columns nobody asks for: the baseline, one tile plus one
    position, ragged in 32 / 64 / 128 with tiles straddling streams, and live halo rows."""
    run_case(key, chain_tile)


def test_f32_mfma_mode(lib, gemm_mode, monkeypatch):
    """GEMM mode 0: the bias gradients' !fcols branch with no job at all, and no SKIP_BIAS rows to
    broadcast."""
    one_chain_form(monkeypatch)
    gemm_mode(0)
    run_case('small_2x256', 'f32 MFMA')


@pytest.mark.parametrize('key', ['arch3_2x512', 'arch3_2x96'])
def test_arch3(lib, key, chain_tile):
    """par/arch3.json without biases: the full depth, and T = 96 with the dilations 128 .. 512 past the
    slice."""
    run_case(key, chain_tile)


def test_tall_gemm_forms(lib, monkeypatch):
    """M = 8192, the smallest M of the tall 256-row forms: dH1 and dS launched with no colpart (another
    dispatch path than with biases) and every head GEMM with bias = nullptr."""
    one_chain_form(monkeypatch)
    run_case('tall_2x4096', 'w32')


@pytest.mark.parametrize('key', ['layers16_2x256', 'arch2_widths_2x200'])
def test_per_layer_kernels(lib, key):
    """Widths the chains do not take: lbwn_layer_fwd / bwd_launch on images packed from null bias
    pointers, and lbwn_layer_reduce_launch with dbsig = dbgate = dbres = nullptr."""
    run_case(key)


@pytest.mark.parametrize('key', ['head_200_100_100', 'head_136_72_260', 'head_64_32_520'])
def test_padded_head_images(lib, monkeypatch, key):
    """head_pad_params / head_pad_grads / head_unpad_grads without their bias pieces; Q = 260 is
    head_reg_kernel<8>; Q = 520 the generic head_kernel, which writes no column partials, so the first
    colsum pass is skipped because there is no POST2_BIAS gradient to sum."""
    one_chain_form(monkeypatch)
    run_case(key, 'w32')


@pytest.mark.parametrize('key', ['cond32_2x256', 'cond32_3x136', 'cond16_2x256'])
def test_conditioning(lib, key, chain_tile):
    """GC + LC without biases: the GC table gradient comes from the backward chain's slab bias
    partials (lbwn_gc_tile_sum_launch) and must be right when nobody asks for the bias gradients."""
    run_case(key, chain_tile)


@pytest.mark.parametrize('pattern', ['all_zero', 'dealer'])
def test_masked_skip(monkeypatch, pattern):
    """tests/test_gpu_masked_skip.py's comparison on arch3 without biases at its shape (2, 4096): a
    skipped tile's epilogue writes plain zeros; all_zero leaves every gradient exactly zero (from NaN)
    with stats[1] == 0."""
    check_masked_skip(monkeypatch, pattern, 2, 4096, arch=arch3_no_bias(), poison_grads=True)


def test_adam_step_matches_oracle():
    """Every element is a weight: l2 applies to the whole buffer (n_weights == n_total through
    lbwn.optim.AdamOptimizer)."""
    net = check_adam_step(small_arch(nb=1, nbl=3, use_bias=False))
    assert net.layout.n_weights == net.layout.n_total == net.flat.numel()
    assert all(getattr(net._params_c, f) is None and getattr(net._grads_c, f) is None for f in BIAS_KINDS)


# ---- the single-layer entries with null bias pointers --------------------------------------------

CANARY = 8


def _layer_problem(d, T, C, given):
    """One layer in float64 (the formula of tests/test_gpu_parity.py::test_layer_forward) with the
    biases named in `given`; the others are absent (None)."""
    B, H = 2, 512
    rng = np.random.default_rng(d + T + C)
    p = dict(B=B, H=H, T=T, d=d, C=C)
    p['xbuf'] = rng.uniform(-1, 1, size=(B, H + T, C))
    p['Ws'] = rng.uniform(-0.3, 0.3, size=(2, C, C))
    p['Wg'] = rng.uniform(-0.3, 0.3, size=(2, C, C))
    p['Wr'] = rng.uniform(-0.3, 0.3, size=(C, C))
    for nm in ('bs', 'bg', 'br'):
        b = rng.uniform(-0.1, 0.1, C)
        p[nm] = b if nm in given else None
    return p


def _bias(p, nm):
    return 0.0 if p[nm] is None else p[nm]


def _dev(a):
    return None if a is None else torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _with_canary(*shape):
    """A NaN-filled output buffer with CANARY NaN floats after it: (whole, output view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + CANARY,), float('nan'), device=DEV)
    return whole, whole[:n].view(*shape)


def _canary_intact(whole, name):
    assert bool(torch.isnan(whole[-CANARY:]).all()), '%s: written past its end' % name


@pytest.mark.parametrize('d,T,C,given', [(1, 128, 32, ()), (64, 256, 32, ()), (512, 300, 5, ()), (2, 200, 5, ()),
                                         (64, 256, 32, ('bs',))])
def test_layer_forward_null_biases(lib, d, T, C, given):
    """lbwn_layer_forward with b_sig = b_gate = b_res = NULL, and with b_sig alone given (each bias is
    nullable on its own and the packers branch per pointer): z at 1e-5, x_out at 2e-5."""
    p = _layer_problem(d, T, C, given)
    B, H = p['B'], p['H']
    x, prev = p['xbuf'][:, H:], p['xbuf'][:, H - d:H - d + T]
    z = (np.tanh(prev @ p['Ws'][0] + x @ p['Ws'][1] + _bias(p, 'bs'))
         * R._sigmoid(prev @ p['Wg'][0] + x @ p['Wg'][1] + _bias(p, 'bg')))
    xo = x + z @ p['Wr'] + _bias(p, 'br')
    xin, ws_, wg_, wr_, bs_, bg_, br_ = (_dev(p[k]) for k in ('xbuf', 'Ws', 'Wg', 'Wr', 'bs', 'bg', 'br'))
    zw, zout = _with_canary(B * T, C)
    xw, xout = _with_canary(B, H + T, C)
    wpk = torch.empty(lib.lbwn_layer_image_floats_abi(), device=DEV)
    _lib.check(lib.lbwn_layer_forward(xin.data_ptr(), xout.data_ptr(), zout.data_ptr(), C, ws_.data_ptr(),
                                      wg_.data_ptr(), _ptr(bs_), _ptr(bg_), wr_.data_ptr(), _ptr(br_),
                                      None, None, None, 0, B, T, H, d, C, C, wpk.data_ptr(), None))
    torch.cuda.synchronize()
    np.testing.assert_allclose(zout.cpu().numpy().reshape(B, T, C), z, rtol=0, atol=1e-5)
    np.testing.assert_allclose(xout.cpu().numpy()[:, H:], xo, rtol=0, atol=2e-5)
    _canary_intact(zw, 'z')
    _canary_intact(xw, 'x_out')


@pytest.mark.parametrize('d,T,C', [(1, 128, 32), (64, 256, 32), (2, 200, 5)])
def test_layer_backward_null_biases(lib, d, T, C):
    """lbwn_layer_backward with the three biases and db_sig = db_gate = db_res NULL: dx_in, dw_sig,
    dw_gate and dw_res against float64 under grad_close, the halo rows before H - d exactly zero,
    and nothing written past any output."""
    p = _layer_problem(d, T, C, ())
    B, H = p['B'], p['H']
    rng = np.random.default_rng(7 + d + T + C)
    dz = rng.uniform(-1, 1, size=(B, T, C))
    dxo = rng.uniform(-1, 1, size=(B, T, C))
    x, prev = p['xbuf'][:, H:], p['xbuf'][:, H - d:H - d + T]
    vs = prev @ p['Ws'][0] + x @ p['Ws'][1]
    vg = prev @ p['Wg'][0] + x @ p['Wg'][1]
    ts, sg = np.tanh(vs), R._sigmoid(vg)
    g = dz + dxo @ p['Wr'].T                               # dL/dz: the skip path's share + the residual's
    dvs, dvg = g * sg * (1 - ts * ts), g * ts * sg * (1 - sg)
    ref = dict(dw_res=np.einsum('btc,bto->co', ts * sg, dxo),
               dw_sig=np.stack([np.einsum('bti,bto->io', prev, dvs), np.einsum('bti,bto->io', x, dvs)]),
               dw_gate=np.stack([np.einsum('bti,bto->io', prev, dvg), np.einsum('bti,bto->io', x, dvg)]))
    dx = np.zeros_like(p['xbuf'])
    dx[:, H:] += dxo + dvs @ p['Ws'][1].T + dvg @ p['Wg'][1].T
    dx[:, H - d:H - d + T] += dvs @ p['Ws'][0].T + dvg @ p['Wg'][0].T
    ref['dx_in'] = dx
    xin, ws_, wg_, wr_, dzd, dxod = (_dev(a) for a in (p['xbuf'], p['Ws'], p['Wg'], p['Wr'], dz, dxo))
    out = {'dx_in': _with_canary(B, H + T, C), 'dw_sig': _with_canary(2, C, C), 'dw_gate': _with_canary(2, C, C),
           'dw_res': _with_canary(C, C)}
    nws = int(lib.lbwn_layer_backward_ws_floats(B, T, C))
    wsw = torch.full((nws + CANARY,), float('nan'), device=DEV)
    assert wsw.data_ptr() % 16 == 0
    _lib.check(lib.lbwn_layer_backward(xin.data_ptr(), dzd.data_ptr(), C, dxod.data_ptr(), ws_.data_ptr(),
                                       wg_.data_ptr(), None, None, wr_.data_ptr(), None, None, None, None, 0,
                                       out['dx_in'][1].data_ptr(), out['dw_sig'][1].data_ptr(),
                                       out['dw_gate'][1].data_ptr(), None, None, out['dw_res'][1].data_ptr(), None,
                                       None, 0, None, B, T, H, d, C, C, wsw.data_ptr(), None))
    torch.cuda.synchronize()
    for name, (whole, view) in out.items():
        got = view.cpu().double().numpy()
        assert np.isfinite(got).all(), '%s: not fully written' % name
        print('%s: max err / own max %.3g' % (name, grad_close(got, ref[name], name)))
        _canary_intact(whole, name)
    _canary_intact(wsw, 'workspace')
    assert not out['dx_in'][1][:, :H - d].any(), 'halo rows before H - d'
