"""float64 references of dmel, the gradient with respect to the mel input, for
tests/test_dmel.py (CPU) and tests/test_gpu_dmel_kernel.py / test_gpu_dmel_plan.py.

Whole network: from the oracle's public pieces only.  R.backward(..., intermediates=True) leaves
cache['bwd']['dv'] (per layer [B, T, 2·Cd], signal | gate);
    dlc = Σ_l dv_sig·LC_SIGNAL_lᵀ + dv_gate·LC_GATE_lᵀ
is the gradient into the upsample stack's output, and R.lc_upsample_bwd(arch, P, cache['lc_acts'],
dlc, {}) returns the stage-0 input gradient that R.backward discards.  The oracle's dlogits are those of
the MEAN loss, so this is d(mean xent)/d(mel): the GPU's raw sums are divided by n_valid before they
are compared, as the other gradient tests do.

Kernel: the stage chain of lbwn_lc_upsample_backward_dmel on the inputs of
tests/test_gpu_cond_kernels.py lc_problem, with the forward error bound of that file beside it.
"""
import numpy as np

from oracle import wavenet_ref as R
from tests.test_gpu_cond_kernels import gamma, stage_shapes


# ---- whole network ---------------------------------------------------------------------------------

def dlc_from_cache(arch, P, cache):
    """d(loss)/d(lc) [B, T, n_lc_out] from the dv the oracle's backward left in cache['bwd']."""
    Cd, dlc = arch['n_dil'], 0.0
    for l in range(R.n_layers(arch)):
        b, bl, _ = R.layer_index(arch, l)
        sfx = '_%d_%d' % (b, bl)
        dv = cache['bwd']['dv'][l]
        dlc = dlc + dv[..., :Cd] @ P['LC_SIGNAL' + sfx].T + dv[..., Cd:] @ P['LC_GATE' + sfx].T
    return dlc


def dmel_ref(arch, P, cache, dlogits):
    """(dmel [B, T/hop, n_lc_in] in P's precision, G): the gradient of the loss whose dlogits these are
    with respect to the mel input, and every parameter gradient of the same backward (l2 0)."""
    G = R.backward(arch, P, cache, dlogits, 0.0, intermediates=True)
    return R.lc_upsample_bwd(arch, P, cache['lc_acts'], dlc_from_cache(arch, P, cache), {}), G


def hop_of(arch):
    return int(np.prod(arch['lc_upsample']))


def tail_mask(ids, hop):
    """Stream 0 scores nothing from position T - 2·hop - 5 on (in place; returns ids).  Where the slice
    is not longer than that (two frames or fewer per stream: hop 256 and 512 at T = 512) the position is
    negative and the whole of stream 0 is masked: the other streams carry the gradient."""
    T = ids.shape[1]
    ids[0, max(T - 2 * hop - 5, 0):] = 0
    return ids


def last_scored_frame(ids, hop):
    """Per stream, the mel frame that holds its last scored position (position t is scored iff
    ids[b][t+1] != 0), or -1 when the stream scores nothing: every later frame lies wholly after it."""
    out = []
    for row in np.asarray(ids):
        t = np.flatnonzero(row[1:] != 0)
        out.append(int(t[-1]) // hop if t.size else -1)
    return out


def check_zero_frames(dmel, ids, hop, name=''):
    """The exact-zero rule on a dmel [B, frames, Li] (any precision): the frames wholly after a stream's
    last scored position are exactly zero, the frame that holds it is not.  Returns the number of
    frames held to exact zero."""
    dmel, n = np.asarray(dmel), 0
    for b, f in enumerate(last_scored_frame(ids, hop)):
        tail = dmel[b, f + 1:]
        assert not np.any(tail != 0), '%s: stream %d: %d non-zero elements in the frames after frame %d' % (
            name, b, int(np.count_nonzero(tail)), f)
        n += tail.shape[0]
        if f >= 0:
            assert np.any(dmel[b, f] != 0), '%s: stream %d: frame %d holds a scored position and is all zero' % (
                name, b, f)
    return n


# ---- kernel ----------------------------------------------------------------------------------------

def kernel_dmel_ref(Li, Lo, strides, frames, F, dlc, drop=None):
    """(dmel [frames][Li] float64, bound): the din chain of oracle lc_upsample_bwd on the partials dlc
    [parts][>= frames·hop·Lo] and
        bound = gamma_K · (|D|·|F_{nup-1}|···|F_0|),  K = (parts - 1) + Σ_k 2·s_k·Lo,
    |D| the sum of the partials' absolute values: the forward error bound of the whole chain of sums,
    two operations per term, whatever their order.  drop: a mutant for the CPU proof, never a tolerance:
    'phase' leaves stage 0's last phase j = s_0 - 1 out, 'part' the last split-K partial."""
    hop, shp, parts = int(np.prod(strides)), stage_shapes(Li, Lo, strides), dlc.shape[0]
    d64 = dlc.astype(np.float64)[:, :frames * hop * Lo]
    D = d64[:parts - 1 if drop == 'part' else parts].sum(axis=0)
    A = np.abs(d64).sum(axis=0)
    K = parts - 1
    for i in reversed(range(len(strides))):
        s, I, Rr = shp[i]
        F64 = F[i].astype(np.float64)
        Fd = F64
        if drop == 'phase' and i == 0:
            Fd = F64.copy()
            Fd[s - 1] = 0.0
        D = np.einsum('btjo,joi->bti', D.reshape(frames, Rr, s, Lo), Fd)
        A = np.einsum('btjo,joi->bti', A.reshape(frames, Rr, s, Lo), np.abs(F64))
        K += 2 * s * Lo
    return D.reshape(frames, Li), gamma(K) * A.reshape(frames, Li)


def check_kernel_dmel(name, got, ref, bound):
    """|got - ref| <= bound element by element; prints and returns the worst err / bound."""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    assert np.all(np.isfinite(err)), 'dmel %s: not finite (an element was not written?)' % name
    ratio = float(np.max(err / bound))
    print('dmel kernel    %-40s worst err / bound %.3g' % (name, ratio))
    assert np.all(err <= bound), 'dmel %s: err / bound %.3f at %s' % (
        name, ratio, np.unravel_index(np.argmax(err / bound), err.shape))
    return ratio
