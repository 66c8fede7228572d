"""Masked-position skip of the backward head and skip GEMMs (bf16-split path): the step prologue
forms the live lists of the step's ids (tlive / klive / nklive plan tensors), dH1 / dS / dZ run no
k-step on 256-row tiles without a valid row, and dPOST2 / dPOST1 / dSKIP walk the live 32-row
k-steps only, inside unchanged split-K slices.  LBWN_SKIP_MASKED=0 (plan creation) is the
unskipped path every case is compared to, from the same weights and inputs.

Shapes: arch3 B=2 T=4096 (M = 8192: the smallest M at which dZ takes its 160-column 256-row form
and dH1 / dS / dSKIP / dPOST1 the forms the benchmark runs) and B=3 T=1000 (M = 3000: no multiple
of 32 or 256, tiles straddle streams, the fallback forms launch: the skip is off or right)."""
import numpy as np
import pytest
import torch

from tests.gradcheck import grad_close
from tests.test_gpu_parity import arch3, make_net

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4096), (3, 1000)]


def make_ids(pattern, B, T):
    ids = np.ones((B, T), np.int32)
    if pattern == 'all_valid':
        pass
    elif pattern == 'all_zero':
        ids[:] = 0
    elif pattern == 'dealer':       # stream 0 masked on [0, 1019), stream 1 on the whole slice
        ids[0, :1019] = 0
        ids[1, :] = 0
    elif pattern == 'lone_rows':    # one valid row in an otherwise dead tile, one invalid row in a live one
        ids[0, :T // 2] = 0
        ids[0, T // 6] = 1
        ids[1, 300] = 0
    elif pattern == 'single':       # one valid row in the whole batch
        ids[:] = 0
        ids[B - 1, T // 2 + 5] = 1
    else:
        raise ValueError(pattern)
    return ids


def live_ref(ids):
    """The head's validity rule (row m = (b, t) valid iff t < T-1 and ids[min(m+1, M-1)] != 0) and
    the lists over it."""
    B, T = ids.shape
    M = B * T
    flat = ids.reshape(-1)
    m = np.arange(M)
    valid = (m % T != T - 1) & (flat[np.minimum(m + 1, M - 1)] != 0)

    def groups(n):
        pad = np.zeros((M + n - 1) // n * n, bool)
        pad[:M] = valid
        return pad.reshape(-1, n).any(axis=1)
    return valid, groups(256).astype(np.int32), np.nonzero(groups(32))[0].astype(np.int32)


def run(monkeypatch, skip, B, T, q, ids, arch=None, poison_grads=False):
    monkeypatch.setenv('LBWN_SKIP_MASKED', skip)
    net = make_net(arch or arch3(), B)
    if poison_grads:   # "every pointer of the struct is fully overwritten" (include/lbwn.h)
        net.grad_flat.fill_(float('nan'))
    net.forward(q, None, ids, backward=True)
    torch.cuda.synchronize()
    out = dict(status=int(net.plan_tensor(T, 'status').view(torch.int32)[0]),
               stats=net.stats[:3].clone(), save=net.save_flat.clone(),
               grads={n: g.clone() for n, g in net.grads.items()},
               **{n: net.plan_tensor(T, n).clone() for n in ('dh', 'ds', 'dz')})
    if skip == '1':
        nk = int(net.plan_tensor(T, 'nklive').view(torch.int32)[0])
        out['nklive'] = nk
        out['klive'] = net.plan_tensor(T, 'klive').view(torch.int32)[:nk].cpu().numpy()
        out['tlive'] = net.plan_tensor(T, 'tlive').view(torch.int32).cpu().numpy()
        out['kpre'] = net.plan_tensor(T, 'kpre').view(torch.int32).cpu().numpy()
    return out


def is_head_weight(name):
    return 'BIAS' not in name and (name.startswith('SKIP') or name in ('POST1', 'POST2'))


@pytest.mark.parametrize('B,T', SHAPES)
@pytest.mark.parametrize('pattern', ['all_valid', 'all_zero', 'dealer', 'lone_rows', 'single'])
def test_masked_skip(monkeypatch, pattern, B, T):
    check_masked_skip(monkeypatch, pattern, B, T)


def check_masked_skip(monkeypatch, pattern, B, T, arch=None, poison_grads=False):
    """arch: another arch than arch3 (tests/test_gpu_no_bias.py); poison_grads: NaN in every gradient
    before each backward."""
    arch = arch or arch3()
    rng = np.random.default_rng(5)
    q = rng.integers(0, arch['n_quant'], size=(B, T)).astype(np.int32)
    ids = make_ids(pattern, B, T)
    valid, tlive, klive = live_ref(ids)
    M = B * T

    on = run(monkeypatch, '1', B, T, q, ids, arch, poison_grads)
    on2 = run(monkeypatch, '1', B, T, q, ids, arch, poison_grads)
    off = run(monkeypatch, '0', B, T, q, ids, arch, poison_grads)
    assert on['status'] == 0 and on2['status'] == 0 and off['status'] == 0
    assert any(is_head_weight(n) for n in on['grads'])

    # the lists are the numpy restatement of the rule
    assert on['nklive'] == len(klive), (on['nklive'], len(klive))
    assert np.array_equal(on['klive'], klive)
    assert np.array_equal(on['tlive'], tlive)
    nk = (M + 31) // 32
    assert np.array_equal(on['kpre'], np.searchsorted(klive, np.arange(nk + 1)))   # entries below k-step k
    assert float(on['stats'][1]) == float(valid.sum())

    # the compaction is deterministic: two skipped runs agree bit for bit
    for n in ('stats', 'save', 'dh', 'ds', 'dz'):
        assert np.array_equal(on[n].cpu().numpy().view(np.int32), on2[n].cpu().numpy().view(np.int32)), n
    for n, g in on['grads'].items():
        assert np.array_equal(g.cpu().numpy().view(np.int32), on2['grads'][n].cpu().numpy().view(np.int32)), n

    assert torch.equal(on['stats'], off['stats']) and torch.equal(on['save'], off['save'])

    if pattern == 'all_valid':
        # the identity list and the same slices: every value bit for bit
        for n in ('dh', 'ds', 'dz'):
            assert np.array_equal(on[n].cpu().numpy().view(np.int32), off[n].cpu().numpy().view(np.int32)), n
        for n, g in on['grads'].items():
            assert np.array_equal(g.cpu().numpy().view(np.int32), off['grads'][n].cpu().numpy().view(np.int32)), n
        return
    if pattern == 'all_zero':
        assert float(on['stats'][1]) == 0.0 and on['nklive'] == 0
        for r in (on, off):
            for n, g in r['grads'].items():
                assert not bool(g.count_nonzero()), n
        return

    # dH1 / dS: the unskipped run's values (a +-0 difference is none)
    assert torch.equal(on['dh'], off['dh'])
    assert torch.equal(on['ds'], off['ds'])
    # dZ: dead tiles all zero, live tiles bit for bit
    dz_on, dz_off = on['dz'].cpu().numpy(), off['dz'].cpu().numpy()
    if M % 256 == 0:
        # chain order: 32-column block j, then 32-row blocks of 1024 floats: a 256-row tile is
        # 8192 consecutive floats of each column block
        t_on = dz_on.reshape(-1, M // 256, 8192)
        t_off = dz_off.reshape(-1, M // 256, 8192)
        dead = tlive == 0
        assert not t_on[:, dead].any()
        assert np.array_equal(t_on[:, ~dead].view(np.int32), t_off[:, ~dead].view(np.int32))
    # (rows past M of the last 32-row block are never written)
    m32 = (M + 31) // 32 * 32
    within = np.arange(dz_on.size) % (m32 * 32)
    written = (within // 1024) * 32 + (within // 8) % 32 < M
    assert np.array_equal(dz_on[written], dz_off[written])

    nv = max(float(valid.sum()), 1.0)
    for n, g in on['grads'].items():
        if is_head_weight(n):
            # the unskipped run is the oracle-verified path; the two differ in f32 summation order
            # only: the project's gradient bar (tests/gradcheck.py: 2e-4 of the tensor's own max)
            grad_close(g.double().cpu().numpy() / nv, off['grads'][n].double().cpu().numpy() / nv, n)
            # ... and, the slices keeping their k ranges, the skipped terms are exact zeros of the
            # same sums: no reordering at all
            assert torch.equal(g, off['grads'][n]), n
        else:
            assert torch.equal(g, off['grads'][n]), n
