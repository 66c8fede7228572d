"""lbwn_train_eval on the GPU against the float64 reference of tests/eval_ref.py, against
lbwn_train_forward on the same inputs, and through WaveNetTrain.evaluate and train.py.

Bars: the per-position value within 2e-4 of float64 (twice the project's logit tolerance of 1e-4:
nll = lse - l_c moves by at most twice the largest logit error); against the plan's own fp32 logits
within Q·2^-24 + 4e-6 (the fp32 sum of Q exponentials, a few ulps of expf / logf, two ulps of an lse
below 16); acc[0] against the returned values at 1e-12 relative (both are sums of the same fp32 values
in double); counts exact; the argmax totals exact on rows whose float64 top-2 gap exceeds 1e-3 (none
excluded on the base chain case, at most 5 % elsewhere: tests/test_eval.py::test_top2_gap_shares)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.optim import AdamOptimizer
from lbwn.tmodel import WaveNetTrain
from tests import eval_ref as E
from tests.conftest import ROOT
from tests.test_gpu_parity import gemm_mode  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NB = E.N_BINS


def make_net(arch, P, B):
    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=1e-3, print_interval=0)
    load_params(net, net.flat, P)
    return net


def load_params(net, flat, P):
    with torch.no_grad():
        for n, v in net.layout.views(flat).items():
            v.copy_(torch.as_tensor(P[n], dtype=torch.float32))


def load_save(net, flat, S):
    with torch.no_grad():
        for n, (o, s) in net.save_index.items():
            flat[o:o + int(np.prod(s))].view(*s).copy_(torch.as_tensor(S[n], dtype=torch.float32))


def save_dict(net, flat):
    return {n: flat[o:o + int(np.prod(s))].view(*s).cpu().double().numpy() for n, (o, s) in net.save_index.items()}


def new_state(net, S, n_bins=NB):
    st = net.eval_state(n_bins)
    load_save(net, st['save'], S)
    return st


def run_slices(net, st, slices, flat=None):
    """eval_slice over the slices with the per-position values kept; returns them as float64 [B, T]."""
    outs = []
    for q, ids, mel in slices:
        out = torch.full((q.shape[0], q.shape[1] + 3), -7.0, dtype=torch.float32, device=DEV)
        net.eval_slice(st, q, mel, ids, flat=flat, nll=out)
        outs.append(out)
    torch.cuda.synchronize()
    assert int(st['status'].item()) == 0
    for o in outs:
        assert torch.all(o[:, -3:] == -7.0)                      # columns past T are not touched
    return [o[:, :-3].cpu().double().numpy() for o in outs]


def check_against_reference(net, st, slices, ref):
    """Checks 1 and 2 on a fresh state; returns the values, acc and by_voice."""
    nll = run_slices(net, st, slices)
    acc = st['acc'].cpu().numpy()
    bv = st['by_voice'].cpu().numpy()
    worst = got_sum = 0.0
    for got, s in zip(nll, ref):
        err = float(np.max(np.abs(got - s['nll'])))
        worst = max(worst, err)
        assert err <= 2e-4, err                                   # 1
        assert np.all(got[~s['scored']] == 0.0)
        got_sum += got.sum()
    print('nll max |err| vs float64: %.3g' % worst)
    np.testing.assert_allclose(acc[0], got_sum, rtol=1e-12)       # 2
    assert acc[1] == sum(s['acc'][1] for s in ref)
    return nll, acc, bv


def argmax_totals(net, T, s, q):
    """acc[2], acc[3] the kernel must give for the rows of ``s`` whose top-2 gap exceeds 1e-3, from the
    reference, plus what the plan's own logits say for the excluded rows (they may go either way)."""
    keep = s['scored'] & (s['gap'] > 1e-3)
    excl = s['scored'] & ~keep
    share = excl.sum() / max(1, s['scored'].sum())
    assert share <= 0.05, share
    lg = net.plan_tensor(T, 'logits').view(q.shape[0], T, -1).cpu().double().numpy()
    own = E.score(lg, q, _shift(excl))
    d = np.abs(s['tgt'] - s['argmax'])[keep].sum() + own['acc'][2]
    h = (s['tgt'] == s['argmax'])[keep].sum() + own['acc'][3]
    return float(d), float(h), float(share)


def _shift(rows):
    """ids that score exactly ``rows``: ids[:, t+1] != 0 iff rows[:, t]."""
    ids = np.zeros(rows.shape, np.int32)
    ids[:, 1:] = rows[:, :-1]
    return ids


# ---- 1-3, 7: values, accumulators and by_voice against float64 --------------------------------------
@pytest.mark.parametrize('name', ['chain', 'per_layer', 'cond', 'no_bias', 'chain_f32'])
def test_eval_matches_float64(lib, gemm_mode, name):
    """Base shape B = 2, T = 64, n_quant 256 on the four configurations, and the chain arch under the
    f32-MFMA GEMMs.  Rows excluded from the argmax totals: chain 0, per_layer 1.1 %, cond 0, no_bias 4.3 %."""
    if name == 'chain_f32':
        gemm_mode(0)
        name = 'chain'
    arch, P, S, slices = E.case(name)
    (s,), _ = E.run(arch, P, slices, S, NB)
    net = make_net(arch, P, 2)
    st = new_state(net, S)
    (nll,), acc, bv = check_against_reference(net, st, slices, [s])
    q, ids, _ = slices[0]
    d, h, share = argmax_totals(net, 64, s, q)                    # 3
    if name == 'chain':
        assert share == 0.0 and d == s['acc'][2] and h == s['acc'][3]
    assert acc[2] == d and acc[3] == h, (acc, d, h)
    # 7: by_voice is np.add.at over the returned values; ids >= n_bins land in bin 0
    want = np.zeros((NB, 2))
    vid = _voice(ids)
    np.add.at(want[:, 0], vid[s['scored']], nll[s['scored']])
    np.add.at(want[:, 1], vid[s['scored']], 1.0)
    np.testing.assert_allclose(bv[:, 0], want[:, 0], rtol=1e-9)
    assert np.array_equal(bv[:, 1], want[:, 1]) and want[0, 1] == np.sum(ids[:, 1:] >= NB) > 0
    np.testing.assert_allclose(bv.sum(axis=0), acc[:2], rtol=1e-12)
    np.testing.assert_allclose(bv, s['by_voice'], rtol=0, atol=2e-4 * max(1.0, s['by_voice'][:, 1].max()))


def _voice(ids):
    vid = np.zeros(ids.shape, np.int64)
    vid[:, :-1] = ids[:, 1:]
    return np.where(vid < NB, vid, 0)


# ---- the row kernel alone: widths and row counts ----------------------------------------------------
@pytest.mark.parametrize('name,B,T,invalid', [('q64', 2, 16, 3), ('q260', 2, 16, 3), ('q1028', 2, 16, 3),
                                              ('chain', 1, 5, 1), ('chain', 2, 2, 1)])
def test_row_kernel_widths_and_row_counts(lib, name, B, T, invalid):
    """n_quant 64 (one 64-column group), 260 (a partial last group of the <= 512 register form), 1028
    (the generic form: n_quant > 512); M = 5 (not a multiple of the block's 4 waves) and T = 2 (one
    target per stream).  Against the plan's own fp32 logits: the value within Q·2^-24 + 4e-6, the argmax
    and every total exact (the same fp32 rows, first maximum)."""
    arch, P, S, slices = E.case(name, B=B, T=T, invalid=invalid)
    (s,), _ = E.run(arch, P, slices, S, NB)
    net = make_net(arch, P, B)
    st = new_state(net, S)
    (nll,), acc, bv = check_against_reference(net, st, slices, [s])
    q, ids, _ = slices[0]
    Q = arch['n_quant']
    own = E.score(net.plan_tensor(T, 'logits').view(B, T, Q).cpu().double().numpy(), q, ids, NB)
    err = float(np.max(np.abs(nll - own['nll'])))
    print('nll max |err| vs own logits: %.3g' % err)
    assert err <= Q * 2.0 ** -24 + 4e-6
    assert np.array_equal(acc[1:], own['acc'][1:])
    assert np.array_equal(bv[:, 1], own['by_voice'][:, 1])
    assert acc[2] == s['acc'][2] and acc[3] == s['acc'][3]       # every gap of these cases exceeds 1e-3


def test_all_masked_slice_adds_nothing(lib):
    arch, P, S, slices = E.case('chain')
    net = make_net(arch, P, 2)
    st = new_state(net, S)
    st['acc'].copy_(torch.tensor([1.25, 3.0, 5.0, 1.0], dtype=torch.float64))
    st['by_voice'].fill_(0.5)
    q, ids, mel = slices[0]
    (nll,) = run_slices(net, st, [(q, np.zeros_like(ids), mel)])
    assert np.all(nll == 0.0)
    assert st['acc'].tolist() == [1.25, 3.0, 5.0, 1.0] and torch.all(st['by_voice'] == 0.5)


def test_by_voice_without_nll_reads_the_scratch_rows(lib):
    """Without an nll buffer the row values go to the scratch's third part and the voice pass reads them
    back from there (leading dimension T): by_voice and acc are the bits of the call with nll, over two
    chained slices."""
    arch, P, S, slices = E.case('chain', n_slices=2)
    net = make_net(arch, P, 2)
    st = new_state(net, S)
    run_slices(net, st, slices)
    bare = new_state(net, S)
    for q, ids, mel in slices:
        net.eval_slice(bare, q, mel, ids)
    torch.cuda.synchronize()
    assert int(bare['status'].item()) == 0 and float(st['by_voice'][:, 1].sum()) > 0
    assert torch.equal(bare['by_voice'].view(torch.int64), st['by_voice'].view(torch.int64))
    assert torch.equal(bare['acc'].view(torch.int64), st['acc'].view(torch.int64))


# ---- 4: against lbwn_train_forward ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chain', 'per_layer', 'cond'])
def test_eval_equals_train_forward(lib, name):
    arch, P, S, slices = E.case(name)
    q, ids, mel = slices[0]
    net = make_net(arch, P, 2)
    load_save(net, net.save_flat, S)
    net.forward(q, mel, ids, backward=False)
    torch.cuda.synchronize()
    stats = net.stats.cpu().numpy().copy()
    st = new_state(net, S)
    net.eval_slice(st, q, mel, ids)
    torch.cuda.synchronize()
    acc = st['acc'].cpu().numpy()
    assert acc[1] == stats[1] and acc[2] == stats[2]
    np.testing.assert_allclose(acc[0], stats[0], rtol=1e-5)
    assert torch.equal(st['save'].view(torch.int32), net.save_flat.view(torch.int32))
    # the raw logits the evaluation left, through the training head, give the training stats
    lg = net.plan_tensor(64, 'logits').clone()
    out = torch.zeros(4, device=DEV)
    ws = torch.zeros(3 * 2048, device=DEV)
    qd, idd = torch.tensor(q, device=DEV), torch.tensor(ids, device=DEV)
    _lib.check(lib.lbwn_head_xent(lg.data_ptr(), qd.data_ptr(), idd.data_ptr(), 2, 64, arch['n_quant'], 0,
                                  out.data_ptr(), ws.data_ptr(), None))
    out = out.cpu().numpy()
    assert out[1] == stats[1] and out[2] == stats[2]
    np.testing.assert_allclose(out[0], stats[0], rtol=1e-6)


# ---- 5, 6: chaining, accumulation, determinism ------------------------------------------------------
@pytest.mark.parametrize('name', ['chain', 'cond'])
def test_two_slices_chain_accumulate_and_repeat_bitwise(lib, name):
    arch, P, S, slices = E.case(name, n_slices=2)
    ref, ref_save = E.run(arch, P, slices, S, NB)
    net = make_net(arch, P, 2)
    st = new_state(net, S)
    _, acc, bv = check_against_reference(net, st, slices, ref)
    want_acc, want_bv = E.totals(ref)
    assert np.array_equal(acc[1:], want_acc[1:])                 # both slices' gaps exceed 1e-3
    np.testing.assert_allclose(acc[0], want_acc[0], rtol=0, atol=2e-4 * want_acc[1])
    assert np.array_equal(bv[:, 1], want_bv[:, 1])
    for n, v in save_dict(net, st['save']).items():              # SAVE carried over both slices
        np.testing.assert_allclose(v, ref_save[n], rtol=0, atol=1e-5 * max(1.0, np.abs(ref_save[n]).max()))
    # a second pass through the same state ADDS; from an equal state it adds the same bits
    st2 = new_state(net, S)
    run_slices(net, st2, slices)
    assert torch.equal(st2['acc'].view(torch.int64), st['acc'].view(torch.int64))
    assert torch.equal(st2['by_voice'].view(torch.int64), st['by_voice'].view(torch.int64))
    load_save(net, st['save'], S)
    run_slices(net, st, slices)
    assert torch.equal(st['acc'], 2 * st2['acc']) and torch.equal(st['by_voice'], 2 * st2['by_voice'])


# ---- 8: training is not disturbed -------------------------------------------------------------------
def _train_run(arch, P, S, batches, with_eval):
    net = make_net(arch, P, 2)
    load_save(net, net.save_flat, S)
    opt = AdamOptimizer(1e-3)
    st = new_state(net, S) if with_eval else None
    for q, ids, mel in batches:
        net.forward(q, mel, ids, backward=True)
        opt.apply(net)
        if with_eval:
            net.evaluate([(0, q, mel, ids)], state=st)
    torch.cuda.synchronize()
    m, v = opt.slots(net)
    return net, [net.flat, m, v, net.save_flat, net.counters, net.stats]


@pytest.mark.parametrize('name', ['chain', 'per_layer', 'no_bias'])
def test_training_is_not_disturbed(lib, name):
    """Three steps of forward + backward + Adam, alone and with an evaluate after each step: weights,
    Adam slots, SAVE, counters and stats bitwise equal, on every configuration without conditioning.
    The conditioned arch is not in the list because two plain runs of it already differ in the last
    bits (its GC gradient is summed with float atomicAdd), which leaves nothing to compare."""
    arch, P, S, slices = E.case(name, n_slices=3)
    _, a = _train_run(arch, P, S, slices, False)
    _, b = _train_run(arch, P, S, slices, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                 # two plain runs first
    net, c = _train_run(arch, P, S, slices, True)
    for k, (x, y) in enumerate(zip(a, c)):
        assert torch.equal(x, y), k
    assert int(net.counters[0]) == 3


def test_backward_after_eval_is_refused_and_forward_recovers(lib):
    arch, P, S, slices = E.case('chain')
    q, ids, mel = slices[0]
    fresh = make_net(arch, P, 2)
    load_save(fresh, fresh.save_flat, S)
    fresh.forward(q, mel, ids, backward=False)
    net = make_net(arch, P, 2)
    load_save(net, net.save_flat, S)
    net.forward(q, mel, ids, backward=True)                      # a backward is legal here ...
    st = new_state(net, S)
    net.eval_slice(st, q, mel, ids)
    qd, idd = st['keep'][-1][0], st['keep'][-1][1]
    ret = lib.lbwn_train_backward(net._plan(64), ctypes.byref(net._params_c), ctypes.byref(net._grads_c),
                                  net._ws.data_ptr(), qd.data_ptr(), idd.data_ptr(), None, _lib.stream_ptr())
    assert ret == 22 and 'no training forward' in lib.lbwn_last_error().decode()      # ... and not here
    load_save(net, net.save_flat, S)
    net.forward(q, mel, ids, backward=True)
    torch.cuda.synchronize()
    assert torch.equal(net.stats, fresh.stats)


# ---- 9: flat= ---------------------------------------------------------------------------------------
def test_flat_selects_another_parameter_buffer(lib):
    arch, P, S, slices = E.case('chain')
    _, P2, _, _ = E.case('chain', pseed=7)
    (s2,), _ = E.run(arch, P2, slices, S, NB)
    net = make_net(arch, P, 2)
    live = net.flat.clone()
    flat2 = torch.zeros_like(net.flat)
    load_params(net, flat2, P2)
    st = new_state(net, S)
    r = net.evaluate([(0,) + (slices[0][0], slices[0][2], slices[0][1])], state=st, flat=flat2, want_nll=True)
    assert torch.equal(net.flat, live)
    assert r['n'] == s2['acc'][1]
    np.testing.assert_allclose(r['nll'], s2['acc'][0] / s2['acc'][1], rtol=0, atol=2e-4)
    np.testing.assert_allclose(r['bits'], r['nll'] / np.log(2.0), rtol=1e-15)
    assert r['avg_diff'] == s2['acc'][2] / s2['acc'][1] and r['top1'] == s2['acc'][3] / s2['acc'][1]
    np.testing.assert_allclose(r['nll_rows'][0].cpu().double().numpy(), s2['nll'], rtol=0, atol=2e-4)
    assert np.array_equal(r['by_voice'][:, 1], s2['by_voice'][:, 1])
    (s1,), _ = E.run(arch, P, slices, S)
    assert abs(s1['acc'][0] - s2['acc'][0]) > 1.0                 # the two buffers do score differently


# ---- 10: train.py end to end ------------------------------------------------------------------------
def _dataset(tmp_path, tag, n_files, seed):
    from lbwn.ops import mu_encode_np
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n_files):
        n = int(rng.integers(600, 1400))
        t = np.arange(n) / 16000.0
        x = 0.8 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + rng.normal(0, 0.05, n)
        wav = mu_encode_np(np.clip(x, -1, 1), 256).astype(np.int32)
        wp, mp = tmp_path / ('%s_w%d.npy' % (tag, i)), tmp_path / ('%s_m%d.npy' % (tag, i))
        np.save(wp, wav)
        np.save(mp, np.zeros((n, 0), np.float32))
        lines.append('%d\t%s\t%s' % (i % 3 + 1, wp, mp))
    cat = tmp_path / ('%s.txt' % tag)
    cat.write_text('\n'.join(lines) + '\n')
    return str(cat)


def test_train_py_valid_file_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import train
    from lbwn.data import eval_batches
    arch = dict(n_blocks=1, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
                n_gc_embed=8, n_gc_category=3, n_lc_in=0, n_lc_out=0, lc_upsample=[], use_bias=True,
                wav_input_type='mu_law_quant')
    par = dict(batch_sz=2, sample_rate=16000, slice_sz=128, l2_factor=1e-3, learning_rate=1e-3, prefetch_sz=4,
               add_summary=False, n_keep_checkpoints=3, n_valid_total=100000)
    af, pf = tmp_path / 'arch.json', tmp_path / 'par.json'
    af.write_text(json.dumps(arch))
    pf.write_text(json.dumps(par))
    cat, vcat = _dataset(tmp_path, 'train', 6, 0), _dataset(tmp_path, 'valid', 3, 1)
    pfx = str(tmp_path / 'ck' / 'run')
    common = ['--valid-file', vcat, '--ema-decay', '0.9', '--valid-ema', '--seed', '1']
    train.main(['--max-steps', '10', '--save-interval', '4', '--valid-interval', '4', '--progress-interval', '0']
               + common + [pfx, str(af), str(pf), cat])
    err = capsys.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith('valid')]
    assert [(l.split('\t')[0], l.split('\t')[1]) for l in lines] == [('valid', '4'), ('valid_ema', '4'),
                                                                      ('valid', '8'), ('valid_ema', '8')]
    assert open(pfx + '.valid.tsv').read().splitlines() == lines
    for l in lines:
        f = l.split('\t')
        assert len(f) == 7 and all(np.isfinite(float(x)) for x in f[1:]) and int(f[6]) > 0
    # --eval-only on the saved step: twice the same lines, those of a direct evaluate
    outs = []
    for _ in range(2):
        net = train.main(['--eval-only', '--resume-step', '8'] + common + [pfx, str(af), str(pf), cat])
        outs.append([l for l in capsys.readouterr().err.splitlines() if l.startswith('valid')])
    assert outs[0] == outs[1] and len(outs[0]) == 2
    assert outs[0][0].split('\t')[2:] == lines[2].split('\t')[2:]          # the step-8 weights, bit for bit
    r = net.evaluate(eval_batches(train.valid_files(vcat, False), 2, 128, net.get_recep_field_sz()))
    assert outs[0][0] == 'valid\t8\t%.6f\t%.6f\t%.6f\t%.4f\t%d' % (r['nll'], r['bits'], r['top1'], r['avg_diff'], r['n'])
    assert int(net.counters[0]) == 8                                       # no training step was taken
