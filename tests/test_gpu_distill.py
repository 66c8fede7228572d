"""The distilling / label-smoothing head on the GPU (lbwn_train_forward_ex):
(a) the kernel alone through lbwn_head_xent_ex against float64, (b) the neutral path bitwise against
lbwn_train_forward, (c) the whole step against the float64 oracle, (d) lbwn.distill.Distiller over two
consecutive slices.

Yardstick of (a) and (d): tests/distill_ref.py's float32 twin on the same input.  The kernel's maximum
absolute dlogits error against float64 may reach 8x the twin's (the margin tests/test_gpu_mel.py gives a
kernel over its numpy twin: another summation order and expf), and so may the errors of stats[0],
stats_ex[0] and stats_ex[1], the twin's error on a sum being its largest over three float32 summation
orders (distill_ref.twin says why); counts and the argmax sum are exact.  Gradients of (c): the project's
2e-4 of each tensor's own max (tests/gradcheck.py).  Every figure is printed before it is asserted
(run with -s); the measured ones are in profiles/r18_distill.md."""
import ctypes

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.distill import Distiller
from oracle import wavenet_ref as R
from tests import distill_ref as D
from tests import eval_ref as E
from tests.dmel_ref import dmel_ref
from tests.gradcheck import GRAD_REL, adopt_relu_signs, adoption_capped, grad_close
from tests.test_gpu_eval import load_save, make_net

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 8.0
QS = [8, 252, 256, 260, 512, 516, 1024]
OPTS = [(0.0, 1.0, 0.1), (0.5, 1.0, 0.0), (0.5, 2.0, 0.1), (1.0, 0.5, 0.0), (1.0, 2.0, 0.0)]

_refs = {}


def kernel_reference(Q, opt):
    """(inputs, float64 head, float32 twin) of a kernel case; computed once, shared, never written to."""
    if (Q, opt) not in _refs:
        inp = D.kernel_case(Q)
        lg, te, q, ids = inp
        _refs[Q, opt] = (inp, D.head(lg, te, q, ids, *opt), D.twin(lg, te, q, ids, *opt))
    return _refs[Q, opt]


def held_to_twin(name, got, ref, twin, scalar=False):
    """|got - ref| <= 8 |twin - ref| on maxima; prints the figures first.  Returns the ratio.
    scalar: ``got`` is one float32 number the kernel returns (a sum of ~13 row values).  Its rounding to
    float32 alone is up to half an ulp, while a twin's single sum lands by accident anywhere inside
    that half ulp (0.016 ulp on stats_ex[0] of the Q = 260 case): no float32 result can be held to 8x an
    error below its own format's rounding, so the twin's error on a scalar counts as no less than
    half a float32 ulp of the value."""
    e_k = float(np.max(np.abs(np.asarray(got, np.float64) - ref)))
    e_t = float(np.max(np.abs(np.asarray(twin, np.float64) - ref)))
    if scalar:
        e_t = max(e_t, 0.5 * float(np.spacing(np.float32(abs(ref)))))
    own = float(np.max(np.abs(ref)))
    print('%-44s kernel %.3e  twin %.3e  ratio %.2f  (own magnitude %.3e)' % (name, e_k, e_t, e_k / e_t if e_t else
                                                                              float('inf') if e_k else 0.0, own))
    assert e_k <= MARGIN * e_t, '%s: kernel err %.3e > 8 x twin err %.3e (own magnitude %.3e)' % (name, e_k, e_t, own)
    return e_k / e_t if e_t else 0.0


def run_head_ex(lib, lg, te, q, ids, opt, ld_pad=4):
    """lbwn_head_xent_ex on device copies; the teacher at ld = Q + ld_pad with NaN in the pad columns and
    in every row that may not be read (unscored, t = T-1).  Returns dlogits [B,T,Q], stats, stats_ex."""
    B, T, Q = lg.shape
    scored = np.zeros((B, T), bool)
    scored[:, :-1] = ids[:, 1:] != 0
    tp = np.full((B * T, Q + ld_pad), np.nan, np.float32)
    tp[scored.reshape(-1), :Q] = te.reshape(B * T, Q)[scored.reshape(-1)]
    lgd, ted = torch.tensor(lg, device=DEV), torch.tensor(tp, device=DEV)
    qd, idd = torch.tensor(q, device=DEV), torch.tensor(ids, device=DEV)
    stats = torch.full((4,), float('nan'), device=DEV)
    ex = torch.full((4,), float('nan'), device=DEV)
    ws = torch.zeros(5 * 2048, device=DEV)
    _lib.check(lib.lbwn_head_xent_ex(lgd.data_ptr(), qd.data_ptr(), idd.data_ptr(), B, T, Q, ted.data_ptr(), Q + ld_pad,
                                     opt[0], opt[1], opt[2], stats.data_ptr(), ex.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    return lgd.cpu().numpy(), stats.cpu().numpy(), ex.cpu().numpy(), scored


# ---- (a) the kernel alone -------------------------------------------------------------------------------
@pytest.mark.parametrize('opt', OPTS, ids=lambda o: 'a%g_t%g_e%g' % o)
@pytest.mark.parametrize('Q', QS)
def test_head_kernel_against_float64(lib, Q, opt):
    """B = 2, T = 9 (M = 18: the last block has idle waves, both t = T-1 rows present), a masked run in
    ids, targets 0 and Q-1, ld_teacher = Q + 4, logits N(0, 3²), one teacher logit 200 below its row's
    maximum.  Q: a row narrower than a wave; a partial last 64-column group in the QV = 4 and QV = 8
    register forms; both full; the generic form just past 512 and at the backward's limit."""
    (lg, te, q, ids), ref, tw = kernel_reference(Q, opt)
    dl, stats, ex, scored = run_head_ex(lib, lg, te, q, ids, opt)
    tag = 'Q=%d a=%g t=%g e=%g ' % ((Q,) + opt)
    assert np.isfinite(dl).all() and np.isfinite(stats).all() and np.isfinite(ex).all(), tag + 'NaN / Inf'
    assert np.all(dl[~scored] == 0.0) and not scored[:, -1].any() and (~scored[:, :-1]).any()
    held_to_twin(tag + 'dlogits', dl, ref[1], tw[1])
    held_to_twin(tag + 'stats[0]', stats[0], ref[2][0], tw[4]['stats0'], scalar=True)
    held_to_twin(tag + 'stats_ex[0]', ex[0], ref[3][0], tw[4]['ex0'], scalar=True)
    if opt[0] > 0:
        held_to_twin(tag + 'stats_ex[1]', ex[1], ref[3][1], tw[4]['ex1'], scalar=True)
    else:
        assert ex[1] == 0.0
    assert stats[1] == ref[2][1] == scored.sum() and ex[2] == 0.0 and ex[3] == 0.0
    assert stats[3] == np.float32(1.0 / ref[2][1])
    # the same argmax as the plain head on the same logits: bitwise, ties or not
    B, T = q.shape
    lgd, qd, idd = torch.tensor(lg, device=DEV), torch.tensor(q, device=DEV), torch.tensor(ids, device=DEV)
    plain = torch.zeros(4, device=DEV)
    ws = torch.zeros(3 * 2048, device=DEV)
    _lib.check(lib.lbwn_head_xent(lgd.data_ptr(), qd.data_ptr(), idd.data_ptr(), B, T, Q, 1, plain.data_ptr(),
                                  ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert plain.cpu().numpy().view(np.int32)[2] == stats.view(np.int32)[2] and stats[2] == ref[2][2]
    # two calls, the same bits
    dl2, stats2, ex2, _ = run_head_ex(lib, lg, te, q, ids, opt)
    assert np.array_equal(dl.view(np.int32), dl2.view(np.int32))
    assert np.array_equal(stats.view(np.int32), stats2.view(np.int32)) and np.array_equal(ex.view(np.int32), ex2.view(np.int32))


def test_head_kernel_reads_no_teacher_with_alpha_zero(lib):
    """alpha = 0 (label smoothing alone): a NULL teacher and an all-NaN teacher give the same bits."""
    (lg, te, q, ids), ref, tw = kernel_reference(260, OPTS[0])
    a = run_head_ex(lib, lg, np.full_like(te, np.nan), q, ids, OPTS[0])
    B, T, Q = lg.shape
    lgd, qd, idd = torch.tensor(lg, device=DEV), torch.tensor(q, device=DEV), torch.tensor(ids, device=DEV)
    stats, ex, ws = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(5 * 2048, device=DEV)
    _lib.check(lib.lbwn_head_xent_ex(lgd.data_ptr(), qd.data_ptr(), idd.data_ptr(), B, T, Q, None, 0, 0.0, 1.0, 0.1,
                                     stats.data_ptr(), ex.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(lgd.cpu().numpy().view(np.int32), a[0].view(np.int32))
    assert np.array_equal(stats.cpu().numpy().view(np.int32), a[1].view(np.int32))
    assert np.isfinite(a[0]).all()


# ---- (b) the neutral path -------------------------------------------------------------------------------
def _bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.parametrize('name', ['chain', 'per_layer', 'cond'])
def test_neutral_forward_ex_is_train_forward_bitwise(lib, name):
    """No teacher, alpha = 0, eps = 0 (tau = 3: without effect), then the backward: stats, "logits" and
    grad_flat are bitwise lbwn_train_forward's, with stats_ex NULL and with stats_ex given (then
    stats_ex = (stats[0], 0, 0, 0)); lbwn_plan_workspace_bytes is what the carve-up always gave: the two
    further partials per block live in "dh"."""
    arch, P, S, slices = E.case(name)
    q, ids, mel = slices[0]
    T = 64
    net = make_net(arch, P, 2)
    gc = [n for n in net.layout.names() if n.startswith('GC_')]

    def run(ex_call, stats_ex=None):
        load_save(net, net.save_flat, S)
        net.grad_flat.fill_(float('nan'))
        net.stats.fill_(float('nan'))
        if not ex_call:
            net.forward(q, mel, ids, backward=True)
        else:
            qd, idd = torch.tensor(q, device=DEV), torch.tensor(ids, device=DEV)
            md = torch.tensor(mel, device=DEV) if mel is not None else None
            h = net._plan(T)
            a = _lib.ForwardArgs(wav_q=qd.data_ptr(), ids=idd.data_ptr(), mel=_lib.ptr(md), save=net.save_flat.data_ptr(),
                                 stats=net.stats.data_ptr(), stats_ex=_lib.ptr(stats_ex), teacher_logits=None,
                                 ld_teacher=0, distill_alpha=0.0, distill_temp=3.0, label_smoothing=0.0)
            Pc, G, ws, sp = ctypes.byref(net._params_c), ctypes.byref(net._grads_c), net._ws.data_ptr(), _lib.stream_ptr()
            _lib.check(lib.lbwn_train_forward_ex(h, Pc, ws, ctypes.byref(a), sp))
            _lib.check(lib.lbwn_train_backward(h, Pc, G, ws, qd.data_ptr(), idd.data_ptr(), _lib.ptr(md), sp))
        torch.cuda.synchronize()
        assert int(net.plan_tensor(T, 'status').view(torch.int32)[0]) == 0
        return (_bits(net.stats), _bits(net.plan_tensor(T, 'logits')), _bits(net.save_flat),
                {n: _bits(g) for n, g in net.grads.items()})

    nbytes = net.workspace_bytes(T)
    plain = run(False)
    again = run(False)
    # what two plain steps on the same inputs disagree on (float atomics of mixed-voice GC tiles,
    # tests/test_gpu_dmel_plan.py): nothing else may differ, and those tensors are held to each other instead
    loose = [n for n in net.layout.names() if not torch.equal(plain[3][n], again[3][n])]
    print('%s: two plain steps differ in %s' % (name, loose or 'nothing'))
    assert set(loose) <= set(gc), loose
    ex = torch.full((4,), float('nan'), device=DEV)
    for what, got in (('stats_ex NULL', run(True)), ('stats_ex', run(True, ex))):
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2]), what
        bad = [n for n in net.layout.names() if n not in loose and not torch.equal(got[3][n], plain[3][n])]
        assert not bad, '%s (%s): gradients differ from lbwn_train_forward + backward: %s' % (name, what, bad)
        for n in loose:
            grad_close(got[3][n].view(torch.float32).cpu().double().numpy(),
                       plain[3][n].view(torch.float32).cpu().double().numpy(), n, rel=1e-5)
    torch.cuda.synchronize()
    assert torch.equal(ex[:1].view(torch.int32), plain[0][:1]) and ex[1:].tolist() == [0.0, 0.0, 0.0]
    assert net.workspace_bytes(T) == nbytes == lib.lbwn_plan_workspace_bytes(net._plan(T))
    assert net.stats_ex is None
    off, nb = _lib.c_size_t(), _lib.c_size_t()
    _lib.check(lib.lbwn_plan_tensor(net._plan(T), b'dh', ctypes.byref(off), ctypes.byref(nb)))
    assert nb.value >= 4 * 2 * ((2 * T + 3) // 4)


# ---- (c) the whole step against float64 ---------------------------------------------------------------------
STEP_CASES = [('chain', (0.5, 2.0, 0.1)), ('per_layer', (0.5, 2.0, 0.1)), ('cond', (0.5, 2.0, 0.1)),
              ('no_bias', (0.5, 2.0, 0.1)), ('q260', (0.5, 2.0, 0.1)), ('q516', (1.0, 1.0, 0.0))]


def step_case(name):
    """(arch, P, S, q, ids, mel, teacher logits fp32 [B, T, Q]): eval_ref.case with the parameters and SAVE
    rounded to what the device holds; the teacher is the oracle forward of a second parameter draw."""
    if name == 'q516':
        E.ARCHS.setdefault('q516', D.q516_arch)
    arch, P, S, slices = E.case(name)
    _, Pt, _, _ = E.case(name, pseed=1)
    P, Pt, S = D.f32_params(P), D.f32_params(Pt), D.f32_params(S)
    q, ids, mel = slices[0]
    te, _, _ = R.forward(arch, Pt, q, ids, S, mel=mel)
    return arch, P, S, q, ids, mel, te.astype(np.float32)


@pytest.mark.parametrize('name,opt', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_whole_step_against_float64(lib, name, opt):
    """R.forward -> distill_ref.head -> R.backward(arch, P, cache, dlogits, 0) at B = 2, T = 64: every
    gradient (raw sums, as the reference's dlogits are) within 2e-4 of its own tensor's max, POST2_BIAS
    through the head's column partials at Q <= 512 and through the column-sum pass at 516; dmel on
    'cond'; stats against the reference; two runs, the same bits."""
    arch, P, S, q, ids, mel, te = step_case(name)
    B, T, Q = 2, 64, arch['n_quant']
    M = B * T
    lg, cache, _ = R.forward(arch, P, q, ids, S, mel=mel)
    value, dl, stats, ex = D.head(lg, te.astype(np.float64), q, ids, *opt)
    net = make_net(arch, P, B)
    ted = torch.tensor(te, device=DEV)                     # [B, T, Q]: the stride becomes ld_teacher
    want_dmel = name == 'cond'

    def run():
        load_save(net, net.save_flat, S)
        net.grad_flat.fill_(float('nan'))
        net.forward(q, mel, ids, backward=True, want_dmel=want_dmel, teacher_logits=ted, distill_alpha=opt[0],
                    distill_temp=opt[1], label_smoothing=opt[2])
        torch.cuda.synchronize()
        assert int(net.plan_tensor(T, 'status').view(torch.int32)[0]) == 0
        return (_bits(net.grad_flat), _bits(net.stats), _bits(net.stats_ex), _bits(net.plan_tensor(T, 'logits')),
                _bits(net.dmel) if want_dmel else None)

    first = run()
    s = net.plan_tensor(T, 's').view(M, -1)[:, :arch['n_skip']].cpu().numpy()
    r2 = net.plan_tensor(T, 'r2').view(M, -1)[:, :arch['n_post']].cpu().numpy()
    adoption_capped(cache, adopt_relu_signs(cache, s, r2))
    if want_dmel:
        dm, G = dmel_ref(arch, P, cache, dl)
    else:
        G = R.backward(arch, P, cache, dl, 0.0)
    got_stats, got_ex = net.stats.cpu().numpy(), net.stats_ex.cpu().numpy()
    print('%s stats %s ref %s | stats_ex %s ref %s' % (name, got_stats[:3], stats[:3], got_ex[:2], ex[:2]))
    assert got_stats[1] == stats[1]
    # the logits carry the forward's 1e-4 (tests/test_gpu_eval.py): a row's value moves by at most
    # twice that through the hard term and 2·tau·(1/tau)·1e-4 through the KL of two softmaxes
    np.testing.assert_allclose(got_stats[0], stats[0], rtol=0, atol=4e-4 * stats[1])
    np.testing.assert_allclose(got_ex[0], ex[0], rtol=0, atol=2e-4 * stats[1])
    np.testing.assert_allclose(got_ex[1], ex[1], rtol=0, atol=4e-4 * stats[1])
    assert got_ex[2] == 0.0 and got_ex[3] == 0.0
    gl = net.plan_tensor(T, 'logits').view(B, T, Q).cpu().numpy()
    scored = np.zeros((B, T), bool)
    scored[:, :-1] = ids[:, 1:] != 0
    assert np.all(gl[~scored] == 0.0)
    worst = {}
    for n in net.layout.names():
        assert torch.isfinite(net.grads[n]).all(), n + ': part of the gradient not written'
        worst[n] = grad_close(net.grads[n].cpu().double().numpy(), G[n], '%s %s' % (name, n))
    top = max(worst, key=worst.get)
    print('%s: worst gradient %s at %.3g of its own max (bar %.3g); POST2_BIAS %.3g' % (
        name, top, worst[top], GRAD_REL, worst.get('POST2_BIAS', float('nan'))))
    if want_dmel:
        print('%s: dmel at %.3g' % (name, grad_close(net.dmel.cpu().double().numpy(), dm, name + ' dmel')))
    second = run()
    gc = [n for n in net.layout.names() if n.startswith('GC_')]     # float atomics, see (b)
    g1, g2 = net.layout.views(first[0]), net.layout.views(second[0])
    bad = [n for n in net.layout.names() if n not in gc and not torch.equal(g1[n], g2[n])]
    assert not bad, 'two runs differ in %s' % bad
    for a, b in zip(first[1:], second[1:]):
        assert a is None or torch.equal(a, b)


# ---- (d) Distiller, two consecutive slices ------------------------------------------------------------------
def test_distiller_two_slices(lib, tmp_path):
    """Teacher 'chain' (2 x 3 layers, parameter draw 1), student 1 x 3 layers; two slices of T = 64 with
    SAVE carried on both sides.  The teacher logits the student read are bitwise those of
    teacher.eval_slice alone; the student's stats / stats_ex are held to the float32 twin of the whole
    chain (oracle forwards in float32, then the float32 head) against float64; the teacher's SAVE
    round-trips through state_tensors / load_state_tensors bitwise."""
    from lbwn.arch import normalize_arch
    alpha, temp = 0.5, 2.0
    tarch, Pt, St, slices = E.case('chain', n_slices=2, pseed=1)
    sarch = normalize_arch(dict(tarch, n_blocks=1))
    Ps = R.init_params(sarch, np.random.default_rng(0), bias_scale=0.5)
    Ss = R.init_save(sarch, 2, np.random.default_rng(1))
    Pt, St, Ps, Ss = (D.f32_params(x) for x in (Pt, St, Ps, Ss))
    T = 64
    student, teacher, alone = make_net(sarch, Ps, 2), make_net(tarch, Pt, 2), make_net(tarch, Pt, 2)
    load_save(student, student.save_flat, Ss)
    dist = Distiller(student, teacher, alpha, temp)
    assert dist.recep_field_sz() == teacher.get_recep_field_sz() > student.get_recep_field_sz()
    load_save(teacher, dist.state['save'], St)
    st_alone = alone.eval_state()
    load_save(alone, st_alone['save'], St)
    # float64 reference and the float32 twin of the whole chain
    f32 = lambda d: {k: v.astype(np.float32) for k, v in d.items()}   # noqa: E731
    ref_s, _ = E.run(sarch, Ps, slices, Ss)
    ref_t, ref_save_t = E.run(tarch, Pt, slices, St)
    tw_s, _ = E.run(sarch, f32(Ps), slices, f32(Ss))
    tw_t, _ = E.run(tarch, f32(Pt), slices, f32(St))
    assert tw_s[0]['logits'].dtype == np.float32
    got = []
    for k, (q, ids, mel) in enumerate(slices):
        dist.step(q, mel, ids, backward=True)
        used = _bits(teacher.logits_view(T))
        alone.eval_slice(st_alone, q, mel, ids)
        torch.cuda.synchronize()
        assert torch.equal(used, _bits(alone.logits_view(T))), 'slice %d: teacher logits differ' % k
        assert torch.equal(_bits(dist.state['save']), _bits(st_alone['save']))
        got.append((student.stats.cpu().numpy().copy(), student.stats_ex.cpu().numpy().copy()))
    assert dist.teacher_status() == 0 and student.status() == 0
    # the progress line keeps its nine columns (total and mean are the objective); plain xent and KL follow
    cols = student.progress_line().split('\t')
    stats, ex = got[-1]
    assert len(cols) == 11 and abs(float(cols[2]) - stats[0] / stats[1]) < 1e-4
    assert abs(float(cols[9]) - ex[0] / stats[1]) < 1e-4 and abs(float(cols[10]) - ex[1] / stats[1]) < 1e-4
    student.forward(slices[0][0], None, slices[0][1], backward=False)
    assert student.stats_ex is None and len(student.progress_line().split('\t')) == 9
    for k, (q, ids, mel) in enumerate(slices):
        ref = D.head(ref_s[k]['logits'], ref_t[k]['logits'], q, ids, alpha, temp, 0.0)
        tw = D.twin(tw_s[k]['logits'], tw_t[k]['logits'], q, ids, alpha, temp, 0.0)
        stats, ex = got[k]
        tag = 'slice %d ' % k
        held_to_twin(tag + 'stats[0]', stats[0], ref[2][0], tw[4]['stats0'], scalar=True)
        held_to_twin(tag + 'stats_ex[0]', ex[0], ref[3][0], tw[4]['ex0'], scalar=True)
        held_to_twin(tag + 'stats_ex[1]', ex[1], ref[3][1], tw[4]['ex1'], scalar=True)
        assert stats[1] == ref[2][1] and ex[2] == 0.0 and ex[3] == 0.0
        print(tag + 'stats[2] kernel %g float64 %g' % (stats[2], ref[2][2]))
        if ref_s[k]['gap'][ref_s[k]['scored']].min() > 1e-3:      # no argmax within the logit tolerance of a tie
            assert stats[2] == ref[2][2]
    # the teacher's SAVE after two slices is the oracle's, and round-trips bitwise
    for n, v in dist.teacher_save_vars.items():
        np.testing.assert_allclose(v.cpu().numpy(), ref_save_t[n], rtol=0, atol=1e-4 * max(1.0, np.abs(ref_save_t[n]).max()))
    from lbwn.ckpt import load_tensors, save_tensors
    tensors = dist.state_tensors()
    assert sorted(tensors) == sorted('TEACHER/' + n for n in teacher.save_index)
    path = save_tensors(str(tmp_path / 'd.safetensors'), tensors)
    before = _bits(dist.state['save'])
    dist.state['save'].fill_(7.0)
    assert dist.load_state_tensors(load_tensors(path)) is True
    assert torch.equal(_bits(dist.state['save']), before)
    import io
    log = io.StringIO()
    assert dist.load_state_tensors({}, log=log) is False and log.getvalue().count('Warning') == 1
    assert not dist.state['save'].any()
