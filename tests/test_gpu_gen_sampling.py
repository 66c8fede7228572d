"""Temperature / top-k / top-p sampling of the cached generator on the GPU, against the float64
reference of tests/sampling_ref.py evaluated along the GPU's own trajectory (R.generate(forced_q=)):
every draw is compared with the reference draw of the float64 logits it was taken from.  A draw may
differ only where a near-tie flag explains it (sampling_ref.flags), at most 2 per case -- the cap of
tests/test_gpu_gen.py; the reference against itself differs nowhere, and a numpy fp32 emulation of the
kernel's bisection with logit noise of 1e-5·max|lg| (ten times what the generator shows) gave 0-1 per
case -- and, with no exception, every draw lies in the reference's kept set up to the logits' tolerance.
The parameters are made on the host (sampling_ref.host_params: POST2 x 30, or x 10 at Q = 100, so the
softmax is peaked and the filters bite; tests/test_gen_sampling.py holds the conditions on them)."""
import os

import numpy as np
import pytest
import torch

from lbwn.arch import load_arch
from lbwn.imodel import WaveNetGen
from oracle import wavenet_ref as R
from tests import sampling_ref as S
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
NEUTRAL = (1.0, 0, 1.0)


@pytest.fixture(params=['persistent', 'per_step'])
def form(request, monkeypatch):
    """Both execution forms, as tests/test_gpu_gen.py: the persistent one-launch kernel and the
    per-step launches (LBWN_GEN_PERSIST=0)."""
    if request.param == 'per_step':
        monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
    else:
        monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    return request.param


def make_gen(arch, scale, B, chunk, setting=NEUTRAL, teacher_q=None):
    P32, P = S.host_params(arch, scale)
    T, k, p = setting
    g = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                   arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                   B, chunk, None, seed=S.SEED, temperature=T, top_k=k, top_p=p)
    g.load_params(P32)
    if teacher_q is not None:
        g.teacher_mu = torch.as_tensor(np.asarray(teacher_q, np.int32), device='cuda')
    return g, P


def finish(g, n, persistent):
    torch.cuda.synchronize()
    assert g.persistent == persistent
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    return g.samples().cpu().numpy()[:, :n].copy()


def check_against_reference(g, arch, P, got, setting, label, **gen_kw):
    """The common check: float64 logits along the GPU's trajectory, every draw against ref_draw, and
    the last step's raw "logits"."""
    B, n = got.shape
    _, _, lg = R.generate(arch, P, B, n, seed=S.SEED, forced_q=got, return_logits=True, **gen_kw)
    S.check_draws(got, lg, setting, label=label)
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())
    return lg


@pytest.mark.parametrize('setting', S.S_ALL, ids=str)
def test_sampling_small_arch_every_setting(setting, form):
    arch = S.small(256)
    B, n = 3, 64
    g, P = make_gen(arch, S.POST2_SCALE[256], B, 16, setting)
    g.run(n)
    got = finish(g, n, form == 'persistent')
    check_against_reference(g, arch, P, got, setting, 'Q=256 %s' % form)


@pytest.mark.parametrize('setting', [NEUTRAL] + S.S_SUB, ids=str)
def test_sampling_q100_two_codes_per_lane_empty_lanes(setting, form):
    """Q = 100: 2 codes per lane, lanes 50..63 hold no code.  The neutral setting runs the default draw
    at this Q, so its failure could be told apart from the filter's."""
    arch = S.small(100)
    B, n = 3, 64
    g, P = make_gen(arch, S.POST2_SCALE[100], B, 16, setting)
    g.run(n)
    got = finish(g, n, form == 'persistent')
    check_against_reference(g, arch, P, got, setting, 'Q=100 %s' % form)


@pytest.mark.parametrize('setting', [NEUTRAL] + S.S_SUB, ids=str)
def test_sampling_q300_eight_slots_ragged_last_lane(setting, monkeypatch):
    """Q = 300 (per-step form only: the persistent form takes Q <= 256): 5 codes per lane in the
    8-slot instantiation, the 60th lane is the last with codes."""
    monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
    arch = S.small(300)
    B, n = 3, 64
    g, P = make_gen(arch, S.POST2_SCALE[300], B, 16, setting)
    g.run(n)
    got = finish(g, n, False)
    check_against_reference(g, arch, P, got, setting, 'Q=300')


def test_neutral_settings_are_bitwise_the_default(form):
    arch = S.small(256)
    B, n = 3, 64
    out = []
    for setter in (None, (1, 0, 1), (1, arch['n_quant'], 1)):
        g, _ = make_gen(arch, S.POST2_SCALE[256], B, 16)
        if setter:
            g.set_sampling(*setter)
        g.run(n)
        got = finish(g, n, form == 'persistent')
        out.append((got, g.logits().cpu().numpy().copy()))
    for got, lg in out[1:]:
        np.testing.assert_array_equal(got, out[0][0])
        assert np.array_equal(lg.view(np.uint32), out[0][1].view(np.uint32))


def test_sampling_b40_gc_teacher_ragged_groups(form):
    """B = 40 (persistent: three ragged stream groups; per step: the GEMM form) with GC and a 12-code
    teacher: the teacher's steps store the filtered draws and feed the teacher's codes."""
    setting = (0.8, 40, 0.95)
    arch = S.small(256, gc=5)
    B, n = 40, 24
    teacher_q = np.random.default_rng(1).integers(0, 256, 12).astype(np.int32)
    gc = [1 + b % 5 for b in range(B)]
    g, P = make_gen(arch, S.POST2_SCALE[256], B, 8, setting, teacher_q=teacher_q)
    g.build_graph(n)
    g.run(n, gc_ids=gc)
    got = finish(g, n, form == 'persistent')
    check_against_reference(g, arch, P, got, setting, 'B=40 %s' % form, teacher_q=teacher_q, gc_ids=gc)
    # the stored draws of the teacher's steps are the model's filtered draws, not the teacher's codes
    assert (got[:, :12] != teacher_q[None, :]).any()


def test_changing_the_setting_under_graph_replay(form):
    """set_sampling between runs on one plan: the captured graph holds the setting of its capture, so
    it must be dropped -- a stale graph would replay the default draw in the second run."""
    arch = S.small(256)
    B, n = 3, 48
    g, P = make_gen(arch, S.POST2_SCALE[256], B, 16)
    g.run(n)
    first = finish(g, n, form == 'persistent')
    assert g._graph is not None
    g.set_sampling(1, 8, 1)
    g.run(n)
    second = finish(g, n, form == 'persistent')
    check_against_reference(g, arch, P, second, (1.0, 8, 1.0), 'replay %s' % form)
    assert (second != first).any()
    g.set_sampling(1, 0, 1)
    g.run(n)
    third = finish(g, n, form == 'persistent')
    np.testing.assert_array_equal(third, first)


def test_sampling_arch3_b10_graph_replay(form):
    """The shipped widths (par/arch3.json), B = 10, 300 steps as three replays of a 100-step graph."""
    setting = (0.8, 40, 0.95)
    arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    B, n = 10, 300
    g, P = make_gen(arch, 30.0, B, 100, setting)
    g.run(n)
    got = finish(g, n, form == 'persistent')
    assert len(np.unique(got)) > 4
    check_against_reference(g, arch, P, got, setting, 'arch3 %s' % form)


@pytest.mark.parametrize('setting', [(1.0, 8, 1.0), (0.8, 40, 0.95)], ids=str)
def test_sampling_with_local_conditioning(setting, form, monkeypatch):
    """The LC instantiations (gen_persist_kernel<true, FILT>, and the per-step sampler after the LC
    chain): the arch, parameters and float64 logits of tests/test_gpu_gen_lc.py."""
    from tests.test_gpu_gen_lc import make_gen as make_gen_lc, oracle_logits, small as small_lc
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    arch = small_lc()
    B, frames, hop = 3, 8, 8
    n = frames * hop + 1
    mel = np.random.default_rng(4).standard_normal((B, frames, arch['n_lc_in'])).astype(np.float32)
    g, P = make_gen_lc(arch, B, 16)
    g.set_sampling(*setting)
    g.run(n, mel=mel)
    got = finish(g, n, form == 'persistent')
    lg = oracle_logits(arch, P, got, mel)
    S.check_draws(got, lg, setting, label='LC %s' % form)
    np.testing.assert_allclose(g.logits().cpu().numpy(), lg[:, -1], rtol=0, atol=1e-4 * np.abs(lg[:, -1]).max())
