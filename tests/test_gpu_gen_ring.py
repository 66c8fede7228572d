"""Ring plans of the cached generator on the GPU (lbwn_gen_plan_create_ex, lbwn_gen_extend, lbwn_gen_collect):
outputs and conditioning addressed by the local step modulo the ring.  The bitwise reference throughout is the
plan without a ring of the same build, whose code path the ring does not touch; the float64 checks are those
of tests/test_gpu_gen_sessions.py (its helpers are imported, the tolerances are its check_session's)."""
import ctypes

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.arch import normalize_arch
from lbwn.imodel import plan_sessions
from tests.test_gpu_gen_lc import make_gen, small
from tests.test_gpu_gen_sessions import check_session, mels, session_logits

pytestmark = pytest.mark.gpu

R = 64
FRAMES = (8, 5, 8, 3, 6, 7, 2, 8, 4)


@pytest.fixture(params=['persistent', 'per_step'])
def form(request, monkeypatch):
    """Both execution forms, as tests/test_gpu_gen_sessions.py: the cond ring holds NC = 4 steps."""
    if request.param == 'per_step':
        monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
    else:
        monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    return request.param


def gen(arch, B, ring, graph=True, chunk=10):
    g, P = make_gen(arch, B, chunk=chunk)
    g.ring_steps = ring
    g.use_graph = graph
    return g, P


def words(g):
    return g.tensor('sessions', torch.int64).view(g.batch_sz, 4).cpu().numpy().copy()


def status(g):
    torch.cuda.synchronize()
    return int(g.tensor('status', torch.int32).item())


# ---- 1. a list through a small ring ------------------------------------------------------------------
@pytest.mark.parametrize('gc', [0, 5])
def test_list_through_a_small_ring(form, gc):
    arch = small(gc=gc)
    B, hop = 3, 8
    ms = mels(61, FRAMES)
    voices = [1 + u % 5 for u in range(len(ms))] if gc else None
    lengths = [f * hop for f in FRAMES]
    rounds, total = plan_sessions(lengths, B, 10)
    assert total > 2 * R
    # the plan without a ring: the wavs, and every utterance's samples at (slot, base) of its schedule
    g0, P = gen(arch, B, 0)
    ref = g0.vocode(ms, gc_ids=voices)
    assert g0.persistent == (form == 'persistent')
    where, t = {}, 0
    for steps, begins in rounds:
        for slot, u in begins:
            where[u] = (slot, t)
        t += steps
    smp0 = g0.samples().cpu().numpy()
    bytes0 = g0.lib.lbwn_gen_workspace_bytes(g0._plan)
    g, _ = gen(arch, B, R)
    got = {u: (w, s) for u, w, s in g.vocode_iter(ms, gc_ids=voices, samples=True)}
    assert sorted(got) == list(range(len(ms))) and g.persistent == (form == 'persistent')
    for u, n in enumerate(lengths):
        slot, b0 = where[u]
        assert tuple(got[u][0].shape) == (n,)
        np.testing.assert_array_equal(got[u][0].cpu().numpy(), ref[u].cpu().numpy())
        np.testing.assert_array_equal(got[u][1].cpu().numpy(), smp0[slot, b0:b0 + n])
    assert int(g.tensor('step', torch.int64).item()) == total
    # the utterance that ends the run ends it at its last local step: its stream's logits are that step's
    last = [u for u, (slot, b0) in where.items() if b0 + lengths[u] == total]
    assert last
    u = last[0]
    s = got[u][1].cpu().numpy()
    lg = session_logits(arch, P, s, ms[u], voices[u] if gc else None)
    check_session(s, g.logits().cpu().numpy()[where[u][0]], lg, key=u)
    # the ring's workspace is smaller than the schedule's and does not follow the list
    bytes1, plan = g.lib.lbwn_gen_workspace_bytes(g._plan), g._plan
    assert bytes1 < bytes0
    out = g.vocode(ms + ms, gc_ids=voices + voices if gc else None, keys=list(range(len(ms))) * 2)
    assert g._plan is plan and g.lib.lbwn_gen_workspace_bytes(g._plan) == bytes1 == g._ws.numel()
    for u in range(len(ms)):                       # equal keys: the second copy of the list draws the same
        np.testing.assert_array_equal(out[u].cpu().numpy(), ref[u].cpu().numpy())
        np.testing.assert_array_equal(out[len(ms) + u].cpu().numpy(), ref[u].cpu().numpy())


# ---- 2. an utterance longer than the ring ------------------------------------------------------------
N_LONG = 160
_LONG = {}


def long_run(form, ring, extends, graph):
    """B = 3, 16 rounds of 10 steps.  Stream 1 carries a 20-frame mel: on the ring plan it is begun with 6
    frames and (``extends``) fed up to the ring's capacity before every round; on the plan without a ring it is
    begun with the whole mel.  Stream 0 carries 8 frames, then from step 70 a 6-frame utterance; stream 2 five
    frames, clamped to the end.  Returns (samples [3, 160], wav [3, 160]) by the absolute step."""
    key = (form, ring, extends, graph)
    if key in _LONG:
        return _LONG[key]
    g, _ = gen(small(), 3, R if ring else 0, graph=graph)
    long = mels(51, [20])[0]
    m0, m2, m0b = mels(52, [8, 5, 6])
    g.build_graph(N_LONG)
    g.init_sessions()
    g.begin([0, 1, 2], [m0, long[:6] if ring else long, m2], keys=[0, 1, 2])
    base = [0, 0, 0]
    smp, wav = [[] for _ in range(3)], [[] for _ in range(3)]
    for r in range(N_LONG // 10):
        t = 10 * r
        if r == 7:
            g.begin([0], [m0b], keys=[5])
            base[0] = t
        if ring and extends:
            rows, want = g._rows[1], min(N_LONG, max(t - 1, 0) // 8 * 8 + R)
            if want > rows:
                g.extend([1], [long[rows // 8:want // 8]])
        g.step(10)
        if ring:
            for b in range(3):
                w, s = g.collect(b, t - base[b], 10)
                smp[b].append(s)
                wav[b].append(w)
    torch.cuda.synchronize()
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == N_LONG
    assert g.persistent == (form == 'persistent')
    if ring:
        out = (torch.stack([torch.cat(s) for s in smp]).cpu().numpy(), torch.stack([torch.cat(w) for w in wav]).cpu().numpy())
        if extends:
            assert words(g)[1].tolist() == [0, 1, N_LONG, 0]
    else:
        out = (g.samples().cpu().numpy()[:, :N_LONG].copy(),
               g.tensor('wav').view(3, N_LONG).cpu().numpy().copy())
    _LONG[key] = out
    return out


@pytest.mark.parametrize('graph', [False, True])
def test_utterance_longer_than_the_ring(form, graph):
    s_ring, w_ring = long_run(form, True, True, graph)
    s_ref, w_ref = long_run(form, False, False, graph)
    assert len(np.unique(s_ref[1])) > 8
    np.testing.assert_array_equal(s_ring[1], s_ref[1])
    np.testing.assert_array_equal(w_ring[1], w_ref[1])
    # the neighbours: against the plan without a ring, and against the twin that never extends
    s_twin, w_twin = long_run(form, True, False, graph)
    for b in (0, 2):
        np.testing.assert_array_equal(s_ring[b], s_ref[b])
        np.testing.assert_array_equal(w_ring[b], w_ref[b])
        np.testing.assert_array_equal(s_ring[b], s_twin[b])
        np.testing.assert_array_equal(w_ring[b], w_twin[b])
    np.testing.assert_array_equal(s_ring[1][:49], s_twin[1][:49])          # rows 0..47 cover steps 0..48
    assert not np.array_equal(s_ring[1], s_twin[1])                         # after that the twin is clamped


# ---- 3. no LC, the dense path ------------------------------------------------------------------------
def test_no_lc_dense_path_through_the_ring(form):
    arch = normalize_arch(dict(small(), n_lc_in=0, n_lc_out=0, lc_upsample=[]))
    B, n = 2, 100
    g0, _ = gen(arch, B, 0)
    g0.build_graph(n)
    g0.init_buffers()
    g0.step(n)
    torch.cuda.synchronize()
    s0 = g0.samples().cpu().numpy()[:, :n]
    w0 = g0.tensor('wav').view(B, n).cpu().numpy()
    assert len(np.unique(s0)) > 8
    g, _ = gen(arch, B, 32)
    g.build_graph(1)
    assert g.max_steps == 32 and tuple(g.samples().shape) == (B, 32)
    g.init_buffers()
    parts = [[], []]
    for k in range(4):
        g.step(25)
        for b in range(B):
            parts[b].append(g.collect(b, 25 * k, 25))
    assert status(g) == 0 and g.persistent == (form == 'persistent')
    for b in range(B):
        np.testing.assert_array_equal(torch.cat([p[1] for p in parts[b]]).cpu().numpy(), s0[b])
        np.testing.assert_array_equal(torch.cat([p[0] for p in parts[b]]).cpu().numpy(), w0[b])
    # the ring itself: column i mod 32 holds the last local step that maps to it
    ring = g.samples().cpu().numpy()
    for i in range(n - 32, n):
        np.testing.assert_array_equal(ring[:, i % 32], s0[:, i])


# ---- 4. outside the fused upsample envelope ----------------------------------------------------------
def test_extends_outside_the_fused_envelope(form):
    """n_lc_in 20 > n_lc_out 16: every stage of every begin and extend is a GEMM.  Ring of 96 rows (12
    frames): begun with 4 frames, extended by 4, then by 8 frames that wrap (frames 8..11, then 0..3)."""
    arch = normalize_arch(dict(small(), n_lc_in=20))
    a = (ctypes.c_int * 2)(2, 4)
    assert _lib.load().lbwn_lc_upsample_fused_ok(2, a, 20, 16) == 0
    B, ring = 3, 96
    ms = mels(71, [16, 4, 4], width=20)
    g, P = gen(arch, B, ring)
    g.build_graph(1)
    g.init_sessions()
    g.begin([0, 1, 2], [ms[0][:4], ms[1], ms[2]], keys=[0, 1, 2])
    got = []
    for steps, f0, f1 in ((30, 4, 8), (30, 8, 16), (68, None, None)):
        g.step(steps)
        e = sum(len(x) for x in got)
        got.append(g.collect(0, e, steps)[1].cpu().numpy())
        if f0 is not None:
            g.extend([0], [ms[0][f0:f1]])
    assert status(g) == 0 and words(g)[0].tolist() == [0, 0, 128, 0]
    s = np.concatenate(got)
    assert len(s) == 128 and len(np.unique(s)) > 8
    lg = session_logits(arch, P, s, ms[0], None)
    check_session(s, g.logits().cpu().numpy()[0], lg, key=0)


# ---- 5. the guards on the device ---------------------------------------------------------------------
def test_device_guards(form):
    arch = small()
    B = 3
    ms = mels(81, [8, 8, 8])
    g, _ = gen(arch, B, R)
    g.build_graph(1)
    lib, P, ws = g.lib, ctypes.byref(g._params_c), g._ws.data_ptr()
    more = torch.from_numpy(mels(82, [2])[0]).cuda()
    sentinel = lambda: (torch.full((10,), -7.0, device='cuda'), torch.full((10,), -7, dtype=torch.int32, device='cuda'))

    def fresh(n):
        g.init_sessions()
        g.begin([0, 1, 2], ms, keys=[0, 1, 2])
        g.step(n)
        assert status(g) == 0
        return words(g), g.samples().cpu().numpy().copy()

    def dead(w0, s0, n):
        """Status 7, the words untouched, a further run draws nothing, lbwn_gen_start clears the status."""
        assert status(g) == 7
        np.testing.assert_array_equal(words(g), w0)
        g._launch(10)
        torch.cuda.synchronize()
        assert int(g.tensor('step', torch.int64).item()) == n
        np.testing.assert_array_equal(g.samples().cpu().numpy(), s0)
        with pytest.raises(RuntimeError, match='status 7'):
            g.check_status()
        g.init_sessions()
        assert status(g) == 0

    # an extend past the ring: 64 rows given, local step 10 reads row 9, 16 more make 71 > 64 unread
    w0, s0 = fresh(10)
    with pytest.raises(ValueError, match='extend: mels\\[0\\] brings 16 rows'):
        g.extend([0], [more])
    e = (_lib.GenExtendEntry * 1)()
    e[0].slot, e[0].mel, e[0].n_frames = 0, more.data_ptr(), 2
    assert lib.lbwn_gen_extend(g._plan, P, ws, e, 1, ctypes.sizeof(_lib.GenExtendEntry), _lib.stream_ptr()) == 0
    dead(w0, s0, 10)
    # one frame fits (64 + 8 - 9 = 63): the same call is taken, the word advances
    w0, s0 = fresh(10)
    e[0].n_frames = 1
    assert lib.lbwn_gen_extend(g._plan, P, ws, e, 1, ctypes.sizeof(_lib.GenExtendEntry), _lib.stream_ptr()) == 0
    assert status(g) == 0 and words(g)[0].tolist() == [0, 0, 72, 0]
    # a collect of steps already overwritten: 80 run, the ring holds 16..79
    w0, s0 = fresh(80)
    with pytest.raises(ValueError, match='overwritten'):
        g.collect(1, 10, 10)
    wv, sm = sentinel()
    assert lib.lbwn_gen_collect(g._plan, ws, 1, 10, 10, wv.data_ptr(), sm.data_ptr(), _lib.stream_ptr()) == 0
    dead(w0, s0, 80)
    assert bool((wv == -7.0).all()) and bool((sm == -7).all())
    # a collect of steps not yet run: 10 run, [5, 15) asked
    w0, s0 = fresh(10)
    with pytest.raises(ValueError, match='only 10 have run'):
        g.collect(2, 5, 10)
    assert lib.lbwn_gen_collect(g._plan, ws, 2, 5, 10, wv.data_ptr(), sm.data_ptr(), _lib.stream_ptr()) == 0
    dead(w0, s0, 10)
    assert bool((wv == -7.0).all()) and bool((sm == -7).all())
    # and the edge that is taken: exactly the last R steps
    w0, s0 = fresh(80)
    wv, sm = g.collect(1, 16, 64)
    assert status(g) == 0
    np.testing.assert_array_equal(sm.cpu().numpy(), np.roll(s0[1], -16))


# ---- extend and collect on a plan without a ring -----------------------------------------------------
def test_extend_and_collect_without_a_ring(form):
    """A plan without a ring: stream 1 is begun with half its mel (5 of 10 frames) and extended after 20 steps;
    its 80 steps, collected in two calls, are bitwise those of the begin with the whole mel read from
    "samples" / "wav", and so are its neighbours'.  The reserved rows (80) bound the extend on the host: EINVAL
    through ``_lib``, ValueError from the wrapper, the row words untouched."""
    arch, B, n = small(), 3, 80
    ms = mels(95, [10, 10, 4])
    runs = []
    for split in (False, True):
        g, _ = gen(arch, B, 0)
        g.build_graph(n)
        g.init_sessions()
        g.begin([0, 1, 2], [ms[0], ms[1][:5] if split else ms[1], ms[2]], keys=[0, 1, 2])
        g.step(20)
        if split:
            g.extend([1], [ms[1][5:]])
            assert g._rows[1] == 80
        g.step(n - 20)
        assert status(g) == 0 and g.persistent == (form == 'persistent')
        runs.append((g.samples().cpu().numpy()[:, :n].copy(), g.tensor('wav').view(B, n).cpu().numpy().copy()))
    (s0, w0), (s1, w1) = runs
    assert len(np.unique(s0[1])) > 8
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(w1, w0)
    assert words(g)[1].tolist() == [0, 1, 80, 0]
    for b in range(B):
        wa, sa = g.collect(b, 0, 30)
        wb, sb = g.collect(b, 30, 50)
        np.testing.assert_array_equal(torch.cat([sa, sb]).cpu().numpy(), s0[b])
        np.testing.assert_array_equal(torch.cat([wa, wb]).cpu().numpy(), w0[b])
    assert status(g) == 0
    # one frame more than the reserved rows hold
    more = torch.from_numpy(mels(96, [1])[0]).cuda()
    with pytest.raises(ValueError, match='extend: mels\\[0\\] brings 8 rows to the 80 of stream 1'):
        g.extend([1], [more])
    e = (_lib.GenExtendEntry * 1)()
    e[0].slot, e[0].mel, e[0].n_frames = 1, more.data_ptr(), 1
    assert g.lib.lbwn_gen_extend(g._plan, ctypes.byref(g._params_c), g._ws.data_ptr(), e, 1,
                                 ctypes.sizeof(_lib.GenExtendEntry), _lib.stream_ptr()) == 22
    assert b"e[0].n_frames = 1: the session's 80 rows + 8 exceed the plan's 80 reserved rows" in g.lib.lbwn_last_error()
    e[0].slot = 2                                   # 32 rows + 8: taken
    assert g.lib.lbwn_gen_extend(g._plan, ctypes.byref(g._params_c), g._ws.data_ptr(), e, 1,
                                 ctypes.sizeof(_lib.GenExtendEntry), _lib.stream_ptr()) == 0
    assert status(g) == 0 and words(g)[:, 2].tolist() == [80, 80, 40]
    # steps that have not run: the wrapper refuses first
    with pytest.raises(ValueError, match='only 80 have run'):
        g.collect(0, 40, 50)


# ---- snapshots ---------------------------------------------------------------------------------------
def test_state_load_on_ring_plans(form):
    """lbwn_gen_state_load is EINVAL on a ring LC plan in session mode (the rows a rewound step reads may be
    gone); on a ring plan without LC an identity rewind repeats the run, ring columns included."""
    g, _ = gen(small(), 3, R)
    g.build_graph(1)
    g.init_sessions()
    g.begin([0, 1, 2], mels(97, [8, 8, 8]), keys=[0, 1, 2])
    g.step(10)
    state = g.save_state()
    with pytest.raises(_lib.LbwnError, match='gen_state_load: a ring LC plan in session mode'):
        g.load_state(state)
    assert status(g) == 0
    arch = normalize_arch(dict(small(), n_lc_in=0, n_lc_out=0, lc_upsample=[]))
    g, _ = gen(arch, 2, 32)
    g.build_graph(1)
    g.init_buffers()
    g.step(40)
    state = g.save_state()
    g.step(50)
    first = g.samples().cpu().numpy().copy(), g.tensor('wav').cpu().numpy().copy(), g.logits().cpu().numpy().copy()
    g.load_state(state)
    g.step(50)
    assert status(g) == 0 and int(g.tensor('step', torch.int64).item()) == 90
    for a, b in zip(first, (g.samples().cpu().numpy(), g.tensor('wav').cpu().numpy(), g.logits().cpu().numpy())):
        np.testing.assert_array_equal(a, b)
    w, _ = g.collect(1, 58, 32)
    np.testing.assert_array_equal(w.cpu().numpy(), np.roll(first[1].reshape(2, 32)[1], -(58 % 32)))


# ---- the command line --------------------------------------------------------------------------------
def test_generate_mel_list_ring_end_to_end(tmp_path, monkeypatch):
    """generate.py --mel-list --mel-list-ring 32 at batch 2: five utterances, one of 9 frames (72 steps, longer
    than the ring), written as they complete; every wav is the one WaveNetGen.vocode gives on a plan without
    a ring at batch 3 (keys = list positions)."""
    import json
    import os
    import generate
    from scipy.io import wavfile
    from lbwn.ckpt import ckpt_file, save_tensors
    from tests.test_gpu_gen_lc import SEED, _PARAMS
    monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    arch = small(gc=5)
    frames = [4, 9, 2, 7, 3]
    ms = mels(91, frames)
    voices = [3, 1, 5, 2, 4]
    g, _ = make_gen(arch, 3, chunk=10)
    want = [w.cpu().numpy() for w in g.vocode(ms, gc_ids=voices)]
    dev = _PARAMS[json.dumps(arch, sort_keys=True)][0]
    pfx = str(tmp_path / 'net')
    save_tensors(ckpt_file(pfx), dev)
    af = tmp_path / 'arch.json'
    af.write_text(json.dumps(dict(arch, wav_input_type='mu_law_quant')))
    lines = []
    for u, m in enumerate(ms):
        np.save(tmp_path / ('m%d.npy' % u), m)
        lines.append('%d\t%s\tutt%d' % (voices[u], tmp_path / ('m%d.npy' % u), u))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    monkeypatch.setattr(generate, 'mel_list_groups', None)          # the ring path does not group
    out = generate.main(['--mel-list', str(tmp_path / 'list.txt'), '--mel-list-ring', '32', '--batch-size', '2',
                         '--chunk-size', '10', '--seed', str(SEED), str(af), pfx, str(tmp_path / 'out')])
    for u in range(5):
        np.testing.assert_array_equal(out[u], want[u], str(u))
        sr, x = wavfile.read(os.path.join(str(tmp_path / 'out'), 'utt%d.wav' % u))
        assert sr == 16000
        np.testing.assert_array_equal(x, want[u])
