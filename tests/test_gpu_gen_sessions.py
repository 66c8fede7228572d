"""Sessions in the cached generator on the GPU (lbwn_gen_begin): a stream restarted between two runs
carries its utterance exactly as a fresh run would, its neighbours are not disturbed, and the Python layer
(begin / take / vocode) schedules a list through it.  The per-step arithmetic of a stream does not depend on
the absolute step, the stream index or its neighbours, so the equalities are bitwise; the float64 checks
follow tests/test_gpu_gen_lc.py (its helpers are imported, the tolerance is its check_run's)."""
import ctypes

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.arch import normalize_arch
from oracle import wavenet_ref as R
from tests.test_gpu_gen_lc import SEED, _near_tie, make_gen, small, step0

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['persistent', 'per_step'])
def form(request, monkeypatch):
    """Both execution forms, as tests/test_gpu_gen_lc.py; the cond ring holds NC = 4 steps, so every run
    below wraps it many times and a chunk is several sub-runs."""
    if request.param == 'per_step':
        monkeypatch.setenv('LBWN_GEN_PERSIST', '0')
    else:
        monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    return request.param


def mels(seed, frames, width=12):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((f, width)).astype(np.float32) for f in frames]


def snap(g, n):
    torch.cuda.synchronize()
    assert int(g.tensor('status', torch.int32).item()) == 0
    assert int(g.tensor('step', torch.int64).item()) == n
    return g.samples().cpu().numpy()[:, :n].copy(), g.logits().cpu().numpy().copy()


def session_logits(arch, P, got, mel, gc):
    """Float64 logits [n, Q] of one utterance alone along its trajectory ``got`` [n]: test_gpu_gen_lc's
    oracle_logits for one stream, with the upsampled mel cut or its last row repeated to the n - 1 positions
    the forward covers (the per-session clamp)."""
    n = len(got)
    mel = np.asarray(mel, np.float64)[None]
    lc, _ = R.lc_upsample_fwd(arch, P, mel)
    gcl = None if gc is None else [gc]
    save, lg0 = step0(arch, P, 1, gcl, lc[:, 0])
    rows = lc[:, :n - 1]
    if rows.shape[1] < n - 1:
        rows = np.concatenate([rows, np.repeat(lc[:, -1:], n - 1 - rows.shape[1], axis=1)], axis=1)
    ids = np.ones((1, n - 1), np.int64) if gc is None else np.full((1, n - 1), gc, np.int64)
    upsample = R.lc_upsample_fwd
    R.lc_upsample_fwd = lambda a, p, m: (rows, None)
    try:
        lg, _, _ = R.forward(arch, P, got[None, :n - 1].copy(), ids, save, mel=mel)
    finally:
        R.lc_upsample_fwd = upsample
    return np.concatenate([lg0[:, None], lg], axis=1)[0]


def check_session(got, logits, lg, key):
    """check_draws / check_run of tests/test_gpu_gen_lc.py for one session: every draw against the float64
    logits with the uniform of (SEED, key, local step) -- differences only at a near tie of the inverse CDF, at
    most 2 -- and the last step's logits within 1e-4 of their largest magnitude."""
    ref = np.array([R.sample_from_logits(lg[i], R.philox_uniform(SEED, key, i)) for i in range(len(got))])
    bad = np.flatnonzero(got != ref)
    print('draws %d, differing %d, max |logit| %.3f' % (len(got), len(bad), np.abs(lg).max()))
    ties = [int(i) for i in bad if _near_tie(lg[i], R.philox_uniform(SEED, key, int(i)))]
    assert len(ties) == len(bad), 'draws differ away from a CDF tie at local steps %s' % (bad[:8].tolist(),)
    assert len(bad) <= 2, bad.tolist()
    err, bound = np.abs(logits - lg[-1]).max(), 1e-4 * np.abs(lg[-1]).max()
    print('last-step logits: max err %.3e (bound %.3e)' % (err, bound))
    np.testing.assert_allclose(logits, lg[-1], rtol=0, atol=bound)


# ---- tests 1, 2, 4: one recycled run, its twin without the restart, and the fresh reference -----------
N1, N2 = 37, 41
VOICES, NEW_VOICE = [1, 2, 3], 4
_RUNS = {}


def recycled_runs(form, B=3, slot=1, gc=5):
    """(arch, P, A, A0, Rf, m_new): A = begin all (8, 5, 8 frames; keys 0..B-1), 37 steps, begin ``slot`` with
    a 6-frame mel, key 2 and another voice, 41 steps; A0 = the same without the second begin; Rf = a fresh
    plan on the lbwn_gen_set_mel path whose stream 2 carries that mel and voice, 41 steps.  Each is (samples,
    final logits).  Computed once per form and batch size."""
    key = (form, B, slot, gc)
    if key in _RUNS:
        return _RUNS[key]
    arch = small(gc=gc)
    frames = [(8, 5, 8)[b % 3] for b in range(B)]
    first = mels(21, frames)
    m_new = mels(22, [6])[0]
    voices = [1 + b % 5 for b in range(B)]
    out = []
    for restart in (True, False):
        g, P = make_gen(arch, B, chunk=10)
        g.build_graph(N1 + N2)
        g.init_sessions()
        g.begin(list(range(B)), first, gc_ids=voices if gc else None, keys=list(range(B)))
        g.step(N1)
        if restart:
            g.begin([slot], [m_new], gc_ids=[NEW_VOICE] if gc else None, keys=[2])
        g.step(N2)
        out.append(snap(g, N1 + N2))
        assert g.persistent == (form == 'persistent')
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(N2)                                    # 6 frames = 48 rows reserved; rows <= 39 are read
    dense = np.stack(mels(23, [6] * B))
    dense[2] = m_new
    rv = list(voices)
    rv[2] = NEW_VOICE
    g.init_buffers(gc_ids=rv if gc else None, mel=dense)
    g.step(N2)
    out.append(snap(g, N2))
    _RUNS[key] = (arch, P, out[0], out[1], out[2], m_new)
    return _RUNS[key]


def test_recycled_slot_equals_a_fresh_run(form):
    _, _, (sa, la), _, (sr, lr), _ = recycled_runs(form)
    assert len(np.unique(sr[2])) > 8
    np.testing.assert_array_equal(sa[1][N1:N1 + N2], sr[2][:N2])
    np.testing.assert_array_equal(la[1], lr[2])


def test_neighbours_undisturbed(form):
    _, _, (sa, la), (s0, l0), _, _ = recycled_runs(form)
    for b in (0, 2):
        np.testing.assert_array_equal(sa[b], s0[b])
        np.testing.assert_array_equal(la[b], l0[b])
    np.testing.assert_array_equal(sa[1][:N1], s0[1][:N1])          # and the slot's own first utterance
    assert not np.array_equal(sa[1][N1:], s0[1][N1:])


def test_recycled_slot_against_float64(form):
    arch, P, (sa, la), _, _, m_new = recycled_runs(form)
    lg = session_logits(arch, P, sa[1][N1:N1 + N2], m_new, NEW_VOICE)
    check_session(sa[1][N1:N1 + N2], la[1], lg, key=2)


# ---- test 3 --------------------------------------------------------------------------------------------
def test_neutral_sessions_equal_the_dense_path(form):
    """Every slot begun at step 0 with key = slot and equal frame counts is lbwn_gen_set_mel of the same mels."""
    arch = small()
    B, n = 3, 65
    ms = mels(31, [8] * B)
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(n)
    g.init_sessions()
    g.begin([2, 0, 1], [ms[2], ms[0], ms[1]], keys=[2, 0, 1])
    g.step(n)
    s1, l1 = snap(g, n)
    words = g.tensor('sessions', torch.int64).view(B, 4).cpu().numpy()
    np.testing.assert_array_equal(words, [[0, b, 64, 0] for b in range(B)])
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(n)
    g.init_buffers(mel=np.stack(ms))
    g.step(n)
    s2, l2 = snap(g, n)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(l1, l2)


# ---- test 5 --------------------------------------------------------------------------------------------
def test_clamp_per_session(form):
    """A 2-frame session (16 rows) run 30 local steps between two 5-frame neighbours, begun mid-run in a slot
    whose first session had 5 frames: the steps past row 15 reuse its own last row (the rows behind it in
    "lc" are a neighbour's in the dense layout and the earlier session's in the reserved layout)."""
    arch = small()
    B, n0, n = 3, 9, 30
    ms = mels(41, [5, 5, 5])
    short = mels(42, [2])[0]
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(n0 + n)
    g.init_sessions()
    g.begin([0, 1, 2], ms, keys=[0, 1, 2])
    g.step(n0)
    g.begin([1], [short], keys=[7])
    g.step(n)
    s, l = snap(g, n0 + n)
    assert g.tensor('sessions', torch.int64).view(B, 4).cpu().numpy()[1].tolist() == [n0, 7, 16, 0]
    wav = g.tensor('wav').view(B, n0 + n).cpu().numpy()
    np.testing.assert_array_equal(g.take(1, n).cpu().numpy(), wav[1, n0:])
    np.testing.assert_allclose(wav[1, n0:], R.mu_decode_np(s[1][n0:], 256), rtol=1e-5, atol=1e-6)
    lg = session_logits(arch, P, s[1][n0:], short, None)
    check_session(s[1][n0:], l[1], lg, key=7)


# ---- test 6 --------------------------------------------------------------------------------------------
def test_gc_without_lc(form):
    """No LC: a begin changes only the voice, the key and the base, and may come at any time (no stream
    needs a session).  The restarted slot equals a fresh run's stream 2 with that voice; the others, and the
    slot before its restart, equal the run without a begin."""
    arch = normalize_arch(dict(small(gc=5), n_lc_in=0, n_lc_out=0, lc_upsample=[]))
    B = 3
    out = []
    for restart in (True, False):
        g, _ = make_gen(arch, B, chunk=10)
        g.build_graph(N1 + N2)
        g.init_buffers(gc_ids=VOICES)
        g.step(N1)
        if restart:
            g.begin([1], gc_ids=[NEW_VOICE], keys=[2])
        g.step(N2)
        out.append(snap(g, N1 + N2))
        assert g.persistent == (form == 'persistent')
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(N2)
    g.init_buffers(gc_ids=[5, 5, NEW_VOICE])
    g.step(N2)
    sr, lr = snap(g, N2)
    (sa, la), (s0, l0) = out
    np.testing.assert_array_equal(sa[1][N1:], sr[2])
    np.testing.assert_array_equal(la[1], lr[2])
    for b in (0, 2):
        np.testing.assert_array_equal(sa[b], s0[b])
        np.testing.assert_array_equal(la[b], l0[b])
    np.testing.assert_array_equal(sa[1][:N1], s0[1][:N1])


# ---- test 7 --------------------------------------------------------------------------------------------
def test_two_persistent_groups(form):
    """B = 20: two persistent groups of 10 (per step: the MFMA-GEMM head); slot 17 of the second group is
    restarted mid-run and equals the fresh run's stream 2, its neighbours the run without the restart."""
    _, _, (sa, la), (s0, l0), (sr, lr), _ = recycled_runs(form, B=20, slot=17)
    np.testing.assert_array_equal(sa[17][N1:N1 + N2], sr[2][:N2])
    np.testing.assert_array_equal(la[17], lr[2])
    keep = [b for b in range(20) if b != 17]
    np.testing.assert_array_equal(sa[keep], s0[keep])
    np.testing.assert_array_equal(la[keep], l0[keep])


# ---- test 8 --------------------------------------------------------------------------------------------
def test_gemm_fallback_upsample(lib, monkeypatch):
    """n_lc_in = 24 is outside the fused upsample's envelope: every session's mel goes through one GEMM per
    stage.  Against float64 only (the GEMM's tile form may change with the row count)."""
    monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    monkeypatch.setenv('LBWN_GEN_LC_CHUNK', '4')
    arch = normalize_arch(dict(small(), n_lc_in=24))
    assert lib.lbwn_lc_upsample_fused_ok(2, (ctypes.c_int * 2)(2, 4), 24, 16) == 0
    B, n0, n = 3, 13, 33
    ms = mels(51, [6, 4, 5], 24)
    m_new = mels(52, [4], 24)[0]
    g, P = make_gen(arch, B, chunk=10)
    g.build_graph(n0 + n)
    g.init_sessions()
    g.begin([0, 1, 2], ms, keys=[0, 1, 2])
    g.step(n0)
    g.begin([1], [m_new], keys=[5])
    g.step(n)
    s, l = snap(g, n0 + n)
    lg = session_logits(arch, P, s[1][n0:], m_new, None)
    check_session(s[1][n0:], l[1], lg, key=5)
    lg0 = session_logits(arch, P, s[0], ms[0], None)       # a stream that was never restarted
    check_session(s[0], l[0], lg0, key=0)


# ---- test 9 --------------------------------------------------------------------------------------------
def test_captured_chunk_stays_valid_across_a_begin(form):
    """One captured chunk of 10 steps, replayed before and after a begin, equals the launches made directly:
    the base, the key, the rows, the voice's projection and the mel are all read on the device."""
    arch = small(gc=5)
    B = 3
    first, m_new = mels(61, [6, 5, 6]), mels(62, [3])[0]
    out = []
    for graph in (True, False):
        g, _ = make_gen(arch, B, chunk=10)
        g.use_graph = graph
        g.build_graph(43)
        g.init_sessions()
        g.begin([0, 1, 2], first, gc_ids=VOICES, keys=[0, 1, 2])
        g.step(20)
        captured = g._graph
        assert (captured is not None) == graph
        g.begin([2], [m_new], gc_ids=[NEW_VOICE], keys=[9])
        assert g._graph is captured                                  # the begin did not drop it
        g.step(23)
        out.append(snap(g, 43))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


# ---- test 10 -------------------------------------------------------------------------------------------
def test_vocode_equals_each_utterance_alone(form):
    """7 mels of 2..9 frames at B = 3, chunk 10: every wav is the utterance run alone (B = 1) with key = its
    index, whatever slot and step the schedule gave it."""
    arch = small(gc=5)
    frames = [4, 9, 2, 7, 3, 8, 5]
    ms = mels(71, frames)
    voices = [1 + u % 5 for u in range(7)]
    g, _ = make_gen(arch, 3, chunk=10)
    wavs = g.vocode(ms, gc_ids=voices)
    torch.cuda.synchronize()
    assert [tuple(w.shape) for w in wavs] == [(f * 8,) for f in frames]
    g1, _ = make_gen(arch, 1, chunk=10)
    g1.use_graph = False
    g1.build_graph(72)
    for u, m in enumerate(ms):
        g1.init_sessions()
        g1.begin([0], [m], gc_ids=[voices[u]], keys=[u])
        g1.step(frames[u] * 8)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(wavs[u].cpu().numpy(), g1.take(0, frames[u] * 8).cpu().numpy(), str(u))
    assert len(np.unique(np.concatenate([w.cpu().numpy() for w in wavs]))) > 16


# ---- test 11 -------------------------------------------------------------------------------------------
def test_device_dependent_refusals(lib, monkeypatch):
    monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    arch = small()
    B = 3
    ms = mels(81, [4, 4, 4])
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(40)
    args = (g._plan, ctypes.byref(g._params_c), g._ws.data_ptr())
    dense = torch.as_tensor(np.stack(ms), device='cuda')
    codes = torch.zeros(B, 4, dtype=torch.int32, device='cuda')
    # a run with a slot missing; prefill, score and lbwn_gen_set_mel after a begin
    g.init_sessions()
    g.begin([0, 2], [ms[0], ms[2]])
    with pytest.raises(_lib.LbwnError, match='only 2 of the 3 streams'):
        g._launch(4)
    assert lib.lbwn_gen_set_mel(*args, dense.data_ptr(), 4, _lib.stream_ptr()) == 22
    assert b'session mode' in lib.lbwn_last_error()
    assert lib.lbwn_gen_prefill(*args, codes.data_ptr(), 4, 4, _lib.stream_ptr()) == 22
    assert b'prefill: not supported in session mode' in lib.lbwn_last_error()
    logp = torch.zeros(B, 4, device='cuda')
    scratch = torch.zeros(lib.lbwn_gen_score_scratch_bytes(g._plan), dtype=torch.uint8, device='cuda')
    assert lib.lbwn_gen_score(*args, codes.data_ptr(), 4, 4, logp.data_ptr(), 4, scratch.data_ptr(),
                              _lib.stream_ptr()) == 22
    assert b'score: not supported in session mode' in lib.lbwn_last_error()
    g.begin([1], [ms[1]])
    g._launch(4)                                         # every stream has a session now
    # lbwn_gen_begin after lbwn_gen_set_mel; lbwn_gen_start clears both modes
    g.init_buffers(mel=np.stack(ms))
    with pytest.raises(_lib.LbwnError, match='exclusive'):
        g.begin([0], [ms[0]])
    g._launch(4)
    snap(g, 4)
    # a teacher loaded by lbwn_gen_start
    gt, _ = make_gen(arch, B, chunk=10, teacher_q=np.arange(5, dtype=np.int32))
    gt.build_graph(40)
    gt.init_buffers(mel=np.stack(ms))
    with pytest.raises(_lib.LbwnError, match='teacher'):
        gt.begin([0], [ms[0]])
    torch.cuda.synchronize()


# ---- the command line ----------------------------------------------------------------------------------
def test_generate_mel_list_end_to_end(tmp_path, monkeypatch):
    """generate.py --mel-list at batch 2 with a byte budget that splits the list into two groups writes, for
    every line, the wav WaveNetGen.vocode gives at batch 3 in one run (keys = list positions): the result
    depends neither on the batch size nor on the grouping."""
    import json
    import os
    import generate
    from scipy.io import wavfile
    from lbwn.ckpt import ckpt_file, save_tensors
    from tests.test_gpu_gen_lc import _PARAMS
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
        lines.append('%d\t%s%s' % (voices[u], tmp_path / ('m%d.npy' % u), '\tutt%d' % u if u % 2 else ''))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    hop, Lo = 8, arch['n_lc_out']
    lengths = [f * hop for f in frames]
    budget_mb = 13000 / 2 ** 20
    groups = generate.mel_list_groups(lengths, 2, 10, Lo, arch['lc_upsample'], int(budget_mb * 2 ** 20))
    assert groups == [[0, 1, 2], [3, 4]]
    out = generate.main(['--mel-list', str(tmp_path / 'list.txt'), '--mel-list-budget-mb', repr(budget_mb),
                         '--batch-size', '2', '--chunk-size', '10', '--seed', str(SEED), str(af), pfx,
                         str(tmp_path / 'out')])
    for u in range(5):
        np.testing.assert_array_equal(out[u], want[u], str(u))
        name = 'utt%d' % u if u % 2 else 'm%d' % u
        sr, x = wavfile.read(os.path.join(str(tmp_path / 'out'), name + '.wav'))
        assert sr == 16000
        np.testing.assert_array_equal(x, want[u])


def test_begin_of_more_streams_than_one_launch_lists(monkeypatch):
    """B = 130 without LC (the per-step form): one begin of all streams is two launches (128 entries each).
    With key = stream the run equals a fresh one started with those voices; a second begin's words carry
    every stream's own key and the step it happened at."""
    monkeypatch.delenv('LBWN_GEN_PERSIST', raising=False)
    arch = normalize_arch(dict(small(gc=5), n_lc_in=0, n_lc_out=0, lc_upsample=[]))
    B, n = 130, 5
    voices = [1 + (3 * b) % 5 for b in range(B)]
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(2 * n)
    g.init_buffers(gc_ids=[5] * B)
    g.begin(list(range(B)), gc_ids=voices, keys=list(range(B)))
    g.step(n)
    s1, l1 = snap(g, n)
    order = list(range(B - 1, -1, -1))
    g.begin(order, gc_ids=[voices[b] for b in order], keys=[1000 + b for b in order])
    words = g.tensor('sessions', torch.int64).view(B, 4).cpu().numpy()
    np.testing.assert_array_equal(words, [[n, 1000 + b, 0, 0] for b in range(B)])
    g.step(n)
    s2, _ = snap(g, 2 * n)
    assert not np.array_equal(s2[:, n:], s1)                     # other keys, other draws
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(n)
    g.init_buffers(gc_ids=voices)
    g.step(n)
    s0, l0 = snap(g, n)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(l1, l0)


# ---- a captured chunk is bound to the mode of its capture ----------------------------------------------
def test_dense_run_after_sessions_on_one_generator(form):
    """A chunk captured in session mode must not be replayed by a dense run on the same generator (it would
    project with the stale session words and the reserved stride, and key the draws by them), nor a dense
    chunk by a session run: vocode, then run(n, mel=) on the same object, then vocode again, each against a
    fresh generator, bit for bit."""
    arch = small(gc=5)
    B, n = 3, 41
    ms = mels(101, [4, 6, 3, 5])
    voices = [2, 5, 1, 4]
    dense = np.stack(mels(102, [5] * B))
    gc = [3, 1, 4]
    g, _ = make_gen(arch, B, chunk=10)
    first = [w.cpu().numpy() for w in g.vocode(ms, gc_ids=voices)]
    captured = g._graph
    assert captured is not None and g._graph_mode == (True, 10)
    assert g.max_steps >= n                                   # the plan is reused by the dense run
    g.run(n, gc_ids=gc, mel=dense)
    assert g._graph is not captured and g._graph_mode == (False, 10)
    s1, l1 = snap(g, n)
    again = [w.cpu().numpy() for w in g.vocode(ms, gc_ids=voices)]     # and back: the dense chunk is dropped
    assert g._graph_mode == (True, 10)
    f, _ = make_gen(arch, B, chunk=10)
    f.run(n, gc_ids=gc, mel=dense)
    s0, l0 = snap(f, n)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(l1, l0)
    for u in range(len(ms)):
        np.testing.assert_array_equal(again[u], first[u], str(u))


def test_dense_run_after_sessions_without_lc(form):
    """The same without LC, where only the draw's key is at stake: begin + a captured chunk, then
    init_buffers + step on the same generator equals a fresh one."""
    arch = normalize_arch(dict(small(gc=5), n_lc_in=0, n_lc_out=0, lc_upsample=[]))
    B, n = 3, 23
    g, _ = make_gen(arch, B, chunk=10)
    g.build_graph(2 * n)
    g.init_buffers(gc_ids=VOICES)
    g.step(7)
    g.begin([0, 2], gc_ids=[5, 4], keys=[11, 12])
    g.step(n)                                                 # captures in session mode
    assert g._graph_mode == (True, 10)
    g.init_buffers(gc_ids=VOICES)
    g.step(n)
    s1, l1 = snap(g, n)
    f, _ = make_gen(arch, B, chunk=10)
    f.build_graph(2 * n)
    f.init_buffers(gc_ids=VOICES)
    f.step(n)
    s0, l0 = snap(f, n)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(l1, l0)


# ---- the filtered draw in session mode -----------------------------------------------------------------
def test_recycled_slot_with_filtered_sampling(form):
    """Temperature, top-k and top-p set: the filtered twin of the draw takes key and base from the session
    words too.  A slot restarted mid-run equals stream 2 of a fresh dense run with the same settings, its
    neighbours the run without the restart; and the filter is live (the unfiltered run draws otherwise)."""
    arch = small(gc=5)
    B, n1, n2 = 3, 17, 25
    first, m_new = mels(111, [6, 4, 6]), mels(112, [4])[0]
    out = []
    for restart, filt in ((True, True), (False, True), (True, False)):
        g, _ = make_gen(arch, B, chunk=10)
        if filt:
            g.set_sampling(temperature=0.8, top_k=40, top_p=0.95)
        g.build_graph(n1 + n2)
        g.init_sessions()
        g.begin([0, 1, 2], first, gc_ids=VOICES, keys=[0, 1, 2])
        g.step(n1)
        if restart:
            g.begin([1], [m_new], gc_ids=[NEW_VOICE], keys=[2])
        g.step(n2)
        out.append(snap(g, n1 + n2))
    g, _ = make_gen(arch, B, chunk=10)
    g.set_sampling(temperature=0.8, top_k=40, top_p=0.95)
    g.build_graph(n2)
    dense = np.stack(mels(113, [4] * B))
    dense[2] = m_new
    g.init_buffers(gc_ids=[1, 2, NEW_VOICE], mel=dense)
    g.step(n2)
    sr, lr = snap(g, n2)
    (sa, la), (s0, l0), (su, _) = out
    np.testing.assert_array_equal(sa[1][n1:], sr[2])
    np.testing.assert_array_equal(la[1], lr[2])
    for b in (0, 2):
        np.testing.assert_array_equal(sa[b], s0[b])
        np.testing.assert_array_equal(la[b], l0[b])
    assert not np.array_equal(sa, su)
