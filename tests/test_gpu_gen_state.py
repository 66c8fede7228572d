"""State save / load / fan-out of the cached generator (lbwn_gen_state_save / _load) on
the GPU, in both execution forms.

Save and load are copies, so everything compared inside the GPU is compared bitwise: a run that is
rewound and repeated must draw the same samples and leave the same rings and logits, and the saved
bytes must be tests/state_ref.pack of the workspace tensors.  Where a load changes which stream
continues from which state (a permuted map, another plan, the fan-out prefill) the continuation is
checked against the oracle along the GPU's trajectory, with check_free_steps' near-tie allowance."""
import copy

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.arch import normalize_arch
from oracle import wavenet_ref as R
from tests import state_ref as S
from tests import test_gpu_gen_lc as LC
from tests.test_gpu_gen import form, make_gen, small  # noqa: F401  (form is a fixture)
from tests.test_gpu_gen_prefill import RING_BAR, SEED, check_free_steps, oracle_state, ring_error

pytestmark = pytest.mark.gpu


def status(g):
    return int(g.tensor('status', torch.int32).item())


def step_of(g):
    return int(g.tensor('step', torch.int64).item())


def snapshot(g, n):
    """Clones of what the last n steps left: (samples of those steps, rings, logits)."""
    torch.cuda.synchronize()
    t = step_of(g)
    return g.samples()[:, t - n:t].clone(), g.tensor('rings').clone(), g.logits().clone()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def blob_of_workspace(g):
    """state_ref.pack of the plan's own tensors: the pending code after a free step is that step's draw."""
    t = step_of(g)
    codes = g.samples()[:, t - 1].cpu().numpy()
    return S.pack(g.tensor('rings').cpu().numpy(), codes, t, g.arch, g.batch_sz)


def rewind(g, n0, k, check_blob=False):
    """n0 steps, save, k steps, load, the same k steps again: bitwise the first pass."""
    g.step(n0)
    st = g.save_state()
    rings0 = g.tensor('rings').clone()
    if check_blob:
        torch.cuda.synchronize()
        assert st.blob.cpu().numpy().tobytes() == blob_of_workspace(g).tobytes()
    g.step(k)
    first = snapshot(g, k)
    assert step_of(g) == n0 + k
    g.load_state(st)
    torch.cuda.synchronize()
    assert step_of(g) == n0 == st.step()
    assert torch.equal(g.tensor('rings'), rings0)
    g.step(k)
    second = snapshot(g, k)
    assert step_of(g) == n0 + k and status(g) == 0
    assert same(first, second), 'the repeated steps differ from the first pass'
    return st


def test_rewind_mid_ring(form):
    """B = 3, 21 steps (no multiple of a d > 1: every ring is mid-slot), save, 11 on, rewind, 11 again;
    the snapshot's bytes are the documented layout of the workspace tensors (n_res = 32: float4 path)."""
    g, _ = make_gen(small(), 3, chunk=16, graph=False)
    g.build_graph(64)
    g.init_buffers()
    rewind(g, 21, 11, check_blob=True)
    assert g.persistent == (form == 'persistent')


@pytest.mark.parametrize('k', [1, 9])
def test_rewind_two_stream_groups(k, form):
    """B = 20 with GC: two persistent groups of 10 (the second one's step counter sits behind the
    granules), or the per-step GEMM head; k = 1 is the load at the step after the one just run."""
    B = 20
    g, _ = make_gen(small(gc=5), B, chunk=16, graph=False)
    g.build_graph(64)
    g.init_buffers([1 + b % 5 for b in range(B)])
    rewind(g, 21, k)
    assert g.persistent == (form == 'persistent')


def permuted(rings, src):
    return [np.array(r[src]) for r in rings]


def test_permuted_load_one_step_later(form):
    """Run 21, save, run 1, load with src = [1, 2, 0]: every hand-off granule the extra step left carries
    tag 22, exactly what the loaded step 21 polls for -- a load that leaves the granules alone continues
    from another stream's values.  The continuation against the oracle along the GPU's trajectory."""
    arch, B, n0, k, src = small(), 3, 21, 5, [1, 2, 0]
    g, P = make_gen(arch, B, chunk=16, graph=False)
    g.build_graph(64)
    g.init_buffers()
    g.step(n0)
    st = g.save_state()
    torch.cuda.synchronize()
    traj = g.samples().cpu().numpy()[:, :n0].copy()
    saved = S.split_rings(S.unpack(st.blob.cpu().numpy(), g.arch)[0], g.arch, B)
    g.step(1)
    g.load_state(st, src)
    torch.cuda.synchronize()
    assert step_of(g) == n0 and status(g) == 0
    for got, want in zip(S.split_rings(g.tensor('rings').cpu().numpy(), g.arch, B), saved):
        assert got.tobytes() == want[src].tobytes()
    g.step(k)
    torch.cuda.synchronize()
    g.check_status()
    assert step_of(g) == n0 + k
    rings_ref = R.generate(arch, P, B, n0, seed=SEED, forced_q=traj, return_state=True)[-1]
    check_free_steps(g, lambda fq: R.generate(
        arch, P, B, k, seed=SEED, return_logits=True, forced_q=fq, start=n0, init_rings=permuted(rings_ref, src),
        init_q=traj[src, n0 - 1]), n0, k)


def test_load_into_a_plan_of_another_batch_size(form):
    """Plan A (B = 2, voices [2, 5]) prefills a 37-code prompt and saves; plan B (B = 5, voices
    [2, 5, 5, 2, 5]) starts and loads it with src = [0, 1, 1, 0, 1].  Streams 1 and 2 continue from one
    record with one voice and must still differ: the draw is keyed by the destination stream."""
    arch, n, k = small(gc=5), 37, 8
    ids_a, ids_b, src = [2, 5], [2, 5, 5, 2, 5], [0, 1, 1, 0, 1]
    prompt = np.random.default_rng(21).integers(0, 256, (2, n)).astype(np.int32)
    ga, P = make_gen(arch, 2, chunk=16, graph=False)
    ga.build_graph(n)
    ga.init_buffers(ids_a)
    ga.prefill(prompt)
    st = ga.save_state()
    assert st.n_streams == 2 and st.step() == n
    gb, _ = make_gen(arch, 5, chunk=16, graph=False)
    gb.build_graph(n + k)
    gb.init_buffers(ids_b)
    gb.load_state(st, src)
    gb.step(k)
    torch.cuda.synchronize()
    gb.check_status()
    assert gb.persistent == (form == 'persistent')
    assert step_of(gb) == n + k
    rings_ref = oracle_state('state_across_plans', arch, P, 2, prompt, ids_a)
    check_free_steps(gb, lambda fq: R.generate(
        arch, P, 5, k, seed=SEED, return_logits=True, forced_q=fq, start=n, init_rings=permuted(rings_ref, src),
        init_q=prompt[src, -1], gc_ids=ids_b), n, k)
    s = gb.samples().cpu().numpy()[:, n:n + k]
    assert not np.array_equal(s[1], s[2]), 'two streams forked from one record drew the same sequence'


def test_odd_widths_round_trip(form):
    """The arch2 widths (n_res 3: the 4-byte path, records padded to 16 bytes) with GC: run 13, save,
    init_buffers (zeroes), load: rings, codes and step are bitwise those before; the blob is the
    documented layout byte for byte."""
    arch = normalize_arch(dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=3, n_dil=4, n_skip=8, n_post=6,
                               n_gc_embed=8, n_gc_category=5, use_bias=True))
    g, _ = make_gen(arch, 2, chunk=16, graph=False)
    g.build_graph(32)
    g.init_buffers([2, 5])
    g.step(13)
    st = g.save_state()
    torch.cuda.synchronize()
    rings0 = g.tensor('rings').clone()
    blob = st.blob.cpu().numpy()
    assert blob.tobytes() == blob_of_workspace(g).tobytes()
    assert S.record_bytes(g.arch) == 384 and blob.size == 256 + 2 * 384
    g.init_buffers([2, 5])
    torch.cuda.synchronize()
    assert step_of(g) == 0 and not g.tensor('rings').any()
    g.load_state(st)
    torch.cuda.synchronize()
    assert step_of(g) == 13 and status(g) == 0
    assert torch.equal(g.tensor('rings'), rings0)
    assert torch.equal(g.save_state().blob, st.blob)          # the pending codes and the step, too


def test_lc_plan_rewind_across_the_cond_ring_wrap(form, monkeypatch):
    """The small LC arch, default NC = 64: run 40, save, run 40 (steps 40..79 cross the cond ring's
    wrap), load, run 40 again: the cond ring is projected again per sub-run, not part of the state."""
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    B = 3
    mel = np.random.default_rng(22).standard_normal((B, 10, 12)).astype(np.float32)
    g, _ = LC.make_gen(LC.small(), B, chunk=100)
    g.build_graph(80)
    g.init_buffers(mel=mel)
    assert g.tensor('lccond').numel() == 64 * 8 * B * 64
    rewind(g, 40, 40)
    assert g.persistent == (form == 'persistent')


def test_graph_replay_across_a_load(form):
    """chunk = 8, graph=True: step(16) captures the graph; save, step(16), load, step(16) -- the last call
    replays the graph captured before the load, which reads the step on the device.  A save captured in a
    graph of its own and replayed writes what an eager save writes."""
    g, _ = make_gen(small(), 3, chunk=8, graph=True)
    g.build_graph(64)
    g.init_buffers()
    g.step(16)
    assert g._graph is not None
    captured = g._graph
    st = g.save_state()
    g.step(16)
    first = snapshot(g, 16)
    g.load_state(st)
    g.step(16)
    second = snapshot(g, 16)
    assert g._graph is captured
    assert step_of(g) == 32 and status(g) == 0
    assert same(first, second)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        st_g = g.save_state()
    gr.replay()
    eager = g.save_state()
    torch.cuda.synchronize()
    assert st_g.step() == 32
    assert torch.equal(st_g.blob, eager.blob)


def test_device_refusals_set_status_6_and_change_nothing(form):
    """The C entry directly: a snapshot of an n_res = 16 arch into the n_res = 32 plan, and a map with an
    entry equal to state_streams.  Both are refused by the launch itself, before any index is used: the
    status is 6 and rings, codes and step stay bitwise what they were; init_buffers clears the status."""
    B = 3
    g, _ = make_gen(small(), B, chunk=16, graph=False)
    g.build_graph(32)
    g16, _ = make_gen(normalize_arch(dict(small(), n_res=16)), B, chunk=16, graph=False)
    g16.build_graph(32)
    g16.init_buffers()
    g16.step(5)
    other = g16.save_state()
    lib = g.lib

    def refused(blob, n_streams, m):
        g.init_buffers()
        g.step(5)
        before = g.save_state()
        rings0 = g.tensor('rings').clone()
        torch.cuda.synchronize()
        assert status(g) == 0
        _lib.check(lib.lbwn_gen_state_load(g._plan, g._ws.data_ptr(), blob.data_ptr(), n_streams, _lib.ptr(m),
                                           _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert status(g) == 6
        assert step_of(g) == 5
        assert torch.equal(g.tensor('rings'), rings0)
        assert torch.equal(g.save_state().blob, before.blob)
        with pytest.raises(RuntimeError, match='status 6'):
            g.check_status()
        g.init_buffers()
        torch.cuda.synchronize()
        assert status(g) == 0
        return before

    mine = refused(other.blob, B, None)
    refused(mine.blob, B, torch.tensor([0, 1, B], dtype=torch.int32, device='cuda'))
    refused(mine.blob, B, torch.tensor([0, -1, 1], dtype=torch.int32, device='cuda'))
    refused(mine.blob, B - 1, torch.tensor([0, 1, 1], dtype=torch.int32, device='cuda'))   # the header says 3


def test_fanout_prefill(form):
    """B = 6, voices [2, 5, 2, 5, 2, 5], a 37-code teacher: run(37 + 8, prefill='fanout') prefills the two
    voices once each and loads them into the six streams."""
    arch, B, n, k = small(gc=5), 6, 37, 8
    ids = [2, 5, 2, 5, 2, 5]
    teacher = np.random.default_rng(23).integers(0, 256, n).astype(np.int32)
    g, P = make_gen(arch, B, chunk=16, graph=False)
    g.teacher_mu = torch.as_tensor(teacher, device='cuda')
    g.build_graph(n + k)
    rings_ref = oracle_state('state_fanout', arch, P, B, teacher, ids)
    assert g.init_buffers(ids, prefill='fanout') == n
    torch.cuda.synchronize()
    assert step_of(g) == n and g._fan[1].batch_sz == 2
    err = ring_error(g, rings_ref)
    fan = g.tensor('rings').clone()
    assert g.init_buffers(ids, prefill=True) == n
    torch.cuda.synchronize()
    err_pf = ring_error(g, rings_ref)
    diff = float((g.tensor('rings') - fan).abs().max())
    print('fanout [%s]: ring error %.3g (prefill=True %.3g), max |fanout - prefill=True| %.3g' % (form, err, err_pf, diff))
    assert err <= RING_BAR, err
    n_run, wav, _ = g.run(n + k, gc_ids=ids, prefill='fanout')
    torch.cuda.synchronize()
    assert n_run == n + k and step_of(g) == n + k and status(g) == 0
    assert g.persistent == (form == 'persistent')
    np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], np.broadcast_to(teacher, (B, n)))
    want = np.broadcast_to(R.mu_decode_tf32(teacher, 256), (B, n))
    np.testing.assert_allclose(g.tensor('wav').view(B, g.max_steps).cpu().numpy()[:, :n], want, rtol=1e-6, atol=1e-6)
    check_free_steps(g, lambda fq: R.generate(
        arch, P, B, k, seed=SEED, return_logits=True, forced_q=fq, start=n, init_rings=copy.deepcopy(rings_ref),
        init_q=np.broadcast_to(teacher, (B, n))[:, -1], gc_ids=ids), n, k)


def test_fanout_prefill_with_a_shared_mel(form, monkeypatch):
    """The small LC arch without GC (one voice), B = 4, a shared 2-D mel, a 37-code teacher: the fan-out
    conditions its one prefilled stream on the same mel rows.  Against prefill=True of the same generator:
    the same step and outputs, and every layer's rings within 2 x RING_BAR of each other (each path is
    held to RING_BAR against the oracle, tests/test_gpu_gen_prefill_lc.py); the difference is printed."""
    monkeypatch.delenv('LBWN_GEN_LC_CHUNK', raising=False)
    B, n = 4, 37
    mel = np.random.default_rng(24).standard_normal((8, 12)).astype(np.float32)
    teacher = np.random.default_rng(25).integers(0, 256, n).astype(np.int32)
    g, _ = LC.make_gen(LC.small(), B, chunk=100, teacher_q=teacher)
    g.build_graph(64)
    out = []
    for pf in (True, 'fanout'):
        assert g.init_buffers(mel=mel, prefill=pf) == n
        torch.cuda.synchronize()
        assert step_of(g) == n and status(g) == 0
        np.testing.assert_array_equal(g.samples().cpu().numpy()[:, :n], np.broadcast_to(teacher, (B, n)))
        out.append((S.split_rings(g.tensor('rings').cpu().numpy(), g.arch, B), g.save_state().blob.clone()))
    assert g._fan[1].batch_sz == 1
    worst = max(float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(out[0][0], out[1][0]))
    print('fanout with mel [%s]: max relative ring difference against prefill=True %.3g' % (form, worst))
    assert worst <= 2 * RING_BAR, worst
    g.step(8)          # and the loaded plan runs on: mel rows, counters and granules are in place
    torch.cuda.synchronize()
    g.check_status()
    assert step_of(g) == n + 8
