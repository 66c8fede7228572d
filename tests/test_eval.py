"""Held-out evaluation without a GPU: lbwn_train_eval's refusals (all made before the device is
touched), the ctypes mirror of lbwn_eval_args, lbwn.data.eval_batches' exact-coverage deal,
tests/eval_ref.py against the oracle's own loss, DPContext.reduce_eval over gloo, and train.py's
option errors."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

from lbwn import _lib
from lbwn.data import eval_batches
from oracle import wavenet_ref as R
from tests import eval_ref as E
from tests.conftest import ROOT


# ---- C ABI ------------------------------------------------------------------------------------------
def test_eval_args_mirror_matches_header():
    txt = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    body = re.search(r'typedef struct lbwn_eval_args \{(.*?)\} lbwn_eval_args;', txt, re.S).group(1)
    fields = [re.findall(r'\w+', piece)[-1] for decl in body.split(';') for piece in decl.split(',') if piece.strip()]
    assert fields == [n for n, _ in _lib.EvalArgs._fields_], fields


def _plan(lib, arch, B, T):
    a = _lib.Arch()
    for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post', 'n_gc_embed',
              'n_gc_category', 'n_lc_in', 'n_lc_out'):
        setattr(a, k, int(arch[k]))
    ups = arch['lc_upsample'] if arch['n_lc_out'] > 0 else []
    a.n_lc_upsample = len(ups)
    for i, s in enumerate(ups):
        a.lc_upsample[i] = int(s)
    a.use_bias = int(arch['use_bias'])
    h = ctypes.c_void_p()
    _lib.check(lib.lbwn_plan_create(ctypes.byref(a), B, T, ctypes.byref(h)))
    return h


def test_train_eval_refusals_without_gpu(lib):
    """Every refusal of include/lbwn.h is EINVAL with the argument's name in lbwn_last_error, on a
    host-only plan and with pointers nothing ever dereferences."""
    T = 64
    h = _plan(lib, E.ARCHS['chain'](), 2, T)
    hc = _plan(lib, E.ARCHS['cond'](), 2, T)
    P = _lib.Params()
    ok = dict(wav_q=0x1000, ids=0x2000, mel=None, save=0x3000, acc=0x4000, nll=None, ld_nll=0, by_voice=None,
              n_bins=0, status=None, scratch=0x5000)

    def refused(word, plan=h, params=P, ws=0x6000, args=True, size=None, **kw):
        a = _lib.EvalArgs(**dict(ok, **kw))
        if size is not None:
            a.struct_size = size
        ret = lib.lbwn_train_eval(plan, ctypes.byref(params) if params is not None else None, ws,
                                  ctypes.byref(a) if args else None, None)
        msg = lib.lbwn_last_error().decode()
        assert ret == 22 and word in msg, (ret, word, msg)

    refused('plan', plan=None)
    refused('params', params=None)
    refused('workspace', ws=None)
    refused('args', args=False)
    refused('struct_size', size=ctypes.sizeof(_lib.EvalArgs) - 8)
    for name in ('wav_q', 'ids', 'save', 'acc', 'scratch'):
        refused(name, **{name: None})
    refused('mel', plan=hc)
    refused('ld_nll', nll=0x7000, ld_nll=T - 1)
    refused('n_bins', by_voice=0x8000, n_bins=0)
    refused('acc', acc=0x4004)
    refused('by_voice', by_voice=0x8004, n_bins=3)
    refused('scratch', scratch=0x5008)
    # the scratch size: 0 for a NULL plan; the bins add the voice partials and the row values
    assert lib.lbwn_train_eval_scratch_bytes(None, 5) == 0
    s0 = lib.lbwn_train_eval_scratch_bytes(h, 0)
    s5 = lib.lbwn_train_eval_scratch_bytes(h, 5)
    assert s0 == 32 * 32 and s5 > s0 and s0 % 256 == 0 and s5 % 256 == 0      # M = 128: 32 blocks of 4 rows
    # any n_quant that is a multiple of 4 makes a plan (the 1024 bound is the backward's)
    lib.lbwn_plan_destroy(_plan(lib, E.ARCHS['q1028'](), 2, 16))
    for p in (h, hc):
        lib.lbwn_plan_destroy(p)


# ---- the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['chain', 'cond'])
def test_eval_ref_matches_oracle_loss(name):
    arch, P, S, slices = E.case(name)
    (s,), _ = E.run(arch, P, slices, S, E.N_BINS)
    st, _ = R.loss_fcn(arch, P, s['logits'], slices[0][0], slices[0][1], 0.0)
    assert s['acc'][1] == st['n_valid'] and s['acc'][2] == st['sum_absdiff']
    np.testing.assert_allclose(s['acc'][0], st['sum_xent'], rtol=1e-13)
    assert np.all(s['nll'][~s['scored']] == 0) and not s['scored'][:, -1].any()
    np.testing.assert_allclose(s['by_voice'].sum(axis=0), s['acc'][:2], rtol=1e-13)
    ids = slices[0][1]
    assert s['by_voice'][0, 1] == np.sum(ids[:, 1:] >= E.N_BINS)     # ids 4 and 5 -> bin 0


def test_score_first_max_tie_rule():
    lg = np.zeros((1, 3, 8))
    lg[0, 0, [5, 2]] = 1.0
    s = E.score(lg, np.array([[0, 2, 7]], np.int32), np.array([[0, 1, 1]], np.int32))
    assert s['argmax'][0, 0] == 2 and s['acc'][3] == 1 and s['acc'][2] == 7 and s['gap'][0, 0] == 0


GAP_CASES = [('chain', {}), ('chain', dict(n_slices=2)), ('per_layer', {}), ('cond', {}), ('no_bias', {}),
             ('q64', dict(T=16, invalid=3)), ('q260', dict(T=16, invalid=3)), ('q1028', dict(T=16, invalid=3)),
             ('chain', dict(B=1, T=5, invalid=1)), ('chain', dict(B=2, T=2, invalid=1)), ('chain', dict(pseed=7))]


@pytest.mark.parametrize('name,kw', GAP_CASES)
def test_top2_gap_shares(name, kw):
    """The oracle alone: the share of scored rows whose float64 top-2 logit gap is below 1e-3 (the rows
    tests/test_gpu_eval.py leaves out of the argmax totals) stays within 5 % for the committed seeds,
    and the base chain case has none: with the committed seeds its smallest gap is 1.067e-2 (asserted
    above 8e-3, 80x the logit tolerance of 1e-4), so no row of it is left out of the argmax totals.
    Shares: chain 0, chain two slices 0 / 0, per_layer 1.1 %, cond 0 (smallest gap 1.5e-3), no_bias
    4.3 %, q64 / q260 / q1028 0, (1, 5) 0, (2, 2) 0, chain with parameter seed 7: 0."""
    arch, P, S, slices = E.case(name, **kw)
    scores, _ = E.run(arch, P, slices, S)
    for s in scores:
        g = s['gap'][s['scored']]
        assert g.size and np.mean(g <= 1e-3) <= 0.05
        if name not in ('per_layer', 'no_bias'):
            assert g.min() > 1e-3
    if name == 'chain' and not kw:
        assert scores[0]['gap'][scores[0]['scored']].min() > 8e-3


# ---- eval_batches -----------------------------------------------------------------------------------
def _catalogue(seed, hop, n_files, F, n_mel=0, short=True):
    """Files whose sample values name (file, position): value = 100000 * file + position."""
    rng = np.random.default_rng(seed)
    files = []
    for i in range(n_files):
        n = int(rng.integers(F, 6 * F)) if not (short and i == 1) else F - 1 - int(rng.integers(0, 3))
        n += int(rng.integers(0, hop))                       # a tail the dealer trims to the hop
        wav = (100000 * (i + 1) + np.arange(n)).astype(np.int64)
        mel = np.full((n // hop, n_mel), i + 1, np.float32) if n_mel else None
        files.append((int(rng.integers(1, 9)), wav, mel))
    return files


def _expected(files, hop, F):
    want = []
    for vid, wav, _ in files:
        n = len(wav) - len(wav) % hop
        if n >= F:
            want.append(wav[F - 1:n])
    return np.sort(np.concatenate(want)) if want else np.zeros(0, np.int64)


@pytest.mark.parametrize('seed,hop,B,T,n_files', [(0, 4, 3, 32, 9), (1, 1, 2, 17, 7), (2, 8, 4, 64, 2)])
def test_eval_batches_deals_every_id_exactly_once(seed, hop, B, T, n_files):
    """Three random catalogues (hop 4, 1, 8; one file shorter than F in each; the last smaller than
    one batch): the samples dealt with a non-zero id are exactly the samples F-1.. of every file of
    length >= F, each once; the deal is finite and ends in the step that dealt the last of them."""
    F = 13
    n_mel = 3 if hop > 1 else 0
    files = _catalogue(seed, hop, n_files, F, n_mel)
    log = io.StringIO()
    steps = list(eval_batches(files, B, T, F, hop, n_mel, log=log))
    assert 'skipping' in log.getvalue()
    got = np.sort(np.concatenate([w[i != 0] for _, w, _, i in steps]))
    assert np.array_equal(got, _expected(files, hop, F))
    assert np.count_nonzero(steps[-1][3]) > 0                  # no all-masked step at the end
    for _, w, m, i in steps:
        assert w.shape == (B, T) and i.shape == (B, T)
        assert np.all(i[w < 100000] == 0)                      # filler samples (zeros) are all masked
        assert (m is None) == (n_mel == 0) and (m is None or m.shape == (B, T // hop, n_mel))
    vids = {int(w) // 100000: v for v, ww, _ in files for w in ww[:1]}
    for _, w, _, i in steps:                                   # every dealt id is its file's voice id
        live = i != 0
        assert np.array_equal(i[live], np.array([vids[int(x) // 100000] for x in w[live]], np.int32))


def test_eval_batches_skips_voice_id_zero_files():
    """A file whose voice id is 0 (the mask value) holds nothing to score: it is skipped with a warning,
    in the middle of the catalogue and at its end, so the deal is that of the catalogue without such
    files and still ends in a step that dealt a non-zero id."""
    F = 13
    files = _catalogue(3, 1, 6, F, short=False)
    zero = lambda k: (0, np.arange(40 * F, dtype=np.int64) + 100000 * k, None)   # noqa: E731
    log = io.StringIO()
    with_zero = list(eval_batches(files[:2] + [zero(7)] + files[2:] + [zero(8), zero(9)], 2, 16, F, log=log))
    plain = list(eval_batches(files, 2, 16, F, log=io.StringIO()))
    assert log.getvalue().count('voice id 0') == 3
    assert len(with_zero) == len(plain) and np.count_nonzero(with_zero[-1][3]) > 0
    for a, b in zip(with_zero, plain):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert list(eval_batches([zero(1)], 2, 16, F, log=io.StringIO())) == []


def test_eval_batches_empty_and_rows():
    F = 13
    assert list(eval_batches([], 2, 16, F)) == []
    assert list(eval_batches([(3, np.arange(F - 1), None)], 2, 16, F, log=io.StringIO())) == []
    files = _catalogue(5, 4, 8, F, 2)
    one = list(eval_batches(files, 4, 32, F, 4, 2, log=io.StringIO()))
    parts = [list(eval_batches(files, 4, 32, F, 4, 2, rows=slice(2 * r, 2 * r + 2), log=io.StringIO())) for r in (0, 1)]
    assert len(parts[0]) == len(parts[1]) == len(one)
    for k, (cnt, w, m, i) in enumerate(one):
        for name, full, idx in (('wav', w, 1), ('mel', m, 2), ('ids', i, 3)):
            assert np.array_equal(np.concatenate([parts[0][k][idx], parts[1][k][idx]]), full), name
        assert parts[0][k][0] == parts[1][k][0] == cnt


# ---- reduce_eval over gloo ----------------------------------------------------------------------------
def _reduce_worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    from lbwn.dist import DPContext
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dp = DPContext(world, rank, rank)
    acc = torch.tensor([1.5 + rank, 10.0 + rank, 7.0 * rank, 3.0], dtype=torch.float64)
    bv = torch.arange(10, dtype=torch.float64).view(5, 2) * (rank + 1) + 2.0 ** -40
    status = torch.tensor([rank * 2], dtype=torch.int32)
    dp.reduce_eval(acc, bv, status)
    alone = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64) * (rank + 1)
    dp.reduce_eval(alone)
    if rank == 0:
        np.savez(out, acc=acc.numpy(), bv=bv.numpy(), status=status.numpy(), alone=alone.numpy())
    dist.destroy_process_group()


def test_reduce_eval_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    from lbwn.dist import DPContext
    out = str(tmp_path / 're.npz')
    port = 29500 + (os.getpid() + 29) % 1000
    mp.spawn(_reduce_worker, args=(2, port, out), nprocs=2, join=True)
    r = np.load(out)
    assert np.array_equal(r['acc'], [4.0, 21.0, 7.0, 6.0])
    assert np.array_equal(r['bv'], np.arange(10, dtype=np.float64).reshape(5, 2) * 3 + 2.0 ** -39)
    assert int(r['status'][0]) == 2 and np.array_equal(r['alone'], [3.0, 6.0, 9.0, 12.0])
    acc = torch.ones(4, dtype=torch.float64)
    DPContext().reduce_eval(acc, None)                          # one process: untouched
    assert torch.equal(acc, torch.ones(4, dtype=torch.float64))


# ---- train.py ---------------------------------------------------------------------------------------
def test_train_valid_option_errors(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
    import train
    arch, par = os.path.join(ROOT, 'par', 'arch3.json'), os.path.join(ROOT, 'par', 'par1.json')
    tail = [str(tmp_path / 'ck'), arch, par, 'none.txt']
    for argv, word in ((['--valid-interval', '5'], '--valid-interval needs --valid-file'),
                       (['--valid-batches', '2'], '--valid-batches needs --valid-file'),
                       (['--valid-ema', '--ema-decay', '0.9'], '--valid-ema needs --valid-file'),
                       (['--eval-only', '--resume-step', '3'], '--eval-only needs --valid-file'),
                       (['--valid-file', 'v.txt', '--valid-ema'], '--valid-ema needs an EMA'),
                       (['--valid-file', 'v.txt', '--valid-interval', '0'], 'must be >= 1'),
                       (['--valid-file', 'v.txt', '--valid-batches', '0'], 'must be >= 1'),
                       (['--valid-interval', '0'], '--valid-interval needs --valid-file'),
                       (['--valid-file', 'v.txt', '--eval-only'], '--eval-only needs --resume-step')):
        with pytest.raises(SystemExit) as e:
            train.main(argv + tail)
        assert e.value.code == 1
        assert word in capsys.readouterr().err, argv
    a = train.get_args(['--valid-file', 'v.txt', 'p', 'a', 'b', 'c'])
    assert train.valid_options(train.override_par(a, {})) == ('v.txt', 1000, None, False)
    assert train.valid_options(dict(valid_file='w.txt', valid_interval=7, valid_batches=3, valid_ema=True,
                                    ema_decay=0.99)) == ('w.txt', 7, 3, True)
    assert train.valid_options({}) is None
