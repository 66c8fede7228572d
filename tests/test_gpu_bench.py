"""bench.py's plain run on the GPU: the result line and --dump-outputs (arch3 at B=2, run
in-process so that no second interpreter starts).  The dealer masks the first receptive field
(5115 positions) of every stream, so with T=4096 slice 0 has no valid sample, slice 1 some and
slices 2.. all: the runs below end on a slice with valid samples."""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

B, T, STEPS, WARMUP = 2, 4096, 3, 1
NAMES = ('xent', 'stats', 'grads', 'params', 'save')


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _run(extra):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = _bench().main(['--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP), '--arch',
                            os.path.join(ROOT, 'par', 'arch3.json'), '--batch', str(B), '--slice', str(T)] + extra)
    assert rc == 0
    lines = buf.getvalue().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """One plain run that dumps its outputs: (result line, directory)."""
    d = str(tmp_path_factory.mktemp('dump'))
    return _run(['--dump-outputs', d]), d


def test_plain_result_line(run):
    """A plain run reports the headline only: --steps timed steps, ms_per_step consistent with
    value, and none of the --full sub-objects."""
    line = run[0]
    assert line['steps'] == STEPS and line['warmup'] == WARMUP
    assert line['unit'] == 'audio samples/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] > 0
    np.testing.assert_allclose(line['value'], B * T / (line['ms_per_step'] / 1000.0), rtol=1e-12)
    for k in ('roofline', 'roofline_dilconv', 'warmup_probe_ms', 'gen', 'c1', 'c4', 'c5_per_gpu', 'cpu_baseline'):
        assert k not in line


def test_dump_outputs_files(run):
    """--dump-outputs writes the last step's mean cross-entropy, stats, gradients, parameters and SAVE rows as
    finite float32 arrays of the net's sizes, under the size limit."""
    from lbwn.arch import ParamLayout, load_arch, save_layout
    bench = _bench()
    arch = load_arch(os.path.join(ROOT, 'par', 'arch3.json'))
    n = ParamLayout(arch).n_total
    d = run[1]
    assert sorted(os.listdir(d)) == sorted(x + '.npy' for x in NAMES)
    arrs = {x: np.load(os.path.join(d, x + '.npy')) for x in NAMES}
    assert sum(os.path.getsize(os.path.join(d, x + '.npy')) for x in NAMES) <= 64 * 10 ** 6
    for x, a in arrs.items():
        assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), x
    assert arrs['xent'].shape == (1,) and arrs['stats'].shape == (4,)
    assert arrs['grads'].shape == (n,) and arrs['params'].shape == (n,)
    assert arrs['save'].shape == (save_layout(arch, B)[1],)
    assert np.abs(arrs['grads']).max() > 0
    # stats = (Σxent, n_valid, ...); an untrained net's cross-entropy is near ln 256
    assert 0 < arrs['stats'][1] <= B * T
    np.testing.assert_allclose(arrs['xent'][0], arrs['stats'][0] / arrs['stats'][1], rtol=1e-6)
    assert 1.0 < arrs['xent'][0] < 2 * np.log(256)
    assert bench.DUMP_LIMIT <= 64 * 10 ** 6


def test_dump_outputs_repeat(tmp_path):
    """The same arguments give the same inputs.  The warmup step sees the fully masked slice 0: its
    gradient is the L2 term alone, elementwise, so both runs enter the timed step with identical
    weights.  That step's SAVE rows, cross-entropy and raw gradients then depend only on its inputs
    (slice 1), and two runs differ by f32 summation order alone: activations are O(1) and the
    kernels are held to 1e-5 of float64 elsewhere in the suite, so 1e-4 absolute on SAVE and 1e-4
    of the largest gradient leave room; a different input slice would move them by O(1)."""
    a, b = [], []
    for out, tag in ((a, 'a'), (b, 'b')):
        d = str(tmp_path / tag)
        _bench().main(['--gpus', '1', '--steps', '1', '--warmup', '1', '--arch', os.path.join(ROOT, 'par', 'arch3.json'),
                       '--batch', str(B), '--slice', str(T), '--dump-outputs', d])
        out.append({x: np.load(os.path.join(d, x + '.npy')) for x in NAMES})
    a, b = a[0], b[0]
    assert 0 < a['stats'][1] == b['stats'][1] < B * T
    assert np.abs(a['grads']).max() > 0
    np.testing.assert_allclose(a['xent'], b['xent'], rtol=1e-5)
    np.testing.assert_allclose(a['save'], b['save'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(a['grads'], b['grads'], rtol=0, atol=1e-4 * np.abs(a['grads']).max())


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An array over its share of the limit is written as the fixed seeded sample of its elements."""
    bench = _bench()
    share = bench.DUMP_LIMIT // 5 // 4
    big = torch.arange(share + 1000, dtype=torch.float32, device='cuda')
    small = torch.ones(4, device='cuda')
    net = types.SimpleNamespace(flat=small, save_flat=small)
    for tag in 'ab':
        bench.dump_outputs(str(tmp_path / tag), net, big, small)
    g = np.load(str(tmp_path / 'a' / 'grads.npy'))
    assert g.dtype == np.float32 and g.shape == (share,)
    assert (np.diff(g) > 0).all() and g[-1] <= share + 999       # distinct elements, in order
    assert (g == np.load(str(tmp_path / 'b' / 'grads.npy'))).all()
    assert np.load(str(tmp_path / 'a' / 'params.npy')).shape == (4,)
