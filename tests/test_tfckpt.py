"""TF V2 checkpoint bundles (lbwn/tfckpt.py): CRC-32C known answers, write -> read round trips,
corruption detection, and restore through the drop-in Checkpoint (ckpt.py:66-81).

Byte-level parity with a TensorFlow-written bundle is unpinned: TF is not importable here and the
reference ships no checkpoint; the CRC is pinned by the RFC 3720 / iSCSI vectors."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'lb-wavenet_amd'))
from lbwn import ckpt, tfckpt  # noqa: E402


def test_crc32c_known_answers():
    assert tfckpt.crc32c(b'123456789') == 0xE3069283
    assert tfckpt.crc32c(b'') == 0
    assert tfckpt.crc32c(bytes(32)) == 0x8A9136AA              # RFC 3720 B.4
    assert tfckpt.crc32c(b'\xff' * 32) == 0x62A8AB43
    assert tfckpt.crc32c(bytes(range(32))) == 0x46DD794E
    assert tfckpt.crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C


def test_crc32c_chunked_equals_bytewise():
    rng = np.random.default_rng(3)
    for n in (8 * 4096, 8 * 4096 + 1, 123457):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert tfckpt.crc32c(data) == tfckpt._raw(0xFFFFFFFF, data) ^ 0xFFFFFFFF
        # continuing a CRC over a split equals the CRC of the whole
        assert tfckpt.crc32c(data[n // 3:], tfckpt.crc32c(data[:n // 3])) == tfckpt.crc32c(data)


def test_mask_roundtrip():
    for c in (0, 1, 0xE3069283, 0xFFFFFFFF):
        assert tfckpt.unmask(tfckpt.mask(c)) == c


def _tensors():
    rng = np.random.default_rng(0)
    t = {'GLOBAL_STEP': np.array(1234, dtype=np.int32), 'VALID_SAMPLES': np.array(99, dtype=np.int32),
         'PRE_0': rng.standard_normal((256, 32)).astype(np.float32),
         'SAVE_512_4_9': rng.standard_normal((8, 512, 32)).astype(np.float32),
         'ids': rng.integers(-5, 1 << 40, (7,), dtype=np.int64), 'EMPTY': np.zeros((0, 3), np.float32),
         'POST1_0/Adam_1': rng.standard_normal((512, 512)).astype(np.float32)}
    for b in range(5):
        for l in range(40):   # enough keys for several 4-KiB index data blocks
            t['SIGNAL_%d_%d' % (b, l)] = rng.standard_normal((2, 4, 4)).astype(np.float32)
    return t


def test_bundle_roundtrip(tmp_path):
    t = _tensors()
    pfx = str(tmp_path / 'model.net-1000')
    tfckpt.write_bundle(pfx, t)
    assert os.path.getsize(pfx + '.index') > 4096
    got = tfckpt.read_bundle(pfx)
    assert set(got) == set(t)
    for k, v in t.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        np.testing.assert_array_equal(got[k], v)


def test_bundle_layout(tmp_path):
    """The index's footer, magic and header entry sit where TF's table reader looks for them."""
    pfx = str(tmp_path / 'x')
    tfckpt.write_bundle(pfx, {'B': np.arange(3, dtype=np.float32), 'A': np.ones(2, np.int64)})
    idx = open(pfx + '.index', 'rb').read()
    assert struct.unpack('<Q', idx[-8:])[0] == tfckpt.MAGIC
    data = open(pfx + tfckpt.DATA_SUFFIX, 'rb').read()
    assert data == np.ones(2, np.int64).tobytes() + np.arange(3, dtype=np.float32).tobytes()   # keys sorted
    footer = idx[-48:-8]
    off, pos = tfckpt._get_varint(footer, 0)
    _, pos = tfckpt._get_varint(footer, pos)
    index_block = tfckpt._read_block(idx, footer[pos:], True)
    keys = [k for _, h in tfckpt._block_entries(index_block)
            for k, _ in tfckpt._block_entries(tfckpt._read_block(idx, h, True))]
    assert keys == [b'', b'A', b'B']


def test_bundle_corruption_detected(tmp_path):
    pfx = str(tmp_path / 'c')
    tfckpt.write_bundle(pfx, {'W': np.arange(64, dtype=np.float32)})
    with open(pfx + tfckpt.DATA_SUFFIX, 'r+b') as f:
        f.seek(17)
        f.write(b'\x7f')
    with pytest.raises(ValueError, match='checksum'):
        tfckpt.read_bundle(pfx)
    assert tfckpt.read_bundle(pfx, verify=False)['W'].shape == (64,)
    with open(pfx + '.index', 'r+b') as f:
        f.seek(-1, 2)
        f.write(b'\x00')
    with pytest.raises(ValueError, match='magic'):
        tfckpt.read_bundle(pfx)


def test_checkpoint_restores_tf_bundle(tmp_path):
    """Checkpoint.restore() at '<ckpt_path>-<step>' reads the reference's bundle when no
    safetensors file is there; TF's int32 scalar counters land in the [1] int64 counters."""
    t = _tensors()
    tfckpt.write_bundle(str(tmp_path / 'run.net-1000'), t)
    dst = {'PRE_0': torch.zeros(256, 32), 'SAVE_512_4_9': torch.zeros(8, 512, 32),
           'GLOBAL_STEP': torch.zeros(1, dtype=torch.int64)}
    c = ckpt.Checkpoint(str(tmp_path / 'run.net'), 5, 1000)
    c.add_saveable_objects(dst)
    c.restore()
    np.testing.assert_array_equal(dst['PRE_0'].numpy(), t['PRE_0'])
    np.testing.assert_array_equal(dst['SAVE_512_4_9'].numpy(), t['SAVE_512_4_9'])
    assert int(dst['GLOBAL_STEP'][0]) == 1234


@pytest.mark.parametrize('use_bias', [True, False])
def test_tf_bundle_import_loads_exactly_the_layout(tmp_path, use_bias):
    """A TF V2 bundle holding a reference net's variables (serial names, int32 scalar counters;
    use_bias = false: no *_BIAS variable) restores into WaveNetTrain: the bundle's names are exactly
    the net's saveable names -- none missing, none extra -- and every tensor arrives bit for bit."""
    from lbwn.arch import normalize_arch
    from lbwn.tmodel import WaveNetTrain
    arch = normalize_arch(dict(n_blocks=1, n_block_layers=3, n_quant=256, n_res=8, n_dil=8, n_skip=16, n_post=8,
                               n_gc_embed=4, n_gc_category=3, n_lc_in=5, n_lc_out=6, lc_upsample=[2, 2],
                               use_bias=use_bias))
    net = WaveNetTrain(**arch, batch_sz=2, l2_factor=0.0, device='cpu', ckpt_path=str(tmp_path / 'run.net'),
                       resume_step=1000)
    rng = np.random.default_rng(1)
    t = {n: rng.standard_normal(tuple(v.shape)).astype(np.float32) for n, v in net.vars.items()}
    t.update({n: rng.standard_normal(tuple(v.shape)).astype(np.float32) for n, v in net.save_vars.items()})
    t['GLOBAL_STEP'] = np.array(1000, dtype=np.int32)
    t['VALID_SAMPLES'] = np.array(4242, dtype=np.int32)
    assert any('BIAS' in n for n in t) == use_bias
    tfckpt.write_bundle(str(tmp_path / 'run.net-1000'), t)
    loaded = net.restore()
    assert set(loaded) == set(t) == set(net.state_tensors())
    for n, v in net.vars.items():
        np.testing.assert_array_equal(v.numpy(), t[n], err_msg=n)
    for n, v in net.save_vars.items():
        np.testing.assert_array_equal(v.numpy(), t[n], err_msg=n)
    assert int(net.counters[0]) == 1000 and int(net.counters[1]) == 4242 and net.global_step_host == 1000


def test_export_and_cli_roundtrip(tmp_path):
    st = {'PRE_0': torch.randn(256, 32), 'GLOBAL_STEP': torch.tensor([77], dtype=torch.int64),
          'VALID_SAMPLES': torch.tensor([5], dtype=torch.int64)}
    ckpt.save_tensors(str(tmp_path / 'a-7.safetensors'), st)
    tfckpt.main(['export', str(tmp_path / 'a-7'), str(tmp_path / 'tf-7')])
    got = tfckpt.read_bundle(str(tmp_path / 'tf-7'))
    assert got['GLOBAL_STEP'].shape == () and got['GLOBAL_STEP'].dtype == np.int32 and int(got['GLOBAL_STEP']) == 77
    tfckpt.main(['import', str(tmp_path / 'tf-7'), str(tmp_path / 'b-7')])
    back = ckpt.load_tensors(str(tmp_path / 'b-7'))
    torch.testing.assert_close(back['PRE_0'], st['PRE_0'], rtol=0, atol=0)
