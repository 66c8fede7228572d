"""numpy restatement of the generator's snapshot layout (lbwn_gen_state_save, include/lbwn.h; DESIGN
§4.24).  A helper module, not a test.

  header, 256 bytes: int32 magic "LBST", version 1, n_streams, n_blocks, n_block_layers, n_res, n_quant,
    record_bytes; int64 step at byte 32; zeros
  n_streams records of record_bytes = round_up_16(16 + 4·D·n_res), D = n_blocks·(2^n_block_layers - 1):
    int32 pending code, 12 zero bytes, the stream's rings in layer order, each fp32 [d][n_res]; zeros

`rings_flat` is the plan's "rings" tensor: layer-major, layer l with dilation d as [B][d][n_res].  Written
with the per-layer loop of the ring tests (oracle layer_index), not the kernel's closed form."""
import numpy as np

from oracle import wavenet_ref as R

MAGIC = 0x5453424c
VERSION = 1
HEADER = 256


def dilations(arch):
    return [R.layer_index(arch, l)[2] for l in range(R.n_layers(arch))]


def record_bytes(arch):
    return (16 + 4 * sum(dilations(arch)) * arch['n_res'] + 15) // 16 * 16


def state_bytes(arch, n_streams):
    return HEADER + n_streams * record_bytes(arch)


def pack(rings_flat, codes, step, arch, B):
    """The snapshot bytes (uint8 [state_bytes]) of rings_flat fp32 [sum_l B·d_l·n_res], codes int32 [B], step."""
    Cr, rb = arch['n_res'], record_bytes(arch)
    rings_flat = np.ascontiguousarray(rings_flat, np.float32).reshape(-1)
    out = np.zeros(state_bytes(arch, B), np.uint8)
    out[:32].view('<i4')[:] = [MAGIC, VERSION, B, arch['n_blocks'], arch['n_block_layers'], Cr, arch['n_quant'], rb]
    out[32:40].view('<i8')[0] = step
    recs = out[HEADER:].reshape(B, rb)
    recs[:, :4] = np.ascontiguousarray(codes, '<i4').reshape(B, 1).view(np.uint8)
    off, pos = 0, 16
    for d in dilations(arch):
        layer = rings_flat[off:off + B * d * Cr].reshape(B, d * Cr)
        recs[:, pos:pos + 4 * d * Cr] = layer.view(np.uint8)
        off += B * d * Cr
        pos += 4 * d * Cr
    assert off == rings_flat.size, (off, rings_flat.size)
    return out


def unpack(blob, arch):
    """(rings_flat fp32 in the plan's layout for B = the header's n_streams, codes int32 [B], step, B)."""
    blob = np.ascontiguousarray(blob, np.uint8).reshape(-1)
    w = blob[:32].view('<i4')
    Cr, rb = arch['n_res'], record_bytes(arch)
    B = int(w[2])
    assert [int(v) for v in w[:2]] == [MAGIC, VERSION], w[:2]
    assert [int(v) for v in w[3:8]] == [arch['n_blocks'], arch['n_block_layers'], Cr, arch['n_quant'], rb], w[:8]
    assert blob.size == state_bytes(arch, B) and not blob[40:HEADER].any()
    step = int(blob[32:40].view('<i8')[0])
    recs = blob[HEADER:].reshape(B, rb)
    codes = np.ascontiguousarray(recs[:, :4]).view('<i4').reshape(B).copy()
    parts, pos = [], 16
    for d in dilations(arch):
        parts.append(np.ascontiguousarray(recs[:, pos:pos + 4 * d * Cr]).view(np.float32).reshape(-1))
        pos += 4 * d * Cr
    return np.concatenate(parts), codes, step, B


def split_rings(rings_flat, arch, B):
    """The "rings" tensor as the oracle's list of [B][d][n_res] float64 arrays (generate's init_rings)."""
    Cr, out, off = arch['n_res'], [], 0
    flat = np.asarray(rings_flat, np.float64).reshape(-1)
    for d in dilations(arch):
        out.append(flat[off:off + B * d * Cr].reshape(B, d, Cr).copy())
        off += B * d * Cr
    assert off == flat.size
    return out
