// Tile and image constants, kernel-argument structs and the device helpers that more than one of
// the layer translation units (layer.hip, pack.hip, chain_fwd.hip, chain_bwd.hip) use.  Everything
// here is constexpr or __forceinline__ inside an anonymous namespace: each TU gets its own copy, and
// kernel symbols keep their _ZN12_GLOBAL__N_1 names.
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LP = LBWN_LAYER_POS;  // positions per tile (4 waves × 32)
constexpr int XS = 36;              // padded LDS row for 32-channel tiles (b128 conflict-free)
constexpr int WS = 68;              // padded row of the [64 in][64 out] conv weight image
constexpr int DS = 68;              // dv tile row [pos][64]
constexpr int WIMG = 64 * WS + 32 * XS + 96;  // packed per-layer image (floats), multiple of 4
constexpr int SLAB = 2048 + 2048 + 1024 + 96;
constexpr int RED_PARTS = 32;       // deferred reduction: parts prefetched per thread (8 lanes × 32)

// Compact kernel arguments (the full lbwn_layer_args by value spilled ~100 SGPRs).
struct FwdK {
  const float* x_in; float* x_out; float* z; const float* wpack;
  const float* gc_tab; const int* ids; const float* cond;
  long ldz, ldcond, gc_ld;
  int B, T, H, d, Cr, Cd;
};
struct BwdK {
  const float* x_in; const float* wpack; const float* dz_skip;
  const float* g_a; const float* g_c0; float* out_a; float* out_c0; float* slab;
  const float* gc_tab; const int* ids; const float* cond; float* dv_out; float* gc_dtab;
  long lddz, ldcond, lddv, gc_ld;
  int B, T, H, d, Cr, Cd, g_d, slab_stride;
};
// Standalone slab reduction (runs on an auxiliary stream, off the layer chain).
struct RedK {
  const float* slab; float* dsig; float* dgate; float* dres; float* dbsig; float* dbgate; float* dbres;
  int nparts, stride, Cr, Cd;
};

// ---- weight images (built by pack.hip) ---------------------------------------------------
// Split image for the forward chain's bf16-split conv / residual, bf16 units:
//   WT[o (sig 0..31 | gate 32..63)][tap][plane][in 0..31]  (row XW_ROW = 192 + 8 pad: rows 100
//     dwords apart, conflict-free b128 fragment reads)
//   RT[out][plane][kk]  (row XR_ROW = 96 + 8 pad), kk = 16s + 8h + j holds z channel
//     16s + 8(j>>2) + 4h + (j&3): the k order of a 32x32 accumulator used as the B operand
//     (registers 8s..8s+7 of lane half h), cdna_hip_programming §3
//   then bs[64], br[32] as f32.
constexpr int XW_ROW = 200, XR_ROW = 104;
constexpr int XB_OFF = 64 * XW_ROW + 32 * XR_ROW;             // bf16 offset of the f32 biases
// bf16 elements per layer image, padded to 32 whole 1-KiB LDS-DMA pieces (the pad is never read)
constexpr int XIMG_US = (XB_OFF + 2 * 96 + 511) / 512 * 512;
constexpr int XIMG_F = XIMG_US / 2;                            // = 8192 floats
static_assert(XIMG_F % 256 == 0 && XB_OFF % 8 == 0, "x3 image alignment");

// Split image of a layer's LC projection for the forward chain's in-chain LC term
// (tmodel.py:155-160: v_k += lc·LC_k), bf16 units: LCT[o (sig 0..31 | gate 32..63)][plane][k 0..79]
// in rows of LC_ROW = 3·80 + 8 pad (124 dwords: 4·odd, so every 16-lane ds_read_b128 group of the
// A-fragment reads is conflict-free, MI355X_MICROARCH §LDS), k >= n_lc_out zero.  31 KiB per layer:
// exactly 31 LDS-DMA pieces.  Used when 64 < n_lc_out <= 80 (LC_K = 5 k-steps of 16).
constexpr int LC_K = 5, LC_KP = 16 * LC_K, LC_ROW = 3 * LC_KP + 8;
constexpr int LCIMG_US = 64 * LC_ROW;                          // bf16 elements per layer image
constexpr int LCIMG_F = LCIMG_US / 2;                          // = 7936 floats
static_assert(LCIMG_F % 256 == 0, "LC image: whole 1-KiB DMA pieces");

// LC image of the 16-lane form: LCT16[o (sig 0..31 | gate 32..63)][plane][k 0..95] (k >= n_lc_out
// zero: three whole 32-deep k-steps), rows of LC16_ROW = 3·96 + 8 bf16 (148 dwords: 4·odd).
constexpr int LC16_KP = 96, LC16_ROW = 3 * LC16_KP + 8;
constexpr int LC16IMG_US = 64 * LC16_ROW;                      // bf16 elements per layer image
constexpr int LC16IMG_F = LC16IMG_US / 2;                      // = 9472 floats = 37 KiB
static_assert(LC16IMG_F % 256 == 0, "LC16 image: whole 1-KiB DMA pieces");

// Backward image per layer: WD[tap][in][plane][kk] (bf16, row XW_ROW) with kk = 16s+8h+j holding
// out channel o = 32(s>>1) + 16(s&1) + 8(j>>2) + 4h + (j&3) (sig 0..31 | gate 32..63): the k order
// of the dv registers used as the B operand; then Rs f32 [c][XS] for the dz product of
// chain_bwd_x3_kernel, padded to a whole number of 1-KiB DMA pieces (BX_F: what that kernel
// loads); then RX, the same residual weights split for chain_bwd16_kernel's dz on the bf16 cores:
// RX[c][plane][kk] (bf16, row RX_ROW) with kk = 8g + e holding res channel 16(e >> 2) + 4g + (e & 3)
// (the order of the lane's two N-layout g registers).  chain_bwd16_kernel loads WD and RX only
// (B16IMG_F floats: global pieces [0, BD_PC) and [RX_GPC, RX_GPC + RX_PC)).
constexpr int BD_US = 2 * 32 * XW_ROW;
constexpr int BX_F = (BD_US / 2 + 32 * XS + 255) / 256 * 256;   // 7680 floats
// 224-B RX rows (14 16-B slots): the 16x16x32 A-fragment reads (rows ch16(bb, i), slot 4p + g) hit
// 16 distinct slots in every ds_read_b128 lane group (MI355X_MICROARCH.md §LDS)
constexpr int RX_ROW = 112;
constexpr int RX_F = 32 * RX_ROW / 2;                          // 1792 floats
constexpr int BIMG_F = BX_F + RX_F;                            // 9472 floats: global stride per layer
constexpr int B16IMG_F = BD_US / 2 + RX_F;                     // 8192 floats in chain_bwd16_kernel's LDS
constexpr int BD_PC = BD_US / 2 / 256, RX_GPC = BX_F / 256, RX_PC = RX_F / 256;
static_assert(BD_US / 2 % 256 == 0 && RX_F % 256 == 0 && B16IMG_F % 256 == 0, "bwd image: whole DMA pieces");

// ---- kernel arguments of the chains ------------------------------------------------------
struct ChainFK {
  int xcd;                     // chain_first: XCD-grouped tile walk
  float* X; long xls;        // x_l for all layers: layer stride (floats); each [B][H+T][32]
  float* Z; long ldz;
  const float* wpack;        // L packed images
  const float* gc_tab; long gc_ld;              // GC table [ncat+1][L·2Cd] (row stride gc_ld; layer l at l·2Cd)
  const int* ids; const float* cond; long ldcond; // LC term COND [M][L·2Cd] (layer l at column l·2Cd) or null
  unsigned* flags; unsigned* status;
  int B, T, H, L, nbl, Cd;
  long long* trace; int trace_blk;   // debug stamps (null in production)
  const unsigned short* ximg;        // L split images (XIMG_US bf16 each): the bf16-split form
  float* SG; long sgls;              // σ(v_gate) rows [L][M32][32] (sg_off blocks) for chain_bwd_x3_kernel, or null
  // in-chain LC term (chain_fwd_kernel<true, true>): the upsampled LC input [M][Lo] and the L
  // split LC images (LCIMG_US bf16 each)
  const float* lcact; const unsigned short* lcimg; int Lo;
};

struct ChainBK {
  int xcd;                     // chain_first: XCD-grouped tile walk
  const float* X; long xls;
  const float* DZ; long lddz; long dzls;   // dzls > 0: DZ in chain order (sg_off blocks per layer)
  const float* wpack;
  float* slab;                 // [L][ntiles][SLAB]
  float* ocg; long ocls;       // out_c0 hand-off rows: [L][B·T][32], layer stride ocls floats
  float* dx0_a; float* dx0_c;  // layer 0's out_a / out_c0 [B·T][32]
  const float* gc_tab; long gc_ld; const int* ids; const float* cond; long ldcond;
  float* dv_out; long lddv;    // dv export for the LC gradients: [M][L·2Cd] (layer l at column l·2Cd) or null
  long dvks;                   // x3 forms: 0, or the chunk stride of the k-blocked export [L·2][Mp][32]
  float* gc_dtab;              // GC gradient table, layout of gc_tab, atomics, or null
  unsigned* flags; unsigned* status;
  int B, T, H, L, nbl, Cd;
  long long* trace; int trace_blk;   // debug stamps (null in production)
  // bf16-split form (chain_bwd_x3_kernel): z rows (row stride lddz), σ rows [L][M][32], images
  const float* Zf; const float* SG; long sgls; const float* bimg;
  int* tile_gid;               // GC: per tile its uniform voice id or -1 (x3 chain), or null
};

// ---- LDS staging ---------------------------------------------------------------------

// dst[r][0..31] = x row (t0 + r + shift) of the halo buffer xb, zero if t0+r >= T.
LBWN_DEV void stage_rows(float* dst, const float* __restrict__ xb, int t0, int shift, int T, int H, int C,
                         int tid) {
  if (C == 32) {
    floatx4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 3, c4 = (e & 7) * 4;
      // unconditional load of a clamped row, then select: a predicated load would sit behind
      // a branch and hipcc waits for each one (one memory round trip per row group)
      v[i] = *(const floatx4*)(xb + (long)(H + min(t0 + r, T - 1) + shift) * 32 + c4);
      if (t0 + r >= T) v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      *(floatx4*)(dst + (e >> 3) * XS + (e & 7) * 4) = v[i];
    }
  } else {
    for (int e = tid; e < LP * 32; e += 256) {
      const int r = e >> 5, c = e & 31;
      float v = 0.f;
      if (t0 + r < T && c < C) v = xb[(long)(H + t0 + r + shift) * C + c];
      dst[r * XS + c] = v;
    }
  }
}

// packed image -> LDS (Ws | Rs | bs | br are contiguous in both)
LBWN_DEV void stage_image(float* W, const float* __restrict__ img, int tid) {
  for (int e = tid; e < WIMG / 4; e += 256) *(floatx4*)(W + 4 * e) = *(const floatx4*)(img + 4 * e);
}

// σ(v_gate) rows (SG) are stored in 32-row blocks laid out in the MFMA register order, [m/32][q][m%32][h][4]
// (channel 8q + 4h + j), so that each wave-instruction of the forward's stores and of the backward's
// loads covers one contiguous KiB instead of 32 partial lines
LBWN_DEV long sg_off(long m, int q, int h) { return (((m >> 5) * 4 + q) * 32 + (m & 31)) * 8 + 4 * h; }

LBWN_DEV void store_rows16(float* row, const floatx16& v, int C, int h) {
  if (C == 32) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *(floatx4*)(row + 8 * q + 4 * h) = floatx4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc_row(r, h) < C) row[acc_row(r, h)] = v[r];
  }
}

// ---- chain hand-off and LDS-DMA ----------------------------------------------------------
// One LDS-DMA piece (global_load_lds_dwordx4: 64 lanes × 16 B from per-lane addresses to
// lds_dst + 16·lane) issued from inline asm, so the compiler neither knows the LDS it writes (no
// conservative vmcnt(0) before every later LDS access) nor counts it: the kernel lands these
// pieces itself with an explicit vmcnt(0) drain + barrier before their first reader.
LBWN_DEV void dma16(const void* g, float* lds_dst) {
  const unsigned base =
      __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds_dst);
  unsigned saved;   // m0 is reserved by the compiler: saved and restored around the piece
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
               : "=&s"(saved)
               : "s"(base), "v"(g)
               : "memory");
}

typedef __attribute__((address_space(1))) unsigned gu32;
constexpr long long SPIN_TIMEOUT = 400000000LL;  // wall_clock64 ticks (100 MHz) = 4 s
constexpr int BUF_DW3 = 0x00020000;

// First tile of this block in the chains' tile walk (tile += gridDim.x after it).  xcd: blocks
// b and b + 8 share an XCD under round-robin dispatch (MI355X_MICROARCH.md, placement: speed only,
// never correctness), so with gridDim.x % 8 == 0 block b takes tile (b % 8)·(G/8) + b / 8 of each
// round: consecutive tiles -- a stream's hand-off neighbours -- run on one XCD (32 tiles = one
// 4096-sample stream at C2).  A bijection of each round's tiles: the rounds are unchanged.
LBWN_DEV int chain_first(int xcd) {
  const int bx = blockIdx.x, G = gridDim.x;
  return (xcd && (G & 7) == 0) ? (bx & 7) * (G >> 3) + (bx >> 3) : bx;
}

LBWN_DEV bool wait_flag_ge(unsigned* f, unsigned want, unsigned* status, unsigned code) {
  const long long t0 = wall_clock64();
  for (;;) {
    if (__hip_atomic_load((gu32*)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return true;
    if (wall_clock64() - t0 > SPIN_TIMEOUT) {
      // OR, not store: the word is zeroed once per step (lbwn_train_forward), so a forward
      // timeout (1) survives the backward chain and both read back as 3
      __hip_atomic_fetch_or((gu32*)status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

LBWN_DEV void publish_flag(unsigned* f, unsigned v) {
  __hip_atomic_store((gu32*)f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- conv pieces of the f32 chains (forward, and the backward gate recompute) ------------
// GC + LC term of layer l for this lane's position, in acc layout: cv[q] = sig channels
// 8q+4h..+3, cv[4+q] = gate channels (16-B loads; issued one layer ahead by the chains).
// CM (compile time): 0 no conditioning, 1 GC only (the in-chain-LC forward of arch5 and GC-only
// archs), 2 any (runtime pointers).  CM 1 loads are issued unconditionally at clamped rows (a row
// past T feeds only its own, discarded, position column) straight into cv: an add right after the
// load (CM 2's zero-init + add) or a register copy merging paths made hipcc wait for the loads --
// with vmcnt(0), which also waited out the x_{l+1} stores issued just before (the drain the own
// tap is meant to hide).
template <int CM, typename K>
LBWN_DEV void load_cond(const K& a, int l, int myid, long m, bool valid, int h, floatx4 (&cv)[8]) {
  if (CM == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) cv[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  if (CM == 1) {
    const float* g = a.gc_tab + (long)myid * a.gc_ld + (long)l * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cv[q] = *(const floatx4*)(g + 8 * q + 4 * h);
      cv[4 + q] = *(const floatx4*)(g + 32 + 8 * q + 4 * h);
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) cv[q] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (!valid) return;
  if (a.gc_tab) {
    const float* g = a.gc_tab + (long)myid * a.gc_ld + (long)l * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cv[q] += *(const floatx4*)(g + 8 * q + 4 * h);
      cv[4 + q] += *(const floatx4*)(g + 32 + 8 * q + 4 * h);
    }
  }
  if (a.cond) {
    const float* c = a.cond + m * a.ldcond + (long)l * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cv[q] += *(const floatx4*)(c + 8 * q + 4 * h);
      cv[4 + q] += *(const floatx4*)(c + 32 + 8 * q + 4 * h);
    }
  }
}

// bias + conditioning into the accumulators (acc layout rows = out channel)
LBWN_DEV void conv_init(const float* bs, const floatx4 (&cv)[8], int h, floatx16& acc_s, floatx16& acc_g) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_s[4 * q + j] = bs[8 * q + 4 * h + j] + cv[q][j];
      acc_g[4 * q + j] = bs[32 + 8 * q + 4 * h + j] + cv[4 + q][j];
    }
}

// acc += Wkᵀ·x over one tap: Wk = the 32 weight-image rows of that tap, xrow = this lane's
// 32-channel input row (LDS)
LBWN_DEV void conv_half(const float* xrow, const float* Wk, int pi, int h, floatx16& acc_s, floatx16& acc_g) {
  // every operand of the 32 MFMAs read first; the sched_barrier stops hipcc from sinking each
  // weight pair next to its MFMA (it did, with an LDS round trip per MFMA pair)
  floatx4 bx[4];
  float ws_[4][4], wg_[4][4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bx[g] = *(const floatx4*)(xrow + 8 * g + 4 * h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 8 * g + 4 * h + j;
      ws_[g][j] = Wk[k * WS + pi];
      wg_[g][j] = Wk[k * WS + 32 + pi];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_s = mfma32(ws_[g][j], bx[g][j], acc_s);
      acc_g = mfma32(wg_[g][j], bx[g][j], acc_g);
    }
}

// ---- 16-position waves (chain_fwd16_kernel, chain_bwd16_kernel) --------------------------
// out channel of A row i of accumulator block b (chain_fwd.hip, the fwd16 section: the permutation
// that puts D row i = 4g + r on channel 8(q0 + b) + 4h + r)
LBWN_DEV int ch16(int b, int i) { return 16 * (i >> 3) + 8 * b + 4 * ((i >> 2) & 1) + (i & 3); }

// acc += A·B over one 32-deep k-step from split fragments (six products, small terms first)
LBWN_DEV floatx4 mfma16x3(const bf16x8 (&a)[3], const bf16x8 (&b)[3], floatx4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  return acc;
}

// ---- GC gradient scatter of the f32 backward kernels ------------------------------------
// dv rows of wave w's 32 positions (DV, position-major) scatter-added into the GC gradient
// table row (row stride ld) of each position's voice id.  uni_id >= 0: the caller knows the
// run is one id (one atomic per column); otherwise the ids are checked here.
LBWN_DEV void gc_scatter(float* gtab, long ld, const int* ids_b, const float* DV, int t0, int T, int w, int lane,
                         int Cd, int uni_id) {
  const int tw0 = t0 + 32 * w;
  const int nv = min(32, T - tw0);
  if (nv <= 0) return;
  const int* idw = ids_b + tw0;
  int id0 = uni_id;
  if (id0 < 0) {
    id0 = idw[0];
    bool uni = true;
    for (int p = 1; p < nv; ++p) uni &= (idw[p] == id0);
    if (!uni) id0 = -1;
  }
  const int o = lane, oc = o & 31;
  const float* dvw = DV + 32 * w * DS;
  if (oc >= Cd) return;
  const int col = o < 32 ? oc : Cd + oc;
  if (id0 >= 0) {
    float s = 0.f;
    for (int p = 0; p < nv; ++p) s += dvw[p * DS + o];
    atomicAdd(gtab + (long)id0 * ld + col, s);
  } else {   // one atomic per run of equal ids (as gc_scatter_x3)
    int p = 0;
    while (p < nv) {
      const int id = idw[p];
      float s = 0.f;
      for (; p < nv && idw[p] == id; ++p) s += dvw[p * DS + o];
      atomicAdd(gtab + (long)id * ld + col, s);
    }
  }
}

}  // namespace
