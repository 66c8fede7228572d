// Cached single-step autoregressive generation (imodel.py:61-272).
//
// All state stays on device, so a chunk of steps can be captured in a hipGraph and replayed:
// the step counter, the per-layer lookback rings (the generation form of the D-separation
// cache: layer l keeps its last d inputs, slot t mod d, replacing imodel's shift-by-chunk
// buffers imodel.py:88-98, :190-207), the next input code, the teacher vector and a
// counter-based RNG.  Two execution forms, chosen at plan creation:
//   persistent (the default while its blocks fit: groups of <= 16 streams, each group with its
//     own head blocks, B <= 80 on 256 CUs): ONE launch per run, gen_persist_kernel — chain
//     blocks (one per stream) and 32 head blocks hand z, the skip vector and the partial logits
//     to each other as tagged granules; weights of the head stay in registers for the run
//   per step (any B): gen_wave (one workgroup per stream: PRE row (+bias), 50 × [dilated conv,
//     gate, residual] while four loader waves stream the per-layer weight images into an LDS
//     ring by LDS-DMA), gen_gemv × 3 (K-split row-vector products with deterministic partial
//     sums: skip = z_cat·SKIPcat, h = relu(relu(skip + Σb)·POST1 + b1), logits = h·POST2) and
//     gen_sample (Σ partials + b2, the draw)
// Local conditioning (no counterpart in imodel.py; tmodel.py:155-160): lbwn_gen_set_mel upsamples
// the mel once, gen_lc_proj_kernel projects it for the next <= NC steps into a cond ring, and the
// step kernels' loaders DMA that step's row into the fourth bias row of each layer's LDS slot.
// Both draw with the same wave-level inverse-CDF code: u = hash(seed, stream, step), µ-law
// decode, next input = teacher[t] or the draw (imodel.py:167-187, :260-269).  A sampling triple other
// than (1, 0, 1) (lbwn_gen_set_sampling: temperature, top_k, top_p) selects the FILT instantiations,
// whose draw filters the codes first (draw_core_filt); the neutral triple runs the plain ones.
// State snapshots (lbwn_gen_state_save / _load): one transposing copy kernel between the layer-major
// rings and stream-major records, after the prefill's kernels; the step kernels know nothing of it.
// Prompt prefill (lbwn_gen_prefill): n steps with known inputs as a sliced per-layer forward
// (layer.hip's layer_fwd_kernel) whose D-separation state is the rings; its kernels are at the end
// of the namespace below, the step kernels know nothing of it.  LC plans project the slice's lc
// rows for G layers at a time on the f32 matrix cores (gen_prefill_lcproj_kernel) into the
// per-row cond term that kernel already takes.
// Teacher-forced scoring (lbwn_gen_score): the same host loop with every layer's z kept side by side
// in a caller-owned Zcat, the per-step GEMM form's head over all rows of a slice, and one wave per
// row for logp = logit[code] - logsumexp (gen_score_logp_kernel).
// Sessions (lbwn_gen_begin): single streams restarted between two runs -- gen_begin_kernel zeroes their
// rings, rewrites their GC rows and writes their words {base, key, rows}; the draw and the LC projection
// read the words when the plan hands them the table, the chains know nothing of it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace {


// Wave-level LDS sync for single-wave workgroups: orders the wave's own LDS traffic without
// the vmcnt(0) that __syncthreads() implies (which would also wait for the next layer's
// weight prefetch, putting its L2 latency back on the chain).
LBWN_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- per-stream layer chain --------------------------------------------------------------
// One workgroup of 8 waves per stream: waves 0-3 compute (one per SIMD), waves 4-7 move data.
//   compute wave w owns channels 8w..8w+7 (lane group c = lane>>3 <-> channel 8w+c):
//     conv      lane = (c, sg = sig|gate, kq): 16 FMAs over inputs 8kq..8kq+7 of x[t-d] and of
//               x[t] (4 weight + 4 broadcast input ds_read_b128), the four lanes' sums summed
//               by two DPP quad permutes, the sig/gate partner fetched by row_half_mirror,
//               z = tanh(sig)·σ(gate) on all 8 lanes of the group
//     residual  lane = (c, kp = k-eighth): 4 FMAs over z[4kp..4kp+3], DPP-reduced over kp
//   Splitting the layer over the four SIMDs is what pays: one wave doing all 64 outputs
//   reads 43 KB of LDS per layer through one SIMD's return path (~16 cycles per 1-KiB
//   ds_read_b128), ~1,500 cycles per layer.
//   loader waves  (a) this step's dilated taps x_l[t-d_l] (ring slot t mod d_l) into the LDS tap
//                 table, two layers per 4-byte LDS-DMA; (b) every layer's slot — weights (20 ×
//                 1 KiB, packed once per gen_start) + bias rows + the stream's GC-projection
//                 row — into an NS-slot LDS ring, NS-1 layers ahead: 5 pieces + 1 row per loader
//                 per layer (counted vmcnt, inside the 6-bit counter).
// Two raw s_barriers per layer: B1 (x of layer l written; before it each loader retires layer
// l's pieces, and the compute waves' reads of slot l-1 retired, so the loaders refill it after
// B1) and B2 (z of layer l written).  No global loads on the compute chain.
// Conv lane (c, sg, kq) takes inputs 8kq..8kq+7 of BOTH taps (pieces m = 0, 1: x[t-d]; m = 2, 3:
// x[t]), so the persistent chain computes the dilated half of the next layer's conv beside the
// residual and only 8 current-tap FMAs (two chains of 4) remain between the x write and the gate
// (with the residual weights read before the z write: 36.3 -> 35.0 us per step at B = 10, same box;
// either change alone: 36.2 / 36.5)
constexpr int GI_W = 16 * 256;              // conv: [w 4][m 4][lane 64][4]  W[32(m>>1)+8kq+4(m&1)+j][32sg+8w+c]
constexpr int GI_R = 4 * 256;               // residual: [h 2][q 4][c 32][4] RES[16h+4q+j][c]
constexpr int GI_WR = GI_W + GI_R;          // 20 pieces of 1 KiB
constexpr int GIMG = GI_WR + 192;           // global image: + conv bias [64] + residual bias [64] + zeros [64]
constexpr int G_SLOT = GI_WR + 256;         // LDS slot: weights | bc [64] | br [64] | gc [64] | pad [64]
constexpr int G_NS = 6;                     // LDS ring depth (layers)
constexpr int G_PIECES = 5;                 // 1-KiB pieces per loader wave per layer (4 loaders)
constexpr int G_DMA = G_PIECES + 1;         // + one 256-B row
constexpr int G_MAXL = 256;                 // tap table rows
constexpr int G_LDS = G_NS * G_SLOT + (G_MAXL + 2) * 32 + 4 * 32 + 2 * 32;   // ring | taps | x[4 waves] | z[2]
static_assert(4 * G_PIECES * 256 == GI_WR, "image pieces");
static_assert(G_LDS * 4 <= 160 * 1024, "LDS");

struct WaveK {
  const float* pre; const float* pre_b; const float* img; const float* gc_proj;
  float* rings; float* zcat; const long long* step; const int* code;
  int B, L, nbl, Cr, Cd, pre_bias;
  long long* trace;   // non-null (LBWN_GEN_TRACE set at plan creation): stream 0's cycle stamps
  const float* lccond; int NC;   // LC plans: the cond ring [NC][L][B][64] (gen_lc_proj_kernel)
};

LBWN_DEV float dot4(const floatx4& w, const floatx4& x, float acc) {
  acc = fmaf(w[0], x[0], acc);
  acc = fmaf(w[1], x[1], acc);
  acc = fmaf(w[2], x[2], acc);
  return fmaf(w[3], x[3], acc);
}

template <int CTRL>
LBWN_DEV float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141;

// workgroup barrier that retires only this wave's LDS ops: no vmcnt wait (outstanding global
// stores and LDS-DMA pieces stay in flight across it); the "memory" clobber pins LDS accesses
LBWN_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS-DMA: lane i's SIZE bytes from src land at lds_dst + i·SIZE (lds_dst wave-uniform)
LBWN_DEV void dma16(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
LBWN_DEV void dma4(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

// LC: the slot's fourth row is this step's projected LC term lccond[t mod NC][l][b] instead of
// the zero row (same DMA count), added to the conv bias beside the GC row
template <bool LC>
__global__ __launch_bounds__(512) void gen_wave_kernel(WaveK a) {
  __shared__ __attribute__((aligned(16))) float sm[G_LDS];
  float* RING = sm;                  // [G_NS][G_SLOT]
  float* XP = sm + G_NS * G_SLOT;    // [L (+2)][32] dilated taps of this step
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.x, L = a.L;
  const long t = *a.step;

  if (wid >= 4) {   // ---- loader waves
    const int lw = wid - 4;
    const float* zeros = a.img + GI_WR + 128;   // the image's zero row (layer 0)
    const float* lcrow = LC ? a.lccond + ((long)(int)(t % a.NC) * L * a.B + b) * 64 : zeros;
    // (a) taps: pair q = layers 2q, 2q+1 (lane half h) by loader q % 4; d is a power of two,
    // slot = t & (d-1); ring offsets carried in scalars (no integer division)
    {
      const int h = lane >> 5, c = lane & 31;
      long roff = 0;
      int bl = 0;
      for (int q = 0; 2 * q < L; ++q) {
        const int dE = 1 << bl;
        const long roffO = roff + (long)dE * a.B * a.Cr;
        const int blO = (bl + 1 == a.nbl) ? 0 : bl + 1;
        const int dO = 1 << blO;
        if ((q & 3) == lw) {
          const int d = h ? dO : dE, l = 2 * q + h;
          const float* src = (l < L && c < a.Cr)
                                 ? a.rings + (h ? roffO : roff) + ((long)b * d + (t & (d - 1))) * a.Cr + c
                                 : zeros + c;
          dma4(src, XP + 2 * q * 32);
        }
        roff = roffO + (long)dO * a.B * a.Cr;
        bl = (blO + 1 == a.nbl) ? 0 : blO + 1;
      }
    }
    // (b) slots: pieces [5lw, 5lw+5) + row lw (bc | br | gc | pad)
    auto issue = [&](int l) {
      const float* src = a.img + (long)l * GIMG;
      float* dst = RING + (l % G_NS) * G_SLOT;
#pragma unroll
      for (int p = 0; p < G_PIECES; ++p) {
        const int pc = lw * G_PIECES + p;
        dma16(src + pc * 256 + lane * 4, dst + pc * 256);
      }
      const float* row = lw < 2 ? src + GI_WR + lw * 64
                       : lw == 2 ? (a.gc_proj ? a.gc_proj + ((long)l * a.B + b) * 64 : zeros)
                                 : (LC ? lcrow + (long)l * a.B * 64 : zeros);
      dma4(row + lane, dst + GI_WR + lw * 64);
    };
    for (int l = 0; l < G_NS - 1 && l < L; ++l) issue(l);
    for (int k = -1; k < L; ++k) {
      // barrier k (after z_k is written; k = -1: the step input) releases the residual of layer
      // k and the conv of layer k+1, so slot k+1 must have landed.  Issued so far: taps, layers
      // 0 .. min(k+NS-2, L-1): retire all but the min(k+NS-2, L-1) - (k+1) youngest layers.
      const int younger = min(k + G_NS - 2, L - 1) - (k + 1);
      if (younger >= G_NS - 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * (G_NS - 3)) : "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * 2) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
      // slot of layer k-1 is dead (its residual ran before barrier k): layer k+NS-1 goes there
      // (k = 0: the slot of layer NS-1, never used yet)
      if (k >= 0 && k + G_NS - 1 < L) issue(k + G_NS - 1);
    }
    return;
  }

  // ---- compute waves: ONE workgroup barrier per layer.  Every wave keeps the whole layer input
  // x (lane c and c+32 hold channel c) and computes the residual of all 32 channels itself
  // (16 FMAs per lane over one z half, the halves summed by v_permlane32_swap), so the next
  // layer's conv needs no second barrier: its inputs go through the wave's own LDS row (XW).
  const int w = wid, Cr = a.Cr, Cd = a.Cd;
  const int c = lane >> 3, sg = (lane >> 2) & 1, kq = lane & 3, kp = lane & 7;
  const int ch = 8 * w + c;                 // the conv channel of this lane group
  const int o = 32 * sg + ch;               // conv output of this lane
  const bool lead = kp == 0;                // one lane per group stores z
  const int rc = lane & 31, rh = lane >> 5; // residual: out channel rc over z half rh
  float* XW = XP + (G_MAXL + 2) * 32 + 32 * w;   // this wave's copy of the layer input
  float* Z = XP + (G_MAXL + 2) * 32 + 128;       // z double buffer [2][32]
  const bool tr = a.trace && b == 0 && w == 0 && lane == 0;
  if (tr) a.trace[0] = clock64();
  // step input: PRE row of the previous draw (+ PRE_BIAS); the zero vector at step 0
  float x = 0.f;    // x[rc] of the current layer input
  if (rc < Cr) {
    const int code = a.code[b];
    if (code >= 0) x = a.pre[(long)code * Cr + rc];
    if (a.pre_bias && a.pre_b) x += a.pre_b[rc];
  }
  if (lane < 32) XW[rc] = x;
  if (tr) a.trace[1] = clock64();
  long roff = 0;   // ring offset of layer l
  int bl = 0;      // l % nbl
  lds_barrier();   // barrier -1: taps and slot 0 landed, every wave's XW written
  if (tr) a.trace[2] = clock64();
  for (int l = 0; l < L; ++l) {
    const float* S = RING + (l % G_NS) * G_SLOT;
    floatx4 wv[4], xv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      wv[m] = *(const floatx4*)(S + (w * 4 + m) * 256 + lane * 4);
      xv[m] = *(const floatx4*)((m < 2 ? XP + l * 32 : XW) + 8 * kq + 4 * (m & 1));
    }
    float bco = S[GI_WR + o] + S[GI_WR + 128 + o];
    if (LC) bco += S[GI_WR + 192 + o];
    __builtin_amdgcn_sched_barrier(0);
    const int d = 1 << bl;
    // x_l[t] into the ring (wave w stores channels 8w..8w+7)
    if (rh == 0 && (rc >> 3) == w && rc < Cr) a.rings[roff + ((long)b * d + (t & (d - 1))) * Cr + rc] = x;
    roff += (long)d * a.B * Cr;
    bl = (bl + 1 == a.nbl) ? 0 : bl + 1;
    float acc0 = dot4(wv[0], xv[0], 0.f), acc1 = dot4(wv[1], xv[1], 0.f);
    acc0 = dot4(wv[2], xv[2], acc0);
    acc1 = dot4(wv[3], xv[3], acc1);
    float v = acc0 + acc1;
    v += dpp<DPP_XOR1>(v);
    v += dpp<DPP_XOR2>(v);
    v += bco;                                      // conv output o (+ bias + GC term)
    const float vp = dpp<DPP_HALF_MIRROR>(v);      // the partner output (sig <-> gate, same channel)
    const float z = gate_z(sg ? vp : v, sg ? v : vp);
    float* Zl = Z + (l & 1) * 32;
    if (lead) {
      Zl[ch] = z;
      if (ch < Cd) a.zcat[(long)b * L * Cd + (long)l * Cd + ch] = z;
    }
    if (tr) a.trace[4 + 2 * l] = clock64();
    lds_barrier();   // barrier l: z_l complete; slot l+1 landed
    // residual of all 32 channels: x_{l+1}[rc] = x[rc] + b[rc] + Σ_k RES[k][rc]·z[k]
    floatx4 zv[4], rw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      zv[q] = *(const floatx4*)(Zl + 16 * rh + 4 * q);
      rw[q] = *(const floatx4*)(S + GI_W + ((rh * 4 + q) * 32 + rc) * 4);
    }
    const float bro = S[GI_WR + 64 + rc];
    float r0 = dot4(rw[0], zv[0], 0.f), r1 = dot4(rw[1], zv[1], 0.f);
    r0 = dot4(rw[2], zv[2], r0);
    r1 = dot4(rw[3], zv[3], r1);
    const float r = r0 + r1;
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), __float_as_uint(r), false, false);
    x += (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + bro;
    if (lane < 32) XW[rc] = x;   // read back by this wave's conv of layer l+1: a wave-local sync only
    wave_sync();
    if (tr) a.trace[5 + 2 * l] = clock64();
  }
}

// per-layer weight image in the compute waves' lane order (reference layouts in, GIMG floats
// per layer out): SIGNAL/GATE [l][tap][Cr][Cd] (tap 0 = x[t-d]), RESIDUAL [l][Cd][Cr]
__global__ void gen_pack_kernel(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                                const float* res, const float* res_b, float* img, int Cr, int Cd) {
  const int l = blockIdx.x;
  float* out = img + (long)l * GIMG;
  for (int e = threadIdx.x; e < GIMG; e += blockDim.x) {
    float v = 0.f;
    if (e < GI_W) {
      const int w = e / 1024, m = (e / 256) % 4, ln = (e % 256) / 4, j = e % 4;
      const int c = ln >> 3, sg = (ln >> 2) & 1, kq = ln & 3;
      const int k = (m < 2 ? 0 : 32) + 8 * kq + 4 * (m & 1) + j;
      const int tap = k >> 5, in = k & 31, oc = 8 * w + c;
      if (in < Cr && oc < Cd) v = (sg ? gate : sig)[(long)l * 2 * Cr * Cd + (tap * Cr + in) * Cd + oc];
    } else if (e < GI_WR) {
      const int f = e - GI_W, j = f & 3, oc = (f >> 2) & 31, q = (f >> 7) & 3, h = f >> 9;
      const int zc = 16 * h + 4 * q + j;
      if (zc < Cd && oc < Cr) v = res[(long)l * Cd * Cr + zc * Cr + oc];
    } else {
      const int f = e - GI_WR;
      if (f < 64) {
        const float* bb = f < 32 ? sig_b : gate_b;
        if (bb && (f & 31) < Cd) v = bb[(long)l * Cd + (f & 31)];
      } else if (f < 128) {
        if (res_b && f - 64 < Cr) v = res_b[(long)l * Cr + f - 64];
      }
    }
    out[e] = v;
  }
}


// ---- K-split row-vector GEMV --------------------------------------------------------------
// part[ks][b][n] = Σ_{k in slice ks} act(in[b][k])·W[k][n]: block = 64 columns (lane = n) ×
// one K slice, 4 waves over the slice's rows.  The input is either a plain [B][K] row buffer
// or the previous GEMV's partials, summed here in a fixed order (+ bias, relu): the chain of
// skip -> post1 -> post2 -> sample stays deterministic without atomics.
constexpr int GV_KSL_MAX = 64;   // K rows per slice (runtime KSL <= this, multiple of 4)

struct GemvK {
  const float* in; long ldin;                   // plain input rows, or
  const float* in_part; int in_parts;           // partials [in_parts][B][K]
  const float* in_bias; int relu_in;            // applied after the sum
  const float* W; long ldw;
  float* out_part;                              // [ceil(K/KSL)][B][N]
  int B, K, N, KSL;
  long long* step_advance;                      // non-null: block (0,0) advances the step counter
  long long* trace;                             // debug (LBWN_GEN_TRACE): [8] stamps of this launch
};

__global__ __launch_bounds__(256) void gen_gemv_kernel(GemvK a) {
  // staged inputs per wave: xs[w][i][j] = x[j][k0 + w + 4i], so a wave reads the 16 stream
  // values of one of its rows with 4 broadcast ds_read_b128 (not 16 ds_read_b32)
  __shared__ __attribute__((aligned(16))) float xs[4][GV_KSL_MAX / 4][16];
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = blockIdx.x * 64 + lane;
  const int KSL = a.KSL, ks = blockIdx.y, k0 = ks * KSL, k1 = min(a.K, k0 + KSL);
  const bool first = blockIdx.x == 0 && blockIdx.y == 0, last = blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1;
  if (a.trace && tid == 0 && first) { a.trace[0] = wall_clock64(); a.trace[2] = clock64(); }
  if (a.trace && tid == 0 && last) a.trace[6] = wall_clock64();
  // weights: branch-free (clamped index, then select), so hipcc can count these loads and the
  // input staging below does not wait for them (behind branches it lost the count and waited
  // vmcnt(0): the weight fetch and the input fetch became two serial round trips)
  float wr[GV_KSL_MAX / 4];
#pragma unroll
  for (int i = 0; i < GV_KSL_MAX / 4; ++i) {
    const int k = k0 + w + 4 * i;
    wr[i] = a.W[(long)min(k, a.K - 1) * a.ldw + min(n, a.N - 1)];
    if (!(4 * i < KSL && k < k1 && n < a.N)) wr[i] = 0.f;
  }
  if (a.step_advance && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)   // no-return atomic: no wait
    __hip_atomic_fetch_add(a.step_advance, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto put = [&](int e, float x) {   // element e = j·KSL + kk of the slice
    const int j = e / KSL, kk = e % KSL;
    xs[kk & 3][kk >> 2][j] = x;
  };
  for (int b0 = 0; b0 < a.B; b0 += 16) {
    const int nbb = min(16, a.B - b0);
    // stage the input slice: every load of this thread issued before the first is consumed
    constexpr int GV_EPT = 16 * GV_KSL_MAX / 256;
    if (a.in_part) {
      // the previous GEMV's partials (≤ 32 per element, all issued at once: one memory round
      // trip) + bias, relu; two elements per pass
      for (int r0 = 0; r0 < GV_EPT; r0 += 2) {
        if (tid + 256 * r0 >= 16 * KSL) break;
        float s2[2] = {0.f, 0.f}, bb[2];
        for (int q0 = 0; q0 < a.in_parts; q0 += 32) {
          float v[2][32];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int e = tid + 256 * (r0 + h), j = min(e / KSL, nbb - 1), k = min(k0 + e % KSL, a.K - 1);
            const float* pp = a.in_part + (long)(b0 + j) * a.K + k;
#pragma unroll
            for (int i = 0; i < 32; ++i) v[h][i] = pp[(long)min(q0 + i, a.in_parts - 1) * a.B * a.K];
            if (q0 == 0) bb[h] = a.in_bias ? a.in_bias[k] : 0.f;
          }
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 32; ++i) s2[h] += (q0 + i < a.in_parts) ? v[h][i] : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = tid + 256 * (r0 + h);
          if (e >= 16 * KSL) continue;
          const int j = e / KSL, k = k0 + e % KSL;
          float v = 0.f;
          if (j < nbb && k < a.K) {
            v = s2[h] + bb[h];
            if (a.relu_in) v = fmaxf(v, 0.f);
          }
          put(e, v);
        }
      }
    } else {
      float v[GV_EPT];
#pragma unroll
      for (int r = 0; r < GV_EPT; ++r) {
        const int e = tid + 256 * r, j = min(e / KSL, nbb - 1), k = min(k0 + e % KSL, a.K - 1);
        v[r] = a.in[(long)(b0 + j) * a.ldin + k];
      }
#pragma unroll
      for (int r = 0; r < GV_EPT; ++r) {
        const int e = tid + 256 * r;
        if (e >= 16 * KSL) continue;
        const int j = e / KSL, kk = e % KSL;
        float x = (j < nbb && k0 + kk < a.K) ? v[r] : 0.f;
        if (a.relu_in) x = fmaxf(x, 0.f);
        put(e, x);
      }
    }
    __syncthreads();
    if (a.trace && tid == 0 && first && b0 == 0) a.trace[3] = clock64();
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < GV_KSL_MAX / 4; ++i)
      if (4 * i < KSL) {
        const floatx4* xr = (const floatx4*)&xs[w][i][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 x = xr[q];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[4 * q + jj] = fmaf(x[jj], wr[i], acc[4 * q + jj]);
        }
      }
#pragma unroll
    for (int j = 0; j < 16; ++j) red[w][j][lane] = acc[j];
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += 256) {
      const int j = e >> 6, c = e & 63, nn = blockIdx.x * 64 + c;
      if (j < nbb && nn < a.N)
        a.out_part[((long)ks * a.B + b0 + j) * a.N + nn] = ((red[0][j][c] + red[1][j][c]) + red[2][j][c]) + red[3][j][c];
    }
    __syncthreads();
  }
  if (a.trace && tid == 0 && first) { a.trace[4] = clock64(); a.trace[1] = wall_clock64(); }
  if (a.trace && tid == 0 && last) a.trace[7] = wall_clock64();
}

// ---- the draw (imodel.py:167-187, :260-269) ----------------------------------------------
// Inverse-CDF draw of softmax(logits): the first k with cumsum(e)[k] > u·Σe, e = exp(logits -
// max), u = hash(seed, stream, step) (oracle/wavenet_ref.py sample_from_logits restates the
// transform).  Wave-level only — lane = a contiguous run of ceil(Q/64) codes, shuffles, no
// workgroup barrier — so every wave that calls it with the same logits draws the same code.
struct DrawK {
  const float* part; int parts; const float* bias;   // logits = Σ part[p][b][:] + bias (per-step path)
  int Q, B;
  float* logits; int* samples; float* wav; long long max_steps;
  const int* teacher; long long n_teacher; unsigned long long seed; int* code;
  float temperature; int top_k; float top_p;   // lbwn_gen_set_sampling; read by the FILT forms only
  // sessions (lbwn_gen_begin): [B][4] int64 {base, key, rows, 0}, or null: key = stream, base = 0
  const long long* sess;
};

// wave-wide max / min / inclusive scan on DPP (row ops + row_bcast, GFX9): one VALU latency
// per step instead of a ds_bpermute round trip per __shfl step
template <int CTRL, int ROWS = 0xF>
LBWN_DEV int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, true); }
LBWN_DEV float wave_max(float v) {
  v = fmaxf(v, __int_as_float(dpp_i<0xB1>(__float_as_int(v))));    // quad_perm xor 1
  v = fmaxf(v, __int_as_float(dpp_i<0x4E>(__float_as_int(v))));    // quad_perm xor 2
  v = fmaxf(v, __int_as_float(dpp_i<0x141>(__float_as_int(v))));   // row_half_mirror
  v = fmaxf(v, __int_as_float(dpp_i<0x140>(__float_as_int(v))));   // row_mirror: every row uniform
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
LBWN_DEV int wave_min(int v) {
  v = min(v, dpp_i<0xB1>(v));
  v = min(v, dpp_i<0x4E>(v));
  v = min(v, dpp_i<0x141>(v));
  v = min(v, dpp_i<0x140>(v));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// inclusive prefix sum over the 64 lanes: Hillis-Steele within rows (row_shr 1, 2, 4, 8), then
// row 15's total into rows 1, 3 and lane 31's into rows 2, 3
LBWN_DEV float wave_scan(float x) {
  x += __int_as_float(dpp_i<0x111>(__float_as_int(x)));
  x += __int_as_float(dpp_i<0x112>(__float_as_int(x)));
  x += __int_as_float(dpp_i<0x114>(__float_as_int(x)));
  x += __int_as_float(dpp_i<0x118>(__float_as_int(x)));
  x += __int_as_float(dpp_i<0x142, 0xA>(__float_as_int(x)));
  x += __int_as_float(dpp_i<0x143, 0xC>(__float_as_int(x)));
  return x;
}
// wave-wide sum, the same value on every lane (each step adds a lane's partner, so both sides of a
// pair form the same sum): the filtered draw's masses
LBWN_DEV float wave_sum(float v) {
  v += __int_as_float(dpp_i<0xB1>(__float_as_int(v)));
  v += __int_as_float(dpp_i<0x4E>(__float_as_int(v)));
  v += __int_as_float(dpp_i<0x141>(__float_as_int(v)));
  v += __int_as_float(dpp_i<0x140>(__float_as_int(v)));
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}

LBWN_DEV uint64_t splitmix(uint64_t seed, uint64_t stream, uint64_t step) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ULL + (stream << 32) + step + 0x632BE59BD9B4E019ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// v[j] = logit of code lane·per + j.  Returns the next input code of stream b after step t (the
// teacher's or the draw); the writing wave stores logits, the sample, its µ-law decode, code[b].
// µ-law decode of one code (ops.py:12-20)
LBWN_DEV float mu_decode_q(int q, int Q) {
  const float mu = (float)(Q - 1), inv = 1.f / mu;
  const float aa = (2.f * (float)q - 1.f) * inv - 1.f;
  const float sg = aa > 0.f ? 1.f : (aa < 0.f ? -1.f : 0.f);
  return sg * (powf(1.f + mu, fabsf(aa)) - 1.f) * inv;
}

// the persistent form's wav: its draws store only the code (powf on lane 0 held the next step's
// PRE row behind it); this decodes the run's samples [step - n, step) after the launch
__global__ void gen_decode_kernel(const int* __restrict__ samples, float* __restrict__ wav, const long long* step,
                                  int B, long long max_steps, int n, int Q) {
  const long long t1 = min(*step, max_steps), t0 = max(*step - n, 0LL);
  const long long span = t1 - t0;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)B * span;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = (e / span) * max_steps + t0 + e % span;
    wav[i] = mu_decode_q(samples[i], Q);
  }
}

template <int MP>
LBWN_DEV int draw_core(float (&v)[MP], const DrawK& a, int b, long long t, bool write, bool decode = true) {
  const int lane = threadIdx.x & 63, Q = a.Q;
  const int per = (Q + 63) >> 6, c0 = lane * per;
  // the draw's key: (stream, absolute step), or the session's (key, local step t - base); the two words
  // are fetched here, ahead of the max / exp / scan they are needed after
  uint64_t skey = (uint64_t)b, sstep = (uint64_t)t;
  if (a.sess) {
    skey = (uint64_t)a.sess[4 * b + 1];
    sstep = (uint64_t)(t - a.sess[4 * b]);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    const bool ok = j < per && c0 + j < Q;
    if (ok) mx = fmaxf(mx, v[j]);
    if (ok && write) a.logits[(long)b * Q + c0 + j] = v[j];
  }
  mx = wave_max(mx);
  float e[MP], loc = 0.f;
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    e[j] = (j < per && c0 + j < Q) ? expf(v[j] - mx) : 0.f;
    loc += e[j];
  }
  const float incl = wave_scan(loc);
  const float total = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
  const float excl = incl - loc;
  const uint64_t h = splitmix(a.seed, skey, sstep);
  const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
  const float target = u * total;
  int found = Q;   // the lane whose run contains the crossing point
  if (excl <= target && target < incl) {
    float run = excl;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (j < per && c0 + j < Q && found == Q) {
        run += e[j];
        if (run > target) found = c0 + j;
      }
    }
    if (found == Q) found = min(c0 + per, Q) - 1;
  }
  found = wave_min(found);
  if (found >= Q) found = Q - 1;
  const int next = (t < a.n_teacher) ? a.teacher[t] : found;   // imodel.py:260-269
  if (write && lane == 0) {
    if (t < a.max_steps) {
      a.samples[(long)b * a.max_steps + t] = found;
      if (decode) a.wav[(long)b * a.max_steps + t] = mu_decode_q(found, Q);
    }
    a.code[b] = next;
  }
  return next;
}

// The filtered draw (lbwn_gen_set_sampling: temperature T, top_k, top_p), same
// contract as draw_core: wave-level only, no LDS, and every step a function of the logits alone, so
// the four compute waves of a chain block reach the same code.  Both filters are thresholds on one
// ordering, found by bisection on integer bit patterns:
//   top_k  key = the logit's bits made order-preserving (slots past Q get key 0, below every real
//          key); K = the largest key with #{key >= K} >= k, i.e. the k-th largest key, built bit by
//          bit from the top: 32 rounds of MP compares, the count = popcount of the wave's ballot
//          (scalar, no cross-lane traffic).  Kept: key >= K, ties with the k-th included.
//   e      exp((l - max) / T) on the kept codes, 0 elsewhere.
//   top_p  e >= 0, so its bits are monotone in e; th = the largest pattern with Σ{e : bits(e) >= th}
//          >= p·Σe, i.e. the smallest e of the shortest descending prefix that reaches p: 30 rounds
//          (e <= 1 < 2^30 as bits) of a masked wave sum.  Kept: bits(e) >= th, its ties included.
// The inverse-CDF walk is draw_core's over the surviving e; its rounding fallbacks (no lane or no
// code crossing the target) take the last SURVIVING code, never a filtered one.
template <int MP>
LBWN_DEV int draw_core_filt(float (&v)[MP], const DrawK& a, int b, long long t, bool write, bool decode = true) {
  const int lane = threadIdx.x & 63, Q = a.Q;
  const int per = (Q + 63) >> 6, c0 = lane * per;
  // the draw's key: (stream, absolute step), or the session's (key, local step t - base); the two words
  // are fetched here, ahead of the max / exp / scan they are needed after
  uint64_t skey = (uint64_t)b, sstep = (uint64_t)t;
  if (a.sess) {
    skey = (uint64_t)a.sess[4 * b + 1];
    sstep = (uint64_t)(t - a.sess[4 * b]);
  }
  float mx = -INFINITY;
  unsigned key[MP];
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    const bool ok = j < per && c0 + j < Q;
    if (ok) mx = fmaxf(mx, v[j]);
    if (ok && write) a.logits[(long)b * Q + c0 + j] = v[j];
    const unsigned bits = __float_as_uint(v[j] + 0.f);   // -0 -> +0: equal logits, equal keys
    key[j] = ok ? (bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u)) : 0u;
  }
  mx = wave_max(mx);
  unsigned K = 1u;   // top_k off: every real key
  if (a.top_k > 0) {
    K = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned tr = K | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < MP; ++j) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[j] >= tr));
      if (cnt >= a.top_k) K = tr;
    }
    K = max(K, 1u);
  }
  const float T = a.temperature;
  float e[MP], loc = 0.f;
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    e[j] = key[j] >= K ? expf((v[j] - mx) / T) : 0.f;
    loc += e[j];
  }
  if (a.top_p < 1.f) {
    const float goal = a.top_p * wave_sum(loc);
    unsigned th = 0u;
    for (int bit = 29; bit >= 0; --bit) {
      const unsigned tr = th | (1u << bit);
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < MP; ++j) m += __float_as_uint(e[j]) >= tr ? e[j] : 0.f;
      if (wave_sum(m) >= goal) th = tr;
    }
    loc = 0.f;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (__float_as_uint(e[j]) < th) e[j] = 0.f;
      loc += e[j];
    }
  }
  const float incl = wave_scan(loc);
  const float total = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
  const float excl = incl - loc;
  const uint64_t h = splitmix(a.seed, skey, sstep);
  const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
  const float target = u * total;
  int found = Q, lastc = -1;   // lastc: this lane's last surviving code (e > 0 only on codes < Q)
#pragma unroll
  for (int j = 0; j < MP; ++j)
    if (e[j] > 0.f) lastc = c0 + j;
  if (loc > 0.f && target < incl) {   // the first such lane holds the crossing point (wave_min below)
    float run = excl;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      if (e[j] > 0.f && found == Q) {
        run += e[j];
        if (run > target) found = c0 + j;
      }
    }
    if (found == Q) found = lastc;
  }
  found = wave_min(found);
  if (found >= Q) found = -wave_min(-lastc);   // target rounded up to the total: the last survivor
  const int next = (t < a.n_teacher) ? a.teacher[t] : found;   // imodel.py:260-269
  if (write && lane == 0) {
    if (t < a.max_steps) {
      a.samples[(long)b * a.max_steps + t] = found;
      if (decode) a.wav[(long)b * a.max_steps + t] = mu_decode_q(found, Q);
    }
    a.code[b] = next;
  }
  return next;
}

// per-step path: logits from the post2 GEMV's K-slice partials, Σ in slice order + bias
template <int MP, bool FILT = false>
LBWN_DEV int draw_wave(const DrawK& a, int b, long long t, bool write) {
  const int lane = threadIdx.x & 63, Q = a.Q;
  const int per = (Q + 63) >> 6, c0 = lane * per;
  float v[MP], bv[MP];
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    v[j] = 0.f;
    bv[j] = a.bias ? a.bias[min(c0 + j, Q - 1)] : 0.f;
  }
  constexpr int CH = MP > 4 ? 8 : 16;
  for (int q0 = 0; q0 < a.parts; q0 += CH) {   // every load of a chunk (and the bias) issued before the first add
    float x[MP][CH];
#pragma unroll
    for (int j = 0; j < MP; ++j)
#pragma unroll
      for (int i = 0; i < CH; ++i)
        x[j][i] = a.part[((long)min(q0 + i, a.parts - 1) * a.B + b) * Q + min(c0 + j, Q - 1)];
#pragma unroll
    for (int j = 0; j < MP; ++j)
#pragma unroll
      for (int i = 0; i < CH; ++i) v[j] += (q0 + i < a.parts) ? x[j][i] : 0.f;
  }
  if (a.bias) {
#pragma unroll
    for (int j = 0; j < MP; ++j) v[j] += bv[j];
  }
  if constexpr (FILT) return draw_core_filt<MP>(v, a, b, t, write);
  else return draw_core<MP>(v, a, b, t, write);
}

// the per-step path's sampler: one wave per stream; the step counter was advanced by this
// step's skip GEMV, so this step is *step - 1
__global__ __launch_bounds__(64) void gen_sample_kernel(DrawK a, const long long* step) {
  const long long t = *step - 1;
  if (a.Q > 256) draw_wave<8>(a, blockIdx.x, t, true);
  else draw_wave<4>(a, blockIdx.x, t, true);
}
// the same with the filtered draw (a second kernel, so the default sampler's code is untouched)
__global__ __launch_bounds__(64) void gen_sample_filt_kernel(DrawK a, const long long* step) {
  const long long t = *step - 1;
  if (a.Q > 256) draw_wave<8, true>(a, blockIdx.x, t, true);
  else draw_wave<4, true>(a, blockIdx.x, t, true);
}

#ifndef LBWN_GEN_SUBSTAMPS
#define LBWN_GEN_SUBSTAMPS 0
#endif
constexpr long long G_SPIN_TIMEOUT = 400000000LL;   // wall_clock64 ticks (100 MHz) = 4 s

// ---- persistent generation: one launch per run (stream groups of <= 16) ----------------
// Roles (one 512-thread workgroup per CU, all resident): streams split into groups of Bg <= 16, each
// group's Bg chain blocks and P_NH head blocks hand off among themselves only (groups x (Bg + P_NH)
// <= CUs; B = 64: four groups, 192 blocks); within a group:
//   chain block b < B   per step: draw the previous step (gather the P_NH partial-logit
//                       granules of stream b, Σ + b2, wave-level draw), PRE row, 50 layers as in
//                       gen_wave (LDS-DMA ring continuous across steps; the next step's taps are
//                       DMA'd right after the last layer), z_l published as tagged granules
//   head block m < P_NH owns skip columns [16m, 16m+16), post1 columns [16m, 16m+16) and the
//                       same post2 rows (POST1 / POST2 slices held in registers for the run):
//                       A. accumulates its skip columns layer by layer as the z granules arrive
//                          (SKIP slice streamed from L2 one layer ahead);
//                       B. publishes them, gathers the whole skip vector, relu(· + Σb);
//                       C. h = relu(skip·POST1[:, cols] + b1), partial logits h·POST2[rows, :]
//                          published as granules for the chain blocks' draw.
// Every hand-off is an 8-byte {value, tag = step + 1} granule written by one sc1 store and polled
// with relaxed agent-scope loads (no flag, no fence: MI355X_MICROARCH.md § visibility, R2);
// single-buffered, because no producer can run a step ahead of its slowest consumer (each
// stage waits on the previous one through the whole ring of roles).  Every spin is bounded
// (status 5).  Three hops per step (z tail, skip all-gather, logit partials) replace the
// per-step path's four launch boundaries and its weight re-fetches.
constexpr int P_NH = 32;     // head blocks
constexpr int P_MAXB = 16;   // streams per group (phase A maps 16 columns x 16 streams onto 512 threads)
constexpr int P_MAXL = 236;  // layers (the draw's two half-sums use tap-table rows 240..255)
constexpr int P_DLROW = 240;
constexpr int P_LA = 8;      // layers per head round (phase A)

struct PersistK {
  const float* pre; const float* pre_b; const float* img; const float* gc_proj;
  float* rings; long long* step; const int* code_in;
  int B, L, nbl, Cr, Cd, pre_bias, n_steps;
  unsigned long long* zg;   // [B][L][32] z granules
  int Cs, Cp, Q;
  const float* skipw; const float* bsum; const float* post1; const float* post1_b; const float* post2;
  unsigned long long* sg;   // [B][Cs] skip granules
  unsigned long long* lg;   // [P_NH][B][Q] partial-logit granules
  DrawK draw;               // outputs; draw.bias = b2
  int* status;
  long long* trace;         // wall stamps of the run's last step (tools/gen_trace.py), or null
  int Bg;                   // streams per group: block g·(Bg + P_NH) + r is group g's chain block r < Bg
                            // (stream g·Bg + r) or head block r - Bg; groups hand off only inside
  long long* gstep;         // step counters of groups 1.. (group 0's is *step, the plan's "step")
  const float* lccond; int NC;   // LC plans: the cond ring [NC][L][B][64]; a run is <= NC steps
};

// poll granules base[off + i·stride], i < nv (N at most; the rest re-read granule nv-1), until
// every tag matches; v[i] = payload.  base is wave-uniform and the index 32-bit, so each load
// is one VGPR offset on an SGPR base.  After any timeout (status != 0) every sweep gives up at
// once, so a failed hand-off drains the launch instead of waiting out each later spin.
template <int N>
LBWN_DEV void sweep(const unsigned long long* base, unsigned off, unsigned stride, int nv, unsigned tag, float (&v)[N],
                    int* status) {
  long long ts = 0;
  const unsigned last = (unsigned)max(nv - 1, 0);
  for (unsigned spins = 1;; ++spins) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const unsigned idx = off + min((unsigned)i, last) * stride;
      const unsigned long long x = __hip_atomic_load(base + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v[i] = __uint_as_float((unsigned)x);
      ok &= (unsigned)(x >> 32) == tag;
    }
    if (ok) return;
    if ((spins & 31) == 0) {   // the clock and the status word cost a round trip each: not every retry
      if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
      const long long now = wall_clock64();
      if (ts == 0) ts = now;
      else if (now - ts > G_SPIN_TIMEOUT) {
        __hip_atomic_store(status, 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

LBWN_DEV void put_granule(unsigned long long* g, unsigned tag, float v) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// ring slot DMA with sc1 (L2-served): a tap line this CU read d steps ago may still sit in its L1
LBWN_DEV void dma4_sc1(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 16);
}


template <bool LC, bool FILT>
LBWN_DEV void persist_chain(const PersistK& a, float* sm, int b, long long* stepc, long long* trace) {
  float* RING = sm;                  // [G_NS][G_SLOT]
  float* XP = sm + G_NS * G_SLOT;    // [L][32] dilated taps of this step
  float* DL = XP + P_DLROW * 32;     // [2][256] half-sums of the partial logits of the step being drawn
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, L = a.L, n = a.n_steps;
  const long long t0 = *stepc;
  const long GT = (long)n * L;       // layers of the run, in order: global index g = s·L + l

  if (wid >= 4) {   // ---- loader waves
    const int lw = wid - 4;
    const float* zeros = a.img + GI_WR + 128;
    auto taps = [&](long long t) {   // as gen_wave (a), for step t
      const int h = lane >> 5, c = lane & 31;
      long roff = 0;
      int bl = 0;
      for (int q = 0; 2 * q < L; ++q) {
        const int dE = 1 << bl;
        const long roffO = roff + (long)dE * a.B * a.Cr;
        const int blO = (bl + 1 == a.nbl) ? 0 : bl + 1;
        const int dO = 1 << blO;
        if ((q & 3) == lw) {
          const int d = h ? dO : dE, l = 2 * q + h;
          const float* src = (l < L && c < a.Cr)
                                 ? a.rings + (h ? roffO : roff) + ((long)b * d + (t & (d - 1))) * a.Cr + c
                                 : zeros + c;
          dma4_sc1(src, XP + 2 * q * 32);
        }
        roff = roffO + (long)dO * a.B * a.Cr;
        bl = (blO + 1 == a.nbl) ? 0 : blO + 1;
      }
    };
    // the layer and ring slot of the next issue, advanced with wrap-around: g mod L and g mod G_NS
    // of a 64-bit g were two long divisions per layer on the loaders' path to every barrier
    int iss_l = 0, iss_slot = 0;
    int iss_c = LC ? (int)(t0 % a.NC) : 0;   // cond-ring slot of the issued layer's step (t mod NC)
    auto issue = [&](long /*g: layer iss_l, slot iss_slot*/) {   // weights of global layer g into slot g mod G_NS
      const int l = iss_l;
      const float* src = a.img + (long)l * GIMG;
      float* dst = RING + iss_slot * G_SLOT;
      const int cs = iss_c;
      iss_l = (iss_l + 1 == L) ? 0 : iss_l + 1;
      if constexpr (LC) {
        if (iss_l == 0) iss_c = (iss_c + 1 == a.NC) ? 0 : iss_c + 1;
      }
      iss_slot = (iss_slot + 1 == G_NS) ? 0 : iss_slot + 1;
#pragma unroll
      for (int p = 0; p < G_PIECES; ++p) {
        const int pc = lw * G_PIECES + p;
        dma16(src + pc * 256 + lane * 4, dst + pc * 256);
      }
      const float* row = lw < 2 ? src + GI_WR + lw * 64
                       : lw == 2 ? (a.gc_proj ? a.gc_proj + ((long)l * a.B + b) * 64 : zeros)
                                 : zeros;
      if constexpr (LC) {
        if (lw == 3) row = a.lccond + (((long)cs * L + l) * a.B + b) * 64;
      }
      dma4(row + lane, dst + GI_WR + lw * 64);
    };
    taps(t0);
    long issued = 0;
    for (; issued < G_NS - 1 && issued < GT; ++issued) issue(issued);
    auto gather_half = [&](long long t) {   // partial logits of heads 16..31 for code q
      const int q = min((int)threadIdx.x - 256, a.Q - 1);
      float v[P_NH / 2], sum = 0.f;
      sweep<P_NH / 2>(a.lg, (unsigned)(((P_NH / 2) * a.B + b) * a.Q + q), (unsigned)(a.B * a.Q), P_NH / 2, (unsigned)t,
                      v, a.status);
#pragma unroll
      for (int i = 0; i < P_NH / 2; ++i) sum += v[i];
      DL[256 + q] = sum;
    };
    for (int s = 0; s < n; ++s) {
      if (s > 0) {
        gather_half(t0 + s);
        lds_barrier();   // D: the previous step's logits are in DL
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();              // -1: taps and the first slot landed, every wave's XW written
      for (int k = 0; k < L; ++k) {
        const long G = (long)s * L + k;
        // barrier G releases the residual of layer G and the conv of G+1: retire all but the
        // slots younger than G+1
        const long younger = (issued - 1) - (G + 1);
        if (younger >= G_NS - 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * (G_NS - 3)) : "memory");
        else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * 2) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        if (issued < GT) issue(issued++);   // into the slot of layer G-1 (dead after barrier G)
        if (k == L - 1 && s + 1 < n) taps(t0 + s + 1);   // the ring stores of step s landed (compute waves drained)
      }
    }
    gather_half(t0 + n);
    lds_barrier();   // D of the run's last draw
    return;
  }

  // ---- compute waves
  const int w = wid, Cr = a.Cr, Cd = a.Cd;
  const int c = lane >> 3, sg = (lane >> 2) & 1, kq = lane & 3, kp = lane & 7;
  const int ch = 8 * w + c, o = 32 * sg + ch;
  const bool lead = kp == 0;
  const int rc = lane & 31, rh = lane >> 5;
  float* XW = XP + (G_MAXL + 2) * 32 + 32 * w;
  float* Z = XP + (G_MAXL + 2) * 32 + 128;
  const int Q = a.Q, per = (Q + 63) >> 6, c0 = lane * per;
  long long* tr = (trace && b == 0 && threadIdx.x == 0) ? trace : nullptr;
  float bq[4];               // b2 of this lane's codes, loaded once (a global load in every draw before)
#pragma unroll
  for (int j = 0; j < 4; ++j) bq[j] = a.draw.bias ? a.draw.bias[min(c0 + j, Q - 1)] : 0.f;
  int code = a.code_in[b];   // step 0 of the run: the previous run's last draw (-1 at t = 0)
  float accd = 0.f;          // the dilated-tap partial of the next layer's conv
  auto dilated = [&](const float* Sl, int l) {
    const floatx4 w0 = *(const floatx4*)(Sl + (w * 4) * 256 + lane * 4);
    const floatx4 w1 = *(const floatx4*)(Sl + (w * 4 + 1) * 256 + lane * 4);
    const floatx4 x0 = *(const floatx4*)(XP + l * 32 + 8 * kq), x1 = *(const floatx4*)(XP + l * 32 + 8 * kq + 4);
    return dot4(w1, x1, dot4(w0, x0, 0.f));
  };
  int slot = 0;              // ring slot of global layer G = s·L + l (G mod G_NS, advanced per layer)
  for (int s = 0; s <= n; ++s) {
    const long long t = t0 + s;
    if (s > 0) {
      // draw step t-1: code q's partial logits of heads 0..15 here, 16..31 by the loader waves;
      // logit = (Σ first half + Σ second half) + b2
      const int q = min((int)threadIdx.x, Q - 1);
      float v[P_NH / 2], lsum = 0.f;
      sweep<P_NH / 2>(a.lg, (unsigned)(b * Q + q), (unsigned)(a.B * Q), P_NH / 2, (unsigned)t, v, a.status);
#pragma unroll
      for (int i = 0; i < P_NH / 2; ++i) lsum += v[i];
      DL[q] = lsum;
      if (tr && s == n) tr[5] = wall_clock64();
      lds_barrier();   // D
      if (tr && s == n) tr[7] = wall_clock64();
      float lv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = min(c0 + j, Q - 1);
        lv[j] = DL[cc] + DL[256 + cc];
        if (a.draw.bias) lv[j] += bq[j];
      }
      if constexpr (FILT) code = draw_core_filt<4>(lv, a.draw, b, t - 1, w == 0, false);
      else code = draw_core<4>(lv, a.draw, b, t - 1, w == 0, false);
      if (s == n) {
        if (tr) tr[6] = wall_clock64();
        break;
      }
    }
    if (tr && s == n - 1) tr[0] = wall_clock64();
    float x = 0.f;   // x[rc] of the current layer input: PRE row of the draw (+ PRE_BIAS); zero at t = 0
    if (rc < Cr) {
      if (code >= 0) x = a.pre[(long)code * Cr + rc];
      if (a.pre_bias && a.pre_b) x += a.pre_b[rc];
    }
    if (lane < 32) XW[rc] = x;
    long roff = 0;
    int bl = 0;
    lds_barrier();   // -1
    accd = dilated(RING + slot * G_SLOT, 0);   // this step's taps and layer 0's slot landed by -1
    for (int l = 0; l < L; ++l) {
      const float* S = RING + slot * G_SLOT;
      slot = (slot + 1 == G_NS) ? 0 : slot + 1;
      floatx4 wv[2], xv[2];   // the current tap's pieces; the dilated half is in accd
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        wv[mm] = *(const floatx4*)(S + (w * 4 + 2 + mm) * 256 + lane * 4);
        xv[mm] = *(const floatx4*)(XW + 8 * kq + 4 * mm);
      }
      float bco = S[GI_WR + o] + S[GI_WR + 128 + o];
      if (LC) bco += S[GI_WR + 192 + o];
      // (round 2: reading ALL of layer l+1's conv operands right after barrier l, and this layer's
      // residual weights ahead of the conv, measured 38.0 -> 38.9 us per step; what is kept is
      // the dilated half after the barrier and the residual weights just before the z write)
      // sub-layer cycle stamps (trace only): layers 16..23 of the traced step, 6 per layer
      // (compiled in only with -DLBWN_GEN_SUBSTAMPS=1: the lane-divergent stamp branches split the
      // layer into basic blocks the scheduler cannot overlap, 38.5 -> 44 us per step at B = 10)
      long long* st6 = (LBWN_GEN_SUBSTAMPS && tr && s == n - 1 && l >= 16 && l < 24 && L + 184 <= 2 * L + 136)
                           ? tr + 8 + L + 128 + 6 * (l - 16) : nullptr;
      if (st6) st6[0] = clock64();
      __builtin_amdgcn_sched_barrier(0);
      const int d = 1 << bl;
      if (rh == 0 && (rc >> 3) == w && rc < Cr) a.rings[roff + ((long)b * d + (t & (d - 1))) * Cr + rc] = x;
      roff += (long)d * a.B * Cr;
      bl = (bl + 1 == a.nbl) ? 0 : bl + 1;
      const float acc0 = dot4(wv[0], xv[0], accd), acc1 = dot4(wv[1], xv[1], 0.f);
      float v = acc0 + acc1;
      v += dpp<DPP_XOR1>(v);
      v += dpp<DPP_XOR2>(v);
      v += bco;
      if (st6) { asm volatile("" ::"v"(v)); st6[1] = clock64(); }
      const float vp = dpp<DPP_HALF_MIRROR>(v);
      const float z = gate_z(sg ? vp : v, sg ? v : vp);
      if (st6) { asm volatile("" ::"v"(z)); st6[2] = clock64(); }
      float* Zl = Z + (l & 1) * 32;
      // residual weights (slot resident since the last barrier) issued before the z write: the
      // barrier's lgkmcnt(0) retires them together with it, so only z is read after the barrier
      floatx4 rw[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rw[q] = *(const floatx4*)(S + GI_W + ((rh * 4 + q) * 32 + rc) * 4);
      const float bro = S[GI_WR + 64 + rc];
      if (lead) {
        Zl[ch] = z;
        if (ch < Cd) put_granule(a.zg + ((long)b * L + l) * 32 + ch, (unsigned)(t + 1), z);
      }
      // the last layer's ring stores must land before the loaders DMA the next step's taps
      if (l == L - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
      if (st6) st6[3] = clock64();
      accd = dilated(RING + slot * G_SLOT, min(l + 1, L - 1));   // layer l+1's slot landed by this barrier
      floatx4 zv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) zv[q] = *(const floatx4*)(Zl + 16 * rh + 4 * q);
      float r0 = dot4(rw[0], zv[0], 0.f), r1 = dot4(rw[1], zv[1], 0.f);
      r0 = dot4(rw[2], zv[2], r0);
      r1 = dot4(rw[3], zv[3], r1);
      const float r = r0 + r1;
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), __float_as_uint(r), false, false);
      x += (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + bro;
      if (st6) { asm volatile("" ::"v"(x)); st6[4] = clock64(); }
      if (lane < 32) XW[rc] = x;
      wave_sync();
      if (st6) st6[5] = clock64();
      if (tr && s == n - 1) tr[8 + l] = wall_clock64();
    }
    if (tr && s == n - 1) tr[1] = wall_clock64();
  }
  if (b % a.Bg == 0 && threadIdx.x == 0) *stepc = t0 + n;   // the group's blocks read it at their start
}

// the head's LDS carve (below) within the kernel's static allocation, at the largest Q (256)
static_assert(2 * P_LA * 528 + P_MAXB * 516 + 32 * 256 + 272 + 16 * 516 + 16 * 256 <= G_LDS, "head LDS");

LBWN_DEV void persist_head(const PersistK& a, int m, float* sm, int b0, int B, long long* stepc, long long* trace) {
  // B: this group's streams b0 .. b0+B-1 (granule and logit layouts are over all a.B streams)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = a.L, Cd = a.Cd, Cs = a.Cs, Cp = a.Cp, Q = a.Q, n = a.n_steps;
  const long long t0 = *stepc;
  // row paddings (33, 516, 17 floats) put the 16 stream rows a 16-lane MFMA operand read touches
  // on distinct banks (unpadded, the 32- / 512- / 16-float rows were 8- to 16-way conflicts)
  float* ZS = sm;                  // [2][P_LA layers][16 b][33] z of a round (double-buffered)
  float* RS = ZS + 2 * P_LA * 528; // [16 b][516] relu(skip + Σb), zero-padded
  float* HP = RS + P_MAXB * 516;   // [8 waves][64 lanes][4] MFMA partials (skip, then post1)
  float* HS = HP + 32 * 256;       // [16 b][17] h
  float* P1T = HS + 272;           // [16 c][516] POST1[:, 16m + c] (rows padded: conflict-free b128 reads)
  float* P2S = P1T + 16 * 516;     // [16 r][Q] POST2[16m + r, :]
  for (int e = tid; e < P_MAXB * 516; e += 512) RS[e] = 0.f;
  for (int e = tid; e < 16 * 512; e += 512) {   // the head's weight slices stay in LDS for the run
    const int cc = e >> 9, k = e & 511;
    P1T[cc * 516 + k] = (k < Cs && m * 16 + cc < Cp) ? a.post1[(long)k * Cp + m * 16 + cc] : 0.f;
  }
  for (int e = tid; e < 16 * Q; e += 512) {
    const int r = e / Q, q = e - r * Q;
    P2S[e] = (m * 16 + r < Cp) ? a.post2[(long)(m * 16 + r) * Q + q] : 0.f;
  }
  // lane roles: c = column within this block's 16, kg = tid >> 4 = 4·wave + (lane >> 4)
  const int c = tid & 15, kg = tid >> 4, kql = lane >> 4;
  const int scol = m * 16 + c, hcol = m * 16 + c, scol16 = m * 16;
  // A: wave wv takes layer l0 + wv of each round, lane quarter kql the channels 8kql..8kql+7
  const float* wsrc = a.skipw + (long)(8 * kql) * Cs + min(scol, Cs - 1);
  // C: post1 rows 16kg .. 16kg+15 of column hcol (P1T); post2 rows 16m .. 16m+15 of column tid (P2S)
  const float b1 = (hcol < Cp && a.post1_b) ? a.post1_b[hcol] : 0.f;
  // z granules polled by this thread: (stream zb0, channel zk) of every layer of a round
  const int zb0 = tid >> 5, zk = tid & 31;
  const bool zn0 = zb0 < B && zk < Cd;
  long long* tr = (trace && m == P_NH - 1 && tid == 0) ? trace : nullptr;
  for (int s = 0; s < n; ++s) {
    const unsigned tag = (unsigned)(t0 + s + 1);
    // A. skip columns, P_LA layers per round: the round's z granules (thread: stream tid >> 5,
    //    channel tid & 31, every layer of the round) and this lane's 8 weights arrive in one round
    //    trip; wave wv accumulates layer l0 + wv of each round into a 16x16 (stream x column)
    //    tile on v_mfma_f32_16x16x4_f32 (8 MFMAs over the layer's 32 channels: A[i = stream][k] =
    //    z, B[k][j = column] = SKIP), summed over the waves once after the last round.  (Round 3's
    //    per-thread FMAs re-read every z row for all 16 columns: ~260 KB of LDS per round.)
    floatx4 pacc = {0.f, 0.f, 0.f, 0.f};
    // rounds are aligned to the END of the stack: the last round is layer L-1 alone, so the
    // round before it finishes while the chains run their last layer and the tail after the
    // chains is one poll + one layer (the first round takes the remainder)
    const int first = (L - 1) % P_LA == 0 ? P_LA : (L - 1) % P_LA;
    const int i16 = lane & 15, kk = lane >> 4;
    for (int l0 = 0, r = 0; l0 < L; l0 += (l0 == 0 ? first : P_LA), ++r) {
      const int nl = l0 == L - 1 ? 1 : (l0 == 0 ? min(first, L) : P_LA), li = l0 + wv;
      float w8[8], zv[P_LA];
      const float* wl = a.skipw + (long)min(li, L - 1) * Cd * Cs + min(scol16 + i16, Cs - 1);
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) w8[s4] = wl[(long)min(4 * s4 + kk, Cd - 1) * Cs];
      sweep<P_LA>(a.zg, (unsigned)((b0 + (zn0 ? zb0 : 0)) * L + l0) * 32 + (zn0 ? zk : 0), 32u, nl, tag, zv, a.status);
      if (tr && s == n - 1) tr[8 + L + 40 + r] = wall_clock64();
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4)
        if (li >= L || 4 * s4 + kk >= Cd || scol16 + i16 >= Cs) w8[s4] = 0.f;
      float* Z = ZS + (r & 1) * (P_LA * 528);   // the other buffer's readers finished last round
#pragma unroll
      for (int i = 0; i < P_LA; ++i) Z[i * 528 + zb0 * 33 + zk] = (zn0 && i < nl) ? zv[i] : 0.f;
      __syncthreads();
      if (tr && s == n - 1) tr[8 + L + 80 + r] = wall_clock64();
      const float* zr = Z + wv * 528 + i16 * 33 + kk;
      float za[8];
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) za[s4] = zr[4 * s4];
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(za[s4], w8[s4], pacc, 0, 0, 0);
      if (tr && s == n - 1) tr[8 + L + r] = wall_clock64();
    }
    // the eight waves' tiles summed through LDS in a fixed order; thread (lane l, e): stream
    // 4(l >> 4) + e, column l & 15
    *(floatx4*)(HP + (wv * 64 + lane) * 4) = pacc;
    __syncthreads();
    if (tid < 256) {
      const int l = tid & 63, e = tid >> 6, sb = 4 * (l >> 4) + e, cc = l & 15;
      float v[8], x = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v[g] = HP[(g * 64 + l) * 4 + e];
#pragma unroll
      for (int g = 0; g < 8; ++g) x += v[g];
      if (sb < B && scol16 + cc < Cs) put_granule(a.sg + (long)(b0 + sb) * Cs + scol16 + cc, tag, x);   // B. publish
    }
    if (tr && s == n - 1) tr[2] = wall_clock64();
    // every head's own stamps (trace only): skip columns published, whole skip vector gathered
    long long* th = (trace && tid == 0 && s == n - 1) ? trace + 2 * L + 136 + 2 * m : nullptr;
    if (th) th[0] = wall_clock64();
    // B. gather the whole skip vector: thread k = tid polls column k of every stream
    if (tid < Cs) {
      // as many granule loads per poll as the group has streams, in fours (a group of 10 polled
      // 16 per thread before: 6 re-reads of its last stream)
      float v[P_MAXB];
      const unsigned o0 = (unsigned)(b0 * Cs + tid);
      if (B <= 4) sweep<4>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[4]>(v), a.status);
      else if (B <= 8) sweep<8>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[8]>(v), a.status);
      else if (B <= 12) sweep<12>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[12]>(v), a.status);
      else sweep<P_MAXB>(a.sg, o0, (unsigned)Cs, B, tag, v, a.status);
      const float bs = a.bsum ? a.bsum[tid] : 0.f;
#pragma unroll
      for (int bb = 0; bb < P_MAXB; ++bb)
        if (bb < B) RS[bb * 516 + tid] = fmaxf(v[bb] + bs, 0.f);
    }
    __syncthreads();
    if (tr && s == n - 1) tr[3] = wall_clock64();
    if (th) th[1] = wall_clock64();
    // C. h = relu(relu(skip + Σb)·POST1[:, cols] + b1) for this block's 16 columns and all 16
    //    stream slots on v_mfma_f32_16x16x4_f32 (exact f32 products): wave wv takes K rows
    //    64wv .. 64wv+63 (16 MFMAs; A[i = stream][k] = RS, B[k][j = column] = P1T), the eight
    //    16x16 partials are summed through LDS in a fixed order.  (Round 3's per-thread FMA form
    //    re-read each RS row for all 16 columns: ~390 KB of LDS reads, ~1.1 us.)
    {
      const int i16 = lane & 15, kk = lane >> 4, k0 = 64 * wv;
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
      float av[16], bv[16];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        av[s4] = RS[i16 * 516 + k0 + 4 * s4 + kk];
        bv[s4] = P1T[i16 * 516 + k0 + 4 * s4 + kk];
      }
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], bv[s4], acc, 0, 0, 0);
      *(floatx4*)(HP + (wv * 64 + lane) * 4) = acc;   // lane-linear: D[4kk + e][i16]
    }
    if (tr && s == n - 1) tr[8 + L + 120] = wall_clock64();
    __syncthreads();
    if (tr && s == n - 1) tr[8 + L + 121] = wall_clock64();
    if (tid < 256) {   // (stream 4·(tid>>6... : element (lane l = tid & 63, e = tid >> 6) of every wave's D
      const int l = tid & 63, e = tid >> 6, sb = 4 * (l >> 4) + e, cc = l & 15;
      float v[8], hsum = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v[g] = HP[(g * 64 + l) * 4 + e];
#pragma unroll
      for (int g = 0; g < 8; ++g) hsum += v[g];
      const float b1c = (m * 16 + cc < Cp && a.post1_b) ? a.post1_b[m * 16 + cc] : 0.f;
      HS[sb * 17 + cc] = (m * 16 + cc < Cp) ? fmaxf(hsum + b1c, 0.f) : 0.f;
    }
    __syncthreads();
    if (tr && s == n - 1) tr[8 + L + 122] = wall_clock64();
    // partial logits over this block's 16 h rows: 16 code columns per MFMA block, blocks wv and
    // wv + 8 of the Q/16: A[i = stream][k = r] = HS, B[k][j = code] = P2S; lane (code, 4 streams)
    {
      const int i16 = lane & 15, kk = lane >> 4;
      float av[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) av[s4] = HS[i16 * 17 + 4 * s4 + kk];
      for (int qb = wv; qb < (Q + 15) / 16; qb += 8) {
        const int q = min(16 * qb + i16, Q - 1);
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], P2S[(4 * s4 + kk) * Q + q], acc, 0, 0, 0);
        if (16 * qb + i16 < Q) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * kk + e < B) put_granule(a.lg + ((long)m * a.B + b0 + 4 * kk + e) * Q + q, tag, acc[e]);
        }
      }
    }
    if (tr && s == n - 1) tr[4] = wall_clock64();
  }
}

// FILT: the chain blocks draw with draw_core_filt (the head blocks are the same code either way)
template <bool LC, bool FILT>
__global__ __launch_bounds__(512) void gen_persist_kernel(PersistK a) {
  __shared__ __attribute__((aligned(16))) float sm[G_LDS];
  const int per = a.Bg + P_NH, g = blockIdx.x / per, r = blockIdx.x % per;
  const int b0 = g * a.Bg, Bg = min(a.Bg, a.B - b0);
  long long* stepc = g ? a.gstep + (g - 1) : a.step;
  long long* trace = g ? nullptr : a.trace;
  if (r < Bg) persist_chain<LC, FILT>(a, sm, b0 + r, stepc, trace);
  else if (r >= a.Bg) persist_head(a, r - a.Bg, sm, b0, Bg, stepc, trace);
  // (a ragged last group leaves chain slots r in [Bg, a.Bg) idle)
}

// gc_proj[l][b][o] = GC_EMBED[gc_id[b]] · [GC_SIGNAL_l | GC_GATE_l]  (imodel.py:53-56, :113-118)
// one element (the sum in k order; gen_begin_kernel forms a restarted stream's row with the same code)
LBWN_DEV float gc_proj_elem(const float* emb, const float* gsig, const float* ggate, int id, int l, int o, int Ge,
                            int Cd) {
  const int oc = o & 31;
  float s = 0.f;
  if (oc < Cd) {
    const float* G = (o < 32 ? gsig : ggate) + (long)l * Ge * Cd;
    const float* em = emb + (long)id * Ge;
    for (int k = 0; k < Ge; ++k) s += em[k] * G[k * Cd + oc];
  }
  return s;
}
__global__ void gen_gc_proj_kernel(const float* emb, const float* gsig, const float* ggate, const int* ids,
                                   float* out, int B, int Ge, int Cd) {
  const int l = blockIdx.x;
  for (int e = threadIdx.x; e < B * 64; e += blockDim.x) {
    const int b = e / 64, o = e % 64;
    out[((long)l * B + b) * 64 + o] = gc_proj_elem(emb, gsig, ggate, ids[b], l, o, Ge, Cd);
  }
}

// ---- local conditioning: the cond ring ----------------------------------------------------
// lccond[t mod NC][l][b][o] = lc[b][r(t)] · [LC_SIGNAL_l | LC_GATE_l][:, o]  (tmodel.py:155-160) for
// the next n <= NC steps t = *step + j, r(t) = min(max(t-1, 0), n_rows-1): generation step t is
// training position t-1, step 0 and steps past the mel take the nearest row.  Hoisted out of the
// step kernels: inside the chain the n_lc_out x 64 product per layer would sit on the serial
// path (arch5: 80 x 64 beside the conv's 64 x 64); here it is one launch per NC steps.
// Block = (layer l, LCP_ROWS rows m = j·B + b); thread (o = tid & 63, row group tid >> 6): 16 rows x
// one output column, plain f32 FMAs in k order (the lc rows staged in LDS and read as broadcasts,
// the weight column coalesced over o and read once per 64 rows).  t and n_rows come from device words, so the launch is
// capturable and a replayed graph follows a mel loaded later.
// SESS (lbwn_gen_begin): every stream has its own region of "lc" (lc_stride rows apart) and its own
// step origin and row count in the session words: r = min(max(t - base_b - 1, 0), rows_b - 1).
constexpr int LCP_KT = 128;   // k tile staged per pass
constexpr int LCP_ROWS = 64, LCP_RPT = LCP_ROWS / 4;   // rows per block / per thread

struct LcProjK {
  const float* lc; const float* wsig; const float* wgate; float* out;
  const long long* step; const int* n_rows;
  int B, L, Lo, Cd, NC, n;
  const long long* sess; long lc_stride;   // SESS only
};

template <bool SESS>
__global__ __launch_bounds__(256) void gen_lc_proj_kernel(LcProjK a) {
  __shared__ __attribute__((aligned(16))) float xs[LCP_ROWS][LCP_KT];
  const int tid = threadIdx.x, l = blockIdx.x, m0 = blockIdx.y * LCP_ROWS, M = a.n * a.B;
  const long long t0 = *a.step;
  const int n_rows = SESS ? 1 : max(*a.n_rows, 1);
  const int o = tid & 63, oc = o & 31, rq = tid >> 6;
  const bool ocv = oc < a.Cd;
  const float* W = (o < 32 ? a.wsig : a.wgate) + (long)l * a.Lo * a.Cd + min(oc, a.Cd - 1);
  float acc[LCP_RPT];
#pragma unroll
  for (int r = 0; r < LCP_RPT; ++r) acc[r] = 0.f;
  // SESS: each block row's lc row index once, through LDS (the words are two dependent loads ahead of
  // the row's address otherwise, for every float4 of the row)
  __shared__ long srow[SESS ? LCP_ROWS : 1];
  if (SESS) {
    if (tid < LCP_ROWS) {
      const int m = min(m0 + tid, M - 1), b = m % a.B;
      const long long rows = max(a.sess[4 * b + 2], 1LL);
      const long long r = min(max(t0 + m / a.B - a.sess[4 * b] - 1, 0LL), rows - 1);
      srow[tid] = (long)b * a.lc_stride + (long)r;
    }
    __syncthreads();
  }
  for (int k0 = 0; k0 < a.Lo; k0 += LCP_KT) {
    const int kt = min(LCP_KT, a.Lo - k0), kt4 = kt >> 2;   // Lo is a multiple of 4
    if (k0) __syncthreads();
    for (int e = tid; e < LCP_ROWS * kt4; e += 256) {
      const int j = e / kt4, k = 4 * (e % kt4), m = min(m0 + j, M - 1);
      const int b = m % a.B;
      const long long t = t0 + m / a.B;
      if (SESS) {
        *(floatx4*)&xs[j][k] = *(const floatx4*)(a.lc + srow[j] * a.Lo + k0 + k);
      } else {
        const long long r = min(max(t - 1, 0LL), (long long)n_rows - 1);
        *(floatx4*)&xs[j][k] = *(const floatx4*)(a.lc + ((long)b * n_rows + r) * a.Lo + k0 + k);
      }
    }
    __syncthreads();
    for (int k = 0; k < kt; k += 4) {
      float w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = W[(long)(k0 + k + i) * a.Cd];
#pragma unroll
      for (int r = 0; r < LCP_RPT; ++r) {
        const floatx4 x = *(const floatx4*)&xs[LCP_RPT * rq + r][k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r] = fmaf(x[i], w[i], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LCP_RPT; ++r) {
    const int m = m0 + LCP_RPT * rq + r;
    if (m >= M) break;
    const int b = m % a.B, slot = (int)((t0 + m / a.B) % a.NC);
    a.out[(((long)slot * a.L + l) * a.B + b) * 64 + o] = ocv ? acc[r] : 0.f;
  }
}

__global__ void gen_set_word_kernel(int* dst, int v) { *dst = v; }

__global__ void gen_reset_kernel(float* rings, long n_ring, unsigned long long* gran, long n_gran, int* code, int B,
                                 long long* step, int* status) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n_ring; e += (long)gridDim.x * blockDim.x)
    rings[e] = 0.f;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n_gran; e += (long)gridDim.x * blockDim.x)
    gran[e] = 0ull;   // tags restart at 1 with the step counter
  if (blockIdx.x == 0) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) code[b] = -1;
    if (threadIdx.x == 0) {
      *step = 0;
      *status = 0;
    }
  }
}

// ---- sessions (lbwn_gen_begin) --------------------------------------------------
// Restart the listed streams between two runs: block (l, i) zeroes stream slot[i]'s [d_l][Cr] block of
// ring l and forms its GC projection row of layer l (gen_gc_proj_kernel's sum); block (0, i) also writes
// the stream's session words {base = *step, key, rows, 0} and its pending code -1 (the zero vector).
// init_all (the first begin since lbwn_gen_start): block (0, 0) gives every stream the launch does not
// list the words lbwn_gen_start stands for, {0, b, 0, 0}.  The list travels in the kernel arguments
// (host memory read at the call, no copy): GB_MAX entries per launch.
constexpr int GB_MAX = 128;
struct BeginK {
  float* rings; int* code; const long long* step; long long* sess;
  const float* emb; const float* gsig; const float* ggate; float* gcp;   // emb null: no GC
  int B, L, nbl, Cr, Ge, Cd, n, init_all;
  int slot[GB_MAX], gc_id[GB_MAX], key[GB_MAX], rows[GB_MAX];
};

__global__ __launch_bounds__(256) void gen_begin_kernel(BeginK a) {
  const int l = blockIdx.x, i = blockIdx.y, b = a.slot[i];
  long roff = 0;   // ring offset of layer l
  for (int k = 0; k < l; ++k) roff += (long)(1 << (k % a.nbl)) * a.B * a.Cr;
  const int d = 1 << (l % a.nbl);
  float* ring = a.rings + roff + (long)b * d * a.Cr;
  for (int e = threadIdx.x; e < d * a.Cr; e += blockDim.x) ring[e] = 0.f;
  if (a.emb) {
    for (int o = threadIdx.x; o < 64; o += blockDim.x)
      a.gcp[((long)l * a.B + b) * 64 + o] = gc_proj_elem(a.emb, a.gsig, a.ggate, a.gc_id[i], l, o, a.Ge, a.Cd);
  }
  if (l != 0) return;
  if (i == 0 && a.init_all) {
    for (int s = threadIdx.x; s < a.B; s += blockDim.x) {
      bool listed = false;
      for (int j = 0; j < a.n; ++j) listed |= a.slot[j] == s;
      if (!listed) {
        a.sess[4 * s] = 0; a.sess[4 * s + 1] = s; a.sess[4 * s + 2] = 0; a.sess[4 * s + 3] = 0;
      }
    }
  }
  if (threadIdx.x == 0) {
    a.sess[4 * b] = *a.step; a.sess[4 * b + 1] = a.key[i]; a.sess[4 * b + 2] = a.rows[i]; a.sess[4 * b + 3] = 0;
    a.code[b] = -1;
  }
}

// ---- parallel prompt prefill (lbwn_gen_prefill) -------------------------------
// n steps whose inputs are known are a training-style forward over n positions: per slice of T
// positions, layer by layer through layer_fwd_kernel on two ping-pong halo buffers [B][H+T][Cr].
// The generator's rings are the D-separation state between slices: layer l's halo rows [H-d, H) are
// the ring slots of steps t0s-d .. t0s-1 (slots never written since gen_reset are zero = the
// reference's zero lookback, so negative times need no case), and the slice's last min(d, T) inputs
// go back into the ring.  t0s = *step + off: the step counter is only read until the finish kernel.

// an input code as the step kernels may read it: pending -1 stays "zero vector", the rest inside PRE
LBWN_DEV int prefill_clamp(int c, int Q) { return min(max(c, 0), Q - 1); }

// layer 0's body rows of the slice: row j = PRE[in_j] (+ PRE_BIAS), in_j = the input of step
// t0 + off + j: the pending code[b] for the call's first step, else codes[b][off + j - 1];
// ids[b][j] = b (the per-stream GC table's row).  V4: one float4 per item (Cr % 4 == 0, aligned).
struct PrefillE {
  const float* pre; const float* pre_b; const int* codes; const int* code; float* x; int* ids;
  long ld_codes, off;
  int B, T, H, Cr, Q, bias;
};
template <bool V4>
__global__ void gen_prefill_embed_kernel(PrefillE a) {
  const int cw = V4 ? a.Cr >> 2 : a.Cr;
  const long total = (long)a.B * a.T * cw;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % cw);
    const long r = e / cw;
    const int j = (int)(r % a.T), b = (int)(r / a.T);
    const long g = a.off + j;
    int q = g == 0 ? a.code[b] : a.codes[(long)b * a.ld_codes + g - 1];
    if (g > 0 || q >= 0) q = prefill_clamp(q, a.Q);
    float* dst = a.x + ((long)b * (a.H + a.T) + a.H + j) * a.Cr;
    if (V4) {
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (q >= 0) v = *(const floatx4*)(a.pre + (long)q * a.Cr + 4 * c);
      if (a.bias) v += *(const floatx4*)(a.pre_b + 4 * c);
      *(floatx4*)(dst + 4 * c) = v;
    } else {
      float v = q >= 0 ? a.pre[(long)q * a.Cr + c] : 0.f;
      if (a.bias) v += a.pre_b[c];
      dst[c] = v;
    }
    if (c == 0 && a.ids) a.ids[(long)b * a.T + j] = b;
  }
}

// Two independent copies of one slice in one launch (either may be absent):
//   gen_body_to_ring  the last min(dw, T) body rows of layer l's input -> their slots of ring l
//   gen_ring_to_halo  ring l+1's slots of steps t0s-dr .. t0s-1 -> halo rows [H-dr, H) of layer l+1's input
// They touch different layers' rings and different buffers.  For ONE layer the halo copy comes a
// launch earlier in stream order than the ring write: with T < d the slots written (steps t0s ..)
// alias the oldest slots the halo copy reads (steps t0s-d ..).
struct PrefillX {
  const long long* step; long off;
  const float* src; float* ring_w; int dw;
  const float* ring_r; float* dst; int dr;
  int B, T, H, Cr;
};
template <bool V4>
__global__ void gen_prefill_xfer_kernel(PrefillX a) {
  const int cw = V4 ? a.Cr >> 2 : a.Cr;
  const long long t0s = *a.step + a.off;
  const int nw = a.ring_w ? min(a.dw, a.T) : 0, nr = a.ring_r ? a.dr : 0;
  const long tw = (long)a.B * nw * cw, total = tw + (long)a.B * nr * cw;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const float* s;
    float* d;
    if (e < tw) {   // body -> ring
      const int c = (int)(e % cw);
      const long r = e / cw;
      const int i = (int)(r % nw), b = (int)(r / nw), j = a.T - nw + i;
      const long slot = (long)((t0s + j) & (long long)(a.dw - 1));
      s = a.src + ((long)b * (a.H + a.T) + a.H + j) * a.Cr;
      d = a.ring_w + ((long)b * a.dw + slot) * a.Cr;
      if (V4) *(floatx4*)(d + 4 * c) = *(const floatx4*)(s + 4 * c);
      else d[c] = s[c];
    } else {        // ring -> halo
      const long f = e - tw;
      const int c = (int)(f % cw);
      const long r = f / cw;
      const int i = (int)(r % nr), b = (int)(r / nr);
      const long slot = (long)((t0s - a.dr + i) & (long long)(a.dr - 1));   // two's complement: also for t < 0
      s = a.ring_r + ((long)b * a.dr + slot) * a.Cr;
      d = a.dst + ((long)b * (a.H + a.T) + a.H - a.dr + i) * a.Cr;
      if (V4) *(floatx4*)(d + 4 * c) = *(const floatx4*)(s + 4 * c);
      else d[c] = s[c];
    }
  }
}

// the per-stream GC rows of the step kernels (gc_proj [L][B][sig 32 | gate 32]) as layer_fwd's table
// [L][B][sig Cd | gate Cd]: the same sums the sequential path adds
__global__ void gen_prefill_gctab_kernel(const float* gc_proj, float* out, long rows, int Cd) {
  const long total = rows * 2 * Cd;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int o = (int)(e % (2 * Cd));
    out[e] = gc_proj[(e / (2 * Cd)) * 64 + (o < Cd ? o : 32 + o - Cd)];
  }
}

// The LC term of one prefill slice for the G consecutive layers l0 .. l0+G-1:
//   out[m][g·2Cd + o] = Σ_k lc[b][r][k] · [LC_SIGNAL_l | LC_GATE_l][k][o],  l = l0 + g, o < 2Cd,
// m = b·T + j the row order layer_fwd_kernel reads (cond + m·ldcond), row stride ld, r = r(t0s + j)
// of gen_lc_proj_kernel from the same two device words.  Exact f32 on the matrix cores
// (v_mfma_f32_32x32x2_f32): the weights are the row operand (rows = out channel, as layer.hip's
// accumulators), the gathered lc rows the column operand, k ascending into ONE accumulator per
// 32 x 32 tile, so each output is the fmaf chain in k order that gen_lc_proj_kernel computes.  A
// wave owns one tile: 32 positions x the signal or the gate half; the MFMA's dependent-accumulator
// latency equals its issue interval, so the one chain keeps the pipe full, and the SIMD's second
// wave (the other half of the same positions) issues while this one waits for its LDS reads.  A
// lane ends with 4 consecutive out channels of one position per accumulator quad and stores them
// as one float4 along o.
// Block = PLC_POS = 128 rows m, 8 waves (signal | gate, 4 waves of 32 positions each).  LDS, both
// k-major so that every operand read is one conflict-free ds_read_b32 (the two lane halves read
// rows k = 2s, 2s + 1):
//   Xs [kt][PLC_POS]  the lc rows of the block's positions, staged once per block while n_lc_out <= PLC_KT
//   Ws [kt][64]       one layer's [signal 32 | gate 32] columns, zero past n_dil; the next layer's are
//                     fetched into registers while this layer's MFMAs issue
// n_lc_out > PLC_KT takes ceil(n_lc_out / PLC_KT) passes per layer into the same accumulators and
// restages Xs for each.
constexpr int PLC_POS = 128, PLC_NW = PLC_POS / 32;   // positions per block, waves per tile half (64 positions: 11 % slower)
constexpr int PLC_THREADS = 128 * PLC_NW, PLC_KW = PLC_THREADS / 64;
constexpr int PLC_KT = 80;   // Xs + Ws = 60 KB of the 64 KB of static LDS (arch5's n_lc_out: one pass)
constexpr int PLC_WR = PLC_KT * 64 / PLC_THREADS;   // weight words a thread carries between passes
static_assert(PLC_KT % 4 == 0 && PLC_WR * PLC_THREADS == PLC_KT * 64 && PLC_KT * (PLC_POS + 64) * 4 <= 65536,
              "PLC tile");

struct PrefillLC {
  const float* lc; const float* wsig; const float* wgate; float* out;
  const long long* step; const int* n_rows;
  long off, ld;
  int B, T, Lo, Cd, l0, G, v4;   // v4: n_dil % 4 == 0 and a 16-byte aligned workspace (float4 stores)
};

// thread (o = tid & 63, k = tid >> 6 + PLC_KW·i): unconditional loads at clamped indices, then selected
LBWN_DEV void plc_load_w(const PrefillLC& a, int l, int k0, int kt, int tid, float (&wr)[PLC_WR]) {
  const int o = tid & 63, oc = o & 31;
  const float* W = (o < 32 ? a.wsig : a.wgate) + ((long)l * a.Lo + k0) * a.Cd + min(oc, a.Cd - 1);
#pragma unroll
  for (int i = 0; i < PLC_WR; ++i) {
    const int k = (tid >> 6) + PLC_KW * i;
    wr[i] = W[(long)min(k, kt - 1) * a.Cd];
    if (k >= kt || oc >= a.Cd) wr[i] = 0.f;
  }
}

__global__ __launch_bounds__(PLC_THREADS) void gen_prefill_lcproj_kernel(PrefillLC a) {
  __shared__ __attribute__((aligned(16))) float sm[PLC_KT * (PLC_POS + 64)];
  float* Xs = sm;
  float* Ws = sm + PLC_KT * PLC_POS;
  const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) % PLC_NW, gate = tid / (64 * PLC_NW);
  const int pi = lane & 31, h = lane >> 5;
  const long M = (long)a.B * a.T, m0 = (long)blockIdx.x * PLC_POS;
  const long long t0s = *a.step + a.off;
  const int n_rows = max(*a.n_rows, 1);
  const int npass = (a.Lo + PLC_KT - 1) / PLC_KT, nst = a.G * npass;
  const long m = m0 + 32 * w + pi;
  const bool v4 = a.v4 != 0;
  float wr[PLC_WR];
  plc_load_w(a, a.l0, 0, min(PLC_KT, a.Lo), tid, wr);
  floatx16 acc;
  for (int p = 0; p < nst; ++p) {
    const int g = p / npass, k0 = (p % npass) * PLC_KT, kt = min(PLC_KT, a.Lo - k0);
    if (p) __syncthreads();   // the previous pass's LDS reads are done
    if (p == 0 || npass > 1) {
      // Xs[k][pos]: lanes along pos (conflict-free stores); a position's row is contiguous in "lc",
      // and consecutive positions of a stream are consecutive rows except at the two clamps
      const int kt4 = kt >> 2;   // Lo is a multiple of 4
      for (int e = tid; e < PLC_POS * kt4; e += PLC_THREADS) {
        const int pos = e & (PLC_POS - 1), k = 4 * (e / PLC_POS);
        const long mm = min(m0 + pos, M - 1);
        const long b = mm / a.T;
        const long long r = min(max(t0s + (mm - b * a.T) - 1, 0LL), (long long)n_rows - 1);
        const floatx4 x = *(const floatx4*)(a.lc + ((long)b * n_rows + r) * a.Lo + k0 + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) Xs[(k + i) * PLC_POS + pos] = x[i];
      }
    }
#pragma unroll
    for (int i = 0; i < PLC_WR; ++i) Ws[((tid >> 6) + PLC_KW * i) * 64 + (tid & 63)] = wr[i];
    __syncthreads();
    if (p + 1 < nst) {   // in flight during the MFMAs below
      const int k1 = ((p + 1) % npass) * PLC_KT;
      plc_load_w(a, a.l0 + (p + 1) / npass, k1, min(PLC_KT, a.Lo - k1), tid, wr);
    }
    if (k0 == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    const float* xk = Xs + h * PLC_POS + 32 * w + pi;
    const float* wk = Ws + h * 64 + 32 * gate + pi;
    // lane half h supplies k = s + h.  Four MFMAs per group of LDS reads: one read latency per 256
    // MFMA cycles instead of one per 64 (kt is a multiple of 4: a last group of two)
    int s = 0;
    for (; s + 8 <= kt; s += 8) {
      float x[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[i] = xk[(s + 2 * i) * PLC_POS]; wv[i] = wk[(s + 2 * i) * 64]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = mfma32(wv[i], x[i], acc);
    }
    if (s < kt) {
      const float x0 = xk[s * PLC_POS], w0 = wk[s * 64], x1 = xk[(s + 2) * PLC_POS], w1 = wk[(s + 2) * 64];
      acc = mfma32(w0, x0, acc);
      acc = mfma32(w1, x1, acc);
    }
    if (k0 + kt == a.Lo && m < M) {
      float* row = a.out + m * a.ld + (long)g * 2 * a.Cd + gate * a.Cd;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 8 * q + 4 * h;   // acc_row(4q, h): this lane's 4 consecutive out channels
        if (v4) {
          if (o < a.Cd) *(floatx4*)(row + o) = floatx4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (o + i < a.Cd) row[o + i] = acc[4 * q + i];
        }
      }
    }
  }
}

// outputs of the prefilled steps: samples = the prompt, wav = its µ-law decode (the counter is only read)
__global__ void gen_prefill_out_kernel(const int* codes, long ld_codes, long n, const long long* step, int* samples,
                                       float* wav, long long max_steps, int B, int Q) {
  const long long t0 = *step;
  const long long span = min((long long)n, max(max_steps - t0, 0LL));
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)B * span;
       e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / span, j = e % span;
    const int q = prefill_clamp(codes[b * ld_codes + j], Q);
    samples[b * max_steps + t0 + j] = q;
    wav[b * max_steps + t0 + j] = mu_decode_q(q, Q);
  }
}

// last launch of a prefill, one block: the pending input, the plan's step counter and the
// persistent groups' (gstep[g-1], g = 1 .. ngroups-1)
__global__ void gen_prefill_finish_kernel(const int* codes, long ld_codes, long n, int* code, long long* step,
                                          long long* gstep, int ngroups, int B, int Q) {
  const long long t1 = *step + n;
  for (int b = threadIdx.x; b < B; b += blockDim.x) code[b] = prefill_clamp(codes[(long)b * ld_codes + n - 1], Q);
  __syncthreads();   // every thread has read *step
  for (int g = threadIdx.x; g < ngroups - 1; g += blockDim.x) gstep[g] = t1;
  if (threadIdx.x == 0) *step = t1;
}

// ---- teacher-forced scoring (lbwn_gen_score) -----------------------------------
// The head over every position of a prefill slice leaves its logits LG [B·T][Q] (row b·T + j = step
// t0 + off + j of stream b).  One wave per row: logp[b][off + j] = LG[c] - (m + log Σ exp(LG - m)) with
// c = the prompt's code at that step and m the row's max.  Each lane holds up to two float4 (Q <= 512,
// Q % 4 == 0); lanes past Q / 4 idle with -inf / 0.  last (nullable, the call's last slice): row T - 1
// of every stream is also the plan's "logits".
struct ScoreK {
  const float* lg; const int* codes; float* logp; float* last;
  long ld_codes, ld_logp, off;
  int B, T, Q;
};
constexpr int SC_ROWS = 4;   // rows (waves) per block
__global__ __launch_bounds__(64 * SC_ROWS) void gen_score_logp_kernel(ScoreK a) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * SC_ROWS + (threadIdx.x >> 6);
  if (r >= (long)a.B * a.T) return;   // whole waves leave: the DPP steps below see 64 lanes
  const int b = (int)(r / a.T), j = (int)(r % a.T);
  const float* row = a.lg + r * a.Q;
  const int nq = a.Q >> 2;
  floatx4 v[2];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (lane + 64 * i < nq) {
      v[i] = *(const floatx4*)(row + 4 * (lane + 64 * i));
      mx = fmaxf(fmaxf(mx, fmaxf(v[i][0], v[i][1])), fmaxf(v[i][2], v[i][3]));
    }
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (lane + 64 * i < nq) se += (expf(v[i][0] - mx) + expf(v[i][1] - mx)) + (expf(v[i][2] - mx) + expf(v[i][3] - mx));
  se = wave_sum(se);
  if (lane == 0) {
    const int c = prefill_clamp(a.codes[(long)b * a.ld_codes + a.off + j], a.Q);
    a.logp[(long)b * a.ld_logp + a.off + j] = row[c] - (mx + logf(se));
  }
  if (a.last && j == a.T - 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (lane + 64 * i < nq) *(floatx4*)(a.last + (long)b * a.Q + 4 * (lane + 64 * i)) = v[i];
  }
}

// ---- state snapshot (lbwn_gen_state_save / lbwn_gen_state_load) ----------------
// What a run is between two launches: the rings, the pending codes, the step counter (and the
// persistent groups' copies of it).  The snapshot is stream-major -- a 256-byte header, then per
// stream a record {code, 12 zero bytes, the stream's rings in layer order, each [d][Cr]} -- so it
// does not depend on the batch size of the plan that wrote it.  Position p (in rows of Cr floats) of
// a record, with m = 2^nbl - 1: block = p / m, r = p % m, bl = floor(log2(r + 1)), slot = r + 1 - 2^bl;
// the workspace row is (block·m + 2^bl - 1)·B + b·2^bl + slot (the layers before it, then [B][d]).
constexpr int GS_MAGIC = 0x5453424c;   // "LBST"
constexpr int GS_VERSION = 1;
constexpr int GS_HEADER = 256;         // bytes; int32 words 0..7 below, the step as int64 at byte 32
constexpr int GS_CODE = 16;            // bytes of a record before its rings
constexpr int GS_UNROLL = 4;           // independent loads per thread before the first store
constexpr int GS_STATUS = 6;           // "status" after a refused load

struct StateK {
  float* rings; int* code; long long* step; long long* gstep; int* status;
  unsigned long long* gran; long n_gran;   // the hand-off granules a load zeroes (without the groups' counters)
  char* state; const int* map;             // the snapshot; load: stream b takes record map[b] (null: b)
  long long max_steps;
  int B, nb, nbl, Cr, Q, rec_bytes, state_streams, ngroups;
};

// a load's refusals, by every block for itself before it writes anything: the header against the plan
// and the call, every map entry in range
LBWN_DEV bool state_refused(const StateK& a) {
  const int* h = reinterpret_cast<const int*>(a.state);
  const long long t = *reinterpret_cast<const long long*>(a.state + 32);
  int bad = !(h[0] == GS_MAGIC && h[1] == GS_VERSION && h[2] == a.state_streams && h[3] == a.nb && h[4] == a.nbl &&
              h[5] == a.Cr && h[6] == a.Q && h[7] == a.rec_bytes && t >= 0 && t <= a.max_steps);
  if (a.map)
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) bad |= a.map[b] < 0 || a.map[b] >= a.state_streams;
  return __syncthreads_or(bad) != 0;
}

// V4: 16 bytes per lane (Cr % 4 == 0, both sides 16-byte aligned), else 4.  LOAD: snapshot -> workspace
// (plus the granules, the codes and the counters), else workspace -> snapshot (plus the header).
template <bool V4, bool LOAD>
__global__ __launch_bounds__(256) void gen_state_copy_kernel(StateK a) {
  if (LOAD && state_refused(a)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.status = GS_STATUS;
    return;
  }
  typedef typename std::conditional<V4, floatx4, float>::type T;
  const int cw = V4 ? a.Cr >> 2 : a.Cr, m = (1 << a.nbl) - 1;
  const long per = (long)a.nb * m * cw, total = (long)a.B * per;   // items of one record, of the call
  const long stride = (long)gridDim.x * blockDim.x;
  auto ends = [&](long e, T*& w, T*& s) {   // the workspace and snapshot ends of item e
    const int b = (int)(e / per);
    const long r = e % per;
    const int c = (int)(r % cw), p = (int)(r / cw);
    const int rr = p % m, bl = 31 - __clz(rr + 1), slot = rr + 1 - (1 << bl);
    const long row = ((long)(p - rr) + (1 << bl) - 1) * a.B + ((long)b << bl) + slot;
    const long rec = LOAD && a.map ? a.map[b] : b;
    w = reinterpret_cast<T*>(a.rings + row * a.Cr) + c;
    s = reinterpret_cast<T*>(a.state + GS_HEADER + rec * a.rec_bytes + GS_CODE + 4L * p * a.Cr) + c;
  };
  for (long e0 = blockIdx.x * (long)blockDim.x + threadIdx.x; e0 < total; e0 += GS_UNROLL * stride) {
    T v[GS_UNROLL];
    T* dst[GS_UNROLL];
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) {
      const long e = e0 + u * stride;
      dst[u] = nullptr;
      if (e < total) {
        T *w, *s;
        ends(e, w, s);
        v[u] = LOAD ? *s : *w;
        dst[u] = LOAD ? w : s;
      }
    }
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u)
      if (dst[u]) *dst[u] = v[u];
  }
  if (LOAD) {   // no granule of the run that was here may carry a tag the loaded step polls for
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < a.n_gran; e += stride) a.gran[e] = 0ull;
  }
  if (blockIdx.x != 0) return;
  int* h = reinterpret_cast<int*>(a.state);
  if (LOAD) {
    const long long t = *reinterpret_cast<const long long*>(a.state + 32);
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
      const long rec = a.map ? a.map[b] : b;
      const int c = *reinterpret_cast<const int*>(a.state + GS_HEADER + rec * a.rec_bytes);
      a.code[b] = min(max(c, -1), a.Q - 1);   // what the step kernels may read: -1 or inside PRE
    }
    for (int g = threadIdx.x; g < a.ngroups - 1; g += blockDim.x) a.gstep[g] = t;
    if (threadIdx.x == 0) *a.step = t;
  } else {
    const int pad = (a.rec_bytes - GS_CODE) / 4 - a.nb * m * a.Cr;   // floats behind a record's rings (n_res % 4 != 0)
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
      int* r = reinterpret_cast<int*>(a.state + GS_HEADER + (long)b * a.rec_bytes);
      r[0] = a.code[b];
      r[1] = r[2] = r[3] = 0;
      for (int i = 0; i < pad; ++i) r[a.rec_bytes / 4 - 1 - i] = 0;
    }
    if (threadIdx.x == 0) {
      h[0] = GS_MAGIC; h[1] = GS_VERSION; h[2] = a.B; h[3] = a.nb; h[4] = a.nbl; h[5] = a.Cr; h[6] = a.Q;
      h[7] = a.rec_bytes;
      *reinterpret_cast<long long*>(a.state + 32) = *a.step;
    } else if (threadIdx.x >= 10 && threadIdx.x < GS_HEADER / 4) {
      h[threadIdx.x] = 0;
    }
  }
}

}  // namespace

// ---- host side: generation plan ----------------------------------------------------------

#include "../../include/lbwn.h"

struct lbwn_gen_plan {
  lbwn_arch a;
  int B, L, nbl, Cr, Cd, Cs, Cp, Q;
  long long max_steps;
  size_t oRING, oZCAT, oSKP, oHP, oLGP, oLOG, oSTEP, oCODE, oTEACH, oSAMP, oWAV, oGCP, oBSUM, oGIMG, oTRACE, total;
  size_t oGRAN;   // persistent form: granules [zg B·L·32 | sg B·Cs | lg P_NH·B·Q]
  // GEMM form (B > P_MAXB): skip / post1 / post2 as bf16-split MFMA GEMMs over the B streams
  // (split-K partial slabs in oGSPL) instead of the vector GEMVs
  size_t oGSPL = 0;
  int gsplit[3] = {1, 1, 1};
  long n_gran;
  bool trace, persist;
  int pgroups = 1, pbg = 0;   // persistent form: stream groups of pbg <= P_MAXB, each with its own P_NH heads
  long n_gran_core = 0;       // granules before the groups' step counters
  int ksl_skip, ks_skip, ks_h, ks_lg;
  long n_ring;
  long long n_teacher, max_teacher;
  unsigned long long seed;
  int pre_bias;
  // the draw's filters (lbwn_gen_set_sampling), normalised; host state like the seed, read by each
  // lbwn_gen_run at launch.  Neutral (1, 0, 1) launches the unfiltered kernels.
  float temperature = 1.f, top_p = 1.f;
  int top_k = 0;
  // local conditioning (Lo = 0: none): the upsampled mel "lc" [B][n_rows][Lo] (dense, n_rows =
  // the loaded mel's frames x hop <= lc_rows), the upsample stages' scratch, and the cond ring
  // "lccond" [NC][L][B][64]; the loaded n_rows also lives in the device word at oSTEP + 12
  int Li = 0, Lo = 0, nup = 0, up[8] = {1, 1, 1, 1, 1, 1, 1, 1}, NC = 0;
  long long hop = 1, lc_rows = 0;
  size_t oLC = 0, oLCACT[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oLCC = 0;
  bool up_fused = false, mel_loaded = false;
  // prefill (lbwn_gen_prefill): slice length, halo, and the scratch -- two halo
  // buffers [B][pfH + pfT][Cr], z [B·pfT][Cd], the L packed layer images, the per-stream GC table
  // [L][B][2·Cd] and ids [B][pfT]
  // LC plans: the projected LC terms of one slice for pfG consecutive layers, "pfcond" [B·pfT][pfG·2·Cd]
  int pfT = 0, pfH = 0, pfG = 0;
  size_t oPFX[2] = {0, 0}, oPFZ = 0, oPFIMG = 0, oPFGC = 0, oPFIDS = 0, oPFCOND = 0;
  int ncu = 0;   // the device's CUs at plan creation (0: none seen), the state copies' grid
  // sessions (lbwn_gen_begin): the words "sessions" int64 [B][4] at the very end of the workspace, over
  // the tail of the prefill scratch (prefill and score are refused in session mode, and the first begin
  // since lbwn_gen_start writes every stream's words); host-tracked like mel_loaded: a begin happened
  // since lbwn_gen_start, and which streams have begun a session
  size_t oSESS = 0;
  bool sess_mode = false;
  std::vector<unsigned char> sess_begun, sess_seen;
  int n_begun = 0;
};

constexpr int G_LC_CHUNK = 64;         // default NC (steps per projection launch / persistent sub-run)
constexpr int G_LC_CHUNK_MAX = 4096;
constexpr int G_PF_ROWS = 32768;       // default prefill slice: B·T_s rows per layer launch (the C2 launch size)
constexpr int G_PF_SLICE_MAX = 65536;
constexpr int G_PF_LC_GROUP = 8;       // default layers per prefill projection launch

// the per-step GEMM form: large B, shapes the split GEMM takes (N % 4, K % 4, row strides)
static bool gemm_form_ok(const lbwn_gen_plan* p) {
  return !p->persist && p->B > P_MAXB && p->Cs % 4 == 0 && p->Cp % 4 == 0 && p->Q % 4 == 0 && (p->L * p->Cd) % 4 == 0;
}

static size_t gcarve(size_t& cur, size_t bytes) {
  size_t o = cur;
  cur += (bytes + 255) / 256 * 256;
  return o;
}

extern "C" int lbwn_gen_plan_create(const lbwn_arch* a, int B, int64_t max_steps, int64_t max_teacher,
                                    lbwn_gen_plan** out) {
  LBWN_REQUIRE(a && out && B >= 1 && max_steps >= 1 && max_teacher >= 0, "gen_plan_create: bad arguments");
  LBWN_REQUIRE(a->n_res <= 32 && a->n_dil <= 32, "gen: n_res/n_dil must be <= 32");
  LBWN_REQUIRE(a->n_blocks * a->n_block_layers <= G_MAXL, "gen: more than %d layers (tap cache)", G_MAXL);
  LBWN_REQUIRE(a->n_quant <= 512, "gen: n_quant must be <= 512");
  // local conditioning: the training plan's limits (lbwn_plan_create)
  long long hop = 1;
  int lc_chunk = G_LC_CHUNK;
  const int n_layers = a->n_blocks * a->n_block_layers;
  int pf_group = std::min(G_PF_LC_GROUP, n_layers);
  if (a->n_lc_out > 0) {
    LBWN_REQUIRE(a->n_lc_upsample >= 1 && a->n_lc_upsample <= 8, "gen: LC needs 1..8 upsample stages");
    for (int i = 0; i < a->n_lc_upsample; ++i) {
      LBWN_REQUIRE(a->lc_upsample[i] >= 1, "gen: bad lc_upsample stride");
      hop *= a->lc_upsample[i];
      LBWN_REQUIRE(hop <= (1LL << 30), "gen: mel hop too large");
    }
    LBWN_REQUIRE(a->n_lc_in >= 4 && a->n_lc_in % 4 == 0 && a->n_lc_out % 4 == 0,
                 "gen: n_lc_in/n_lc_out must be multiples of 4");
    LBWN_REQUIRE((max_steps + hop - 1) / hop * hop < (1LL << 31), "gen: max_steps too large for an LC plan");
    if (const char* ce = getenv("LBWN_GEN_LC_CHUNK")) {
      char* end = nullptr;
      const long v = strtol(ce, &end, 10);
      LBWN_REQUIRE(end != ce && *end == 0 && v >= 1 && v <= G_LC_CHUNK_MAX,
                   "gen: LBWN_GEN_LC_CHUNK must be an integer in 1..%d (got '%s')", G_LC_CHUNK_MAX, ce);
      lc_chunk = (int)v;
    }
    LBWN_REQUIRE((long long)lc_chunk * B / LCP_ROWS < 65535, "gen: LBWN_GEN_LC_CHUNK %d x batch_sz %d is too large",
                 lc_chunk, B);   // the projection's grid: one block row per LCP_ROWS (step, stream) pairs
    if (const char* ge = getenv("LBWN_GEN_PREFILL_LC_GROUP")) {
      char* end = nullptr;
      const long v = strtol(ge, &end, 10);
      LBWN_REQUIRE(end != ge && *end == 0 && v >= 1 && v <= n_layers,
                   "gen: LBWN_GEN_PREFILL_LC_GROUP must be an integer in 1..%d, the number of layers (got '%s')",
                   n_layers, ge);
      pf_group = (int)v;
    }
  }
  // prefill slice length: the largest multiple of 128 with B·T_s <= G_PF_ROWS, at least 128
  int pf_slice = std::max(LBWN_LAYER_POS, G_PF_ROWS / B / LBWN_LAYER_POS * LBWN_LAYER_POS);
  if (const char* pe = getenv("LBWN_GEN_PREFILL_SLICE")) {
    char* end = nullptr;
    const long v = strtol(pe, &end, 10);
    LBWN_REQUIRE(end != pe && *end == 0 && v >= 1 && v <= G_PF_SLICE_MAX,
                 "gen: LBWN_GEN_PREFILL_SLICE must be an integer in 1..%d (got '%s')", G_PF_SLICE_MAX, pe);
    pf_slice = (int)v;
  }
  lbwn_gen_plan* p = new lbwn_gen_plan();
  p->a = *a;
  p->B = B;
  p->nbl = a->n_block_layers;
  p->L = a->n_blocks * a->n_block_layers;
  p->Cr = a->n_res; p->Cd = a->n_dil; p->Cs = a->n_skip; p->Cp = a->n_post; p->Q = a->n_quant;
  p->max_steps = max_steps;
  p->max_teacher = max_teacher;
  long dsum = (long)a->n_blocks * ((1L << a->n_block_layers) - 1);
  p->n_ring = dsum * B * p->Cr;
  size_t cur = 0;
  p->oRING = gcarve(cur, 4 * (size_t)p->n_ring);
  p->oZCAT = gcarve(cur, 4 * (size_t)B * p->L * p->Cd);
  // K-split GEMV partials: skip (K = L·Cd, 64-row slices), post1 and post2 (32-row slices)
  p->ksl_skip = 64;
  p->ks_skip = (p->L * p->Cd + p->ksl_skip - 1) / p->ksl_skip;
  p->ks_h = (p->Cs + 31) / 32;
  p->ks_lg = (p->Cp + 31) / 32;
  p->oSKP = gcarve(cur, 4 * (size_t)p->ks_skip * B * p->Cs);
  p->oHP = gcarve(cur, 4 * (size_t)p->ks_h * B * p->Cp);
  p->oLGP = gcarve(cur, 4 * (size_t)p->ks_lg * B * p->Q);
  p->oLOG = gcarve(cur, 4 * (size_t)B * p->Q);
  p->oSTEP = gcarve(cur, 16);   // step counter + status word
  p->oCODE = gcarve(cur, 4 * (size_t)B);
  p->oTEACH = gcarve(cur, 4 * (size_t)std::max<int64_t>(1, max_teacher));
  p->oSAMP = gcarve(cur, 4 * (size_t)B * max_steps);
  p->oWAV = gcarve(cur, 4 * (size_t)B * max_steps);
  p->oGCP = gcarve(cur, 4 * (size_t)p->L * B * 64);
  p->oBSUM = gcarve(cur, 4 * (size_t)p->Cs);
  p->oGIMG = gcarve(cur, 4 * (size_t)p->L * GIMG);
  p->oTRACE = gcarve(cur, 8 * (size_t)(2 * p->L + 8 + 128 + 2 * P_NH));
  p->trace = getenv("LBWN_GEN_TRACE") != nullptr;
  // persistent form: every block resident (one 512-thread block per CU), phase A maps
  // (16 skip columns × B streams) onto the threads, the draw's logits fit the tap table's tail
  int dev = 0, ncu = 0;
  const bool have_dev = hipGetDevice(&dev) == hipSuccess &&
                        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
  const char* pe = getenv("LBWN_GEN_PERSIST");
  // B > P_MAXB: ceil(B / P_MAXB) independent groups in the same launch while every block fits
  // (4 x (16 + 32) = 192 blocks for B = 64 on 256 CUs; beyond that the per-step GEMM form)
  p->pgroups = (B + P_MAXB - 1) / P_MAXB;
  p->pbg = (B + p->pgroups - 1) / p->pgroups;
  p->persist = (!pe || strcmp(pe, "0") != 0) && p->L <= P_MAXL && p->Q <= 256 && p->Cs <= 16 * P_NH &&
               p->Cp <= 16 * P_NH && have_dev && p->pgroups * (p->pbg + P_NH) <= ncu;
  p->ncu = have_dev ? ncu : 0;
  p->n_gran_core = (long)B * p->L * 32 + (long)B * p->Cs + (long)P_NH * B * p->Q;
  p->n_gran = p->n_gran_core + p->pgroups;   // + the groups' step counters (zeroed with the granules)
  p->oGRAN = gcarve(cur, 8 * (size_t)p->n_gran);
  if (gemm_form_ok(p)) {
    // split K until ~256 blocks of 128 x 128 tiles (M = B streams is short), >= 4 k-steps of 32 each
    const int Ns[3] = {p->Cs, p->Cp, p->Q}, Ks[3] = {p->L * p->Cd, p->Cs, p->Cp};
    long most = 0;
    for (int i = 0; i < 3; ++i) {
      const int tiles = ((B + 127) / 128) * ((Ns[i] + 127) / 128);
      p->gsplit[i] = std::max(1, std::min(256 / std::max(1, tiles), Ks[i] / 128));
      most = std::max(most, (long)p->gsplit[i] * B * Ns[i]);
    }
    p->oGSPL = gcarve(cur, 4 * (size_t)most);
  }
  if (a->n_lc_out > 0) {
    p->Li = a->n_lc_in; p->Lo = a->n_lc_out; p->nup = a->n_lc_upsample; p->hop = hop; p->NC = lc_chunk;
    for (int i = 0; i < p->nup; ++i) p->up[i] = a->lc_upsample[i];
    const long long frames = (max_steps + hop - 1) / hop;
    p->lc_rows = frames * hop;
    p->oLC = gcarve(cur, 4 * (size_t)B * p->lc_rows * p->Lo);
    long long r = frames;
    for (int i = 0; i + 1 < p->nup; ++i) {   // outputs of the stages before the last
      r *= p->up[i];
      p->oLCACT[i] = gcarve(cur, 4 * (size_t)B * r * p->Lo);
    }
    p->oLCACT[p->nup - 1] = p->oLC;
    p->oLCC = gcarve(cur, 4 * (size_t)p->NC * p->L * B * 64);
    p->up_fused = lbwn_lc_up_fused_ok(p->nup, p->up, p->Li, p->Lo) != 0;
  }
  {   // prefill scratch: independent of the prompt length (a plan's workspace is that of the same
      // arch without LC plus the LC tensors, "pfcond" the last of them)
    p->pfT = pf_slice;
    p->pfH = 1 << (p->nbl - 1);
    for (int i = 0; i < 2; ++i) p->oPFX[i] = gcarve(cur, 4 * (size_t)B * ((size_t)p->pfH + p->pfT) * p->Cr);
    p->oPFZ = gcarve(cur, 4 * (size_t)B * p->pfT * p->Cd);
    p->oPFIMG = gcarve(cur, 4 * (size_t)p->L * lbwn_layer_image_floats());
    if (a->n_gc_embed > 0) {
      p->oPFGC = gcarve(cur, 4 * (size_t)p->L * B * 2 * p->Cd);
      p->oPFIDS = gcarve(cur, 4 * (size_t)B * p->pfT);
    }
    if (p->Lo > 0) {
      p->pfG = pf_group;
      p->oPFCOND = gcarve(cur, 4 * (size_t)B * p->pfT * p->pfG * 2 * p->Cd);
    }
  }
  {   // "sessions": the last 32·B bytes (rounded up to 256) of the workspace.  They lie over the prefill
      // scratch, which no call reads in session mode, so a plan's workspace keeps its size; only a plan
      // whose prefill scratch is smaller than the words (a degenerate slice) grows by the difference
    const size_t sb = (32 * (size_t)B + 255) / 256 * 256;
    if (cur - p->oPFX[0] < sb) gcarve(cur, sb - (cur - p->oPFX[0]));
    p->oSESS = cur - sb;
    p->sess_begun.assign(B, 0);
    p->sess_seen.assign(B, 0);
  }
  p->total = cur;
  *out = p;
  return 0;
}

extern "C" void lbwn_gen_plan_destroy(lbwn_gen_plan* p) { delete p; }
extern "C" size_t lbwn_gen_workspace_bytes(const lbwn_gen_plan* p) { return p ? p->total : 0; }

extern "C" int lbwn_gen_tensor(const lbwn_gen_plan* p, const char* name, size_t* off, size_t* bytes) {
  LBWN_REQUIRE(p && name && off && bytes, "gen_tensor: null argument");
  const size_t B = p->B;
  if (!strcmp(name, "samples")) { *off = p->oSAMP; *bytes = 4 * B * p->max_steps; }
  else if (!strcmp(name, "wav")) { *off = p->oWAV; *bytes = 4 * B * p->max_steps; }
  else if (!strcmp(name, "logits")) { *off = p->oLOG; *bytes = 4 * B * p->Q; }
  else if (!strcmp(name, "step")) { *off = p->oSTEP; *bytes = 8; }
  // 0, or 5: a persistent hand-off timed out, or 6: lbwn_gen_state_load refused its snapshot or map
  else if (!strcmp(name, "status")) { *off = p->oSTEP + 8; *bytes = 4; }
  else if (!strcmp(name, "trace")) { *off = p->oTRACE; *bytes = 8 * (size_t)(2 * p->L + 8 + 128 + 2 * P_NH); }
  else if (!strcmp(name, "rings")) { *off = p->oRING; *bytes = 4 * (size_t)p->n_ring; }
  else if (!strcmp(name, "teacher")) { *off = p->oTEACH; *bytes = 4 * (size_t)std::max<long long>(1, p->n_teacher); }
  else if (p->Lo > 0 && !strcmp(name, "lc")) { *off = p->oLC; *bytes = 4 * B * (size_t)p->lc_rows * p->Lo; }
  else if (p->Lo > 0 && !strcmp(name, "lccond")) { *off = p->oLCC; *bytes = 4 * (size_t)p->NC * p->L * B * 64; }
  else if (!strcmp(name, "sessions")) { *off = p->oSESS; *bytes = 32 * B; }
  else if (p->Lo > 0 && !strcmp(name, "pfcond")) { *off = p->oPFCOND; *bytes = 4 * B * (size_t)p->pfT * p->pfG * 2 * p->Cd; }
  else LBWN_REQUIRE(false, "gen_tensor: unknown tensor '%s'", name);
  return 0;
}

template <typename T>
static T* gat(void* ws, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

extern "C" int lbwn_gen_start(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* gc_ids,
                              const int* teacher, int64_t n_teacher, uint64_t seed, int pre_bias, void* stream) {
  LBWN_REQUIRE(p && P && ws, "gen_start: null argument");
  LBWN_REQUIRE(p->a.n_gc_embed == 0 || gc_ids, "gen_start: GC arch needs gc_ids [B]");
  LBWN_REQUIRE(!teacher || (n_teacher >= 0 && n_teacher <= p->max_teacher),
               "gen_start: teacher length %lld exceeds plan capacity %lld", (long long)n_teacher, p->max_teacher);
  hipStream_t st = (hipStream_t)stream;
  p->n_teacher = teacher ? n_teacher : 0;
  p->mel_loaded = false;
  p->sess_mode = false;
  p->n_begun = 0;
  std::fill(p->sess_begun.begin(), p->sess_begun.end(), 0);
  p->seed = seed;
  p->pre_bias = pre_bias;
  gen_reset_kernel<<<256, 256, 0, st>>>(gat<float>(ws, p->oRING), p->n_ring, gat<unsigned long long>(ws, p->oGRAN),
                                        p->n_gran, gat<int>(ws, p->oCODE), p->B, gat<long long>(ws, p->oSTEP),
                                        gat<int>(ws, p->oSTEP + 8));
  LBWN_CHECK_LAUNCH();
  if (p->n_teacher > 0) {
    hipError_t e = hipMemcpyAsync(gat<int>(ws, p->oTEACH), teacher, 4 * (size_t)p->n_teacher, hipMemcpyDeviceToDevice,
                                  st);
    LBWN_REQUIRE(e == hipSuccess, "gen_start: teacher copy failed: %s", hipGetErrorString(e));
  }
  if (P->skip_b) {
    if (int e = lbwn_sum_bias_launch(P->skip_b, p->L, p->Cs, gat<float>(ws, p->oBSUM), st)) return e;
  }
  gen_pack_kernel<<<p->L, 256, 0, st>>>(P->sig, P->gate, P->sig_b, P->gate_b, P->res, P->res_b, gat<float>(ws, p->oGIMG),
                                        p->Cr, p->Cd);
  LBWN_CHECK_LAUNCH();
  if (p->a.n_gc_embed > 0) {
    gen_gc_proj_kernel<<<p->L, 256, 0, st>>>(P->gc_embed, P->gc_sig, P->gc_gate, gc_ids, gat<float>(ws, p->oGCP),
                                             p->B, p->a.n_gc_embed, p->Cd);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

// the plan's upsample stack over `frames` mel frames [frames][Li] into act[i] (stage i's output; the last
// is the lc rows): the fused launcher inside its envelope, else one GEMM per stage
static int gen_upsample(const lbwn_gen_plan* p, const lbwn_params* P, const float* mel, long long frames,
                        float* const* act, hipStream_t st) {
  if (p->up_fused) return lbwn_lc_up_fwd_launch(p->nup, p->up, p->Li, p->Lo, (int)frames, mel, P->lc_up, act, st);
  // per-stage GEMMs against the [s][O][I] filters read as k-contiguous (engine.cpp cond_forward)
  const float* in = mel;
  long long rows = frames;
  int I = p->Li;
  for (int i = 0; i < p->nup; ++i) {
    const int s = p->up[i];
    lbwn_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = in; g.lda = I; g.B = P->lc_up[i]; g.ldb = I; g.C = act[i]; g.ldc = (long)s * p->Lo;
    g.M = (int)rows; g.N = s * p->Lo; g.K = I;
    if (int e = lbwn_gemm_launch(g, 1, 1, 1, nullptr, st)) return e;
    in = act[i];
    rows *= s;
    I = p->Lo;
  }
  return 0;
}

extern "C" int lbwn_gen_set_mel(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const float* mel, int64_t n_frames,
                                void* stream) {
  LBWN_REQUIRE(p && P && ws, "gen_set_mel: null argument");
  LBWN_REQUIRE(p->Lo > 0, "gen_set_mel: the arch has no local conditioning");
  LBWN_REQUIRE(mel, "gen_set_mel: mel is null");
  LBWN_REQUIRE(n_frames >= 1, "gen_set_mel: n_frames must be >= 1");
  LBWN_REQUIRE(n_frames <= p->lc_rows / p->hop, "gen_set_mel: %lld frames x hop %lld exceed the plan's %lld rows",
               (long long)n_frames, p->hop, p->lc_rows);
  LBWN_REQUIRE(P->lc_sig && P->lc_gate, "gen_set_mel: LC_SIGNAL/LC_GATE pointers are null");
  for (int i = 0; i < p->nup; ++i) LBWN_REQUIRE(P->lc_up[i], "gen_set_mel: LC_UPSAMPLE_%d pointer is null", i);
  LBWN_REQUIRE(!p->sess_mode, "gen_set_mel: the run is in session mode (lbwn_gen_begin since lbwn_gen_start); the "
               "mels come with the sessions");
  hipStream_t st = (hipStream_t)stream;
  const long long frames = (long long)p->B * n_frames;
  LBWN_REQUIRE(frames * p->hop < (1LL << 31), "gen_set_mel: too many rows");
  float* act[8];
  for (int i = 0; i < p->nup; ++i) act[i] = gat<float>(ws, p->oLCACT[i]);
  if (int e = gen_upsample(p, P, mel, frames, act, st)) return e;
  gen_set_word_kernel<<<1, 1, 0, st>>>(gat<int>(ws, p->oSTEP + 12), (int)(n_frames * p->hop));
  LBWN_CHECK_LAUNCH();
  p->mel_loaded = true;
  return 0;
}

extern "C" int lbwn_gen_is_persistent(const lbwn_gen_plan* p) { return p && p->persist ? 1 : 0; }

extern "C" int lbwn_gen_set_sampling(lbwn_gen_plan* p, float temperature, int top_k, float top_p) {
  LBWN_REQUIRE(p, "gen_set_sampling: plan is null");
  LBWN_REQUIRE(std::isfinite(temperature) && temperature > 0.f,
               "gen_set_sampling: temperature must be finite and > 0 (got %g)", (double)temperature);
  LBWN_REQUIRE(top_k >= 0, "gen_set_sampling: top_k must be >= 0 (got %d)", top_k);
  LBWN_REQUIRE(top_p > 0.f && top_p <= 1.f, "gen_set_sampling: top_p must be in (0, 1] (got %g)", (double)top_p);
  p->temperature = temperature;
  p->top_k = top_k >= p->Q ? 0 : top_k;   // every code kept: off
  p->top_p = top_p;
  return 0;
}

extern "C" int lbwn_gen_get_sampling(const lbwn_gen_plan* p, float* temperature, int* top_k, float* top_p) {
  LBWN_REQUIRE(p, "gen_get_sampling: plan is null");
  if (temperature) *temperature = p->temperature;
  if (top_k) *top_k = p->top_k;
  if (top_p) *top_p = p->top_p;
  return 0;
}

static bool gen_filtered(const lbwn_gen_plan* p) { return p->temperature != 1.f || p->top_k != 0 || p->top_p != 1.f; }
static void launch_sample(const lbwn_gen_plan* p, const DrawK& d, const long long* step, hipStream_t st) {
  if (gen_filtered(p)) gen_sample_filt_kernel<<<p->B, 64, 0, st>>>(d, step);
  else gen_sample_kernel<<<p->B, 64, 0, st>>>(d, step);
}

static void launch_wave(const lbwn_gen_plan* p, const WaveK& c, hipStream_t st) {
  if (p->Lo > 0) gen_wave_kernel<true><<<p->B, 512, 0, st>>>(c);
  else gen_wave_kernel<false><<<p->B, 512, 0, st>>>(c);
}

static WaveK wave_args(lbwn_gen_plan* p, const lbwn_params* P, void* ws) {
  WaveK c;
  c.lccond = p->Lo > 0 ? gat<float>(ws, p->oLCC) : nullptr; c.NC = p->NC;
  c.pre = P->pre; c.pre_b = P->pre_b; c.img = gat<float>(ws, p->oGIMG);
  c.gc_proj = p->a.n_gc_embed > 0 ? gat<float>(ws, p->oGCP) : nullptr;
  c.rings = gat<float>(ws, p->oRING); c.zcat = gat<float>(ws, p->oZCAT);
  c.step = gat<long long>(ws, p->oSTEP); c.code = gat<int>(ws, p->oCODE);
  c.trace = nullptr;
  c.B = p->B; c.L = p->L; c.nbl = p->nbl; c.Cr = p->Cr; c.Cd = p->Cd; c.pre_bias = p->pre_bias;
  return c;
}

// Per-step GEMM form (B > P_MAXB): the chain (gen_wave, one workgroup per stream) then the head as
// three bf16-split MFMA GEMMs over all B streams (imodel.py:125-164: skip = Σ_l z_l·SKIP_l + Σb,
// h = relu(relu(skip)·POST1 + b1), logits = h·POST2 + b2) and the sampler.  The K-split vector GEMVs
// re-read every weight per 16-stream group with FMA (B = 256: 211 µs per step).
static int gen_run_gemm(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, DrawK d, hipStream_t st) {
  const WaveK c = wave_args(p, P, ws);
  float* S = gat<float>(ws, p->oSKP);     // [B][Cs]   (the GEMV partial buffers are larger)
  float* H = gat<float>(ws, p->oHP);      // [B][Cp]
  float* LG = gat<float>(ws, p->oLGP);    // [B][Q] logits with b2
  float* SPL = gat<float>(ws, p->oGSPL);
  lbwn_gemm_args sk, p1, p2;
  memset(&sk, 0, sizeof(sk));
  sk.A = c.zcat; sk.lda = (long)p->L * p->Cd; sk.B = P->skip; sk.ldb = p->Cs; sk.C = S; sk.ldc = p->Cs;
  sk.M = p->B; sk.N = p->Cs; sk.K = p->L * p->Cd; sk.bias = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
  sk.step_advance = gat<long long>(ws, p->oSTEP);   // the sampler reads step - 1
  p1 = sk;
  p1.step_advance = nullptr;
  p1.A = S; p1.lda = p->Cs; p1.relu_a = 1; p1.B = P->post1; p1.ldb = p->Cp; p1.C = H; p1.ldc = p->Cp;
  p1.N = p->Cp; p1.K = p->Cs; p1.bias = P->post1_b; p1.relu_out = 1;
  p2 = p1;
  p2.A = H; p2.lda = p->Cp; p2.relu_a = 0; p2.B = P->post2; p2.ldb = p->Q; p2.C = LG; p2.ldc = p->Q;
  p2.N = p->Q; p2.K = p->Cp; p2.bias = P->post2_b; p2.relu_out = 0;
  d.part = LG; d.parts = 1; d.bias = nullptr;   // b2 added by the GEMM
  for (int i = 0; i < n_steps; ++i) {
    launch_wave(p, c, st);
    LBWN_CHECK_LAUNCH();
    if (int e = lbwn_gemm_launch(sk, 1, 0, p->gsplit[0], SPL, st)) return e;
    if (int e = lbwn_gemm_launch(p1, 1, 0, p->gsplit[1], SPL, st)) return e;
    if (int e = lbwn_gemm_launch(p2, 1, 0, p->gsplit[2], SPL, st)) return e;
    launch_sample(p, d, c.step, st);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

// n_steps steps in the plan's form (LC plans: n_steps <= NC, their cond-ring rows projected)
static int gen_run_sub(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, hipStream_t st) {
  DrawK d;
  memset(&d, 0, sizeof(d));
  d.Q = p->Q; d.B = p->B; d.bias = P->post2_b;
  d.logits = gat<float>(ws, p->oLOG); d.samples = gat<int>(ws, p->oSAMP); d.wav = gat<float>(ws, p->oWAV);
  d.max_steps = p->max_steps; d.teacher = gat<int>(ws, p->oTEACH); d.n_teacher = p->n_teacher; d.seed = p->seed;
  d.code = gat<int>(ws, p->oCODE);
  d.temperature = p->temperature; d.top_k = p->top_k; d.top_p = p->top_p;
  d.sess = p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr;
  if (p->persist) {
    if (n_steps == 0) return 0;
    PersistK k;
    memset(&k, 0, sizeof(k));
    k.pre = P->pre; k.pre_b = P->pre_b; k.img = gat<float>(ws, p->oGIMG);
    k.gc_proj = p->a.n_gc_embed > 0 ? gat<float>(ws, p->oGCP) : nullptr;
    k.rings = gat<float>(ws, p->oRING); k.step = gat<long long>(ws, p->oSTEP); k.code_in = gat<int>(ws, p->oCODE);
    k.B = p->B; k.L = p->L; k.nbl = p->nbl; k.Cr = p->Cr; k.Cd = p->Cd; k.pre_bias = p->pre_bias; k.n_steps = n_steps;
    unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
    k.zg = g; k.sg = g + (long)p->B * p->L * 32; k.lg = k.sg + (long)p->B * p->Cs;
    k.Cs = p->Cs; k.Cp = p->Cp; k.Q = p->Q;
    k.skipw = P->skip; k.bsum = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
    k.post1 = P->post1; k.post1_b = P->post1_b; k.post2 = P->post2;
    k.draw = d;
    k.status = gat<int>(ws, p->oSTEP + 8);
    k.trace = p->trace ? gat<long long>(ws, p->oTRACE) : nullptr;
    k.Bg = p->pbg;
    k.gstep = reinterpret_cast<long long*>(g + p->n_gran_core);
    const int nblk = p->pgroups * (p->pbg + P_NH);
    const bool filt = gen_filtered(p);
    if (p->Lo > 0) {
      k.lccond = gat<float>(ws, p->oLCC); k.NC = p->NC;
      if (filt) gen_persist_kernel<true, true><<<nblk, 512, 0, st>>>(k);
      else gen_persist_kernel<true, false><<<nblk, 512, 0, st>>>(k);
    } else {
      if (filt) gen_persist_kernel<false, true><<<nblk, 512, 0, st>>>(k);
      else gen_persist_kernel<false, false><<<nblk, 512, 0, st>>>(k);
    }
    LBWN_CHECK_LAUNCH();
    return 0;
  }
  if (p->oGSPL && !p->trace && lbwn_gemm_mode() == 1) return gen_run_gemm(p, P, ws, n_steps, d, st);
  WaveK c;
  c.pre = P->pre; c.pre_b = P->pre_b; c.img = gat<float>(ws, p->oGIMG);
  c.gc_proj = p->a.n_gc_embed > 0 ? gat<float>(ws, p->oGCP) : nullptr;
  c.rings = gat<float>(ws, p->oRING); c.zcat = gat<float>(ws, p->oZCAT);
  c.step = gat<long long>(ws, p->oSTEP); c.code = gat<int>(ws, p->oCODE);
  c.trace = p->trace ? gat<long long>(ws, p->oTRACE) : nullptr;
  c.B = p->B; c.L = p->L; c.nbl = p->nbl; c.Cr = p->Cr; c.Cd = p->Cd; c.pre_bias = p->pre_bias;
  c.lccond = p->Lo > 0 ? gat<float>(ws, p->oLCC) : nullptr; c.NC = p->NC;
  // skip = z_cat·SKIPcat (+Σb and relu applied by the consumer), h = relu(relu(skip)·POST1 + b1),
  // logits = h·POST2 + b2 (summed in the sampler)
  GemvK sk = {}, p1 = {}, p2 = {};
  memset(&sk, 0, sizeof(sk));
  sk.in = c.zcat; sk.ldin = (long)p->L * p->Cd; sk.W = P->skip; sk.ldw = p->Cs; sk.out_part = gat<float>(ws, p->oSKP);
  sk.B = p->B; sk.K = p->L * p->Cd; sk.N = p->Cs; sk.KSL = p->ksl_skip;
  sk.step_advance = gat<long long>(ws, p->oSTEP);   // the sampler reads step - 1
  p1 = sk;
  p1.step_advance = nullptr;
  p1.in = nullptr; p1.in_part = sk.out_part; p1.in_parts = p->ks_skip; p1.in_bias = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
  p1.relu_in = 1; p1.W = P->post1; p1.ldw = p->Cp; p1.out_part = gat<float>(ws, p->oHP); p1.K = p->Cs; p1.N = p->Cp; p1.KSL = 32;
  p2 = p1;
  p2.in_part = p1.out_part; p2.in_parts = p->ks_h; p2.in_bias = P->post1_b; p2.relu_in = 1;
  p2.W = P->post2; p2.ldw = p->Q; p2.out_part = gat<float>(ws, p->oLGP); p2.K = p->Cp; p2.N = p->Q; p2.KSL = 32;
  d.part = p2.out_part; d.parts = p->ks_lg;
  const dim3 gsk((sk.N + 63) / 64, p->ks_skip), gp1((p1.N + 63) / 64, (p1.K + 31) / 32), gp2((p2.N + 63) / 64, (p2.K + 31) / 32);
  if (p->trace) {   // GEMV stamps after the wave kernel's: [skip | post1 | post2] × 8
    long long* tb = gat<long long>(ws, p->oTRACE) + 2 * p->L + 8;
    sk.trace = tb; p1.trace = tb + 8; p2.trace = tb + 16;
  }
  for (int i = 0; i < n_steps; ++i) {
    launch_wave(p, c, st);
    gen_gemv_kernel<<<gsk, 256, 0, st>>>(sk);
    gen_gemv_kernel<<<gp1, 256, 0, st>>>(p1);
    gen_gemv_kernel<<<gp2, 256, 0, st>>>(p2);
    launch_sample(p, d, c.step, st);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int lbwn_gen_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, void* stream) {
  LBWN_REQUIRE(p && P && ws && n_steps >= 0, "gen_run: bad arguments");
  LBWN_REQUIRE(p->Lo == 0 || p->mel_loaded || p->sess_mode,
               "gen_run: LC plan without a mel (lbwn_gen_set_mel after lbwn_gen_start)");
  LBWN_REQUIRE(p->Lo == 0 || !p->sess_mode || p->n_begun == p->B,
               "gen_run: session mode, but only %d of the %d streams have begun a session (lbwn_gen_begin gives "
               "each its mel)", p->n_begun, p->B);
  hipStream_t st = (hipStream_t)stream;
  if (p->Lo == 0) {
    if (int e = gen_run_sub(p, P, ws, n_steps, st)) return e;
  } else {
    // sub-runs of <= NC steps: project their cond-ring rows (step t -> slot t mod NC), then the steps
    LcProjK k;
    k.lc = gat<float>(ws, p->oLC); k.wsig = P->lc_sig; k.wgate = P->lc_gate; k.out = gat<float>(ws, p->oLCC);
    k.step = gat<long long>(ws, p->oSTEP); k.n_rows = gat<int>(ws, p->oSTEP + 12);
    k.B = p->B; k.L = p->L; k.Lo = p->Lo; k.Cd = p->Cd; k.NC = p->NC;
    k.sess = p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr; k.lc_stride = (long)p->lc_rows;
    for (int done = 0; done < n_steps; done += p->NC) {
      k.n = std::min(p->NC, n_steps - done);
      const dim3 grid(p->L, (k.n * p->B + LCP_ROWS - 1) / LCP_ROWS);
      if (p->sess_mode) gen_lc_proj_kernel<true><<<grid, 256, 0, st>>>(k);
      else gen_lc_proj_kernel<false><<<grid, 256, 0, st>>>(k);
      LBWN_CHECK_LAUNCH();
      if (int e = gen_run_sub(p, P, ws, k.n, st)) return e;
    }
  }
  if (p->persist && n_steps > 0) {   // the persistent form's wav: decode the call's samples [step - n_steps, step)
    gen_decode_kernel<<<std::max(1, std::min(1024, (int)(((long long)p->B * n_steps + 255) / 256))), 256, 0, st>>>(
        gat<int>(ws, p->oSAMP), gat<float>(ws, p->oWAV), gat<long long>(ws, p->oSTEP), p->B, p->max_steps, n_steps,
        p->Q);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

// ---- sessions: restart single streams between two runs -------------------------------------------
extern "C" int lbwn_gen_begin(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const lbwn_gen_session* s, int n,
                              size_t struct_size, void* stream) {
  LBWN_REQUIRE(p, "gen_begin: plan is null");
  LBWN_REQUIRE(P, "gen_begin: params is null");
  LBWN_REQUIRE(ws, "gen_begin: workspace is null");
  LBWN_REQUIRE(s, "gen_begin: s (the session array) is null");
  LBWN_REQUIRE(struct_size == sizeof(lbwn_gen_session), "gen_begin: struct_size %zu != %zu", struct_size,
               sizeof(lbwn_gen_session));
  LBWN_REQUIRE(n >= 1 && n <= p->B, "gen_begin: n = %d sessions must be in 1..batch_sz = %d", n, p->B);
  LBWN_REQUIRE(p->n_teacher == 0, "gen_begin: lbwn_gen_start loaded a teacher of n_teacher = %lld codes; the teacher "
               "override is keyed by the absolute step and sessions do not take it", p->n_teacher);
  LBWN_REQUIRE(!(p->mel_loaded && !p->sess_mode), "gen_begin: lbwn_gen_set_mel loaded a dense mel since "
               "lbwn_gen_start; the two modes are exclusive");
  const bool gc = p->a.n_gc_embed > 0, lc = p->Lo > 0;
  if (lc) {
    LBWN_REQUIRE(P->lc_sig && P->lc_gate, "gen_begin: LC_SIGNAL/LC_GATE pointers are null");
    for (int i = 0; i < p->nup; ++i) LBWN_REQUIRE(P->lc_up[i], "gen_begin: LC_UPSAMPLE_%d pointer is null", i);
  }
  if (gc) LBWN_REQUIRE(P->gc_embed && P->gc_sig && P->gc_gate, "gen_begin: GC_EMBED/GC_SIGNAL/GC_GATE pointers are null");
  const long long max_frames = lc ? p->lc_rows / p->hop : 0;
  std::vector<unsigned char>& seen = p->sess_seen;   // sized at plan creation: no allocation here
  std::fill(seen.begin(), seen.end(), 0);
  for (int i = 0; i < n; ++i) {
    LBWN_REQUIRE(s[i].slot >= 0 && s[i].slot < p->B, "gen_begin: s[%d].slot = %d is outside [0, batch_sz = %d)", i,
                 s[i].slot, p->B);
    LBWN_REQUIRE(!seen[s[i].slot], "gen_begin: s[%d].slot = %d is listed twice", i, s[i].slot);
    seen[s[i].slot] = 1;
    LBWN_REQUIRE(s[i].key >= 0 && s[i].key < (1LL << 31), "gen_begin: s[%d].key = %lld is outside [0, 2^31)", i,
                 (long long)s[i].key);
    LBWN_REQUIRE(!gc || (s[i].gc_id >= 0 && s[i].gc_id <= p->a.n_gc_category),
                 "gen_begin: s[%d].gc_id = %d is outside [0, n_gc_category = %d]", i, s[i].gc_id, p->a.n_gc_category);
    if (lc) {
      LBWN_REQUIRE(s[i].mel, "gen_begin: s[%d].mel is null on an LC arch", i);
      LBWN_REQUIRE((((uintptr_t)s[i].mel) & 15) == 0, "gen_begin: s[%d].mel %p is not 16-byte aligned", i,
                   (const void*)s[i].mel);
      LBWN_REQUIRE(s[i].n_frames >= 1 && s[i].n_frames <= max_frames,
                   "gen_begin: s[%d].n_frames = %lld must be in 1..%lld (x hop %lld within the plan's %lld rows)", i,
                   (long long)s[i].n_frames, max_frames, p->hop, p->lc_rows);
    } else {
      LBWN_REQUIRE(!s[i].mel, "gen_begin: s[%d].mel is given, but the arch has no local conditioning", i);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += GB_MAX) {
    BeginK k;
    memset(&k, 0, sizeof(k));
    k.rings = gat<float>(ws, p->oRING); k.code = gat<int>(ws, p->oCODE); k.step = gat<long long>(ws, p->oSTEP);
    k.sess = gat<long long>(ws, p->oSESS);
    if (gc) { k.emb = P->gc_embed; k.gsig = P->gc_sig; k.ggate = P->gc_gate; k.gcp = gat<float>(ws, p->oGCP); }
    k.B = p->B; k.L = p->L; k.nbl = p->nbl; k.Cr = p->Cr; k.Ge = p->a.n_gc_embed; k.Cd = p->Cd;
    k.n = std::min(GB_MAX, n - i0);
    k.init_all = !p->sess_mode && i0 == 0;
    for (int i = 0; i < k.n; ++i) {
      const lbwn_gen_session& e = s[i0 + i];
      k.slot[i] = e.slot; k.gc_id[i] = gc ? e.gc_id : 0; k.key[i] = (int)e.key;
      k.rows[i] = lc ? (int)(e.n_frames * p->hop) : 0;
    }
    gen_begin_kernel<<<dim3(p->L, k.n), 256, 0, st>>>(k);
    LBWN_CHECK_LAUNCH();
  }
  p->sess_mode = true;
  for (int i = 0; i < n; ++i) {
    if (!p->sess_begun[s[i].slot]) { p->sess_begun[s[i].slot] = 1; ++p->n_begun; }
  }
  if (lc) {
    const long long max_fr = p->lc_rows / p->hop;
    for (int i = 0; i < n; ++i) {   // the stream's own region of "lc" and of the stages' scratch
      float* act[8];
      long long r = max_fr;
      for (int j = 0; j + 1 < p->nup; ++j) {
        r *= p->up[j];
        act[j] = gat<float>(ws, p->oLCACT[j]) + (size_t)s[i].slot * r * p->Lo;
      }
      act[p->nup - 1] = gat<float>(ws, p->oLC) + (size_t)s[i].slot * p->lc_rows * p->Lo;
      if (int e = gen_upsample(p, P, s[i].mel, s[i].n_frames, act, st)) return e;
    }
  }
  return 0;
}

// ---- parallel prompt prefill ----------------------------------------------------------------
// the refusals lbwn_gen_prefill and lbwn_gen_score share (what: the call's name in the message)
static int prefill_check(const char* what, const lbwn_gen_plan* p, const lbwn_params* P, const void* ws,
                         const int* codes, int64_t ld_codes, int64_t n) {
  LBWN_REQUIRE(p && P && ws && codes, "%s: null argument", what);
  LBWN_REQUIRE(n >= 1, "%s: n must be >= 1 (got %lld)", what, (long long)n);
  LBWN_REQUIRE(ld_codes == 0 || ld_codes >= n, "%s: ld_codes %lld must be 0 (one shared vector) or >= n = %lld", what,
               (long long)ld_codes, (long long)n);
  LBWN_REQUIRE(!p->sess_mode, "%s: not supported in session mode (lbwn_gen_begin since lbwn_gen_start): it is a "
               "whole-batch operation", what);
  LBWN_REQUIRE(p->Lo == 0 || p->mel_loaded,
               "%s: local conditioning is not supported before lbwn_gen_set_mel (no mel loaded)", what);
  LBWN_REQUIRE(p->Lo == 0 || (P->lc_sig && P->lc_gate), "%s: LC_SIGNAL/LC_GATE pointers are null", what);
  LBWN_REQUIRE((long long)p->B * p->pfT * p->Cr < (1LL << 31), "%s: batch_sz %d x slice %d x n_res %d >= 2^31", what,
               p->B, p->pfT, p->Cr);
  return 0;
}

// lbwn_gen_score's part of a prefill: the caller's logp and the scratch [Zcat | S | H | LG]
struct ScoreRun {
  float* logp; long ld_logp;
  float *zcat, *S, *H, *LG;
};

// sc == nullptr: the prefill, launch for launch.  Otherwise every layer's z goes to its column block of
// Zcat [B·T][L·Cd] instead of the per-layer scratch, and each slice ends with the head over its rows
// (skip as ONE GEMM with K = L·Cd, post1, post2: gen_run_gemm's three products) and gen_score_logp_kernel.
static int gen_prefill_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                           int64_t n, const ScoreRun* sc, hipStream_t st) {
  const int B = p->B, L = p->L, H = p->pfH, Cr = p->Cr, Cd = p->Cd;
  float* X[2] = {gat<float>(ws, p->oPFX[0]), gat<float>(ws, p->oPFX[1])};
  float* Z = gat<float>(ws, p->oPFZ);
  float* img = gat<float>(ws, p->oPFIMG);
  float* rings = gat<float>(ws, p->oRING);
  long long* step = gat<long long>(ws, p->oSTEP);
  int* code = gat<int>(ws, p->oCODE);
  const bool gc = p->a.n_gc_embed > 0;
  float* gtab = gc ? gat<float>(ws, p->oPFGC) : nullptr;
  int* ids = gc ? gat<int>(ws, p->oPFIDS) : nullptr;
  const bool bias = p->pre_bias && P->pre_b;
  float* pfcond = p->Lo > 0 ? gat<float>(ws, p->oPFCOND) : nullptr;
  const long ldcond = (long)p->pfG * 2 * Cd;
  // float4 rows: the buffers and rings are 256-B carved and every ring offset is a multiple of Cr
  const bool xv4 = Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  const bool ev4 = xv4 && (((uintptr_t)P->pre) & 15) == 0 && (!bias || (((uintptr_t)P->pre_b) & 15) == 0);
  auto grid = [](long items) { return (int)std::max(1L, std::min(2048L, (items + 255) / 256)); };
  if (int e = lbwn_pack_layers_launch(P->sig, P->gate, P->sig_b, P->gate_b, P->res, P->res_b, img, L, Cr, Cd, st))
    return e;
  if (gc) {
    gen_prefill_gctab_kernel<<<grid((long)L * B * 2 * Cd), 256, 0, st>>>(gat<float>(ws, p->oGCP), gtab, (long)L * B, Cd);
    LBWN_CHECK_LAUNCH();
  }
  const int WI = lbwn_layer_image_floats();
  for (int64_t off = 0; off < n; off += p->pfT) {
    const int T = (int)std::min<int64_t>(p->pfT, n - off);
    PrefillE e;
    e.pre = P->pre; e.pre_b = P->pre_b; e.codes = codes; e.code = code; e.x = X[0]; e.ids = ids;
    e.ld_codes = (long)ld_codes; e.off = (long)off;
    e.B = B; e.T = T; e.H = H; e.Cr = Cr; e.Q = p->Q; e.bias = bias ? 1 : 0;
    if (ev4) gen_prefill_embed_kernel<true><<<grid((long)B * T * (Cr / 4)), 256, 0, st>>>(e);
    else gen_prefill_embed_kernel<false><<<grid((long)B * T * Cr), 256, 0, st>>>(e);
    LBWN_CHECK_LAUNCH();
    long roff = 0;   // ring offset of layer l
    for (int l = -1; l < L; ++l) {
      // launch l: the ring write of layer l and the halo of layer l + 1 (whose buffer layer l - 1 has read)
      PrefillX x;
      memset(&x, 0, sizeof(x));
      x.step = step; x.off = (long)off; x.B = B; x.T = T; x.H = H; x.Cr = Cr;
      long items = 0;
      if (l >= 0) {
        x.dw = 1 << (l % p->nbl);
        x.src = X[l & 1]; x.ring_w = rings + roff;
        items += (long)B * std::min(x.dw, T);
        roff += (long)x.dw * B * Cr;
      }
      if (l + 1 < L) {
        x.dr = 1 << ((l + 1) % p->nbl);
        x.ring_r = rings + roff; x.dst = X[(l + 1) & 1];
        items += (long)B * x.dr;
      }
      if (xv4) gen_prefill_xfer_kernel<true><<<grid(items * (Cr / 4)), 256, 0, st>>>(x);
      else gen_prefill_xfer_kernel<false><<<grid(items * Cr), 256, 0, st>>>(x);
      LBWN_CHECK_LAUNCH();
      if (l < 0) continue;
      if (p->Lo > 0 && l % p->pfG == 0) {   // the LC terms of layers l .. l + G - 1 for this slice
        PrefillLC c;
        c.lc = gat<float>(ws, p->oLC); c.wsig = P->lc_sig; c.wgate = P->lc_gate; c.out = pfcond;
        c.step = step; c.n_rows = gat<int>(ws, p->oSTEP + 12);
        c.off = (long)off; c.ld = ldcond;
        c.B = B; c.T = T; c.Lo = p->Lo; c.Cd = Cd; c.l0 = l; c.G = std::min(p->pfG, L - l);
        c.v4 = Cd % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
        gen_prefill_lcproj_kernel<<<(unsigned)(((long)B * T + PLC_POS - 1) / PLC_POS), PLC_THREADS, 0, st>>>(c);
        LBWN_CHECK_LAUNCH();
      }
      lbwn_layer_args a;
      memset(&a, 0, sizeof(a));
      a.x_in = X[l & 1]; a.x_out = l + 1 < L ? X[(l + 1) & 1] : nullptr;   // the last layer's output is not needed
      if (sc) { a.z = sc->zcat + (long)l * Cd; a.ldz = (long)L * Cd; }
      else { a.z = Z; a.ldz = Cd; }
      a.wpack = img + (long)l * WI;
      if (gc) { a.gc_tab = gtab + (long)l * B * 2 * Cd; a.gc_ld = 2L * Cd; a.ids = ids; }
      if (p->Lo > 0) { a.cond = pfcond + (long)(l % p->pfG) * 2 * Cd; a.ldcond = ldcond; }   // GC and LC add, as in training
      a.B = B; a.T = T; a.H = H; a.d = x.dw; a.Cr = Cr; a.Cd = Cd;
      if (int e2 = lbwn_layer_fwd_launch(a, st)) return e2;
    }
    if (sc) {
      lbwn_gemm_args sk, p1, p2;
      memset(&sk, 0, sizeof(sk));
      sk.A = sc->zcat; sk.lda = (long)L * Cd; sk.B = P->skip; sk.ldb = p->Cs; sk.C = sc->S; sk.ldc = p->Cs;
      sk.M = B * T; sk.N = p->Cs; sk.K = L * Cd; sk.bias = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
      p1 = sk;
      p1.A = sc->S; p1.lda = p->Cs; p1.relu_a = 1; p1.B = P->post1; p1.ldb = p->Cp; p1.C = sc->H; p1.ldc = p->Cp;
      p1.N = p->Cp; p1.K = p->Cs; p1.bias = P->post1_b; p1.relu_out = 1;
      p2 = p1;
      p2.A = sc->H; p2.lda = p->Cp; p2.relu_a = 0; p2.B = P->post2; p2.ldb = p->Q; p2.C = sc->LG; p2.ldc = p->Q;
      p2.N = p->Q; p2.K = p->Cp; p2.bias = P->post2_b; p2.relu_out = 0;
      if (int e2 = lbwn_gemm_launch(sk, 1, 0, 1, nullptr, st)) return e2;
      if (int e2 = lbwn_gemm_launch(p1, 1, 0, 1, nullptr, st)) return e2;
      if (int e2 = lbwn_gemm_launch(p2, 1, 0, 1, nullptr, st)) return e2;
      ScoreK k;
      k.lg = sc->LG; k.codes = codes; k.logp = sc->logp;
      k.last = off + T == n ? gat<float>(ws, p->oLOG) : nullptr;
      k.ld_codes = (long)ld_codes; k.ld_logp = sc->ld_logp; k.off = (long)off;
      k.B = B; k.T = T; k.Q = p->Q;
      gen_score_logp_kernel<<<(unsigned)(((long)B * T + SC_ROWS - 1) / SC_ROWS), 64 * SC_ROWS, 0, st>>>(k);
      LBWN_CHECK_LAUNCH();
    }
  }
  gen_prefill_out_kernel<<<grid((long)B * n), 256, 0, st>>>(codes, (long)ld_codes, (long)n, step, gat<int>(ws, p->oSAMP),
                                                          gat<float>(ws, p->oWAV), p->max_steps, B, p->Q);
  LBWN_CHECK_LAUNCH();
  // last: a call that failed above leaves the counters where the rings' owners expect them
  unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
  gen_prefill_finish_kernel<<<1, 256, 0, st>>>(codes, (long)ld_codes, (long)n, code, step,
                                               reinterpret_cast<long long*>(g + p->n_gran_core), p->pgroups, B, p->Q);
  LBWN_CHECK_LAUNCH();
  return 0;
}

extern "C" int lbwn_gen_prefill(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                                int64_t n, void* stream) {
  if (int e = prefill_check("prefill", p, P, ws, codes, ld_codes, n)) return e;
  return gen_prefill_run(p, P, ws, codes, ld_codes, n, nullptr, (hipStream_t)stream);
}

// ---- teacher-forced scoring -------------------------------------------------------------------
// the scratch of lbwn_gen_score: Zcat [R][L·Cd] | S [R][Cs] | H [R][Cp] | LG [R][Q], R = B·T_s rows, each
// part rounded up to 256 bytes
static void score_carve(const lbwn_gen_plan* p, size_t (&off)[4], size_t& total) {
  const size_t rows = (size_t)p->B * p->pfT;
  const size_t cols[4] = {(size_t)p->L * p->Cd, (size_t)p->Cs, (size_t)p->Cp, (size_t)p->Q};
  size_t cur = 0;
  for (int i = 0; i < 4; ++i) off[i] = gcarve(cur, 4 * rows * cols[i]);
  total = cur;
}

extern "C" size_t lbwn_gen_score_scratch_bytes(const lbwn_gen_plan* p) {
  if (!p) return 0;
  size_t off[4], total;
  score_carve(p, off, total);
  return total;
}

extern "C" int lbwn_gen_score(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                              int64_t n, float* logp, int64_t ld_logp, void* scratch, void* stream) {
  if (int e = prefill_check("score", p, P, ws, codes, ld_codes, n)) return e;
  LBWN_REQUIRE(logp, "score: logp is null");
  LBWN_REQUIRE(scratch, "score: scratch is null");
  LBWN_REQUIRE((((uintptr_t)scratch) & 15) == 0, "score: scratch %p is not 16-byte aligned", scratch);
  LBWN_REQUIRE(ld_logp >= n, "score: ld_logp %lld must be >= n = %lld", (long long)ld_logp, (long long)n);
  // what the head GEMMs and the float4 rows of the log-softmax take
  LBWN_REQUIRE(p->Cs % 4 == 0 && p->Cp % 4 == 0 && p->Q % 4 == 0 && (p->L * p->Cd) % 4 == 0,
               "score: n_skip %d, n_post %d, n_quant %d and layers x n_dil %d must be multiples of 4", p->Cs, p->Cp,
               p->Q, p->L * p->Cd);
  const long long widest = std::max(std::max((long long)p->L * p->Cd, (long long)p->Cs),
                                    std::max((long long)p->Cp, (long long)p->Q));
  LBWN_REQUIRE((long long)p->B * p->pfT * widest < (1LL << 31), "score: batch_sz %d x slice %d x %lld columns >= 2^31",
               p->B, p->pfT, widest);
  LBWN_REQUIRE(P->skip && P->post1 && P->post2, "score: SKIP/POST1/POST2 pointers are null");
  LBWN_REQUIRE(((((uintptr_t)P->skip) | ((uintptr_t)P->post1) | ((uintptr_t)P->post2) | ((uintptr_t)ws)) & 15) == 0,
               "score: SKIP/POST1/POST2 and the workspace must be 16-byte aligned");
  size_t off[4], total;
  score_carve(p, off, total);
  ScoreRun sc;
  sc.logp = logp; sc.ld_logp = (long)ld_logp;
  sc.zcat = gat<float>(scratch, off[0]); sc.S = gat<float>(scratch, off[1]);
  sc.H = gat<float>(scratch, off[2]); sc.LG = gat<float>(scratch, off[3]);
  return gen_prefill_run(p, P, ws, codes, ld_codes, n, &sc, (hipStream_t)stream);
}

// ---- state snapshot ---------------------------------------------------------------------------
static size_t state_record_bytes(const lbwn_gen_plan* p) {
  const size_t rows = (size_t)p->a.n_blocks * (((size_t)1 << p->nbl) - 1);
  return (GS_CODE + 4 * rows * p->Cr + 15) / 16 * 16;
}

extern "C" size_t lbwn_gen_state_bytes(const lbwn_gen_plan* p, int n_streams) {
  return p && n_streams >= 1 ? GS_HEADER + (size_t)n_streams * state_record_bytes(p) : 0;
}

static StateK state_args(const lbwn_gen_plan* p, void* ws, void* state) {
  StateK k;
  memset(&k, 0, sizeof(k));
  unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
  k.rings = gat<float>(ws, p->oRING); k.code = gat<int>(ws, p->oCODE); k.step = gat<long long>(ws, p->oSTEP);
  k.gstep = reinterpret_cast<long long*>(g + p->n_gran_core); k.status = gat<int>(ws, p->oSTEP + 8);
  k.gran = g; k.n_gran = p->n_gran_core;
  k.state = static_cast<char*>(state);
  k.max_steps = p->max_steps;
  k.B = p->B; k.nb = p->a.n_blocks; k.nbl = p->nbl; k.Cr = p->Cr; k.Q = p->Q;
  k.rec_bytes = (int)state_record_bytes(p); k.state_streams = p->B; k.ngroups = p->pgroups;
  return k;
}

// a grid sized to the CUs (8 blocks of 4 waves each), or to the items when those are fewer
static int state_grid(const lbwn_gen_plan* p, bool v4) {
  const long items = p->n_ring / (v4 ? 4 : 1);
  const long want = (items + 256L * GS_UNROLL - 1) / (256L * GS_UNROLL);
  return (int)std::max(1L, std::min(want, 8L * (p->ncu > 0 ? p->ncu : 256)));
}

extern "C" int lbwn_gen_state_save(const lbwn_gen_plan* p, const void* ws, void* state, void* stream) {
  LBWN_REQUIRE(p, "gen_state_save: plan is null");
  LBWN_REQUIRE(ws, "gen_state_save: workspace is null");
  LBWN_REQUIRE(state, "gen_state_save: state is null");
  LBWN_REQUIRE((((uintptr_t)state) & 15) == 0, "gen_state_save: state %p is not 16-byte aligned", state);
  hipStream_t st = (hipStream_t)stream;
  const StateK k = state_args(p, const_cast<void*>(ws), state);
  const bool v4 = p->Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  if (v4) gen_state_copy_kernel<true, false><<<state_grid(p, true), 256, 0, st>>>(k);
  else gen_state_copy_kernel<false, false><<<state_grid(p, false), 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

extern "C" int lbwn_gen_state_load(lbwn_gen_plan* p, void* ws, const void* state, int state_streams,
                                   const int* src_stream, void* stream) {
  LBWN_REQUIRE(p, "gen_state_load: plan is null");
  LBWN_REQUIRE(ws, "gen_state_load: workspace is null");
  LBWN_REQUIRE(state, "gen_state_load: state is null");
  LBWN_REQUIRE(state_streams >= 1, "gen_state_load: state_streams must be >= 1 (got %d)", state_streams);
  LBWN_REQUIRE(src_stream || state_streams == p->B,
               "gen_state_load: src_stream is null (identity) but state_streams %d != batch_sz %d", state_streams, p->B);
  LBWN_REQUIRE((((uintptr_t)state) & 15) == 0, "gen_state_load: state %p is not 16-byte aligned", state);
  hipStream_t st = (hipStream_t)stream;
  StateK k = state_args(p, ws, const_cast<void*>(state));   // LOAD only reads it
  k.state_streams = state_streams;
  k.map = src_stream;
  const bool v4 = p->Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  if (v4) gen_state_copy_kernel<true, true><<<state_grid(p, true), 256, 0, st>>>(k);
  else gen_state_copy_kernel<false, true><<<state_grid(p, false), 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}
