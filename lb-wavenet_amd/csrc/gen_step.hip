// The generator's per-step form (any B): gen_wave (one workgroup per stream: PRE row (+bias), 50 ×
// [dilated conv, gate, residual] while four loader waves stream the per-layer weight images into an
// LDS ring by LDS-DMA), gen_gemv × 3 (K-split row-vector products with deterministic partial sums:
// skip = z_cat·SKIPcat, h = relu(relu(skip + Σb)·POST1 + b1), logits = h·POST2) and gen_sample
// (Σ partials + b2, the draw).  Sessions, snapshots and the prefill: nothing here knows of them.
#include "gen_draw.h"

namespace {

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
struct WaveK {
  const float* pre; const float* pre_b; const float* img; const float* gc_proj;
  float* rings; float* zcat; const long long* step; const int* code;
  int B, L, nbl, Cr, Cd, pre_bias;
  long long* trace;   // non-null (LBWN_GEN_TRACE set at plan creation): stream 0's cycle stamps
  const float* lccond; int NC;   // LC plans: the cond ring [NC][L][B][64] (gen_lc_proj_kernel)
};

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
    v += dpp_f<DPP_XOR1>(v);
    v += dpp_f<DPP_XOR2>(v);
    v += bco;                                      // conv output o (+ bias + GC term)
    const float vp = dpp_f<DPP_HALF_MIRROR>(v);      // the partner output (sig <-> gate, same channel)
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

// Ring plans only (as in the persistent form): a stopped run (the status word, 8 bytes behind the step counter,
// is nonzero since lbwn_gen_start: 7 from lbwn_gen_extend / lbwn_gen_collect) takes no step: the sampler, the last launch of a step, draws nothing and block 0 takes back the step's count (the
// chain has moved the rings, which only lbwn_gen_start brings back, as it clears the status).  No block of
// this launch reads the counter after that.
LBWN_DEV bool sample_stopped(const long long* step) {
  if (reinterpret_cast<const int*>(step)[2] == 0) return false;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_fetch_add(const_cast<long long*>(step), -1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// the per-step path's sampler: one wave per stream; the step counter was advanced by this
// step's skip GEMV, so this step is *step - 1
__global__ __launch_bounds__(64) void gen_sample_kernel(DrawK a, const long long* step) {
  if (a.ring && sample_stopped(step)) return;
  const long long t = *step - 1;
  if (a.Q > 256) draw_wave<8>(a, blockIdx.x, t, true);
  else draw_wave<4>(a, blockIdx.x, t, true);
}
// the same with the filtered draw (a second kernel, so the default sampler's code is untouched)
__global__ __launch_bounds__(64) void gen_sample_filt_kernel(DrawK a, const long long* step) {
  if (a.ring && sample_stopped(step)) return;
  const long long t = *step - 1;
  if (a.Q > 256) draw_wave<8, true>(a, blockIdx.x, t, true);
  else draw_wave<4, true>(a, blockIdx.x, t, true);
}

}  // namespace

static void launch_sample(const lbwn_gen_plan* p, const DrawK& d, const long long* step, hipStream_t st) {
  (gen_filtered(p) ? gen_sample_filt_kernel : gen_sample_kernel)<<<p->B, 64, 0, st>>>(d, step);
}
static void launch_wave(const lbwn_gen_plan* p, const WaveK& c, hipStream_t st) {
  (p->Lo > 0 ? gen_wave_kernel<true> : gen_wave_kernel<false>)<<<p->B, 512, 0, st>>>(c);
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
  float* LG = gat<float>(ws, p->oLGP);    // [B][Q] logits with b2; S [B][Cs] and H [B][Cp] likewise
  float* SPL = gat<float>(ws, p->oGSPL);  // (the GEMV partial buffers are larger)
  lbwn_gemm_args g[3];
  gen_head_gemms(p, P, ws, c.zcat, p->B, gat<float>(ws, p->oSKP), gat<float>(ws, p->oHP), LG, g);
  g[0].step_advance = gat<long long>(ws, p->oSTEP);   // the sampler reads step - 1
  d.part = LG; d.parts = 1; d.bias = nullptr;   // b2 added by the GEMM
  for (int i = 0; i < n_steps; ++i) {
    launch_wave(p, c, st);
    LBWN_CHECK_LAUNCH();
    for (int j = 0; j < 3; ++j)
      if (int e = lbwn_gemm_launch(g[j], 1, 0, p->gsplit[j], SPL, st)) return e;
    launch_sample(p, d, c.step, st);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

// n_steps steps in the per-step form (LC plans: n_steps <= NC, their cond-ring rows projected)
int lbwn_gen_step_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, hipStream_t st) {
  DrawK d = draw_args(p, P, ws);
  if (p->oGSPL && !p->trace && lbwn_gemm_mode() == 1) return gen_run_gemm(p, P, ws, n_steps, d, st);
  WaveK c = wave_args(p, P, ws);
  c.trace = p->trace ? gat<long long>(ws, p->oTRACE) : nullptr;
  // skip = z_cat·SKIPcat (+Σb and relu applied by the consumer), h = relu(relu(skip)·POST1 + b1),
  // logits = h·POST2 + b2 (summed in the sampler)
  GemvK sk, p1, p2;
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
