// Global / local conditioning (tmodel.py:68-83, :92-114, :150-160).
//
// GC: the per-layer term GC_EMBED[ids]·GC_k_l depends on the position only through its
// voice id, so it is a lookup in a per-step table GCTAB[c][l][sig Cd | gate Cd] =
// GC_EMBED[c]·[GC_SIGNAL_l | GC_GATE_l]; the layer kernels add row ids[m].  Backward: the
// layer kernels scatter-add dv rows into GCD[c][l][2Cd] (per voice id), and
//   dGC_SIGNAL_l = GC_EMBEDᵀ·GCD_l[:, :Cd],  dGC_EMBED = Σ_l GCD_l·[GC_SIGNAL_l | GC_GATE_l]ᵀ.
// LC: the per-layer projections LC_SIGNAL_l / LC_GATE_l are packed side by side into one
// [Clc][L·2Cd] matrix so the whole conditioning input is ONE GEMM lc·LCcat (engine.cpp).
#include <string.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

// Tables are [ncat+1][L·2Cd]: row c holds every layer's (sig Cd | gate Cd) block, n = l·2Cd + s·Cd + o.
LBWN_DEV const float* gc_w(const float* wsig, const float* wgate, int n, int e, int Ge, int Cd) {
  const int l = n / (2 * Cd), s = (n / Cd) & 1, o = n % Cd;
  return (s == 0 ? wsig : wgate) + ((long)l * Ge + e) * Cd + o;
}

// out[c][n] = Σ_e emb[c][e] · W(n)[e]
__global__ void gc_table_kernel(const float* __restrict__ emb, const float* __restrict__ wsig,
                                const float* __restrict__ wgate, float* __restrict__ out, int N, int ncat1, int Ge,
                                int Cd) {
  const long total = (long)ncat1 * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i % N), c = (int)(i / N);
    const float* e = emb + (long)c * Ge;
    float acc = 0.f;
    for (int k = 0; k < Ge; ++k) acc += e[k] * *gc_w(wsig, wgate, n, k, Ge, Cd);
    out[i] = acc;
  }
}

constexpr int GC_CSPLIT = 16;   // category chunks of the weight-gradient pass
constexpr int GC_EMAX = 32;     // n_gc_embed supported by the gradient kernels

// dW(n)[e] = Σ_c emb[c][e] · gcd[c][n], one thread per (e, n), the categories in order
// (deterministic).  At most 32 VGPRs (scalar index math, batches of 8 loads): it runs on the side
// stream beside dSKIP's A-in-registers GEMM blocks (2 waves of 240 VGPRs per SIMD leave 32), so it
// must fit in what they leave free or it waits for them (round 5: 164 us at C4 as a 32-accumulator
// split-C kernel whose blocks could not start beside dSKIP).
__global__ __launch_bounds__(256) void gc_wgrad_kernel(const float* __restrict__ emb, const float* __restrict__ gcd,
                                                       float* __restrict__ dsig, float* __restrict__ dgate, int N,
                                                       int ncat1, int Ge, int Cd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Ge * N) return;
  const int e = i / N, n = i - e * N;
  float acc = 0.f;
  int c = 0;
  for (; c + 8 <= ncat1; c += 8) {
    float g[8], w[8];
    const float* gp = gcd + c * N + n;
    const float* wp = emb + c * Ge + e;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] = gp[j * N];
      w[j] = wp[j * Ge];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += w[j] * g[j];
  }
  for (; c < ncat1; ++c) acc += emb[c * Ge + e] * gcd[c * N + n];
  *const_cast<float*>(gc_w(dsig, dgate, n, e, Ge, Cd)) = acc;
}

// dEMB[c][e] = Σ_n gcd[c][n] · W(n)[e] as a small tiled product: block (category group cg, n chunk
// k) stages gcd[cg·CPB .. +CPB][k·256 .. +256] and W(n)[0..Ge) for its 256 n into LDS with all
// loads issued at once, then thread (category cl, column e) sums its 256 products; the chunk
// partials part[k][c][e] are summed in chunk order by gc_egrad_sum_kernel (deterministic).
// (One block per category looping over n ran 114-308 µs: dependent load chains behind integer
// divisions; this form is one wave of ~300 blocks.)
constexpr int GE_N = 256;
__global__ __launch_bounds__(256) void gc_egrad_part_kernel(const float* __restrict__ gcd,
                                                            const float* __restrict__ wsig,
                                                            const float* __restrict__ wgate,
                                                            float* __restrict__ part, int N, int ncat1, int Ge,
                                                            int Cd) {
  __shared__ float gs[16][GE_N + 1];
  __shared__ float wsm[GE_N][GC_EMAX + 1];
  const int ep = Ge <= 16 ? 16 : 32, cpb = 256 / ep;
  const int cg = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  const int n = k * GE_N + t, nc = min(n, N - 1);
  {   // batches of 4 loads: at most 32 VGPRs (it runs on the side stream beside dSKIP, as gc_wgrad_kernel)
    const int l = nc / (2 * Cd), s = (nc / Cd) & 1, o = nc % Cd;
    const float* W = (s == 0 ? wsig : wgate) + l * Ge * Cd + o;
    const bool in = n < N;
#pragma unroll 1
    for (int e0 = 0; e0 < GC_EMAX; e0 += 4) {
      float wv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = W[min(e0 + j, Ge - 1) * Cd];
#pragma unroll
      for (int j = 0; j < 4; ++j) wsm[t][e0 + j] = in ? wv[j] : 0.f;
    }
#pragma unroll 1
    for (int c0 = 0; c0 < 16; c0 += 4) {
      float gv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = gcd[min(cg * cpb + min(c0 + j, cpb - 1), ncat1 - 1) * N + nc];
#pragma unroll
      for (int j = 0; j < 4; ++j) gs[c0 + j][t] = in ? gv[j] : 0.f;
    }
  }
  __syncthreads();
  const int cl = t / ep, e = t % ep, c = cg * cpb + cl;
  float acc = 0.f;
#pragma unroll 4
  for (int j = 0; j < GE_N; ++j) acc += gs[cl][j] * wsm[j][e];
  if (c < ncat1 && e < Ge) part[((long)k * ncat1 + c) * Ge + e] = acc;
}

__global__ void gc_egrad_sum_kernel(const float* __restrict__ part, float* __restrict__ demb, int nk, int ncat1,
                                    int Ge) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncat1 * Ge) return;
  float s = 0.f;
  for (int k = 0; k < nk; ++k) s += part[(long)k * ncat1 * Ge + i];
  demb[i] = s;
}

// LCcat[i][l·2Cd + s·Cd + o] = W_s[l][i][o]  (pack = 1)  or the inverse scatter (pack = 0)
__global__ void lc_pack_kernel(float* __restrict__ cat, float* __restrict__ wsig, float* __restrict__ wgate, int L,
                               int Clc, int Cd, int pack) {
  const long total = (long)Clc * L * 2 * Cd;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i % ((long)L * 2 * Cd)), k = (int)(i / ((long)L * 2 * Cd));
    const int l = n / (2 * Cd), s = (n / Cd) & 1, o = n % Cd;
    float* w = (s == 0 ? wsig : wgate) + ((long)l * Clc + k) * Cd + o;
    if (pack == 1) cat[i] = *w;
    else if (pack == 2) *w = cat[(long)n * Clc + k];   // unpack from catᵀ [L·2Cd][Clc]
    else *w = cat[i];
  }
}

int grid_for(long n) { return (int)std::min<long>((n + 255) / 256, 4096); }

// ---- LC upsample fused over its stages (tmodel.py:68-83) ------------------------------------------
// Stage i (conv1d_transpose, kernel = stride = s_i, SAME: non-overlapping) maps a frame's rows
// [R_i][I_i] to [R_i·s_i][Lo]: out[s·t + j][o] = Σ_c in[t][c]·F_i[j][o][c].  A mel frame's whole
// upsample (1 -> 4 -> 16 -> 64 -> 256 rows for arch5) is one block's work: one launch per
// direction instead of a (split-K) GEMM per stage and direction (arch5 B = 8: 4 + 9 launches of
// 20-40 µs each, latency-bound).  f32 FMA, 4 x s / 4 x 4 / 2 x 4 register micro-tiles over LDS
// operands (b128 reads, filter rows padded to I + 4 floats: conflict-free).
constexpr int UP_THREADS = 1024;   // 16 waves: the stages are LDS-latency bound at one block per CU
constexpr int UP_MAXS = 8;           // stride per stage
constexpr int UP_LDS = 40448;        // floats (158 KiB)
struct UpK {
  const float* mel;                  // [frames][Li]
  const float* F[4];                 // stage filters [s][Lo][I]
  float* act[4];                     // stage outputs, [frames·R_{i+1}][Lo]
  const float* dlc;                  // backward: d(last stage output) [frames·hop][Lo], or its
  int dlc_parts; long dlc_stride;    // dlc_parts split-K partials dlc_stride floats apart (summed here)
  float* dpart;                      // backward: per-frame filter-gradient partials [frames][Σ_i s_i·Lo·I_i]
  int nup, s[4], Li, Lo, frames;
  float* dmel;                       // backward<true>: d(mel) [frames][Li]
};

// F_i rows [n0, n0 + nr) (n = j·Lo + o, each I floats) -> W[n - n0][I + 4]
LBWN_DEV void up_load_rows(float* W, const float* F, int n0, int nr, int I, int tid) {
  const int I4 = I / 4, tot = nr * I4;
  for (int e0 = tid; e0 < tot; e0 += 8 * UP_THREADS) {
    floatx4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = min(e0 + u * UP_THREADS, tot - 1);
      v[u] = *(const floatx4*)(F + (long)(n0 + e / I4) * I + 4 * (e % I4));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + u * UP_THREADS;
      if (e < tot) *(floatx4*)(W + (e / I4) * (I + 4) + 4 * (e % I4)) = v[u];
    }
  }
}
// rows [R][C] of global src (row stride C) -> LDS [R][C + 4]
LBWN_DEV void up_load_tile(float* dst, const float* src, int R, int C, int tid) {
  const int C4 = C / 4, tot = R * C4;
  for (int e0 = tid; e0 < tot; e0 += 4 * UP_THREADS) {
    floatx4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = min(e0 + u * UP_THREADS, tot - 1);
      v[u] = *(const floatx4*)(src + (long)(e / C4) * C + 4 * (e % C4));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * UP_THREADS;
      if (e < tot) *(floatx4*)(dst + (e / C4) * (C + 4) + 4 * (e % C4)) = v[u];
    }
  }
}

LBWN_DEV float dot4f(floatx4 a, floatx4 b, float c) {
  c = fmaf(a[0], b[0], c);
  c = fmaf(a[1], b[1], c);
  c = fmaf(a[2], b[2], c);
  return fmaf(a[3], b[3], c);
}

// Forward: LDS = W (the stage's filter, [s·Lo][I + 4]) | two row buffers [R][Lo + 4].
// SC > 0: every stage's stride is SC (arch5: 4, 4, 4, 4), so the j loop has no runtime guard: with
// `if (j < s)` each j's filter read sat in its own basic block behind an `s_waitcnt vmcnt(0)
// lgkmcnt(0)`, one exposed LDS round trip (and store drain) per j and k-step.
template <int SC>
__global__ __launch_bounds__(UP_THREADS) void lc_up_fwd_kernel(UpK a) {
  __shared__ __attribute__((aligned(16))) float sm[UP_LDS];
  const int f = blockIdx.x, tid = threadIdx.x, Lo = a.Lo, LP = Lo + 4;
  int R = 1, I = a.Li;
  int maxw = 0, last_in = 1;
  for (int i = 0; i < a.nup; ++i) {
    maxw = max(maxw, a.s[i] * Lo * ((i ? Lo : a.Li) + 4));
    if (i + 1 < a.nup) last_in *= a.s[i];
  }
  float* W = sm;
  // the two row buffers by offset from the LDS array (a pointer table indexed at run time lost
  // the address space: the x reads became flat loads, each k-step waiting on vmcnt(0) behind the
  // block's outstanding global stores)
  const int ob0 = maxw, ob1 = maxw + last_in * LP;
  int in_off = ob0;
  up_load_tile(sm + in_off, a.mel + (long)f * a.Li, 1, a.Li, tid);   // stage 0 input: the mel frame (row stride Li + 4)
  int IP = a.Li + 4;
  constexpr int NJ = SC ? SC : UP_MAXS;
  for (int i = 0; i < a.nup; ++i) {
    const int s = SC ? SC : a.s[i], N = s * Lo;
    up_load_rows(W, a.F[i], 0, N, I, tid);
    __syncthreads();
    const int out_off = ((i + 1) & 1) ? ob1 : ob0;
    const float* in = sm + in_off;
    float* out = sm + out_off;
    const bool keep = i + 1 < a.nup;
    float* g = a.act[i] + (long)f * R * s * Lo;
    const int RT = (R + 3) / 4;
    for (int w = tid; w < Lo * RT; w += UP_THREADS) {
      const int o = w % Lo, rt = w / Lo;
      float acc[4][NJ];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[ii][j] = 0.f;
#pragma unroll 2
      for (int k = 0; k < I; k += 4) {
        floatx4 x[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) x[ii] = *(const floatx4*)(in + min(4 * rt + ii, R - 1) * IP + k);
        if (SC) {   // every filter read of the k-step issued before the FMAs
          floatx4 wv[NJ];
#pragma unroll
          for (int j = 0; j < NJ; ++j) wv[j] = *(const floatx4*)(W + (j * Lo + o) * (I + 4) + k);
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) acc[ii][j] = dot4f(x[ii], wv[j], acc[ii][j]);
        } else {
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (j < s) {
              const floatx4 wv = *(const floatx4*)(W + (j * Lo + o) * (I + 4) + k);
#pragma unroll
              for (int ii = 0; ii < 4; ++ii) acc[ii][j] = dot4f(x[ii], wv, acc[ii][j]);
            }
          }
        }
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int t = 4 * rt + ii;
        if (t >= R) break;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < s) {
            g[(long)(s * t + j) * Lo + o] = acc[ii][j];
            if (keep) out[(s * t + j) * LP + o] = acc[ii][j];
          }
        }
      }
    }
    __syncthreads();   // W and `in` are free; `out` is the next stage's input
    in_off = out_off;
    IP = LP;
    R *= s;
    I = Lo;
  }
}

// Backward, per frame, stages nup-1 .. 0 with D = d(stage output) rows [R·s][Lo] in LDS:
//   dF_i partial [s·Lo][I] = Σ_t D[t][n]·IN[t][c]  (D viewed [R][s·Lo], IN = the stage input rows)
//   din [R][I]             = Σ_n D[t][n]·F_i[n][c]  (the previous stage's D; for stage 0 the mel
//                            gradient: DMEL forms its one row in a loop of its own and stores it to
//                            a.dmel, else it is skipped)
// LDS = D [hop][Lo + 4] | DN (din) [hop / s_last][Lo + 4] | IN [R][I + 4] | W (one phase j of
// F_i: [Lo][I + 4]), D and DN swapping roles per stage.
template <bool DMEL>
__global__ __launch_bounds__(UP_THREADS) void lc_up_bwd_kernel(UpK a) {
  __shared__ __attribute__((aligned(16))) float sm[UP_LDS];
  const int f = blockIdx.x, tid = threadIdx.x, Lo = a.Lo, LP = Lo + 4;
  int hop = 1, offs[4], ptot = 0;
  for (int i = 0; i < a.nup; ++i) {
    hop *= a.s[i];
    offs[i] = ptot;
    ptot += a.s[i] * Lo * (i ? Lo : a.Li);
  }
  const int Imax = max(a.Li, Lo);
  float* D = sm;
  float* DN = D + hop * LP;
  float* INB = DN + (hop / a.s[a.nup - 1]) * LP;
  float* W = INB + (hop / a.s[a.nup - 1]) * (Imax + 4);
  {   // D = d(last stage output) rows of this frame: the dlc GEMM's split-K partials summed in order
    const float* src = a.dlc + (long)f * hop * Lo;
    const int C4 = Lo / 4, tot = hop * C4;
    for (int e = tid; e < tot; e += UP_THREADS) {
      const long off = (long)(e / C4) * Lo + 4 * (e % C4);
      floatx4 v = *(const floatx4*)(src + off);
      for (int z = 1; z < a.dlc_parts; ++z) v += *(const floatx4*)(src + z * a.dlc_stride + off);
      *(floatx4*)(D + (e / C4) * LP + 4 * (e % C4)) = v;
    }
  }
  int R = hop;
  for (int i = a.nup - 1; i >= 0; --i) {
    const int s = a.s[i], I = i ? Lo : a.Li, IP = I + 4, N = s * Lo;
    R /= s;   // stage input rows
    const float* inp = i ? a.act[i - 1] + (long)f * R * Lo : a.mel + (long)f * a.Li;
    up_load_tile(INB, inp, R, I, tid);
    __syncthreads();
    // dF_i partial: work item = (n4 group, c4 group), 4 x 4 outputs, K = R rows
    float* dp = a.dpart + (long)f * ptot + offs[i];
    const int C4 = I / 4;
    for (int w = tid; w < (N / 4) * C4; w += UP_THREADS) {
      const int c4 = w % C4, n4 = w / C4, j = (4 * n4) / Lo, o = (4 * n4) % Lo;
      floatx4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
      for (int t = 0; t < R; ++t) {
        const floatx4 dv = *(const floatx4*)(D + (s * t + j) * LP + o);
        const floatx4 xv = *(const floatx4*)(INB + t * IP + 4 * c4);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += dv[q] * xv;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) *(floatx4*)(dp + (long)(4 * n4 + q) * I + 4 * c4) = acc[q];
    }
    if (i == 0) {   // no previous stage: the gradient into the mel input, when it is wanted
      if (DMEL) {
        // dmel row [Li] = Σ_{j,o} D[j][o]·F_0[j][o][c]: R = 1 input row, so the 2-row work items below
        // would leave all but Li / 4 threads idle over K = s·Lo.  Here K is spread instead: thread
        // (c4, sl) sums the o groups sl, sl + NS, ... of every phase j (F_0's phases through W as
        // below), the NS slice sums go through W (free after the last phase: NS <= Lo / 4 rows of
        // [Lo][I + 4]) and thread c4 adds them in slice order: a fixed order, the same bits every run.
        const int G = Lo / 4, NS = min(G, UP_THREADS / C4), c4 = tid % C4, sl = tid / C4;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < s; ++j) {
          __syncthreads();   // W free
          up_load_rows(W, a.F[0], j * Lo, Lo, I, tid);
          __syncthreads();
          if (sl < NS) {
            for (int og = sl; og < G; og += NS) {
              const floatx4 d0 = *(const floatx4*)(D + j * LP + 4 * og);
#pragma unroll
              for (int q = 0; q < 4; ++q) acc += d0[q] * *(const floatx4*)(W + (4 * og + q) * IP + 4 * c4);
            }
          }
        }
        __syncthreads();   // the last phase's readers are done with W
        if (sl < NS) *(floatx4*)(W + sl * IP + 4 * c4) = acc;
        __syncthreads();
        if (tid < C4) {
          floatx4 r = *(const floatx4*)(W + 4 * tid);
          for (int z = 1; z < NS; ++z) r += *(const floatx4*)(W + z * IP + 4 * tid);
          *(floatx4*)(a.dmel + (long)f * a.Li + 4 * tid) = r;
        }
      }
      break;
    }
    // din: work item = (2-row group, c4 group), K = s·Lo in phases j (one phase of F_i in W)
    const int RT2 = (R + 1) / 2, nwork = RT2 * C4;
    floatx4 acc[2][2];   // up to 2 work items per thread (R·I/8 <= 2·512)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[u][0] = acc[u][1] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < s; ++j) {
      __syncthreads();   // W free (previous phase / the dF loop's readers done with INB are not W's)
      up_load_rows(W, a.F[i], j * Lo, Lo, I, tid);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int w = tid + u * UP_THREADS;
        if (w >= nwork) break;
        const int c4 = w % C4, r2 = w / C4, t0 = 2 * r2, t1 = min(2 * r2 + 1, R - 1);
#pragma unroll 2
        for (int o = 0; o < Lo; o += 4) {
          const floatx4 d0 = *(const floatx4*)(D + (s * t0 + j) * LP + o);
          const floatx4 d1 = *(const floatx4*)(D + (s * t1 + j) * LP + o);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const floatx4 wv = *(const floatx4*)(W + (o + q) * IP + 4 * c4);
            acc[u][0] += d0[q] * wv;
            acc[u][1] += d1[q] * wv;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int w = tid + u * UP_THREADS;
      if (w >= nwork) break;
      const int c4 = w % C4, r2 = w / C4;
      *(floatx4*)(DN + (2 * r2) * LP + 4 * c4) = acc[u][0];
      if (2 * r2 + 1 < R) *(floatx4*)(DN + (2 * r2 + 1) * LP + 4 * c4) = acc[u][1];
    }
    __syncthreads();   // DN complete; D and INB free
    float* tmp = D;
    D = DN;
    DN = tmp;
  }
}

// filter gradients: dF[e] = Σ_f dpart[f][e], frames in order (deterministic)
__global__ void lc_up_sum_kernel(const float* __restrict__ dpart, UpK a, float* g0, float* g1, float* g2, float* g3,
                                 int ptot) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ptot) return;
  float s = 0.f;
  for (int f = 0; f < a.frames; ++f) s += dpart[(long)f * ptot + e];
  int off = 0;
  float* g[4] = {g0, g1, g2, g3};
  for (int i = 0; i < a.nup; ++i) {
    const int n = a.s[i] * a.Lo * (i ? a.Lo : a.Li);
    if (e < off + n) { g[i][e - off] = s; return; }
    off += n;
  }
}

}  // namespace

int lbwn_gc_part_floats(int L, int Ge, int Cd) { return GC_CSPLIT * Ge * 2 * L * Cd; }

// the fused upsample's envelope (else the per-stage GEMMs): <= 4 stages of stride <= 8, widths
// multiples of 4, hop <= 256, and both kernels' LDS carve-outs within UP_LDS
int lbwn_lc_up_fused_ok(int nup, const int* s, int Li, int Lo) {
  if (nup < 1 || nup > 4 || Li % 4 || Lo % 4 || Li < 4 || Lo < 4 || Li > Lo) return 0;
  int hop = 1, maxw = 0, last_in = 1;
  for (int i = 0; i < nup; ++i) {
    if (s[i] < 1 || s[i] > UP_MAXS) return 0;
    hop *= s[i];
    maxw = std::max(maxw, s[i] * Lo * ((i ? Lo : Li) + 4));
    if (i + 1 < nup) last_in *= s[i];
  }
  if (hop > 256) return 0;
  const int fwd = maxw + 2 * std::max(last_in, 1) * (Lo + 4) + (Li + 4);
  const int Imax = std::max(Li, Lo), rin = hop / s[nup - 1];
  const int bwd = hop * (Lo + 4) + rin * (Lo + 4) + rin * (Imax + 4) + Lo * (Imax + 4);
  // din work items per thread <= 2
  for (int i = 1; i < nup; ++i) {
    int R = 1;
    for (int j = 0; j < i; ++j) R *= s[j];
    if ((R + 1) / 2 * (Lo / 4) > 2 * UP_THREADS) return 0;
  }
  return fwd <= UP_LDS && bwd <= UP_LDS;
}
int lbwn_lc_up_part_floats(int nup, const int* s, int Li, int Lo, int frames) {
  long tot = 0;
  for (int i = 0; i < nup; ++i) tot += (long)s[i] * Lo * (i ? Lo : Li);
  return (int)(tot * frames);
}

static UpK up_args(int nup, const int* s, int Li, int Lo, int frames, const float* mel, const float* const* F,
                   float* const* act) {
  UpK k;
  memset(&k, 0, sizeof(k));
  k.mel = mel; k.nup = nup; k.Li = Li; k.Lo = Lo; k.frames = frames;
  for (int i = 0; i < nup; ++i) { k.s[i] = s[i]; k.F[i] = F[i]; k.act[i] = act[i]; }
  return k;
}

int lbwn_lc_up_fwd_launch(int nup, const int* s, int Li, int Lo, int frames, const float* mel, const float* const* F,
                          float* const* act, hipStream_t st) {
  LBWN_REQUIRE(lbwn_lc_up_fused_ok(nup, s, Li, Lo), "lc upsample: shape outside the fused kernel's envelope");
  UpK k = up_args(nup, s, Li, Lo, frames, mel, F, act);
  bool all4 = true;
  for (int i = 0; i < nup; ++i) all4 = all4 && s[i] == 4;
  if (all4) lc_up_fwd_kernel<4><<<frames, UP_THREADS, 0, st>>>(k);
  else lc_up_fwd_kernel<0><<<frames, UP_THREADS, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_lc_up_bwd_launch(int nup, const int* s, int Li, int Lo, int frames, const float* mel, const float* const* F,
                          float* const* act, const float* dlc, float* dpart, float* const* dF, hipStream_t st,
                          hipStream_t st_sum, hipEvent_t ev, int dlc_parts, long dlc_stride, float* dmel) {
  LBWN_REQUIRE(lbwn_lc_up_fused_ok(nup, s, Li, Lo), "lc upsample: shape outside the fused kernel's envelope");
  UpK k = up_args(nup, s, Li, Lo, frames, mel, F, act);
  k.dlc = dlc; k.dpart = dpart;
  k.dlc_parts = std::max(dlc_parts, 1); k.dlc_stride = dlc_stride;
  k.dmel = dmel;
  if (dmel) lc_up_bwd_kernel<true><<<frames, UP_THREADS, 0, st>>>(k);    // ... and stage 0's din, to dmel
  else lc_up_bwd_kernel<false><<<frames, UP_THREADS, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  int ptot = 0;
  for (int i = 0; i < nup; ++i) ptot += s[i] * Lo * (i ? Lo : Li);
  if (st_sum && st_sum != st && ev) {
    LBWN_HIP(hipEventRecord(ev, st));
    LBWN_HIP(hipStreamWaitEvent(st_sum, ev, 0));
  } else {
    st_sum = st;
  }
  lc_up_sum_kernel<<<(ptot + 255) / 256, 256, 0, st_sum>>>(dpart, k, dF[0], nup > 1 ? dF[1] : nullptr,
                                                       nup > 2 ? dF[2] : nullptr, nup > 3 ? dF[3] : nullptr, ptot);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_gc_table_launch(const float* emb, const float* wsig, const float* wgate, float* out, int L, int ncat1,
                         int Ge, int Cd, hipStream_t st) {
  const int N = 2 * L * Cd;
  gc_table_kernel<<<grid_for((long)ncat1 * N), 256, 0, st>>>(emb, wsig, wgate, out, N, ncat1, Ge, Cd);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_gc_grad_launch(const float* emb, const float* wsig, const float* wgate, const float* gcd, float* part,
                        float* demb, float* dsig, float* dgate, int L, int ncat1, int Ge, int Cd, hipStream_t st) {
  LBWN_REQUIRE(Ge >= 1 && Ge <= GC_EMAX, "gc grads: n_gc_embed must be in [1, %d]", GC_EMAX);
  const int N = 2 * L * Cd;
  gc_wgrad_kernel<<<(Ge * N + 255) / 256, 256, 0, st>>>(emb, gcd, dsig, dgate, N, ncat1, Ge, Cd);
  LBWN_CHECK_LAUNCH();
  // (part: GC_CSPLIT·Ge·N >= nk·ncat1·Ge floats holds for every shipped arch and is checked here)
  const int nk = (N + GE_N - 1) / GE_N, ep = Ge <= 16 ? 16 : 32, cpb = 256 / ep;
  LBWN_REQUIRE((long)nk * ncat1 * Ge <= (long)GC_CSPLIT * Ge * N, "gc grads: partial buffer too small");
  gc_egrad_part_kernel<<<dim3((ncat1 + cpb - 1) / cpb, nk), 256, 0, st>>>(gcd, wsig, wgate, part, N, ncat1, Ge, Cd);
  LBWN_CHECK_LAUNCH();
  gc_egrad_sum_kernel<<<(ncat1 * Ge + 255) / 256, 256, 0, st>>>(part, demb, nk, ncat1, Ge);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_lc_pack_launch(float* cat, float* wsig, float* wgate, int L, int Clc, int Cd, int pack, hipStream_t st) {
  lc_pack_kernel<<<grid_for((long)Clc * L * 2 * Cd), 256, 0, st>>>(cat, wsig, wgate, L, Clc, Cd, pack);
  LBWN_CHECK_LAUNCH();
  return 0;
}
