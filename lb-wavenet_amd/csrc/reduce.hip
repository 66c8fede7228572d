// Deterministic sum kernels of the backward: the PRE-embedding gradient (the transpose of the
// one-hot product, tmodel.py:53-66) as an LDS-histogram scatter, and the column sums behind the
// bias gradients.  Both are two passes, partials then a fixed-order reduce: no atomics on global memory.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

// ---- PRE-embedding gradient -------------------------------------------------------------
// dPRE[q][c] = Σ_{t: code_t = q} dx0[t][c] and dPRE_B[c] = Σ_t dx0[t][c]: the transpose of the
// one-hot product (tmodel.py:64-66; tf.one_hot: a code outside [0, Q) has no row).  A scatter
// into an LDS histogram, not a dense GEMM against the one-hot matrix (K = B·T, M = Q, N = Cr:
// ~200 µs of tiles that are almost all zeros).  dx0 = g + shift(dprev) (layer 0's input
// gradient) is formed on the fly and never stored.  Each wave of a block
// owns an LDS histogram and a contiguous sub-chunk of the block's positions, walked two positions
// per instruction (half-wave h takes h, h+2, ...) with no-return LDS float atomics (ds_add_f32:
// no read-modify-write round trip); a single wave's atomics are applied in program and lane
// order, the block's wave histograms are summed in wave order and the block partials are reduced
// in a fixed order, so the sums are deterministic.  Default 256 one-wave blocks (32 KB of LDS
// each, so they find room beside dSKIP's GEMM blocks; 128 x 1 and 256 x 2 measured slower).
constexpr int PG_BLOCKS = 256;
constexpr int PG_WAVES = 2;
constexpr int PG_BATCH = 4;    // small: <= 32 VGPRs so the blocks fit beside dSKIP's (see below)

// At most 32 VGPRs (27 / 25 for the reduce at this writing): it runs beside dSKIP's A-in-registers GEMM (2 waves of 240 VGPRs per SIMD)
__global__ __launch_bounds__(64 * PG_WAVES) void pre_grad_part_kernel(
    const int* __restrict__ q, const float* __restrict__ g, const float* __restrict__ dprev, int gd, int B, int T,
    int Cr, int Q, float* part, float* bpart) {
  extern __shared__ __attribute__((aligned(16))) float hist_all[];   // [nw][Q][32]
  __shared__ float bred[PG_WAVES][32];
  const int nw = blockDim.x >> 6;   // PG_WAVES, or 1 when two histograms exceed 64 KB (Q > 256)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, c = lane & 31, cc = min(c, Cr - 1);
  float* hist = hist_all + (long)wv * Q * 32;
  for (int i = threadIdx.x; i < nw * Q * 32 / 4; i += 64 * nw)
    ((float4*)hist_all)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const long M = (long)B * T;
  const long chunk = (M + gridDim.x - 1) / gridDim.x, b0 = blockIdx.x * chunk, b1 = min(M, b0 + chunk);
  const long sub = (chunk + nw - 1) / nw, m0 = b0 + wv * sub, m1 = min(b1, m0 + sub);
  float bsum = 0.f;
  // 32-bit position arithmetic (M·Cr < 2^31, checked by the launcher): the kernel must stay within
  // the 32 VGPRs dSKIP's blocks leave per SIMD
  const int Mi = (int)M, m1i = (int)m1;
  for (int mb = (int)m0 + h; mb < m1i; mb += 2 * PG_BATCH) {
    int cd[PG_BATCH];
    float v[PG_BATCH], w[PG_BATCH];
#pragma unroll
    for (int i = 0; i < PG_BATCH; ++i) {   // loads first (clamped indices: no branch per load)
      const int m = min(mb + 2 * i, m1i - 1);
      const int ms = min(m + gd, Mi - 1);
      cd[i] = q[m];
      v[i] = g[m * Cr + cc];
      w[i] = dprev[ms * Cr + cc];
    }
#pragma unroll
    for (int i = 0; i < PG_BATCH; ++i) {
      const int m = mb + 2 * i;
      if (m >= m1i || c >= Cr) continue;
      const float x = v[i] + (m % T + gd < T ? w[i] : 0.f);
      bsum += x;
      if (cd[i] >= 0 && cd[i] < Q)
        __hip_atomic_fetch_add(hist + cd[i] * 32 + c, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  const float bo = __shfl_xor(bsum, 32);
  if (lane < 32) bred[wv][lane] = bsum + bo;
  __syncthreads();
  float* P = part + (long)blockIdx.x * Q * Cr;
  for (int e = threadIdx.x; e < Q * Cr; e += 64 * nw) {
    const int qq = e / Cr, c2 = e % Cr;
    float s = hist_all[qq * 32 + c2];
    for (int k = 1; k < nw; ++k) s += hist_all[(long)k * Q * 32 + qq * 32 + c2];
    P[e] = s;
  }
  if (threadIdx.x < Cr) {
    float s = bred[0][threadIdx.x];
    for (int k = 1; k < nw; ++k) s += bred[k][threadIdx.x];
    bpart[(long)blockIdx.x * Cr + threadIdx.x] = s;
  }
}

// 256 threads = 16 part lanes x 16 columns per block: lane pl sums partials pl, pl + 16, ... in
// order, then the 16 lane sums are added in order (deterministic).  (One thread per column
// walking all 256 partials ran 50 us beside dSKIP.)
__global__ __launch_bounds__(256) void pre_grad_reduce_kernel(const float* part, const float* bpart, int nparts,
                                                              int Q, int Cr, float* dpre, float* dpre_b) {
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + cl, n = Q * Cr;
  const bool bias = e >= n;
  const bool live = bias ? (dpre_b != nullptr && e - n < Cr) : true;
  const float* p = bias ? bpart + min(e - n, Cr - 1) : part + e;
  const long stride = bias ? Cr : n;
  float s = 0.f;
  if (live) {
    const int sti = (int)stride;
    for (int q0 = pl; q0 < nparts; q0 += 64) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p[min(q0 + 16 * i, nparts - 1) * sti];
#pragma unroll
      for (int i = 0; i < 4; ++i) s += (q0 + 16 * i < nparts) ? v[i] : 0.f;
    }
  }
  red[pl][cl] = s;
  __syncthreads();
  if (threadIdx.x < 16 && live) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cl];
    if (bias) dpre_b[e - n] = t;
    else dpre[e] = t;
  }
}

// ---- column sums (bias gradients), deterministic two-pass ------------------------------------
// pass 1: block = CS_ROWS rows × all N columns (float4 groups × row lanes); pass 2: 1024
// threads per 64 columns sum the chunk partials.  N % 4 == 0, N <= 1024.

constexpr int CS_ROWS = 64;
// up to 4 column sums of M-row matrices in one launch pair (blockIdx.y = job)
struct ColsumJobs {
  const float* X[4];
  long ldx[4];
  int N[4];
  float* out[4];
  int accumulate[4];
  float* ws[4];
  int nparts[4];   // partial rows per job (colsum_final_kernel)
  int reps[4];     // copies of the result row written (out + r·N), colsum_final_kernel
};
__global__ __launch_bounds__(256) void colsum_partial_kernel(ColsumJobs jb, int M) {
  __shared__ floatx4 red[256];
  const int j = blockIdx.y;
  const float* X = jb.X[j];
  const long ldx = jb.ldx[j];
  const int N = jb.N[j];
  float* part = jb.ws[j];
  const int ng = N / 4, RL = max(1, 256 / ng);
  const int t = threadIdx.x, g = t % ng, rl = t / ng;
  const int r0 = blockIdx.x * CS_ROWS;
  floatx4 s = {0.f, 0.f, 0.f, 0.f};
  if (rl < RL && g < ng) {
    const int r1 = min(M, r0 + CS_ROWS);
#pragma unroll 8
    for (int r = r0 + rl; r < r1; r += RL) s += *(const floatx4*)(X + (long)r * ldx + 4 * g);
  }
  red[t] = s;
  __syncthreads();
  if (t < ng) {
    floatx4 tot = red[t];
    for (int k = 1; k < RL; ++k) tot += red[k * ng + t];
    *(floatx4*)(part + (long)blockIdx.x * N + 4 * t) = tot;
  }
}
// 256 threads = 16 part lanes × 16 columns per block (grid: N/16 column blocks × jobs): each lane
// sums every 16th partial row in order, then the 16 lane sums are added in order (deterministic).
// (4 part lanes × 64 columns left 256-deep serial sums per thread once the head wrote 1024
// partial rows: 21 µs for the three bias sums)
__global__ __launch_bounds__(256) void colsum_final_kernel(ColsumJobs jb) {
  __shared__ float red[16][17];
  const int j = blockIdx.y, N = jb.N[j], nparts = jb.nparts[j];
  const float* part = jb.ws[j];
  const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  if (blockIdx.x * 16 >= N) return;   // block-uniform
  float s = 0.f;
  if (c < N) {
#pragma unroll 8
    for (int p = lane; p < nparts; p += 16) s += part[(long)p * N + c];
  }
  red[lane][cl] = s;
  __syncthreads();
  if (threadIdx.x < 16 && c < N) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) tot += red[k][cl];
    float* out = jb.out[j];
    for (int r = 0; r < max(1, jb.reps[j]); ++r) {
      float* o = out + (long)r * N + c;
      *o = jb.accumulate[j] ? *o + tot : tot;
    }
  }
}

__global__ void sum_bias_kernel(const float* b, int L, int N, float* out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 10
  for (int l = 0; l < L; ++l) s += b[(long)l * N + n];
  out[n] = s;
}

}  // namespace

int lbwn_pre_grad_ws_floats(int Q, int Cr) { return PG_BLOCKS * (Q * Cr + Cr); }

int lbwn_pre_grad_launch(const int* q, const float* g, const float* dprev, int gd, int B, int T, int Cr, int Q,
                         float* dpre, float* dpre_b, float* ws, hipStream_t st) {
  // the histogram is Q rows of 32 floats: up to 64 KB (Q <= 512) as ever; a wider head (the plan takes
  // any n_quant) asks for a larger dynamic LDS block, up to 128 KB of the CU's 160
  LBWN_REQUIRE(Cr >= 1 && Cr <= 32 && Q >= 1 && Q <= 1024, "pre_grad: Cr <= 32 and Q <= 1024 required");
  LBWN_REQUIRE((long)B * T * Cr < (1L << 31), "pre_grad: B*T*Cr must be < 2^31");
  const int nb = PG_BLOCKS, nw = 1;   // one-wave blocks (two-wave blocks wait for LDS)
  if (nw * Q * 32 * 4 > 65536)
    LBWN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pre_grad_part_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, nw * Q * 32 * 4));
  float* part = ws;
  float* bpart = ws + (long)PG_BLOCKS * Q * Cr;
  pre_grad_part_kernel<<<nb, 64 * nw, nw * Q * 32 * 4, st>>>(q, g, dprev, gd, B, T, Cr, Q, part, bpart);
  LBWN_CHECK_LAUNCH();
  const int n = Q * Cr + Cr;
  pre_grad_reduce_kernel<<<(n + 15) / 16, 256, 0, st>>>(part, bpart, nb, Q, Cr, dpre, dpre_b);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_colsum_ws_floats(int M, int N) { return ((M + CS_ROWS - 1) / CS_ROWS) * N; }

// job j's fields for the first pass: the matrix, and where its partial rows go
static int colsum_job_in(ColsumJobs& jb, int j, const float* X, long ldx, int N, float* ws) {
  LBWN_REQUIRE(N % 4 == 0 && N <= 1024 && ldx % 4 == 0, "colsum: N %% 4 / N <= 1024 / ldx %% 4 required");
  jb.X[j] = X; jb.ldx[j] = ldx; jb.N[j] = N; jb.ws[j] = ws;
  return 0;
}
// job j's fields for the second pass: the partial rows, and where their sum goes
static void colsum_job_out(ColsumJobs& jb, int j, float* parts, int nparts, int N, float* out, int acc, int reps) {
  jb.ws[j] = parts; jb.nparts[j] = nparts; jb.N[j] = N; jb.out[j] = out; jb.accumulate[j] = acc; jb.reps[j] = reps;
}

int lbwn_colsum_multi_launch(int njobs, const float* const* X, const long* ldx, const int* N, float* const* out,
                             const int* accumulate, int M, float* ws, hipStream_t st) {
  LBWN_REQUIRE(njobs >= 1 && njobs <= 4, "colsum: 1..4 jobs");
  ColsumJobs jb;
  memset(&jb, 0, sizeof(jb));
  const int np = (M + CS_ROWS - 1) / CS_ROWS;
  int nmax = 0, e;
  float* w = ws;
  for (int j = 0; j < njobs; ++j) {
    if ((e = colsum_job_in(jb, j, X[j], ldx[j], N[j], w))) return e;
    colsum_job_out(jb, j, w, np, N[j], out[j], accumulate[j], 1);
    w += (long)np * N[j];
    nmax = std::max(nmax, N[j]);
  }
  colsum_partial_kernel<<<dim3(np, njobs), 256, 0, st>>>(jb, M);
  colsum_final_kernel<<<dim3((nmax + 15) / 16, njobs), 256, 0, st>>>(jb);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_colsum_partial_launch(const float* X, long ldx, int M, int N, float* ws, int* nparts, hipStream_t st) {
  ColsumJobs jb;
  memset(&jb, 0, sizeof(jb));
  int e;
  if ((e = colsum_job_in(jb, 0, X, ldx, N, ws))) return e;
  const int np = (M + CS_ROWS - 1) / CS_ROWS;
  colsum_partial_kernel<<<dim3(np, 1), 256, 0, st>>>(jb, M);
  LBWN_CHECK_LAUNCH();
  *nparts = np;
  return 0;
}

int lbwn_colsum_final_launch(int njobs, float* const* parts, const int* N, float* const* out, const int* accumulate,
                             const int* nparts, hipStream_t st, const int* reps) {
  LBWN_REQUIRE(njobs >= 1 && njobs <= 4, "colsum_final: 1..4 jobs");
  ColsumJobs jb;
  memset(&jb, 0, sizeof(jb));
  int nmax = 0;
  for (int j = 0; j < njobs; ++j) {
    LBWN_REQUIRE(nparts[j] >= 1, "colsum_final: nparts >= 1");
    colsum_job_out(jb, j, parts[j], nparts[j], N[j], out[j], accumulate[j], reps ? reps[j] : 1);
    nmax = std::max(nmax, N[j]);
  }
  colsum_final_kernel<<<dim3((nmax + 15) / 16, njobs), 256, 0, st>>>(jb);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_sum_bias_launch(const float* b, int L, int N, float* out, hipStream_t st) {
  sum_bias_kernel<<<(N + 63) / 64, 64, 0, st>>>(b, L, N, out);
  LBWN_CHECK_LAUNCH();
  return 0;
}
