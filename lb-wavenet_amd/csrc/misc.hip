// Small byte-bound utilities: D-separation prepend/save (tmodel.py:122-127, :165), the PRE embedding
// (tmodel.py:53-66, :86-102), the µ-law codec (ops.py:4-39), the zero and row-broadcast fillers.  The heads
// are in head.hip, the optimizer in optim.hip, the PRE gradient and the column sums in reduce.hip.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "prologue.h"

namespace {

// ---- D-separation state and embedding: bodies in prologue.h ---------------------------------
template <bool TO_X>
__global__ void dsep_kernel(float* xall, long xls, float* save, int L, int nbl, int B, int T, int H, int Cr, bool v4) {
  dsep_flat_body<TO_X>(blockIdx.x, gridDim.x, xall, xls, save, L, nbl, B, T, H, Cr, v4);
}

__global__ void embed_kernel(const int* __restrict__ q, const float* __restrict__ pre, const float* pre_b,
                             float* x0, int B, int T, int H, int Cr, int Q, bool v4) {
  embed_flat_body(blockIdx.x, gridDim.x, q, pre, pre_b, x0, B, T, H, Cr, Q, v4);
}

// ---- µ-law ---------------------------------------------------------------------------------

__global__ void mulaw_encode_kernel(const float* x, int* q, long n, int nq, int tf32) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    if (tf32) {  // ops.py:4-9, float32 throughout
      const float mu = (float)(nq - 1), xv = x[e];
      const float sg = xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f);
      const float amp = sg * log1pf(mu * fabsf(xv)) / log1pf(mu);
      q[e] = (int)((amp + 1.f) * 0.5f * mu + 0.5f);
    } else {  // ops.py:23-28, numpy float64
      const double mu = (double)(nq - 1), xv = (double)x[e];
      const double sg = xv > 0 ? 1.0 : (xv < 0 ? -1.0 : 0.0);
      const double amp = sg * log1p(mu * fabs(xv)) / log1p(mu);
      q[e] = (int)((amp + 1.0) * 0.5 * mu + 0.5);
    }
  }
}

__global__ void mulaw_decode_kernel(const int* q, float* x, long n, int nq) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const float mu = (float)(nq - 1), inv_mu = 1.f / mu;  // ops.py:12-20
    const float a = (2.f * (float)q[e] - 1.f) * inv_mu - 1.f;
    const float sg = a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f);
    x[e] = sg * (powf(1.f + mu, fabsf(a)) - 1.f) * inv_mu;
  }
}

// ---- fillers ---------------------------------------------------------------------------------

__global__ void bcast_rows_kernel(float* dst, int L, int N) {
  // dst[l][n] = dst[0][n] for l in [1, L)
  const long n_all = (long)(L - 1) * N;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n_all; e += (long)gridDim.x * blockDim.x)
    dst[N + e] = dst[e % N];
}

__global__ void zero_words_kernel(unsigned* p, long n) { zero_body(blockIdx.x, gridDim.x, p, n); }

}  // namespace

// one flat launch over every layer's SAVE rows (dsep_flat_body), one item per thread
static int dsep_launch(bool to_x, float* xall, long xls, float* save, int L, int nbl, int B, int T, int H, int Cr,
                       hipStream_t st) {
  LBWN_REQUIRE(L >= 1 && nbl >= 1 && nbl <= 16 && B >= 1 && Cr >= 1, "dsep: bad shape");
  LBWN_REQUIRE((long)dsep_rows(L, nbl, 1) * B * Cr < (1L << 31), "dsep: SAVE exceeds 32-bit indexing");
  const bool v4 = dsep_v4(xall, xls, save, Cr);
  const long n = (long)dsep_rows(L, nbl, B) * (v4 ? Cr / 4 : Cr);
  const int grid = (int)std::max(1L, std::min(2048L, (n + 255) / 256));
  if (to_x) dsep_kernel<true><<<grid, 256, 0, st>>>(xall, xls, save, L, nbl, B, T, H, Cr, v4);
  else dsep_kernel<false><<<grid, 256, 0, st>>>(xall, xls, save, L, nbl, B, T, H, Cr, v4);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_dsep_prepend_launch(float* xall, long xls, const float* save, int L, int nbl, int B, int T, int H,
                             int Cr, hipStream_t st) {
  return dsep_launch(true, xall, xls, const_cast<float*>(save), L, nbl, B, T, H, Cr, st);
}

int lbwn_dsep_save_launch(const float* xall, long xls, float* save, int L, int nbl, int B, int T, int H, int Cr,
                          hipStream_t st) {
  return dsep_launch(false, const_cast<float*>(xall), xls, save, L, nbl, B, T, H, Cr, st);
}

int lbwn_embed_launch(const int* q, const float* pre, const float* pre_b, float* x0, int B, int T, int H, int Cr,
                      int Q, hipStream_t st) {
  LBWN_REQUIRE((long)B * T * Cr < (1L << 31), "embed: B*T*n_res exceeds 32-bit indexing");
  const bool v4 = embed_v4(pre, pre_b, x0, Cr);
  embed_kernel<<<lbwn_grid_for((long)B * T * (v4 ? Cr / 4 : Cr)), 256, 0, st>>>(q, pre, pre_b, x0, B, T, H, Cr, Q,
                                                                                v4);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_mulaw_encode_launch(const float* x, int* q, long n, int nq, int tf32, hipStream_t st) {
  mulaw_encode_kernel<<<lbwn_grid_for(n), 256, 0, st>>>(x, q, n, nq, tf32);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_mulaw_decode_launch(const int* q, float* x, long n, int nq, hipStream_t st) {
  mulaw_decode_kernel<<<lbwn_grid_for(n), 256, 0, st>>>(q, x, n, nq);
  LBWN_CHECK_LAUNCH();
  return 0;
}

// Zero n_bytes (a multiple of 4) on the stream: an ordinary kernel in the step's launch sequence.
// hipMemsetAsync's fill kernel started 13-18 us after the kernel before it (runtime blit path;
// profiles/r03_v2_step_timeline.txt: counters -> fill at the step start), a plain launch ~2 us.
int lbwn_zero_launch(void* p, size_t n_bytes, hipStream_t st) {
  LBWN_REQUIRE(n_bytes % 4 == 0, "zero: byte count must be a multiple of 4");
  const long n = (long)(n_bytes / 4);
  if (n == 0) return 0;
  zero_words_kernel<<<lbwn_grid_for(n, 256, 1024), 256, 0, st>>>((unsigned*)p, n);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_bcast_rows_launch(float* dst, int L, int N, hipStream_t st) {
  if (L <= 1) return 0;
  bcast_rows_kernel<<<lbwn_grid_for((long)(L - 1) * N), 256, 0, st>>>(dst, L, N);
  LBWN_CHECK_LAUNCH();
  return 0;
}
