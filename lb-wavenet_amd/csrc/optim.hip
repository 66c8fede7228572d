// The optimizer step over the flat parameter buffer: TF1 Adam (train.py:178, :186), the extended
// step (lbwn_adam_ex: global-norm clipping, non-finite skip, weight EMA, LR schedule) and the
// step counters.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

// ---- TF1 Adam over the flat parameter buffer --------------------------------------------------
// grads hold Σ-xent gradients; g = raw·(1/n_valid) + l2·θ for the weight region
// [0, n_weights) (non-BIAS vars, tmodel.py:250-261); biases get no l2 term.
// counters[2] (int64) is Adam's apply count t-1; lr_t = lr·√(1-β2^t)/(1-β1^t).
// status (nullable): the step's chain status word; nonzero = a hand-off timed out and the
// gradients are garbage, so the update is skipped (params, m, v untouched).
// one element of TF1 Adam (training_ops.cc ApplyAdam restated: m, v, then θ -= lr_t·m/(√v + ε))
LBWN_DEV float adam_elem(float th, float g, float& m, float& v, float lr_t, float b1, float b2, float eps) {
  const float mm = b1 * m + (1.f - b1) * g;
  const float vv = b2 * v + (1.f - b2) * g * g;
  m = mm;
  v = vv;
  return th - lr_t * mm / (sqrtf(vv) + eps);
}

// 1/n_valid from the head's stats (0 if no position was scored); 1 without stats
LBWN_DEV float inv_valid(const float* stats) { return stats ? (stats[1] > 0.f ? 1.f / stats[1] : 0.f) : 1.f; }

// the gradient Adam and the norm pass see: raw·inv, + l2·θ on the weight region
LBWN_DEV float adam_grad(float raw, float inv, float l2, float th, bool weight) {
  float g = raw * inv;
  if (weight) g += l2 * th;
  return g;
}

// Four elements per thread as dwordx4 loads and stores (the flat buffers are 16-B aligned, checked
// by the launcher); the n % 4 tail elements one per thread.  HBM-bound: 28 B per parameter.
// HAS_SCALE: Adam takes g·scale (global-norm clipping); HAS_EMA: the shadow follows the element's
// new value in the same pass, shadow -= omd·(shadow - θ_new) (8 more bytes per parameter).  Each
// is compiled in only where asked for, so <false, false> is the plain TF1 step instruction for
// instruction (hipcc contracts a·b + c per kernel).
template <bool HAS_SCALE, bool HAS_EMA>
LBWN_DEV void adam_loop(float* __restrict__ p, const float* __restrict__ gr, float* __restrict__ m,
                        float* __restrict__ v, long nw, long n, float lr_t, float inv, float b1, float b2, float eps,
                        float l2, float scale, float* __restrict__ ema, float omd) {
  const long n4 = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const floatx4 th = ((const floatx4*)p)[i];
    floatx4 g = ((const floatx4*)gr)[i];
    floatx4 mm = ((const floatx4*)m)[i], vv = ((const floatx4*)v)[i], out;
    floatx4 sh;
    if (HAS_EMA) sh = ((const floatx4*)ema)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gj = adam_grad(g[j], inv, l2, th[j], 4 * i + j < nw);
      if (HAS_SCALE) gj *= scale;
      float mj = mm[j], vj = vv[j];
      out[j] = adam_elem(th[j], gj, mj, vj, lr_t, b1, b2, eps);
      mm[j] = mj;
      vv[j] = vj;
      if (HAS_EMA) sh[j] -= omd * (sh[j] - out[j]);
    }
    ((floatx4*)m)[i] = mm;
    ((floatx4*)v)[i] = vv;
    ((floatx4*)p)[i] = out;
    if (HAS_EMA) ((floatx4*)ema)[i] = sh;
  }
  const long e = 4 * n4 + blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e < n) {
    float g = adam_grad(gr[e], inv, l2, p[e], e < nw);
    if (HAS_SCALE) g *= scale;
    float mj = m[e], vj = v[e];
    p[e] = adam_elem(p[e], g, mj, vj, lr_t, b1, b2, eps);
    m[e] = mj;
    v[e] = vj;
    if (HAS_EMA) ema[e] -= omd * (ema[e] - p[e]);
  }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ gr,
                                                   float* __restrict__ m, float* __restrict__ v, long nw, long n,
                                                   float lr, float b1, float b2, float eps, float l2,
                                                   const float* stats, const long long* counters,
                                                   const unsigned* status) {
  if (status && *status) return;
  const double t = (double)(counters[2] + 1);
  const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
  const float inv = inv_valid(stats);
  adam_loop<false, false>(p, gr, m, v, nw, n, lr_t, inv, b1, b2, eps, l2, 1.f, nullptr, 0.f);
}

// ---- the extended step (lbwn_adam_ex): global-norm clipping, non-finite skip, EMA, LR schedule ----
// Pass 1: Σ g² with g exactly the gradient Adam sees (f32 raw·inv, + l2·θ on the weight region),
// squared and summed in double.  The grid is lbwn_adam_ex_nparts(n) blocks, a function of n alone;
// a thread adds its grid-stride elements in index order, the block's 256 sums meet in a fixed LDS
// tree and the block stores one double: no atomics, so the partials are the same bits on every
// device and in every run.  HBM-bound (8 B per weight, 4 B per bias).
constexpr int AX_PARTS = 512;

__global__ __launch_bounds__(256) void adam_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ gr,
                                                         long nw, long n, float l2, const float* stats,
                                                         double* __restrict__ part) {
  __shared__ double sh[256];
  const float inv = inv_valid(stats);
  const long n4 = n >> 2;
  double s = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const floatx4 g = ((const floatx4*)gr)[i];
    floatx4 th = {0.f, 0.f, 0.f, 0.f};
    if (4 * i < nw) th = ((const floatx4*)p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = adam_grad(g[j], inv, l2, th[j], 4 * i + j < nw);
      s += (double)gj * (double)gj;
    }
  }
  const long e = 4 * n4 + blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e < n) {
    float g = gr[e] * inv;
    if (e < nw) g += l2 * p[e];   // not adam_grad(): θ is read on the weight region only
    s += (double)g * (double)g;
  }
  const double tot = block_sum256(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// Pass 2: every block sums the partials in the same fixed order (so all hold the same bits), forms
// scale, the scheduled lr and the EMA step, and updates its elements.  Block 0 leaves the
// non-finite decision in *a.decision for counters_kernel (next in stream order) and writes info.
template <bool HAS_SCALE, bool HAS_EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(lbwn_adam_ex_dev a) {
  __shared__ double sh[256];
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  const double t = (double)(a.counters[2] + 1);
  double lr_eff = (double)a.lr;
  if (a.warmup > 0) lr_eff *= fmin(1.0, t / (double)a.warmup);
  if (a.decay_steps > 0) {
    double ex = t / (double)a.decay_steps;
    if (a.staircase) ex = floor(ex);
    lr_eff *= pow((double)a.decay_rate, ex);
  }
  if (a.status && *a.status) {   // the chain status skips as in adam_kernel; not a non-finite skip
    if (lead) {
      if (a.decision) *a.decision = 0u;
      if (a.info) {
        a.info[0] = 0.f; a.info[1] = 0.f; a.info[2] = 0.f; a.info[3] = (float)lr_eff;
      }
    }
    return;
  }
  double norm = 0.0;
  float scale = 1.f;
  bool skip = false;
  if (a.part) {   // uniform over the grid
    double s = 0.0;
    for (int k = threadIdx.x; k < a.nparts; k += 256) s += a.part[k];
    const double sum = block_sum256(s, sh);
    norm = sqrt(sum);
    skip = (HAS_SCALE || a.skip_nonfinite) && !(fabs(norm) <= 1.7976931348623157e308);
    if (HAS_SCALE && !skip) scale = (float)((double)a.clip / fmax(norm, (double)a.clip));
  }
  if (lead) {
    if (a.decision) *a.decision = skip ? 1u : 0u;
    if (a.info) {
      a.info[0] = (float)norm; a.info[1] = scale; a.info[2] = skip ? 1.f : 0.f; a.info[3] = (float)lr_eff;
    }
  }
  if (skip) return;
  const float lr_t = (float)(lr_eff * sqrt(1.0 - pow((double)a.b2, t)) / (1.0 - pow((double)a.b1, t)));
  const float inv = inv_valid(a.stats);
  float omd = 0.f;
  if (HAS_EMA) {
    double d = (double)a.ema_decay;
    if (a.ema_num_updates) d = fmin(d, (1.0 + t) / (10.0 + t));
    omd = (float)(1.0 - d);
  }
  adam_loop<HAS_SCALE, HAS_EMA>(a.p, a.gr, a.m, a.v, a.nw, a.n, lr_t, inv, a.b1, a.b2, a.eps, a.l2, scale, a.ema,
                                omd);
}

// counters: [0] GLOBAL_STEP, [1] VALID_SAMPLES, [2] Adam t-1 (tmodel.py:282-287), [3] the
// cumulative status: every step's status word ORed in (never reset by a step), so one read
// after many steps tells whether any of them timed out.  A failed step advances nothing else.
__global__ void counters_kernel(long long* counters, const float* stats, int adam_applied, const unsigned* status,
                                const unsigned* nonfinite, long long* nonfinite_skips) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned s = status ? *status : 0u;
    if (s) {
      counters[3] |= (long long)s;
      return;
    }
    // the extended step's non-finite skip (adam_ex_kernel's decision word; nullptr = none): counted
    // apart from the chain status, which counters[3] alone keeps
    if (nonfinite && *nonfinite) {
      if (nonfinite_skips) *nonfinite_skips += 1;
      return;
    }
    counters[0] += 1;
    counters[1] += (long long)stats[1];
    counters[2] += adam_applied;
  }
}

}  // namespace

int lbwn_adam_launch2(float* params, const float* grads, float* m, float* v, long nw, long n, float lr, float b1,
                      float b2, float eps, float l2, const float* stats, const long long* counters, const unsigned* status,
                      hipStream_t st) {
  LBWN_REQUIRE(!(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v) & 15),
               "adam: parameter, gradient and slot buffers must be 16-byte aligned");
  adam_kernel<<<lbwn_grid_for(std::max(n / 4, 1L), 256, 4096), 256, 0, st>>>(params, grads, m, v, nw, n, lr, b1, b2,
                                                                             eps, l2, stats, counters, status);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_counters_launch(long long* counters, const float* stats, int adam_applied, const unsigned* status,
                         hipStream_t st, const unsigned* nonfinite, long long* nonfinite_skips) {
  counters_kernel<<<1, 64, 0, st>>>(counters, stats, adam_applied, status, nonfinite, nonfinite_skips);
  LBWN_CHECK_LAUNCH();
  return 0;
}

// The partial count of the norm pass: a function of n alone (the sums' order must not depend on the device).
int lbwn_adam_ex_nparts(long n) { return n < 1 ? 0 : lbwn_grid_for(std::max(n / 4, 1L), 256, AX_PARTS); }

// the partials as doubles, then the decision word (padded to 16 B)
long lbwn_adam_ex_ws_floats_impl(long n) { return n < 1 ? 0 : 2L * lbwn_adam_ex_nparts(n) + 4; }

int lbwn_adam_ex_launch(lbwn_adam_ex_dev a, float* ws, bool norm_pass, hipStream_t st, const unsigned** decision) {
  LBWN_REQUIRE(!(((uintptr_t)a.p | (uintptr_t)a.gr | (uintptr_t)a.m | (uintptr_t)a.v) & 15),
               "adam: parameter, gradient and slot buffers must be 16-byte aligned");
  a.part = nullptr;
  a.nparts = 0;
  a.decision = nullptr;
  if (norm_pass && a.n >= 1) {
    a.nparts = lbwn_adam_ex_nparts(a.n);
    a.part = (double*)ws;
    a.decision = (unsigned*)(ws + 2L * a.nparts);
    adam_sumsq_kernel<<<a.nparts, 256, 0, st>>>(a.p, a.gr, a.nw, a.n, a.l2, a.stats, (double*)ws);
    LBWN_CHECK_LAUNCH();
  }
  *decision = a.decision;
  const int grid = lbwn_grid_for(std::max(a.n / 4, 1L), 256, 4096);
  void (*const form[2][2])(lbwn_adam_ex_dev) = {{adam_ex_kernel<false, false>, adam_ex_kernel<false, true>},
                                                {adam_ex_kernel<true, false>, adam_ex_kernel<true, true>}};
  form[a.clip > 0.f][a.ema != nullptr]<<<grid, 256, 0, st>>>(a);   // <HAS_SCALE, HAS_EMA>
  LBWN_CHECK_LAUNCH();
  return 0;
}
