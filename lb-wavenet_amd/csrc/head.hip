// The softmax cross-entropy heads over the [M][Q] logits (tmodel.py:218-289): the training head
// (dlogits in place), the distilling / label-smoothing head and the evaluation head
// (lbwn_train_eval), with the reductions of their block partials.  One wave per position row.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

// ---- softmax cross-entropy head ------------------------------------------------------------
// One wave per position row; dlogits (unnormalised) written in place.

// wave-wide sum beside common.h's wave_max / wave_min.  The order is fixed: quads, pairs of quads,
// half rows, then rows 0 + 1 + 2 + 3.
LBWN_DEV float wave_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return ((r0 + r1) + r2) + r3;
}

// ((w0 + w1) + w2) + w3 of entry k of the block's four wave rows: the order of every block partial
template <class F, int N>
LBWN_DEV F block_fold4(const F (&p)[4][N], int k) { return ((p[0][k] + p[1][k]) + p[2][k]) + p[3][k]; }

// ---- the register form's row: QV values per lane, c = lane + 64·j ----
// Shared by the distilling and the evaluation head.  head_reg_kernel, the training step's, takes
// row_max() alone and spells the rest out: through any other of these helpers hipcc schedules it
// differently (tools/kernel_diff.py).  load_row: src[off + c], c clamped to the row's last code, so a
// padded lane (Q <= c) reads a live address; pad_row() discards its value.
template <int QV>
LBWN_DEV void load_row(float (&vn)[QV], const float* src, long off, int lane, int Q) {
#pragma unroll
  for (int j = 0; j < QV; ++j) vn[j] = src[off + min(lane + 64 * j, Q - 1)];
}
template <int QV>
LBWN_DEV void pad_row(float (&v)[QV], const float (&vn)[QV], int lane, int Q) {
#pragma unroll
  for (int j = 0; j < QV; ++j) v[j] = (lane + 64 * j < Q) ? vn[j] : -INFINITY;
}
// the row's maximum, and the first code holding it (the same first-max tie-break as a (value, index)
// reduction, in two DPP passes)
template <int QV>
LBWN_DEV float row_max(const float (&v)[QV]) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < QV; ++j) mx = fmaxf(mx, v[j]);
  return wave_max(mx);
}
template <int QV>
LBWN_DEV int lane_first(const float (&v)[QV], float mx, int lane) {   // before wave_min
  int am = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < QV; ++j)
    if (am == 0x7fffffff && v[j] == mx) am = lane + 64 * j;
  return am;
}
// e = exp(v - mx) (0 in padded lanes), and the lane's share of Σe and of the target's logit: the one
// lane holding the target has it, the rest 0 (both then go through wave_sum).  GUARD: a target
// outside [0, Q) picks 0, not a padded lane's -INF.
struct row_sums { float se, pick; };
template <int QV, bool GUARD>
LBWN_DEV row_sums row_exp_pick(const float (&v)[QV], float mx, int tgt, int lane, int Q, float (&e)[QV]) {
  float se = 0.f, pick = 0.f;
#pragma unroll
  for (int j = 0; j < QV; ++j) {
    e[j] = (lane + 64 * j < Q) ? expf(v[j] - mx) : 0.f;
    se += e[j];
    if (lane + 64 * j == tgt && (!GUARD || tgt < Q)) pick = v[j];
  }
  return {se, pick};
}

__global__ __launch_bounds__(256) void head_kernel(lbwn_head_args a) {
  __shared__ float part[4][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long M = (long)a.B * a.T;
  float s_xent = 0.f, s_valid = 0.f, s_diff = 0.f;
  for (long m = (long)blockIdx.x * 4 + w; m < M; m += (long)gridDim.x * 4) {
    float* row = a.logits + m * a.Q;
    const int t = (int)(m % a.T);
    if (t == a.T - 1) {  // logits_out[:, :-1] (tmodel.py:231): the last position has no target
      if (a.write_grad)
        for (int c = lane; c < a.Q; c += 64) row[c] = 0.f;
      continue;
    }
    const int tgt = a.q[m + 1];
    const bool valid = a.ids[m + 1] != 0;   // tmodel.py:232
    // max + first argmax
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < a.Q; c += 64) {
      const float v = row[c];
      if (v > mx) { mx = v; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(mx, o);
      const int oa = __shfl_xor(am, o);
      if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
    }
    float se = 0.f;
    for (int c = lane; c < a.Q; c += 64) se += expf(row[c] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    const float xent = lse - row[tgt];
    if (a.write_grad) {
      const float inv = 1.f / se;
      for (int c = lane; c < a.Q; c += 64) {
        float g = expf(row[c] - mx) * inv - (c == tgt ? 1.f : 0.f);
        row[c] = valid ? g : 0.f;
      }
    }
    if (lane == 0 && valid) {
      s_xent += xent;
      s_valid += 1.f;
      s_diff += fabsf((float)(tgt - am));
    }
  }
  if (lane == 0) {
    part[w][0] = s_xent;
    part[w][1] = s_valid;
    part[w][2] = s_diff;
  }
  __syncthreads();
  if (threadIdx.x < 3) a.partial[blockIdx.x * 3 + threadIdx.x] = block_fold4(part, threadIdx.x);
}

// The same head with the row held in registers (Q <= 64·QV): one coalesced load pass, exp once,
// the gradient written from registers (the generic kernel above re-reads the row three times and
// evaluates exp twice).  Lane c-order (c = lane + 64·j) and the first-max tie-break are kept, so
// argmax (avg_diff) is identical; Σe is summed per lane, then across the wave.
// With a.colpart, the block's column sums of the dlogits it wrote go to colpart[block][Q] (the
// post2 bias gradient's partials, summed by colsum_final: no second pass over the [M][Q] matrix).
template <int QV>
__global__ __launch_bounds__(256) void head_reg_kernel(lbwn_head_args a) {
  __shared__ float part[4][3];
  __shared__ float cpart[4][64 * QV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long M = (long)a.B * a.T;
  const int Q = a.Q;
  float s_xent = 0.f, s_valid = 0.f, s_diff = 0.f;
  float cs[QV];
#pragma unroll
  for (int j = 0; j < QV; ++j) cs[j] = 0.f;
  // the next row's logits and target are loaded while this row is processed (one row of HBM
  // latency in flight per wave instead of none)
  const long stride = (long)gridDim.x * 4;
  long m = (long)blockIdx.x * 4 + w;
  float vn[QV];
  int tn = 0, idn = 0;
  {
    const long mc = min(m, M - 1), mq = min(mc + 1, M - 1);
#pragma unroll
    for (int j = 0; j < QV; ++j) vn[j] = a.logits[mc * Q + min(lane + 64 * j, Q - 1)];
    tn = a.q[mq];
    idn = a.ids[mq];
  }
  for (; m < M; m += stride) {
    float* row = a.logits + m * Q;
    float v[QV];
#pragma unroll
    for (int j = 0; j < QV; ++j) v[j] = (lane + 64 * j < Q) ? vn[j] : -INFINITY;
    const int tgt = tn;
    const bool valid = idn != 0;   // tmodel.py:232
    {
      const long mc = min(m + stride, M - 1), mq = min(mc + 1, M - 1);
#pragma unroll
      for (int j = 0; j < QV; ++j) vn[j] = a.logits[mc * Q + min(lane + 64 * j, Q - 1)];
      tn = a.q[mq];
      idn = a.ids[mq];
    }
    const int t = (int)(m % a.T);
    if (t == a.T - 1) {  // logits_out[:, :-1] (tmodel.py:231): the last position has no target
      if (a.write_grad)
#pragma unroll
        for (int j = 0; j < QV; ++j)
          if (lane + 64 * j < Q) row[lane + 64 * j] = 0.f;
      continue;
    }
    const float mx = row_max(v);
    int am = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < QV; ++j)
      if (am == 0x7fffffff && v[j] == mx) am = lane + 64 * j;
    am = wave_min(am);
    float e[QV], se = 0.f, pick = 0.f;
#pragma unroll
    for (int j = 0; j < QV; ++j) {
      e[j] = (lane + 64 * j < Q) ? expf(v[j] - mx) : 0.f;
      se += e[j];
      if (lane + 64 * j == tgt) pick = v[j];
    }
    se = wave_sum(se);
    pick = wave_sum(pick);   // the one lane holding the target's logit; the rest add 0
    const float xent = (mx + logf(se)) - pick;
    if (a.write_grad) {
      const float inv = 1.f / se;
#pragma unroll
      for (int j = 0; j < QV; ++j) {
        const int c = lane + 64 * j;
        const float g = valid ? e[j] * inv - (c == tgt ? 1.f : 0.f) : 0.f;
        if (c < Q) row[c] = g;
        cs[j] += g;
      }
    }
    if (lane == 0 && valid) {
      s_xent += xent;
      s_valid += 1.f;
      s_diff += fabsf((float)(tgt - am));
    }
  }
  if (lane == 0) {
    part[w][0] = s_xent;
    part[w][1] = s_valid;
    part[w][2] = s_diff;
  }
  if (a.colpart) {
#pragma unroll
    for (int j = 0; j < QV; ++j) cpart[w][lane + 64 * j] = cs[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) a.partial[blockIdx.x * 3 + threadIdx.x] = block_fold4(part, threadIdx.x);
  if (a.colpart)
    for (int c = threadIdx.x; c < Q; c += 256)
      a.colpart[(long)blockIdx.x * Q + c] = block_fold4(cpart, c);
}

// stats[0] = Σxent, [1] = n_valid, [2] = Σ|diff|, [3] = 1/n_valid (0 if none)
// NS = 3: those; NS = 5 (the distilling head's reduce): also stats_ex[0] = Σ plain xent, [1] = Σ KL,
// [2] = [3] = 0 from partial_ex [nparts][2].  partial_ex NULL (the plain head ran): stats_ex[0] =
// stats[0], [1] = 0.  The same sums in the same order in both.
template <int NS>
LBWN_DEV void stats_reduce_body(const float* partial, const float* partial_ex, int nparts, float* stats,
                                float* stats_ex) {
  __shared__ double sh[NS][256];
  double s[NS] = {};
  for (int p = threadIdx.x; p < nparts; p += blockDim.x) {
    for (int k = 0; k < 3; ++k) s[k] += partial[p * 3 + k];
    if (NS > 3 && partial_ex)
      for (int k = 0; k < NS - 3; ++k) s[3 + k] += partial_ex[p * 2 + k];
  }
  for (int k = 0; k < NS; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < NS; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[0] = (float)sh[0][0];
    stats[1] = (float)sh[1][0];
    stats[2] = (float)sh[2][0];
    stats[3] = sh[1][0] > 0 ? (float)(1.0 / sh[1][0]) : 0.f;
    if constexpr (NS == 5)
      if (stats_ex) {
        stats_ex[0] = (float)(partial_ex ? sh[3][0] : sh[0][0]);
        stats_ex[1] = (float)sh[4][0];
        stats_ex[2] = 0.f;
        stats_ex[3] = 0.f;
      }
  }
}
__global__ void stats_reduce_kernel(const float* partial, int nparts, float* stats) {
  stats_reduce_body<3>(partial, nullptr, nparts, stats, nullptr);
}

// ---- distilling / label-smoothing head (lbwn_train_forward_ex) -------------------------
// The objective of include/lbwn.h: per scored row, with l the student's logits, u the teacher's,
//   value = (1-α)·(lse(l) - Σ q·l) + α·τ²·KL(softmax(u/τ) ‖ softmax(l/τ)),   q = (1-ε)·onehot + ε/Q,
//   dlogits = (1-α)·(softmax(l) - q) + α·τ·(softmax(l/τ) - softmax(u/τ)),
// written in place over the logits; 0 at unscored rows and at t = T-1.  The skeleton is the plain
// head's: one wave per row, the register form in lane order c = lane + 64·j, the next row fetched
// one row ahead.  The teacher's row is fetched only for a row that will be scored, so the ids run
// two rows ahead of the row in hand: the id that decides whether row m + stride is scored has to be
// in a register when that row's loads are issued.  a.teacher is NULL when α = 0: nothing of it is
// read.  Block partials: partial [nb][3] (Σ value, count, Σ|argmax - c|) as the plain head, and
// partial_ex [nb][2] (Σ plain xent, Σ KL), each ((w0+w1)+w2)+w3.
struct head_ex_row { float value, xent, kl; int am; };

// One scored row from registers.  v: the student's logits (-INF in padded lanes), u: the teacher's
// (read only with TEACH); g: the gradient out (0 in padded lanes).
template <int QV, bool TEACH>
LBWN_DEV head_ex_row head_ex_row_reg(const lbwn_head_ex_args& a, const float (&v)[QV], const float (&u)[QV], int tgt,
                                     int lane, float (&g)[QV]) {
  const int Q = a.Q;
  const float mx = row_max(v);
  float e[QV], sv = 0.f;
  head_ex_row r;
  r.am = wave_min(lane_first(v, mx, lane));
  const row_sums rs = row_exp_pick<QV, false>(v, mx, tgt, lane, Q, e);
#pragma unroll
  for (int j = 0; j < QV; ++j) sv += (lane + 64 * j < Q) ? v[j] : 0.f;
  const float se = wave_sum(rs.se), pick = wave_sum(rs.pick);
  const float lse = mx + logf(se);
  r.xent = lse - pick;
  r.kl = 0.f;
  float hard = r.xent;
  const float qoff = a.eps / (float)Q, qon = 1.f - a.eps;
  if (a.eps != 0.f) {
    sv = wave_sum(sv);
    hard = lse - (qon * pick + qoff * sv);
  }
  const float inv = 1.f / se, wh = 1.f - a.alpha;
#pragma unroll
  for (int j = 0; j < QV; ++j) {
    const int c = lane + 64 * j;
    g[j] = c < Q ? wh * (e[j] * inv - ((c == tgt ? qon : 0.f) + qoff)) : 0.f;
  }
  if (TEACH) {
    const float it = a.inv_temp;
    const float umx = row_max(u);
    // softmax(l/τ): the maximum of l/τ is mx/τ (τ > 0); at τ = 1 the exponentials above serve
    const bool t1 = a.temp == 1.f;
    float es[QV], et[QV], ses = 0.f, set = 0.f;
#pragma unroll
    for (int j = 0; j < QV; ++j) {
      const bool in = lane + 64 * j < Q;
      es[j] = t1 ? e[j] : (in ? expf((v[j] - mx) * it) : 0.f);
      et[j] = in ? expf((u[j] - umx) * it) : 0.f;
      ses += es[j];
      set += et[j];
    }
    ses = t1 ? se : wave_sum(ses);
    set = wave_sum(set);
    const float ls = logf(ses), lt = logf(set), is = 1.f / ses, itt = 1.f / set, wt = a.alpha * a.temp;
    float kl = 0.f;
#pragma unroll
    for (int j = 0; j < QV; ++j) {
      const float ps = es[j] * is, pt = et[j] * itt;
      // a padded lane (-INF in both rows) and a code whose teacher probability underflowed have
      // et = 0 and add exactly 0, never (-INF) - (-INF)
      if (et[j] > 0.f) kl += pt * (((u[j] - umx) * it - lt) - ((v[j] - mx) * it - ls));
      g[j] += wt * (ps - pt);   // padded lanes: 0 - 0
    }
    r.kl = wave_sum(kl);
  }
  r.value = wh * hard + a.alpha * (a.temp * a.temp) * r.kl;
  return r;
}

// Lane 0's five sums of each wave to LDS, then the block's fold of each to partial / partial_ex.  One
// barrier inside: the caller's own LDS stores before the call are visible after it.
LBWN_DEV void head_ex_partials(const lbwn_head_ex_args& a, float (&part)[4][5], const float (&s)[5]) {
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    const float t = block_fold4(part, k);
    if (k < 3) a.partial[blockIdx.x * 3 + k] = t;
    else a.partial_ex[blockIdx.x * 2 + (k - 3)] = t;
  }
}

template <int QV, bool TEACH>
__global__ __launch_bounds__(256) void head_ex_reg_kernel(lbwn_head_ex_args a) {
  __shared__ float part[4][5];
  __shared__ float cpart[4][64 * QV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long M = (long)a.B * a.T;
  const int Q = a.Q, T = a.T;
  float s_val = 0.f, s_valid = 0.f, s_diff = 0.f, s_xent = 0.f, s_kl = 0.f;
  float cs[QV];
#pragma unroll
  for (int j = 0; j < QV; ++j) cs[j] = 0.f;
  const long stride = (long)gridDim.x * 4;
  long m = (long)blockIdx.x * 4 + w;
  auto scored_at = [&](long r, int id) { return r < M && (int)(r % T) != T - 1 && id != 0; };
  float vn[QV], un[QV];
#pragma unroll
  for (int j = 0; j < QV; ++j) un[j] = 0.f;
  int tn = 0, idn = 0, idnn = a.ids[min(min(m, M - 1) + 1, M - 1)];
  // (student row, target, id, teacher row) of row r, fetched while its predecessor is in hand; the id
  // of the row after
  auto fetch = [&](long r) {
    const long mc = min(r, M - 1), mq = min(mc + 1, M - 1);
    load_row(vn, a.logits, mc * Q, lane, Q);
    tn = a.q[mq];
    idn = idnn;
    idnn = a.ids[min(min(r + stride, M - 1) + 1, M - 1)];
    if (TEACH && scored_at(r, idn)) load_row(un, a.teacher, r * a.ld_teacher, lane, Q);   // wave-uniform
  };
  fetch(m);
  for (; m < M; m += stride) {
    float* row = a.logits + m * Q;
    float v[QV], u[QV];
    pad_row(v, vn, lane, Q);
    pad_row(u, un, lane, Q);
    const int tgt = tn;
    const bool scored = scored_at(m, idn);
    fetch(m + stride);
    if (!scored) {   // t = T-1 (no target, tmodel.py:231) or a masked target (tmodel.py:232): dlogits = 0
#pragma unroll
      for (int j = 0; j < QV; ++j)
        if (lane + 64 * j < Q) row[lane + 64 * j] = 0.f;
      continue;
    }
    float g[QV];
    const head_ex_row r = head_ex_row_reg<QV, TEACH>(a, v, u, tgt, lane, g);
#pragma unroll
    for (int j = 0; j < QV; ++j) {
      if (lane + 64 * j < Q) row[lane + 64 * j] = g[j];
      cs[j] += g[j];
    }
    if (lane == 0) {
      s_val += r.value;
      s_valid += 1.f;
      s_diff += fabsf((float)(tgt - r.am));
      s_xent += r.xent;
      s_kl += r.kl;
    }
  }
  if (a.colpart) {
#pragma unroll
    for (int j = 0; j < QV; ++j) cpart[w][lane + 64 * j] = cs[j];
  }
  head_ex_partials(a, part, {s_val, s_valid, s_diff, s_xent, s_kl});
  if (a.colpart)
    for (int c = threadIdx.x; c < Q; c += 256)
      a.colpart[(long)blockIdx.x * Q + c] = block_fold4(cpart, c);
}

// Any width (Q > 512): the rows are walked in memory, three passes (maxima; sums; gradient and KL).
template <bool TEACH>
__global__ __launch_bounds__(256) void head_ex_kernel(lbwn_head_ex_args a) {
  __shared__ float part[4][5];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long M = (long)a.B * a.T;
  const int Q = a.Q;
  float s_val = 0.f, s_valid = 0.f, s_diff = 0.f, s_xent = 0.f, s_kl = 0.f;
  for (long m = (long)blockIdx.x * 4 + w; m < M; m += (long)gridDim.x * 4) {
    float* row = a.logits + m * Q;
    const int t = (int)(m % a.T);
    const bool scored = t != a.T - 1 && a.ids[min(m + 1, M - 1)] != 0;
    if (!scored) {
      for (int c = lane; c < Q; c += 64) row[c] = 0.f;
      continue;
    }
    const int tgt = a.q[m + 1];
    const float* trow = TEACH ? a.teacher + m * a.ld_teacher : nullptr;
    float mx = -INFINITY, umx = -INFINITY;
    for (int c = lane; c < Q; c += 64) {
      mx = fmaxf(mx, row[c]);
      if (TEACH) umx = fmaxf(umx, trow[c]);
    }
    mx = wave_max(mx);
    if (TEACH) umx = wave_max(umx);
    const bool t1 = a.temp == 1.f;
    const float it = a.inv_temp;
    int am = 0x7fffffff;
    float se = 0.f, pick = 0.f, sv = 0.f, ses = 0.f, set = 0.f;
    for (int c = lane; c < Q; c += 64) {
      const float x = row[c];
      if (am == 0x7fffffff && x == mx) am = c;
      se += expf(x - mx);
      sv += x;
      if (c == tgt) pick = x;
      if (TEACH) {
        if (!t1) ses += expf((x - mx) * it);
        set += expf((trow[c] - umx) * it);
      }
    }
    am = wave_min(am);
    se = wave_sum(se);
    pick = wave_sum(pick);
    const float lse = mx + logf(se);
    const float xent = lse - pick;
    float hard = xent;
    const float qoff = a.eps / (float)Q, qon = 1.f - a.eps;
    if (a.eps != 0.f) {
      sv = wave_sum(sv);
      hard = lse - (qon * pick + qoff * sv);
    }
    float ls = 0.f, lt = 0.f, is = 0.f, itt = 0.f;
    if (TEACH) {
      ses = t1 ? se : wave_sum(ses);
      set = wave_sum(set);
      ls = logf(ses); lt = logf(set); is = 1.f / ses; itt = 1.f / set;
    }
    const float inv = 1.f / se, wh = 1.f - a.alpha, wt = a.alpha * a.temp;
    float kl = 0.f;
    for (int c = lane; c < Q; c += 64) {
      const float x = row[c];
      float g = wh != 0.f ? wh * (expf(x - mx) * inv - ((c == tgt ? qon : 0.f) + qoff)) : 0.f;
      if (TEACH) {
        const float ds = (x - mx) * it, dt = (trow[c] - umx) * it;
        const float es = expf(ds), et = expf(dt);
        if (et > 0.f) kl += (et * itt) * ((dt - lt) - (ds - ls));
        g += wt * (es * is - et * itt);
      }
      row[c] = g;
    }
    if (TEACH) kl = wave_sum(kl);
    if (lane == 0) {
      s_val += wh * hard + a.alpha * (a.temp * a.temp) * kl;
      s_valid += 1.f;
      s_diff += fabsf((float)(tgt - am));
      s_xent += xent;
      s_kl += kl;
    }
  }
  head_ex_partials(a, part, {s_val, s_valid, s_diff, s_xent, s_kl});
}

// stats and stats_ex: stats_reduce_body<5>
__global__ void stats_reduce_ex_kernel(const float* partial, const float* partial_ex, int nparts, float* stats,
                                       float* stats_ex) {
  stats_reduce_body<5>(partial, partial_ex, nparts, stats, stats_ex);
}

// ---- evaluation head (lbwn_train_eval) -----------------------------------------------------------
// The training head's xent without its gradient: the logits are read and never written.  One wave
// per row, the row in registers for QV > 0 (Q <= 64·QV, head_reg_kernel's lane order c = lane +
// 64·j, so Σe, the first-max argmax and the value are that kernel's bits); QV = 0 walks a row of
// any width three times.  The target's logit is picked by lane compare in both forms, so a code
// outside [0, Q) reads nothing and picks 0 (the register form's padded lanes, Q <= c < 64·QV, are
// excluded by the compare with Q): its value is the row's lse.  Each wave adds its rows' values in
// double in row order; a block stores ((w0 + w1) + w2) + w3 of (Σnll, count, Σ|argmax - c|, hits).
// The grid is lbwn_eval_nblocks(M), a function of M alone: the same partials in every run and on
// every device.
constexpr int EV_MAXBLK = 2048;
constexpr int EV_CHUNK = 256;   // positions per block of eval_voice_kernel

template <int QV>
__global__ __launch_bounds__(256) void eval_head_kernel(lbwn_eval_head_args a) {
  __shared__ double part[4][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long M = (long)a.B * a.T;
  const int Q = a.Q;
  double s_nll = 0.0, s_cnt = 0.0, s_diff = 0.0, s_hit = 0.0;
  const long stride = (long)gridDim.x * 4;
  long m = (long)blockIdx.x * 4 + w;
  constexpr int NV = QV > 0 ? QV : 1;
  float vn[NV];
  int tn = 0, idn = 0;
  auto fetch = [&](long r) {   // row r's logits, target and id (r clamped to the last row)
    const long mc = min(r, M - 1), mq = min(mc + 1, M - 1);
    if (QV > 0) load_row(vn, a.logits, mc * Q, lane, Q);
    tn = a.q[mq];
    idn = a.ids[mq];
  };
  fetch(m);   // the first row; then one row ahead, as in head_reg_kernel
  for (; m < M; m += stride) {
    const float* row = a.logits + m * Q;
    float v[NV];
    if (QV > 0) pad_row(v, vn, lane, Q);
    const int tgt = tn;
    const int vid = idn;
    fetch(m + stride);
    const int b = (int)(m / a.T), t = (int)(m - (long)b * a.T);
    const bool scored = t != a.T - 1 && vid != 0;   // tmodel.py:231-232
    float nll = 0.f;
    if (scored) {   // wave-uniform
      float mx = -INFINITY, se = 0.f, pick = 0.f;
      int am = 0x7fffffff;
      if (QV > 0) {
        mx = row_max(v);
        am = lane_first(v, mx, lane);
        float e[NV];
        const row_sums r = row_exp_pick<NV, true>(v, mx, tgt, lane, Q, e);
        se = r.se, pick = r.pick;
      } else {
        for (int c = lane; c < Q; c += 64) mx = fmaxf(mx, row[c]);
        mx = wave_max(mx);
        for (int c = lane; c < Q; c += 64) {
          const float x = row[c];
          if (am == 0x7fffffff && x == mx) am = c;
          se += expf(x - mx);
          if (c == tgt) pick = x;
        }
      }
      am = wave_min(am);
      se = wave_sum(se);
      pick = wave_sum(pick);   // the one lane holding the target's logit; the rest add 0
      nll = (mx + logf(se)) - pick;
      s_nll += (double)nll;
      s_cnt += 1.0;
      s_diff += (double)abs(tgt - am);
      s_hit += am == tgt ? 1.0 : 0.0;
    }
    if (lane == 0) {
      if (a.nll) a.nll[(long)b * a.ld_nll + t] = nll;
      if (a.rowv) a.rowv[m] = nll;
    }
  }
  if (lane == 0) {
    part[w][0] = s_nll;
    part[w][1] = s_cnt;
    part[w][2] = s_diff;
    part[w][3] = s_hit;
  }
  __syncthreads();
  if (threadIdx.x < 4) a.partial[(long)blockIdx.x * 4 + threadIdx.x] = block_fold4(part, threadIdx.x);
}

// Per-voice partials: block c takes positions [256c, 256c + 256) into LDS as (bin, value) pairs
// (bin -1: not scored), then thread v walks the 256 pairs in position order and adds those of bin
// v in double: no atomics on values, an order fixed by the position.  Only the bins between the
// chunk's smallest and largest one are walked (a chunk lies in one or two files, so mostly one
// bin); the rest store zeros.  vpart is [nchunks][n_bins][2] (Σnll, count).
__global__ __launch_bounds__(256) void eval_voice_kernel(const float* __restrict__ val, long ldv, const int* __restrict__ ids,
                                                         int B, int T, int n_bins, double* __restrict__ vpart) {
  __shared__ int sbin[EV_CHUNK];
  __shared__ float sval[EV_CHUNK];
  __shared__ int lo, hi;
  if (threadIdx.x == 0) { lo = 0x7fffffff; hi = -1; }
  __syncthreads();
  const long M = (long)B * T, m = (long)blockIdx.x * EV_CHUNK + threadIdx.x;
  int bin = -1;
  float x = 0.f;
  if (m < M) {
    const int b = (int)(m / T), t = (int)(m - (long)b * T);
    if (t != T - 1) {
      const int id = ids[m + 1];
      if (id != 0) {
        bin = (unsigned)id < (unsigned)n_bins ? id : 0;
        x = val[(long)b * ldv + t];
      }
    }
  }
  sbin[threadIdx.x] = bin;
  sval[threadIdx.x] = x;
  if (bin >= 0) {   // integer min / max: the result does not depend on the order
    atomicMin(&lo, bin);
    atomicMax(&hi, bin);
  }
  __syncthreads();
  const int l0 = lo, h0 = hi;
  double* out = vpart + (long)blockIdx.x * n_bins * 2;
  for (int v = threadIdx.x; v < n_bins; v += 256) {
    double s = 0.0, n = 0.0;
    if (v >= l0 && v <= h0) {
      for (int i = 0; i < EV_CHUNK; ++i)
        if (sbin[i] == v) { s += (double)sval[i]; n += 1.0; }
    }
    out[2 * v] = s;
    out[2 * v + 1] = n;
  }
}

// Fold: block 0 adds the head's block partials into acc (thread t sums partials t, t + 256, ... in
// order, then the fixed LDS tree) and ORs the plan's status word into the caller's; blocks 1.. take
// one bin per thread and add the chunks' partials in chunk order into by_voice.
__global__ __launch_bounds__(256) void eval_fold_kernel(const double* __restrict__ partial, int nparts, double* acc,
                                                        const double* __restrict__ vpart, int nchunks, int n_bins,
                                                        double* by_voice, const unsigned* plan_status,
                                                        unsigned* status) {
  __shared__ double sh[256];
  if (blockIdx.x == 0) {
    for (int k = 0; k < 4; ++k) {   // uniform
      double s = 0.0;
      for (int p = threadIdx.x; p < nparts; p += 256) s += partial[(long)p * 4 + k];
      const double tot = block_sum256(s, sh);
      if (threadIdx.x == 0) acc[k] += tot;
      __syncthreads();
    }
    if (threadIdx.x == 0 && status) *status |= *plan_status;
    return;
  }
  const int v = (blockIdx.x - 1) * 256 + threadIdx.x;
  if (v >= n_bins) return;
  double s = 0.0, n = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    s += vpart[((long)c * n_bins + v) * 2];
    n += vpart[((long)c * n_bins + v) * 2 + 1];
  }
  by_voice[2 * v] += s;
  by_voice[2 * v + 1] += n;
}

// The width ladder of the three heads: the row in 4 or in 8 registers per lane (Q <= 256, <= 512),
// else the kernel that walks a row of any width in memory.  nb blocks, reported in *nb_out (nullable).
template <class A>
int launch_by_width(const A& a, int nb, int* nb_out, hipStream_t st, void (*reg4)(A), void (*reg8)(A),
                    void (*any)(A)) {
  (a.Q <= 256 ? reg4 : a.Q <= 512 ? reg8 : any)<<<nb, 256, 0, st>>>(a);
  LBWN_CHECK_LAUNCH();
  if (nb_out) *nb_out = nb;
  return 0;
}

}  // namespace

int lbwn_head_launch(const lbwn_head_args& a, int* nblocks_out, hipStream_t st) {
  const long M = (long)a.B * a.T;
  LBWN_REQUIRE(!a.colpart || a.Q <= 512, "head: column partials need Q <= 512");
  const int nb = lbwn_head_nblocks(M, a.colpart != nullptr);
  return launch_by_width(a, nb, nblocks_out, st, head_reg_kernel<4>, head_reg_kernel<8>, head_kernel);
}
// with column partials: at most ceil(M/32) blocks, so colpart fits the colsum workspace
int lbwn_head_nblocks(long M, bool colpart) {
  return (int)(colpart ? std::min<long>((M + 31) / 32, 1024) : std::min<long>((M + 3) / 4, 2048));
}

int lbwn_stats_reduce_launch(const float* partial, int nparts, float* stats, hipStream_t st) {
  stats_reduce_kernel<<<1, 256, 0, st>>>(partial, nparts, stats);
  LBWN_CHECK_LAUNCH();
  return 0;
}

// the distilling / smoothing head: the plain head's grid; a.teacher NULL (α = 0) selects the forms
// that read no teacher
int lbwn_head_ex_launch(const lbwn_head_ex_args& a, int* nblocks_out, hipStream_t st) {
  const long M = (long)a.B * a.T;
  LBWN_REQUIRE(!a.colpart || a.Q <= 512, "head_ex: column partials need Q <= 512");
  LBWN_REQUIRE(a.teacher || a.alpha == 0.f, "head_ex: alpha > 0 needs the teacher's logits");
  const int nb = lbwn_head_nblocks(M, a.colpart != nullptr);
  if (a.teacher)
    return launch_by_width(a, nb, nblocks_out, st, head_ex_reg_kernel<4, true>, head_ex_reg_kernel<8, true>,
                           head_ex_kernel<true>);
  return launch_by_width(a, nb, nblocks_out, st, head_ex_reg_kernel<4, false>, head_ex_reg_kernel<8, false>,
                         head_ex_kernel<false>);
}

int lbwn_stats_reduce_ex_launch(const float* partial, const float* partial_ex, int nparts, float* stats,
                                float* stats_ex, hipStream_t st) {
  stats_reduce_ex_kernel<<<1, 256, 0, st>>>(partial, partial_ex, nparts, stats, stats_ex);
  LBWN_CHECK_LAUNCH();
  return 0;
}

// ---- lbwn_train_eval's head: row kernel, per-voice partials, fold ----
int lbwn_eval_nblocks(long M) { return (int)std::min<long>((M + 3) / 4, EV_MAXBLK); }
int lbwn_eval_nchunks(long M) { return (int)((M + EV_CHUNK - 1) / EV_CHUNK); }

// scratch: head partials double [nblocks][4] | voice partials double [nchunks][n_bins][2] | row values
// float [M] (the last two only with bins), each part rounded up to 256 bytes
static size_t ev_up(size_t b) { return (b + 255) / 256 * 256; }
size_t lbwn_eval_scratch_bytes(long M, int n_bins) {
  size_t n = ev_up(sizeof(double) * 4 * (size_t)lbwn_eval_nblocks(M));
  if (n_bins > 0)
    n += ev_up(sizeof(double) * 2 * (size_t)lbwn_eval_nchunks(M) * (size_t)n_bins) + ev_up(sizeof(float) * (size_t)M);
  return n;
}

int lbwn_eval_head_launch(const float* logits, const int* q, const int* ids, int B, int T, int Q, float* nll,
                          long ld_nll, double* acc, double* by_voice, int n_bins, const unsigned* plan_status,
                          unsigned* status, void* scratch, hipStream_t st) {
  const long M = (long)B * T;
  char* sc = static_cast<char*>(scratch);
  lbwn_eval_head_args a;
  a.logits = logits; a.q = q; a.ids = ids; a.B = B; a.T = T; a.Q = Q; a.nll = nll; a.ld_nll = ld_nll;
  a.partial = reinterpret_cast<double*>(sc);
  const int nb = lbwn_eval_nblocks(M), nch = lbwn_eval_nchunks(M);
  double* vpart = nullptr;
  a.rowv = nullptr;
  if (by_voice) {
    vpart = reinterpret_cast<double*>(sc + ev_up(sizeof(double) * 4 * (size_t)nb));
    if (!nll)   // the voice pass reads the values back: from the caller's nll, else from the scratch rows
      a.rowv = reinterpret_cast<float*>(sc + ev_up(sizeof(double) * 4 * (size_t)nb) +
                                        ev_up(sizeof(double) * 2 * (size_t)nch * (size_t)n_bins));
  }
  if (int e = launch_by_width(a, nb, nullptr, st, eval_head_kernel<4>, eval_head_kernel<8>, eval_head_kernel<0>))
    return e;
  if (by_voice) {
    eval_voice_kernel<<<nch, 256, 0, st>>>(nll ? nll : a.rowv, nll ? ld_nll : (long)T, ids, B, T, n_bins, vpart);
    LBWN_CHECK_LAUNCH();
  }
  eval_fold_kernel<<<1 + (by_voice ? (n_bins + 255) / 256 : 0), 256, 0, st>>>(a.partial, nb, acc, vpart, nch, n_bins,
                                                                            by_voice, plan_status, status);
  LBWN_CHECK_LAUNCH();
  return 0;
}
