// Both execution forms draw with the same wave-level inverse-CDF code: u = hash(seed, stream, step), µ-law
// decode, next input = teacher[t] or the draw (imodel.py:167-187, :260-269).  A sampling triple other
// than (1, 0, 1) (lbwn_gen_set_sampling: temperature, top_k, top_p) selects the FILT instantiations,
// whose draw filters the codes first (draw_core_filt); the neutral triple runs the plain ones.
// gen_prefill.hip takes mu_decode_q and wave_sum from here.
#pragma once
#include "gen_common.h"

namespace {

// ---- the draw (imodel.py:167-187, :260-269) ----------------------------------------------
// Inverse-CDF draw of softmax(logits): the first k with cumsum(e)[k] > u·Σe, e = exp(logits -
// max), u = hash(seed, stream, step) (oracle/wavenet_ref.py sample_from_logits restates the
// transform).  Wave-level only — lane = a contiguous run of ceil(Q/64) codes, shuffles, no
// workgroup barrier — so every wave that calls it with the same logits draws the same code.
struct DrawK {
  const float* part; int parts;   // logits = Σ part[p][b][:] + bias (per-step path)
  unsigned ring;                  // ring plans: R, column = local step mod R (0: none); in the struct's padding, so
  const float* bias;              // no other member moves
  int Q, B;
  float* logits; int* samples; float* wav;
  long long max_steps;   // columns of samples / wav, by the absolute step (0 on a ring plan: ring says where)
  const int* teacher; long long n_teacher; unsigned long long seed; int* code;
  float temperature; int top_k; float top_p;   // lbwn_gen_set_sampling; read by the FILT forms only
  // sessions (lbwn_gen_begin): [B][4] int64 {base, key, rows, 0}, or null: key = stream, base = 0
  const long long* sess;
};

// inclusive prefix sum over the 64 lanes: Hillis-Steele within rows (row_shr 1, 2, 4, 8), then
// row 15's total into rows 1, 3 and lane 31's into rows 2, 3
LBWN_DEV float wave_scan(float x) {
  x += dpp_f<0x111>(x);
  x += dpp_f<0x112>(x);
  x += dpp_f<0x114>(x);
  x += dpp_f<0x118>(x);
  x += dpp_f<0x142, 0xA>(x);
  x += dpp_f<0x143, 0xC>(x);
  return x;
}
// wave-wide sum, the same value on every lane (each step adds a lane's partner, so both sides of a
// pair form the same sum): the filtered draw's masses.  Rows added as (r0+r1)+(r2+r3): not head.hip's
LBWN_DEV float wave_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
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

// µ-law decode of one code (ops.py:12-20)
LBWN_DEV float mu_decode_q(int q, int Q) {
  const float mu = (float)(Q - 1), inv = 1.f / mu;
  const float aa = (2.f * (float)q - 1.f) * inv - 1.f;
  const float sg = aa > 0.f ? 1.f : (aa < 0.f ? -1.f : 0.f);
  return sg * (powf(1.f + mu, fabsf(aa)) - 1.f) * inv;
}

// the end of both draws: the next input code of stream b after step t (the teacher's or the draw);
// the writing wave's lane 0 stores the sample, its µ-law decode and code[b].  RING = false leaves out the ring
// plans' store (the persistent kernel's instantiations for plans without a ring).
template <bool RING>
LBWN_DEV int draw_commit(const DrawK& a, int b, long long t, int found, bool write, bool decode) {
  const int next = (t < a.n_teacher) ? a.teacher[t] : found;   // imodel.py:260-269
  if (write && (threadIdx.x & 63) == 0) {
    if (t < a.max_steps) {
      a.samples[(long)b * a.max_steps + t] = found;
      if (decode) a.wav[(long)b * a.max_steps + t] = mu_decode_q(found, a.Q);
    } else if (RING && a.ring) {   // ring plan: every step stored
      const long c = (long)b * a.ring + ring_col(t - (a.sess ? a.sess[4 * b] : 0LL), a.ring);
      a.samples[c] = found;
      if (decode) a.wav[c] = mu_decode_q(found, a.Q);
    }
    a.code[b] = next;
  }
  return next;
}

// v[j] = logit of code lane·per + j.  Returns draw_commit's next input code; the writing wave also
// stores the logits.
template <int MP, bool RING = true>
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
  return draw_commit<RING>(a, b, t, found, write, decode);
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
template <int MP, bool RING = true>
LBWN_DEV int draw_core_filt(float (&v)[MP], const DrawK& a, int b, long long t, bool write, bool decode = true) {
  const int lane = threadIdx.x & 63, Q = a.Q;
  const int per = (Q + 63) >> 6, c0 = lane * per;
  uint64_t skey = (uint64_t)b, sstep = (uint64_t)t;   // the draw's key, as in draw_core
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
  return draw_commit<RING>(a, b, t, found, write, decode);
}

// the draw's arguments of a run in either form (part / parts: the per-step form sets them)
DrawK draw_args(const lbwn_gen_plan* p, const lbwn_params* P, void* ws) {
  DrawK d;
  memset(&d, 0, sizeof(d));
  d.Q = p->Q; d.B = p->B; d.bias = P->post2_b;
  d.logits = gat<float>(ws, p->oLOG); d.samples = gat<int>(ws, p->oSAMP); d.wav = gat<float>(ws, p->oWAV);
  d.max_steps = p->ring ? 0 : p->max_steps; d.ring = (unsigned)p->ring; d.teacher = gat<int>(ws, p->oTEACH); d.n_teacher = p->n_teacher; d.seed = p->seed;
  d.code = gat<int>(ws, p->oCODE);
  d.temperature = p->temperature; d.top_k = p->top_k; d.top_p = p->top_p;
  d.sess = p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr;
  return d;
}

}  // namespace
