// extern "C" surface of liblbwn.so (declared in include/lbwn.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lbwn.h"
#include "common.h"
#include "kernels.h"

static thread_local char g_err[1024] = "";

void lbwn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

const char* lbwn_last_error(void) { return g_err; }
int lbwn_abi_version(void) { return LBWN_ABI_VERSION; }

int lbwn_adam_tf1(float* params, const float* grads, float* m, float* v, int64_t n_weights, int64_t n_total,
                  float lr, float beta1, float beta2, float eps, float l2_factor, const float* stats,
                  int64_t* counters, const uint32_t* step_status, void* stream) {
  LBWN_REQUIRE(params && grads && m && v && counters, "adam_tf1: null argument");
  LBWN_REQUIRE(n_weights >= 0 && n_weights <= n_total, "adam_tf1: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const unsigned* ss = (const unsigned*)step_status;
  int e = lbwn_adam_launch2(params, grads, m, v, (long)n_weights, (long)n_total, lr, beta1, beta2, eps, l2_factor,
                            stats, (const long long*)counters, ss, st);
  if (e) return e;
  if (stats) return lbwn_counters_launch((long long*)counters, stats, 1, ss, st);
  return 0;
}

int64_t lbwn_adam_ex_ws_floats(int64_t n_total) { return (int64_t)lbwn_adam_ex_ws_floats_impl((long)n_total); }

int lbwn_adam_ex(const lbwn_adam_ex_args* a, void* stream) {
  LBWN_REQUIRE(a != nullptr, "adam_ex: null argument struct");
  LBWN_REQUIRE(a->struct_size == sizeof(lbwn_adam_ex_args), "adam_ex: struct_size %zu != %zu (another ABI?)",
               a->struct_size, sizeof(lbwn_adam_ex_args));
  LBWN_REQUIRE(a->params && a->grads && a->m && a->v && a->counters, "adam_ex: null argument");
  LBWN_REQUIRE(a->n_weights >= 0 && a->n_weights <= a->n_total, "adam_ex: bad sizes");
  LBWN_REQUIRE(a->clip_norm >= 0.f && a->clip_norm <= 3.402823466e38f, "adam_ex: clip_norm must be 0 (off) or finite and > 0");
  LBWN_REQUIRE(a->ema_decay >= 0.f && a->ema_decay < 1.f, "adam_ex: ema_decay must be 0 (off) or in (0, 1)");
  const bool has_ema = a->ema_decay > 0.f;
  LBWN_REQUIRE(!has_ema || (a->ema && !((uintptr_t)a->ema & 15)),
               "adam_ex: ema must be a 16-byte aligned [n_total] buffer when ema_decay > 0");
  LBWN_REQUIRE(a->lr_warmup_steps >= 0, "adam_ex: lr_warmup_steps must be >= 0");
  LBWN_REQUIRE(a->lr_decay_steps >= 0, "adam_ex: lr_decay_steps must be >= 0");
  LBWN_REQUIRE(a->lr_decay_steps == 0 || (a->lr_decay_rate > 0.f && a->lr_decay_rate <= 1.f),
               "adam_ex: lr_decay_rate must be in (0, 1] when lr_decay_steps > 0");
  const bool norm_pass = a->clip_norm > 0.f || a->skip_nonfinite || a->info != nullptr;
  LBWN_REQUIRE(!norm_pass || (a->ws && !((uintptr_t)a->ws & 15)),
               "adam_ex: ws must be a 16-byte aligned buffer of lbwn_adam_ex_ws_floats(n_total) floats when "
               "clip_norm, skip_nonfinite or info asks for the norm");
  hipStream_t st = (hipStream_t)stream;
  const unsigned* ss = (const unsigned*)a->step_status;
  const bool sched = a->lr_warmup_steps > 0 || a->lr_decay_steps > 0;
  if (!norm_pass && !has_ema && !sched) {   // every option neutral: the launches of lbwn_adam_tf1
    int e = lbwn_adam_launch2(a->params, a->grads, a->m, a->v, (long)a->n_weights, (long)a->n_total, a->lr, a->beta1,
                              a->beta2, a->eps, a->l2_factor, a->stats, (const long long*)a->counters, ss, st);
    if (e) return e;
    if (a->stats) return lbwn_counters_launch((long long*)a->counters, a->stats, 1, ss, st);
    return 0;
  }
  lbwn_adam_ex_dev d;
  memset(&d, 0, sizeof(d));
  d.p = a->params; d.gr = a->grads; d.m = a->m; d.v = a->v;
  d.nw = (long)a->n_weights; d.n = (long)a->n_total;
  d.lr = a->lr; d.b1 = a->beta1; d.b2 = a->beta2; d.eps = a->eps; d.l2 = a->l2_factor;
  d.stats = a->stats; d.counters = (const long long*)a->counters; d.status = ss;
  d.clip = a->clip_norm; d.skip_nonfinite = a->skip_nonfinite ? 1 : 0;
  d.ema_decay = a->ema_decay; d.ema_num_updates = a->ema_num_updates ? 1 : 0; d.ema = has_ema ? a->ema : nullptr;
  d.warmup = (long)a->lr_warmup_steps; d.decay_steps = (long)a->lr_decay_steps;
  d.decay_rate = a->lr_decay_rate; d.staircase = a->lr_decay_staircase ? 1 : 0;
  d.info = a->info;
  const unsigned* decision = nullptr;
  int e = lbwn_adam_ex_launch(d, a->ws, norm_pass, st, &decision);
  if (e) return e;
  if (a->stats)
    return lbwn_counters_launch((long long*)a->counters, a->stats, 1, ss, st, decision,
                                (long long*)a->nonfinite_skips);
  return 0;
}

int lbwn_mulaw_encode(const float* x, int* q, int64_t n, int n_quanta, int tf32, void* stream) {
  LBWN_REQUIRE(n >= 0 && n_quanta >= 2, "mulaw_encode: bad arguments");
  if (n == 0) return 0;
  return lbwn_mulaw_encode_launch(x, q, (long)n, n_quanta, tf32, (hipStream_t)stream);
}

int lbwn_mulaw_decode(const int* q, float* x, int64_t n, int n_quanta, void* stream) {
  LBWN_REQUIRE(n >= 0 && n_quanta >= 2, "mulaw_decode: bad arguments");
  if (n == 0) return 0;
  return lbwn_mulaw_decode_launch(q, x, (long)n, n_quanta, (hipStream_t)stream);
}

int lbwn_gemm_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb, int b_kcontig, float* C,
                  int64_t ldc, int M, int N, int K, const float* bias, int relu_a, int relu_out, const float* mask,
                  int64_t ldm, int accumulate, int split_k, float* slab_ws, void* stream) {
  lbwn_gemm_args g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = (long)lda; g.B = B; g.ldb = (long)ldb; g.C = C; g.ldc = (long)ldc;
  g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu_a = relu_a; g.relu_out = relu_out;
  g.mask = mask; g.ldm = (long)ldm; g.accumulate = accumulate;
  return lbwn_gemm_launch(g, a_kcontig, b_kcontig, split_k, slab_ws, (hipStream_t)stream);
}

int lbwn_gemm_f32_presplit(const float* A, int64_t lda, int a_kcontig, const uint16_t* b3, int N, const float* B,
                           int64_t ldb, int b_kcontig, float* C, int64_t ldc, int M, int K, const float* bias,
                           int relu_a, int relu_out, const float* mask, int64_t ldm, int accumulate, void* stream) {
  LBWN_REQUIRE(b3 != nullptr, "gemm_f32_presplit: b3 is null");
  // the x3r/x3q kernels read b3 with 16-byte loads over lbwn_split_planes_elems(N, K) elements
  LBWN_REQUIRE(((uintptr_t)b3 & 15) == 0, "gemm_f32_presplit: b3 must be 16-byte aligned");
  lbwn_gemm_args g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = (long)lda; g.B = B; g.ldb = (long)ldb; g.C = C; g.ldc = (long)ldc;
  g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu_a = relu_a; g.relu_out = relu_out;
  g.mask = mask; g.ldm = (long)ldm; g.accumulate = accumulate; g.b3 = (const unsigned short*)b3;
  return lbwn_gemm_launch(g, a_kcontig, b_kcontig, 1, nullptr, (hipStream_t)stream);
}

int64_t lbwn_split_planes_elems_abi(int rows, int K) { return (int64_t)lbwn_split_planes_elems(rows, K); }

int lbwn_split_planes(const float* W, int64_t ldw, int rows, int K, int trans, uint16_t* out, void* stream) {
  const long l = (long)ldw;
  unsigned short* o = (unsigned short*)out;
  return lbwn_split_planes_launch(1, &W, &l, &rows, &K, &trans, &o, (hipStream_t)stream);
}

int lbwn_gemm_ex(const lbwn_gemm_ex_args* a, void* stream) {
  LBWN_REQUIRE(a != nullptr, "gemm_ex: null argument struct");
  LBWN_REQUIRE(a->struct_size == sizeof(lbwn_gemm_ex_args), "gemm_ex: struct_size %zu != %zu (another ABI?)",
               a->struct_size, sizeof(lbwn_gemm_ex_args));
  LBWN_REQUIRE(a->A && a->B && a->C, "gemm_ex: A, B or C is null");
  lbwn_gemm_args g;
  memset(&g, 0, sizeof(g));
  g.A = a->A; g.lda = (long)a->lda; g.B = a->B; g.ldb = (long)a->ldb; g.C = a->C; g.ldc = (long)a->ldc;
  g.M = a->M; g.N = a->N; g.K = a->K; g.bias = a->bias; g.mask = a->mask; g.ldm = (long)a->ldm;
  g.relu_a = a->relu_a; g.relu_out = a->relu_out; g.accumulate = a->accumulate;
  g.b3 = (const unsigned short*)a->b3; g.colpart = a->colpart; g.step_advance = (long long*)a->step_advance;
  g.c_chain_ls = (long)a->c_chain_ls; g.xcd2d = a->xcd2d;
  g.a_kstride = (long)a->a_kstride; g.b_gstride = (long)a->b_gstride; g.a_gstride = (long)a->a_gstride;
  g.row_exact = a->row_exact;
  g.mbits_out = (unsigned long long*)a->mbits_out; g.mbits = (const unsigned long long*)a->mbits;
  g.row_live = a->row_live; g.k_live = a->k_live; g.nk_live = a->nk_live; g.k_pre = a->k_pre;
  g.splits_deferred = a->splits_deferred;
  return lbwn_gemm_launch(g, a->a_kcontig, a->b_kcontig, a->split_k, a->slab_ws, (hipStream_t)stream);
}

const char* lbwn_gemm_last_form(void) { return lbwn_gemm_last_form_impl(); }
int64_t lbwn_gemm_mbits_words_abi(int M, int N) { return (int64_t)lbwn_gemm_mbits_words(M, N); }
int lbwn_colpart_parts_abi(int M) { return lbwn_colpart_parts(M); }
int lbwn_gemm_form_query(int which, int M, int N, int K, int a_kcontig, int presplit, int row_exact, int colpart) {
  switch (which) {
    case 0: return lbwn_gemm_x3q8_form(M, N, K, a_kcontig, presplit, row_exact, colpart) ? 1 : 0;
    case 1: return lbwn_gemm_row_live_form(M, N, K, a_kcontig, presplit, row_exact, colpart) ? 1 : 0;
    case 2: return lbwn_gemm_k_live_form(M, N, K) ? 1 : 0;
  }
  lbwn_set_error("gemm_form_query: which must be 0 (x3q<8>), 1 (row_live) or 2 (k_live), got %d", which);
  return -1;
}

// ---- the conditioning kernels on their own inputs (cond.hip) ----
int lbwn_lc_upsample_fused_ok(int nup, const int* strides, int Li, int Lo) {
  if (!strides) return 0;
  return lbwn_lc_up_fused_ok(nup, strides, Li, Lo) ? 1 : 0;
}

int64_t lbwn_lc_upsample_part_floats(int nup, const int* strides, int Li, int Lo, int frames) {
  if (!strides || nup < 1 || nup > 8 || frames < 1) return 0;
  int64_t tot = 0;
  for (int i = 0; i < nup; ++i) tot += (int64_t)strides[i] * Lo * (i ? Lo : Li);
  return tot * frames;
}

int lbwn_lc_upsample_forward(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                             const float* const* F, float* const* act, void* stream) {
  LBWN_REQUIRE(strides && mel && F && act, "lc_upsample_forward: null argument");
  LBWN_REQUIRE(frames >= 1, "lc_upsample_forward: frames must be >= 1");
  LBWN_REQUIRE(lbwn_lc_up_fused_ok(nup, strides, Li, Lo),
               "lc_upsample_forward: shape outside the fused kernel's envelope");
  LBWN_REQUIRE(((uintptr_t)mel & 15) == 0, "lc_upsample_forward: mel must be 16-byte aligned");
  for (int i = 0; i < nup; ++i) {
    LBWN_REQUIRE(F[i] && act[i], "lc_upsample_forward: F[%d] or act[%d] is null", i, i);
    LBWN_REQUIRE((((uintptr_t)F[i] | (uintptr_t)act[i]) & 15) == 0,
                 "lc_upsample_forward: F[%d], act[%d] must be 16-byte aligned", i, i);
  }
  LBWN_REQUIRE(lbwn_lc_upsample_part_floats(nup, strides, Li, Lo, frames) < (1ll << 31),
               "lc_upsample_forward: too many frames");
  return lbwn_lc_up_fwd_launch(nup, strides, Li, Lo, frames, mel, F, act, (hipStream_t)stream);
}

}  // extern "C"

// lbwn_lc_upsample_backward (dmel NULL) and lbwn_lc_upsample_backward_dmel: the same checks
static int lc_upsample_backward(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                                const float* const* F, const float* const* act, const float* dlc, int dlc_parts,
                                int64_t dlc_stride, float* dpart, float* const* dF, float* dmel, void* stream) {
  LBWN_REQUIRE(strides && mel && F && act && dlc && dpart && dF, "lc_upsample_backward: null argument");
  LBWN_REQUIRE(frames >= 1, "lc_upsample_backward: frames must be >= 1");
  LBWN_REQUIRE(lbwn_lc_up_fused_ok(nup, strides, Li, Lo),
               "lc_upsample_backward: shape outside the fused kernel's envelope");
  for (int i = 0; i < nup; ++i) {
    LBWN_REQUIRE(F[i] && dF[i], "lc_upsample_backward: F[%d] or dF[%d] is null", i, i);
    LBWN_REQUIRE(i + 1 == nup || act[i], "lc_upsample_backward: act[%d] is null", i);
    LBWN_REQUIRE((((uintptr_t)F[i] | (uintptr_t)dF[i] | (uintptr_t)act[i]) & 15) == 0,
                 "lc_upsample_backward: F[%d], dF[%d], act[%d] must be 16-byte aligned", i, i, i);
  }
  LBWN_REQUIRE(lbwn_lc_upsample_part_floats(nup, strides, Li, Lo, frames) < (1ll << 31),
               "lc_upsample_backward: too many frames");
  int hop = 1;
  for (int i = 0; i < nup; ++i) hop *= strides[i];
  LBWN_REQUIRE(dlc_parts >= 1, "lc_upsample_backward: dlc_parts must be >= 1");
  LBWN_REQUIRE(dlc_parts == 1 || (dlc_stride >= (int64_t)frames * hop * Lo && dlc_stride % 4 == 0),
               "lc_upsample_backward: dlc_stride must be a multiple of 4 and >= frames*hop*Lo");
  LBWN_REQUIRE((((uintptr_t)dlc | (uintptr_t)mel | (uintptr_t)dpart) & 15) == 0,
               "lc_upsample_backward: mel, dlc and dpart must be 16-byte aligned");
  LBWN_REQUIRE(((uintptr_t)dmel & 15) == 0, "lc_upsample_backward: dmel must be 16-byte aligned");
  float* a[4] = {nullptr, nullptr, nullptr, nullptr};   // read only by the backward
  for (int i = 0; i < nup; ++i) a[i] = const_cast<float*>(act[i]);
  return lbwn_lc_up_bwd_launch(nup, strides, Li, Lo, frames, mel, F, a, dlc, dpart, dF, (hipStream_t)stream, nullptr,
                               nullptr, dlc_parts, (long)dlc_stride, dmel);
}

extern "C" {

int lbwn_lc_upsample_backward(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                              const float* const* F, const float* const* act, const float* dlc, int dlc_parts,
                              int64_t dlc_stride, float* dpart, float* const* dF, void* stream) {
  return lc_upsample_backward(nup, strides, Li, Lo, frames, mel, F, act, dlc, dlc_parts, dlc_stride, dpart, dF, nullptr,
                              stream);
}

int lbwn_lc_upsample_backward_dmel(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                                   const float* const* F, const float* const* act, const float* dlc, int dlc_parts,
                                   int64_t dlc_stride, float* dpart, float* const* dF, float* dmel, void* stream) {
  LBWN_REQUIRE(dmel != nullptr, "lc_upsample_backward_dmel: dmel is null");
  return lc_upsample_backward(nup, strides, Li, Lo, frames, mel, F, act, dlc, dlc_parts, dlc_stride, dpart, dF, dmel,
                              stream);
}

int lbwn_gc_table(const float* emb, const float* wsig, const float* wgate, float* out, int L, int ncat1, int Ge, int Cd,
                  void* stream) {
  LBWN_REQUIRE(emb && wsig && wgate && out, "gc_table: null argument");
  LBWN_REQUIRE(L >= 1 && ncat1 >= 1 && Cd >= 1, "gc_table: L, ncat1 and Cd must be >= 1");
  LBWN_REQUIRE(Ge >= 1 && Ge <= 32, "gc_table: n_gc_embed must be in [1, 32]");
  return lbwn_gc_table_launch(emb, wsig, wgate, out, L, ncat1, Ge, Cd, (hipStream_t)stream);
}

int64_t lbwn_gc_part_floats_abi(int L, int Ge, int Cd) {
  if (L < 1 || Ge < 1 || Cd < 1) return 0;
  return (int64_t)lbwn_gc_part_floats(L, Ge, Cd);
}

int lbwn_gc_grads(const float* emb, const float* wsig, const float* wgate, const float* gcd, float* part, float* demb,
                  float* dsig, float* dgate, int L, int ncat1, int Ge, int Cd, void* stream) {
  LBWN_REQUIRE(emb && wsig && wgate && gcd && part && demb && dsig && dgate, "gc_grads: null argument");
  LBWN_REQUIRE(L >= 1 && ncat1 >= 1 && Cd >= 1, "gc_grads: L, ncat1 and Cd must be >= 1");
  return lbwn_gc_grad_launch(emb, wsig, wgate, gcd, part, demb, dsig, dgate, L, ncat1, Ge, Cd, (hipStream_t)stream);
}

int lbwn_gemm_set_mode(int mode) { return lbwn_gemm_set_mode_impl(mode); }
int lbwn_gemm_get_mode(void) { return lbwn_gemm_mode(); }

int lbwn_layer_image_floats_abi(void) { return lbwn_layer_image_floats(); }

int lbwn_layer_forward(const float* x_in, float* x_out, float* z, int64_t ldz, const float* w_sig,
                       const float* w_gate, const float* b_sig, const float* b_gate, const float* w_res,
                       const float* b_res, const float* gc_tab, const int* ids, const float* cond, int64_t ldcond,
                       int B, int T, int H, int dilation, int n_res, int n_dil, float* wpack_ws, void* stream) {
  LBWN_REQUIRE(x_in && z && w_sig && w_gate && w_res && wpack_ws, "layer_forward: null argument");
  LBWN_REQUIRE(!gc_tab || ids, "layer_forward: gc_tab needs ids");
  lbwn_layer_args a;
  memset(&a, 0, sizeof(a));
  a.x_in = x_in; a.x_out = x_out; a.z = z; a.ldz = (long)ldz;
  a.w_sig = w_sig; a.w_gate = w_gate; a.b_sig = b_sig; a.b_gate = b_gate; a.w_res = w_res; a.b_res = b_res;
  a.gc_tab = gc_tab; a.ids = ids; a.cond = cond; a.ldcond = (long)ldcond;
  a.B = B; a.T = T; a.H = H; a.d = dilation; a.Cr = n_res; a.Cd = n_dil;
  a.wpack = wpack_ws;
  if (int e = lbwn_pack_layers_launch(w_sig, w_gate, b_sig, b_gate, w_res, b_res, wpack_ws, 1, n_res, n_dil,
                                      (hipStream_t)stream))
    return e;
  return lbwn_layer_fwd_launch(a, (hipStream_t)stream);
}

// workspace of lbwn_layer_backward: packed image | per-tile weight-gradient slabs | out_a | out_c0
int64_t lbwn_layer_backward_ws_floats(int B, int T, int n_res) {
  const long M = (long)B * T;
  return (int64_t)lbwn_layer_image_floats() + (int64_t)lbwn_layer_bwd_grid(B, T) * lbwn_layer_slab_stride() +
         2 * (int64_t)M * n_res + 64;
}

int lbwn_layer_backward(const float* x_in, const float* dz, int64_t lddz, const float* dx_out, const float* w_sig,
                        const float* w_gate, const float* b_sig, const float* b_gate, const float* w_res,
                        const float* b_res, const float* gc_tab, const int* ids, const float* cond, int64_t ldcond,
                        float* dx_in, float* dw_sig, float* dw_gate, float* db_sig, float* db_gate, float* dw_res,
                        float* db_res, float* dcond, int64_t lddcond, float* gc_dtab, int B, int T, int H, int dilation,
                        int n_res, int n_dil, float* ws, void* stream) {
  LBWN_REQUIRE(x_in && dz && w_sig && w_gate && w_res && dx_in && dw_sig && dw_gate && dw_res && ws,
               "layer_backward: null argument");
  LBWN_REQUIRE(!gc_tab || ids, "layer_backward: gc_tab needs ids");
  LBWN_REQUIRE(!gc_dtab || gc_tab, "layer_backward: gc_dtab needs gc_tab");
  LBWN_REQUIRE(!dcond || cond, "layer_backward: dcond needs cond");
  LBWN_REQUIRE((((uintptr_t)ws) & 15) == 0, "layer_backward: workspace must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)B * T;
  float* img = ws;
  float* slab = img + lbwn_layer_image_floats();
  const int nblk = lbwn_layer_bwd_grid(B, T), sstr = lbwn_layer_slab_stride();
  float* out_a = slab + (long)nblk * sstr;
  out_a += (16 - ((uintptr_t)out_a & 15)) / 4 % 4;
  float* out_c0 = out_a + M * n_res;
  lbwn_layer_args a;
  memset(&a, 0, sizeof(a));
  a.x_in = x_in; a.dz_skip = dz; a.lddz = (long)lddz;
  a.g_a = dx_out; a.g_c0 = nullptr; a.g_d = 0;   // the caller's dL/dx_{l+1}, already combined
  a.w_sig = w_sig; a.w_gate = w_gate; a.b_sig = b_sig; a.b_gate = b_gate; a.w_res = w_res; a.b_res = b_res;
  a.gc_tab = gc_tab; a.ids = ids; a.cond = cond; a.ldcond = (long)ldcond;
  a.dv_out = dcond; a.lddv = (long)lddcond; a.gc_dtab = gc_dtab;
  a.out_a = out_a; a.out_c0 = out_c0;
  a.slab = slab; a.slab_stride = sstr;
  a.B = B; a.T = T; a.H = H; a.d = dilation; a.Cr = n_res; a.Cd = n_dil;
  a.wpack = img;
  if (int e = lbwn_pack_layers_launch(w_sig, w_gate, b_sig, b_gate, w_res, b_res, img, 1, n_res, n_dil, st)) return e;
  if (int e = lbwn_layer_bwd_launch(a, st)) return e;
  lbwn_layer_red_args r;
  memset(&r, 0, sizeof(r));
  r.slab = slab; r.nparts = nblk; r.stride = sstr; r.Cr = n_res; r.Cd = n_dil;
  r.dsig = dw_sig; r.dgate = dw_gate; r.dres = dw_res; r.dbsig = db_sig; r.dbgate = db_gate; r.dbres = db_res;
  if (int e = lbwn_layer_reduce_launch(r, st)) return e;
  return lbwn_layer_dx_combine_launch(out_a, out_c0, dx_in, B, T, H, dilation, n_res, st);
}

int lbwn_dsep_prepend(float* x_all, int64_t xls, const float* save, int n_layers, int nbl, int B, int T, int H,
                      int n_res, void* stream) {
  LBWN_REQUIRE(H >= (1 << (nbl - 1)), "dsep_prepend: halo %d < max dilation", H);
  return lbwn_dsep_prepend_launch(x_all, (long)xls, save, n_layers, nbl, B, T, H, n_res, (hipStream_t)stream);
}

int lbwn_dsep_save(const float* x_all, int64_t xls, float* save, int n_layers, int nbl, int B, int T, int H,
                   int n_res, void* stream) {
  LBWN_REQUIRE(H >= (1 << (nbl - 1)), "dsep_save: halo %d < max dilation", H);
  return lbwn_dsep_save_launch(x_all, (long)xls, save, n_layers, nbl, B, T, H, n_res, (hipStream_t)stream);
}

int lbwn_head_xent(float* logits, const int* wav_q, const int* ids, int B, int T, int Q, int write_grad, float* stats,
                   float* partial_ws, void* stream) {
  LBWN_REQUIRE(logits && wav_q && ids && stats && partial_ws, "head_xent: null argument");
  LBWN_REQUIRE(T >= 2, "head_xent: slice_sz must be >= 2");
  lbwn_head_args h;
  h.logits = logits; h.q = wav_q; h.ids = ids; h.B = B; h.T = T; h.Q = Q; h.partial = partial_ws;
  h.write_grad = write_grad;
  h.colpart = nullptr;
  int nb = 0;
  hipStream_t st = (hipStream_t)stream;
  if (int e = lbwn_head_launch(h, &nb, st)) return e;
  return lbwn_stats_reduce_launch(partial_ws, nb, stats, st);
}

int lbwn_head_xent_ex(float* logits, const int* wav_q, const int* ids, int B, int T, int Q, const float* teacher,
                      int64_t ld_teacher, float alpha, float temp, float smoothing, float* stats, float* stats_ex,
                      float* partial_ws, void* stream) {
  LBWN_REQUIRE(logits && wav_q && ids && stats && partial_ws, "head_xent_ex: null argument");
  LBWN_REQUIRE(T >= 2 && B >= 1 && Q >= 1, "head_xent_ex: B >= 1, slice_sz >= 2 and Q >= 1 required");
  LBWN_REQUIRE(alpha >= 0.f && alpha <= 1.f, "head_xent_ex: alpha %g outside [0, 1]", (double)alpha);
  LBWN_REQUIRE(std::isfinite(temp) && temp > 0.f, "head_xent_ex: temp %g must be finite and > 0", (double)temp);
  LBWN_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "head_xent_ex: smoothing %g outside [0, 1)", (double)smoothing);
  LBWN_REQUIRE(alpha == 0.f || teacher, "head_xent_ex: alpha > 0 needs the teacher's logits");
  LBWN_REQUIRE(!teacher || ld_teacher >= Q, "head_xent_ex: ld_teacher %lld < Q %d", (long long)ld_teacher, Q);
  lbwn_head_ex_args h;
  h.logits = logits; h.q = wav_q; h.ids = ids; h.B = B; h.T = T; h.Q = Q;
  h.teacher = alpha > 0.f ? teacher : nullptr;
  h.ld_teacher = (long)ld_teacher;
  h.alpha = alpha; h.temp = temp; h.inv_temp = 1.f / temp; h.eps = smoothing;
  h.partial = partial_ws;
  h.partial_ex = partial_ws + 3 * 2048;
  h.colpart = nullptr;
  int nb = 0;
  hipStream_t st = (hipStream_t)stream;
  if (int e = lbwn_head_ex_launch(h, &nb, st)) return e;
  return lbwn_stats_reduce_ex_launch(h.partial, h.partial_ex, nb, stats, stats_ex, st);
}

}  // extern "C"
