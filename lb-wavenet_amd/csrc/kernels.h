// Internal launch interfaces shared by the kernel TUs and the engine (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct lbwn_gemm_args {
  const float* A; long lda;
  const float* B; long ldb;
  float* C; long ldc;
  int M, N, K;
  const float* bias;   // [N] nullable
  const float* mask;   // mask[m*ldm+n] > 0 keeps the value; nullable
  long ldm;
  int relu_a, relu_out, accumulate;
  const unsigned short* b3;  // nullable: B pre-split into bf16 planes [N][K/32][3][32] (lbwn_split_planes_launch)
  const int* a_codes;  // m-contiguous A only: A[k][m] = (a_codes[k] == m)  (one-hot, tmodel.py:64-65)
  // nullable, bf16-split form without split-K only: column partial sums of the final C values
  // (after bias/relu/mask), [ceil(M/256)][N] (one part per 256-row block tile), summed by
  // lbwn_colsum_final_launch: the bias gradient without a second pass over C
  float* colpart;
  long long* step_advance;   // nullable, bf16-split form only: block 0 adds 1 (the per-step generator's counter)
  // bf16-split form, no split-K / accumulate / mask: > 0 stores C in the backward chain's row-load
  // order instead of rows (ldc unused): 32-column block j at C + j·c_chain_ls, element (m, c) at
  // sg_off(m, c / 8, (c / 4) & 1) + c % 4 (layer_common.h), so the chain's own-row loads are 1-KiB runs.
  // The A-in-registers forms (gemm_x3q_kernel) store the raw sums in this order: there the launcher
  // also refuses bias / relu_out / mbits / mbits_out; the LDS-staged forms apply bias and relu_out
  long c_chain_ls;
  int k_per_split;     // set by the launcher
  int* splits_deferred;   // host, nullable: split-K partials left unsummed in the slab workspace
                          // ([splits][M][N]); the launcher stores the split count here (1: C written)
  long split_stride;   // set by the launcher
  int xcd2d;           // gemm_x3q_kernel<10> (N % 160 == 0): the 2-D XCD blocking of its tiles (xcd2d_tile)
  // k-blocked operands (the backward chain's DV export, [K/32][Mp][32]): 0 = plain layout.
  // a_kstride: A k-contiguous with lda = 32, element (m, k) at A[m·32 + (k/32)·a_kstride + k%32]
  // (gemm_x3q_kernel only); b_gstride: B mn-contiguous with ldb = 32, element (k, n) at
  // B[k·32 + (n/32)·b_gstride + n%32] (the LDS-staged bf16-split kernel only); a_gstride: A
  // mn-contiguous with lda = 32, element (m, k) at A[k·32 + (m/32)·a_gstride + m%32] (the AMN
  // form of gemm_x3q_kernel only: dLCcat as DVᵀ·lc)
  long a_kstride, b_gstride, a_gstride;
  // 1: every output row is computed by the same kernel and k order whatever M is (the tall
  // 256-row form below M = 8192 too), so a row's value depends only on its own A row: the
  // training forward's head GEMMs, so a slice processed in stages equals one long slice bit for
  // bit (README.md:6-21)
  int row_exact;
  // gemm_x3q_kernel<8> tile form (lbwn_gemm_x3q8_form) only: the relu / mask predicate of the C
  // values as one 64-bit word per lane ([tile][wave][lane]: bit 8·nb + e = element (e, nb) of the
  // lane's epilogue), so a later GEMM of the SAME shape and form masks by it (mbits) instead of
  // reading an f32 M×N mask: mbits_out (producer) sets bit = (final C > 0); mbits (consumer)
  // replaces mask.  lbwn_gemm_mbits_words(M, N) words each.
  unsigned long long* mbits_out;
  const unsigned long long* mbits;
  // Masked-position skip (live_lists_body, prologue.h), both nullable.  row_live (the tall
  // k-contiguous gemm_x3q_kernel<8 / 10> forms only, lbwn_gemm_row_live_form): [ceil(M/256)], 0 =
  // every A row of the 256-row tile is exactly zero: the tile runs no k-step and its epilogue writes
  // what zero accumulators give.  k_live / nk_live (the mn-contiguous weight-gradient forms only,
  // lbwn_gemm_k_live_form): the ascending list of the 32-deep k-steps whose B rows are not all
  // exactly zero, its length, and k_pre[k] = the number of list entries below k-step k
  // ([K/32 + 1]).  Every split-K slice keeps its own k range and walks the list entries inside it,
  // so each partial sums the same non-zero terms in the same order as without the list: the
  // result is the same bit for bit (a skipped term is an exact zero).
  const int* row_live;
  const int* k_live;
  const int* nk_live;
  const int* k_pre;
};
// the launches that take row_live / k_live (anything else refuses them)
bool lbwn_gemm_row_live_form(int M, int N, int K, int a_kcontig, int presplit, int row_exact, int colpart);
bool lbwn_gemm_k_live_form(int M, int N, int K);
// the tall pre-split product that runs gemm_x3q_kernel<8> (the form mbits / mbits_out need)
bool lbwn_gemm_x3q8_form(int M, int N, int K, int a_kcontig, int presplit, int row_exact, int colpart);
inline long lbwn_gemm_mbits_words(long M, long N) { return ((M + 255) / 256) * ((N + 127) / 128) * 8 * 64; }
int lbwn_gemm_launch(const lbwn_gemm_args& a, int a_kcontig, int b_kcontig, int split_k, float* slab_ws,
                     hipStream_t st);
// the kernel instantiation the most recent lbwn_gemm_launch on this thread chose (the names
// of include/lbwn.h lbwn_gemm_last_form; "" while the call has launched nothing)
const char* lbwn_gemm_last_form_impl(void);
inline int lbwn_colpart_parts(long M) { return (int)((M + 255) / 256); }
// Pre-split planes of a weight for lbwn_gemm_args::b3: rows = N of the product it feeds,
// W[r][k] (trans = 0) or W[k][r] (trans = 1), row stride ldw; up to 6 weights per launch.
// Element count of one output:
size_t lbwn_split_planes_elems(int rows, int K);
int lbwn_split_planes_launch(int njobs, const float* const* W, const long* ldw, const int* rows, const int* K,
                             const int* trans, unsigned short* const* out, hipStream_t st);
// 1: bf16-split (default), 0: f32 MFMA (gemm.hip)
int lbwn_gemm_mode(void);
int lbwn_gemm_set_mode_impl(int mode);

// One residual layer (tmodel.py:117-184).  x buffers are [B][H+T][Cr]; rows [H-d, H) of
// x_in hold the D-separation state SAVE_l (prepended by lbwn_dsep_prepend).
struct lbwn_layer_args {
  const float* x_in;
  float* x_out;             // nullable (last layer's residual output is dead)
  float* z; long ldz;       // Zcat column block of this layer
  const float* w_sig; const float* w_gate;  // [2][Cr][Cd]
  const float* b_sig; const float* b_gate;  // [Cd] nullable
  const float* w_res; const float* b_res;   // [Cd][Cr], [Cr] nullable
  const float* wpack;       // packed LDS image of this layer (lbwn_pack_layers_launch)
  const float* gc_tab;      // rows [ncat+1] of (sig Cd | gate Cd), row stride gc_ld (0 = 2Cd); nullable
  long gc_ld;
  const int* ids;           // [B][T]
  const float* cond; long ldcond;  // [M][2*Cd] nullable (LC projection)
  int B, T, H, d, Cr, Cd;
  // ---- backward only ----
  const float* dz_skip; long lddz;   // [M] rows of dS·SKIP_lᵀ (column block of dZ)
  const float* g_a; const float* g_c0; int g_d;  // dx_{l+1}[t] = g_a[t] + g_c0[t+g_d]; nullable => 0
  float* out_a; float* out_c0;                    // [M][Cr]
  float* slab;              // per-block weight-grad partials [nblocks][slab_stride]
  int slab_stride;
  float* dv_out; long lddv; // [M][2Cd] nullable (needed for LC grads)
  float* gc_dtab;           // [ncat+1][2Cd] atomically accumulated (nullable)
};
// Sum a layer's per-block weight-grad partials into the reference-layout gradients.
struct lbwn_layer_red_args {
  const float* slab; int nparts; int stride;
  float* dsig; float* dgate; float* dres;      // [2][Cr][Cd], [2][Cr][Cd], [Cd][Cr]
  float* dbsig; float* dbgate; float* dbres;   // nullable
  int Cr, Cd;
};
constexpr int LBWN_LAYER_POS = 128;   // positions per layer-kernel block
int lbwn_layer_fwd_launch(const lbwn_layer_args& a, hipStream_t st);
int lbwn_layer_bwd_launch(const lbwn_layer_args& a, hipStream_t st);
int lbwn_layer_slab_stride();
// split weight images for the forward chain's bf16-split products (bf16 elements per layer)
int lbwn_layer_image_x3_elems();
// The training step's start-of-step work in one launch (pack.hip step_prologue_kernel): the
// arguments of lbwn_pack_layers_fb_x3_launch, lbwn_split_planes_launch (njobs 0..6),
// lbwn_embed_launch, lbwn_dsep_prepend_launch and lbwn_zero_launch (zero_bytes may be 0).
struct lbwn_prologue_args {
  const float *sig, *gate, *sig_b, *gate_b, *res, *res_b;
  unsigned short* fout;
  float* bout;
  int L, Cr, Cd;
  const float* skip_b;
  int Cs;
  float* bsum;
  const float *lc_sig, *lc_gate;
  int Lo;
  unsigned short* lcout;
  int lc16;
  int njobs;
  const float* W[6];
  long ldw[6];
  int rows[6], K[6], trans[6];
  unsigned short* out[6];
  const int* q;
  const float *pre, *pre_b;
  float* X;
  long xls;
  const float* save;
  int nbl, B, T, H, Q;
  void* zero;
  size_t zero_bytes;
  // nullable: the masked-position live lists of this step's ids ([B][T]; live_lists_body)
  const int* ids;
  int *tlive, *klive, *nklive, *kpre;
};
int lbwn_step_prologue_launch(const lbwn_prologue_args& a, hipStream_t st);
// Both chains' split images in one launch: the L forward images (fout, lbwn_layer_image_x3_elems
// each) and the L backward images (bout, lbwn_layer_image_bx3_floats each), plus (skip_b, bsum
// non-null) bsum[n] = Σ_l skip_b[l·Cs + n] (lbwn_sum_bias_launch)
// ... and (lcout non-null) the L split LC images of the in-chain LC term (lbwn_lc_image_x3_elems each)
int lbwn_pack_layers_fb_x3_launch(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                                  const float* res, const float* res_b, unsigned short* fout, float* bout, int L,
                                  int Cr, int Cd, const float* skip_b, int Cs, float* bsum, const float* lc_sig,
                                  const float* lc_gate, int Lo, unsigned short* lcout, hipStream_t st,
                                  int lc16 = 0);
int lbwn_lc_image_x3_elems();
int lbwn_lc_image16_elems();       // the 16-lane forward chain's LC image (lc16 = 1 above)
// forward chain form: 0 = 32-position waves (chain_fwd_kernel, 128-position tiles), 4 / 8 =
// 16-position waves (chain_fwd16_kernel) with 4 / 8 waves = 64- / 128-position tiles
int lbwn_chain_fwd_tile(int fwd_nw);
int lbwn_lc_in_chain_ok(int Lo);   // n_lc_out the forward chain's in-chain LC term supports
int lbwn_layer_image_floats();
int lbwn_layer_dx_combine_launch(const float* out_a, const float* out_c0, float* dx, int B, int T, int H, int d, int C,
                                 hipStream_t st);
// backward split images (WD bf16 + Rs f32) for the bf16-split backward chain, floats per layer
int lbwn_layer_image_bx3_floats();
int lbwn_layer_nblocks(int B, int T);
int lbwn_layer_bwd_grid(int B, int T);   // = number of slab partials per layer
int lbwn_pack_layers_launch(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                            const float* res, const float* res_b, float* out, int L, int Cr, int Cd, hipStream_t st);
int lbwn_layer_reduce_launch(const lbwn_layer_red_args& r, hipStream_t st);

// Persistent layer chain (all L layers in one launch, tile hand-offs through flags).
struct lbwn_chain_args {
  float* X; long xls;          // x_l buffers of all layers, layer stride in floats
  float* Z; long ldz;
  const float* wpack;
  const unsigned short* wpack_x3;   // forward: split images (bf16-split conv/residual) or null
  const float* gc_tab; long gc_ld; const int* ids;   // GC table [ncat+1][L·2Cd] or null
  const float* cond; long ldcond;                     // LC term [M][L·2Cd] or null
  float* dv_out; long lddv; float* gc_dtab;           // backward: LC dv export, GC grad table
  unsigned* flags;             // [B·ceil(T/128)] (zeroed by the launcher unless flags_zeroed)
  int flags_zeroed;            // the caller zeroed flags on this stream (no memset here)
  unsigned* status;            // sticky error word (spin timeout)
  int B, T, H, L, nbl, Cr, Cd;
  int grid;                    // ≤ blocks resident at once (rounds of tiles)
  // backward only
  const float* DZ;             // dZ (row stride ldz), or in chain order (dzls > 0, bf16-split chain)
  long dzls = 0;               // chain order: layer stride of DZ (lbwn_gemm_args::c_chain_ls)
  float* slab;                 // [L][ntiles][slab_stride]
  float* ocg; long ocls;       // out_c0 hand-off rows per layer [L][B·T][32]
  float* dx0_a; float* dx0_c;  // layer 0's dx parts [B·T][32]
  long long* trace = nullptr;  // debug: cycle stamps of block trace_blk, [L][16] (LBWN_CHAIN_TRACE)
  int trace_blk = 0;
  // bf16-split backward (chain_bwd_x3_kernel): σ(v_gate) rows [L][M][32] written by the X3
  // forward chain (layer stride sgls floats), and the backward images (lbwn_pack_layers_fb_x3)
  float* SG = nullptr; long sgls = 0;
  const float* bimg = nullptr;
  int* tile_gid = nullptr;     // x3 backward + GC: [ntiles] uniform voice id per tile or -1
  // forward, bf16-split form: in-chain LC term (instead of cond): LC input [M][Lo], split images
  const float* lcact = nullptr; const unsigned short* lcimg = nullptr; int Lo = 0;
  int fwd_nw = 0;              // forward form (lbwn_chain_fwd_tile); lcimg in the matching layout
  int bwd_nw = 0;              // backward form: 0 = chain_bwd_x3_kernel (128), 4 / 8 = chain_bwd16_kernel
  int xcd = 0;                 // XCD-grouped tile walk (layer_common.h chain_first)
  long dvks = 0;               // x3 backward forms: dv_out k-blocked ([L·2][Mp][32], chunk stride dvks)
};
int lbwn_chain_fwd_launch(const lbwn_chain_args& c, hipStream_t st);
int lbwn_chain_bwd_launch(const lbwn_chain_args& c, hipStream_t st);
int lbwn_layer_reduce_all_launch(const lbwn_layer_red_args& r, int L, long slab_layer, hipStream_t st);

// D-separation state transfer for ALL layers at once.
int lbwn_dsep_prepend_launch(float* xall, long xlayer_stride, const float* save, int L, int nbl,
                             int B, int T, int H, int Cr, hipStream_t st);
int lbwn_dsep_save_launch(const float* xall, long xlayer_stride, float* save, int L, int nbl, int B,
                          int T, int H, int Cr, hipStream_t st);

int lbwn_embed_launch(const int* q, const float* pre, const float* pre_b, float* x0, int B, int T, int H,
                      int Cr, int Q, hipStream_t st);

struct lbwn_head_args {
  float* logits;            // [M][Q] in: logits, out: dlogits (unnormalised: (softmax-onehot)·mask)
  const int* q;             // [B][T] targets (mu-law codes)
  const int* ids;           // [B][T]
  int B, T, Q;
  float* partial;           // [nblocks][3] (sum_xent, n_valid, sum |argmax diff|)
  int write_grad;
  float* colpart;           // nullable: [nblocks][Q] column sums of the dlogits written (Q <= 512)
};
int lbwn_head_nblocks(long M, bool colpart);
int lbwn_head_launch(const lbwn_head_args& a, int* nblocks_out, hipStream_t st);
int lbwn_stats_reduce_launch(const float* partial, int nparts, float* stats, hipStream_t st);

// The head against a second distribution (include/lbwn.h lbwn_train_forward_ex: distillation and
// label smoothing; arguments checked by the caller).  The grid is lbwn_head_nblocks'.
struct lbwn_head_ex_args {
  float* logits;            // [M][Q] in: the student's logits, out: dlogits (unnormalised)
  const int* q;             // [B][T] targets
  const int* ids;           // [B][T]
  int B, T, Q;
  const float* teacher;     // [M][ld_teacher] the teacher's logits; NULL with alpha = 0 (never read)
  long ld_teacher;
  float alpha, temp, inv_temp, eps;
  float* partial;           // [nblocks][3] (Σ value, n_valid, Σ |argmax diff|)
  float* partial_ex;        // [nblocks][2] (Σ plain xent, Σ KL)
  float* colpart;           // nullable: [nblocks][Q] column sums of the dlogits written (Q <= 512)
};
int lbwn_head_ex_launch(const lbwn_head_ex_args& a, int* nblocks_out, hipStream_t st);
// stats as lbwn_stats_reduce_launch; stats_ex (nullable) = (Σ plain xent, Σ KL, 0, 0), or with
// partial_ex NULL (after the plain head) (stats[0], 0, 0, 0)
int lbwn_stats_reduce_ex_launch(const float* partial, const float* partial_ex, int nparts, float* stats,
                                float* stats_ex, hipStream_t st);

// lbwn_train_eval's head (head.hip): the xent of the training head with no gradient written, per-block
// partials in double, then a fixed-order fold into acc / by_voice
struct lbwn_eval_head_args {
  const float* logits;      // [M][Q], read only
  const int* q;             // [B][T] targets
  const int* ids;           // [B][T]
  int B, T, Q;
  float* nll;               // nullable: [B][ld_nll], the value or 0 where not scored
  long ld_nll;
  float* rowv;              // nullable: [M], the same values for the per-voice pass
  double* partial;          // [nblocks][4] (Σnll, count, Σ|argmax - c|, hits)
};
int lbwn_eval_nblocks(long M);
size_t lbwn_eval_scratch_bytes(long M, int n_bins);
int lbwn_eval_head_launch(const float* logits, const int* q, const int* ids, int B, int T, int Q, float* nll,
                          long ld_nll, double* acc, double* by_voice, int n_bins, const unsigned* plan_status,
                          unsigned* status, void* scratch, hipStream_t st);

// several column sums in one launch pair; ws holds Σ_j lbwn_colsum_ws_floats(M, N[j]) floats
int lbwn_colsum_multi_launch(int njobs, const float* const* X, const long* ldx, const int* N, float* const* out,
                             const int* accumulate, int M, float* ws, hipStream_t st);
int lbwn_colsum_ws_floats(int M, int N);
// the two passes apart: the first pass alone (*nparts = its partial row count; ws holds that ×
// N floats), and the second over any partials (first-pass ones or a GEMM epilogue's colpart)
int lbwn_colsum_partial_launch(const float* X, long ldx, int M, int N, float* ws, int* nparts, hipStream_t st);
int lbwn_colsum_final_launch(int njobs, float* const* parts, const int* N, float* const* out, const int* accumulate,
                             const int* nparts, hipStream_t st,
                             const int* reps = nullptr);
int lbwn_sum_bias_launch(const float* b, int L, int N, float* out, hipStream_t st);

int lbwn_adam_launch2(float* params, const float* grads, float* m, float* v, long n_weights, long n_total,
                      float lr, float b1, float b2, float eps, float l2, const float* stats,
                      const long long* counters, const unsigned* status, hipStream_t st);
// nonfinite (nullable): the decision word lbwn_adam_ex_launch's update left; set = count the step in
// *nonfinite_skips (nullable) and advance nothing
int lbwn_counters_launch(long long* counters, const float* stats, int adam_applied, const unsigned* status,
                         hipStream_t st, const unsigned* nonfinite = nullptr, long long* nonfinite_skips = nullptr);
// The extended Adam step (include/lbwn.h lbwn_adam_ex; arguments checked by the caller).  part,
// nparts and decision are carved from ws by the launcher.
struct lbwn_adam_ex_dev {
  float* p; const float* gr; float* m; float* v;
  long nw, n;
  float lr, b1, b2, eps, l2;
  const float* stats; const long long* counters; const unsigned* status;
  float clip;           // 0 = no clipping
  int skip_nonfinite;
  float ema_decay; int ema_num_updates; float* ema;   // ema == nullptr: no EMA
  long warmup, decay_steps; float decay_rate; int staircase;
  const double* part; int nparts; unsigned* decision;
  float* info;
};
int lbwn_adam_ex_nparts(long n);
long lbwn_adam_ex_ws_floats_impl(long n);
// norm_pass: run the Σ g² launch first (ws holds lbwn_adam_ex_ws_floats_impl(n) floats).
// *decision: the word for lbwn_counters_launch's `nonfinite` (nullptr without the norm pass)
int lbwn_adam_ex_launch(lbwn_adam_ex_dev a, float* ws, bool norm_pass, hipStream_t st, const unsigned** decision);
// dPRE = onehot(q)ᵀ·dx0 as an LDS-histogram scatter + fixed-order reduction; dPRE_B = Σ dx0 (nullable);
// dx0[m] = g[m] + (t+gd < T ? dprev[m+gd] : 0) formed on the fly
int lbwn_pre_grad_ws_floats(int Q, int Cr);
int lbwn_pre_grad_launch(const int* q, const float* g, const float* dprev, int gd, int B, int T, int Cr, int Q,
                         float* dpre, float* dpre_b, float* ws, hipStream_t st);

int lbwn_mulaw_encode_launch(const float* x, int* q, long n, int n_quanta, int tf32, hipStream_t st);
int lbwn_mulaw_decode_launch(const int* q, float* x, long n, int n_quanta, hipStream_t st);
int lbwn_bcast_rows_launch(float* dst, int L, int N, hipStream_t st);
int lbwn_zero_launch(void* p, size_t n_bytes, hipStream_t st);
// GC table gradient of the uniform-id tiles from the backward chain's slab bias partials
int lbwn_gc_tile_sum_launch(const float* slab, int L, int ntiles, const int* tile_gid, float* gtab, long ld,
                            int ncat1, hipStream_t st);

// Conditioning (cond.hip)
int lbwn_gc_table_launch(const float* emb, const float* wsig, const float* wgate, float* out, int L, int ncat1,
                         int Ge, int Cd, hipStream_t st);
int lbwn_gc_grad_launch(const float* emb, const float* wsig, const float* wgate, const float* gcd, float* part,
                        float* demb, float* dsig, float* dgate, int L, int ncat1, int Ge, int Cd, hipStream_t st);
int lbwn_gc_part_floats(int L, int Ge, int Cd);
int lbwn_lc_pack_launch(float* cat, float* wsig, float* wgate, int L, int Clc, int Cd, int pack, hipStream_t st);
// LC upsample (tmodel.py:68-83) fused over its stages, one block per mel frame (cond.hip)
int lbwn_lc_up_fused_ok(int nup, const int* s, int Li, int Lo);
int lbwn_lc_up_part_floats(int nup, const int* s, int Li, int Lo, int frames);
int lbwn_lc_up_fwd_launch(int nup, const int* s, int Li, int Lo, int frames, const float* mel, const float* const* F,
                          float* const* act, hipStream_t st);
// the per-frame pass on st; the frame-partial sum on st_sum (after ev, recorded on st, when they differ);
// dmel: nullable, d(mel) [frames][Li] (stage 0's input gradient, stored by the per-frame pass)
int lbwn_lc_up_bwd_launch(int nup, const int* s, int Li, int Lo, int frames, const float* mel, const float* const* F,
                          float* const* act, const float* dlc, float* dpart, float* const* dF, hipStream_t st,
                          hipStream_t st_sum = nullptr, hipEvent_t ev = nullptr, int dlc_parts = 1,
                          long dlc_stride = 0, float* dmel = nullptr);

// Log-mel front end (mel.hip).  The tables live in the caller's workspace:
// basis [ncb][n_fft/4][2 (cos | sin)][32 bins][4 samples] f32 (windowed, zero past bin n_fft/2), then
// the filterbank [ncb·32][nt·32] f32 (zero-padded), 256-byte aligned.
struct lbwn_mel_dims {
  int n_fft, win, hop, n_mels, power;
  int nbins, ncb, nt;     // n_fft/2+1 bins in ncb 32-bin column blocks; nt 32-band tiles
  int cb_lo, cb_hi;       // the column blocks that hold a bin with a nonzero filterbank row: [cb_lo, cb_hi)
  int rows;               // frames per block: 64 or 32
  float log_floor;
};
size_t lbwn_mel_basis_floats(const lbwn_mel_dims& d);
size_t lbwn_mel_lds_bytes(const lbwn_mel_dims& d, int rows);
int lbwn_mel_basis_launch(const lbwn_mel_dims& d, float* basis, hipStream_t st);
// once per device before the first lbwn_mel_fwd_launch of these dims: the kernel's dynamic-LDS limit
int lbwn_mel_fwd_prepare(const lbwn_mel_dims& d);
int lbwn_mel_fwd_launch(const lbwn_mel_dims& d, const float* basis, const float* fb, const float* wav, long ld_wav,
                        int batch, long n, long frames, float* out, long ld_out, hipStream_t st);
