/* lbwn — MI355X-native WaveNet hot path, C ABI.
 *
 * Drop-in boundary for hrbigelow/lb-wavenet's TensorFlow graph builders.  The reference
 * has no FFI (it is pure Python over TensorFlow 1.x C++ kernels); each entry point below
 * replaces the TF kernel sequence built at the cited reference line.  Host code (the
 * Python `lbwn` package, or any C/C++ caller) owns every buffer; the library never
 * allocates device memory, never synchronises, and is stateless except for the opaque
 * plan (shapes + workspace carving).  All device pointers are fp32 [B][T][C]
 * channels-last unless noted; int32 for µ-law codes and voice ids.  Every call is
 * stream-ordered on the caller's hipStream_t (passed as void*; NULL = default stream).
 * Return value: 0 on success, otherwise a hipError_t or 22 (EINVAL); the message is
 * available from lbwn_last_error() (thread-local).  Errors mirror the reference's
 * "print to stderr + exit(1)" checks (arch.py:147-161) as return codes instead.
 */
#ifndef LBWN_H
#define LBWN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBWN_ABI_VERSION 5

/* par/arch*.json after normalisation (tmodel.py:10-23, arch.py:31-103). */
typedef struct lbwn_arch {
  int n_blocks, n_block_layers;
  int n_quant, n_res, n_dil, n_skip, n_post;
  int n_gc_embed, n_gc_category; /* n_gc_embed == 0: no global conditioning */
  int n_lc_in, n_lc_out;         /* n_lc_out == 0: no local conditioning     */
  int n_lc_upsample;
  int lc_upsample[8];
  int use_bias;
} lbwn_arch;

/* Device pointers into a caller-owned flat fp32 buffer, reference layouts
 * (arch.py:85-103).  Per-layer tensors of one kind are contiguous over the
 * L = n_blocks*n_block_layers layers in (block, layer) order, e.g. sig = SIGNAL_0_0,
 * SIGNAL_0_1, ... each [2][n_res][n_dil].  Bias pointers are NULL when !use_bias; GC/LC
 * pointers are NULL when the arch has no GC/LC. */
typedef struct lbwn_params {
  float* pre;   float* pre_b;          /* PRE [Q][Cr], PRE_BIAS [Cr]                    */
  float* sig;   float* sig_b;          /* SIGNAL [L][2][Cr][Cd], SIGNAL_BIAS [L][Cd]     */
  float* gate;  float* gate_b;         /* GATE   [L][2][Cr][Cd], GATE_BIAS   [L][Cd]     */
  float* res;   float* res_b;          /* RESIDUAL [L][Cd][Cr], RESIDUAL_BIAS [L][Cr]    */
  float* skip;  float* skip_b;         /* SKIP [L][Cd][Cs], SKIP_BIAS [L][Cs]            */
  float* gc_embed;                     /* GC_EMBED [n_cat+1][Ge]                         */
  float* gc_sig; float* gc_gate;       /* GC_SIGNAL/GC_GATE [L][Ge][Cd]                  */
  float* lc_sig; float* lc_gate;       /* LC_SIGNAL/LC_GATE [L][Clc][Cd]                 */
  float* lc_up[8];                     /* LC_UPSAMPLE_i [s_i][Clc][dim2]                 */
  float* post1; float* post1_b;        /* POST1 [Cs][Cp], POST1_BIAS [Cp]                */
  float* post2; float* post2_b;        /* POST2 [Cp][Q],  POST2_BIAS [Q]                 */
} lbwn_params;

const char* lbwn_last_error(void);
int lbwn_abi_version(void);

/* ---- plan: the WaveNetTrain graph for a fixed (arch, batch_sz, slice_sz) ------------ */
typedef struct lbwn_plan lbwn_plan;
/* replaces WaveNetTrain.__init__ + build() graph construction (tmodel.py:8-48, :292-340).
 * n_quant is a multiple of 4; lbwn_train_backward takes n_quant <= 1024 (EINVAL beyond).
 * n_blocks >= 1, n_block_layers in 1..16, batch_sz >= 1, slice_sz >= 2 and
 * batch_sz * slice_sz >= 4 positions (EINVAL below: the bf16-split GEMMs take no fewer than 4 rows). */
int lbwn_plan_create(const lbwn_arch* arch, int batch_sz, int slice_sz, lbwn_plan** out);
void lbwn_plan_destroy(lbwn_plan* plan);
size_t lbwn_plan_workspace_bytes(const lbwn_plan* plan);
/* Byte offset/size of a named workspace tensor (for parity tests / debugging):
 * "x" [L][B][H+T][n_res] (layer inputs with D-sep halo, H = 2^(n_block_layers-1)),
 * "z" [M][L·n_dil] (gate outputs), "s" [M][n_skip] (skip sum), "r2" [M][n_post],
 * "logits" [M][n_quant] (dlogits after forward), "dh" [M][n_post], "ds" [M][n_skip],
 * "dz" [M][L·n_dil] (backward: dS·SKIPcatᵀ; with the bf16-split chains in the chain's 32-row
 * block order instead of rows, c_chain_ls below, [L·n_dil/32][ceil(M/32)·32·32], the size
 * reported accordingly after such a backward), "status" (int32: 0, or the code of a chain hand-off that timed out), and
 * for conditioned archs "cond" [M][L·2·n_dil] (LC term), "dvall" (its dv: rows [M][L·2·n_dil],
 * or after a bf16-split chain backward k-blocked [2L][ceil(M/32)·32][32], the size reported
 * accordingly), "gctab"/"gcd" [n_cat+1][L·2·n_dil] (GC table, its gradient).  */
int lbwn_plan_tensor(const lbwn_plan* plan, const char* name, size_t* offset, size_t* bytes);
/* Which branch of the conditioning dispatch the plan takes (host fields, no device work; added after
 * ABI 5 was declared, same ABI).  Keys: "up_fused" / "up_fused_bwd" (the LC upsample runs as one
 * fused launch forward / backward, else one GEMM per stage), "lc_in_chain" (the plan carved the LC
 * images: the bf16-split forward chain computes the LC term itself), "split_dlc", "split_dlcx",
 * "split_dlct", "split_up0" .. "split_up7" (split-K counts of dLCcat, dlc, dLCcatᵀ and the per-stage
 * filter gradients; 0 for a stage the arch does not have), and, valid after a backward, "dv_blk" (DV
 * was exported k-blocked) and "dlc_parts" (split-K partials dlc left for the fused upsample backward);
 * "dmel_fused", valid after a lbwn_train_backward_ex that wrote dmel: 1 = the fused upsample backward
 * wrote it, 0 = a GEMM after the per-stage products, -1 before any such backward.
 * An unknown key is EINVAL. */
int lbwn_plan_info(const lbwn_plan* plan, const char* key, int64_t* value);
/* One-shot timing probe: the next lbwn_train_forward/backward on this plan records
 * hipEvent_t ev_start right before and ev_stop right after the named launch(es):
 * "layer_fwd" (the residual stack: the persistent chain launch, or the span of the
 * per-layer launches; "layer_fwd@<l>" = layer l of the per-layer path), "layer_bwd",
 * "layer_reduce", "skip_fwd" (S = Zcat·SKIPcat), "post1_fwd", "post2_fwd", "head", "lc_cond",
 * "dpost2", "dh", "dpost1", "ds", "dskip" (Zcatᵀ·dS), "dz" (dS·SKIPcatᵀ).  Events are the
 * caller's (e.g. torch.cuda.Event(enable_timing=True).cuda_event). */
int lbwn_plan_probe(lbwn_plan* plan, const char* launch_name, void* ev_start, void* ev_stop);
/* Make `stream` wait (hipStreamWaitEvent, no host sync) for a point of the last
 * lbwn_train_backward on this plan, so that a data-parallel caller can start a gradient
 * all-reduce bucket before the backward ends.  point "head_grads": the POST1/POST2 weight
 * gradients, their biases and SKIP_BIAS are final and the backward chain has completed (no
 * collective can then share the chip with a persistent chain launch).  point "side_grads": the
 * end of the plan's side stream -- PRE, SIGNAL, GATE, RESIDUAL, the GC tables and their biases
 * are final (dSKIP may still run).  *waited = 1 if the plan has that point (chain plans; for
 * "head_grads" without padded head widths), else 0 and nothing is enqueued (wait for the whole
 * backward instead).  Added in ABI 2 ("side_grads": round 6, same ABI). */
int lbwn_plan_stream_wait(lbwn_plan* plan, const char* point, void* stream, int* waited);
/* receptive field F = n_blocks·Σ2^l (tmodel.py:50-51) */
int lbwn_recep_field_sz(const lbwn_arch* arch);

/* Forward + loss of one slice (tmodel.py:292-328 + _loss_fcn :218-289).
 *   wav_q  int32 [B][T] µ-law codes; ids int32 [B][T] (0 = invalid window);
 *   mel    fp32 [B][T/hop][n_lc_in] or NULL;  save fp32 D-sep state, layers packed in
 *          (block, layer) order, each SAVE_{d}_{b}_{bl} [B][d][n_res]; read (prepend) and
 *          updated in place (tmodel.py:122-127, :163-166).
 *   stats  fp32[4] out: Σ masked xent, n_valid, Σ|argmax diff|·mask, 1/n_valid (0 if none).
 * The plan's workspace keeps the activations for lbwn_train_backward. */
int lbwn_train_forward(lbwn_plan* plan, const lbwn_params* params, void* workspace, const int* wav_q,
                       const int* ids, const float* mel, float* save, float* stats, void* stream);

/* The training forward against a second distribution: knowledge distillation (soft targets at a
 * temperature, mixed with the hard loss) and label smoothing (added after ABI 5 was declared, same ABI:
 * symbols added, none altered).  The forward is lbwn_train_forward's up to the raw logits;
 * the head then forms, per row m = (b, t), t < T-1, scored iff ids[b][t+1] != 0 with the target
 * c = wav_q[b][t+1] (exactly as lbwn_train_forward), with l the student's logits of the row, u the
 * teacher's, Q = n_quant, τ = distill_temp, α = distill_alpha, ε = label_smoothing:
 *   p = softmax(l),  pS = softmax(l/τ),  pT = softmax(u/τ),  q_k = (1-ε)·[k == c] + ε/Q,
 *   hard  = lse(l) - Σ_k q_k·l_k                    (lbwn_train_forward's xent when ε = 0)
 *   kl    = Σ_k pT_k·(log pT_k - log pS_k)          (a term with pT_k = 0 contributes 0)
 *   value = (1-α)·hard + α·τ²·kl
 *   dlogits_k = (1-α)·(p_k - q_k) + α·τ·(pS_k - pT_k)
 * dlogits are written in place over "logits", 0 at unscored rows and at t = T-1; the gradient is
 * unnormalised and carries no l2 term, so lbwn_adam_* apply to it as they are.  The plan is left in the
 * state lbwn_train_forward leaves: lbwn_train_backward and lbwn_train_backward_ex (dmel included) follow
 * unchanged and give the gradients of Σ value.
 *   stats     fp32[4] out: [0] Σ value (the quantity optimised), [1] n_valid, [2] Σ|argmax(l) - c|·mask,
 *             [3] 1/n_valid (0 if none): [1..3] are lbwn_train_forward's.
 *   stats_ex  nullable device fp32[4] out: [0] Σ plain, unsmoothed xent (comparable with lbwn_train_forward
 *             and lbwn_train_eval), [1] Σ kl (not scaled by τ²), [2] = [3] = 0.
 *   teacher_logits  device fp32, row m at teacher_logits + m·ld_teacher, n_quant values read; 16-byte
 *             aligned, ld_teacher >= n_quant and a multiple of 4.  Rows of unscored positions and of
 *             t = T-1 are not read; with α = 0 nothing is read and the pointer may be NULL.  The student's
 *             logits are overwritten in place, so the teacher's must lie outside this plan's workspace:
 *             another plan's workspace ("logits" after lbwn_train_eval) or a buffer of the caller's.
 * All sums are formed in the head's fixed order (per wave in row order, ((w0+w1)+w2)+w3 per block, one
 * fold); no floating-point atomics: two calls on the same inputs give the same bits.  The workspace size
 * of every plan is what it was without this call.
 * With α = 0 and ε = 0 (τ is then without effect, teacher_logits is not read) and stats_ex NULL the call
 * launches exactly what lbwn_train_forward launches and gives its bits; with stats_ex the fold also writes
 * stats_ex = (stats[0], 0, 0, 0), in the same number of launches.
 * α, τ and ε are host scalars read at the call: a captured graph bakes them in (capture again to change
 * them), as with lbwn_gen_set_sampling.
 * EINVAL before any launch and before the device is touched, naming the argument: every refusal of
 * lbwn_train_forward (a null plan, params, workspace, wav_q, ids, save or stats; mel NULL on an LC arch); a
 * null args; struct_size != sizeof(lbwn_forward_args); distill_alpha outside [0, 1]; distill_temp not
 * finite or <= 0; label_smoothing outside [0, 1); distill_alpha > 0 with teacher_logits NULL;
 * teacher_logits not 16-byte aligned; ld_teacher < n_quant or not a multiple of 4; teacher_logits
 * overlapping this plan's workspace. */
typedef struct lbwn_forward_args {
  size_t struct_size;
  const int* wav_q;
  const int* ids;
  const float* mel;
  float* save;
  float* stats;
  float* stats_ex;
  const float* teacher_logits;
  int64_t ld_teacher;
  float distill_alpha;
  float distill_temp;
  float label_smoothing;
} lbwn_forward_args;
int lbwn_train_forward_ex(lbwn_plan* plan, const lbwn_params* params, void* workspace, const lbwn_forward_args* a,
                          void* stream);

/* Gradients of Σ masked xent (NOT divided by n_valid, no l2 term: both are applied in
 * lbwn_adam_tf1, so data-parallel ranks can all-reduce raw sums).  Replaces
 * compute_gradients (tmodel.py:354-358).  Must follow lbwn_train_forward on the same
 * workspace/stream.  grads: every pointer of the struct is fully overwritten. */
int lbwn_train_backward(lbwn_plan* plan, const lbwn_params* params, const lbwn_params* grads, void* workspace,
                        const int* wav_q, const int* ids, const float* mel, void* stream);

/* lbwn_train_backward with optional outputs (added after ABI 5 was declared, same ABI: symbols added,
 * none altered).  wav_q, ids and mel are lbwn_train_backward's.
 *   dmel  nullable device fp32 [B][T/hop][n_lc_in], dense, 16-byte aligned, fully overwritten: the
 *         gradient with respect to the mel input of the same quantity as every other gradient of this
 *         call -- Σ masked xent, NOT divided by n_valid, no l2 term.  With dlc [B·T][n_lc_out] the gradient
 *         into the upsample stack's output (the sum of the dlc product's split-K partials),
 *           d(in_i)[t][c] = Σ_{j,o} d(out_i)[s_i·t + j][o]·F_i[j][o][c],  i = nup-1 .. 0,  dmel = d(in_0).
 *         Kernel = stride, so a frame's row depends only on the hop rows of dlc under it: no atomics, a
 *         summation order the shapes alone fix, two calls give the same bits.  A frame that lies wholly
 *         after its stream's last scored position (position t is scored iff ids[b][t+1] != 0) is exactly 0.
 *         Written by the fused upsample backward (plans with "up_fused_bwd") or by one more product after
 *         the per-stage GEMMs; lbwn_plan_info "dmel_fused" says which.  It must not alias mel, the
 *         gradients or the workspace, and is final when the call's work on `stream` is, like the gradients.
 * With dmel NULL the call is lbwn_train_backward: the same launches, the same bits.  The workspace size
 * of every plan is what it was without this call.
 * EINVAL before any launch and before the device is touched, naming the argument: every refusal of
 * lbwn_train_backward (a null plan, params, grads, workspace, wav_q or ids; mel NULL on an LC arch; no
 * training forward on the plan, as after lbwn_train_eval; a GEMM mode changed since the forward); a null
 * a; struct_size != sizeof(lbwn_backward_args); dmel on an arch without LC; dmel not 16-byte aligned;
 * dmel overlapping mel or the workspace. */
typedef struct lbwn_backward_args {
  size_t struct_size;
  const int* wav_q;
  const int* ids;
  const float* mel;
  float* dmel;
} lbwn_backward_args;
int lbwn_train_backward_ex(lbwn_plan* plan, const lbwn_params* params, const lbwn_params* grads, void* workspace,
                           const lbwn_backward_args* a, void* stream);

/* Held-out evaluation of one slice (added after ABI 5 was declared, same ABI: two symbols added, none
 * altered).  Runs lbwn_train_forward's forward up to the raw logits [B·T][n_quant] -- the
 * same launches and the same bits for the same inputs, weights and save: conditioning, D-sep prepend and
 * save, head padding -- then scores the logits without writing a gradient.  params may be any buffer of
 * the layout (the optimizer's EMA shadow, another checkpoint).
 * Scoring (tmodel.py:228-249): position (b, t), t < T-1, has the target c = wav_q[b][t+1] and is scored
 * iff ids[b][t+1] != 0.  Its value is the training head's xent in nats, (max + logf(Σ exp(l - max))) - l[c],
 * and its argmax the first code holding the maximum.  A target outside [0, n_quant) is the caller's error:
 * nothing is read for it and the row's value is its log-sum-exp.
 *   acc     device double[4], required, ADDED to (zero it once per evaluation): [0] Σ value, [1] scored
 *            positions, [2] Σ |argmax - c|, [3] positions with argmax == c.
 *   nll      nullable device fp32 [B][ld_nll], ld_nll >= T: the value, or 0 where not scored and at
 *            t = T-1; columns past T are not touched.
 *   by_voice nullable device double [n_bins][2], ADDED to: [v][0] Σ value, [v][1] count over the scored
 *            positions with v = ids[b][t+1]; ids outside [0, n_bins) are counted in bin 0, which no
 *            scored position otherwise uses.
 *   status   nullable device word: the plan's status word of this call is ORed into it.
 *   save     the evaluation's OWN D-sep state (lbwn_train_forward's layout), read and advanced in place as
 *            in training, so consecutive slices of one deal chain.
 *   scratch  caller-owned, 16-byte aligned, lbwn_train_eval_scratch_bytes(plan, n_bins) bytes (n_bins = 0
 *            without by_voice; 0 for a NULL plan): head partials double [blocks][4] | voice partials double
 *            [ceil(B·T/256)][n_bins][2] | row values fp32 [B·T], each part rounded up to 256 bytes.  The
 *            plan's workspace size is what it was without this call.
 * All sums are formed in double in an order the shapes alone fix (one wave per row, per-block partials,
 * a fixed-order fold; per voice the positions in order inside 256-position chunks, then the chunks in
 * order); no floating-point atomics: two calls on the same inputs add the same bits.
 * Afterwards "logits" holds the raw logits and the plan has no training forward: a lbwn_train_backward
 * that follows is refused (EINVAL); the next lbwn_train_forward works as ever.  n_quant is any multiple of
 * 4 (the 1024 bound is the backward's).  Stream-ordered, no host synchronisation, no allocation.
 * EINVAL before any launch and before the device is touched, naming the argument: a null plan, params,
 * workspace, args, wav_q, ids, save, acc or scratch; struct_size != sizeof(lbwn_eval_args); mel NULL on an
 * LC arch; ld_nll < T with nll; n_bins < 1 with by_voice; acc or by_voice not 8-byte aligned; scratch
 * not 16-byte aligned. */
typedef struct lbwn_eval_args {
  size_t struct_size;
  const int* wav_q;
  const int* ids;
  const float* mel;
  float* save;
  double* acc;
  float* nll;
  int64_t ld_nll;
  double* by_voice;
  int n_bins;
  uint32_t* status;
  void* scratch;
} lbwn_eval_args;
size_t lbwn_train_eval_scratch_bytes(const lbwn_plan* plan, int n_bins);
int lbwn_train_eval(lbwn_plan* plan, const lbwn_params* params, void* workspace, const lbwn_eval_args* a,
                    void* stream);

/* tf.train.AdamOptimizer.apply_gradients (train.py:178, :186), TF1 semantics, over the
 * flat buffers [0, n_total); elements [0, n_weights) are non-BIAS trainables and get the
 * l2 term (tmodel.py:250-261): g = raw·inv_n + l2_factor·θ with inv_n = 1/stats[1]
 * (0 if stats[1] == 0).  counters int64[4]: [0] GLOBAL_STEP, [1] VALID_SAMPLES,
 * [2] Adam applies so far (t-1), [3] cumulative status (every step's status word ORed in,
 * never reset by a step).  lr_t = lr·√(1-β2^t)/(1-β1^t) is derived on device, so the call
 * is graph-capturable.  Then counters advance by (1, n_valid, 1).
 * step_status (nullable): the plan's "status" word of this step (under data parallelism the
 * sum over ranks).  Nonzero means a chain hand-off timed out and the gradients are garbage:
 * the update is skipped on the device (params, m, v and counters[0..2] unchanged) and the
 * word is ORed into counters[3], so the host needs no per-step synchronisation.
 * (ABI 2: step_status added.) */
int lbwn_adam_tf1(float* params, const float* grads, float* m, float* v, int64_t n_weights, int64_t n_total,
                  float lr, float beta1, float beta2, float eps, float l2_factor, const float* stats,
                  int64_t* counters, const uint32_t* step_status, void* stream);

/* The same step with global-norm clipping, a guard against non-finite gradients, an exponential
 * moving average of the weights and a learning-rate schedule, all decided on the device (added
 * after ABI 5 was declared, same ABI: two symbols added, none altered; lbwn_adam_tf1 keeps its
 * kernels and its bits).  struct_size = sizeof(this struct), else EINVAL.  The
 * fields up to step_status mean what lbwn_adam_tf1's arguments mean, with the same refusals.
 *   t      = counters[2] + 1, read on the device: the t of lr_t.
 *   g      the gradient Adam sees: with inv = 1/stats[1] (0 if stats[1] == 0), g = fl(raw·inv),
 *          plus l2_factor·θ on [0, n_weights).
 *   norm   = sqrt(Σ g²) over all n_total elements (tf.global_norm of the total loss's gradients),
 *          summed in double in an order that depends on n_total alone: the same bits on every
 *          device and run, so data-parallel ranks decide alike.  The norm pass (one more launch)
 *          runs iff clip_norm > 0, skip_nonfinite or info != NULL, and then needs ws.
 *   scale  = clip_norm / max(norm, clip_norm) with clipping on, else 1; Adam takes g·scale.
 *   non-finite skip: the norm pass ran, norm is NaN or Inf, and skipping is on (skip_nonfinite, or
 *          implied by clip_norm > 0).  The step is skipped exactly as a timed-out one: params, m,
 *          v, ema and counters[0..2] stay bitwise unchanged.  counters[3] is not touched (it
 *          stays the chain status); instead *nonfinite_skips += 1.  (Squares are formed in
 *          double: finite gradients whose squares overflow fp32 do not skip.)
 *   status skip: a nonzero *step_status skips as in lbwn_adam_tf1, is ORed into counters[3] and
 *          does not count as a non-finite skip.
 *   lr     lr_eff = lr·w·r, in double on the device: w = min(1, t / lr_warmup_steps) with warmup
 *          on, else 1; r = lr_decay_rate^(t / lr_decay_steps) with decay on, else 1, the exponent
 *          floor(t / lr_decay_steps) with lr_decay_staircase (tf.train.exponential_decay with
 *          global_step = t).  Then lr_t = lr_eff·√(1-β2^t)/(1-β1^t).  A skipped step does not
 *          advance t, so the schedule waits with it.
 *   ema    after the element's update, in the same kernel and pass: shadow -= (1 - d_t)·(shadow -
 *          θ_new), d_t = min(ema_decay, (1+t)/(10+t)) with ema_num_updates, else ema_decay
 *          (tf.train.ExponentialMovingAverage with num_updates = t).  The caller initialises the
 *          shadow, from the parameters.
 *   info   (nullable) written by one thread on every call: [0] norm before clipping, [1] the scale
 *          applied, [2] 1 if the step was skipped as non-finite else 0, [3] lr_eff.  On a status
 *          skip [0..2] are 0.
 * As lbwn_adam_tf1, the counters (and the skip count) advance only when stats is given.
 * Stream-ordered, no host synchronisation or allocation, graph-capturable.  With every option
 * neutral (no norm pass, ema_decay 0, no schedule) the call launches what lbwn_adam_tf1 launches.
 * EINVAL before any launch, naming the argument: lbwn_adam_tf1's refusals, a wrong struct_size,
 * clip_norm negative or not finite, ema_decay outside [0, 1), ema NULL or misaligned with
 * ema_decay > 0, ws NULL or misaligned when the norm pass runs, negative step counts,
 * lr_decay_rate outside (0, 1] with decay on. */
typedef struct lbwn_adam_ex_args {
  size_t struct_size;
  float* params; const float* grads; float* m; float* v;
  int64_t n_weights, n_total;
  float lr, beta1, beta2, eps, l2_factor;
  const float* stats; int64_t* counters; const uint32_t* step_status;   /* as lbwn_adam_tf1 */
  float clip_norm;            /* 0 = off; else finite and > 0 */
  int skip_nonfinite;         /* clip_norm > 0 implies it */
  float ema_decay;            /* 0 = off; else in (0, 1) */
  int ema_num_updates;        /* 1: d_t = min(ema_decay, (1+t)/(10+t)); 0: d_t = ema_decay */
  float* ema;                 /* [n_total] shadow, required iff ema_decay > 0, 16-B aligned */
  int64_t lr_warmup_steps;    /* 0 = off */
  int64_t lr_decay_steps;     /* 0 = off */
  float lr_decay_rate;        /* in (0, 1] when lr_decay_steps > 0 */
  int lr_decay_staircase;
  float* ws;                  /* lbwn_adam_ex_ws_floats(n_total) floats, 16-B aligned; required when the norm pass runs */
  float* info;                /* nullable device fp32[4] out */
  int64_t* nonfinite_skips;   /* nullable device counter */
} lbwn_adam_ex_args;
/* Floats of ws for n_total elements (0 for n_total < 1; never shrinks as n_total grows). */
int64_t lbwn_adam_ex_ws_floats(int64_t n_total);
int lbwn_adam_ex(const lbwn_adam_ex_args* a, void* stream);

/* ---- cached autoregressive generation (imodel.WaveNetGen, imodel.py:7-303) ------------ */
typedef struct lbwn_gen_plan lbwn_gen_plan;
/* B streams, outputs for up to max_steps samples, teacher vector up to max_teacher codes.
 * Archs with local conditioning (n_lc_out > 0; ABI 3) take the training plan's limits (1..8
 * upsample stages, strides >= 1, n_lc_in and n_lc_out multiples of 4; else EINVAL) and carve the
 * upsampled mel, the upsample stages' scratch and a ring of projected per-step LC terms of NC
 * steps (default 64; env LBWN_GEN_LC_CHUNK=<integer 1..4096> at plan creation overrides it,
 * anything else is EINVAL).  NC bounds the ring's size (NC·L·B·256 bytes), not the run length.
 * LC plans also carve "pfcond", the projected LC terms of one prefill slice for G consecutive layers
 * (B·T_s·G·2·n_dil floats; G = min(8, L), env LBWN_GEN_PREFILL_LC_GROUP=<integer 1..L> at plan
 * creation overrides it, anything else is EINVAL; plans without LC do not read it and keep their
 * workspace size). */
int lbwn_gen_plan_create(const lbwn_arch* arch, int batch_sz, int64_t max_steps, int64_t max_teacher,
                         lbwn_gen_plan** out);
void lbwn_gen_plan_destroy(lbwn_gen_plan* plan);
size_t lbwn_gen_workspace_bytes(const lbwn_gen_plan* plan);
/* "samples" int32 [B][max_steps] (drawn µ-law codes), "wav" fp32 [B][max_steps]
 * (mu_decode of the draws, imodel.py:181-182), "logits" [B][Q] (last step), "step" int64,
 * "rings" (lookback state, SAVE layout), "teacher" int32, "status" int32 (0; 5 when a persistent
 * hand-off timed out; 6 when lbwn_gen_state_load refused its snapshot or map; 7 when lbwn_gen_extend or
 * lbwn_gen_collect refused its range on the device); ring plans (lbwn_gen_plan_create_ex) size "samples", "wav"
 * and "lc" by their ring instead; LC plans also "lc" fp32, ceil(max_steps/hop)·hop rows per stream reserved
 * ([B][rows][n_lc_out] bytes), of which lbwn_gen_set_mel fills the first B·n_frames·hop rows
 * densely as [B][n_frames·hop][n_lc_out], and "lccond" fp32 [NC][L][B][64] (slot = step mod NC;
 * columns: signal 0..31 | gate 32..63, zero past n_dil) and "pfcond" fp32 [B·T_s][G·2·n_dil], the
 * prefill's scratch (row b·T + j of a slice of T positions, layer l0 + g at column g·2·n_dil: signal
 * n_dil | gate n_dil; what the last projection launch of the last prefill left).  Every plan also has
 * "sessions" int64 [B][4], the words of lbwn_gen_begin (below).  A name the plan does not have is EINVAL. */
int lbwn_gen_tensor(const lbwn_gen_plan* plan, const char* name, size_t* offset, size_t* bytes);
/* Reset the state (zero lookback rings = imodel's zero-initialised buffers, step 0 input =
 * zero vector), load the teacher codes (device int32, may be NULL) and GC ids (device
 * int32 [B], GC archs; imodel.py:53-56).  pre_bias=1 adds PRE_BIAS to the input embedding
 * (tmodel-consistent); 0 reproduces imodel.py:75-77 literally.  Draws use
 * u = splitmix64(seed, stream, step) >> 40 / 2^24 and the inverse softmax CDF (the
 * reference's tf.multinomial, imodel.py:179, is TF-RNG and not reproducible). */
int lbwn_gen_start(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const int* gc_ids,
                   const int* teacher, int64_t n_teacher, uint64_t seed, int pre_bias, void* stream);
/* Load the local conditioning of an LC plan (ABI 3): mel is device fp32 [B][n_frames][n_lc_in];
 * runs the upsample stack of the training plan (transposed convolutions, kernel = stride) once
 * into "lc".  Call after lbwn_gen_start (which clears the loaded state) and before the first
 * lbwn_gen_run.  Generation step i (input: sample i-1, output: sample i) is training position
 * i-1, so it is conditioned on lc row r(i) = min(max(i-1, 0), n_frames·hop - 1): step 0 uses row
 * 0 and steps past the mel reuse its last row.  EINVAL before any launch when the arch has no
 * LC, mel is NULL, n_frames < 1 or n_frames·hop exceeds the plan's rows. */
int lbwn_gen_set_mel(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const float* mel,
                     int64_t n_frames, void* stream);
/* Generate n_steps more samples for every stream (the tf.while_loop body, imodel.py:214-272).
 * Device-resident step counter: the launches are graph-capturable and replayable.  Persistent
 * plans (lbwn_gen_is_persistent) run the whole call as ONE launch whose blocks must all be
 * resident: nothing else may occupy the device's CUs meanwhile.  LC plans split the call into
 * sub-runs of <= NC steps, each a projection launch (the sub-run's LC terms into "lccond") followed
 * by the step launches (persistent plans: one persistent launch per sub-run); EINVAL before any
 * launch when no mel is loaded or, after a lbwn_gen_begin, while a stream has begun no session. */
int lbwn_gen_run(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, int n_steps, void* stream);
/* 1 when the plan runs the persistent one-launch form (groups of <= 16 streams, each with its
 * own 32 head blocks, while every block fits on the device: B <= 80 on 256 CUs; layer/head sizes fit;
 * LBWN_GEN_PERSIST=0 at plan creation selects the per-step launches), else 0. */
int lbwn_gen_is_persistent(const lbwn_gen_plan* plan);
/* Advance every stream by n steps whose inputs are already known, in parallel over the n positions
 * (ABI 5; the state n teacher-forced lbwn_gen_run steps leave, computed as a training-style forward).
 * codes: device int32, stream b's j-th code at codes[b*ld_codes + j], j < n; ld_codes == 0: one
 * vector shared by all streams (the reference's teacher_vec).
 * With t0 the device step counter at the call, step t0 takes the pending input (the previous draw or
 * prefilled code; the zero vector right after lbwn_gen_start) and step t0+j, j >= 1, takes
 * codes[b][j-1]; PRE_BIAS is added as lbwn_gen_start's pre_bias says.  Afterwards every layer's ring
 * holds x_l of the last min(d_l, t0+n) steps (slot t mod d_l), the pending input is codes[b][n-1], and
 * the step counter (every persistent stream group's included) is t0+n.  For t0+j < max_steps,
 * "samples"[b][t0+j] = codes[b][j] and "wav" its mu-law decode: the output holds the prompt followed by
 * the continuation.  (On purpose unlike the teacher vector of lbwn_gen_start, whose steps store the
 * model's ignored draws there.)  "logits" is not touched.  The uniform of step t stays
 * splitmix64(seed, stream, t), so lbwn_gen_start without a teacher + prefill(c, n) + run(k) draws at
 * steps n..n+k-1 what lbwn_gen_start(teacher = c, n) + run(n+k) draws there, up to fp32 rounding of
 * the logits (a draw can differ only at a near tie of the CDF).
 * LC plans (widened after ABI 5 was declared, same ABI: no signature or symbol changed): step t0+j is
 * conditioned on lc row r(t0+j) of lbwn_gen_set_mel, r(i) = min(max(i-1, 0), n_frames·hop - 1), as
 * the same step of lbwn_gen_run is; GC and LC terms add.  Per slice and per G layers one launch
 * projects the slice's lc rows on the f32 matrix cores into "pfcond"; t0 and the loaded row count are
 * read on the device, so a captured prefill follows a mel loaded later.  Call after lbwn_gen_set_mel.
 * Stream-ordered, no host synchronisation or allocation, graph-capturable (t0 is read on the device);
 * may be called at t0 = 0 or in the middle of a run, any number of times.  The positions are
 * processed in slices of T_s = the largest multiple of 128 with batch_sz*T_s <= 32768 (at least 128;
 * env LBWN_GEN_PREFILL_SLICE=<integer 1..65536> at plan creation overrides it, anything else is
 * EINVAL there); the scratch, carved at plan creation, does not grow with n.
 * EINVAL before any launch: a null argument, n < 1, ld_codes neither 0 nor >= n, an LC plan with no
 * mel loaded since lbwn_gen_start, batch_sz*T_s*n_res >= 2^31.  Codes outside [0, n_quant) are the caller's error; they
 * are clamped into it. */
int lbwn_gen_prefill(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const int* codes,
                     int64_t ld_codes, int64_t n, void* stream);
/* Teacher-forced scoring: log p(code | history) of a known waveform under the model, per step and per
 * stream (added after ABI 5 was declared, same ABI: two symbols added, none altered).
 * codes, ld_codes and n are lbwn_gen_prefill's.  With t0 the device step counter at the call, step t0+j
 * takes the input lbwn_gen_prefill gives it (the pending input for j = 0, codes[b][j-1] after that), and
 * its logits l_j are those lbwn_gen_run would compute at that step (the same GC term, LC row r(t0+j) and
 * pre_bias).  logp[b*ld_logp + j] = l_j[c] - logsumexp(l_j), c = codes[b][j] clamped into [0, n_quant):
 * the natural log of the probability of the code the prompt holds at that step.  The sampling settings
 * (lbwn_gen_set_sampling) do not enter it.  All n positions of all batch_sz streams are written; logp is
 * device fp32, ld_logp >= n, columns past n are not touched.
 * State: the call changes the state exactly as lbwn_gen_prefill(codes, ld_codes, n) does -- rings,
 * pending code, step counter and the persistent groups' counters are bitwise those of a prefill of the
 * same codes on the same plan, "samples" / "wav" hold the prompt over the scored steps -- and in addition
 * leaves "logits" = l_{n-1} for every stream.  To score without advancing, wrap the call in
 * lbwn_gen_state_save / lbwn_gen_state_load.
 * Per slice of T_s positions (lbwn_gen_prefill's slices, LBWN_GEN_PREFILL_SLICE included) the layers write
 * their gate outputs side by side into Zcat [B·T][L·n_dil]; the head is lbwn_gen_run's three GEMMs over
 * those rows (skip as one product with K = L·n_dil, post1, post2), then one wave per row forms the
 * log-softmax gather.
 * scratch: caller-owned device memory, 16-byte aligned, lbwn_gen_score_scratch_bytes(plan) bytes (0 for a
 * NULL plan): Zcat [R][L·n_dil] | S [R][n_skip] | H [R][n_post] | LG [R][n_quant] fp32 with R =
 * batch_sz·T_s rows, each part rounded up to 256 bytes.  It does not depend on n or max_steps; the plan's
 * workspace is what it was without this call.
 * Stream-ordered, no host synchronisation or allocation, graph-capturable (t0 is read on the device); at
 * t0 = 0 or in the middle of a run, any number of times.
 * EINVAL before any launch, naming the argument: every refusal of lbwn_gen_prefill; logp or scratch NULL;
 * scratch not 16-byte aligned; ld_logp < n; n_skip, n_post, n_quant or L·n_dil not a multiple of 4, SKIP /
 * POST1 / POST2 NULL or not 16-byte aligned (what the GEMMs take); batch_sz*T_s*max(L·n_dil, n_skip,
 * n_post, n_quant) >= 2^31. */
size_t lbwn_gen_score_scratch_bytes(const lbwn_gen_plan* plan);
int lbwn_gen_score(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const int* codes,
                   int64_t ld_codes, int64_t n, float* logp, int64_t ld_logp, void* scratch, void* stream);
/* Temperature, top-k and nucleus (top-p) filtering of the draw (added after ABI 5 was declared, same
 * ABI: two symbols added, none altered -- the convention of the LC widening of lbwn_gen_prefill).
 * With l a stream's logits at a step (the values "logits" holds, which stays raw):
 *  1. top_k (0 = off): keep the codes whose logit is >= the k-th largest logit; ties with the k-th are
 *     kept; top_k >= n_quant is normalised to 0.
 *  2. temperature T (finite, > 0; 1 = off): e_c = exp((l_c - max l) / T) for kept codes, 0 otherwise.
 *     Greedy decoding is top_k = 1.
 *  3. top_p (0 < p <= 1; 1 = off), applied after top-k: order the kept codes by e, descending; keep the
 *     shortest prefix whose mass is >= p·Σe, plus every code whose e equals that prefix's last member;
 *     all others get e = 0.
 *  4. The draw is lbwn_gen_start's, over the surviving e in code order: the first code with
 *     cumsum(e) > u·Σe, u = splitmix64(seed, stream, step) >> 40 / 2^24.  The µ-law decode, "samples",
 *     "wav", the pending input and the teacher override are unchanged: a teacher-forced step stores the
 *     filtered draw and feeds the teacher's code.  lbwn_gen_prefill draws nothing and is not affected.
 * Plan host state like the seed: (1, 0, 1) at plan creation, kept across lbwn_gen_start, read by each
 * later lbwn_gen_run when it launches -- so a captured graph bakes in the values of its capture; capture
 * again after changing them.  No launch, no device access, no workspace: the workspace size does not
 * depend on it.  The neutral triple (1, 0, 1) launches the unfiltered kernels: draws are bitwise what
 * they were without this call.  Otherwise the same launches run a filtered form of the draw (wave-level
 * bisection on the logit and e bit patterns, <= 32 + 30 short rounds per draw).
 * EINVAL, naming the argument, and nothing changed: plan NULL, temperature not finite or <= 0,
 * top_k < 0, top_p NaN, <= 0 or > 1. */
int lbwn_gen_set_sampling(lbwn_gen_plan* plan, float temperature, int top_k, float top_p);
/* The plan's normalised values (a top_k >= n_quant reads back as 0); NULL outputs are skipped.
 * EINVAL when plan is NULL. */
int lbwn_gen_get_sampling(const lbwn_gen_plan* plan, float* temperature, int* top_k, float* top_p);
/* Save, restore and fan out the state of a run (added after ABI 5 was declared, same ABI: three symbols
 * added, none altered).  Between two launches a run is the lookback rings, every stream's
 * pending input code, the step counter and the persistent stream groups' copies of it; the rest of the
 * workspace is recomputed by every launch or set by lbwn_gen_start / _set_mel / _set_sampling.
 * The snapshot is caller-owned device memory, 16-byte aligned, not overlapping the workspace, and
 * stream-major, so it does not depend on the batch size of the plan that wrote it:
 *   header, 256 bytes: int32 magic 0x5453424c ("LBST"), layout version 1, n_streams, n_blocks,
 *     n_block_layers, n_res, n_quant, record_bytes; int64 step at byte 32; the rest zero;
 *   n_streams records of record_bytes = round_up_16(16 + 4·D·n_res), D = n_blocks·(2^n_block_layers - 1):
 *     the pending code (int32; -1: the zero vector after lbwn_gen_start), 12 zero bytes, then the stream's
 *     rings in layer order, layer (block, bl) with d = 2^bl as fp32 [d][n_res], slot = step mod d; zero
 *     bytes up to record_bytes.
 * lbwn_gen_state_bytes: 256 + n_streams·record_bytes; 0 for a NULL plan or n_streams < 1.
 * lbwn_gen_state_save writes all batch_sz streams (one launch; the step is read on the device) and
 * changes nothing in the workspace.
 * lbwn_gen_state_load must follow lbwn_gen_start on this workspace (which supplies the packed images, GC
 * projections, seed, pre_bias and teacher; LC plans also load the mel with lbwn_gen_set_mel before the
 * next run).  Stream b takes record src_stream[b] (device int32 [batch_sz], entries in
 * [0, state_streams); several streams may take one record; NULL = identity, state_streams == batch_sz).
 * Afterwards the rings and pending codes are the records', the step counter and every persistent group's
 * are the header's step, and every hand-off granule is zero (a granule left by the run that was here could
 * carry the tag the loaded step polls for).  "samples", "wav", "logits", "teacher", "lc", "status" and all
 * host state are untouched.  The uniform of a draw stays splitmix64(seed, destination stream, step): an
 * identity load continues exactly as the saved run did, two streams loaded from one record continue
 * differently.  A captured lbwn_gen_run stays valid across a load (it reads the step on the device).
 * Both are stream-ordered, without host synchronisation or allocation, and graph-capturable.
 * EINVAL before any launch, naming the argument: plan, workspace or state NULL, state not 16-byte
 * aligned, state_streams < 1, src_stream NULL with state_streams != batch_sz.  The header is device
 * memory, so the load's launch checks it before it writes: magic, version, n_blocks, n_block_layers,
 * n_res, n_quant and record_bytes against the plan, n_streams against state_streams, 0 <= step <=
 * max_steps, every map entry in range.  On a mismatch "status" becomes 6 and nothing else in the
 * workspace changes; lbwn_gen_start clears it.  A nonzero status does not stop a lbwn_gen_run on a plan without
 * a ring (it only makes the persistent form's spinning hand-offs give up): check "status" before trusting what
 * follows.  On a ring plan (below) a lbwn_gen_run takes no step while the status is nonzero. */
size_t lbwn_gen_state_bytes(const lbwn_gen_plan* plan, int n_streams);
int lbwn_gen_state_save(const lbwn_gen_plan* plan, const void* workspace, void* state, void* stream);
int lbwn_gen_state_load(lbwn_gen_plan* plan, void* workspace, const void* state, int state_streams,
                        const int* src_stream, void* stream);
/* Sessions: begin a new utterance in single streams between two lbwn_gen_run calls while the other
 * streams continue (added after ABI 5 was declared, same ABI: one symbol added, none altered; DESIGN
 * §4.29).  With t0 the device step counter at the call (read on the device), every listed stream b = slot
 * is afterwards in the state lbwn_gen_start leaves a stream in -- zero rings, the zero vector as pending
 * input (code -1), PRE_BIAS as lbwn_gen_start's pre_bias says -- and in addition has
 *   a step origin and a draw key: base_b = t0, key_b = key.  Its local step at absolute step t is
 *     i = t - base_b and its uniform splitmix64(seed, key_b, i) >> 40 / 2^24: an utterance draws the same
 *     whichever stream carries it and whenever it starts.  lbwn_gen_start stands for base_b = 0, key_b = b.
 *   GC archs: its rows of the GC projection table recomputed from gc_id, bitwise what lbwn_gen_start
 *     writes for that id.
 *   LC archs: its own mel, run through the plan's upsample stack (the fused launch inside its envelope,
 *     else one GEMM per stage) into the stream's own region of "lc", which in this mode is
 *     [B][reserved rows][n_lc_out]; local step i is conditioned on local row min(max(i - 1, 0),
 *     n_frames·hop - 1), lbwn_gen_set_mel's rule per session.
 * "samples" and "wav" stay [B][max_steps] indexed by the absolute step: a session's j-th sample is column
 * base_b + j.  The other streams, their "logits", the step counter, "status", the hand-off granules and the
 * sampling settings are untouched.  On a plan without a ring a run does not outlive max_steps: size it for
 * the whole schedule, or make a ring plan (lbwn_gen_plan_create_ex below), whose columns are i mod R.
 * The words live in "sessions", int64 [B][4] = {base, key, rows = n_frames·hop, 0}: the last 32·B bytes
 * (rounded up to 256) of the workspace, over the tail of the prefill scratch, so the workspace size of a
 * plan is what it was (a plan whose prefill scratch is smaller than the words grows by the difference).
 * Their content is defined from the first begin after lbwn_gen_start, which also writes {0, b, 0, 0} for the
 * streams it does not list.  Until that begin the draw and the projection take no table: the kernels
 * launched and the bits drawn are those of a build without this call.
 * One call is one reset-and-GC launch for all listed streams (one per 128 of them) plus each stream's
 * upsample launches; stream-ordered, no allocation, no host synchronisation.  s is host memory, read at
 * the call; each mel is device memory that must stay valid until its upsample launches have run.
 * A captured lbwn_gen_run is bound to the mode it was captured in, in both directions: the capture bakes in
 * whether the draw and the LC projection take the words.  One captured in session mode (after the first
 * begin) stays valid across later begins, whose words are read on the device, but must not be replayed
 * after a lbwn_gen_start until a begin has put the run back into session mode; one captured on the dense
 * path must not be replayed after a begin.  Replaying across a mode change raises no error: it draws and
 * projects from the wrong words.  Capture again instead.
 * Modes between two lbwn_gen_start calls: on LC plans lbwn_gen_set_mel and lbwn_gen_begin exclude each
 * other (EINVAL for the later one), and after a begin lbwn_gen_run is EINVAL until every stream has begun a
 * session.  Plans without LC may begin any subset at any time.  lbwn_gen_prefill and lbwn_gen_score are
 * EINVAL after a begin: both stay whole-batch operations (and they overwrite "sessions").
 * lbwn_gen_state_save / _load work as documented and do not carry the words: an identity rewind with no
 * begin in between repeats the run.
 * EINVAL before any launch, naming the argument: a null plan, params, workspace or s; struct_size !=
 * sizeof(lbwn_gen_session); n < 1 or n > batch_sz; a teacher loaded by lbwn_gen_start (n_teacher > 0: the
 * override is keyed by the absolute step); a slot outside [0, batch_sz) or listed twice; a key outside
 * [0, 2^31); gc_id outside [0, n_gc_category] on a GC arch (ignored without GC); on an LC arch mel NULL
 * or not 16-byte aligned, n_frames < 1 or n_frames·hop beyond the plan's reserved rows; mel non-NULL on
 * an arch without LC. */
typedef struct lbwn_gen_session {
  int slot;          /* stream index in [0, batch_sz) */
  int gc_id;         /* GC archs: voice id in [0, n_gc_category]; ignored without GC */
  int64_t key;       /* the draw's stream key, 0 <= key < 2^31 */
  const float* mel;  /* LC archs: device fp32 [n_frames][n_lc_in], 16-B aligned; must be NULL without LC */
  int64_t n_frames;  /* LC archs: >= 1, n_frames*hop <= the plan's reserved rows; 0 without LC */
} lbwn_gen_session;
int lbwn_gen_begin(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const lbwn_gen_session* s,
                   int n, size_t struct_size, void* stream);
/* Ring plans: outputs and conditioning addressed by the session's local step modulo a capacity chosen at
 * plan creation, so the workspace does not depend on how long the process runs (added after ABI 5 was
 * declared, same ABI: three symbols added, none altered).
 * lbwn_gen_plan_create_ex with ring_steps == 0 is lbwn_gen_plan_create(arch, batch_sz, max_steps,
 * max_teacher, out): the same workspace, kernels and bits.  ring_steps = R >= 1 makes a ring plan:
 *   "samples" and "wav" are [B][R]; the sample of a stream's local step i = t - base_b lies in column
 *     i mod R (base_b = 0 until a lbwn_gen_begin, as lbwn_gen_start stands for).  Every step stores; no
 *     step is dropped for lying past max_steps, which a ring plan ignores (for the snapshot check
 *     0 <= step <= max_steps of lbwn_gen_state_load it is unbounded).  The step counter is bounded by
 *     int64 only: a run has no end, and nothing needs sizing for the schedule.
 *   LC plans: "lc" is [B][Rlc][n_lc_out], Rlc = ceil(R/hop)·hop (< 2^31), and the upsample stages' scratch
 *     holds Rlc/hop frames per stream.  In session mode local row r of a stream lies at row r mod Rlc of
 *     its own region; a lbwn_gen_begin may bring at most Rlc/hop frames (more come by lbwn_gen_extend).
 *     lbwn_gen_set_mel keeps its dense layout [B][n_frames·hop][n_lc_out] and its bound n_frames·hop <=
 *     Rlc, under which r mod Rlc = r.
 *   lbwn_gen_workspace_bytes does not depend on max_steps; lbwn_gen_tensor reports the sizes above.
 *   EINVAL on a ring plan, before any launch: lbwn_gen_prefill and lbwn_gen_score (both stay whole-batch
 *     operations over absolute steps), a teacher (lbwn_gen_start with n_teacher > 0: the override is keyed
 *     by the absolute step), and lbwn_gen_state_load in session mode on an LC plan (below).
 * EINVAL from lbwn_gen_plan_create_ex: arch, args or out NULL, struct_size != sizeof(lbwn_gen_plan_args),
 * ring_steps < 0, Rlc >= 2^31, and every refusal of lbwn_gen_plan_create.
 *
 * lbwn_gen_extend appends n_frames more mel frames to the live session of each listed stream: the plan's
 * upsample stack (as in lbwn_gen_begin) into local rows [rows_b, rows_b + n_frames·hop) of the stream's
 * region -- on a ring plan in at most two pieces where the range wraps; hop divides Rlc, so no frame
 * straddles the wrap -- and rows_b += n_frames·hop in the session words, on the device.  The plan keeps a
 * host mirror of every slot's row count for the destination (lbwn_gen_begin and lbwn_gen_extend are its
 * only writers; lbwn_gen_start clears it; it is advanced with each check launch, so it equals the row words
 * of every run that the device has not refused).  On a plan without a ring the bound is the reserved rows (EINVAL
 * from the mirror).  On a ring plan the rows a stream has already read are known on the device only (a
 * captured lbwn_gen_run replays without the host), so the call's first launch checks there: with i the
 * stream's local step and r = min(max(i - 1, 0), rows_b) the row that step reads (rows_b: every row given
 * so far is behind it), rows_b + n_frames·hop - r > Rlc sets "status" to 7 and advances no row word of that
 * launch (neither does a launch that finds the status nonzero already).  The upsample launches of a refused
 * call still run (the host cannot see the refusal) and may overwrite unread rows; the run is dead anyway:
 * on a ring plan a lbwn_gen_run takes no step (the counter stays, nothing is drawn) while the status is
 * nonzero, in both execution forms, until lbwn_gen_start clears it (a plan without a ring runs on, as after
 * status 6: check "status").
 * One check-and-advance launch per call (one per 128 streams) plus each piece's upsample launches;
 * stream-ordered, no allocation, no host synchronisation; valid between replays of a captured lbwn_gen_run.
 * EINVAL before any launch, naming the argument: plan, params, workspace or e NULL; struct_size !=
 * sizeof(lbwn_gen_extend_entry); n < 1 or n > batch_sz; an arch without LC; a slot outside [0, batch_sz),
 * listed twice or whose stream has begun no session since lbwn_gen_start; mel NULL or not 16-byte aligned;
 * n_frames < 1; n_frames·hop beyond Rlc (ring) or rows_b + n_frames·hop beyond the reserved rows (no ring).
 *
 * lbwn_gen_collect copies local steps [i0, i0 + n) of stream `slot` out of "wav" and "samples" into dense
 * caller buffers (device memory; either may be NULL), one launch.  The stream's base and the step counter
 * are read on the device: with e = step - base_b the local steps already run, the range must satisfy
 * i0 + n <= e and, on a ring plan, i0 >= e - R (not yet overwritten); on a plan without a ring, base_b + i0
 * + n <= max_steps.  Otherwise "status" becomes 7 and nothing is written.  Without a ring it is the same
 * copy without the wrap.  EINVAL before any launch: plan or workspace NULL, slot outside [0, batch_sz),
 * i0 < 0, n < 0, both outputs NULL (n == 0 launches nothing).
 *
 * lbwn_gen_state_save / _load on a ring plan: as documented, the session words are not carried, and neither
 * is the host row mirror.  An identity rewind (save, run, load, run, no begin or extend in between) repeats
 * the run bit for bit, "samples" and "wav" columns included, when the plan has no LC, is on the
 * lbwn_gen_set_mel path, or is not a ring plan.  On a ring LC plan in session mode the rows the rewound
 * steps read may have been overwritten by later extends and the mirror would be ahead of the words, so
 * lbwn_gen_state_load is EINVAL there. */
typedef struct lbwn_gen_plan_args {
  size_t struct_size;   /* sizeof(lbwn_gen_plan_args) */
  int batch_sz;
  int64_t max_steps;    /* as lbwn_gen_plan_create; ignored by a ring plan (>= 1 all the same) */
  int64_t max_teacher;
  int64_t ring_steps;   /* 0: no ring (lbwn_gen_plan_create); R >= 1: a ring plan */
} lbwn_gen_plan_args;
int lbwn_gen_plan_create_ex(const lbwn_arch* arch, const lbwn_gen_plan_args* args, lbwn_gen_plan** out);
typedef struct lbwn_gen_extend_entry {
  int slot;          /* stream index in [0, batch_sz), with a live session */
  const float* mel;  /* device fp32 [n_frames][n_lc_in], 16-B aligned: the frames after those already given */
  int64_t n_frames;  /* >= 1 */
} lbwn_gen_extend_entry;
int lbwn_gen_extend(lbwn_gen_plan* plan, const lbwn_params* params, void* workspace, const lbwn_gen_extend_entry* e,
                    int n, size_t struct_size, void* stream);
int lbwn_gen_collect(lbwn_gen_plan* plan, void* workspace, int slot, int64_t i0, int64_t n, float* wav_out,
                     int* samples_out, void* stream);

/* ---- log-mel front end: wav to the LC conditioning, one launch (added after ABI 5 was declared, same
 * ABI: symbols added, none altered) ----
 * The reference made its mels offline with librosa (data.py:143 keeps len(wav) == len(mel)·hop); this is
 * that transform on the device.  For a mono signal x[0..n) per stream:
 *   frames  F = n / hop (a tail shorter than a hop is dropped); frame t is centred at sample t·hop: its
 *           sample k < n_fft is x~[t·hop + k - n_fft/2] with reflect padding that does not repeat the edge
 *           (x~[i] = x[-i] for i < 0, x[2(n-1) - i] for i >= n).  n > n_fft/2 (one reflection) and F >= 1.
 *   window  periodic Hann of win_length, w[j] = 0.5 - 0.5·cos(2πj/win_length), zero-padded centrally
 *           (left pad (n_fft - win_length)/2) to n_fft.
 *   P[k]    = |Σ_j w[j]·frame[j]·e^(-2πi·jk/n_fft)|^power, k = 0..n_fft/2.
 *   M[j]    = Σ_k P[k]·fb[k][j]: triangles over n_mels + 2 points equally spaced on the mel scale between
 *           fmin and fmax (Slaney: linear below 1 kHz at 200/3 Hz per mel, log above with step ln(6.4)/27;
 *           htk = 1: 2595·log10(1 + f/700)); weight of bin frequency f = k·sample_rate/n_fft in band j:
 *           max(0, min((f - p_j)/(p_j+1 - p_j), (p_j+2 - f)/(p_j+2 - p_j+1))), times 2/(p_j+2 - p_j) with
 *           norm = 1.  Built on the host in double, rounded once to f32.
 *   out     ln(max(M, log_floor)) with log_floor > 0, the linear M with log_floor = 0; fp32 [B][F][n_mels].
 * lbwn_mel_plan_create is host-only (no GPU needed).  struct_size = sizeof(lbwn_mel_cfg), else EINVAL.
 * EINVAL naming the argument: n_fft not a multiple of 32 in [64, 2048]; hop not a multiple of 4 in
 * [4, n_fft]; win_length outside [2, n_fft]; n_mels not a multiple of 4 in [4, 128]; not 0 <= fmin < fmax
 * <= sample_rate/2; power not 1 or 2; log_floor negative or not finite; a filterbank with an empty band
 * (an all-zero column); a frame tile (64 frames, else 32: (rows-1)·hop + n_fft samples) beyond the device's
 * 160 KiB of LDS.
 * lbwn_mel_frames: F for a signal of n_samples, 0 when the length is refused.
 * lbwn_mel_workspace_bytes: the tables (the windowed DFT basis and the filterbank); independent of the
 * signal length.  The workspace is caller-owned device memory, 256-byte aligned.
 * lbwn_mel_filterbank: the [n_fft/2+1][n_mels] f32 filterbank to host memory; touches no device.
 * lbwn_mel_init: fills the tables (one launch and one copy from plan-owned host memory) and raises the
 * forward kernel's dynamic-LDS limit on the current device, so that lbwn_mel_forward is the launch alone;
 * once per workspace (hence at least once per device and process before the first forward there); the
 * plan must outlive the copy; not graph-capturable.  The tables depend on the configuration alone: two
 * workspaces hold the same bits.
 * lbwn_mel_forward: stream b < batch is read at wav + b·ld_wav (n_samples floats) and its F rows are
 * written densely [F][n_mels] at out + b·ld_out_stream; nothing else is read or written.  One launch,
 * stream-ordered, no allocation or synchronisation, graph-capturable, deterministic (no float atomics;
 * a stream's rows do not depend on the batch).  EINVAL before any launch: a null argument, wav or out not
 * 16-byte aligned, ld_wav not a multiple of 4 or (batch > 1) < n_samples, ld_out_stream < F·n_mels
 * (batch > 1), batch outside [1, 65535], n_samples that lbwn_mel_frames refuses. */
typedef struct lbwn_mel_cfg {
  size_t struct_size;
  int sample_rate, n_fft, win_length, hop, n_mels;
  float fmin, fmax;
  int power, htk, norm;
  float log_floor;
} lbwn_mel_cfg;
typedef struct lbwn_mel_plan lbwn_mel_plan;
int lbwn_mel_plan_create(const lbwn_mel_cfg* cfg, lbwn_mel_plan** out);
void lbwn_mel_plan_destroy(lbwn_mel_plan* plan);
int64_t lbwn_mel_frames(const lbwn_mel_plan* plan, int64_t n_samples);
size_t lbwn_mel_workspace_bytes(const lbwn_mel_plan* plan);
int lbwn_mel_filterbank(const lbwn_mel_plan* plan, float* host_out);
int lbwn_mel_init(const lbwn_mel_plan* plan, void* workspace, void* stream);
int lbwn_mel_forward(const lbwn_mel_plan* plan, const void* workspace, const float* wav, int64_t ld_wav, int batch,
                     int64_t n_samples, float* out, int64_t ld_out_stream, void* stream);

/* ---- fine-grained kernels (parity tests, custom drivers) ------------------------------ */
/* ops.mu_encode_np (ops.py:23-28, tf32=0, float64 math) / ops.mu_encode (ops.py:4-9, tf32=1) */
int lbwn_mulaw_encode(const float* x, int* q, int64_t n, int n_quanta, int tf32, void* stream);
/* ops.mu_decode (ops.py:12-20) */
int lbwn_mulaw_decode(const int* q, float* x, int64_t n, int n_quanta, void* stream);

/* GEMM arithmetic for every lbwn 1x1 product (process-wide; not a reference interface).
 * mode 1 (default): f32 operands split exactly into three bf16 terms, six cross products on
 * the bf16 matrix cores, f32 accumulation (f32-class error, tests/test_gpu_parity.py
 * ::test_gemm_split_accuracy).  mode 0: v_mfma_f32_32x32x2_f32.  Env LBWN_GEMM=f32 sets 0. */
int lbwn_gemm_set_mode(int mode);
int lbwn_gemm_get_mode(void);

/* ops.conv1x1 and every 1x1 product (ops.py:41-55): C[M][N] = epi(A·B).
 * a_kcontig: A stored A[m*lda+k] (else A[k*lda+m]); b_kcontig: B stored B[n*ldb+k]
 * (else B[k*ldb+n]).  Epilogue: +bias[n], relu, zero where mask[m*ldm+n] <= 0, += C.
 * relu_a applies relu to A on load.  split_k > 1 needs slab_ws of split_k·M·N floats. */
int lbwn_gemm_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb, int b_kcontig,
                  float* C, int64_t ldc, int M, int N, int K, const float* bias, int relu_a, int relu_out,
                  const float* mask, int64_t ldm, int accumulate, int split_k, float* slab_ws, void* stream);

/* The same product with B given ALSO as pre-split bf16 planes b3 (lbwn_split_planes of B with
 * rows = N: trans = 0 for B[n*ldb+k], 1 for B[k*ldb+n]), the form the training step uses for its
 * weight operands; no split-K.  B stays required for the f32 mode (mode 0 ignores b3).
 * b3 must be 16-byte aligned (else EINVAL) and hold lbwn_split_planes_elems_abi(N, K) elements. */
int lbwn_gemm_f32_presplit(const float* A, int64_t lda, int a_kcontig, const uint16_t* b3, int N, const float* B,
                           int64_t ldb, int b_kcontig, float* C, int64_t ldc, int M, int K, const float* bias,
                           int relu_a, int relu_out, const float* mask, int64_t ldm, int accumulate, void* stream);
/* Exact three-term bf16 split of a weight, out[r][K/32][3][32] (K rounded up to 32, zero-filled):
 * W[r*ldw+k] (trans = 0) or W[k*ldw+r] (trans = 1), r < rows. */
int64_t lbwn_split_planes_elems_abi(int rows, int K);
int lbwn_split_planes(const float* W, int64_t ldw, int rows, int K, int trans, uint16_t* out, void* stream);

/* The same product with every option of the step's GEMM launcher (ABI 4; for parity tests of the
 * kernel forms and epilogues the two entries above cannot reach).  struct_size = sizeof(this struct)
 * (else EINVAL); unused fields are zero.  A / B / C, strides, a_kcontig / b_kcontig, bias, mask,
 * relu_a, relu_out, accumulate, split_k / slab_ws and b3 are those of lbwn_gemm_f32[_presplit]
 * (b3 may be NULL: B is then split on the fly).  The rest, all optional, bf16-split mode only:
 *   colpart   fp32 [ceil(M/256)][N] out: column sums of the final C per 256-row block (no split-K);
 *             lbwn_colpart_parts_abi(M) rows.
 *   step_advance  int64 device counter, +1 per launch.
 *   c_chain_ls > 0: C in the backward chain's order instead of rows (ldc unused): 32-column block j
 *             at C + j*c_chain_ls, element (m, c) of it at
 *             ((((m >> 5)*4 + ((c >> 3) & 3))*32 + (m & 31))*8 + (c & 7)); needs N % 32 == 0,
 *             c_chain_ls >= ceil(M/32)*1024, no split-K / accumulate / mask, and on the x3q forms
 *             no bias / relu_out / mask bits either.
 *   xcd2d     x3q<10> only: 2-D placement of the tiles over the XCDs (same values).
 *   a_kstride A k-contiguous, lda = 32, K % 32 == 0: element (m, k) at A[m*32 + (k/32)*a_kstride + k%32].
 *   b_gstride B n-contiguous, ldb = 32, no b3: element (k, n) at B[k*32 + (n/32)*b_gstride + n%32].
 *   a_gstride A m-contiguous, lda = 32 (the x3q<6 / 8,amn> forms only, M >= 256, no bias / mask):
 *             element (m, k) at A[k*32 + (m/32)*a_gstride + m%32].
 *   row_exact every row is computed by the tall form whatever M is (a row's value depends only on
 *             its own A row).
 *   mbits_out / mbits  x3q<8> only, no split-K: uint64 [lbwn_gemm_mbits_words_abi(M, N)], bit =
 *             (final C > 0) written by a producer; a consumer of the same shape and form masks by it.
 *   row_live  x3q<8> / x3q<10> only, no split-K: int32 [ceil(M/256)], 0 = every A row of that
 *             256-row tile is exactly zero (the tile skips its k-loop).
 *   k_live / nk_live / k_pre  both operands mn-contiguous, K % 32 == 0, no b3: the ascending list of
 *             the 32-deep k-steps whose B rows are not all zero, its length (int32[1]) and
 *             k_pre[k] = number of list entries below k-step k (int32 [K/32 + 1]).
 *   splits_deferred  host int out (nullable): the split-K partials stay unsummed in slab_ws
 *             ([splits][M][N]) and the split count actually used is stored here (1: C was written);
 *             plain products only.
 * Combinations the chosen kernel would not honour are refused with EINVAL before any launch.
 * (Not exposed: the one-hot A operand lbwn_gemm_args::a_codes.) */
typedef struct lbwn_gemm_ex_args {
  size_t struct_size;
  const float* A; const float* B; float* C;
  int64_t lda, ldb, ldc;
  int M, N, K;
  int a_kcontig, b_kcontig, split_k;
  float* slab_ws;
  const float* bias; const float* mask;
  int64_t ldm;
  int relu_a, relu_out, accumulate, xcd2d;
  const uint16_t* b3;
  float* colpart;
  int64_t* step_advance;
  int64_t c_chain_ls, a_kstride, b_gstride, a_gstride;
  uint64_t* mbits_out; const uint64_t* mbits;
  const int* row_live; const int* k_live; const int* nk_live; const int* k_pre;
  int* splits_deferred;
  int row_exact, reserved;
} lbwn_gemm_ex_args;
int lbwn_gemm_ex(const lbwn_gemm_ex_args* a, void* stream);
/* The kernel instantiation the most recent GEMM launch on this thread chose ("" when that call was
 * refused before a launch; the string is static).  bf16-split mode:
 *   "x3q<8>" "x3q<10>" "x3q<6>"                     A in registers, 256 x 128 / 160 / 96 tiles
 *   "x3q<8,amn>" "x3q<8,amn,kl>" "x3q<6,amn>"       their weight-gradient forms (kl: over k_live)
 *   "x3<A,B,K,W>"   LDS-staged: A = akc | amn, B = bkc | bmn | pre (b3), K = kfull (K % 32 == 0) |
 *                   kany, W = wm2 (128-row tiles) | wm4 (256-row: row_exact, M >= 8192 or colpart)
 *   "x3<kl>"        the 128-row form over k_live
 * f32 mode: "f32<A,B>" with A = akc | amn, B = bkc | bmn. */
const char* lbwn_gemm_last_form(void);
int64_t lbwn_gemm_mbits_words_abi(int M, int N);
int lbwn_colpart_parts_abi(int M);
/* The launcher's own predicates for a product of this shape (1 / 0; -1 for another `which`):
 * which 0: it runs "x3q<8>" (mbits / mbits_out allowed); 1: it runs "x3q<8>" or "x3q<10>"
 * (row_live allowed); 2: k_live is allowed (both operands mn-contiguous assumed; only M, N, K are
 * read). */
int lbwn_gemm_form_query(int which, int M, int N, int K, int a_kcontig, int presplit, int row_exact, int colpart);

/* ---- the conditioning kernels on their own inputs (parity tests; added after ABI 5 was declared,
 * same ABI: symbols added, none altered) ----
 * LC upsample (tmodel.py:68-83): nup stages of conv1d_transpose with kernel = stride = strides[i],
 * stage i maps rows [R_i][I_i] to [R_i·s_i][Lo] (R_0 = 1 per mel frame, I_0 = Li, later I_i = Lo):
 * out[s·t + j][o] = Σ_c in[t][c]·F_i[j][o][c], F_i fp32 [s_i][Lo][I_i].  The fused kernels run one
 * block per mel frame inside an envelope: 1..4 stages of stride 1..8, Li <= Lo, both multiples of 4,
 * hop = Π s_i <= 256, and both kernels' LDS layouts within 40448 floats.
 * lbwn_lc_upsample_fused_ok: 1 inside the envelope, else 0 (no device work).
 * lbwn_lc_upsample_part_floats: floats of the backward's scratch dpart, frames·Σ_i s_i·Lo·I_i.
 * lbwn_lc_upsample_forward: mel [frames][Li] -> act[i] [frames·R_{i+1}][Lo], every stage's output.
 * lbwn_lc_upsample_backward: dF[i] = the filter gradients [s_i][Lo][I_i] (overwritten) given
 *   d(act[nup-1]) = the sum of dlc_parts (>= 1) partials [frames·hop][Lo], dlc_stride floats apart
 *   (a multiple of 4, >= frames·hop·Lo; unused for one part), the mel and the stage inputs
 *   act[0 .. nup-2] (act[nup-1] is not read and may be NULL).  Per-frame partials go to dpart and are
 *   summed in frame order (deterministic).
 * lbwn_lc_upsample_backward_dmel: the same, and dmel [frames][Li] (required, overwritten) = stage 0's
 *   input gradient, d(in_0)[f][c] = Σ_{j,o} d(out_0)[s_0·f + j][o]·F_0[j][o][c], each frame's row by its own
 *   block in a fixed order.  Same envelope, same refusals; dF and dpart are bitwise those of
 *   lbwn_lc_upsample_backward on the same inputs.
 * Every pointer is device memory, 16-byte aligned; F, act and dF are host arrays of nup device
 * pointers.  Outside the envelope both launches return EINVAL, naming the envelope, before any launch. */
int lbwn_lc_upsample_fused_ok(int nup, const int* strides, int Li, int Lo);
int64_t lbwn_lc_upsample_part_floats(int nup, const int* strides, int Li, int Lo, int frames);
int lbwn_lc_upsample_forward(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                             const float* const* F, float* const* act, void* stream);
int lbwn_lc_upsample_backward(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                              const float* const* F, const float* const* act, const float* dlc, int dlc_parts,
                              int64_t dlc_stride, float* dpart, float* const* dF, void* stream);
int lbwn_lc_upsample_backward_dmel(int nup, const int* strides, int Li, int Lo, int frames, const float* mel,
                                   const float* const* F, const float* const* act, const float* dlc, int dlc_parts,
                                   int64_t dlc_stride, float* dpart, float* const* dF, float* dmel, void* stream);
/* GC table and its gradients (tmodel.py:92-114, :150-154), with N = L·2·Cd and column
 * n = l·2Cd + s·Cd + o (s = 0 signal, 1 gate), emb [ncat1][Ge], wsig / wgate [L][Ge][Cd]:
 *   lbwn_gc_table: out[c][n] = Σ_e emb[c][e]·W_s[l][e][o], out [ncat1][N].
 *   lbwn_gc_grads, from gcd [ncat1][N] = d(out): dsig / dgate [L][Ge][Cd], dW_s[l][e][o] =
 *     Σ_c emb[c][e]·gcd[c][n], and demb[c][e] = Σ_n gcd[c][n]·W_s[l][e][o]; all three overwritten.
 *     part: scratch of lbwn_gc_part_floats_abi(L, Ge, Cd) floats.
 * Ge (n_gc_embed) must be in [1, 32], else EINVAL before any launch. */
int lbwn_gc_table(const float* emb, const float* wsig, const float* wgate, float* out, int L, int ncat1, int Ge,
                  int Cd, void* stream);
int lbwn_gc_grads(const float* emb, const float* wsig, const float* wgate, const float* gcd, float* part,
                  float* demb, float* dsig, float* dgate, int L, int ncat1, int Ge, int Cd, void* stream);
int64_t lbwn_gc_part_floats_abi(int L, int Ge, int Cd);

/* One residual layer forward (tmodel.py:117-184): x_in is the [B][H+T][n_res] halo
 * buffer whose rows [H-d, H) hold SAVE; writes z [M][*] (row stride ldz) and, if x_out,
 * x_out body rows (x + z·RES + b). gc_tab [n_cat+1][2·n_dil] / ids, cond [M][2·n_dil]
 * (row stride ldcond) are optional conditioning adds.  wpack_ws: 16-B aligned scratch of
 * lbwn_layer_image_floats_abi() floats for the packed weight image. */
int lbwn_layer_image_floats_abi(void);
int lbwn_layer_forward(const float* x_in, float* x_out, float* z, int64_t ldz, const float* w_sig,
                       const float* w_gate, const float* b_sig, const float* b_gate, const float* w_res,
                       const float* b_res, const float* gc_tab, const int* ids, const float* cond,
                       int64_t ldcond, int B, int T, int H, int dilation, int n_res, int n_dil, float* wpack_ws,
                       void* stream);

/* One residual layer backward: TF's autodiff of tmodel.py:117-184 for one layer (the SURVEY
 * §8b lbwn_dilconv_gate_bwd).  Inputs as lbwn_layer_forward plus dz = dL/dz from the skip path
 * ([M] rows, stride lddz) and dx_out = dL/dx_out of the layer's output x_{l+1} ([M][n_res], NULL
 * for the last layer).  Recomputes the gate from x_in.  Writes dx_in = dL/d(x_in) over the whole
 * [B][H+T][n_res] halo buffer (rows [H-d, H) are the SAVE rows' share; earlier rows 0), the
 * weight and bias gradients in the reference layouts (overwritten), dcond = dL/d(cond) ([M] rows
 * of 2·n_dil, stride lddcond) when cond is given, and adds into gc_dtab [ncat+1][2·n_dil] (per
 * voice id) when given.  ws: 16-B aligned scratch of lbwn_layer_backward_ws_floats() floats. */
int64_t lbwn_layer_backward_ws_floats(int B, int T, int n_res);
int lbwn_layer_backward(const float* x_in, const float* dz, int64_t lddz, const float* dx_out, const float* w_sig,
                        const float* w_gate, const float* b_sig, const float* b_gate, const float* w_res,
                        const float* b_res, const float* gc_tab, const int* ids, const float* cond, int64_t ldcond,
                        float* dx_in, float* dw_sig, float* dw_gate, float* db_sig, float* db_gate, float* dw_res,
                        float* db_res, float* dcond, int64_t lddcond, float* gc_dtab, int B, int T, int H, int dilation,
                        int n_res, int n_dil, float* ws, void* stream);

/* D-separation prepend/save for all layers at once (tmodel.py:122-127, :165). */
int lbwn_dsep_prepend(float* x_all, int64_t x_layer_stride, const float* save, int n_layers, int n_block_layers,
                      int B, int T, int H, int n_res, void* stream);
int lbwn_dsep_save(const float* x_all, int64_t x_layer_stride, float* save, int n_layers, int n_block_layers,
                   int B, int T, int H, int n_res, void* stream);

/* softmax_cross_entropy_with_logits_v2 on logits[:, :-1] vs one-hot(wav_q[:, 1:]) with
 * mask ids[:, 1:] != 0 (tmodel.py:228-249).  Overwrites logits with the unnormalised
 * gradient (softmax - onehot)·mask when write_grad; stats as lbwn_train_forward.
 * partial_ws: 3·2048 floats. */
int lbwn_head_xent(float* logits, const int* wav_q, const int* ids, int B, int T, int Q, int write_grad,
                   float* stats, float* partial_ws, void* stream);

/* The head of lbwn_train_forward_ex alone (its objective, stats and stats_ex; no column partials):
 * logits [B·T][Q] are overwritten with dlogits.  teacher: rows at teacher + m·ld_teacher, NULL allowed with
 * alpha = 0.  stats_ex is nullable.  partial_ws: 5·2048 floats (the 3·2048 of lbwn_head_xent, then 2·2048
 * for the plain xent and the KL).  alpha, temp and smoothing are host scalars read at the call. */
int lbwn_head_xent_ex(float* logits, const int* wav_q, const int* ids, int B, int T, int Q, const float* teacher,
                      int64_t ld_teacher, float alpha, float temp, float smoothing, float* stats, float* stats_ex,
                      float* partial_ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LBWN_H */
