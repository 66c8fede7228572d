// Cached generation, the plan (gen_common.h has its state): creation and the workspace, the sampling
// triple and lbwn_gen_run.  Two execution forms, chosen at plan creation: persistent (gen_persist.hip)
// and per step (gen_step.hip).  lbwn_gen_start, the mel, sessions and snapshots are in gen_state.hip,
// the prompt prefill and teacher-forced scoring in gen_prefill.hip.
#include "gen_common.h"

constexpr int G_LC_CHUNK = 64;         // default NC (steps per projection launch / persistent sub-run)
constexpr int G_LC_CHUNK_MAX = 4096;
constexpr int G_PF_ROWS = 32768;       // default prefill slice: B·T_s rows per layer launch (the C2 launch size)
constexpr int G_PF_SLICE_MAX = 65536;
constexpr int G_PF_LC_GROUP = 8;       // default layers per prefill projection launch

// the per-step GEMM form: large B, shapes the split GEMM takes (N % 4, K % 4, row strides)
static bool gemm_form_ok(const lbwn_gen_plan* p) {
  return !p->persist && p->B > P_MAXB && p->Cs % 4 == 0 && p->Cp % 4 == 0 && p->Q % 4 == 0 && (p->L * p->Cd) % 4 == 0;
}

// *v = the environment's `name`, an integer in 1..hi (unset: *v stays); what: the bound's name in the refusal
static int gen_env_int(const char* name, int hi, const char* what, int* v) {
  const char* s = getenv(name);
  if (!s) return 0;
  char* end = nullptr;
  const long x = strtol(s, &end, 10);
  LBWN_REQUIRE(end != s && *end == 0 && x >= 1 && x <= hi, "gen: %s must be an integer in 1..%d%s (got '%s')", name, hi,
               what, s);
  *v = (int)x;
  return 0;
}

// ring = 0: the plan of lbwn_gen_plan_create; ring = R >= 1: a ring plan, whose outputs hold R
// columns and whose "lc" holds Rlc = ceil(R/hop)·hop rows per stream, whatever max_steps says
static int gen_plan_make(const lbwn_arch* a, int B, int64_t max_steps, int64_t max_teacher, int64_t ring,
                         lbwn_gen_plan** out) {
  LBWN_REQUIRE(a && out && B >= 1 && max_steps >= 1 && max_teacher >= 0, "gen_plan_create: bad arguments");
  const long long cols = ring ? ring : max_steps;   // columns of "samples" / "wav", steps the lc rows cover
  LBWN_REQUIRE(a->n_res <= 32 && a->n_dil <= 32, "gen: n_res/n_dil must be <= 32");
  LBWN_REQUIRE(a->n_blocks * a->n_block_layers <= G_MAXL, "gen: more than %d layers (tap cache)", G_MAXL);
  LBWN_REQUIRE(a->n_quant <= 512, "gen: n_quant must be <= 512");
  // local conditioning: the training plan's limits (lbwn_plan_create)
  long long hop = 1;
  int lc_chunk = G_LC_CHUNK;
  const int n_layers = a->n_blocks * a->n_block_layers;
  int pf_group = std::min(G_PF_LC_GROUP, n_layers);
  if (a->n_lc_out > 0) {
    LBWN_REQUIRE(a->n_lc_upsample >= 1 && a->n_lc_upsample <= 8, "gen: LC needs 1..8 upsample stages");
    for (int i = 0; i < a->n_lc_upsample; ++i) {
      LBWN_REQUIRE(a->lc_upsample[i] >= 1, "gen: bad lc_upsample stride");
      hop *= a->lc_upsample[i];
      LBWN_REQUIRE(hop <= (1LL << 30), "gen: mel hop too large");
    }
    LBWN_REQUIRE(a->n_lc_in >= 4 && a->n_lc_in % 4 == 0 && a->n_lc_out % 4 == 0,
                 "gen: n_lc_in/n_lc_out must be multiples of 4");
    LBWN_REQUIRE(cols < (1LL << 31) && (cols + hop - 1) / hop * hop < (1LL << 31), "gen: %s too large for an LC plan",
                 ring ? "ring_steps" : "max_steps");
    if (int e = gen_env_int("LBWN_GEN_LC_CHUNK", G_LC_CHUNK_MAX, "", &lc_chunk)) return e;
    LBWN_REQUIRE((long long)lc_chunk * B / LCP_ROWS < 65535, "gen: LBWN_GEN_LC_CHUNK %d x batch_sz %d is too large",
                 lc_chunk, B);   // the projection's grid: one block row per LCP_ROWS (step, stream) pairs
    if (int e = gen_env_int("LBWN_GEN_PREFILL_LC_GROUP", n_layers, ", the number of layers", &pf_group)) return e;
  }
  // prefill slice length: the largest multiple of 128 with B·T_s <= G_PF_ROWS, at least 128
  int pf_slice = std::max(LBWN_LAYER_POS, G_PF_ROWS / B / LBWN_LAYER_POS * LBWN_LAYER_POS);
  if (int e = gen_env_int("LBWN_GEN_PREFILL_SLICE", G_PF_SLICE_MAX, "", &pf_slice)) return e;
  lbwn_gen_plan* p = new lbwn_gen_plan();
  p->a = *a;
  p->B = B;
  p->nbl = a->n_block_layers;
  p->L = a->n_blocks * a->n_block_layers;
  p->Cr = a->n_res; p->Cd = a->n_dil; p->Cs = a->n_skip; p->Cp = a->n_post; p->Q = a->n_quant;
  p->max_steps = ring ? INT64_MAX : max_steps;
  p->ring = ring;
  p->max_teacher = max_teacher;
  long dsum = (long)a->n_blocks * ((1L << a->n_block_layers) - 1);
  p->n_ring = dsum * B * p->Cr;
  size_t cur = 0;
  p->oRING = gcarve(cur, 4 * (size_t)p->n_ring);
  p->oZCAT = gcarve(cur, 4 * (size_t)B * p->L * p->Cd);
  // K-split GEMV partials: skip (K = L·Cd, 64-row slices), post1 and post2 (32-row slices)
  p->ksl_skip = 64;
  p->ks_skip = (p->L * p->Cd + p->ksl_skip - 1) / p->ksl_skip;
  p->ks_h = (p->Cs + 31) / 32;
  p->ks_lg = (p->Cp + 31) / 32;
  p->oSKP = gcarve(cur, 4 * (size_t)p->ks_skip * B * p->Cs);
  p->oHP = gcarve(cur, 4 * (size_t)p->ks_h * B * p->Cp);
  p->oLGP = gcarve(cur, 4 * (size_t)p->ks_lg * B * p->Q);
  p->oLOG = gcarve(cur, 4 * (size_t)B * p->Q);
  p->oSTEP = gcarve(cur, 16);   // step counter + status word
  p->oCODE = gcarve(cur, 4 * (size_t)B);
  p->oTEACH = gcarve(cur, 4 * (size_t)std::max<int64_t>(1, max_teacher));
  p->oSAMP = gcarve(cur, 4 * (size_t)B * cols);
  p->oWAV = gcarve(cur, 4 * (size_t)B * cols);
  p->oGCP = gcarve(cur, 4 * (size_t)p->L * B * 64);
  p->oBSUM = gcarve(cur, 4 * (size_t)p->Cs);
  p->oGIMG = gcarve(cur, 4 * (size_t)p->L * GIMG);
  p->oTRACE = gcarve(cur, 8 * (size_t)(2 * p->L + 8 + 128 + 2 * P_NH));
  p->trace = getenv("LBWN_GEN_TRACE") != nullptr;
  // persistent form: every block resident (one 512-thread block per CU), phase A maps
  // (16 skip columns × B streams) onto the threads, the draw's logits fit the tap table's tail
  int dev = 0, ncu = 0;
  const bool have_dev = hipGetDevice(&dev) == hipSuccess &&
                        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
  const char* pe = getenv("LBWN_GEN_PERSIST");
  // B > P_MAXB: ceil(B / P_MAXB) independent groups in the same launch while every block fits
  // (4 x (16 + 32) = 192 blocks for B = 64 on 256 CUs; beyond that the per-step GEMM form)
  p->pgroups = (B + P_MAXB - 1) / P_MAXB;
  p->pbg = (B + p->pgroups - 1) / p->pgroups;
  p->persist = (!pe || strcmp(pe, "0") != 0) && p->L <= P_MAXL && p->Q <= 256 && p->Cs <= 16 * P_NH &&
               p->Cp <= 16 * P_NH && have_dev && p->pgroups * (p->pbg + P_NH) <= ncu;
  p->ncu = have_dev ? ncu : 0;
  p->n_gran_core = (long)B * p->L * 32 + (long)B * p->Cs + (long)P_NH * B * p->Q;
  p->n_gran = p->n_gran_core + p->pgroups;   // + the groups' step counters (zeroed with the granules)
  p->oGRAN = gcarve(cur, 8 * (size_t)p->n_gran);
  if (gemm_form_ok(p)) {
    // split K until ~256 blocks of 128 x 128 tiles (M = B streams is short), >= 4 k-steps of 32 each
    const int Ns[3] = {p->Cs, p->Cp, p->Q}, Ks[3] = {p->L * p->Cd, p->Cs, p->Cp};
    long most = 0;
    for (int i = 0; i < 3; ++i) {
      const int tiles = ((B + 127) / 128) * ((Ns[i] + 127) / 128);
      p->gsplit[i] = std::max(1, std::min(256 / std::max(1, tiles), Ks[i] / 128));
      most = std::max(most, (long)p->gsplit[i] * B * Ns[i]);
    }
    p->oGSPL = gcarve(cur, 4 * (size_t)most);
  }
  if (a->n_lc_out > 0) {
    p->Li = a->n_lc_in; p->Lo = a->n_lc_out; p->nup = a->n_lc_upsample; p->hop = hop; p->NC = lc_chunk;
    for (int i = 0; i < p->nup; ++i) p->up[i] = a->lc_upsample[i];
    const long long frames = (cols + hop - 1) / hop;
    p->lc_rows = frames * hop;
    p->oLC = gcarve(cur, 4 * (size_t)B * p->lc_rows * p->Lo);
    long long r = frames;
    for (int i = 0; i + 1 < p->nup; ++i) {   // outputs of the stages before the last
      r *= p->up[i];
      p->oLCACT[i] = gcarve(cur, 4 * (size_t)B * r * p->Lo);
    }
    p->oLCACT[p->nup - 1] = p->oLC;
    p->oLCC = gcarve(cur, 4 * (size_t)p->NC * p->L * B * 64);
    p->up_fused = lbwn_lc_up_fused_ok(p->nup, p->up, p->Li, p->Lo) != 0;
  }
  {   // prefill scratch: independent of the prompt length (a plan's workspace is that of the same
      // arch without LC plus the LC tensors, "pfcond" the last of them)
    p->pfT = pf_slice;
    p->pfH = 1 << (p->nbl - 1);
    for (int i = 0; i < 2; ++i) p->oPFX[i] = gcarve(cur, 4 * (size_t)B * ((size_t)p->pfH + p->pfT) * p->Cr);
    p->oPFZ = gcarve(cur, 4 * (size_t)B * p->pfT * p->Cd);
    p->oPFIMG = gcarve(cur, 4 * (size_t)p->L * lbwn_layer_image_floats());
    if (a->n_gc_embed > 0) {
      p->oPFGC = gcarve(cur, 4 * (size_t)p->L * B * 2 * p->Cd);
      p->oPFIDS = gcarve(cur, 4 * (size_t)B * p->pfT);
    }
    if (p->Lo > 0) {
      p->pfG = pf_group;
      p->oPFCOND = gcarve(cur, 4 * (size_t)B * p->pfT * p->pfG * 2 * p->Cd);
    }
  }
  {   // "sessions": the last 32·B bytes (rounded up to 256) of the workspace.  They lie over the prefill
      // scratch, which no call reads in session mode, so a plan's workspace keeps its size; only a plan
      // whose prefill scratch is smaller than the words (a degenerate slice) grows by the difference
    const size_t sb = (32 * (size_t)B + 255) / 256 * 256;
    if (cur - p->oPFX[0] < sb) gcarve(cur, sb - (cur - p->oPFX[0]));
    p->oSESS = cur - sb;
    p->sess_begun.assign(B, 0);
    p->sess_seen.assign(B, 0);
    p->sess_rows.assign(B, 0);
  }
  p->total = cur;
  *out = p;
  return 0;
}

extern "C" int lbwn_gen_plan_create(const lbwn_arch* a, int B, int64_t max_steps, int64_t max_teacher,
                                    lbwn_gen_plan** out) {
  return gen_plan_make(a, B, max_steps, max_teacher, 0, out);
}

extern "C" int lbwn_gen_plan_create_ex(const lbwn_arch* a, const lbwn_gen_plan_args* args, lbwn_gen_plan** out) {
  LBWN_REQUIRE(a, "gen_plan_create_ex: arch is null");
  LBWN_REQUIRE(args, "gen_plan_create_ex: args is null");
  LBWN_REQUIRE(out, "gen_plan_create_ex: out is null");
  LBWN_REQUIRE(args->struct_size == sizeof(lbwn_gen_plan_args), "gen_plan_create_ex: struct_size %zu != %zu",
               args->struct_size, sizeof(lbwn_gen_plan_args));
  LBWN_REQUIRE(args->ring_steps >= 0, "gen_plan_create_ex: ring_steps = %lld must be >= 0", (long long)args->ring_steps);
  LBWN_REQUIRE(args->ring_steps < (1LL << 31), "gen_plan_create_ex: ring_steps = %lld must be < 2^31",
               (long long)args->ring_steps);
  return gen_plan_make(a, args->batch_sz, args->max_steps, args->max_teacher, args->ring_steps, out);
}

extern "C" void lbwn_gen_plan_destroy(lbwn_gen_plan* p) { delete p; }
extern "C" size_t lbwn_gen_workspace_bytes(const lbwn_gen_plan* p) { return p ? p->total : 0; }

extern "C" int lbwn_gen_tensor(const lbwn_gen_plan* p, const char* name, size_t* off, size_t* bytes) {
  LBWN_REQUIRE(p && name && off && bytes, "gen_tensor: null argument");
  const size_t B = p->B, cols = gen_out_cols(p);
  if (!strcmp(name, "samples")) { *off = p->oSAMP; *bytes = 4 * B * cols; }
  else if (!strcmp(name, "wav")) { *off = p->oWAV; *bytes = 4 * B * cols; }
  else if (!strcmp(name, "logits")) { *off = p->oLOG; *bytes = 4 * B * p->Q; }
  else if (!strcmp(name, "step")) { *off = p->oSTEP; *bytes = 8; }
  // 0, or 5: a persistent hand-off timed out, or 6: lbwn_gen_state_load refused its snapshot or map, or 7:
  // lbwn_gen_extend / lbwn_gen_collect refused their range
  else if (!strcmp(name, "status")) { *off = p->oSTEP + 8; *bytes = 4; }
  else if (!strcmp(name, "trace")) { *off = p->oTRACE; *bytes = 8 * (size_t)(2 * p->L + 8 + 128 + 2 * P_NH); }
  else if (!strcmp(name, "rings")) { *off = p->oRING; *bytes = 4 * (size_t)p->n_ring; }
  else if (!strcmp(name, "teacher")) { *off = p->oTEACH; *bytes = 4 * (size_t)std::max<long long>(1, p->n_teacher); }
  else if (p->Lo > 0 && !strcmp(name, "lc")) { *off = p->oLC; *bytes = 4 * B * (size_t)p->lc_rows * p->Lo; }
  else if (p->Lo > 0 && !strcmp(name, "lccond")) { *off = p->oLCC; *bytes = 4 * (size_t)p->NC * p->L * B * 64; }
  else if (!strcmp(name, "sessions")) { *off = p->oSESS; *bytes = 32 * B; }
  else if (p->Lo > 0 && !strcmp(name, "pfcond")) { *off = p->oPFCOND; *bytes = 4 * B * (size_t)p->pfT * p->pfG * 2 * p->Cd; }
  else LBWN_REQUIRE(false, "gen_tensor: unknown tensor '%s'", name);
  return 0;
}

extern "C" int lbwn_gen_is_persistent(const lbwn_gen_plan* p) { return p && p->persist ? 1 : 0; }

extern "C" int lbwn_gen_set_sampling(lbwn_gen_plan* p, float temperature, int top_k, float top_p) {
  LBWN_REQUIRE(p, "gen_set_sampling: plan is null");
  LBWN_REQUIRE(std::isfinite(temperature) && temperature > 0.f,
               "gen_set_sampling: temperature must be finite and > 0 (got %g)", (double)temperature);
  LBWN_REQUIRE(top_k >= 0, "gen_set_sampling: top_k must be >= 0 (got %d)", top_k);
  LBWN_REQUIRE(top_p > 0.f && top_p <= 1.f, "gen_set_sampling: top_p must be in (0, 1] (got %g)", (double)top_p);
  p->temperature = temperature;
  p->top_k = top_k >= p->Q ? 0 : top_k;   // every code kept: off
  p->top_p = top_p;
  return 0;
}

extern "C" int lbwn_gen_get_sampling(const lbwn_gen_plan* p, float* temperature, int* top_k, float* top_p) {
  LBWN_REQUIRE(p, "gen_get_sampling: plan is null");
  if (temperature) *temperature = p->temperature;
  if (top_k) *top_k = p->top_k;
  if (top_p) *top_p = p->top_p;
  return 0;
}

extern "C" int lbwn_gen_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, void* stream) {
  LBWN_REQUIRE(p && P && ws && n_steps >= 0, "gen_run: bad arguments");
  LBWN_REQUIRE(p->Lo == 0 || p->mel_loaded || p->sess_mode,
               "gen_run: LC plan without a mel (lbwn_gen_set_mel after lbwn_gen_start)");
  LBWN_REQUIRE(p->Lo == 0 || !p->sess_mode || p->n_begun == p->B,
               "gen_run: session mode, but only %d of the %d streams have begun a session (lbwn_gen_begin gives "
               "each its mel)", p->n_begun, p->B);
  hipStream_t st = (hipStream_t)stream;
  const auto run = p->persist ? lbwn_gen_persist_run : lbwn_gen_step_run;
  if (p->Lo == 0) {
    if (int e = run(p, P, ws, n_steps, st)) return e;
  } else {
    // sub-runs of <= NC steps: project their cond-ring rows (step t -> slot t mod NC), then the steps
    for (int done = 0; done < n_steps; done += p->NC) {
      const int n = std::min(p->NC, n_steps - done);
      if (int e = lbwn_gen_lc_proj_launch(p, P, ws, n, st)) return e;
      if (int e = run(p, P, ws, n, st)) return e;
    }
  }
  // the persistent form's wav: decode the call's samples [step - n_steps, step)
  if (p->persist && n_steps > 0) return lbwn_gen_decode_launch(p, ws, n_steps, st);
  return 0;
}
