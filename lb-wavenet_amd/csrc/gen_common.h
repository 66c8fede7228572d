// Cached single-step autoregressive generation (imodel.py:61-272): what two or more of gen.hip,
// gen_step.hip, gen_persist.hip, gen_prefill.hip and gen_state.hip use.
// All state stays on device, so a chunk of steps can be captured in a hipGraph and replayed:
// the step counter, the per-layer lookback rings (the generation form of the D-separation
// cache: layer l keeps its last d inputs, slot t mod d, replacing imodel's shift-by-chunk
// buffers imodel.py:88-98, :190-207), the next input code, the teacher vector and a
// counter-based RNG.  Kernels and their argument structs stay in each file's anonymous namespace.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lbwn.h"
#include "common.h"
#include "kernels.h"

struct lbwn_gen_plan {
  lbwn_arch a;
  int B, L, nbl, Cr, Cd, Cs, Cp, Q;
  long long max_steps;
  size_t oRING, oZCAT, oSKP, oHP, oLGP, oLOG, oSTEP, oCODE, oTEACH, oSAMP, oWAV, oGCP, oBSUM, oGIMG, oTRACE, total;
  size_t oGRAN;   // persistent form: granules [zg B·L·32 | sg B·Cs | lg P_NH·B·Q]
  // GEMM form (B > P_MAXB): skip / post1 / post2 as bf16-split MFMA GEMMs over the B streams
  // (split-K partial slabs in oGSPL) instead of the vector GEMVs
  size_t oGSPL = 0;
  int gsplit[3] = {1, 1, 1};
  long n_gran;
  bool trace, persist;
  int pgroups = 1, pbg = 0;   // persistent form: stream groups of pbg <= P_MAXB, each with its own P_NH heads
  long n_gran_core = 0;       // granules before the groups' step counters
  int ksl_skip, ks_skip, ks_h, ks_lg;
  long n_ring;
  long long n_teacher, max_teacher;
  unsigned long long seed;
  int pre_bias;
  // the draw's filters (lbwn_gen_set_sampling), normalised; host state like the seed, read by each
  // lbwn_gen_run at launch.  Neutral (1, 0, 1) launches the unfiltered kernels.
  float temperature = 1.f, top_p = 1.f;
  int top_k = 0;
  // local conditioning (Lo = 0: none): the upsampled mel "lc" [B][n_rows][Lo] (dense, n_rows =
  // the loaded mel's frames x hop <= lc_rows), the upsample stages' scratch, and the cond ring
  // "lccond" [NC][L][B][64]; the loaded n_rows also lives in the device word at oSTEP + 12
  int Li = 0, Lo = 0, nup = 0, up[8] = {1, 1, 1, 1, 1, 1, 1, 1}, NC = 0;
  long long hop = 1, lc_rows = 0;
  size_t oLC = 0, oLCACT[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oLCC = 0;
  bool up_fused = false, mel_loaded = false;
  // prefill (lbwn_gen_prefill): slice length, halo, and the scratch -- two halo
  // buffers [B][pfH + pfT][Cr], z [B·pfT][Cd], the L packed layer images, the per-stream GC table
  // [L][B][2·Cd] and ids [B][pfT]
  // LC plans: the projected LC terms of one slice for pfG consecutive layers, "pfcond" [B·pfT][pfG·2·Cd]
  int pfT = 0, pfH = 0, pfG = 0;
  size_t oPFX[2] = {0, 0}, oPFZ = 0, oPFIMG = 0, oPFGC = 0, oPFIDS = 0, oPFCOND = 0;
  int ncu = 0;   // the device's CUs at plan creation (0: none seen), the state copies' grid
  // sessions (lbwn_gen_begin): the words "sessions" int64 [B][4] at the very end of the workspace, over
  // the tail of the prefill scratch (prefill and score are refused in session mode, and the first begin
  // since lbwn_gen_start writes every stream's words); host-tracked like mel_loaded: a begin happened
  // since lbwn_gen_start, and which streams have begun a session
  size_t oSESS = 0;
  bool sess_mode = false;
  std::vector<unsigned char> sess_begun, sess_seen;
  int n_begun = 0;
  // ring plans (lbwn_gen_plan_create_ex): ring = R > 0 makes "samples" / "wav" [B][R], column =
  // local step mod R, and lc_rows = Rlc = ceil(R/hop)·hop a ring of local rows per stream; max_steps is then
  // unbounded.  sess_rows: the host mirror of each slot's row count (lbwn_gen_begin and lbwn_gen_extend write
  // it, lbwn_gen_start clears it): where an extend's rows go
  long long ring = 0;
  std::vector<long long> sess_rows;
};

// What lbwn_gen_run (gen.hip) starts: n_steps steps in the per-step form (gen_step.hip) or in one launch
// (gen_persist.hip), the wav of a persistent call's samples, the cond-ring rows of the next n steps (gen_state.hip)
int lbwn_gen_step_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, hipStream_t st);
int lbwn_gen_persist_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, hipStream_t st);
int lbwn_gen_decode_launch(const lbwn_gen_plan* p, void* ws, int n_steps, hipStream_t st);
int lbwn_gen_lc_proj_launch(const lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n, hipStream_t st);

// columns of "samples" / "wav": the ring's R, else max_steps
static long long gen_out_cols(const lbwn_gen_plan* p) { return p->ring ? p->ring : p->max_steps; }

static size_t gcarve(size_t& cur, size_t bytes) {
  size_t o = cur;
  cur += (bytes + 255) / 256 * 256;
  return o;
}

template <typename T>
static T* gat(void* ws, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// The head over M rows of Zcat [M][L·Cd] as three GEMMs (imodel.py:125-164): S = Zcat·SKIPcat + Σb, H = relu(
// relu(S)·POST1 + b1), LG = H·POST2 + b2; for the per-step GEMM form (M = B) and lbwn_gen_score (a slice's rows)
static void gen_head_gemms(const lbwn_gen_plan* p, const lbwn_params* P, void* ws, const float* zcat, int M, float* S,
                           float* H, float* LG, lbwn_gemm_args (&g)[3]) {
  memset(&g[0], 0, sizeof(g[0]));
  g[0].A = zcat; g[0].lda = (long)p->L * p->Cd; g[0].B = P->skip; g[0].ldb = p->Cs; g[0].C = S; g[0].ldc = p->Cs;
  g[0].M = M; g[0].N = p->Cs; g[0].K = p->L * p->Cd; g[0].bias = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
  g[1] = g[0];
  g[1].A = S; g[1].lda = p->Cs; g[1].relu_a = 1; g[1].B = P->post1; g[1].ldb = p->Cp; g[1].C = H; g[1].ldc = p->Cp;
  g[1].N = p->Cp; g[1].K = p->Cs; g[1].bias = P->post1_b; g[1].relu_out = 1;
  g[2] = g[1];
  g[2].A = H; g[2].lda = p->Cp; g[2].relu_a = 0; g[2].B = P->post2; g[2].ldb = p->Q; g[2].C = LG; g[2].ldc = p->Q;
  g[2].N = p->Q; g[2].K = p->Cp; g[2].bias = P->post2_b; g[2].relu_out = 0;
}

static bool gen_filtered(const lbwn_gen_plan* p) { return p->temperature != 1.f || p->top_k != 0 || p->top_p != 1.f; }

namespace {

constexpr int GI_W = 16 * 256;              // conv: [w 4][m 4][lane 64][4]  W[32(m>>1)+8kq+4(m&1)+j][32sg+8w+c]
constexpr int GI_R = 4 * 256;               // residual: [h 2][q 4][c 32][4] RES[16h+4q+j][c]
constexpr int GI_WR = GI_W + GI_R;          // 20 pieces of 1 KiB
constexpr int GIMG = GI_WR + 192;           // global image: + conv bias [64] + residual bias [64] + zeros [64]
constexpr int G_SLOT = GI_WR + 256;         // LDS slot: weights | bc [64] | br [64] | gc [64] | pad [64]
constexpr int G_NS = 6;                     // LDS ring depth (layers)
constexpr int G_PIECES = 5;                 // 1-KiB pieces per loader wave per layer (4 loaders)
constexpr int G_DMA = G_PIECES + 1;         // + one 256-B row
constexpr int G_MAXL = 256;                 // tap table rows
constexpr int G_LDS = G_NS * G_SLOT + (G_MAXL + 2) * 32 + 4 * 32 + 2 * 32;   // ring | taps | x[4 waves] | z[2]
static_assert(4 * G_PIECES * 256 == GI_WR, "image pieces");
static_assert(G_LDS * 4 <= 160 * 1024, "LDS");

constexpr int P_NH = 32;     // head blocks
constexpr int P_MAXB = 16;   // streams per group (phase A maps 16 columns x 16 streams onto 512 threads)
constexpr int P_MAXL = 236;  // layers (the draw's two half-sums use tap-table rows 240..255)
constexpr int LCP_ROWS = 64;   // (step, stream) rows per block of gen_lc_proj_kernel

// ring plans: i mod R for a local step or row i >= 0 and a ring of R < 2^31 -- the 32-bit division while i
// fits (the first 2^32 steps of a session, 74 hours at 16 kHz), the 64-bit one after that
LBWN_DEV unsigned ring_col(long long i, unsigned R) {
  const unsigned long long u = (unsigned long long)i;
  return (u >> 32) == 0 ? (unsigned)u % R : (unsigned)(u % R);
}

// ---- device helpers of both chains (gen_wave_kernel, persist_chain) -------------------------
// Wave-level LDS sync for single-wave workgroups: orders the wave's own LDS traffic without
// the vmcnt(0) that __syncthreads() implies (which would also wait for the next layer's
// weight prefetch, putting its L2 latency back on the chain).
LBWN_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

LBWN_DEV float dot4(const floatx4& w, const floatx4& x, float acc) {
  acc = fmaf(w[0], x[0], acc);
  acc = fmaf(w[1], x[1], acc);
  acc = fmaf(w[2], x[2], acc);
  return fmaf(w[3], x[3], acc);
}

constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141;

// workgroup barrier that retires only this wave's LDS ops: no vmcnt wait (outstanding global
// stores and LDS-DMA pieces stay in flight across it); the "memory" clobber pins LDS accesses
LBWN_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS-DMA: lane i's SIZE bytes from src land at lds_dst + i·SIZE (lds_dst wave-uniform).  The builtin, which
// the compiler counts in vmcnt; layer_common.h's dma16 is inline asm so that it does not: they stay apart.
LBWN_DEV void dma16(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
LBWN_DEV void dma4(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

}  // namespace
