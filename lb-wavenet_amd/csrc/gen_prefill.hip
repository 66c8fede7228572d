// Prompt prefill (lbwn_gen_prefill): n steps with known inputs as a sliced per-layer forward
// (layer.hip's layer_fwd_kernel) whose D-separation state is the rings.  LC plans project the slice's
// lc rows for G layers at a time on the f32 matrix cores (gen_prefill_lcproj_kernel) into the
// per-row cond term that kernel already takes.
// Teacher-forced scoring (lbwn_gen_score): the same host loop with every layer's z kept side by side
// in a caller-owned Zcat, the per-step GEMM form's head over all rows of a slice, and one wave per
// row for logp = logit[code] - logsumexp (gen_score_logp_kernel).
#include "gen_draw.h"

namespace {

// ---- parallel prompt prefill (lbwn_gen_prefill) -------------------------------
// n steps whose inputs are known are a training-style forward over n positions: per slice of T
// positions, layer by layer through layer_fwd_kernel on two ping-pong halo buffers [B][H+T][Cr].
// The generator's rings are the D-separation state between slices: layer l's halo rows [H-d, H) are
// the ring slots of steps t0s-d .. t0s-1 (slots never written since gen_reset are zero = the
// reference's zero lookback, so negative times need no case), and the slice's last min(d, T) inputs
// go back into the ring.  t0s = *step + off: the step counter is only read until the finish kernel.

// an input code as the step kernels may read it: pending -1 stays "zero vector", the rest inside PRE
LBWN_DEV int prefill_clamp(int c, int Q) { return min(max(c, 0), Q - 1); }

// layer 0's body rows of the slice: row j = PRE[in_j] (+ PRE_BIAS), in_j = the input of step
// t0 + off + j: the pending code[b] for the call's first step, else codes[b][off + j - 1];
// ids[b][j] = b (the per-stream GC table's row).  V4: one float4 per item (Cr % 4 == 0, aligned).
struct PrefillE {
  const float* pre; const float* pre_b; const int* codes; const int* code; float* x; int* ids;
  long ld_codes, off;
  int B, T, H, Cr, Q, bias;
};
template <bool V4>
__global__ void gen_prefill_embed_kernel(PrefillE a) {
  const int cw = V4 ? a.Cr >> 2 : a.Cr;
  const long total = (long)a.B * a.T * cw;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % cw);
    const long r = e / cw;
    const int j = (int)(r % a.T), b = (int)(r / a.T);
    const long g = a.off + j;
    int q = g == 0 ? a.code[b] : a.codes[(long)b * a.ld_codes + g - 1];
    if (g > 0 || q >= 0) q = prefill_clamp(q, a.Q);
    float* dst = a.x + ((long)b * (a.H + a.T) + a.H + j) * a.Cr;
    if (V4) {
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (q >= 0) v = *(const floatx4*)(a.pre + (long)q * a.Cr + 4 * c);
      if (a.bias) v += *(const floatx4*)(a.pre_b + 4 * c);
      *(floatx4*)(dst + 4 * c) = v;
    } else {
      float v = q >= 0 ? a.pre[(long)q * a.Cr + c] : 0.f;
      if (a.bias) v += a.pre_b[c];
      dst[c] = v;
    }
    if (c == 0 && a.ids) a.ids[(long)b * a.T + j] = b;
  }
}

// Two independent copies of one slice in one launch (either may be absent):
//   gen_body_to_ring  the last min(dw, T) body rows of layer l's input -> their slots of ring l
//   gen_ring_to_halo  ring l+1's slots of steps t0s-dr .. t0s-1 -> halo rows [H-dr, H) of layer l+1's input
// They touch different layers' rings and different buffers.  For ONE layer the halo copy comes a
// launch earlier in stream order than the ring write: with T < d the slots written (steps t0s ..)
// alias the oldest slots the halo copy reads (steps t0s-d ..).
struct PrefillX {
  const long long* step; long off;
  const float* src; float* ring_w; int dw;
  const float* ring_r; float* dst; int dr;
  int B, T, H, Cr;
};
template <bool V4>
__global__ void gen_prefill_xfer_kernel(PrefillX a) {
  const int cw = V4 ? a.Cr >> 2 : a.Cr;
  const long long t0s = *a.step + a.off;
  const int nw = a.ring_w ? min(a.dw, a.T) : 0, nr = a.ring_r ? a.dr : 0;
  const long tw = (long)a.B * nw * cw, total = tw + (long)a.B * nr * cw;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const float* s;
    float* d;
    if (e < tw) {   // body -> ring
      const int c = (int)(e % cw);
      const long r = e / cw;
      const int i = (int)(r % nw), b = (int)(r / nw), j = a.T - nw + i;
      const long slot = (long)((t0s + j) & (long long)(a.dw - 1));
      s = a.src + ((long)b * (a.H + a.T) + a.H + j) * a.Cr;
      d = a.ring_w + ((long)b * a.dw + slot) * a.Cr;
      if (V4) *(floatx4*)(d + 4 * c) = *(const floatx4*)(s + 4 * c);
      else d[c] = s[c];
    } else {        // ring -> halo
      const long f = e - tw;
      const int c = (int)(f % cw);
      const long r = f / cw;
      const int i = (int)(r % nr), b = (int)(r / nr);
      const long slot = (long)((t0s - a.dr + i) & (long long)(a.dr - 1));   // two's complement: also for t < 0
      s = a.ring_r + ((long)b * a.dr + slot) * a.Cr;
      d = a.dst + ((long)b * (a.H + a.T) + a.H - a.dr + i) * a.Cr;
      if (V4) *(floatx4*)(d + 4 * c) = *(const floatx4*)(s + 4 * c);
      else d[c] = s[c];
    }
  }
}

// the per-stream GC rows of the step kernels (gc_proj [L][B][sig 32 | gate 32]) as layer_fwd's table
// [L][B][sig Cd | gate Cd]: the same sums the sequential path adds
__global__ void gen_prefill_gctab_kernel(const float* gc_proj, float* out, long rows, int Cd) {
  const long total = rows * 2 * Cd;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int o = (int)(e % (2 * Cd));
    out[e] = gc_proj[(e / (2 * Cd)) * 64 + (o < Cd ? o : 32 + o - Cd)];
  }
}

// The LC term of one prefill slice for the G consecutive layers l0 .. l0+G-1:
//   out[m][g·2Cd + o] = Σ_k lc[b][r][k] · [LC_SIGNAL_l | LC_GATE_l][k][o],  l = l0 + g, o < 2Cd,
// m = b·T + j the row order layer_fwd_kernel reads (cond + m·ldcond), row stride ld, r = r(t0s + j)
// of gen_lc_proj_kernel from the same two device words.  Exact f32 on the matrix cores
// (v_mfma_f32_32x32x2_f32): the weights are the row operand (rows = out channel, as layer.hip's
// accumulators), the gathered lc rows the column operand, k ascending into ONE accumulator per
// 32 x 32 tile, so each output is the fmaf chain in k order that gen_lc_proj_kernel computes.  A
// wave owns one tile: 32 positions x the signal or the gate half; the MFMA's dependent-accumulator
// latency equals its issue interval, so the one chain keeps the pipe full, and the SIMD's second
// wave (the other half of the same positions) issues while this one waits for its LDS reads.  A
// lane ends with 4 consecutive out channels of one position per accumulator quad and stores them
// as one float4 along o.
// Block = PLC_POS = 128 rows m, 8 waves (signal | gate, 4 waves of 32 positions each).  LDS, both
// k-major so that every operand read is one conflict-free ds_read_b32 (the two lane halves read
// rows k = 2s, 2s + 1):
//   Xs [kt][PLC_POS]  the lc rows of the block's positions, staged once per block while n_lc_out <= PLC_KT
//   Ws [kt][64]       one layer's [signal 32 | gate 32] columns, zero past n_dil; the next layer's are
//                     fetched into registers while this layer's MFMAs issue
// n_lc_out > PLC_KT takes ceil(n_lc_out / PLC_KT) passes per layer into the same accumulators and
// restages Xs for each.
constexpr int PLC_POS = 128, PLC_NW = PLC_POS / 32;   // positions per block, waves per tile half (64 positions: 11 % slower)
constexpr int PLC_THREADS = 128 * PLC_NW, PLC_KW = PLC_THREADS / 64;
constexpr int PLC_KT = 80;   // Xs + Ws = 60 KB of the 64 KB of static LDS (arch5's n_lc_out: one pass)
constexpr int PLC_WR = PLC_KT * 64 / PLC_THREADS;   // weight words a thread carries between passes
static_assert(PLC_KT % 4 == 0 && PLC_WR * PLC_THREADS == PLC_KT * 64 && PLC_KT * (PLC_POS + 64) * 4 <= 65536,
              "PLC tile");

struct PrefillLC {
  const float* lc; const float* wsig; const float* wgate; float* out;
  const long long* step; const int* n_rows;
  long off, ld;
  int B, T, Lo, Cd, l0, G, v4;   // v4: n_dil % 4 == 0 and a 16-byte aligned workspace (float4 stores)
};

// thread (o = tid & 63, k = tid >> 6 + PLC_KW·i): unconditional loads at clamped indices, then selected
LBWN_DEV void plc_load_w(const PrefillLC& a, int l, int k0, int kt, int tid, float (&wr)[PLC_WR]) {
  const int o = tid & 63, oc = o & 31;
  const float* W = (o < 32 ? a.wsig : a.wgate) + ((long)l * a.Lo + k0) * a.Cd + min(oc, a.Cd - 1);
#pragma unroll
  for (int i = 0; i < PLC_WR; ++i) {
    const int k = (tid >> 6) + PLC_KW * i;
    wr[i] = W[(long)min(k, kt - 1) * a.Cd];
    if (k >= kt || oc >= a.Cd) wr[i] = 0.f;
  }
}

__global__ __launch_bounds__(PLC_THREADS) void gen_prefill_lcproj_kernel(PrefillLC a) {
  __shared__ __attribute__((aligned(16))) float sm[PLC_KT * (PLC_POS + 64)];
  float* Xs = sm;
  float* Ws = sm + PLC_KT * PLC_POS;
  const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) % PLC_NW, gate = tid / (64 * PLC_NW);
  const int pi = lane & 31, h = lane >> 5;
  const long M = (long)a.B * a.T, m0 = (long)blockIdx.x * PLC_POS;
  const long long t0s = *a.step + a.off;
  const int n_rows = max(*a.n_rows, 1);
  const int npass = (a.Lo + PLC_KT - 1) / PLC_KT, nst = a.G * npass;
  const long m = m0 + 32 * w + pi;
  const bool v4 = a.v4 != 0;
  float wr[PLC_WR];
  plc_load_w(a, a.l0, 0, min(PLC_KT, a.Lo), tid, wr);
  floatx16 acc;
  for (int p = 0; p < nst; ++p) {
    const int g = p / npass, k0 = (p % npass) * PLC_KT, kt = min(PLC_KT, a.Lo - k0);
    if (p) __syncthreads();   // the previous pass's LDS reads are done
    if (p == 0 || npass > 1) {
      // Xs[k][pos]: lanes along pos (conflict-free stores); a position's row is contiguous in "lc",
      // and consecutive positions of a stream are consecutive rows except at the two clamps
      const int kt4 = kt >> 2;   // Lo is a multiple of 4
      for (int e = tid; e < PLC_POS * kt4; e += PLC_THREADS) {
        const int pos = e & (PLC_POS - 1), k = 4 * (e / PLC_POS);
        const long mm = min(m0 + pos, M - 1);
        const long b = mm / a.T;
        const long long r = min(max(t0s + (mm - b * a.T) - 1, 0LL), (long long)n_rows - 1);
        const floatx4 x = *(const floatx4*)(a.lc + ((long)b * n_rows + r) * a.Lo + k0 + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) Xs[(k + i) * PLC_POS + pos] = x[i];
      }
    }
#pragma unroll
    for (int i = 0; i < PLC_WR; ++i) Ws[((tid >> 6) + PLC_KW * i) * 64 + (tid & 63)] = wr[i];
    __syncthreads();
    if (p + 1 < nst) {   // in flight during the MFMAs below
      const int k1 = ((p + 1) % npass) * PLC_KT;
      plc_load_w(a, a.l0 + (p + 1) / npass, k1, min(PLC_KT, a.Lo - k1), tid, wr);
    }
    if (k0 == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    const float* xk = Xs + h * PLC_POS + 32 * w + pi;
    const float* wk = Ws + h * 64 + 32 * gate + pi;
    // lane half h supplies k = s + h.  Four MFMAs per group of LDS reads: one read latency per 256
    // MFMA cycles instead of one per 64 (kt is a multiple of 4: a last group of two)
    int s = 0;
    for (; s + 8 <= kt; s += 8) {
      float x[4], wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[i] = xk[(s + 2 * i) * PLC_POS]; wv[i] = wk[(s + 2 * i) * 64]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = mfma32(wv[i], x[i], acc);
    }
    if (s < kt) {
      const float x0 = xk[s * PLC_POS], w0 = wk[s * 64], x1 = xk[(s + 2) * PLC_POS], w1 = wk[(s + 2) * 64];
      acc = mfma32(w0, x0, acc);
      acc = mfma32(w1, x1, acc);
    }
    if (k0 + kt == a.Lo && m < M) {
      float* row = a.out + m * a.ld + (long)g * 2 * a.Cd + gate * a.Cd;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 8 * q + 4 * h;   // acc_row(4q, h): this lane's 4 consecutive out channels
        if (v4) {
          if (o < a.Cd) *(floatx4*)(row + o) = floatx4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (o + i < a.Cd) row[o + i] = acc[4 * q + i];
        }
      }
    }
  }
}

// outputs of the prefilled steps: samples = the prompt, wav = its µ-law decode (the counter is only read)
__global__ void gen_prefill_out_kernel(const int* codes, long ld_codes, long n, const long long* step, int* samples,
                                       float* wav, long long max_steps, int B, int Q) {
  const long long t0 = *step;
  const long long span = min((long long)n, max(max_steps - t0, 0LL));
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)B * span;
       e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / span, j = e % span;
    const int q = prefill_clamp(codes[b * ld_codes + j], Q);
    samples[b * max_steps + t0 + j] = q;
    wav[b * max_steps + t0 + j] = mu_decode_q(q, Q);
  }
}

// last launch of a prefill, one block: the pending input, the plan's step counter and the
// persistent groups' (gstep[g-1], g = 1 .. ngroups-1)
__global__ void gen_prefill_finish_kernel(const int* codes, long ld_codes, long n, int* code, long long* step,
                                          long long* gstep, int ngroups, int B, int Q) {
  const long long t1 = *step + n;
  for (int b = threadIdx.x; b < B; b += blockDim.x) code[b] = prefill_clamp(codes[(long)b * ld_codes + n - 1], Q);
  __syncthreads();   // every thread has read *step
  for (int g = threadIdx.x; g < ngroups - 1; g += blockDim.x) gstep[g] = t1;
  if (threadIdx.x == 0) *step = t1;
}

// ---- teacher-forced scoring (lbwn_gen_score) -----------------------------------
// The head over every position of a prefill slice leaves its logits LG [B·T][Q] (row b·T + j = step
// t0 + off + j of stream b).  One wave per row: logp[b][off + j] = LG[c] - (m + log Σ exp(LG - m)) with
// c = the prompt's code at that step and m the row's max.  Each lane holds up to two float4 (Q <= 512,
// Q % 4 == 0); lanes past Q / 4 idle with -inf / 0.  last (nullable, the call's last slice): row T - 1
// of every stream is also the plan's "logits".
struct ScoreK {
  const float* lg; const int* codes; float* logp; float* last;
  long ld_codes, ld_logp, off;
  int B, T, Q;
};
constexpr int SC_ROWS = 4;   // rows (waves) per block
__global__ __launch_bounds__(64 * SC_ROWS) void gen_score_logp_kernel(ScoreK a) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * SC_ROWS + (threadIdx.x >> 6);
  if (r >= (long)a.B * a.T) return;   // whole waves leave: the DPP steps below see 64 lanes
  const int b = (int)(r / a.T), j = (int)(r % a.T);
  const float* row = a.lg + r * a.Q;
  const int nq = a.Q >> 2;
  floatx4 v[2];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (lane + 64 * i < nq) {
      v[i] = *(const floatx4*)(row + 4 * (lane + 64 * i));
      mx = fmaxf(fmaxf(mx, fmaxf(v[i][0], v[i][1])), fmaxf(v[i][2], v[i][3]));
    }
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (lane + 64 * i < nq) se += (expf(v[i][0] - mx) + expf(v[i][1] - mx)) + (expf(v[i][2] - mx) + expf(v[i][3] - mx));
  se = wave_sum(se);
  if (lane == 0) {
    const int c = prefill_clamp(a.codes[(long)b * a.ld_codes + a.off + j], a.Q);
    a.logp[(long)b * a.ld_logp + a.off + j] = row[c] - (mx + logf(se));
  }
  if (a.last && j == a.T - 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (lane + 64 * i < nq) *(floatx4*)(a.last + (long)b * a.Q + 4 * (lane + 64 * i)) = v[i];
  }
}

}  // namespace

// the refusals lbwn_gen_prefill and lbwn_gen_score share (what: the call's name in the message)
static int prefill_check(const char* what, const lbwn_gen_plan* p, const lbwn_params* P, const void* ws,
                         const int* codes, int64_t ld_codes, int64_t n) {
  LBWN_REQUIRE(p && P && ws && codes, "%s: null argument", what);
  LBWN_REQUIRE(n >= 1, "%s: n must be >= 1 (got %lld)", what, (long long)n);
  LBWN_REQUIRE(ld_codes == 0 || ld_codes >= n, "%s: ld_codes %lld must be 0 (one shared vector) or >= n = %lld", what,
               (long long)ld_codes, (long long)n);
  LBWN_REQUIRE(p->ring == 0, "%s: not supported on a ring plan (ring_steps = %lld): it is a whole-batch operation over "
               "absolute steps", what, p->ring);
  LBWN_REQUIRE(!p->sess_mode, "%s: not supported in session mode (lbwn_gen_begin since lbwn_gen_start): it is a "
               "whole-batch operation", what);
  LBWN_REQUIRE(p->Lo == 0 || p->mel_loaded,
               "%s: local conditioning is not supported before lbwn_gen_set_mel (no mel loaded)", what);
  LBWN_REQUIRE(p->Lo == 0 || (P->lc_sig && P->lc_gate), "%s: LC_SIGNAL/LC_GATE pointers are null", what);
  LBWN_REQUIRE((long long)p->B * p->pfT * p->Cr < (1LL << 31), "%s: batch_sz %d x slice %d x n_res %d >= 2^31", what,
               p->B, p->pfT, p->Cr);
  return 0;
}

// lbwn_gen_score's part of a prefill: the caller's logp and the scratch [Zcat | S | H | LG]
struct ScoreRun {
  float* logp; long ld_logp;
  float *zcat, *S, *H, *LG;
};

// sc == nullptr: the prefill, launch for launch.  Otherwise every layer's z goes to its column block of
// Zcat [B·T][L·Cd] instead of the per-layer scratch, and each slice ends with the head over its rows
// (skip as ONE GEMM with K = L·Cd, post1, post2: gen_run_gemm's three products) and gen_score_logp_kernel.
static int gen_prefill_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                           int64_t n, const ScoreRun* sc, hipStream_t st) {
  const int B = p->B, L = p->L, H = p->pfH, Cr = p->Cr, Cd = p->Cd;
  float* X[2] = {gat<float>(ws, p->oPFX[0]), gat<float>(ws, p->oPFX[1])};
  float* Z = gat<float>(ws, p->oPFZ);
  float* img = gat<float>(ws, p->oPFIMG);
  float* rings = gat<float>(ws, p->oRING);
  long long* step = gat<long long>(ws, p->oSTEP);
  int* code = gat<int>(ws, p->oCODE);
  const bool gc = p->a.n_gc_embed > 0;
  float* gtab = gc ? gat<float>(ws, p->oPFGC) : nullptr;
  int* ids = gc ? gat<int>(ws, p->oPFIDS) : nullptr;
  const bool bias = p->pre_bias && P->pre_b;
  float* pfcond = p->Lo > 0 ? gat<float>(ws, p->oPFCOND) : nullptr;
  const long ldcond = (long)p->pfG * 2 * Cd;
  // float4 rows: the buffers and rings are 256-B carved and every ring offset is a multiple of Cr
  const bool xv4 = Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  const bool ev4 = xv4 && (((uintptr_t)P->pre) & 15) == 0 && (!bias || (((uintptr_t)P->pre_b) & 15) == 0);
  auto grid = [](long items) { return (int)std::max(1L, std::min(2048L, (items + 255) / 256)); };
  if (int e = lbwn_pack_layers_launch(P->sig, P->gate, P->sig_b, P->gate_b, P->res, P->res_b, img, L, Cr, Cd, st))
    return e;
  if (gc) {
    gen_prefill_gctab_kernel<<<grid((long)L * B * 2 * Cd), 256, 0, st>>>(gat<float>(ws, p->oGCP), gtab, (long)L * B, Cd);
    LBWN_CHECK_LAUNCH();
  }
  const int WI = lbwn_layer_image_floats();
  for (int64_t off = 0; off < n; off += p->pfT) {
    const int T = (int)std::min<int64_t>(p->pfT, n - off);
    PrefillE e;
    e.pre = P->pre; e.pre_b = P->pre_b; e.codes = codes; e.code = code; e.x = X[0]; e.ids = ids;
    e.ld_codes = (long)ld_codes; e.off = (long)off;
    e.B = B; e.T = T; e.H = H; e.Cr = Cr; e.Q = p->Q; e.bias = bias ? 1 : 0;
    if (ev4) gen_prefill_embed_kernel<true><<<grid((long)B * T * (Cr / 4)), 256, 0, st>>>(e);
    else gen_prefill_embed_kernel<false><<<grid((long)B * T * Cr), 256, 0, st>>>(e);
    LBWN_CHECK_LAUNCH();
    long roff = 0;   // ring offset of layer l
    for (int l = -1; l < L; ++l) {
      // launch l: the ring write of layer l and the halo of layer l + 1 (whose buffer layer l - 1 has read)
      PrefillX x;
      memset(&x, 0, sizeof(x));
      x.step = step; x.off = (long)off; x.B = B; x.T = T; x.H = H; x.Cr = Cr;
      long items = 0;
      if (l >= 0) {
        x.dw = 1 << (l % p->nbl);
        x.src = X[l & 1]; x.ring_w = rings + roff;
        items += (long)B * std::min(x.dw, T);
        roff += (long)x.dw * B * Cr;
      }
      if (l + 1 < L) {
        x.dr = 1 << ((l + 1) % p->nbl);
        x.ring_r = rings + roff; x.dst = X[(l + 1) & 1];
        items += (long)B * x.dr;
      }
      if (xv4) gen_prefill_xfer_kernel<true><<<grid(items * (Cr / 4)), 256, 0, st>>>(x);
      else gen_prefill_xfer_kernel<false><<<grid(items * Cr), 256, 0, st>>>(x);
      LBWN_CHECK_LAUNCH();
      if (l < 0) continue;
      if (p->Lo > 0 && l % p->pfG == 0) {   // the LC terms of layers l .. l + G - 1 for this slice
        PrefillLC c;
        c.lc = gat<float>(ws, p->oLC); c.wsig = P->lc_sig; c.wgate = P->lc_gate; c.out = pfcond;
        c.step = step; c.n_rows = gat<int>(ws, p->oSTEP + 12);
        c.off = (long)off; c.ld = ldcond;
        c.B = B; c.T = T; c.Lo = p->Lo; c.Cd = Cd; c.l0 = l; c.G = std::min(p->pfG, L - l);
        c.v4 = Cd % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
        gen_prefill_lcproj_kernel<<<(unsigned)(((long)B * T + PLC_POS - 1) / PLC_POS), PLC_THREADS, 0, st>>>(c);
        LBWN_CHECK_LAUNCH();
      }
      lbwn_layer_args a;
      memset(&a, 0, sizeof(a));
      a.x_in = X[l & 1]; a.x_out = l + 1 < L ? X[(l + 1) & 1] : nullptr;   // the last layer's output is not needed
      if (sc) { a.z = sc->zcat + (long)l * Cd; a.ldz = (long)L * Cd; }
      else { a.z = Z; a.ldz = Cd; }
      a.wpack = img + (long)l * WI;
      if (gc) { a.gc_tab = gtab + (long)l * B * 2 * Cd; a.gc_ld = 2L * Cd; a.ids = ids; }
      if (p->Lo > 0) { a.cond = pfcond + (long)(l % p->pfG) * 2 * Cd; a.ldcond = ldcond; }   // GC and LC add, as in training
      a.B = B; a.T = T; a.H = H; a.d = x.dw; a.Cr = Cr; a.Cd = Cd;
      if (int e2 = lbwn_layer_fwd_launch(a, st)) return e2;
    }
    if (sc) {
      lbwn_gemm_args g[3];
      gen_head_gemms(p, P, ws, sc->zcat, B * T, sc->S, sc->H, sc->LG, g);
      for (int j = 0; j < 3; ++j)
        if (int e2 = lbwn_gemm_launch(g[j], 1, 0, 1, nullptr, st)) return e2;
      ScoreK k;
      k.lg = sc->LG; k.codes = codes; k.logp = sc->logp;
      k.last = off + T == n ? gat<float>(ws, p->oLOG) : nullptr;
      k.ld_codes = (long)ld_codes; k.ld_logp = sc->ld_logp; k.off = (long)off;
      k.B = B; k.T = T; k.Q = p->Q;
      gen_score_logp_kernel<<<(unsigned)(((long)B * T + SC_ROWS - 1) / SC_ROWS), 64 * SC_ROWS, 0, st>>>(k);
      LBWN_CHECK_LAUNCH();
    }
  }
  gen_prefill_out_kernel<<<grid((long)B * n), 256, 0, st>>>(codes, (long)ld_codes, (long)n, step, gat<int>(ws, p->oSAMP),
                                                          gat<float>(ws, p->oWAV), p->max_steps, B, p->Q);
  LBWN_CHECK_LAUNCH();
  // last: a call that failed above leaves the counters where the rings' owners expect them
  unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
  gen_prefill_finish_kernel<<<1, 256, 0, st>>>(codes, (long)ld_codes, (long)n, code, step,
                                               reinterpret_cast<long long*>(g + p->n_gran_core), p->pgroups, B, p->Q);
  LBWN_CHECK_LAUNCH();
  return 0;
}

extern "C" int lbwn_gen_prefill(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                                int64_t n, void* stream) {
  if (int e = prefill_check("prefill", p, P, ws, codes, ld_codes, n)) return e;
  return gen_prefill_run(p, P, ws, codes, ld_codes, n, nullptr, (hipStream_t)stream);
}

// the scratch of lbwn_gen_score: Zcat [R][L·Cd] | S [R][Cs] | H [R][Cp] | LG [R][Q], R = B·T_s rows, each
// part rounded up to 256 bytes
static void score_carve(const lbwn_gen_plan* p, size_t (&off)[4], size_t& total) {
  const size_t rows = (size_t)p->B * p->pfT;
  const size_t cols[4] = {(size_t)p->L * p->Cd, (size_t)p->Cs, (size_t)p->Cp, (size_t)p->Q};
  size_t cur = 0;
  for (int i = 0; i < 4; ++i) off[i] = gcarve(cur, 4 * rows * cols[i]);
  total = cur;
}

extern "C" size_t lbwn_gen_score_scratch_bytes(const lbwn_gen_plan* p) {
  if (!p) return 0;
  size_t off[4], total;
  score_carve(p, off, total);
  return total;
}

extern "C" int lbwn_gen_score(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* codes, int64_t ld_codes,
                              int64_t n, float* logp, int64_t ld_logp, void* scratch, void* stream) {
  if (int e = prefill_check("score", p, P, ws, codes, ld_codes, n)) return e;
  LBWN_REQUIRE(logp, "score: logp is null");
  LBWN_REQUIRE(scratch, "score: scratch is null");
  LBWN_REQUIRE((((uintptr_t)scratch) & 15) == 0, "score: scratch %p is not 16-byte aligned", scratch);
  LBWN_REQUIRE(ld_logp >= n, "score: ld_logp %lld must be >= n = %lld", (long long)ld_logp, (long long)n);
  // what the head GEMMs and the float4 rows of the log-softmax take
  LBWN_REQUIRE(p->Cs % 4 == 0 && p->Cp % 4 == 0 && p->Q % 4 == 0 && (p->L * p->Cd) % 4 == 0,
               "score: n_skip %d, n_post %d, n_quant %d and layers x n_dil %d must be multiples of 4", p->Cs, p->Cp,
               p->Q, p->L * p->Cd);
  const long long widest = std::max(std::max((long long)p->L * p->Cd, (long long)p->Cs),
                                    std::max((long long)p->Cp, (long long)p->Q));
  LBWN_REQUIRE((long long)p->B * p->pfT * widest < (1LL << 31), "score: batch_sz %d x slice %d x %lld columns >= 2^31",
               p->B, p->pfT, widest);
  LBWN_REQUIRE(P->skip && P->post1 && P->post2, "score: SKIP/POST1/POST2 pointers are null");
  LBWN_REQUIRE(((((uintptr_t)P->skip) | ((uintptr_t)P->post1) | ((uintptr_t)P->post2) | ((uintptr_t)ws)) & 15) == 0,
               "score: SKIP/POST1/POST2 and the workspace must be 16-byte aligned");
  size_t off[4], total;
  score_carve(p, off, total);
  ScoreRun sc;
  sc.logp = logp; sc.ld_logp = (long)ld_logp;
  sc.zcat = gat<float>(scratch, off[0]); sc.S = gat<float>(scratch, off[1]);
  sc.H = gat<float>(scratch, off[2]); sc.LG = gat<float>(scratch, off[3]);
  return gen_prefill_run(p, P, ws, codes, ld_codes, n, &sc, (hipStream_t)stream);
}
