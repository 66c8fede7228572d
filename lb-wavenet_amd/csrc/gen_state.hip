// The generator's state between two launches and what rewrites it; the step kernels know none of it.
// Local conditioning (no counterpart in imodel.py; tmodel.py:155-160): lbwn_gen_set_mel upsamples
// the mel once, gen_lc_proj_kernel projects it for the next <= NC steps into a cond ring, and the
// step kernels' loaders DMA that step's row into the fourth bias row of each layer's LDS slot.
// Sessions (lbwn_gen_begin): single streams restarted between two runs -- gen_begin_kernel zeroes their
// rings, rewrites their GC rows and writes their words {base, key, rows}; the draw and the LC projection
// read the words when the plan hands them the table.
// State snapshots (lbwn_gen_state_save / _load): one transposing copy kernel between the layer-major
// rings and stream-major records.
#include <type_traits>

#include "gen_common.h"

namespace {

// gc_proj[l][b][o] = GC_EMBED[gc_id[b]] · [GC_SIGNAL_l | GC_GATE_l]  (imodel.py:53-56, :113-118)
// one element (the sum in k order; gen_begin_kernel forms a restarted stream's row with the same code)
LBWN_DEV float gc_proj_elem(const float* emb, const float* gsig, const float* ggate, int id, int l, int o, int Ge,
                            int Cd) {
  const int oc = o & 31;
  float s = 0.f;
  if (oc < Cd) {
    const float* G = (o < 32 ? gsig : ggate) + (long)l * Ge * Cd;
    const float* em = emb + (long)id * Ge;
    for (int k = 0; k < Ge; ++k) s += em[k] * G[k * Cd + oc];
  }
  return s;
}
__global__ void gen_gc_proj_kernel(const float* emb, const float* gsig, const float* ggate, const int* ids,
                                   float* out, int B, int Ge, int Cd) {
  const int l = blockIdx.x;
  for (int e = threadIdx.x; e < B * 64; e += blockDim.x) {
    const int b = e / 64, o = e % 64;
    out[((long)l * B + b) * 64 + o] = gc_proj_elem(emb, gsig, ggate, ids[b], l, o, Ge, Cd);
  }
}

// ---- local conditioning: the cond ring ----------------------------------------------------
// lccond[t mod NC][l][b][o] = lc[b][r(t)] · [LC_SIGNAL_l | LC_GATE_l][:, o]  (tmodel.py:155-160) for
// the next n <= NC steps t = *step + j, r(t) = min(max(t-1, 0), n_rows-1): generation step t is
// training position t-1, step 0 and steps past the mel take the nearest row.  Hoisted out of the
// step kernels: inside the chain the n_lc_out x 64 product per layer would sit on the serial
// path (arch5: 80 x 64 beside the conv's 64 x 64); here it is one launch per NC steps.
// Block = (layer l, LCP_ROWS rows m = j·B + b); thread (o = tid & 63, row group tid >> 6): 16 rows x
// one output column, plain f32 FMAs in k order (the lc rows staged in LDS and read as broadcasts,
// the weight column coalesced over o and read once per 64 rows).  t and n_rows come from device words, so the launch is
// capturable and a replayed graph follows a mel loaded later.
// SESS (lbwn_gen_begin): every stream has its own region of "lc" (lc_stride rows apart) and its own
// step origin and row count in the session words: r = min(max(t - base_b - 1, 0), rows_b - 1).  On a ring
// plan the region holds Rlc rows and local row r lies at r mod Rlc (lbwn_gen_extend keeps rows_b ahead of r).
constexpr int LCP_KT = 128;             // k tile staged per pass
constexpr int LCP_RPT = LCP_ROWS / 4;   // rows per thread

struct LcProjK {
  const float* lc; const float* wsig; const float* wgate; float* out;
  const long long* step; const int* n_rows;
  int B, L, Lo, Cd, NC, n;
  const long long* sess; long lc_stride;   // SESS only
  unsigned lc_ring;                        // SESS on a ring plan: Rlc, local row r lies at row r mod Rlc (0: at r)
};

template <bool SESS>
__global__ __launch_bounds__(256) void gen_lc_proj_kernel(LcProjK a) {
  __shared__ __attribute__((aligned(16))) float xs[LCP_ROWS][LCP_KT];
  const int tid = threadIdx.x, l = blockIdx.x, m0 = blockIdx.y * LCP_ROWS, M = a.n * a.B;
  const long long t0 = *a.step;
  const int n_rows = SESS ? 1 : max(*a.n_rows, 1);
  const int o = tid & 63, oc = o & 31, rq = tid >> 6;
  const bool ocv = oc < a.Cd;
  const float* W = (o < 32 ? a.wsig : a.wgate) + (long)l * a.Lo * a.Cd + min(oc, a.Cd - 1);
  float acc[LCP_RPT];
#pragma unroll
  for (int r = 0; r < LCP_RPT; ++r) acc[r] = 0.f;
  // SESS: each block row's lc row index once, through LDS (the words are two dependent loads ahead of
  // the row's address otherwise, for every float4 of the row)
  __shared__ long srow[SESS ? LCP_ROWS : 1];
  if (SESS) {
    if (tid < LCP_ROWS) {
      const int m = min(m0 + tid, M - 1), b = m % a.B;
      const long long rows = max(a.sess[4 * b + 2], 1LL);
      const long long r = min(max(t0 + m / a.B - a.sess[4 * b] - 1, 0LL), rows - 1);
      srow[tid] = (long)b * a.lc_stride + (a.lc_ring ? (long)ring_col(r, a.lc_ring) : (long)r);
    }
    __syncthreads();
  }
  for (int k0 = 0; k0 < a.Lo; k0 += LCP_KT) {
    const int kt = min(LCP_KT, a.Lo - k0), kt4 = kt >> 2;   // Lo is a multiple of 4
    if (k0) __syncthreads();
    for (int e = tid; e < LCP_ROWS * kt4; e += 256) {
      const int j = e / kt4, k = 4 * (e % kt4), m = min(m0 + j, M - 1);
      const int b = m % a.B;
      const long long t = t0 + m / a.B;
      if (SESS) {
        *(floatx4*)&xs[j][k] = *(const floatx4*)(a.lc + srow[j] * a.Lo + k0 + k);
      } else {
        const long long r = min(max(t - 1, 0LL), (long long)n_rows - 1);
        *(floatx4*)&xs[j][k] = *(const floatx4*)(a.lc + ((long)b * n_rows + r) * a.Lo + k0 + k);
      }
    }
    __syncthreads();
    for (int k = 0; k < kt; k += 4) {
      float w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = W[(long)(k0 + k + i) * a.Cd];
#pragma unroll
      for (int r = 0; r < LCP_RPT; ++r) {
        const floatx4 x = *(const floatx4*)&xs[LCP_RPT * rq + r][k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r] = fmaf(x[i], w[i], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LCP_RPT; ++r) {
    const int m = m0 + LCP_RPT * rq + r;
    if (m >= M) break;
    const int b = m % a.B, slot = (int)((t0 + m / a.B) % a.NC);
    a.out[(((long)slot * a.L + l) * a.B + b) * 64 + o] = ocv ? acc[r] : 0.f;
  }
}

// per-layer weight image in the compute waves' lane order (reference layouts in, GIMG floats
// per layer out): SIGNAL/GATE [l][tap][Cr][Cd] (tap 0 = x[t-d]), RESIDUAL [l][Cd][Cr]
__global__ void gen_pack_kernel(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                                const float* res, const float* res_b, float* img, int Cr, int Cd) {
  const int l = blockIdx.x;
  float* out = img + (long)l * GIMG;
  for (int e = threadIdx.x; e < GIMG; e += blockDim.x) {
    float v = 0.f;
    if (e < GI_W) {
      const int w = e / 1024, m = (e / 256) % 4, ln = (e % 256) / 4, j = e % 4;
      const int c = ln >> 3, sg = (ln >> 2) & 1, kq = ln & 3;
      const int k = (m < 2 ? 0 : 32) + 8 * kq + 4 * (m & 1) + j;
      const int tap = k >> 5, in = k & 31, oc = 8 * w + c;
      if (in < Cr && oc < Cd) v = (sg ? gate : sig)[(long)l * 2 * Cr * Cd + (tap * Cr + in) * Cd + oc];
    } else if (e < GI_WR) {
      const int f = e - GI_W, j = f & 3, oc = (f >> 2) & 31, q = (f >> 7) & 3, h = f >> 9;
      const int zc = 16 * h + 4 * q + j;
      if (zc < Cd && oc < Cr) v = res[(long)l * Cd * Cr + zc * Cr + oc];
    } else {
      const int f = e - GI_WR;
      if (f < 64) {
        const float* bb = f < 32 ? sig_b : gate_b;
        if (bb && (f & 31) < Cd) v = bb[(long)l * Cd + (f & 31)];
      } else if (f < 128) {
        if (res_b && f - 64 < Cr) v = res_b[(long)l * Cr + f - 64];
      }
    }
    out[e] = v;
  }
}

__global__ void gen_set_word_kernel(int* dst, int v) { *dst = v; }

__global__ void gen_reset_kernel(float* rings, long n_ring, unsigned long long* gran, long n_gran, int* code, int B,
                                 long long* step, int* status) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n_ring; e += (long)gridDim.x * blockDim.x)
    rings[e] = 0.f;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n_gran; e += (long)gridDim.x * blockDim.x)
    gran[e] = 0ull;   // tags restart at 1 with the step counter
  if (blockIdx.x == 0) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) code[b] = -1;
    if (threadIdx.x == 0) {
      *step = 0;
      *status = 0;
    }
  }
}

// ---- sessions (lbwn_gen_begin) --------------------------------------------------
// Restart the listed streams between two runs: block (l, i) zeroes stream slot[i]'s [d_l][Cr] block of
// ring l and forms its GC projection row of layer l (gen_gc_proj_kernel's sum); block (0, i) also writes
// the stream's session words {base = *step, key, rows, 0} and its pending code -1 (the zero vector).
// init_all (the first begin since lbwn_gen_start): block (0, 0) gives every stream the launch does not
// list the words lbwn_gen_start stands for, {0, b, 0, 0}.  The list travels in the kernel arguments
// (host memory read at the call, no copy): GB_MAX entries per launch.
constexpr int GB_MAX = 128;
struct BeginK {
  float* rings; int* code; const long long* step; long long* sess;
  const float* emb; const float* gsig; const float* ggate; float* gcp;   // emb null: no GC
  int B, L, nbl, Cr, Ge, Cd, n, init_all;
  int slot[GB_MAX], gc_id[GB_MAX], key[GB_MAX], rows[GB_MAX];
};

__global__ __launch_bounds__(256) void gen_begin_kernel(BeginK a) {
  const int l = blockIdx.x, i = blockIdx.y, b = a.slot[i];
  long roff = 0;   // ring offset of layer l
  for (int k = 0; k < l; ++k) roff += (long)(1 << (k % a.nbl)) * a.B * a.Cr;
  const int d = 1 << (l % a.nbl);
  float* ring = a.rings + roff + (long)b * d * a.Cr;
  for (int e = threadIdx.x; e < d * a.Cr; e += blockDim.x) ring[e] = 0.f;
  if (a.emb) {
    for (int o = threadIdx.x; o < 64; o += blockDim.x)
      a.gcp[((long)l * a.B + b) * 64 + o] = gc_proj_elem(a.emb, a.gsig, a.ggate, a.gc_id[i], l, o, a.Ge, a.Cd);
  }
  if (l != 0) return;
  if (i == 0 && a.init_all) {
    for (int s = threadIdx.x; s < a.B; s += blockDim.x) {
      bool listed = false;
      for (int j = 0; j < a.n; ++j) listed |= a.slot[j] == s;
      if (!listed) {
        a.sess[4 * s] = 0; a.sess[4 * s + 1] = s; a.sess[4 * s + 2] = 0; a.sess[4 * s + 3] = 0;
      }
    }
  }
  if (threadIdx.x == 0) {
    a.sess[4 * b] = *a.step; a.sess[4 * b + 1] = a.key[i]; a.sess[4 * b + 2] = a.rows[i]; a.sess[4 * b + 3] = 0;
    a.code[b] = -1;
  }
}

// ---- feeding and draining a session while it runs (lbwn_gen_extend, lbwn_gen_collect) ----
// The host cannot see a captured run's replays, so what depends on the step is checked here: plain compares
// and one word store.  A refusal leaves "status" 7 (an earlier nonzero status stays) and changes nothing else.
constexpr int GS_RANGE = 7;

// The first launch of an extend: stream slot[i] gains add[i] rows.  cap = the rows its region holds; on a ring
// plan the rows behind r, the row its current local step reads, are free again.  One block; a refusal of any
// entry (or a run that is already stopped) advances none of the launch's words.
struct ExtendK {
  long long* sess; const long long* step; int* status;
  long long cap;
  int ring, n;
  int slot[GB_MAX], add[GB_MAX];
};

__global__ __launch_bounds__(GB_MAX) void gen_extend_kernel(ExtendK a) {
  const int i = threadIdx.x;
  const int st0 = *a.status;
  bool bad = st0 != 0;
  if (i < a.n) {
    const int b = a.slot[i];
    const long long rows = a.sess[4 * b + 2], loc = *a.step - a.sess[4 * b];
    const long long r = a.ring ? min(max(loc - 1, 0LL), rows) : 0LL;   // r = rows: every row given is read
    bad |= rows + a.add[i] - r > a.cap;
  }
  if (__syncthreads_or(bad)) {
    if (i == 0 && st0 == 0) *a.status = GS_RANGE;
    return;
  }
  if (i < a.n) a.sess[4 * a.slot[i] + 2] += a.add[i];
}

// Local steps [i0, i0 + n) of stream b out of "samples" / "wav" [B][cols] into dense buffers (either may be
// null).  e = the local steps already run; on a ring plan column = local step mod R and the range must not be
// overwritten yet, else column = base + local step.  Every block decides for itself before it writes.
struct CollectK {
  const int* samples; const float* wav; const long long* step; const long long* sess; int* status;
  int* samples_out; float* wav_out;
  long long i0, n, cols;
  unsigned ring;
  int b;
};

__global__ __launch_bounds__(256) void gen_collect_kernel(CollectK a) {
  const long long base = a.sess ? a.sess[4 * a.b] : 0LL, e = *a.step - base;
  const bool ok = a.i0 + a.n <= e && (a.ring ? a.i0 >= e - (long long)a.ring : base + a.i0 + a.n <= a.cols);
  if (!ok) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *a.status == 0) *a.status = GS_RANGE;
    return;
  }
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < a.n; j += (long long)gridDim.x * blockDim.x) {
    const long c = (long)a.b * a.cols + (a.ring ? (long)ring_col(a.i0 + j, a.ring) : (long)(base + a.i0 + j));
    if (a.samples_out) a.samples_out[j] = a.samples[c];
    if (a.wav_out) a.wav_out[j] = a.wav[c];
  }
}

// ---- state snapshot (lbwn_gen_state_save / lbwn_gen_state_load) ----------------
// What a run is between two launches: the rings, the pending codes, the step counter (and the
// persistent groups' copies of it).  The snapshot is stream-major -- a 256-byte header, then per
// stream a record {code, 12 zero bytes, the stream's rings in layer order, each [d][Cr]} -- so it
// does not depend on the batch size of the plan that wrote it.  Position p (in rows of Cr floats) of
// a record, with m = 2^nbl - 1: block = p / m, r = p % m, bl = floor(log2(r + 1)), slot = r + 1 - 2^bl;
// the workspace row is (block·m + 2^bl - 1)·B + b·2^bl + slot (the layers before it, then [B][d]).
constexpr int GS_MAGIC = 0x5453424c;   // "LBST"
constexpr int GS_VERSION = 1;
constexpr int GS_HEADER = 256;         // bytes; int32 words 0..7 below, the step as int64 at byte 32
constexpr int GS_CODE = 16;            // bytes of a record before its rings
constexpr int GS_UNROLL = 4;           // independent loads per thread before the first store
constexpr int GS_STATUS = 6;           // "status" after a refused load

struct StateK {
  float* rings; int* code; long long* step; long long* gstep; int* status;
  unsigned long long* gran; long n_gran;   // the hand-off granules a load zeroes (without the groups' counters)
  char* state; const int* map;             // the snapshot; load: stream b takes record map[b] (null: b)
  long long max_steps;
  int B, nb, nbl, Cr, Q, rec_bytes, state_streams, ngroups;
};

// a load's refusals, by every block for itself before it writes anything: the header against the plan
// and the call, every map entry in range
LBWN_DEV bool state_refused(const StateK& a) {
  const int* h = reinterpret_cast<const int*>(a.state);
  const long long t = *reinterpret_cast<const long long*>(a.state + 32);
  int bad = !(h[0] == GS_MAGIC && h[1] == GS_VERSION && h[2] == a.state_streams && h[3] == a.nb && h[4] == a.nbl &&
              h[5] == a.Cr && h[6] == a.Q && h[7] == a.rec_bytes && t >= 0 && t <= a.max_steps);
  if (a.map)
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) bad |= a.map[b] < 0 || a.map[b] >= a.state_streams;
  return __syncthreads_or(bad) != 0;
}

// V4: 16 bytes per lane (Cr % 4 == 0, both sides 16-byte aligned), else 4.  LOAD: snapshot -> workspace
// (plus the granules, the codes and the counters), else workspace -> snapshot (plus the header).
template <bool V4, bool LOAD>
__global__ __launch_bounds__(256) void gen_state_copy_kernel(StateK a) {
  if (LOAD && state_refused(a)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.status = GS_STATUS;
    return;
  }
  typedef typename std::conditional<V4, floatx4, float>::type T;
  const int cw = V4 ? a.Cr >> 2 : a.Cr, m = (1 << a.nbl) - 1;
  const long per = (long)a.nb * m * cw, total = (long)a.B * per;   // items of one record, of the call
  const long stride = (long)gridDim.x * blockDim.x;
  auto ends = [&](long e, T*& w, T*& s) {   // the workspace and snapshot ends of item e
    const int b = (int)(e / per);
    const long r = e % per;
    const int c = (int)(r % cw), p = (int)(r / cw);
    const int rr = p % m, bl = 31 - __clz(rr + 1), slot = rr + 1 - (1 << bl);
    const long row = ((long)(p - rr) + (1 << bl) - 1) * a.B + ((long)b << bl) + slot;
    const long rec = LOAD && a.map ? a.map[b] : b;
    w = reinterpret_cast<T*>(a.rings + row * a.Cr) + c;
    s = reinterpret_cast<T*>(a.state + GS_HEADER + rec * a.rec_bytes + GS_CODE + 4L * p * a.Cr) + c;
  };
  for (long e0 = blockIdx.x * (long)blockDim.x + threadIdx.x; e0 < total; e0 += GS_UNROLL * stride) {
    T v[GS_UNROLL];
    T* dst[GS_UNROLL];
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) {
      const long e = e0 + u * stride;
      dst[u] = nullptr;
      if (e < total) {
        T *w, *s;
        ends(e, w, s);
        v[u] = LOAD ? *s : *w;
        dst[u] = LOAD ? w : s;
      }
    }
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u)
      if (dst[u]) *dst[u] = v[u];
  }
  if (LOAD) {   // no granule of the run that was here may carry a tag the loaded step polls for
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < a.n_gran; e += stride) a.gran[e] = 0ull;
  }
  if (blockIdx.x != 0) return;
  int* h = reinterpret_cast<int*>(a.state);
  if (LOAD) {
    const long long t = *reinterpret_cast<const long long*>(a.state + 32);
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
      const long rec = a.map ? a.map[b] : b;
      const int c = *reinterpret_cast<const int*>(a.state + GS_HEADER + rec * a.rec_bytes);
      a.code[b] = min(max(c, -1), a.Q - 1);   // what the step kernels may read: -1 or inside PRE
    }
    for (int g = threadIdx.x; g < a.ngroups - 1; g += blockDim.x) a.gstep[g] = t;
    if (threadIdx.x == 0) *a.step = t;
  } else {
    const int pad = (a.rec_bytes - GS_CODE) / 4 - a.nb * m * a.Cr;   // floats behind a record's rings (n_res % 4 != 0)
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
      int* r = reinterpret_cast<int*>(a.state + GS_HEADER + (long)b * a.rec_bytes);
      r[0] = a.code[b];
      r[1] = r[2] = r[3] = 0;
      for (int i = 0; i < pad; ++i) r[a.rec_bytes / 4 - 1 - i] = 0;
    }
    if (threadIdx.x == 0) {
      h[0] = GS_MAGIC; h[1] = GS_VERSION; h[2] = a.B; h[3] = a.nb; h[4] = a.nbl; h[5] = a.Cr; h[6] = a.Q;
      h[7] = a.rec_bytes;
      *reinterpret_cast<long long*>(a.state + 32) = *a.step;
    } else if (threadIdx.x >= 10 && threadIdx.x < GS_HEADER / 4) {
      h[threadIdx.x] = 0;
    }
  }
}

}  // namespace

extern "C" int lbwn_gen_start(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const int* gc_ids,
                              const int* teacher, int64_t n_teacher, uint64_t seed, int pre_bias, void* stream) {
  LBWN_REQUIRE(p && P && ws, "gen_start: null argument");
  LBWN_REQUIRE(p->a.n_gc_embed == 0 || gc_ids, "gen_start: GC arch needs gc_ids [B]");
  LBWN_REQUIRE(!teacher || (n_teacher >= 0 && n_teacher <= p->max_teacher),
               "gen_start: teacher length %lld exceeds plan capacity %lld", (long long)n_teacher, p->max_teacher);
  LBWN_REQUIRE(p->ring == 0 || !teacher || n_teacher == 0, "gen_start: n_teacher = %lld on a ring plan; the teacher "
               "override is keyed by the absolute step and ring plans do not take it", (long long)n_teacher);
  hipStream_t st = (hipStream_t)stream;
  p->n_teacher = teacher ? n_teacher : 0;
  std::fill(p->sess_rows.begin(), p->sess_rows.end(), 0LL);
  p->mel_loaded = false;
  p->sess_mode = false;
  p->n_begun = 0;
  std::fill(p->sess_begun.begin(), p->sess_begun.end(), 0);
  p->seed = seed;
  p->pre_bias = pre_bias;
  gen_reset_kernel<<<256, 256, 0, st>>>(gat<float>(ws, p->oRING), p->n_ring, gat<unsigned long long>(ws, p->oGRAN),
                                        p->n_gran, gat<int>(ws, p->oCODE), p->B, gat<long long>(ws, p->oSTEP),
                                        gat<int>(ws, p->oSTEP + 8));
  LBWN_CHECK_LAUNCH();
  if (p->n_teacher > 0) {
    hipError_t e = hipMemcpyAsync(gat<int>(ws, p->oTEACH), teacher, 4 * (size_t)p->n_teacher, hipMemcpyDeviceToDevice,
                                  st);
    LBWN_REQUIRE(e == hipSuccess, "gen_start: teacher copy failed: %s", hipGetErrorString(e));
  }
  if (P->skip_b) {
    if (int e = lbwn_sum_bias_launch(P->skip_b, p->L, p->Cs, gat<float>(ws, p->oBSUM), st)) return e;
  }
  gen_pack_kernel<<<p->L, 256, 0, st>>>(P->sig, P->gate, P->sig_b, P->gate_b, P->res, P->res_b, gat<float>(ws, p->oGIMG),
                                        p->Cr, p->Cd);
  LBWN_CHECK_LAUNCH();
  if (p->a.n_gc_embed > 0) {
    gen_gc_proj_kernel<<<p->L, 256, 0, st>>>(P->gc_embed, P->gc_sig, P->gc_gate, gc_ids, gat<float>(ws, p->oGCP),
                                             p->B, p->a.n_gc_embed, p->Cd);
    LBWN_CHECK_LAUNCH();
  }
  return 0;
}

// the plan's upsample stack over `frames` mel frames [frames][Li] into act[i] (stage i's output; the last
// is the lc rows): the fused launcher inside its envelope, else one GEMM per stage
static int gen_upsample(const lbwn_gen_plan* p, const lbwn_params* P, const float* mel, long long frames,
                        float* const* act, hipStream_t st) {
  if (p->up_fused) return lbwn_lc_up_fwd_launch(p->nup, p->up, p->Li, p->Lo, (int)frames, mel, P->lc_up, act, st);
  // per-stage GEMMs against the [s][O][I] filters read as k-contiguous (engine.cpp cond_forward)
  const float* in = mel;
  long long rows = frames;
  int I = p->Li;
  for (int i = 0; i < p->nup; ++i) {
    const int s = p->up[i];
    lbwn_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = in; g.lda = I; g.B = P->lc_up[i]; g.ldb = I; g.C = act[i]; g.ldc = (long)s * p->Lo;
    g.M = (int)rows; g.N = s * p->Lo; g.K = I;
    if (int e = lbwn_gemm_launch(g, 1, 1, 1, nullptr, st)) return e;
    in = act[i];
    rows *= s;
    I = p->Lo;
  }
  return 0;
}

extern "C" int lbwn_gen_set_mel(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const float* mel, int64_t n_frames,
                                void* stream) {
  LBWN_REQUIRE(p && P && ws, "gen_set_mel: null argument");
  LBWN_REQUIRE(p->Lo > 0, "gen_set_mel: the arch has no local conditioning");
  LBWN_REQUIRE(mel, "gen_set_mel: mel is null");
  LBWN_REQUIRE(n_frames >= 1, "gen_set_mel: n_frames must be >= 1");
  LBWN_REQUIRE(n_frames <= p->lc_rows / p->hop, "gen_set_mel: %lld frames x hop %lld exceed the plan's %lld rows",
               (long long)n_frames, p->hop, p->lc_rows);
  LBWN_REQUIRE(P->lc_sig && P->lc_gate, "gen_set_mel: LC_SIGNAL/LC_GATE pointers are null");
  for (int i = 0; i < p->nup; ++i) LBWN_REQUIRE(P->lc_up[i], "gen_set_mel: LC_UPSAMPLE_%d pointer is null", i);
  LBWN_REQUIRE(!p->sess_mode, "gen_set_mel: the run is in session mode (lbwn_gen_begin since lbwn_gen_start); the "
               "mels come with the sessions");
  hipStream_t st = (hipStream_t)stream;
  const long long frames = (long long)p->B * n_frames;
  LBWN_REQUIRE(frames * p->hop < (1LL << 31), "gen_set_mel: too many rows");
  float* act[8];
  for (int i = 0; i < p->nup; ++i) act[i] = gat<float>(ws, p->oLCACT[i]);
  if (int e = gen_upsample(p, P, mel, frames, act, st)) return e;
  gen_set_word_kernel<<<1, 1, 0, st>>>(gat<int>(ws, p->oSTEP + 12), (int)(n_frames * p->hop));
  LBWN_CHECK_LAUNCH();
  p->mel_loaded = true;
  return 0;
}

// the cond-ring rows of the next n <= NC steps (step t -> slot t mod NC)
int lbwn_gen_lc_proj_launch(const lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n, hipStream_t st) {
  LcProjK k;
  k.lc = gat<float>(ws, p->oLC); k.wsig = P->lc_sig; k.wgate = P->lc_gate; k.out = gat<float>(ws, p->oLCC);
  k.step = gat<long long>(ws, p->oSTEP); k.n_rows = gat<int>(ws, p->oSTEP + 12);
  k.B = p->B; k.L = p->L; k.Lo = p->Lo; k.Cd = p->Cd; k.NC = p->NC; k.n = n;
  k.sess = p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr; k.lc_stride = (long)p->lc_rows;
  k.lc_ring = p->ring ? (unsigned)p->lc_rows : 0u;
  const dim3 grid(p->L, (n * p->B + LCP_ROWS - 1) / LCP_ROWS);
  (p->sess_mode ? gen_lc_proj_kernel<true> : gen_lc_proj_kernel<false>)<<<grid, 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

extern "C" int lbwn_gen_begin(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const lbwn_gen_session* s, int n,
                              size_t struct_size, void* stream) {
  LBWN_REQUIRE(p, "gen_begin: plan is null");
  LBWN_REQUIRE(P, "gen_begin: params is null");
  LBWN_REQUIRE(ws, "gen_begin: workspace is null");
  LBWN_REQUIRE(s, "gen_begin: s (the session array) is null");
  LBWN_REQUIRE(struct_size == sizeof(lbwn_gen_session), "gen_begin: struct_size %zu != %zu", struct_size,
               sizeof(lbwn_gen_session));
  LBWN_REQUIRE(n >= 1 && n <= p->B, "gen_begin: n = %d sessions must be in 1..batch_sz = %d", n, p->B);
  LBWN_REQUIRE(p->n_teacher == 0, "gen_begin: lbwn_gen_start loaded a teacher of n_teacher = %lld codes; the teacher "
               "override is keyed by the absolute step and sessions do not take it", p->n_teacher);
  LBWN_REQUIRE(!(p->mel_loaded && !p->sess_mode), "gen_begin: lbwn_gen_set_mel loaded a dense mel since "
               "lbwn_gen_start; the two modes are exclusive");
  const bool gc = p->a.n_gc_embed > 0, lc = p->Lo > 0;
  if (lc) {
    LBWN_REQUIRE(P->lc_sig && P->lc_gate, "gen_begin: LC_SIGNAL/LC_GATE pointers are null");
    for (int i = 0; i < p->nup; ++i) LBWN_REQUIRE(P->lc_up[i], "gen_begin: LC_UPSAMPLE_%d pointer is null", i);
  }
  if (gc) LBWN_REQUIRE(P->gc_embed && P->gc_sig && P->gc_gate, "gen_begin: GC_EMBED/GC_SIGNAL/GC_GATE pointers are null");
  const long long max_frames = lc ? p->lc_rows / p->hop : 0;
  std::vector<unsigned char>& seen = p->sess_seen;   // sized at plan creation: no allocation here
  std::fill(seen.begin(), seen.end(), 0);
  for (int i = 0; i < n; ++i) {
    LBWN_REQUIRE(s[i].slot >= 0 && s[i].slot < p->B, "gen_begin: s[%d].slot = %d is outside [0, batch_sz = %d)", i,
                 s[i].slot, p->B);
    LBWN_REQUIRE(!seen[s[i].slot], "gen_begin: s[%d].slot = %d is listed twice", i, s[i].slot);
    seen[s[i].slot] = 1;
    LBWN_REQUIRE(s[i].key >= 0 && s[i].key < (1LL << 31), "gen_begin: s[%d].key = %lld is outside [0, 2^31)", i,
                 (long long)s[i].key);
    LBWN_REQUIRE(!gc || (s[i].gc_id >= 0 && s[i].gc_id <= p->a.n_gc_category),
                 "gen_begin: s[%d].gc_id = %d is outside [0, n_gc_category = %d]", i, s[i].gc_id, p->a.n_gc_category);
    if (lc) {
      LBWN_REQUIRE(s[i].mel, "gen_begin: s[%d].mel is null on an LC arch", i);
      LBWN_REQUIRE((((uintptr_t)s[i].mel) & 15) == 0, "gen_begin: s[%d].mel %p is not 16-byte aligned", i,
                   (const void*)s[i].mel);
      LBWN_REQUIRE(s[i].n_frames >= 1 && s[i].n_frames <= max_frames,
                   "gen_begin: s[%d].n_frames = %lld must be in 1..%lld (x hop %lld within the plan's %lld rows)", i,
                   (long long)s[i].n_frames, max_frames, p->hop, p->lc_rows);
    } else {
      LBWN_REQUIRE(!s[i].mel, "gen_begin: s[%d].mel is given, but the arch has no local conditioning", i);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += GB_MAX) {
    BeginK k;
    memset(&k, 0, sizeof(k));
    k.rings = gat<float>(ws, p->oRING); k.code = gat<int>(ws, p->oCODE); k.step = gat<long long>(ws, p->oSTEP);
    k.sess = gat<long long>(ws, p->oSESS);
    if (gc) { k.emb = P->gc_embed; k.gsig = P->gc_sig; k.ggate = P->gc_gate; k.gcp = gat<float>(ws, p->oGCP); }
    k.B = p->B; k.L = p->L; k.nbl = p->nbl; k.Cr = p->Cr; k.Ge = p->a.n_gc_embed; k.Cd = p->Cd;
    k.n = std::min(GB_MAX, n - i0);
    k.init_all = !p->sess_mode && i0 == 0;
    for (int i = 0; i < k.n; ++i) {
      const lbwn_gen_session& e = s[i0 + i];
      k.slot[i] = e.slot; k.gc_id[i] = gc ? e.gc_id : 0; k.key[i] = (int)e.key;
      k.rows[i] = lc ? (int)(e.n_frames * p->hop) : 0;
    }
    gen_begin_kernel<<<dim3(p->L, k.n), 256, 0, st>>>(k);
    LBWN_CHECK_LAUNCH();
  }
  p->sess_mode = true;
  for (int i = 0; i < n; ++i) {
    if (!p->sess_begun[s[i].slot]) { p->sess_begun[s[i].slot] = 1; ++p->n_begun; }
    p->sess_rows[s[i].slot] = lc ? s[i].n_frames * p->hop : 0;
  }
  if (lc) {
    for (int i = 0; i < n; ++i) {   // the stream's own region of "lc" and of the stages' scratch
      float* act[8];
      long long r = max_frames;
      for (int j = 0; j + 1 < p->nup; ++j) {
        r *= p->up[j];
        act[j] = gat<float>(ws, p->oLCACT[j]) + (size_t)s[i].slot * r * p->Lo;
      }
      act[p->nup - 1] = gat<float>(ws, p->oLC) + (size_t)s[i].slot * p->lc_rows * p->Lo;
      if (int e = gen_upsample(p, P, s[i].mel, s[i].n_frames, act, st)) return e;
    }
  }
  return 0;
}

extern "C" int lbwn_gen_extend(lbwn_gen_plan* p, const lbwn_params* P, void* ws, const lbwn_gen_extend_entry* e, int n,
                               size_t struct_size, void* stream) {
  LBWN_REQUIRE(p, "gen_extend: plan is null");
  LBWN_REQUIRE(P, "gen_extend: params is null");
  LBWN_REQUIRE(ws, "gen_extend: workspace is null");
  LBWN_REQUIRE(e, "gen_extend: e (the entry array) is null");
  LBWN_REQUIRE(struct_size == sizeof(lbwn_gen_extend_entry), "gen_extend: struct_size %zu != %zu", struct_size,
               sizeof(lbwn_gen_extend_entry));
  LBWN_REQUIRE(n >= 1 && n <= p->B, "gen_extend: n = %d entries must be in 1..batch_sz = %d", n, p->B);
  LBWN_REQUIRE(p->Lo > 0, "gen_extend: the arch has no local conditioning (no mel to extend)");
  LBWN_REQUIRE(P->lc_sig && P->lc_gate, "gen_extend: LC_SIGNAL/LC_GATE pointers are null");
  for (int i = 0; i < p->nup; ++i) LBWN_REQUIRE(P->lc_up[i], "gen_extend: LC_UPSAMPLE_%d pointer is null", i);
  const long long max_frames = p->lc_rows / p->hop;
  std::vector<unsigned char>& seen = p->sess_seen;
  std::fill(seen.begin(), seen.end(), 0);
  for (int i = 0; i < n; ++i) {
    LBWN_REQUIRE(e[i].slot >= 0 && e[i].slot < p->B, "gen_extend: e[%d].slot = %d is outside [0, batch_sz = %d)", i,
                 e[i].slot, p->B);
    LBWN_REQUIRE(!seen[e[i].slot], "gen_extend: e[%d].slot = %d is listed twice", i, e[i].slot);
    seen[e[i].slot] = 1;
    LBWN_REQUIRE(e[i].mel, "gen_extend: e[%d].mel is null", i);
    LBWN_REQUIRE((((uintptr_t)e[i].mel) & 15) == 0, "gen_extend: e[%d].mel %p is not 16-byte aligned", i,
                 (const void*)e[i].mel);
    LBWN_REQUIRE(e[i].n_frames >= 1 && e[i].n_frames <= max_frames,
                 "gen_extend: e[%d].n_frames = %lld must be in 1..%lld (x hop %lld within the plan's %lld rows)", i,
                 (long long)e[i].n_frames, max_frames, p->hop, p->lc_rows);
  }
  for (int i = 0; i < n; ++i) {   // what depends on the run, after what the entries alone decide
    LBWN_REQUIRE(p->sess_mode && p->sess_begun[e[i].slot], "gen_extend: e[%d].slot = %d has begun no session since "
                 "lbwn_gen_start (lbwn_gen_begin first)", i, e[i].slot);
    LBWN_REQUIRE(p->ring || p->sess_rows[e[i].slot] + e[i].n_frames * p->hop <= p->lc_rows,
                 "gen_extend: e[%d].n_frames = %lld: the session's %lld rows + %lld exceed the plan's %lld reserved rows",
                 i, (long long)e[i].n_frames, p->sess_rows[e[i].slot], (long long)e[i].n_frames * p->hop, p->lc_rows);
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += GB_MAX) {
    ExtendK k;
    memset(&k, 0, sizeof(k));
    k.sess = gat<long long>(ws, p->oSESS); k.step = gat<long long>(ws, p->oSTEP); k.status = gat<int>(ws, p->oSTEP + 8);
    k.cap = p->lc_rows; k.ring = p->ring != 0; k.n = std::min(GB_MAX, n - i0);
    for (int i = 0; i < k.n; ++i) { k.slot[i] = e[i0 + i].slot; k.add[i] = (int)(e[i0 + i].n_frames * p->hop); }
    gen_extend_kernel<<<1, GB_MAX, 0, st>>>(k);
    LBWN_CHECK_LAUNCH();
    // the mirror follows the words launch by launch, whatever the upsample launches below return
    for (int i = 0; i < k.n; ++i) p->sess_rows[k.slot[i]] += k.add[i];
  }
  for (int i = 0; i < n; ++i) {
    // frames [f0, f0 + n_frames) of the stream's region, the second piece from frame 0 where the ring wraps;
    // every piece uses the head of the stream's stage scratch
    const int b = e[i].slot;
    const long long f0 = (p->sess_rows[b] / p->hop - e[i].n_frames) % max_frames;
    float* act[8];
    long long r = max_frames;
    for (int j = 0; j + 1 < p->nup; ++j) {
      r *= p->up[j];
      act[j] = gat<float>(ws, p->oLCACT[j]) + (size_t)b * r * p->Lo;
    }
    for (long long done = 0; done < e[i].n_frames;) {
      const long long f = (f0 + done) % max_frames, nf = std::min<long long>(e[i].n_frames - done, max_frames - f);
      act[p->nup - 1] = gat<float>(ws, p->oLC) + ((size_t)b * p->lc_rows + (size_t)f * p->hop) * p->Lo;
      if (int err = gen_upsample(p, P, e[i].mel + done * p->Li, nf, act, st)) return err;
      done += nf;
    }
  }
  return 0;
}

extern "C" int lbwn_gen_collect(lbwn_gen_plan* p, void* ws, int slot, int64_t i0, int64_t n, float* wav_out,
                                int* samples_out, void* stream) {
  LBWN_REQUIRE(p, "gen_collect: plan is null");
  LBWN_REQUIRE(ws, "gen_collect: workspace is null");
  LBWN_REQUIRE(slot >= 0 && slot < p->B, "gen_collect: slot = %d is outside [0, batch_sz = %d)", slot, p->B);
  LBWN_REQUIRE(i0 >= 0, "gen_collect: i0 = %lld must be >= 0", (long long)i0);
  LBWN_REQUIRE(n >= 0 && n <= INT64_MAX - i0, "gen_collect: n = %lld must be >= 0 (and i0 + n within int64)", (long long)n);
  LBWN_REQUIRE(wav_out || samples_out, "gen_collect: wav_out and samples_out are both null");
  if (n == 0) return 0;
  CollectK k;
  memset(&k, 0, sizeof(k));
  k.samples = gat<int>(ws, p->oSAMP); k.wav = gat<float>(ws, p->oWAV); k.step = gat<long long>(ws, p->oSTEP);
  k.sess = p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr; k.status = gat<int>(ws, p->oSTEP + 8);
  k.samples_out = samples_out; k.wav_out = wav_out;
  k.i0 = i0; k.n = n; k.cols = gen_out_cols(p); k.ring = (unsigned)p->ring; k.b = slot;
  const int grid = (int)std::max<long long>(1, std::min<long long>(1024, (n + 255) / 256));
  gen_collect_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

static size_t state_record_bytes(const lbwn_gen_plan* p) {
  const size_t rows = (size_t)p->a.n_blocks * (((size_t)1 << p->nbl) - 1);
  return (GS_CODE + 4 * rows * p->Cr + 15) / 16 * 16;
}

extern "C" size_t lbwn_gen_state_bytes(const lbwn_gen_plan* p, int n_streams) {
  return p && n_streams >= 1 ? GS_HEADER + (size_t)n_streams * state_record_bytes(p) : 0;
}

static StateK state_args(const lbwn_gen_plan* p, void* ws, void* state) {
  StateK k;
  memset(&k, 0, sizeof(k));
  unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
  k.rings = gat<float>(ws, p->oRING); k.code = gat<int>(ws, p->oCODE); k.step = gat<long long>(ws, p->oSTEP);
  k.gstep = reinterpret_cast<long long*>(g + p->n_gran_core); k.status = gat<int>(ws, p->oSTEP + 8);
  k.gran = g; k.n_gran = p->n_gran_core;
  k.state = static_cast<char*>(state);
  k.max_steps = p->max_steps;
  k.B = p->B; k.nb = p->a.n_blocks; k.nbl = p->nbl; k.Cr = p->Cr; k.Q = p->Q;
  k.rec_bytes = (int)state_record_bytes(p); k.state_streams = p->B; k.ngroups = p->pgroups;
  return k;
}

// a grid sized to the CUs (8 blocks of 4 waves each), or to the items when those are fewer
static int state_grid(const lbwn_gen_plan* p, bool v4) {
  const long items = p->n_ring / (v4 ? 4 : 1);
  const long want = (items + 256L * GS_UNROLL - 1) / (256L * GS_UNROLL);
  return (int)std::max(1L, std::min(want, 8L * (p->ncu > 0 ? p->ncu : 256)));
}

extern "C" int lbwn_gen_state_save(const lbwn_gen_plan* p, const void* ws, void* state, void* stream) {
  LBWN_REQUIRE(p, "gen_state_save: plan is null");
  LBWN_REQUIRE(ws, "gen_state_save: workspace is null");
  LBWN_REQUIRE(state, "gen_state_save: state is null");
  LBWN_REQUIRE((((uintptr_t)state) & 15) == 0, "gen_state_save: state %p is not 16-byte aligned", state);
  hipStream_t st = (hipStream_t)stream;
  const StateK k = state_args(p, const_cast<void*>(ws), state);
  const bool v4 = p->Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  (v4 ? gen_state_copy_kernel<true, false> : gen_state_copy_kernel<false, false>)<<<state_grid(p, v4), 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

extern "C" int lbwn_gen_state_load(lbwn_gen_plan* p, void* ws, const void* state, int state_streams,
                                   const int* src_stream, void* stream) {
  LBWN_REQUIRE(p, "gen_state_load: plan is null");
  LBWN_REQUIRE(ws, "gen_state_load: workspace is null");
  LBWN_REQUIRE(state, "gen_state_load: state is null");
  LBWN_REQUIRE(state_streams >= 1, "gen_state_load: state_streams must be >= 1 (got %d)", state_streams);
  LBWN_REQUIRE(src_stream || state_streams == p->B,
               "gen_state_load: src_stream is null (identity) but state_streams %d != batch_sz %d", state_streams, p->B);
  LBWN_REQUIRE((((uintptr_t)state) & 15) == 0, "gen_state_load: state %p is not 16-byte aligned", state);
  LBWN_REQUIRE(!(p->ring && p->sess_mode && p->Lo > 0), "gen_state_load: a ring LC plan in session mode: the rows the "
               "rewound steps read may be overwritten and the row mirror is not carried");
  hipStream_t st = (hipStream_t)stream;
  StateK k = state_args(p, ws, const_cast<void*>(state));   // LOAD only reads it
  k.state_streams = state_streams;
  k.map = src_stream;
  const bool v4 = p->Cr % 4 == 0 && (((uintptr_t)ws) & 15) == 0;
  (v4 ? gen_state_copy_kernel<true, true> : gen_state_copy_kernel<false, true>)<<<state_grid(p, v4), 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}
