// The generator's persistent form (the default while its blocks fit: groups of <= 16 streams, each
// group with its own head blocks, B <= 80 on 256 CUs): ONE launch per run, gen_persist_kernel — chain
// blocks (one per stream) and 32 head blocks hand z, the skip vector and the partial logits to each
// other as tagged granules; weights of the head stay in registers for the run.  Sessions, snapshots
// and the prefill: nothing here knows of them.
#include "gen_draw.h"

namespace {

#ifndef LBWN_GEN_SUBSTAMPS
#define LBWN_GEN_SUBSTAMPS 0
#endif
constexpr long long G_SPIN_TIMEOUT = 400000000LL;   // wall_clock64 ticks (100 MHz) = 4 s

// ---- persistent generation: one launch per run (stream groups of <= 16) ----------------
// Roles (one 512-thread workgroup per CU, all resident): streams split into groups of Bg <= 16, each
// group's Bg chain blocks and P_NH head blocks hand off among themselves only (groups x (Bg + P_NH)
// <= CUs; B = 64: four groups, 192 blocks); within a group:
//   chain block b < B   per step: draw the previous step (gather the P_NH partial-logit
//                       granules of stream b, Σ + b2, wave-level draw), PRE row, 50 layers as in
//                       gen_wave (LDS-DMA ring continuous across steps; the next step's taps are
//                       DMA'd right after the last layer), z_l published as tagged granules
//   head block m < P_NH owns skip columns [16m, 16m+16), post1 columns [16m, 16m+16) and the
//                       same post2 rows (POST1 / POST2 slices held in registers for the run):
//                       A. accumulates its skip columns layer by layer as the z granules arrive
//                          (SKIP slice streamed from L2 one layer ahead);
//                       B. publishes them, gathers the whole skip vector, relu(· + Σb);
//                       C. h = relu(skip·POST1[:, cols] + b1), partial logits h·POST2[rows, :]
//                          published as granules for the chain blocks' draw.
// Every hand-off is an 8-byte {value, tag = step + 1} granule written by one sc1 store and polled
// with relaxed agent-scope loads (no flag, no fence: MI355X_MICROARCH.md § visibility, R2);
// single-buffered, because no producer can run a step ahead of its slowest consumer (each
// stage waits on the previous one through the whole ring of roles).  Every spin is bounded
// (status 5).  Three hops per step (z tail, skip all-gather, logit partials) replace the
// per-step path's four launch boundaries and its weight re-fetches.
constexpr int P_DLROW = 240; // the draw's two half-sums: tap-table rows 240..255 (P_MAXL = 236 layers)
constexpr int P_LA = 8;      // layers per head round (phase A)

struct PersistK {
  const float* pre; const float* pre_b; const float* img; const float* gc_proj;
  float* rings; long long* step; const int* code_in;
  int B, L, nbl, Cr, Cd, pre_bias, n_steps;
  unsigned long long* zg;   // [B][L][32] z granules
  int Cs, Cp, Q;
  const float* skipw; const float* bsum; const float* post1; const float* post1_b; const float* post2;
  unsigned long long* sg;   // [B][Cs] skip granules
  unsigned long long* lg;   // [P_NH][B][Q] partial-logit granules
  DrawK draw;               // outputs; draw.bias = b2
  int* status;
  long long* trace;         // wall stamps of the run's last step (tools/gen_trace.py), or null
  int Bg;                   // streams per group: block g·(Bg + P_NH) + r is group g's chain block r < Bg
                            // (stream g·Bg + r) or head block r - Bg; groups hand off only inside
  long long* gstep;         // step counters of groups 1.. (group 0's is *step, the plan's "step")
  const float* lccond; int NC;   // LC plans: the cond ring [NC][L][B][64]; a run is <= NC steps
};

// poll granules base[off + i·stride], i < nv (N at most; the rest re-read granule nv-1), until
// every tag matches; v[i] = payload.  base is wave-uniform and the index 32-bit, so each load
// is one VGPR offset on an SGPR base.  After any timeout (status != 0) every sweep gives up at
// once, so a failed hand-off drains the launch instead of waiting out each later spin.
template <int N>
LBWN_DEV void sweep(const unsigned long long* base, unsigned off, unsigned stride, int nv, unsigned tag, float (&v)[N],
                    int* status) {
  long long ts = 0;
  const unsigned last = (unsigned)max(nv - 1, 0);
  for (unsigned spins = 1;; ++spins) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const unsigned idx = off + min((unsigned)i, last) * stride;
      const unsigned long long x = __hip_atomic_load(base + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v[i] = __uint_as_float((unsigned)x);
      ok &= (unsigned)(x >> 32) == tag;
    }
    if (ok) return;
    if ((spins & 31) == 0) {   // the clock and the status word cost a round trip each: not every retry
      if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
      const long long now = wall_clock64();
      if (ts == 0) ts = now;
      else if (now - ts > G_SPIN_TIMEOUT) {
        __hip_atomic_store(status, 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

LBWN_DEV void put_granule(unsigned long long* g, unsigned tag, float v) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// ring slot DMA with sc1 (L2-served): a tap line this CU read d steps ago may still sit in its L1
LBWN_DEV void dma4_sc1(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 16);
}

template <bool LC, bool FILT, bool RP>
LBWN_DEV void persist_chain(const PersistK& a, float* sm, int b, long long* stepc, long long* trace) {
  float* RING = sm;                  // [G_NS][G_SLOT]
  float* XP = sm + G_NS * G_SLOT;    // [L][32] dilated taps of this step
  float* DL = XP + P_DLROW * 32;     // [2][256] half-sums of the partial logits of the step being drawn
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, L = a.L, n = a.n_steps;
  const long long t0 = *stepc;
  const long GT = (long)n * L;       // layers of the run, in order: global index g = s·L + l

  if (wid >= 4) {   // ---- loader waves
    const int lw = wid - 4;
    const float* zeros = a.img + GI_WR + 128;
    auto taps = [&](long long t) {   // as gen_wave (a), for step t
      const int h = lane >> 5, c = lane & 31;
      long roff = 0;
      int bl = 0;
      for (int q = 0; 2 * q < L; ++q) {
        const int dE = 1 << bl;
        const long roffO = roff + (long)dE * a.B * a.Cr;
        const int blO = (bl + 1 == a.nbl) ? 0 : bl + 1;
        const int dO = 1 << blO;
        if ((q & 3) == lw) {
          const int d = h ? dO : dE, l = 2 * q + h;
          const float* src = (l < L && c < a.Cr)
                                 ? a.rings + (h ? roffO : roff) + ((long)b * d + (t & (d - 1))) * a.Cr + c
                                 : zeros + c;
          dma4_sc1(src, XP + 2 * q * 32);
        }
        roff = roffO + (long)dO * a.B * a.Cr;
        bl = (blO + 1 == a.nbl) ? 0 : blO + 1;
      }
    };
    // the layer and ring slot of the next issue, advanced with wrap-around: g mod L and g mod G_NS
    // of a 64-bit g were two long divisions per layer on the loaders' path to every barrier
    int iss_l = 0, iss_slot = 0;
    int iss_c = LC ? (int)(t0 % a.NC) : 0;   // cond-ring slot of the issued layer's step (t mod NC)
    auto issue = [&](long /*g: layer iss_l, slot iss_slot*/) {   // weights of global layer g into slot g mod G_NS
      const int l = iss_l;
      const float* src = a.img + (long)l * GIMG;
      float* dst = RING + iss_slot * G_SLOT;
      const int cs = iss_c;
      iss_l = (iss_l + 1 == L) ? 0 : iss_l + 1;
      if constexpr (LC) {
        if (iss_l == 0) iss_c = (iss_c + 1 == a.NC) ? 0 : iss_c + 1;
      }
      iss_slot = (iss_slot + 1 == G_NS) ? 0 : iss_slot + 1;
#pragma unroll
      for (int p = 0; p < G_PIECES; ++p) {
        const int pc = lw * G_PIECES + p;
        dma16(src + pc * 256 + lane * 4, dst + pc * 256);
      }
      const float* row = lw < 2 ? src + GI_WR + lw * 64
                       : lw == 2 ? (a.gc_proj ? a.gc_proj + ((long)l * a.B + b) * 64 : zeros)
                                 : zeros;
      if constexpr (LC) {
        if (lw == 3) row = a.lccond + (((long)cs * L + l) * a.B + b) * 64;
      }
      dma4(row + lane, dst + GI_WR + lw * 64);
    };
    taps(t0);
    long issued = 0;
    for (; issued < G_NS - 1 && issued < GT; ++issued) issue(issued);
    auto gather_half = [&](long long t) {   // partial logits of heads 16..31 for code q
      const int q = min((int)threadIdx.x - 256, a.Q - 1);
      float v[P_NH / 2], sum = 0.f;
      sweep<P_NH / 2>(a.lg, (unsigned)(((P_NH / 2) * a.B + b) * a.Q + q), (unsigned)(a.B * a.Q), P_NH / 2, (unsigned)t,
                      v, a.status);
#pragma unroll
      for (int i = 0; i < P_NH / 2; ++i) sum += v[i];
      DL[256 + q] = sum;
    };
    for (int s = 0; s < n; ++s) {
      if (s > 0) {
        gather_half(t0 + s);
        lds_barrier();   // D: the previous step's logits are in DL
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();              // -1: taps and the first slot landed, every wave's XW written
      for (int k = 0; k < L; ++k) {
        const long G = (long)s * L + k;
        // barrier G releases the residual of layer G and the conv of G+1: retire all but the
        // slots younger than G+1
        const long younger = (issued - 1) - (G + 1);
        if (younger >= G_NS - 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * (G_NS - 3)) : "memory");
        else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA * 2) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G_DMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        if (issued < GT) issue(issued++);   // into the slot of layer G-1 (dead after barrier G)
        if (k == L - 1 && s + 1 < n) taps(t0 + s + 1);   // the ring stores of step s landed (compute waves drained)
      }
    }
    gather_half(t0 + n);
    lds_barrier();   // D of the run's last draw
    return;
  }

  // ---- compute waves
  const int w = wid, Cr = a.Cr, Cd = a.Cd;
  const int c = lane >> 3, sg = (lane >> 2) & 1, kq = lane & 3, kp = lane & 7;
  const int ch = 8 * w + c, o = 32 * sg + ch;
  const bool lead = kp == 0;
  const int rc = lane & 31, rh = lane >> 5;
  float* XW = XP + (G_MAXL + 2) * 32 + 32 * w;
  float* Z = XP + (G_MAXL + 2) * 32 + 128;
  const int Q = a.Q, per = (Q + 63) >> 6, c0 = lane * per;
  long long* tr = (trace && b == 0 && threadIdx.x == 0) ? trace : nullptr;
  float bq[4];               // b2 of this lane's codes, loaded once (a global load in every draw before)
#pragma unroll
  for (int j = 0; j < 4; ++j) bq[j] = a.draw.bias ? a.draw.bias[min(c0 + j, Q - 1)] : 0.f;
  int code = a.code_in[b];   // step 0 of the run: the previous run's last draw (-1 at t = 0)
  float accd = 0.f;          // the dilated-tap partial of the next layer's conv
  auto dilated = [&](const float* Sl, int l) {
    const floatx4 w0 = *(const floatx4*)(Sl + (w * 4) * 256 + lane * 4);
    const floatx4 w1 = *(const floatx4*)(Sl + (w * 4 + 1) * 256 + lane * 4);
    const floatx4 x0 = *(const floatx4*)(XP + l * 32 + 8 * kq), x1 = *(const floatx4*)(XP + l * 32 + 8 * kq + 4);
    return dot4(w1, x1, dot4(w0, x0, 0.f));
  };
  int slot = 0;              // ring slot of global layer G = s·L + l (G mod G_NS, advanced per layer)
  for (int s = 0; s <= n; ++s) {
    const long long t = t0 + s;
    if (s > 0) {
      // draw step t-1: code q's partial logits of heads 0..15 here, 16..31 by the loader waves;
      // logit = (Σ first half + Σ second half) + b2
      const int q = min((int)threadIdx.x, Q - 1);
      float v[P_NH / 2], lsum = 0.f;
      sweep<P_NH / 2>(a.lg, (unsigned)(b * Q + q), (unsigned)(a.B * Q), P_NH / 2, (unsigned)t, v, a.status);
#pragma unroll
      for (int i = 0; i < P_NH / 2; ++i) lsum += v[i];
      DL[q] = lsum;
      if (tr && s == n) tr[5] = wall_clock64();
      lds_barrier();   // D
      if (tr && s == n) tr[7] = wall_clock64();
      float lv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = min(c0 + j, Q - 1);
        lv[j] = DL[cc] + DL[256 + cc];
        if (a.draw.bias) lv[j] += bq[j];
      }
      if constexpr (FILT) code = draw_core_filt<4, RP>(lv, a.draw, b, t - 1, w == 0, false);
      else code = draw_core<4, RP>(lv, a.draw, b, t - 1, w == 0, false);
      if (s == n) {
        if (tr) tr[6] = wall_clock64();
        break;
      }
    }
    if (tr && s == n - 1) tr[0] = wall_clock64();
    float x = 0.f;   // x[rc] of the current layer input: PRE row of the draw (+ PRE_BIAS); zero at t = 0
    if (rc < Cr) {
      if (code >= 0) x = a.pre[(long)code * Cr + rc];
      if (a.pre_bias && a.pre_b) x += a.pre_b[rc];
    }
    if (lane < 32) XW[rc] = x;
    long roff = 0;
    int bl = 0;
    lds_barrier();   // -1
    accd = dilated(RING + slot * G_SLOT, 0);   // this step's taps and layer 0's slot landed by -1
    for (int l = 0; l < L; ++l) {
      const float* S = RING + slot * G_SLOT;
      slot = (slot + 1 == G_NS) ? 0 : slot + 1;
      floatx4 wv[2], xv[2];   // the current tap's pieces; the dilated half is in accd
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        wv[mm] = *(const floatx4*)(S + (w * 4 + 2 + mm) * 256 + lane * 4);
        xv[mm] = *(const floatx4*)(XW + 8 * kq + 4 * mm);
      }
      float bco = S[GI_WR + o] + S[GI_WR + 128 + o];
      if (LC) bco += S[GI_WR + 192 + o];
      // (round 2: reading ALL of layer l+1's conv operands right after barrier l, and this layer's
      // residual weights ahead of the conv, measured 38.0 -> 38.9 us per step; what is kept is
      // the dilated half after the barrier and the residual weights just before the z write)
      // sub-layer cycle stamps (trace only): layers 16..23 of the traced step, 6 per layer
      // (compiled in only with -DLBWN_GEN_SUBSTAMPS=1: the lane-divergent stamp branches split the
      // layer into basic blocks the scheduler cannot overlap, 38.5 -> 44 us per step at B = 10)
      long long* st6 = (LBWN_GEN_SUBSTAMPS && tr && s == n - 1 && l >= 16 && l < 24 && L + 184 <= 2 * L + 136)
                           ? tr + 8 + L + 128 + 6 * (l - 16) : nullptr;
      if (st6) st6[0] = clock64();
      __builtin_amdgcn_sched_barrier(0);
      const int d = 1 << bl;
      if (rh == 0 && (rc >> 3) == w && rc < Cr) a.rings[roff + ((long)b * d + (t & (d - 1))) * Cr + rc] = x;
      roff += (long)d * a.B * Cr;
      bl = (bl + 1 == a.nbl) ? 0 : bl + 1;
      const float acc0 = dot4(wv[0], xv[0], accd), acc1 = dot4(wv[1], xv[1], 0.f);
      float v = acc0 + acc1;
      v += dpp_f<DPP_XOR1>(v);
      v += dpp_f<DPP_XOR2>(v);
      v += bco;
      if (st6) { asm volatile("" ::"v"(v)); st6[1] = clock64(); }
      const float vp = dpp_f<DPP_HALF_MIRROR>(v);
      const float z = gate_z(sg ? vp : v, sg ? v : vp);
      if (st6) { asm volatile("" ::"v"(z)); st6[2] = clock64(); }
      float* Zl = Z + (l & 1) * 32;
      // residual weights (slot resident since the last barrier) issued before the z write: the
      // barrier's lgkmcnt(0) retires them together with it, so only z is read after the barrier
      floatx4 rw[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rw[q] = *(const floatx4*)(S + GI_W + ((rh * 4 + q) * 32 + rc) * 4);
      const float bro = S[GI_WR + 64 + rc];
      if (lead) {
        Zl[ch] = z;
        if (ch < Cd) put_granule(a.zg + ((long)b * L + l) * 32 + ch, (unsigned)(t + 1), z);
      }
      // the last layer's ring stores must land before the loaders DMA the next step's taps
      if (l == L - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
      if (st6) st6[3] = clock64();
      accd = dilated(RING + slot * G_SLOT, min(l + 1, L - 1));   // layer l+1's slot landed by this barrier
      floatx4 zv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) zv[q] = *(const floatx4*)(Zl + 16 * rh + 4 * q);
      float r0 = dot4(rw[0], zv[0], 0.f), r1 = dot4(rw[1], zv[1], 0.f);
      r0 = dot4(rw[2], zv[2], r0);
      r1 = dot4(rw[3], zv[3], r1);
      const float r = r0 + r1;
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), __float_as_uint(r), false, false);
      x += (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + bro;
      if (st6) { asm volatile("" ::"v"(x)); st6[4] = clock64(); }
      if (lane < 32) XW[rc] = x;
      wave_sync();
      if (st6) st6[5] = clock64();
      if (tr && s == n - 1) tr[8 + l] = wall_clock64();
    }
    if (tr && s == n - 1) tr[1] = wall_clock64();
  }
  if (b % a.Bg == 0 && threadIdx.x == 0) *stepc = t0 + n;   // the group's blocks read it at their start
}

// the head's LDS carve (below) within the kernel's static allocation, at the largest Q (256)
static_assert(2 * P_LA * 528 + P_MAXB * 516 + 32 * 256 + 272 + 16 * 516 + 16 * 256 <= G_LDS, "head LDS");

LBWN_DEV void persist_head(const PersistK& a, int m, float* sm, int b0, int B, long long* stepc, long long* trace) {
  // B: this group's streams b0 .. b0+B-1 (granule and logit layouts are over all a.B streams)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = a.L, Cd = a.Cd, Cs = a.Cs, Cp = a.Cp, Q = a.Q, n = a.n_steps;
  const long long t0 = *stepc;
  // row paddings (33, 516, 17 floats) put the 16 stream rows a 16-lane MFMA operand read touches
  // on distinct banks (unpadded, the 32- / 512- / 16-float rows were 8- to 16-way conflicts)
  float* ZS = sm;                  // [2][P_LA layers][16 b][33] z of a round (double-buffered)
  float* RS = ZS + 2 * P_LA * 528; // [16 b][516] relu(skip + Σb), zero-padded
  float* HP = RS + P_MAXB * 516;   // [8 waves][64 lanes][4] MFMA partials (skip, then post1)
  float* HS = HP + 32 * 256;       // [16 b][17] h
  float* P1T = HS + 272;           // [16 c][516] POST1[:, 16m + c] (rows padded: conflict-free b128 reads)
  float* P2S = P1T + 16 * 516;     // [16 r][Q] POST2[16m + r, :]
  for (int e = tid; e < P_MAXB * 516; e += 512) RS[e] = 0.f;
  for (int e = tid; e < 16 * 512; e += 512) {   // the head's weight slices stay in LDS for the run
    const int cc = e >> 9, k = e & 511;
    P1T[cc * 516 + k] = (k < Cs && m * 16 + cc < Cp) ? a.post1[(long)k * Cp + m * 16 + cc] : 0.f;
  }
  for (int e = tid; e < 16 * Q; e += 512) {
    const int r = e / Q, q = e - r * Q;
    P2S[e] = (m * 16 + r < Cp) ? a.post2[(long)(m * 16 + r) * Q + q] : 0.f;
  }
  // lane roles: c = column within this block's 16, kg = tid >> 4 = 4·wave + (lane >> 4)
  const int c = tid & 15, kg = tid >> 4, kql = lane >> 4;
  const int scol = m * 16 + c, hcol = m * 16 + c, scol16 = m * 16;
  // A: wave wv takes layer l0 + wv of each round, lane quarter kql the channels 8kql..8kql+7
  const float* wsrc = a.skipw + (long)(8 * kql) * Cs + min(scol, Cs - 1);
  // C: post1 rows 16kg .. 16kg+15 of column hcol (P1T); post2 rows 16m .. 16m+15 of column tid (P2S)
  const float b1 = (hcol < Cp && a.post1_b) ? a.post1_b[hcol] : 0.f;
  // z granules polled by this thread: (stream zb0, channel zk) of every layer of a round
  const int zb0 = tid >> 5, zk = tid & 31;
  const bool zn0 = zb0 < B && zk < Cd;
  long long* tr = (trace && m == P_NH - 1 && tid == 0) ? trace : nullptr;
  for (int s = 0; s < n; ++s) {
    const unsigned tag = (unsigned)(t0 + s + 1);
    // A. skip columns, P_LA layers per round: the round's z granules (thread: stream tid >> 5,
    //    channel tid & 31, every layer of the round) and this lane's 8 weights arrive in one round
    //    trip; wave wv accumulates layer l0 + wv of each round into a 16x16 (stream x column)
    //    tile on v_mfma_f32_16x16x4_f32 (8 MFMAs over the layer's 32 channels: A[i = stream][k] =
    //    z, B[k][j = column] = SKIP), summed over the waves once after the last round.  (Round 3's
    //    per-thread FMAs re-read every z row for all 16 columns: ~260 KB of LDS per round.)
    floatx4 pacc = {0.f, 0.f, 0.f, 0.f};
    // rounds are aligned to the END of the stack: the last round is layer L-1 alone, so the
    // round before it finishes while the chains run their last layer and the tail after the
    // chains is one poll + one layer (the first round takes the remainder)
    const int first = (L - 1) % P_LA == 0 ? P_LA : (L - 1) % P_LA;
    const int i16 = lane & 15, kk = lane >> 4;
    for (int l0 = 0, r = 0; l0 < L; l0 += (l0 == 0 ? first : P_LA), ++r) {
      const int nl = l0 == L - 1 ? 1 : (l0 == 0 ? min(first, L) : P_LA), li = l0 + wv;
      float w8[8], zv[P_LA];
      const float* wl = a.skipw + (long)min(li, L - 1) * Cd * Cs + min(scol16 + i16, Cs - 1);
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) w8[s4] = wl[(long)min(4 * s4 + kk, Cd - 1) * Cs];
      sweep<P_LA>(a.zg, (unsigned)((b0 + (zn0 ? zb0 : 0)) * L + l0) * 32 + (zn0 ? zk : 0), 32u, nl, tag, zv, a.status);
      if (tr && s == n - 1) tr[8 + L + 40 + r] = wall_clock64();
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4)
        if (li >= L || 4 * s4 + kk >= Cd || scol16 + i16 >= Cs) w8[s4] = 0.f;
      float* Z = ZS + (r & 1) * (P_LA * 528);   // the other buffer's readers finished last round
#pragma unroll
      for (int i = 0; i < P_LA; ++i) Z[i * 528 + zb0 * 33 + zk] = (zn0 && i < nl) ? zv[i] : 0.f;
      __syncthreads();
      if (tr && s == n - 1) tr[8 + L + 80 + r] = wall_clock64();
      const float* zr = Z + wv * 528 + i16 * 33 + kk;
      float za[8];
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) za[s4] = zr[4 * s4];
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(za[s4], w8[s4], pacc, 0, 0, 0);
      if (tr && s == n - 1) tr[8 + L + r] = wall_clock64();
    }
    // the eight waves' tiles summed through LDS in a fixed order; thread (lane l, e): stream
    // 4(l >> 4) + e, column l & 15
    *(floatx4*)(HP + (wv * 64 + lane) * 4) = pacc;
    __syncthreads();
    if (tid < 256) {
      const int l = tid & 63, e = tid >> 6, sb = 4 * (l >> 4) + e, cc = l & 15;
      float v[8], x = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v[g] = HP[(g * 64 + l) * 4 + e];
#pragma unroll
      for (int g = 0; g < 8; ++g) x += v[g];
      if (sb < B && scol16 + cc < Cs) put_granule(a.sg + (long)(b0 + sb) * Cs + scol16 + cc, tag, x);   // B. publish
    }
    if (tr && s == n - 1) tr[2] = wall_clock64();
    // every head's own stamps (trace only): skip columns published, whole skip vector gathered
    long long* th = (trace && tid == 0 && s == n - 1) ? trace + 2 * L + 136 + 2 * m : nullptr;
    if (th) th[0] = wall_clock64();
    // B. gather the whole skip vector: thread k = tid polls column k of every stream
    if (tid < Cs) {
      // as many granule loads per poll as the group has streams, in fours (a group of 10 polled
      // 16 per thread before: 6 re-reads of its last stream)
      float v[P_MAXB];
      const unsigned o0 = (unsigned)(b0 * Cs + tid);
      if (B <= 4) sweep<4>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[4]>(v), a.status);
      else if (B <= 8) sweep<8>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[8]>(v), a.status);
      else if (B <= 12) sweep<12>(a.sg, o0, (unsigned)Cs, B, tag, *reinterpret_cast<float(*)[12]>(v), a.status);
      else sweep<P_MAXB>(a.sg, o0, (unsigned)Cs, B, tag, v, a.status);
      const float bs = a.bsum ? a.bsum[tid] : 0.f;
#pragma unroll
      for (int bb = 0; bb < P_MAXB; ++bb)
        if (bb < B) RS[bb * 516 + tid] = fmaxf(v[bb] + bs, 0.f);
    }
    __syncthreads();
    if (tr && s == n - 1) tr[3] = wall_clock64();
    if (th) th[1] = wall_clock64();
    // C. h = relu(relu(skip + Σb)·POST1[:, cols] + b1) for this block's 16 columns and all 16
    //    stream slots on v_mfma_f32_16x16x4_f32 (exact f32 products): wave wv takes K rows
    //    64wv .. 64wv+63 (16 MFMAs; A[i = stream][k] = RS, B[k][j = column] = P1T), the eight
    //    16x16 partials are summed through LDS in a fixed order.  (Round 3's per-thread FMA form
    //    re-read each RS row for all 16 columns: ~390 KB of LDS reads, ~1.1 us.)
    {
      const int i16 = lane & 15, kk = lane >> 4, k0 = 64 * wv;
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
      float av[16], bv[16];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        av[s4] = RS[i16 * 516 + k0 + 4 * s4 + kk];
        bv[s4] = P1T[i16 * 516 + k0 + 4 * s4 + kk];
      }
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], bv[s4], acc, 0, 0, 0);
      *(floatx4*)(HP + (wv * 64 + lane) * 4) = acc;   // lane-linear: D[4kk + e][i16]
    }
    if (tr && s == n - 1) tr[8 + L + 120] = wall_clock64();
    __syncthreads();
    if (tr && s == n - 1) tr[8 + L + 121] = wall_clock64();
    if (tid < 256) {   // (stream 4·(tid>>6... : element (lane l = tid & 63, e = tid >> 6) of every wave's D
      const int l = tid & 63, e = tid >> 6, sb = 4 * (l >> 4) + e, cc = l & 15;
      float v[8], hsum = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) v[g] = HP[(g * 64 + l) * 4 + e];
#pragma unroll
      for (int g = 0; g < 8; ++g) hsum += v[g];
      const float b1c = (m * 16 + cc < Cp && a.post1_b) ? a.post1_b[m * 16 + cc] : 0.f;
      HS[sb * 17 + cc] = (m * 16 + cc < Cp) ? fmaxf(hsum + b1c, 0.f) : 0.f;
    }
    __syncthreads();
    if (tr && s == n - 1) tr[8 + L + 122] = wall_clock64();
    // partial logits over this block's 16 h rows: 16 code columns per MFMA block, blocks wv and
    // wv + 8 of the Q/16: A[i = stream][k = r] = HS, B[k][j = code] = P2S; lane (code, 4 streams)
    {
      const int i16 = lane & 15, kk = lane >> 4;
      float av[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) av[s4] = HS[i16 * 17 + 4 * s4 + kk];
      for (int qb = wv; qb < (Q + 15) / 16; qb += 8) {
        const int q = min(16 * qb + i16, Q - 1);
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4], P2S[(4 * s4 + kk) * Q + q], acc, 0, 0, 0);
        if (16 * qb + i16 < Q) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * kk + e < B) put_granule(a.lg + ((long)m * a.B + b0 + 4 * kk + e) * Q + q, tag, acc[e]);
        }
      }
    }
    if (tr && s == n - 1) tr[4] = wall_clock64();
  }
}

// FILT: the chain blocks draw with draw_core_filt (the head blocks are the same code either way).
// RP: the instantiations of ring plans -- the draw stores by the local step mod R, and a stopped run (a
// nonzero status since lbwn_gen_start: 7 from lbwn_gen_extend / lbwn_gen_collect) takes no step; every block
// of the launch reads the word before any of them can have written it.  They are instantiations of their own
// because this kernel's time follows its code layout: the plans without a ring keep the code
// they had.
template <bool LC, bool FILT, bool RP>
__global__ __launch_bounds__(512) void gen_persist_kernel(PersistK a) {
  __shared__ __attribute__((aligned(16))) float sm[G_LDS];
  if constexpr (RP) {
    if (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  }
  const int per = a.Bg + P_NH, g = blockIdx.x / per, r = blockIdx.x % per;
  const int b0 = g * a.Bg, Bg = min(a.Bg, a.B - b0);
  long long* stepc = g ? a.gstep + (g - 1) : a.step;
  long long* trace = g ? nullptr : a.trace;
  if (r < Bg) persist_chain<LC, FILT, RP>(a, sm, b0 + r, stepc, trace);
  else if (r >= a.Bg) persist_head(a, r - a.Bg, sm, b0, Bg, stepc, trace);
  // (a ragged last group leaves chain slots r in [Bg, a.Bg) idle)
}

// the persistent form's wav: its draws store only the code (powf on lane 0 held the next step's
// PRE row behind it); this decodes the run's samples [step - n, step) after the launch
__global__ void gen_decode_kernel(const int* __restrict__ samples, float* __restrict__ wav, const long long* step,
                                  int B, long long max_steps, int n, int Q) {
  const long long t1 = min(*step, max_steps), t0 = max(*step - n, 0LL);
  const long long span = t1 - t0;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)B * span;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = (e / span) * max_steps + t0 + e % span;
    wav[i] = mu_decode_q(samples[i], Q);
  }
}

// the same on a ring plan: stream b's steps [step - n, step) are its local steps t - base_b, each in column
// (t - base_b) mod R (a begin lies between two runs, so base_b <= step - n; n > R decodes the survivors twice)
__global__ void gen_decode_ring_kernel(const int* __restrict__ samples, float* __restrict__ wav, const long long* step,
                                       const long long* sess, int B, unsigned R, int n, int Q) {
  const long long t1 = *step, t0 = max(t1 - n, 0LL);
  const long long span = t1 - t0;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)B * span;
       e += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(e / span);
    const long long i = t0 + e % span - (sess ? sess[4 * b] : 0LL);
    if (i < 0) continue;
    const long c = (long)b * R + ring_col(i, R);
    wav[c] = mu_decode_q(samples[c], Q);
  }
}

}  // namespace

// n_steps steps in one launch (LC plans: n_steps <= NC, their cond-ring rows projected)
int lbwn_gen_persist_run(lbwn_gen_plan* p, const lbwn_params* P, void* ws, int n_steps, hipStream_t st) {
  if (n_steps == 0) return 0;
  PersistK k;
  memset(&k, 0, sizeof(k));
  k.pre = P->pre; k.pre_b = P->pre_b; k.img = gat<float>(ws, p->oGIMG);
  k.gc_proj = p->a.n_gc_embed > 0 ? gat<float>(ws, p->oGCP) : nullptr;
  k.rings = gat<float>(ws, p->oRING); k.step = gat<long long>(ws, p->oSTEP); k.code_in = gat<int>(ws, p->oCODE);
  k.B = p->B; k.L = p->L; k.nbl = p->nbl; k.Cr = p->Cr; k.Cd = p->Cd; k.pre_bias = p->pre_bias; k.n_steps = n_steps;
  unsigned long long* g = gat<unsigned long long>(ws, p->oGRAN);
  k.zg = g; k.sg = g + (long)p->B * p->L * 32; k.lg = k.sg + (long)p->B * p->Cs;
  k.Cs = p->Cs; k.Cp = p->Cp; k.Q = p->Q;
  k.skipw = P->skip; k.bsum = P->skip_b ? gat<float>(ws, p->oBSUM) : nullptr;
  k.post1 = P->post1; k.post1_b = P->post1_b; k.post2 = P->post2;
  k.draw = draw_args(p, P, ws);
  k.status = gat<int>(ws, p->oSTEP + 8);
  k.trace = p->trace ? gat<long long>(ws, p->oTRACE) : nullptr;
  k.Bg = p->pbg;
  k.gstep = reinterpret_cast<long long*>(g + p->n_gran_core);
  const int nblk = p->pgroups * (p->pbg + P_NH);
  const bool lc = p->Lo > 0, filt = gen_filtered(p);
  if (lc) { k.lccond = gat<float>(ws, p->oLCC); k.NC = p->NC; }
  const auto kern = p->ring ? (lc ? (filt ? gen_persist_kernel<true, true, true> : gen_persist_kernel<true, false, true>)
                                  : (filt ? gen_persist_kernel<false, true, true> : gen_persist_kernel<false, false, true>))
                            : (lc ? (filt ? gen_persist_kernel<true, true, false> : gen_persist_kernel<true, false, false>)
                                  : (filt ? gen_persist_kernel<false, true, false> : gen_persist_kernel<false, false, false>));
  kern<<<nblk, 512, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_gen_decode_launch(const lbwn_gen_plan* p, void* ws, int n_steps, hipStream_t st) {
  if (p->ring) {
    gen_decode_ring_kernel<<<std::max(1, std::min(1024, (int)(((long long)p->B * n_steps + 255) / 256))), 256, 0, st>>>(
        gat<int>(ws, p->oSAMP), gat<float>(ws, p->oWAV), gat<long long>(ws, p->oSTEP),
        p->sess_mode ? gat<long long>(ws, p->oSESS) : nullptr, p->B, (unsigned)p->ring, n_steps, p->Q);
    LBWN_CHECK_LAUNCH();
    return 0;
  }
  gen_decode_kernel<<<std::max(1, std::min(1024, (int)(((long long)p->B * n_steps + 255) / 256))), 256, 0, st>>>(
      gat<int>(ws, p->oSAMP), gat<float>(ws, p->oWAV), gat<long long>(ws, p->oSTEP), p->B, p->max_steps, n_steps,
      p->Q);
  LBWN_CHECK_LAUNCH();
  return 0;
}
