// The persistent forward chain (all L layers in one launch) in its three forms: chain_fwd_kernel
// (32-position waves; f32 or bf16-split weight images) and chain_fwd16_kernel<4 | 8> (16-position
// waves), with their launcher.
#include "common.h"
#include "kernels.h"
#include "layer_common.h"

namespace {

// ---- persistent forward chain -------------------------------------------------------------
// The 50 dependent layers as ONE launch.  A block owns a 128-position tile of one stream for
// every layer; its own rows stay in LDS (double-buffered x_l / x_{l+1}), and only the dilated
// tap's halo (rows t0-d .. t0-1: min(d,128) rows of ONE producer tile of the same stream, or
// SAVE) crosses blocks.  Hand-off (cdna_hip_programming §6 G16, R1 form): the producer stores
// x_{l+1} write-through (sc1), every wave drains (s_waitcnt vmcnt(0)), block barrier, one
// lane stores flag[tile] = l+1 (relaxed, agent); the consumer polls that word relaxed from one
// lane, barriers, and reads the halo ONLY with sc1 loads (no acquire fence needed).  The own
// tap (W1·x[t]) is computed before the poll so the hand-off latency hides behind it.
// Deadlock freedom: tiles run in rounds of gridDim.x ≤ resident blocks, in increasing tile
// order; a producer tile is always in the same round (resident) or an earlier one (done).
// Every spin is bounded (SPIN_TIMEOUT) and reports through the status word.

// orders this wave's LDS writes before its later LDS reads of another lane's data (LDS ops of
// one wave are performed in issue order; this stops hipcc from reordering them) — no barrier
LBWN_DEV void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lc·[LC_SIGNAL_l | LC_GATE_l] onto the accumulators (tmodel.py:155-160): A = the layer's LC
// image rows (out channel), B = this lane's LC input row, pre-split once per tile (lcb); the
// fragments of k-step s+1 are read while step s's MFMAs issue
LBWN_DEV void lc_terms(const unsigned short* LI, const bf16x8 (&lcb)[LC_K][3], int pi, int h, floatx16& acc_s,
                       floatx16& acc_g) {
  bf16x8 fs[2][3], fg[2][3];
  auto load = [&](int s2, int buf) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      fs[buf][p] = *(const bf16x8*)(LI + pi * LC_ROW + LC_KP * p + 16 * s2 + 8 * h);
      fg[buf][p] = *(const bf16x8*)(LI + (32 + pi) * LC_ROW + LC_KP * p + 16 * s2 + 8 * h);
    }
  };
  load(0, 0);
#pragma unroll
  for (int s2 = 0; s2 < LC_K; ++s2) {
    const int cb = s2 & 1;
    if (s2 + 1 < LC_K) load(s2 + 1, cb ^ 1);
    acc_s = mfma_x3(fs[cb], lcb[s2], acc_s);
    acc_g = mfma_x3(fg[cb], lcb[s2], acc_g);
  }
}

// one layer's LC image into LDS by LDS-DMA (wave w moves pieces w, w+4, ...); landed by the
// caller's next vmcnt drain + barrier
LBWN_DEV void dma_lc_image(const unsigned short* lcimg, int l, float* LCI, int w, int lane) {
  const float* src = (const float*)lcimg + (long)l * LCIMG_F + lane * 4;
#pragma unroll
  for (int i = 0; i < (LCIMG_F / 256 + 3) / 4; ++i) {
    const int pc = w + 4 * i;
    if (pc < LCIMG_F / 256) dma16(src + pc * 256, LCI + pc * 256);
  }
}

// conv_half on the bf16 cores: acc += Wkᵀ·x over one tap (2 k-steps of 16 channels, sig and
// gate), Wt = the split image's WT at this tap (bf16, rows XW_ROW), x split on the fly
LBWN_DEV void conv_half_x3(const float* xrow, const unsigned short* Wt, int pi, int h, floatx16& acc_s, floatx16& acc_g) {
  floatx4 xv[4];
  bf16x8 ws_[2][3], wg_[2][3];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    xv[2 * c] = *(const floatx4*)(xrow + 16 * c + 8 * h);
    xv[2 * c + 1] = *(const floatx4*)(xrow + 16 * c + 8 * h + 4);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      ws_[c][p] = *(const bf16x8*)(Wt + pi * XW_ROW + 32 * p + 16 * c + 8 * h);
      wg_[c][p] = *(const bf16x8*)(Wt + (32 + pi) * XW_ROW + 32 * p + 16 * c + 8 * h);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    bf16x8 xb[3];
    split8(xv[2 * c], xv[2 * c + 1], xb);
    acc_s = mfma_x3(ws_[c], xb, acc_s);
    acc_g = mfma_x3(wg_[c], xb, acc_g);
  }
}

constexpr int CF_LDS = 3 * LP * XS + 2 * WIMG;      // Xc[2] | HALO | IMG[2]  (99.8 KB)
constexpr int CF_LDS_X3 = 3 * LP * XS + 2 * XIMG_F;  // with split images (120.6 KB)
constexpr int CF_LDS_X3LC = CF_LDS_X3 + LCIMG_F;      // + one LC image (151.6 KB)
static_assert(CF_LDS_X3LC * 4 + 16 <= 160 * 1024, "chain fwd x3 + LC LDS");

// Per layer l (weight image IMG[l&1]):
//   wait for the producer tile's x_l, halo rows (sc1 loads), barrier;
//   dilated tap W0·x[t-d] onto the accumulators that already hold W1·x[t] (done last layer);
//   gate; residual → x_{l+1} to LDS and (sc1) to HBM;
//   the NEXT layer's own tap W1'·x_{l+1}[t]: it reads only rows this wave just wrote, so it needs
//   no barrier and runs while the x stores drain; then drain, barrier, publish, z store, and
//   the image of layer l+2 into IMG[l&1] (dead after that barrier; first read after the next
//   layer's halo barrier).  Double-buffered images are what let the own tap move: one image
//   forced a barrier between this layer's last read and the next layer's first.
// X3: the conv and residual products on the bf16 cores from split images (ChainFK::ximg);
// otherwise v_mfma_f32_32x32x2_f32 from the f32 images.
// LC (X3 only): the LC term lc·LC_l computed in the chain (no [M][L·2Cd] COND round trip): the
// tile's LC input rows are split once into registers; the layer's LC image (one LDS buffer) is
// read with the own tap in step 7 of the previous layer (tile start for layer 0), and the image
// two layers ahead is LDS-DMA'd in step 9, after the publish barrier (every wave is past its
// reads), landing with the next layer's halo loads (in-order vmcnt) before its halo barrier.
// TR: the traced build (in-kernel clock stamps, lbwn_plan's LBWN_CHAIN_TRACE): the stamps'
// lane-divergent branches cost the untraced chains 0.5-3 % (same-box A/B, tools/ab_step.sh)
template <bool X3, bool LC, int CM, bool TR>
__global__ __launch_bounds__(256) void chain_fwd_kernel(ChainFK a) {
  static_assert(X3 || !LC, "in-chain LC needs the split images");
  constexpr int IMGF = X3 ? XIMG_F : WIMG;              // floats per layer image
  constexpr int PF = (IMGF / 4 + 255) / 256;            // float4 per thread to prefetch one
  __shared__ __attribute__((aligned(16))) float sm[LC ? CF_LDS_X3LC : X3 ? CF_LDS_X3 : CF_LDS];
  __shared__ int s_fail;
  float* HALO = sm + 2 * LP * XS;
  float* IMG0 = HALO + LP * XS;
  // f32: [W 64×WS | R 32×XS | bs 64 | br 32]; X3: [WT | RT | bs 64 | br 32] (bf16 + f32)
  auto img = [&](int l) { return IMG0 + (l & 1) * IMGF; };
  float* LCI = IMG0 + 2 * IMGF;   // LC: the one LC image buffer
  const unsigned short* LCIu = (const unsigned short*)LCI;
  const float* wsrc = X3 ? (const float*)a.ximg : a.wpack;
  auto bias_of = [&](const float* im) { return X3 ? im + XB_OFF / 2 : im + 64 * WS + 32 * XS; };

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pi = lane & 31, h = lane >> 5;
  const int r = 32 * w + pi;  // this lane's row of the tile
  const int tps = (a.T + LP - 1) / LP, ntiles = a.B * tps;
  if (tid == 0) s_fail = 0;
  const int first = chain_first(a.xcd);
  for (int tile = first; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, tt = tile % tps, t0 = tt * LP;
    const int t = t0 + r;
    const bool valid = t < a.T;
    const long m = (long)b * a.T + t;
    const long sb = (long)b * (a.H + a.T) * 32;  // stream base inside a layer buffer
    constexpr bool has_cond = CM != 0;
    const int myid = (a.gc_tab && valid) ? a.ids[m] : 0;
    floatx4 cv[8];
    load_cond<CM>(a, 0, myid, m, valid && has_cond, h, cv);
    // LC: this lane's LC input row, split once for the tile (B operand: k = 16s + 8h + j)
    bf16x8 lcb[LC_K][3];
    if (LC) {
      const float* lrow = a.lcact + ((long)b * a.T + min(t, a.T - 1)) * a.Lo;
#pragma unroll
      for (int s2 = 0; s2 < LC_K; ++s2) {
        const int k0 = 16 * s2 + 8 * h;
        floatx4 u = *(const floatx4*)(lrow + min(k0, a.Lo - 4));       // clamped, then select
        floatx4 v = *(const floatx4*)(lrow + min(k0 + 4, a.Lo - 4));
        if (k0 >= a.Lo) u = floatx4{0.f, 0.f, 0.f, 0.f};
        if (k0 + 4 >= a.Lo) v = floatx4{0.f, 0.f, 0.f, 0.f};
        split8(u, v, lcb[s2]);
      }
    }
    __syncthreads();  // previous tile's LDS use done
    if (LC) dma_lc_image(a.lcimg, 0, LCI, w, lane);
    {  // images of layers 0 and 1 (contiguous in both places): every load issued before the first
       // store (a load-store loop waited out one round trip per iteration)
      constexpr int NI = (2 * IMGF / 4 + 255) / 256;
      const int nimg4 = min(a.L, 2) * IMGF / 4;
      floatx4 iv[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) iv[i] = *(const floatx4*)(wsrc + 4 * min(tid + 256 * i, nimg4 - 1));
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int e = tid + 256 * i;
        if (e < nimg4) *(floatx4*)(img(0) + 4 * e) = iv[i];
      }
    }
    stage_rows(sm, a.X + sb, t0, 0, a.T, a.H, 32, tid);  // x_0 (embed output, pre-launch)
    if (LC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LC image DMA
    __syncthreads();
    // layer 0's own tap W1·x_0[t] (+ its LC term)
    floatx16 acc_s, acc_g;
    conv_init(bias_of(img(0)), cv, h, acc_s, acc_g);
    if (has_cond && a.L > 1) load_cond<CM>(a, 1, myid, m, valid, h, cv);
    if (X3) conv_half_x3(sm + r * XS, (const unsigned short*)img(0) + 96, pi, h, acc_s, acc_g);
    else conv_half(sm + r * XS, img(0) + 32 * WS, pi, h, acc_s, acc_g);
    if (LC) {
      lc_terms(LCIu, lcb, pi, h, acc_s, acc_g);
      if (a.L > 1) {
        __syncthreads();   // every wave is past its LC_0 reads
        dma_lc_image(a.lcimg, 1, LCI, w, lane);   // lands with layer 0's halo loads
      }
    }
    const bool trc = a.trace && (int)blockIdx.x == a.trace_blk && tid == 0 && tile == first;
#define FSTAMP(i) if (TR && trc) a.trace[16 * l + (i)] = clock64()
    auto store_zs = [&](int ll, const floatx16& zz, const floatx16& ss) {
      if (valid) store_rows16(a.Z + m * a.ldz + (long)ll * a.Cd, zz, a.Cd, h);
      if (X3 && a.SG && valid) {
        float* sgl = a.SG + (long)ll * a.sgls;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *(floatx4*)(sgl + sg_off(m, q, h)) = floatx4{ss[4 * q], ss[4 * q + 1], ss[4 * q + 2], ss[4 * q + 3]};
      }
    };
    for (int l = 0; l < a.L; ++l) {
      FSTAMP(0);
      const int d = 1 << (l % a.nbl);
      float* cur = sm + (l & 1) * LP * XS;
      float* nxt = sm + ((l + 1) & 1) * LP * XS;
      float* xl = a.X + (long)l * a.xls + sb;
      const float* Wl = img(l);
      const float* Rs = Wl + 64 * WS;
      const float* br = bias_of(Wl) + 64;
      floatx4 pf[PF];   // image of layer l+2, loaded in step 3
      FSTAMP(1);
      // 2. wait for the producer of the halo rows (x_l is layer l-1's output)
      const int ptt = tt - max(1, d / LP);
      if (l > 0 && ptt >= 0) {
        if (tid == 0 && !s_fail) {
          if (!wait_flag_ge(a.flags + (long)b * tps + ptt, (unsigned)l, a.status, 1u)) s_fail = 1;
        }
        __syncthreads();
      }
      FSTAMP(2);
      // 3. halo rows [0, min(d,LP)): x_l rows t0-d+row (SAVE rows when < 0), sc1 loads
      {
        const int nh = min(d, LP);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(xl, (short)0, (int)((long)(a.H + a.T) * 32 * 4), BUF_DW3);
        floatx4 hv[4];   // all four issued before the first is stored (clamped rows)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = min(tid + 256 * i, nh * 8 - 1), row = e >> 3, c4 = (e & 7) * 4;
          hv[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((a.H + t0 + row - d) * 32 + c4) * 4, 0, 16);
        }
        // 1. prefetch the image of layer l+2 (pre-launch data: plain loads, clamped: no branch),
        //    issued BEHIND the halo loads: the halo wait then leaves them in flight (vmcnt(PF)),
        //    where in front of the producer poll they were waited out by lane 0's vmcnt(0)
        //    (unconditional, at a clamped layer: a skipped branch made hipcc wait as if they were
        //    not in flight)
        {
          const floatx4* src = (const floatx4*)(wsrc + (long)min(l + 2, a.L - 1) * IMGF);
#pragma unroll
          for (int i = 0; i < PF; ++i) pf[i] = src[min(tid + 256 * i, IMGF / 4 - 1)];
        }
        // every HALO row written (rows >= nh get a copy of row nh-1 and are never read: only rows
        // r < d are): a store behind `e < nh*8` made hipcc sink the 4th load into that branch,
        // issued after the first three had drained (one more L2 round trip per layer)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i;
          *(floatx4*)(HALO + (e >> 3) * XS + (e & 7) * 4) = hv[i];
        }
      }
      __syncthreads();
      FSTAMP(3);
      // 4. residual weights read now (they wait behind the conv, not in front of the residual)
      float ra[16];
      bf16x8 rf[2][3];   // X3: RT fragments of the two 16-channel k-steps
      if (X3) {
        const unsigned short* rt = (const unsigned short*)Wl + 64 * XW_ROW + pi * XR_ROW + 8 * h;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int p = 0; p < 3; ++p) rf[s2][p] = *(const bf16x8*)(rt + 32 * p + 16 * s2);
      } else {
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) ra[s2] = Rs[acc_row(s2, h) * XS + pi];
      }
      __builtin_amdgcn_sched_barrier(0);
      // 5. dilated tap W0·x[t-d], gate
      const float* xp = (r >= d) ? cur + (r - d) * XS : HALO + r * XS;
      if (X3) conv_half_x3(xp, (const unsigned short*)Wl, pi, h, acc_s, acc_g);
      else conv_half(xp, Wl, pi, h, acc_s, acc_g);
      floatx16 z, sgv;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float sq;
        z[q] = gate_zs(acc_s[q], acc_g[q], sq);
        sgv[q] = sq;
      }
      FSTAMP(4);
      if (l + 1 < a.L) {
        // 6. residual: x_{l+1} = x_l + br + RES·z → LDS (next layer's rows) and HBM (sc1)
        floatx16 acc_r;
        const float* xc = cur + r * XS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 xv = *(const floatx4*)(xc + 8 * q + 4 * h);
          const floatx4 bv = *(const floatx4*)(br + 8 * q + 4 * h);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc_r[4 * q + j] = xv[j] + bv[j];
        }
        if (X3) {
          // z (acc layout) is the B operand: registers 8s..8s+7 form k-step s (RT holds the
          // matching permuted channel order)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 zb[3];
            split8(floatx4{z[8 * s2], z[8 * s2 + 1], z[8 * s2 + 2], z[8 * s2 + 3]},
                   floatx4{z[8 * s2 + 4], z[8 * s2 + 5], z[8 * s2 + 6], z[8 * s2 + 7]}, zb);
            acc_r = mfma_x3(rf[s2], zb, acc_r);
          }
        } else {
#pragma unroll
          for (int s2 = 0; s2 < 16; ++s2) acc_r = mfma32(ra[s2], z[s2], acc_r);
        }
        float* xn = a.X + (long)(l + 1) * a.xls + sb;
        const __amdgpu_buffer_rsrc_t rn =
            __builtin_amdgcn_make_buffer_rsrc(xn, (short)0, (int)((long)(a.H + a.T) * 32 * 4), BUF_DW3);
        float* nrow = nxt + r * XS;
        // only the rows the next layer's consumer tile reads (the last min(d_{l+1}, LP)) cross
        // CUs inside this launch: those are written through (sc1) and drained before the publish;
        // the rest are plain stores, read after the launch (backward, SAVE).  Writing every row
        // through cost ~3k cycles per layer (drain 2.4k + slower issue; tools/fwd_abl.sh)
        const bool halo_row = r >= LP - min(1 << ((l + 1) % a.nbl), LP);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 v = floatx4{acc_r[4 * q], acc_r[4 * q + 1], acc_r[4 * q + 2], acc_r[4 * q + 3]};
          *(floatx4*)(nrow + 8 * q + 4 * h) = v;
          const int off = ((a.H + t) * 32 + 8 * q + 4 * h) * 4;
          if (valid && halo_row) __builtin_amdgcn_raw_buffer_store_b128(v, rn, off, 0, 16);
          if (valid && !halo_row) __builtin_amdgcn_raw_buffer_store_b128(v, rn, off, 0, 0);
        }
        FSTAMP(8);
        // 7. the next layer's own tap from the row this wave just wrote (wave-local: no barrier)
        //    while the x stores drain; its image IMG[(l+1)&1] landed before this layer's barriers
        wave_lds_fence();
        const float* Wn = img(l + 1);
        conv_init(bias_of(Wn), cv, h, acc_s, acc_g);
        if (has_cond && l + 2 < a.L) load_cond<CM>(a, l + 2, myid, m, valid, h, cv);
        if (X3) conv_half_x3(nrow, (const unsigned short*)Wn + 96, pi, h, acc_s, acc_g);
        else conv_half(nrow, Wn + 32 * WS, pi, h, acc_s, acc_g);
        if (LC) lc_terms(LCIu, lcb, pi, h, acc_s, acc_g);   // LC_{l+1}: landed before this layer's halo barrier
      }
      FSTAMP(5);
      // 8. publish x_{l+1}: every wave drains its sc1 stores, barrier, one lane signals
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      FSTAMP(9);
      __syncthreads();
      FSTAMP(10);
      if (tid == 0 && l + 1 < a.L) publish_flag(a.flags + tile, (unsigned)(l + 1));
      // 9. image of layer l+2 into IMG[l&1] (everyone is past this layer's reads of it; its loads
      //    landed with the drain), and the LC image of layer l+2 (LC_{l+1} was read in step 7,
      //    before the publish barrier)
      if (LC && l + 2 < a.L) dma_lc_image(a.lcimg, l + 2, LCI, w, lane);
      if (l + 2 < a.L) {
        float* dst = IMG0 + (l & 1) * IMGF;
#pragma unroll
        for (int i = 0; i < PF; ++i) {
          const int e = tid + 256 * i;
          if (e < IMGF / 4) *(floatx4*)(dst + 4 * e) = pf[i];
        }
      }
      FSTAMP(6);
      // 10. z (skip GEMM input) and σ rows, issued last: they drain in the shadow of the next
      //     layer (written before the image, the image writes' vmcnt waits waited them out)
      // (stored during the next layer instead, after its halo barrier, they lengthened that
      // layer's publish drain: forward 276 -> 287 us, same box)
      store_zs(l, z, sgv);
      FSTAMP(7);
    }
#undef FSTAMP
  }
}

// ---- forward chain, 16-position waves (round 4) ---------------------------------------------
// chain_fwd16_kernel<NW, LC, CM, TR>: the X3 forward chain on v_mfma_f32_16x16x32_bf16 with 16
// positions per wave and NW waves per block: tile TP = 16·NW positions (the C4 tile axis:
// NW = 8 → 128 positions with TWO waves per SIMD, NW = 4 → 64 positions).  The per-layer protocol
// (halo hand-off, own tap of the next layer inside the store drain, double-buffered images, the
// LC image two layers ahead) is chain_fwd_kernel's; what changes is the MFMA geometry:
//   lane = (j = lane & 15: the wave's position, g = lane >> 4), and with q0 = 2(g >> 1), h = g & 1
//   the lane's accumulator block b (0, 1) register r holds channel 8(q0 + b) + 4h + r — the same
//   (q, h) channel groups chain_fwd_kernel's lanes hold, so z / σ go to the same rows / sg_off
//   blocks and the residual's B operand (the lane's 8 z values) is in the split image's RT k order
//   unchanged.  For that, conv A row i of block b reads out channel ch16(b, i) (the permutation
//   that puts D row i = 4g + r on that channel).  The residual's rows are unpermuted: x_{l+1}
//   block rb register r = channel 16rb + 4g + r.
// Per wave and layer: conv 2 taps × (sig, gate) × 2 blocks × 6 products = 48 MFMAs of 16 cycles,
// residual 2 blocks × 6 = 12 — per position the MFMA work of chain_fwd_kernel, in half the
// positions per wave, so two waves share each SIMD at NW = 8 and hide each other's latencies.

template <int NW>
LBWN_DEV void dma_lc16_image(const unsigned short* lcimg, int l, float* LCI, int w, int lane) {
  const float* src = (const float*)lcimg + (long)l * LC16IMG_F + lane * 4;
  constexpr int NP = LC16IMG_F / 256;
#pragma unroll
  for (int i = 0; i < (NP + NW - 1) / NW; ++i) {
    const int pc = w + NW * i;
    if (pc < NP) dma16(src + pc * 256, LCI + pc * 256);
  }
}

// GC / COND term of layer l for this lane's channels: cv[2·kind + b] = channels 8(q0+b)+4h..+3
// (kind 0 sig, 1 gate); CM as load_cond
template <int CM>
LBWN_DEV void load_cond16(const ChainFK& a, int l, int myid, long m, bool valid, int q0, int h, floatx4 (&cv)[4]) {
  if (CM == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  if (CM == 1) {
    const float* g = a.gc_tab + (long)myid * a.gc_ld + (long)l * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] = *(const floatx4*)(g + 32 * (i >> 1) + 8 * (q0 + (i & 1)) + 4 * h);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) cv[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (!valid) return;
  if (a.gc_tab) {
    const float* g = a.gc_tab + (long)myid * a.gc_ld + (long)l * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] += *(const floatx4*)(g + 32 * (i >> 1) + 8 * (q0 + (i & 1)) + 4 * h);
  }
  if (a.cond) {
    const float* c = a.cond + m * a.ldcond + (long)l * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] += *(const floatx4*)(c + 32 * (i >> 1) + 8 * (q0 + (i & 1)) + 4 * h);
  }
}

// acc[2·kind + b] = bias + conditioning
LBWN_DEV void conv16_init(const float* bs, const floatx4 (&cv)[4], int q0, int h, floatx4 (&acc)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const floatx4 bv = *(const floatx4*)(bs + 32 * (i >> 1) + 8 * (q0 + (i & 1)) + 4 * h);
    acc[i] = bv + cv[i];
  }
}

// acc += Wtapᵀ·x for one tap: Wt = the split image's WT at this tap (rows XW_ROW), xrow = this
// lane's position row in LDS (channels 8g..8g+7 = the B operand's k group); the operands of each
// of the NP parts (4 / NP accumulator blocks) are read before its MFMAs (NP = 2 halves the live
// fragments for the register-tight LC form)
template <int NP = 1>
LBWN_DEV void conv16_tap_x(floatx4 x0, floatx4 x1, const unsigned short* Wt, int i16, int g, floatx4 (&acc)[4]) {
  bf16x8 xb[3];
#pragma unroll
  for (int part = 0; part < NP; ++part) {
    constexpr int NB = 4 / NP;
    bf16x8 wf[NB][3];
#pragma unroll
    for (int ii = 0; ii < NB; ++ii) {
      const int i = part * NB + ii, o = 32 * (i >> 1) + ch16(i & 1, i16);
#pragma unroll
      for (int p = 0; p < 3; ++p) wf[ii][p] = *(const bf16x8*)(Wt + o * XW_ROW + 32 * p + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (part == 0) split8(x0, x1, xb);
#pragma unroll
    for (int ii = 0; ii < NB; ++ii) acc[part * NB + ii] = mfma16x3(wf[ii], xb, acc[part * NB + ii]);
  }
}
template <int NP = 1>
LBWN_DEV void conv16_tap(const float* xrow, const unsigned short* Wt, int i16, int g, floatx4 (&acc)[4]) {
  conv16_tap_x<NP>(*(const floatx4*)(xrow + 8 * g), *(const floatx4*)(xrow + 8 * g + 4), Wt, i16, g, acc);
}

// lc·[LC_SIGNAL_l | LC_GATE_l] onto the accumulators: A = LC16 image rows, B = the lane's LC input
// row (k = 32s + 8g + j), held as raw f32 (lcv: 24 registers instead of 36 pre-split: at two
// waves per SIMD the split form spilled) and split per k-step
LBWN_DEV void lc16_terms(const unsigned short* LI, const floatx4 (&lcv)[6], int i16, int g, floatx4 (&acc)[4]) {
#pragma unroll
  for (int s2 = 0; s2 < 3; ++s2) {
    bf16x8 xb[3];
    split8(lcv[2 * s2], lcv[2 * s2 + 1], xb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = 32 * (i >> 1) + ch16(i & 1, i16);
      bf16x8 wf[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) wf[p] = *(const bf16x8*)(LI + o * LC16_ROW + LC16_KP * p + 32 * s2 + 8 * g);
      acc[i] = mfma16x3(wf, xb, acc[i]);
    }
  }
}

template <int NW>
constexpr int cf16_lds(bool lc) { return 3 * 16 * NW * XS + 2 * XIMG_F + (lc ? LC16IMG_F : 0); }
static_assert(cf16_lds<8>(true) * 4 + 16 <= 160 * 1024, "chain fwd16 + LC LDS");

template <int NW, bool LC, int CM, bool TR>
__global__ __launch_bounds__(64 * NW) void chain_fwd16_kernel(ChainFK a) {
  constexpr int TP = 16 * NW, NT = 64 * NW;
  constexpr int IMGF = XIMG_F;
  // the LC form (register-tight at two waves per SIMD) moves the image of layer l+2 by LDS-DMA
  // after the publish barrier (landing with the next layer's halo loads, like the LC image);
  // the others prefetch it into registers behind the halo loads and write it after the barrier
  constexpr bool DMAIMG = LC;
  // per-wave halo (below)
  constexpr bool WH = true;
  // LC form: the LC term of layer l+1 (72 MFMAs per wave) runs after layer l's publish instead of
  // inside its store drain, where it outlasted the drain and held the publish back; its image is
  // DMA'd during layer l (after the dilated tap: ahead of the halo loads it would have held their
  // vmcnt waits) into the single LCI buffer, which nothing reads between layer l's top barrier and
  // its publish barrier
  constexpr bool LCLATE = LC;
  constexpr int PF = DMAIMG ? 1 : (IMGF / 4 + NT - 1) / NT;   // float4 per thread to prefetch one image
  constexpr int NR = TP * 8 / NT;                       // float4 per thread of a TP-row tile (2)
  __shared__ __attribute__((aligned(16))) float sm[cf16_lds<NW>(LC)];
  __shared__ int s_fail;
  float* HALO = sm + 2 * TP * XS;
  float* IMG0 = HALO + TP * XS;
  auto img = [&](int l) { return IMG0 + (l & 1) * IMGF; };
  float* LCI = IMG0 + 2 * IMGF;
  const unsigned short* LCIu = (const unsigned short*)LCI;
  const float* wsrc = (const float*)a.ximg;
  auto bias_of = [&](const float* im) { return im + XB_OFF / 2; };

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4, q0 = 2 * (g >> 1), h = g & 1;
  const int r = 16 * w + i16;  // this lane's row of the tile
  const int tps = (a.T + TP - 1) / TP, ntiles = a.B * tps;
  if (tid == 0) s_fail = 0;
  const int first = chain_first(a.xcd);
  for (int tile = first; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, tt = tile % tps, t0 = tt * TP;
    const int t = t0 + r;
    const bool valid = t < a.T;
    const long m = (long)b * a.T + t;
    const long sb = (long)b * (a.H + a.T) * 32;
    constexpr bool has_cond = CM != 0;
    const int myid = (a.gc_tab && valid) ? a.ids[m] : 0;
    floatx4 cv[4];
    load_cond16<CM>(a, 0, myid, m, valid && has_cond, q0, h, cv);
    floatx4 lcv[6];   // LC: this lane's LC input row, k = 32s + 8g + 0..7 (zero past n_lc_out)
    if (LC) {
      const float* lrow = a.lcact + ((long)b * a.T + min(t, a.T - 1)) * a.Lo;
#pragma unroll
      for (int s2 = 0; s2 < 3; ++s2) {
        const int k0 = 32 * s2 + 8 * g;
        lcv[2 * s2] = *(const floatx4*)(lrow + min(k0, a.Lo - 4));       // clamped, then select
        lcv[2 * s2 + 1] = *(const floatx4*)(lrow + min(k0 + 4, a.Lo - 4));
        if (k0 >= a.Lo) lcv[2 * s2] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (k0 + 4 >= a.Lo) lcv[2 * s2 + 1] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();  // previous tile's LDS use done
    if (LC) dma_lc16_image<NW>(a.lcimg, 0, LCI, w, lane);
    {  // images of layers 0 and 1, every load before the first store
      constexpr int NI = (2 * IMGF / 4 + NT - 1) / NT;
      const int nimg4 = min(a.L, 2) * IMGF / 4;
      floatx4 iv[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) iv[i] = *(const floatx4*)(wsrc + 4 * min(tid + NT * i, nimg4 - 1));
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int e = tid + NT * i;
        if (e < nimg4) *(floatx4*)(img(0) + 4 * e) = iv[i];
      }
    }
    {  // x_0 rows (embed output, pre-launch): unconditional clamped loads, then select
      const float* xb = a.X + sb;
      floatx4 v[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int e = tid + NT * i, rr = e >> 3, c4 = (e & 7) * 4;
        v[i] = *(const floatx4*)(xb + (long)(a.H + min(t0 + rr, a.T - 1)) * 32 + c4);
        if (t0 + rr >= a.T) v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int e = tid + NT * i;
        *(floatx4*)(sm + (e >> 3) * XS + (e & 7) * 4) = v[i];
      }
    }
    if (LC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LC image DMA
    __syncthreads();
    // layer 0's own tap W1·x_0[t] (+ its LC term)
    floatx4 acc[4];
    conv16_init(bias_of(img(0)), cv, q0, h, acc);
    if (has_cond && a.L > 1) load_cond16<CM>(a, 1, myid, m, valid, q0, h, cv);
    conv16_tap<LC ? 2 : 1>(sm + r * XS, (const unsigned short*)img(0) + 96, i16, g, acc);
    if (LC) {
      lc16_terms(LCIu, lcv, i16, g, acc);
      if (a.L > 1) {
        __syncthreads();   // every wave is past its LC_0 reads
        dma_lc16_image<NW>(a.lcimg, 1, LCI, w, lane);   // lands with layer 0's halo loads
      }
    }
    const bool trc = a.trace && (int)blockIdx.x == a.trace_blk && tid == 0 && tile == first;
#define FSTAMP(i) if (TR && trc) a.trace[16 * l + (i)] = clock64()
    for (int l = 0; l < a.L; ++l) {
      FSTAMP(0);
      const int d = 1 << (l % a.nbl);
      float* cur = sm + (l & 1) * TP * XS;
      float* nxt = sm + ((l + 1) & 1) * TP * XS;
      float* xl = a.X + (long)l * a.xls + sb;
      const float* Wl = img(l);
      const float* br = bias_of(Wl) + 64;
      floatx4 pf[PF];
      FSTAMP(1);
      const int ptt = tt - max(1, d / TP);
      floatx4 hx[2];   // WH: this lane's halo row x[t0 + r - d], channels 8g..8g+7 (rows r < d)
      // (zeroed in the LC form: left undefined on the waves that do not load it, the registers
      // stayed live around the loop there and spilled; zeroed in the others, C2's forward measured
      // 206 -> 216 us)
      if (LC) hx[0] = hx[1] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (WH) {
        // per-wave halo: only the waves holding rows r < d wait for the producer (one lane polls)
        // and load their lanes' halo rows into registers; the rest start the layer at once, so a
        // SIMD's other wave computes through the hand-off.  The barrier here only publishes the
        // image written after the last layer's end barrier (the own tap of the next layer reads it
        // before any later barrier)
        // (DMAIMG: the images of layer l+1 DMA'd at the end of the last layer land first)
        if (DMAIMG && l > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (l > 0) __syncthreads();
        FSTAMP(2);
        const int nh = min(d, TP);
        if (16 * w < nh) {
          if (l > 0 && ptt >= 0 && lane == 0 && !s_fail) {
            if (!wait_flag_ge(a.flags + (long)b * tps + ptt, (unsigned)l, a.status, 1u)) s_fail = 1;
          }
          const __amdgpu_buffer_rsrc_t rs =
              __builtin_amdgcn_make_buffer_rsrc(xl, (short)0, (int)((long)(a.H + a.T) * 32 * 4), BUF_DW3);
          const int off = ((a.H + t0 + min(r, nh - 1) - d) * 32 + 8 * g) * 4;
          hx[0] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
          hx[1] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 16);
        }
        if (!DMAIMG) {   // the image of layer l+2 behind the halo loads
          const floatx4* src = (const floatx4*)(wsrc + (long)min(l + 2, a.L - 1) * IMGF);
#pragma unroll
          for (int i = 0; i < PF; ++i) pf[i] = src[min(tid + NT * i, IMGF / 4 - 1)];
        }
      } else {
      // wait for the producer of the halo rows
      if (l > 0 && ptt >= 0) {
        if (tid == 0 && !s_fail) {
          if (!wait_flag_ge(a.flags + (long)b * tps + ptt, (unsigned)l, a.status, 1u)) s_fail = 1;
        }
        __syncthreads();
      }
      FSTAMP(2);
      {  // halo rows [0, min(d,TP)): sc1 loads (clamped rows), then the image of layer l+2 behind them
        const int nh = min(d, TP);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(xl, (short)0, (int)((long)(a.H + a.T) * 32 * 4), BUF_DW3);
        floatx4 hv[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int e = min(tid + NT * i, nh * 8 - 1), row = e >> 3, c4 = (e & 7) * 4;
          hv[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((a.H + t0 + row - d) * 32 + c4) * 4, 0, 16);
        }
        if (!DMAIMG) {
          const floatx4* src = (const floatx4*)(wsrc + (long)min(l + 2, a.L - 1) * IMGF);
#pragma unroll
          for (int i = 0; i < PF; ++i) pf[i] = src[min(tid + NT * i, IMGF / 4 - 1)];
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int e = tid + NT * i;
          *(floatx4*)(HALO + (e >> 3) * XS + (e & 7) * 4) = hv[i];
        }
      }
      __syncthreads();
      }
      FSTAMP(3);
      // residual weights (RT rows 16rb + i16, k group g) read now
      // (the LC form, register-tight, reads them after the dilated tap: with the halo row in
      // registers across them it spilled)
      bf16x8 rf[2][3];
      auto read_rf = [&]() {
        const unsigned short* rt = (const unsigned short*)Wl + 64 * XW_ROW + i16 * XR_ROW + 8 * g;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int p = 0; p < 3; ++p) rf[rb][p] = *(const bf16x8*)(rt + 16 * rb * XR_ROW + 32 * p);
      };
      if (!LC) read_rf();
      __builtin_amdgcn_sched_barrier(0);
      // dilated tap W0·x[t-d], gate
      if (WH) {
        const float* xp = cur + max(r - d, 0) * XS + 8 * g;
        floatx4 x0 = *(const floatx4*)xp, x1 = *(const floatx4*)(xp + 4);
        if (r < d) {
          x0 = hx[0];
          x1 = hx[1];
        }
        conv16_tap_x<LC ? 2 : 1>(x0, x1, (const unsigned short*)Wl, i16, g, acc);
        if (LC) read_rf();
        if (LCLATE && l > 0 && l + 1 < a.L) dma_lc16_image<NW>(a.lcimg, l + 1, LCI, w, lane);
      } else {
        const float* xp = (r >= d) ? cur + (r - d) * XS : HALO + r * XS;
        conv16_tap<LC ? 2 : 1>(xp, (const unsigned short*)Wl, i16, g, acc);
      }
      floatx4 z[2], sg[2];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float sq;
          z[bb][j] = gate_zs(acc[bb][j], acc[2 + bb][j], sq);
          sg[bb][j] = sq;
        }
      // z (skip GEMM input) and σ rows (sg_off blocks for chain_bwd_x3_kernel): issued last, after
      // the publish, so the drain before it does not wait for them -- except in the LC form, whose
      // 16 registers they hold through the residual and the next own tap spilled with the
      // per-wave halo
      auto store_zs = [&]() {
        if (valid) {
          float* zr = a.Z + m * a.ldz + (long)l * a.Cd;
#pragma unroll
          for (int bb = 0; bb < 2; ++bb) *(floatx4*)(zr + 8 * (q0 + bb) + 4 * h) = z[bb];
          if (a.SG) {
            float* sgl = a.SG + (long)l * a.sgls;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) *(floatx4*)(sgl + sg_off(m, q0 + bb, h)) = sg[bb];
          }
        }
      };
      if (LC) store_zs();
      FSTAMP(4);
      if (l + 1 < a.L) {
        // residual: x_{l+1} = x_l + br + RES·z → LDS (next layer's rows) and HBM (sc1 for halo rows)
        floatx4 accr[2];
        const float* xc = cur + r * XS;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          accr[rb] = *(const floatx4*)(xc + 16 * rb + 4 * g) + *(const floatx4*)(br + 16 * rb + 4 * g);
        {
          bf16x8 zb[3];
          split8(z[0], z[1], zb);   // k = 8g + j: block 0 regs, then block 1 regs (RT's k order)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) accr[rb] = mfma16x3(rf[rb], zb, accr[rb]);
        }
        float* xn = a.X + (long)(l + 1) * a.xls + sb;
        const __amdgpu_buffer_rsrc_t rn =
            __builtin_amdgcn_make_buffer_rsrc(xn, (short)0, (int)((long)(a.H + a.T) * 32 * 4), BUF_DW3);
        float* nrow = nxt + r * XS;
        const bool halo_row = r >= TP - min(1 << ((l + 1) % a.nbl), TP);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          *(floatx4*)(nrow + 16 * rb + 4 * g) = accr[rb];
          const int off = ((a.H + t) * 32 + 16 * rb + 4 * g) * 4;
          if (valid && halo_row) __builtin_amdgcn_raw_buffer_store_b128(accr[rb], rn, off, 0, 16);
          if (valid && !halo_row) __builtin_amdgcn_raw_buffer_store_b128(accr[rb], rn, off, 0, 0);
        }
        FSTAMP(8);
        // the next layer's own tap from the row this wave's lanes just wrote (wave-local)
        wave_lds_fence();
        const float* Wn = img(l + 1);
        conv16_init(bias_of(Wn), cv, q0, h, acc);
        if (has_cond && l + 2 < a.L) load_cond16<CM>(a, l + 2, myid, m, valid, q0, h, cv);
        conv16_tap<LC ? 2 : 1>(nrow, (const unsigned short*)Wn + 96, i16, g, acc);
        if (LC && !LCLATE) lc16_terms(LCIu, lcv, i16, g, acc);
      }
      FSTAMP(5);
      // publish x_{l+1}: every wave drains its stores, barrier, one lane signals
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      FSTAMP(9);
      __syncthreads();
      FSTAMP(10);
      if (tid == 0 && l + 1 < a.L) publish_flag(a.flags + tile, (unsigned)(l + 1));
      if (LC && !LCLATE && l + 2 < a.L) dma_lc16_image<NW>(a.lcimg, l + 2, LCI, w, lane);
      if (DMAIMG && l + 2 < a.L) {
        const float* src = wsrc + (long)(l + 2) * IMGF + lane * 4;
        float* dst = IMG0 + (l & 1) * IMGF;
#pragma unroll
        for (int i = 0; i < IMGF / 256 / NW; ++i) dma16(src + (w + NW * i) * 256, dst + (w + NW * i) * 256);
      }
      // (LCLATE) the LC image of layer l+1 landed by the drain before the barrier above
      if (LCLATE && l + 1 < a.L) lc16_terms(LCIu, lcv, i16, g, acc);
      if (!DMAIMG && l + 2 < a.L) {
        float* dst = IMG0 + (l & 1) * IMGF;
#pragma unroll
        for (int i = 0; i < PF; ++i) {
          const int e = tid + NT * i;
          if (e < IMGF / 4) *(floatx4*)(dst + 4 * e) = pf[i];
        }
      }
      FSTAMP(6);
      if (!LC) store_zs();
      FSTAMP(7);
    }
#undef FSTAMP
  }
}

}  // namespace

int lbwn_chain_fwd_tile(int fwd_nw) { return fwd_nw ? 16 * fwd_nw : LP; }

// the 128-position forward chain, by operand form (x3: the bf16-split images), LC / conditioning mode
static void launch_fwd(bool tr, bool x3, bool lc, int cm, int grid, const ChainFK& k, hipStream_t st) {
  void (*f)(ChainFK);
  if (lc) f = cm == 0 ? (tr ? chain_fwd_kernel<true, true, 0, true> : chain_fwd_kernel<true, true, 0, false>)
                      : (tr ? chain_fwd_kernel<true, true, 1, true> : chain_fwd_kernel<true, true, 1, false>);   // lc: cond is null
  else if (!x3) f = cm == 0 ? (tr ? chain_fwd_kernel<false, false, 0, true> : chain_fwd_kernel<false, false, 0, false>)
                            : (tr ? chain_fwd_kernel<false, false, 2, true> : chain_fwd_kernel<false, false, 2, false>);
  else if (cm == 0) f = tr ? chain_fwd_kernel<true, false, 0, true> : chain_fwd_kernel<true, false, 0, false>;
  else if (cm == 1) f = tr ? chain_fwd_kernel<true, false, 1, true> : chain_fwd_kernel<true, false, 1, false>;
  else f = tr ? chain_fwd_kernel<true, false, 2, true> : chain_fwd_kernel<true, false, 2, false>;
  hipLaunchKernelGGL(f, dim3(grid), dim3(256), 0, st, k);
}

// the 16-position-wave forward chain of NW waves (64·NW threads), by LC / conditioning mode
template <int NW>
static void launch_fwd16(bool tr, bool lc, int cm, int grid, const ChainFK& k, hipStream_t st) {
  void (*f)(ChainFK);
  if (lc) f = cm == 0 ? (tr ? chain_fwd16_kernel<NW, true, 0, true> : chain_fwd16_kernel<NW, true, 0, false>)
                      : (tr ? chain_fwd16_kernel<NW, true, 1, true> : chain_fwd16_kernel<NW, true, 1, false>);
  else if (cm == 0) f = tr ? chain_fwd16_kernel<NW, false, 0, true> : chain_fwd16_kernel<NW, false, 0, false>;
  else if (cm == 1) f = tr ? chain_fwd16_kernel<NW, false, 1, true> : chain_fwd16_kernel<NW, false, 1, false>;
  else f = tr ? chain_fwd16_kernel<NW, false, 2, true> : chain_fwd16_kernel<NW, false, 2, false>;
  hipLaunchKernelGGL(f, dim3(grid), dim3(64 * NW), 0, st, k);
}

int lbwn_chain_fwd_launch(const lbwn_chain_args& c, hipStream_t st) {
  LBWN_REQUIRE(c.Cr == 32 && c.Cd == 32, "chain fwd: n_res = n_dil = 32 only");
  LBWN_REQUIRE(c.grid >= 1 && c.flags && c.status, "chain fwd: bad launch state");
  LBWN_REQUIRE((((uintptr_t)c.X) & 15) == 0 && (c.xls & 3) == 0, "chain fwd: x not 16-B aligned");
  ChainFK k;
  k.X = c.X; k.xls = c.xls; k.Z = c.Z; k.ldz = c.ldz; k.wpack = c.wpack;
  k.gc_tab = c.gc_tab; k.gc_ld = c.gc_ld; k.ids = c.ids; k.cond = c.cond; k.ldcond = c.ldcond;
  k.flags = c.flags; k.status = c.status;
  k.B = c.B; k.T = c.T; k.H = c.H; k.L = c.L; k.nbl = c.nbl; k.Cd = c.Cd;
  k.trace = c.trace; k.trace_blk = c.trace_blk;
  k.ximg = c.wpack_x3;
  k.xcd = c.xcd;
  k.SG = c.SG; k.sgls = c.sgls;
  k.lcact = c.lcact; k.lcimg = c.lcimg; k.Lo = c.Lo;
  LBWN_REQUIRE(!c.wpack_x3 || (((uintptr_t)c.wpack_x3) & 15) == 0, "chain fwd: split images not 16-B aligned");
  const bool lc = c.lcimg != nullptr;
  if (lc)
    LBWN_REQUIRE(c.wpack_x3 && c.lcact && !c.cond && c.Lo > 16 * (LC_K - 1) && c.Lo <= LC_KP && c.Lo % 4 == 0 &&
                     (((uintptr_t)c.lcact) & 15) == 0 && (((uintptr_t)c.lcimg) & 15) == 0,
                 "chain fwd: in-chain LC needs the split images, %d < n_lc_out <= %d, aligned rows", 16 * (LC_K - 1),
                 LC_KP);
  LBWN_REQUIRE(c.fwd_nw == 0 || ((c.fwd_nw == 4 || c.fwd_nw == 8) && c.wpack_x3 && c.SG),
               "chain fwd: 16-position waves need the split images and the SG rows, 4 or 8 waves");
  const int tp = lbwn_chain_fwd_tile(c.fwd_nw);
  const int tps = (c.T + tp - 1) / tp;
  // hand-off flags only: the status word is sticky for the whole step
  if (!c.flags_zeroed) {
    if (int e = lbwn_zero_launch(c.flags, ((size_t)c.B * tps * 4 + 15) / 16 * 16, st)) return e;
  }
  const int cm = (!c.gc_tab && !c.cond) ? 0 : (c.gc_tab && !c.cond) ? 1 : 2;
  const bool tr = c.trace != nullptr;
  if (c.fwd_nw == 8) launch_fwd16<8>(tr, lc, cm, c.grid, k, st);
  else if (c.fwd_nw == 4) launch_fwd16<4>(tr, lc, cm, c.grid, k, st);
  else launch_fwd(tr, c.wpack_x3 != nullptr, lc, cm, c.grid, k, st);
  LBWN_CHECK_LAUNCH();
  return 0;
}
