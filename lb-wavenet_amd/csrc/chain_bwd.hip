// The persistent backward chain (layers L-1 .. 0 in one launch) in its three forms: chain_bwd_kernel
// (f32), chain_bwd_x3_kernel (bf16-split, 32-position waves) and chain_bwd16_kernel<4 | 8>
// (bf16-split, 16-position waves), with their launcher.
#include "common.h"
#include "kernels.h"
#include "layer_common.h"

namespace {

// ---- persistent backward chain -------------------------------------------------------------
// Layers L-1 .. 0 in one launch; tiles in DECREASING order (layer l's tile needs dx_{l+1} at
// rows t + d_{l+1}, i.e. from the same or LATER tiles).  dx_{l+1}[t] = out_a[t] + out_c0[t+d']
// (tmodel.py:122-127 autodiff): out_a never leaves the block (registers, acc layout = the B
// operand of the next dz product); out_c0 stays in LDS for the block's own rows and only its
// first min(d,128) rows are published (sc1) to the per-layer hand-off buffer for the tile
// below.  The gate recompute runs before the hand-off wait and the weight-gradient products
// after the publish, so the cross-tile critical path per layer is G-build → dz → dx.
// Weight-gradient partials go to slab[l][tile] (summed by layer_reduce_all_kernel).

// Xp Xc | IMG | DV | G | OC | XpN XcN (the next layer's rows, DMA-staged, unpadded): 163,712 B
constexpr int CB_LDS = 2 * LP * XS + WIMG + LP * DS + 2 * LP * XS + 2 * LP * 32;
static_assert(CB_LDS * 4 + 16 <= 160 * 1024, "chain bwd LDS");
static_assert(4096 + 768 <= 2 * LP * XS, "RED + bias partials must fit in Xp and Xc");
constexpr int IMG_PF = (WIMG / 4 + 255) / 256;      // float4 per thread to prefetch an image

// next-layer rows by LDS-DMA: wave w moves rows [32w, 32w+32) of the dilated-tap and own-row
// blocks, 8 rows (1 KiB) per global_load_lds_dwordx4; rows past T are clamped here and zeroed
// by the copy
LBWN_DEV void dma_rows(float* XpN, float* XcN, const float* xl, int t0, int d, int T, int H, int w, int lane,
                       int j0, int j1) {
#pragma unroll
  for (int j = j0; j < j1; ++j) {
    const int row = 32 * w + 8 * j + (lane >> 3), c4 = (lane & 7) * 4;
    const int trow = min(t0 + row, T - 1);
    __builtin_amdgcn_global_load_lds(xl + (long)(H + trow - d) * 32 + c4,
                                     (__attribute__((address_space(3))) void*)(XpN + (32 * w + 8 * j) * 32), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(xl + (long)(H + trow) * 32 + c4,
                                     (__attribute__((address_space(3))) void*)(XcN + (32 * w + 8 * j) * 32), 16, 0, 0);
  }
}
// unpadded staged rows -> padded tile rows (zero past T)
LBWN_DEV void copy_rows(float* dst, const float* src, int t0, int T, int tid) {
  floatx4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i;
    v[i] = *(const floatx4*)(src + (e >> 3) * 32 + (e & 7) * 4);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i;
    if (t0 + (e >> 3) >= T) v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    *(floatx4*)(dst + (e >> 3) * XS + (e & 7) * 4) = v[i];
  }
}

__global__ __launch_bounds__(256) void chain_bwd_kernel(ChainBK a) {
  __shared__ __attribute__((aligned(16))) float sm[CB_LDS];
  __shared__ int s_fail;
  float* Xp = sm;
  float* Xc = Xp + LP * XS;
  float* Ws = Xc + LP * XS;
  float* Rs = Ws + 64 * WS;
  float* bs = Rs + 32 * XS;
  float* DV = Ws + WIMG;
  float* G = DV + LP * DS;
  float* OC = G + LP * XS;
  float* XpN = OC + LP * XS;    // next layer's rows, DMA-staged during this layer
  float* XcN = XpN + LP * 32;
  float* ZT = Ws;   // after dx
  float* RED = Xp;  // after dSIG
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pi = lane & 31, h = lane >> 5;
  const int r = 32 * w + pi;
  const int tps = (a.T + LP - 1) / LP, ntiles = a.B * tps;
  const int oc_bytes = (int)std::min<long>(a.ocls * 4, 0x7fffffffL);
  if (tid == 0) s_fail = 0;
  const int first = chain_first(a.xcd);
  for (int it = first; it < ntiles; it += gridDim.x) {
    const int tile = ntiles - 1 - it;
    const int b = tile / tps, tt = tile % tps, t0 = tt * LP;
    const int t = t0 + r;
    const bool valid = t < a.T;
    const long mb = (long)b * a.T, m = mb + t;
    const long sb = (long)b * (a.H + a.T) * 32;
    const bool has_cond = a.gc_tab || a.cond;
    const int myid = (a.gc_tab && valid) ? a.ids[m] : 0;
    floatx4 cv[8];
    load_cond<2>(a, a.L - 1, myid, m, valid && has_cond, h, cv);
    // GC grads: is this wave's 32-position run one voice id?  (fast scatter path)
    const int wave_id = __shfl(myid, 0);
    const bool wave_uni = __all(!valid || myid == wave_id);
    __syncthreads();
    stage_image(Ws, a.wpack + (long)(a.L - 1) * WIMG, tid);
    floatx16 oa;  // out_a of layer l+1, own row
#pragma unroll
    for (int q = 0; q < 16; ++q) oa[q] = 0.f;
    const bool trc = a.trace && (int)blockIdx.x == a.trace_blk && tid == 0 && it == first;
#define CSTAMP(i) if (trc) a.trace[16 * l + (i)] = clock64()
    for (int l = a.L - 1; l >= 0; --l) {
      CSTAMP(0);
      const int d = 1 << (l % a.nbl);
      const int dn = (l + 1 < a.L) ? 1 << ((l + 1) % a.nbl) : 0;
      const float* xl = a.X + (long)l * a.xls + sb;
      // 0. this layer's inputs: x_l taps / own rows (the tile's first layer: from HBM; later
      //    layers: DMA-staged during the previous layer, landed by its publish drain + barrier),
      //    dZ rows (first used after the gate recompute and G build); next image prefetch
      if (l == a.L - 1) {
        stage_rows(Xp, xl, t0, -d, a.T, a.H, 32, tid);
        stage_rows(Xc, xl, t0, 0, a.T, a.H, 32, tid);
      } else {
        copy_rows(Xp, XpN, t0, a.T, tid);
        copy_rows(Xc, XcN, t0, a.T, tid);
      }
      floatx16 dz;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        floatx4 v = *(const floatx4*)(a.DZ + (mb + min(t, a.T - 1)) * a.lddz + (long)l * a.Cd + 8 * q + 4 * h);
        if (!valid) v = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[4 * q + j] = v[j];
      }
      floatx4 pf[IMG_PF];
      if (l > 0) {
        const floatx4* src = (const floatx4*)(a.wpack + (long)(l - 1) * WIMG);
#pragma unroll
        for (int i = 0; i < IMG_PF; ++i) {
          const int e = tid + 256 * i;
          pf[i] = src[min(e, WIMG / 4 - 1)];   // clamped: no load behind a branch
        }
      }
      __syncthreads();
      CSTAMP(1);
      // the next layer's rows into XpN / XcN (everyone has copied them out: the barrier above),
      // half before each conv half so the DMA issue overlaps in-flight MFMAs
      const float* xnext = a.X + (long)(l > 0 ? l - 1 : 0) * a.xls + sb;
      const int dnext = 1 << ((l > 0 ? l - 1 : 0) % a.nbl);
      if (l > 0) dma_rows(XpN, XcN, xnext, t0, dnext, a.T, a.H, w, lane, 0, 2);
      // 1. recompute the gate (no cross-tile dependency)
      floatx16 acc_s, acc_g;
      conv_init(bs, cv, h, acc_s, acc_g);
      if (has_cond && l > 0) load_cond<2>(a, l - 1, myid, m, valid, h, cv);
      conv_half(Xc + r * XS, Ws + 32 * WS, pi, h, acc_s, acc_g);
      if (l > 0) dma_rows(XpN, XcN, xnext, t0, dnext, a.T, a.H, w, lane, 2, 4);
      conv_half(Xp + r * XS, Ws, pi, h, acc_s, acc_g);
      floatx16 th, sg;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        th[q] = tanhf_(acc_s[q]);
        sg[q] = sigmoidf_(acc_g[q]);
      }
      CSTAMP(2);
      // 2. G = dx_{l+1} rows of this tile: out_c0_{l+1}[t + dn] (own LDS / published rows) + out_a
      if (dn) {
        const int ptt = tt + max(1, dn / LP);
        if (ptt < tps) {
          if (tid == 0 && !s_fail) {
            if (!wait_flag_ge(a.flags + (long)b * tps + ptt, (unsigned)(a.L - l - 1), a.status, 2u)) s_fail = 1;
          }
          __syncthreads();
        }
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)(l + 1) * a.ocls, (short)0, oc_bytes, BUF_DW3);
        // rows from the own tile's OC (LDS) or the producer's published rows (sc1 loads): all
        // loads issued unconditionally at clamped indices, then selected (no load behind a branch)
        floatx4 gl[4], go[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, row = e >> 3, c4 = (e & 7) * 4, sr = row + dn;
          const int ts = min(t0 + sr, a.T - 1);
          gl[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(((mb + ts) * 32 + c4) * 4), 0, 16);
          go[i] = *(const floatx4*)(OC + min(sr, LP - 1) * XS + c4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, row = e >> 3, c4 = (e & 7) * 4, sr = row + dn, ts = t0 + sr;
          floatx4 v = sr < LP ? go[i] : gl[i];
          if (ts >= a.T) v = floatx4{0.f, 0.f, 0.f, 0.f};
          *(floatx4*)(G + row * XS + c4) = v;
        }
        __syncthreads();
      }
      CSTAMP(3);
      floatx16 gv;
      {  // own row: + out_a (at the top layer g = 0: the row is written here, not read)
        float* grow = G + r * XS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          floatx4 v = dn ? *(const floatx4*)(grow + 8 * q + 4 * h) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) { v[j] += oa[4 * q + j]; gv[4 * q + j] = v[j]; }
          *(floatx4*)(grow + 8 * q + 4 * h) = v;
        }
      }
      // 3. dz += RES·g; dv
      {
        floatx4 rx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rx[q] = *(const floatx4*)(Rs + pi * XS + 8 * q + 4 * h);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) dz = mfma32(rx[q][j], gv[4 * q + j], dz);
      }
      floatx16 dvs, dvg;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        dvs[q] = dz[q] * sg[q] * (1.f - th[q] * th[q]);
        dvg[q] = dz[q] * th[q] * sg[q] * (1.f - sg[q]);
      }
      {
        float* dvrow = DV + r * DS;
        float* dvo = (a.dv_out && valid) ? a.dv_out + m * a.lddv + (long)l * 64 : nullptr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 vs = floatx4{dvs[4 * q], dvs[4 * q + 1], dvs[4 * q + 2], dvs[4 * q + 3]};
          const floatx4 vg = floatx4{dvg[4 * q], dvg[4 * q + 1], dvg[4 * q + 2], dvg[4 * q + 3]};
          *(floatx4*)(dvrow + 8 * q + 4 * h) = vs;
          *(floatx4*)(dvrow + 32 + 8 * q + 4 * h) = vg;
          if (dvo) {
            *(floatx4*)(dvo + 8 * q + 4 * h) = vs;
            *(floatx4*)(dvo + 32 + 8 * q + 4 * h) = vg;
          }
        }
      }
      CSTAMP(4);
      // 4. dx: out_a = g + W1·dv, out_c0 = W0·dv
      floatx16 acc_a = gv, acc_c;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc_c[q] = 0.f;
      {
        floatx4 wv[2][4];
        auto loadw = [&](int q, int buf) {
          const int ko = 8 * q + 4 * h;
          wv[buf][0] = *(const floatx4*)(Ws + pi * WS + ko);
          wv[buf][1] = *(const floatx4*)(Ws + pi * WS + 32 + ko);
          wv[buf][2] = *(const floatx4*)(Ws + (32 + pi) * WS + ko);
          wv[buf][3] = *(const floatx4*)(Ws + (32 + pi) * WS + 32 + ko);
        };
        loadw(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cb = q & 1;
          if (q + 1 < 4) loadw(q + 1, cb ^ 1);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int s2 = 4 * q + j;
            acc_a = mfma32(wv[cb][2][j], dvs[s2], acc_a);
            acc_c = mfma32(wv[cb][0][j], dvs[s2], acc_c);
            acc_a = mfma32(wv[cb][3][j], dvg[s2], acc_a);
            acc_c = mfma32(wv[cb][1][j], dvg[s2], acc_c);
          }
        }
      }
      {
        float* ocrow = OC + r * XS;
        const __amdgpu_buffer_rsrc_t rw =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)l * a.ocls, (short)0, oc_bytes, BUF_DW3);
        const bool pub = l > 0 && valid && r < min(d, LP);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 v = floatx4{acc_c[4 * q], acc_c[4 * q + 1], acc_c[4 * q + 2], acc_c[4 * q + 3]};
          *(floatx4*)(ocrow + 8 * q + 4 * h) = v;
          if (pub) __builtin_amdgcn_raw_buffer_store_b128(v, rw, (int)((m * 32 + 8 * q + 4 * h) * 4), 0, 16);
        }
      }
      if (l == 0 && valid) {
        store_rows16(a.dx0_a + m * 32, acc_a, 32, h);
        store_rows16(a.dx0_c + m * 32, acc_c, 32, h);
      }
      oa = acc_a;
      CSTAMP(5);
      // publish out_c0_l (every wave drains its sc1 stores, barrier, one lane signals)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // also: DV complete, the weight image is dead
      if (tid == 0 && l > 0) publish_flag(a.flags + tile, (unsigned)(a.L - l));
      if (a.gc_dtab) gc_scatter(a.gc_dtab + (long)l * 64, a.gc_ld, a.ids + mb, DV, t0, a.T, w, lane, 32,
                                wave_uni ? wave_id : -1);
      CSTAMP(6);
      // 5. weight gradients of layer l over this tile
      {
        float* zrow = ZT + r * XS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          floatx4 zv;
#pragma unroll
          for (int j = 0; j < 4; ++j) zv[j] = th[4 * q + j] * sg[4 * q + j];
          *(floatx4*)(zrow + 8 * q + 4 * h) = zv;
        }
      }
      floatx16 accW, accR;
#pragma unroll
      for (int q = 0; q < 16; ++q) { accW[q] = 0.f; accR[q] = 0.f; }
      {  // dSIG/dGATE tile w: A[i=in][k=pos] = X[pos][in], B[k][j=o] = DV[pos][o]
        // Operands for 16 MFMAs are read one chunk ahead; the sched_barriers keep hipcc from
        // sinking each read next to its MFMA (at this kernel's register pressure it otherwise
        // does, and every MFMA waits out an LDS round trip: ~3.5x the MFMA time)
        const float* X = (w & 1) ? Xc : Xp;
        const int oc = (w >> 1) * 32 + pi;
        float xa[2][16], da[2][16];
        auto loadc = [&](int c, int buf) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int p = 2 * (16 * c + i) + h;
            xa[buf][i] = X[p * XS + pi];
            da[buf][i] = DV[p * DS + oc];
          }
        };
        loadc(0, 0);
#pragma unroll
        for (int c = 0; c < LP / 32; ++c) {
          const int cb = c & 1;
          if (c + 1 < LP / 32) loadc(c + 1, cb ^ 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 16; ++i) accW = mfma32(xa[cb][i], da[cb][i], accW);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      CSTAMP(7);
      __syncthreads();  // ZT visible; Xp/Xc free for RED
      {  // dRES part over this wave's 32 positions (all operands read before the first MFMA)
        float za[16], ga[16];
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          const int p = 32 * w + 2 * s2 + h;
          za[s2] = ZT[p * XS + pi];
          ga[s2] = G[p * XS + pi];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) accR = mfma32(za[s2], ga[s2], accR);
      }
      CSTAMP(8);
      float* slab = a.slab + ((long)l * ntiles + tile) * SLAB;
      {  // bias partials: column sums of DV (64) and G (32)
        float* part = RED + 4096;  // [8][96] after the dRES exchange area
        if (tid < 128) {
          const int c4 = (tid & 15) * 4, pc = tid >> 4;
          floatx4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < 16; ++p) s4 += *(const floatx4*)(DV + (pc * 16 + p) * DS + c4);
          *(floatx4*)(part + pc * 96 + c4) = s4;
        } else if (tid < 192) {
          const int c4 = ((tid - 128) & 7) * 4, pc = (tid - 128) >> 3;
          floatx4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < 16; ++p) s4 += *(const floatx4*)(G + (pc * 16 + p) * XS + c4);
          *(floatx4*)(part + pc * 96 + 64 + c4) = s4;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          slab[w * 1024 + acc_row(q, h) * 32 + pi] = accW[q];
          RED[w * 1024 + acc_row(q, h) * 32 + pi] = accR[q];
        }
        __syncthreads();
        if (tid < 96) {
          float s1 = 0.f;
#pragma unroll
          for (int pc = 0; pc < 8; ++pc) s1 += part[pc * 96 + tid];
          slab[5120 + tid] = s1;
        }
        for (int e = tid; e < 1024; e += 256)
          slab[4096 + e] = ((RED[e] + RED[1024 + e]) + RED[2048 + e]) + RED[3072 + e];
      }
      CSTAMP(9);
      // 6. next layer's weight image (ZT is dead: every wave passed the barrier after dRES)
      if (l > 0) {
#pragma unroll
        for (int i = 0; i < IMG_PF; ++i) {
          const int e = tid + 256 * i;
          if (e < WIMG / 4) *(floatx4*)(Ws + 4 * e) = pf[i];
        }
      }
      __syncthreads();
      CSTAMP(10);
    }
#undef CSTAMP
  }
}

// ---- backward chain on the bf16 cores (the X3 arithmetic of DESIGN §4.0) -----------------------
// Same tile walk, hand-off and slab layout as chain_bwd_kernel; what changes:
//  * no gate recompute: the X3 forward chain stores σ(v_gate) (SG [L][M][32]) beside z (Zcat),
//    so tanh = z·σ⁻¹ and dv come from two row loads (prefetched a layer ahead) instead of a
//    second 64-channel conv;
//  * dx = W·dv (K = 64) and the weight gradients dSIG/dGATE = Xᵀ·DV (K = 128 positions) and
//    dRES = Zᵀ·G run on v_mfma_f32_32x32x16_bf16 / 16x16x32 from exact 3-term splits (six
//    products); dz = dZ + RES·g (16 f32 MFMAs) stays on v_mfma_f32_32x32x2_f32;
//  * this layer's x rows (both taps) and z rows are LDS-DMA'd into unpadded tiles during the
//    G build, the next layer's weight image right after the publish; DV, G and OC live in
//    32-float rows with an XOR swizzle of the 4-float groups (swz) so that both the own-row
//    b128 writes and the column reads of the weight-gradient products are conflict-free.

constexpr int CBX_LDS = BX_F + 7 * LP * 32 + 8 * 96;              // IMG | Xp Xc ZT | DVs DVg G OC | part
static_assert(CBX_LDS * 4 + 16 <= 160 * 1024, "chain bwd x3 LDS");

// element (p, c) of a 32-float-row tile with the 4-float groups XOR-permuted: bit 4 of the column
// by row parity, bits 2-3 by (p >> 1) & 3.  Eight consecutive rows (the 8 lanes of one
// ds_write_b128 group writing the same column group of their own rows) land on 8 distinct groups:
// conflict-free; rows p, p+1 read by the two lane halves of a b32 read fall in opposite 16-bank
// halves (a row-pair permutation left those writes 2-way conflicted: 6.6M of the kernel's 15.6M
// SQ_LDS_BANK_CONFLICT cycles, tools/lds_conf.sh)
LBWN_DEV int swz(int p, int c) { return p * 32 + (c ^ (((p & 1) << 4) | (((p >> 1) & 3) << 2))); }

// GC rows of a wave whose 32 positions are not one voice: dv column sums per run of equal ids
// (ids change only at file boundaries), one atomic per run and column.  The runs come from the
// lanes' own ids (lane p of either half holds position 32w + p; -1 past the end): run starts =
// ballot of id changes, computed once per tile by the caller (`starts`, bit p = a run starts at
// position p; `pid` = the lane's id).  No global loads: the old per-position loop loaded each id
// inside the loop and waited on every one (arch5 backward chain 550 -> 900 us on such batches).
LBWN_DEV void gc_scatter_x3(float* gtab, long ld, const float* DVs, const float* DVg, int w, int lane, int Cd,
                            unsigned starts, int pid) {
  const int o = lane, oc = o & 31;
  const float* pl = o < 32 ? DVs : DVg;
  const int col = o < 32 ? oc : Cd + oc;
  unsigned rest = starts;
  while (rest) {   // wave-uniform
    const int p0 = __ffs(rest) - 1;
    rest &= rest - 1;
    const int p1 = rest ? __ffs(rest) - 1 : 32;
    const int id = __shfl(pid, p0);
    if (id < 0) continue;   // positions past T
    float s = 0.f;
    for (int p = p0; p < p1; ++p) s += pl[swz(32 * w + p, oc)];
    if (oc < Cd) atomicAdd(gtab + (long)id * ld + col, s);
  }
}

template <bool TR>
__global__ __launch_bounds__(256) void chain_bwd_x3_kernel(ChainBK a) {
  __shared__ __attribute__((aligned(16))) float sm[CBX_LDS];
  __shared__ int s_fail;
  float* IMG = sm;
  const unsigned short* WD = (const unsigned short*)IMG;
  const float* Rs = IMG + BD_US / 2;
  float* Xp = IMG + BX_F;
  float* Xc = Xp + LP * 32;
  float* ZT = Xc + LP * 32;
  float* DVs = ZT + LP * 32;
  float* DVg = DVs + LP * 32;
  float* G = DVg + LP * 32;
  float* OC = G + LP * 32;
  float* part = OC + LP * 32;   // [8][96] bias partials
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pi = lane & 31, h = lane >> 5;
  const int r = 32 * w + pi;
  const int tps = (a.T + LP - 1) / LP, ntiles = a.B * tps;
  const int oc_bytes = (int)std::min<long>(a.ocls * 4, 0x7fffffffL);
  if (tid == 0) s_fail = 0;
  const int first = chain_first(a.xcd);
  for (int it = first; it < ntiles; it += gridDim.x) {
    const int tile = ntiles - 1 - it;
    const int b = tile / tps, tt = tile % tps, t0 = tt * LP;
    const int t = t0 + r;
    const bool valid = t < a.T;
    const long mb = (long)b * a.T, m = mb + t, mc = mb + min(t, a.T - 1);
    const long sb = (long)b * (a.H + a.T) * 32;
    const int myid = (a.gc_tab && valid) ? a.ids[m] : 0;
    const int wave_id = __shfl(myid, 0);
    const bool wave_uni = __all(!valid || myid == wave_id);
    // GC grads: a tile whose valid positions share one voice id (the common case: ids change only
    // at file boundaries) contributes its dv column sums -- the bias partials in its slab, computed
    // anyway -- to that id's row; lbwn_gc_tile_sum_launch adds them after the chain in tile order
    // (tile_gid[tile] = the id, or -1: this chain scatters the tile's rows itself).  64 atomics
    // per tile and layer onto the few voice rows serialised at L2 and stretched the publish drains.
    const int tile_id = a.gc_tab ? a.ids[mb + t0] : 0;
    const bool tile_uni = __syncthreads_and(!valid || myid == tile_id);
    if (a.tile_gid && tid == 0) a.tile_gid[tile] = tile_uni ? tile_id : -1;
    // this wave's id runs (gc_scatter_x3): lane pi's position id, -1 past T; bit p = a run starts at p
    const int gc_pid = valid ? myid : -1;
    const int gc_prev = __shfl(gc_pid, max(pi - 1, 0));
    const unsigned gc_starts = (unsigned)(__ballot(h == 0 && (pi == 0 || gc_pid != gc_prev)) & 0xffffffffull);
    // per-layer rows of this lane's position: dZ, z, σ (issued a layer ahead)
    floatx4 dzr[4], zr[4], sgr[4];
    auto load_regs = [&](int l) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        dzr[q] = *(const floatx4*)(a.DZ + l * a.dzls + sg_off(mc, q, h));   // chain order: 1-KiB runs
        zr[q] = *(const floatx4*)(a.Zf + mc * a.lddz + (long)l * 32 + 8 * q + 4 * h);
        sgr[q] = *(const floatx4*)(a.SG + (long)l * a.sgls + sg_off(mc, q, h));
      }
    };
    auto dma_image = [&](int l) {
      const float* src = a.bimg + (long)l * BIMG_F + lane * 4;
      for (int i = w; i < BX_F / 256; i += 4) dma16(src + i * 256, IMG + i * 256);
    };
    __syncthreads();  // previous tile's LDS use done
    dma_image(a.L - 1);
    load_regs(a.L - 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    floatx16 oa;  // out_a of layer l+1, own row
#pragma unroll
    for (int q = 0; q < 16; ++q) oa[q] = 0.f;
    const bool trc = a.trace && (int)blockIdx.x == a.trace_blk && tid == 0 && it == first;
#define XSTAMP(i) if (TR && trc) a.trace[16 * l + (i)] = clock64()
    for (int l = a.L - 1; l >= 0; --l) {
      XSTAMP(0);
      const int d = 1 << (l % a.nbl);
      const int dn = (l + 1 < a.L) ? 1 << ((l + 1) % a.nbl) : 0;
      // 1. G = dx_{l+1} rows: out_c0_{l+1}[t + dn] (own OC / the producer's published rows) + out_a
      floatx4 gl[4], go[4];
      if (dn) {
        const int ptt = tt + max(1, dn / LP);
        if (ptt < tps) {
          if (tid == 0 && !s_fail) {
            if (!wait_flag_ge(a.flags + (long)b * tps + ptt, (unsigned)(a.L - l - 1), a.status, 2u)) s_fail = 1;
          }
          __syncthreads();
        }
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)(l + 1) * a.ocls, (short)0, oc_bytes, BUF_DW3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, row = e >> 3, c4 = (e & 7) * 4, sr = row + dn;
          const int ts = min(t0 + sr, a.T - 1);
          gl[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(((mb + ts) * 32 + c4) * 4), 0, 16);
          go[i] = *(const floatx4*)(OC + swz(min(sr, LP - 1), c4));
        }
      }
      if (dn) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, row = e >> 3, c4 = (e & 7) * 4, sr = row + dn, ts = t0 + sr;
          floatx4 v = sr < LP ? go[i] : gl[i];
          if (ts >= a.T) v = floatx4{0.f, 0.f, 0.f, 0.f};
          *(floatx4*)(G + swz(row, c4)) = v;
        }
        // lands this wave's part of the weight image (LDS-DMA'd after the last layer's publish)
        // and the prefetched rows; the barrier then covers every wave's part
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      // the prefetched rows are consumed here, in the compiler's view, so that it has no load of
      // its own outstanding behind the DMA pieces below (its waits would count them)
#pragma unroll
      for (int q = 0; q < 4; ++q) asm volatile("" ::"v"(dzr[q]), "v"(zr[q]), "v"(sgr[q]));
      // this layer's x rows (x[t-d] | x[t]) and z rows by LDS-DMA into Xp / Xc / ZT (free since the
      // last layer's end barrier; first read after this layer's publish drain + barrier); the
      // pieces are issued between the dz MFMAs (row group j: 3 pieces)
      const float* xl = a.X + (long)l * a.xls + sb;
      auto dma_rows3 = [&](int j) {
        const int row = 32 * w + 8 * j + (lane >> 3), c4 = (lane & 7) * 4;
        const int trow = min(t0 + row, a.T - 1);
        dma16(xl + (long)(a.H + trow - d) * 32 + c4, Xp + (32 * w + 8 * j) * 32);
        dma16(xl + (long)(a.H + trow) * 32 + c4, Xc + (32 * w + 8 * j) * 32);
        dma16(a.Zf + (mb + trow) * a.lddz + (long)l * 32 + c4, ZT + (32 * w + 8 * j) * 32);
      };
      XSTAMP(1);
      floatx16 gv;
#pragma unroll
      for (int q = 0; q < 4; ++q) {   // own row: + out_a (the top layer writes it, g = 0)
        float* gp = G + swz(r, 8 * q + 4 * h);
        floatx4 v = dn ? *(const floatx4*)gp : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += oa[4 * q + j]; gv[4 * q + j] = v[j]; }
        *(floatx4*)gp = v;
      }
      // 2. dz = dZ + RES·g  (f32 MFMA)
      floatx16 dz;
      {
        floatx4 rx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rx[q] = *(const floatx4*)(Rs + (pi * XS + 8 * q + 4 * h));
          floatx4 v = dzr[q];
          if (!valid) v = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) dz[4 * q + j] = v[j];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) dz = mfma32(rx[q][j], gv[4 * q + j], dz);
          dma_rows3(q);
        }
      }
      // 3. dv from z and σ: tanh = z/σ (σ = 0 only where dv is 0 anyway)
      floatx16 dvs, dvg;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float zz = zr[q >> 2][q & 3], sg = sgr[q >> 2][q & 3];
        const float th = sg > 1e-30f ? zz * __builtin_amdgcn_rcpf(sg) : 0.f;
        dvs[q] = dz[q] * sg * (1.f - th * th);
        dvg[q] = dz[q] * zz * (1.f - sg);
      }
      {
        // DV export: rows (layer l at columns l·64) or k-blocked (a.dvks: [L·2][Mp][32] chunks)
        float* dvo = (a.dv_out && valid)
                         ? a.dv_out + (a.dvks ? 2L * l * a.dvks + m * 32 : m * a.lddv + (long)l * 64) : nullptr;
        const long dgo = a.dvks ? a.dvks : 32;   // gate half
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 vs = floatx4{dvs[4 * q], dvs[4 * q + 1], dvs[4 * q + 2], dvs[4 * q + 3]};
          const floatx4 vg = floatx4{dvg[4 * q], dvg[4 * q + 1], dvg[4 * q + 2], dvg[4 * q + 3]};
          *(floatx4*)(DVs + swz(r, 8 * q + 4 * h)) = vs;
          *(floatx4*)(DVg + swz(r, 8 * q + 4 * h)) = vg;
          if (dvo) {
            *(floatx4*)(dvo + 8 * q + 4 * h) = vs;
            *(floatx4*)(dvo + dgo + 8 * q + 4 * h) = vg;
          }
        }
      }
      XSTAMP(2);
      // 4. dx on the bf16 cores: out_a = g + W1·dv, out_c0 = W0·dv  (k-steps 0,1: sig; 2,3: gate)
      floatx16 acc_a = gv, acc_c;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc_c[q] = 0.f;
      {
        // fragments of k-step s+1 read while step s's MFMAs issue
        bf16x8 fa[2][3], fc[2][3];
        auto loadf = [&](int s2, int buf) {
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            fa[buf][p] = *(const bf16x8*)(WD + ((32 + pi) * XW_ROW + 64 * p + 16 * s2 + 8 * h));
            fc[buf][p] = *(const bf16x8*)(WD + (pi * XW_ROW + 64 * p + 16 * s2 + 8 * h));
          }
        };
        loadf(0, 0);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
          const int o8 = 8 * (s2 & 1), cb = s2 & 1;
          if (s2 + 1 < 4) loadf(s2 + 1, cb ^ 1);
          bf16x8 bx[3];
          if (s2 < 2)
            split8(floatx4{dvs[o8], dvs[o8 + 1], dvs[o8 + 2], dvs[o8 + 3]},
                   floatx4{dvs[o8 + 4], dvs[o8 + 5], dvs[o8 + 6], dvs[o8 + 7]}, bx);
          else
            split8(floatx4{dvg[o8], dvg[o8 + 1], dvg[o8 + 2], dvg[o8 + 3]},
                   floatx4{dvg[o8 + 4], dvg[o8 + 5], dvg[o8 + 6], dvg[o8 + 7]}, bx);
          acc_a = mfma_x3(fa[cb], bx, acc_a);
          acc_c = mfma_x3(fc[cb], bx, acc_c);
        }
      }
      {
        const __amdgpu_buffer_rsrc_t rw =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)l * a.ocls, (short)0, oc_bytes, BUF_DW3);
        const bool pub = l > 0 && valid && r < min(d, LP);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 v = floatx4{acc_c[4 * q], acc_c[4 * q + 1], acc_c[4 * q + 2], acc_c[4 * q + 3]};
          *(floatx4*)(OC + swz(r, 8 * q + 4 * h)) = v;
          if (pub) __builtin_amdgcn_raw_buffer_store_b128(v, rw, (int)((m * 32 + 8 * q + 4 * h) * 4), 0, 16);
        }
      }
      if (l == 0 && valid) {
        store_rows16(a.dx0_a + m * 32, acc_a, 32, h);
        store_rows16(a.dx0_c + m * 32, acc_c, 32, h);
      }
      oa = acc_a;
      XSTAMP(3);
      // 5. publish out_c0_l (the drain also lands this layer's x / z DMA pieces)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // DV, G, Xp/Xc/ZT complete; the weight image is dead
      if (tid == 0 && l > 0) publish_flag(a.flags + tile, (unsigned)(a.L - l));
      // the next layer's weight image and rows are issued between the dSIG MFMAs below (landed
      // by the next layer's G build: vmcnt(0) + barrier)
      if (a.gc_dtab && !tile_uni) gc_scatter_x3(a.gc_dtab + (long)l * 64, a.gc_ld, DVs, DVg, w, lane, 32, gc_starts, gc_pid);
      XSTAMP(4);
      // 6. dSIG / dGATE partials of ALL four tiles t (0 sig·prev, 1 sig·cur, 2 gate·prev, 3
      //    gate·cur) over this wave's own 32 positions: A[i=in][k=pos] = X[pos][in], B[k][j=o] =
      //    DV[pos][o], k-step s: p = 32w + 16s + 2j + h (the lane halves read rows of opposite
      //    parity).  Every X and DV value is split once per layer (one tile per wave over all 128
      //    positions split each twice); the four waves' partials are summed through LDS at the end.
      floatx16 accT[4];
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
        for (int q = 0; q < 16; ++q) accT[t4][q] = 0.f;
      {
        const float* isrc = a.bimg + (long)(l > 0 ? l - 1 : 0) * BIMG_F + lane * 4;
        // both k-steps' operands are read before the DMA issue (its asm is a compiler barrier for
        // LDS reads), so that their latency is exposed once
        float xp[2][8], xc[2][8], ds[2][8], dg[2][8];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int p = 32 * w + 16 * s2 + 2 * j + h;
            xp[s2][j] = Xp[p * 32 + pi];
            xc[s2][j] = Xc[p * 32 + pi];
            ds[s2][j] = DVs[swz(p, pi)];
            dg[s2][j] = DVg[swz(p, pi)];
          }
        XSTAMP(8);
        if (l > 0) {   // image pieces w, w+4, ... (30 of 1 KiB)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int pc = w + 4 * i;
            if (pc < BX_F / 256) dma16(isrc + pc * 256, IMG + pc * 256);
          }
          load_regs(l - 1);
        }
        XSTAMP(9);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          bf16x8 fxp[3], fxc[3], fds[3], fdg[3];
          split8(floatx4{xp[s2][0], xp[s2][1], xp[s2][2], xp[s2][3]}, floatx4{xp[s2][4], xp[s2][5], xp[s2][6], xp[s2][7]}, fxp);
          split8(floatx4{ds[s2][0], ds[s2][1], ds[s2][2], ds[s2][3]}, floatx4{ds[s2][4], ds[s2][5], ds[s2][6], ds[s2][7]}, fds);
          accT[0] = mfma_x3(fxp, fds, accT[0]);
          split8(floatx4{xc[s2][0], xc[s2][1], xc[s2][2], xc[s2][3]}, floatx4{xc[s2][4], xc[s2][5], xc[s2][6], xc[s2][7]}, fxc);
          accT[1] = mfma_x3(fxc, fds, accT[1]);
          split8(floatx4{dg[s2][0], dg[s2][1], dg[s2][2], dg[s2][3]}, floatx4{dg[s2][4], dg[s2][5], dg[s2][6], dg[s2][7]}, fdg);
          accT[2] = mfma_x3(fxp, fdg, accT[2]);
          accT[3] = mfma_x3(fxc, fdg, accT[3]);
          if (s2 == 0) XSTAMP(10);
        }
      }
      XSTAMP(5);
      // 7. dRES quarter of wave w (16x16: z channels 16(w>>1).., res out 16(w&1)..) over all LP
      //    positions on v_mfma_f32_16x16x4_f32 (K = 2048 flop/pos is too little to pay for
      //    splitting): A[i=c][k=pos] = z[pos][c], B[k][j=o] = g[pos][o]; k = lane>>4
      floatx4 accR = {0.f, 0.f, 0.f, 0.f};
      {
        const int i16 = lane & 15, kg = lane >> 4, cz = 16 * (w >> 1) + i16, og = 16 * (w & 1) + i16;
#pragma unroll
        for (int c8 = 0; c8 < LP / 32; ++c8) {
          float za[8], ga[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int p = 32 * c8 + 4 * j + kg;
            za[j] = ZT[p * 32 + cz];
            ga[j] = G[swz(p, og)];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 8; ++j) accR = __builtin_amdgcn_mfma_f32_16x16x4f32(za[j], ga[j], accR, 0, 0, 0);
        }
      }
      XSTAMP(11);
      // 8. bias partials (column sums of DV and G) and the slab
      float* slab = a.slab + ((long)l * ntiles + tile) * SLAB;
      //    (wave 0: DVs, 1: DVg, 2: G; lane = (row class pc, 4-column group c4), rows pc + 8p:
      //    each 16-lane b128 read group then covers both bank halves, conflict-free under swz)
      if (tid < 192) {
        const int c4 = (lane & 7) * 4, pc = lane >> 3;
        const float* pl = w == 0 ? DVs : w == 1 ? DVg : G;
        floatx4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 16; ++p) s4 += *(const floatx4*)(pl + swz(pc + 8 * p, c4));
        *(floatx4*)(part + pc * 96 + 32 * w + c4) = s4;
      }
      {
        const int i16 = lane & 15, kg = lane >> 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) slab[4096 + (16 * (w >> 1) + 4 * kg + q) * 32 + 16 * (w & 1) + i16] = accR[q];
      }
      __syncthreads();   // every read of Xp/Xc/ZT/DV/G of this layer is done; part complete
      if (tid < 96) {
        float s1 = 0.f;
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) s1 += part[pc * 96 + tid];
        slab[5120 + tid] = s1;
      }
      XSTAMP(12);
      // dSIG / dGATE: partial of tile t to slot (wave, t) of Xp..DVs (64 KiB, dead until the next
      // layer's G-build barrier), lane-linear in accumulator order; wave w sums tile w over waves
      {
        float* SCR = Xp;
        const int wu = __builtin_amdgcn_readfirstlane(w);
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(floatx4*)(SCR + (wu * 4 + t4) * 1024 + (g * 64 + lane) * 4) =
                floatx4{accT[t4][4 * g], accT[t4][4 * g + 1], accT[t4][4 * g + 2], accT[t4][4 * g + 3]};
        __syncthreads();
        XSTAMP(13);
        floatx16 accW;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          floatx4 v[4];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) v[s4] = *(const floatx4*)(SCR + ((s4 * 4 + wu) * 1024 + (g * 64 + lane) * 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) accW[4 * g + e] = (v[0][e] + v[1][e]) + (v[2][e] + v[3][e]);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) slab[w * 1024 + acc_row(q, h) * 32 + pi] = accW[q];
      }
      XSTAMP(6);
    }
#undef XSTAMP
  }
}

// ---- backward chain, 16-position waves (round 4) --------------------------------------------
// chain_bwd16_kernel<NW, TR>: chain_bwd_x3_kernel's layer walk, hand-off protocol, images and slab
// layout with 16 positions per wave and NW waves per block (tile TP = 16·NW: NW = 8 puts two
// waves on each SIMD).  Lane = (j = lane & 15: the wave's position, g = lane >> 4); two channel
// layouts per lane (q0 = 2(g >> 1), h = g & 1):
//   N  (x / g / out_a / out_c0): block xb register r = channel 16xb + 4g + r;
//   Zl (dz / z / σ / dv, the forward's z layout): block b register r = channel 8(q0 + b) + 4h + r.
//  * dz = dZ + RES·g on 16x16x32 bf16 splits (round 5; 16 f32 16x16x4 MFMAs before): A row i of
//    block b = z channel ch16(b, i) from the RX image, k = 8g + e = g's channel 16(e >> 2) + 4g +
//    (e & 3), i.e. the lane's two N-layout g registers split as they are;
//  * dx = W·dv on 16x16x32 bf16 splits, k-step S = sig / gate: the lane's 8 dv values of kind S
//    (Zl blocks 0, 1) are exactly the backward image's k order kk = 32S + 8g + e (WD unchanged);
//  * dSIG / dGATE: wave w takes weight-gradient tile w & 3 (2·kind + tap) over positions
//    [(w >> 2)·TP/NH, +TP/NH) (NH = NW/4 position halves) on 32x32x16 bf16 splits (k = 16
//    positions), and dRES quarter w & 3 over the same positions on 16x16x4 f32; with NH = 2 the
//    two halves' partials are summed through LDS by waves 0-3.
// LDS rows: Xp / Xc / ZT unpadded (LDS-DMA), DVs / DVg / G / OC padded to XS = 36 floats (the
// b128 own-row writes of 16 consecutive rows fall on 16 distinct bank groups).
template <int NW>
constexpr int cb16_lds() { return B16IMG_F + 3 * 16 * NW * 32 + 4 * 16 * NW * XS + 8 * 96; }
static_assert(cb16_lds<8>() * 4 + 16 <= 160 * 1024, "chain bwd16 LDS");
static_assert(4 * 1280 <= 3 * 128 * 32, "bwd16: the partial scratch (waves 4-7) must fit in Xp | Xc | ZT");

// GC rows of a wave whose 16 positions are not one voice: dv column sums per run of equal ids,
// one atomic per run and column (as gc_scatter_x3, 16 positions)
LBWN_DEV void gc_scatter16(float* gtab, long ld, const float* DVs, const float* DVg, int w, int lane, int Cd,
                           unsigned starts, int pid) {
  const int o = lane, oc = o & 31;
  const float* pl = o < 32 ? DVs : DVg;
  const int col = o < 32 ? oc : Cd + oc;
  unsigned rest = starts;
  while (rest) {   // wave-uniform
    const int p0 = __ffs(rest) - 1;
    rest &= rest - 1;
    const int p1 = rest ? __ffs(rest) - 1 : 16;
    const int id = __shfl(pid, p0);
    if (id < 0) continue;   // positions past T
    float s = 0.f;
    for (int p = p0; p < p1; ++p) s += pl[(16 * w + p) * XS + oc];
    if (oc < Cd) atomicAdd(gtab + (long)id * ld + col, s);
  }
}

template <int NW, bool TR>
__global__ __launch_bounds__(64 * NW) void chain_bwd16_kernel(ChainBK a) {
  constexpr int TP = 16 * NW, NT = 64 * NW, NH = NW / 4, PH = TP / NH;   // PH: positions per half
  constexpr int NR = TP * 8 / NT;                                        // float4 per thread of a tile (2)
  __shared__ __attribute__((aligned(16))) float sm[cb16_lds<NW>()];
  __shared__ int s_fail;
  float* IMG = sm;
  const unsigned short* WD = (const unsigned short*)IMG;
  const unsigned short* RX = WD + BD_US;
  // Xp | Xc | ZT | DVs | DVg | G | OC | part
  float* Xp = IMG + B16IMG_F;
  float* Xc = Xp + TP * 32;
  float* ZT = Xc + TP * 32;
  float* DVs = ZT + TP * 32;
  float* DVg = DVs + TP * XS;
  float* G = DVg + TP * XS;
  float* OC = G + TP * XS;
  float* part = OC + TP * XS;   // [8][96] bias partials
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4, q0 = 2 * (g >> 1), h = g & 1;
  const int r = 16 * w + i16;
  const int tps = (a.T + TP - 1) / TP, ntiles = a.B * tps;
  const int oc_bytes = (int)std::min<long>(a.ocls * 4, 0x7fffffffL);
  if (tid == 0) s_fail = 0;
  const int first = chain_first(a.xcd);
  for (int it = first; it < ntiles; it += gridDim.x) {
    const int tile = ntiles - 1 - it;
    const int b = tile / tps, tt = tile % tps, t0 = tt * TP;
    const int t = t0 + r;
    const bool valid = t < a.T;
    const long mb = (long)b * a.T, m = mb + t, mc = mb + min(t, a.T - 1);
    const long sb = (long)b * (a.H + a.T) * 32;
    const int myid = (a.gc_tab && valid) ? a.ids[m] : 0;
    const int tile_id = a.gc_tab ? a.ids[mb + t0] : 0;
    const bool tile_uni = __syncthreads_and(!valid || myid == tile_id);
    if (a.tile_gid && tid == 0) a.tile_gid[tile] = tile_uni ? tile_id : -1;
    // this wave's id runs over its 16 positions (lanes j of the first group), -1 past T
    const int gc_pid = valid ? myid : -1;
    const int gc_prev = __shfl(gc_pid, max(lane - 1, 0) & 15);
    const unsigned gc_starts = (unsigned)(__ballot(g == 0 && (i16 == 0 || gc_pid != gc_prev)) & 0xffffull);
    // per-layer rows of this lane's position (Zl channels): dZ, z, σ, issued a layer ahead
    // (buffer loads: a per-layer scalar base and one 32-bit lane offset per array, instead of three
    // 64-bit lane addresses held across the layer loop; the launcher checks the byte ranges)
    floatx4 dzr[2], zr[2], sgr[2];
    const int o_sg = (int)(sg_off(mc, q0, h) * 4), o_z = (int)((mc * a.lddz + 8 * q0 + 4 * h) * 4);
    auto load_regs = [&](int l) {
      const __amdgpu_buffer_rsrc_t rdz = __builtin_amdgcn_make_buffer_rsrc((void*)(a.DZ + l * a.dzls), (short)0, 0x7fffffff, BUF_DW3);
      const __amdgpu_buffer_rsrc_t rsg = __builtin_amdgcn_make_buffer_rsrc((void*)(a.SG + (long)l * a.sgls), (short)0, 0x7fffffff, BUF_DW3);
      const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)(a.Zf + (long)l * 32), (short)0, 0x7fffffff, BUF_DW3);
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {   // q0 + 1: the next 8-channel group (sg_off + 256 floats, z + 8)
        dzr[bb] = __builtin_amdgcn_raw_buffer_load_b128(rdz, o_sg + 1024 * bb, 0, 0);
        zr[bb] = __builtin_amdgcn_raw_buffer_load_b128(rz, o_z + 32 * bb, 0, 0);
        sgr[bb] = __builtin_amdgcn_raw_buffer_load_b128(rsg, o_sg + 1024 * bb, 0, 0);
      }
    };
    auto dma_image = [&](int l) {
      const float* src = a.bimg + (long)l * BIMG_F + lane * 4;
      for (int i = w; i < B16IMG_F / 256; i += NW) dma16(src + (i < BD_PC ? i : i - BD_PC + RX_GPC) * 256, IMG + i * 256);
    };
    __syncthreads();  // previous tile's LDS use done
    dma_image(a.L - 1);
    load_regs(a.L - 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    floatx4 oa[2];  // out_a of layer l+1, own row (N layout)
    oa[0] = oa[1] = floatx4{0.f, 0.f, 0.f, 0.f};
    const bool trc = a.trace && (int)blockIdx.x == a.trace_blk && tid == 0 && it == first;
#define XSTAMP(i) if (TR && trc) a.trace[16 * l + (i)] = clock64()
    // the producer's out_c0 rows for the next layer's G build, loaded in this layer's tail (after
    // the weight-gradient products, when the producer published long ago): its flag wait and
    // load latency overlap the bias sums and slab stores instead of opening the next layer
    floatx4 gl[NR];
    for (int l = a.L - 1; l >= 0; --l) {
      XSTAMP(0);
      const int d = 1 << (l % a.nbl);
      const int dn = (l + 1 < a.L) ? 1 << ((l + 1) % a.nbl) : 0;
      // 1. G = dx_{l+1} rows: out_c0_{l+1}[t + dn] (own OC / the producer's rows, gl) + out_a
      if (dn) {
        XSTAMP(7);
        floatx4 go[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int e = tid + NT * i, sr = (e >> 3) + dn, c4 = (e & 7) * 4;
          go[i] = *(const floatx4*)(OC + min(sr, TP - 1) * XS + c4);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int e = tid + NT * i, row = e >> 3, c4 = (e & 7) * 4, sr = row + dn, ts = t0 + sr;
          floatx4 v = sr < TP ? go[i] : gl[i];
          if (ts >= a.T) v = floatx4{0.f, 0.f, 0.f, 0.f};
          *(floatx4*)(G + row * XS + c4) = v;
        }
        XSTAMP(14);
        // lands this wave's part of the weight image (DMA'd during the last layer) and the
        // prefetched rows; the barrier then covers every wave's part
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        XSTAMP(15);
        __syncthreads();
      }
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) asm volatile("" ::"v"(dzr[bb]), "v"(zr[bb]), "v"(sgr[bb]));
      const float* xl = a.X + (long)l * a.xls + sb;
      // this layer's x rows (x[t-d] | x[t]) and z rows by LDS-DMA into Xp / Xc / ZT, 8 rows per piece
      auto dma_rows3 = [&](int k) {
        const int row = 8 * k + (lane >> 3), c4 = (lane & 7) * 4;
        const int trow = min(t0 + row, a.T - 1);
        dma16(xl + (long)(a.H + trow - d) * 32 + c4, Xp + 8 * k * 32);
        dma16(xl + (long)(a.H + trow) * 32 + c4, Xc + 8 * k * 32);
        dma16(a.Zf + (mb + trow) * a.lddz + (long)l * 32 + c4, ZT + 8 * k * 32);
      };
      XSTAMP(1);
      floatx4 gv[2];
#pragma unroll
      for (int xb = 0; xb < 2; ++xb) {   // own row: + out_a (the top layer writes it, g = 0)
        float* gp = G + r * XS + 16 * xb + 4 * g;
        floatx4 v = dn ? *(const floatx4*)gp : floatx4{0.f, 0.f, 0.f, 0.f};
        v += oa[xb];
        gv[xb] = v;
        *(floatx4*)gp = v;
      }
      // 2. dz = dZ + RES·g on the bf16 cores: one 32-deep k-step of six split products per block
      //    bb (A row i = z channel ch16(bb, i) of RX, k = 8g + e = the lane's g registers in order)
      floatx4 dz[2];
      {
        bf16x8 gb[3];
        split8(gv[0], gv[1], gb);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          bf16x8 rx[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) rx[p] = *(const bf16x8*)(RX + ch16(bb, i16) * RX_ROW + 32 * p + 8 * g);
          dz[bb] = mfma16x3(rx, gb, valid ? dzr[bb] : floatx4{0.f, 0.f, 0.f, 0.f});
          // x / z rows of this layer: pieces k = w, w + NW, ... (3·TP/8 rows of 8 over the block)
#pragma unroll
          for (int k2 = 0; k2 < TP / 8 / NW / 2 + 1; ++k2) {
            const int k = w + NW * (2 * k2 + bb);
            if (k < TP / 8) dma_rows3(k);
          }
        }
      }
      // 3. dv from z and σ: tanh = z/σ (σ = 0 only where dv is 0 anyway)
      floatx4 dvs[2], dvg[2];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float zz = zr[bb][e], sg = sgr[bb][e];
          const float th = sg > 1e-30f ? zz * __builtin_amdgcn_rcpf(sg) : 0.f;
          dvs[bb][e] = dz[bb][e] * sg * (1.f - th * th);
          dvg[bb][e] = dz[bb][e] * zz * (1.f - sg);
        }
      {
        // DV export: rows (layer l at columns l·64) or k-blocked (a.dvks: [L·2][Mp][32] chunks)
        float* dvo = (a.dv_out && valid)
                         ? a.dv_out + (a.dvks ? 2L * l * a.dvks + m * 32 : m * a.lddv + (long)l * 64) : nullptr;
        const long dgo = a.dvks ? a.dvks : 32;   // gate half
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          const int c = 8 * (q0 + bb) + 4 * h;
          *(floatx4*)(DVs + r * XS + c) = dvs[bb];
          *(floatx4*)(DVg + r * XS + c) = dvg[bb];
          if (dvo) {
            *(floatx4*)(dvo + c) = dvs[bb];
            *(floatx4*)(dvo + dgo + c) = dvg[bb];
          }
        }
      }
      XSTAMP(2);
      // 4. dx on the bf16 cores: out_a = g + W1·dv, out_c0 = W0·dv (k-steps S = 0 sig, 1 gate)
      floatx4 acc_a[2] = {gv[0], gv[1]}, acc_c[2];
      acc_c[0] = acc_c[1] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int S = 0; S < 2; ++S) {
        bf16x8 fa[2][3], fc[2][3];
#pragma unroll
        for (int xb = 0; xb < 2; ++xb)
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            fa[xb][p] = *(const bf16x8*)(WD + (32 + 16 * xb + i16) * XW_ROW + 64 * p + 32 * S + 8 * g);
            fc[xb][p] = *(const bf16x8*)(WD + (16 * xb + i16) * XW_ROW + 64 * p + 32 * S + 8 * g);
          }
        bf16x8 bx[3];
        if (S == 0) split8(dvs[0], dvs[1], bx);
        else split8(dvg[0], dvg[1], bx);
#pragma unroll
        for (int xb = 0; xb < 2; ++xb) {
          acc_a[xb] = mfma16x3(fa[xb], bx, acc_a[xb]);
          acc_c[xb] = mfma16x3(fc[xb], bx, acc_c[xb]);
        }
      }
      {
        const __amdgpu_buffer_rsrc_t rw =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)l * a.ocls, (short)0, oc_bytes, BUF_DW3);
        const bool pub = l > 0 && valid && r < min(d, TP);
#pragma unroll
        for (int xb = 0; xb < 2; ++xb) {
          *(floatx4*)(OC + r * XS + 16 * xb + 4 * g) = acc_c[xb];
          if (pub) __builtin_amdgcn_raw_buffer_store_b128(acc_c[xb], rw, (int)((m * 32 + 16 * xb + 4 * g) * 4), 0, 16);
        }
      }
      if (l == 0 && valid) {
#pragma unroll
        for (int xb = 0; xb < 2; ++xb) {
          *(floatx4*)(a.dx0_a + m * 32 + 16 * xb + 4 * g) = acc_a[xb];
          *(floatx4*)(a.dx0_c + m * 32 + 16 * xb + 4 * g) = acc_c[xb];
        }
      }
      oa[0] = acc_a[0];
      oa[1] = acc_a[1];
      XSTAMP(3);
      // 5. publish out_c0_l (the drain also lands this layer's x / z DMA pieces)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // DV, G, OC, Xp/Xc/ZT complete; the weight image is dead
      if (tid == 0 && l > 0) publish_flag(a.flags + tile, (unsigned)(a.L - l));
      if (a.gc_dtab && !tile_uni) gc_scatter16(a.gc_dtab + (long)l * 64, a.gc_ld, DVs, DVg, w, lane, 32, gc_starts, gc_pid);
      XSTAMP(4);
      // 6. dSIG / dGATE tile t4 = w & 3 (2·kind + tap) over this wave's position half:
      //    A[i = in][k = pos] = X_tap[pos][in], B[k = pos][j = o] = DV_kind[pos][o]
      const int t4 = w & 3, p0 = (w >> 2) * PH;
      floatx16 accT;
#pragma unroll
      for (int q = 0; q < 16; ++q) accT[q] = 0.f;
      {
        const float* XA = (t4 & 1) ? Xc : Xp;
        const float* DB = (t4 & 2) ? DVg : DVs;
        const int pi = lane & 31, hh = lane >> 5;
        float xa[PH / 16][8], db[PH / 16][8];
#pragma unroll
        for (int s2 = 0; s2 < PH / 16; ++s2)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int p = p0 + 16 * s2 + 8 * hh + e;
            xa[s2][e] = XA[p * 32 + pi];
            db[s2][e] = DB[p * XS + pi];
          }
        XSTAMP(8);
        if (l > 0) {   // the next layer's image and rows, behind this layer's operand reads
          dma_image(l - 1);
          load_regs(l - 1);
        }
        XSTAMP(9);
#pragma unroll
        for (int s2 = 0; s2 < PH / 16; ++s2) {
          bf16x8 fx[3], fd[3];
          split8(floatx4{xa[s2][0], xa[s2][1], xa[s2][2], xa[s2][3]}, floatx4{xa[s2][4], xa[s2][5], xa[s2][6], xa[s2][7]}, fx);
          split8(floatx4{db[s2][0], db[s2][1], db[s2][2], db[s2][3]}, floatx4{db[s2][4], db[s2][5], db[s2][6], db[s2][7]}, fd);
          accT = mfma_x3(fx, fd, accT);
          if (s2 == 0) XSTAMP(10);
        }
      }
      XSTAMP(5);
      // 7. dRES quarter t4 (16x16: z channels 16(t4>>1).., res out 16(t4&1)..) over the same
      //    positions on v_mfma_f32_16x16x4_f32: A[i=c][k=pos] = z[pos][c], B[k=pos][j=o] = g[pos][o]
      floatx4 accR = {0.f, 0.f, 0.f, 0.f};
      {
        const int cz = 16 * (t4 >> 1) + i16, og = 16 * (t4 & 1) + i16;
#pragma unroll
        for (int c8 = 0; c8 < PH / 32; ++c8) {
          float za[8], ga[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int p = p0 + 32 * c8 + 4 * e + g;
            za[e] = ZT[p * 32 + cz];
            ga[e] = G[p * XS + og];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int e = 0; e < 8; ++e) accR = __builtin_amdgcn_mfma_f32_16x16x4f32(za[e], ga[e], accR, 0, 0, 0);
        }
      }
      XSTAMP(11);
      // 8. bias partials (column sums of DVs, DVg, G: waves 0-2; lane = (row class pc, 4-column
      //    group c4), rows pc + 8p)
      float* slab = a.slab + ((long)l * ntiles + tile) * SLAB;
      if (w < 3) {
        const int c4 = (lane & 7) * 4, pc = lane >> 3;
        const float* pl = w == 0 ? DVs : w == 1 ? DVg : G;
        floatx4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < TP / 8; ++p) s4 += *(const floatx4*)(pl + (pc + 8 * p) * XS + c4);
        *(floatx4*)(part + pc * 96 + 32 * w + c4) = s4;
      }
      // the next layer's producer: its flag (published after its dx of this layer, half a layer
      // ago) and then its out_c0 rows, loaded after the barrier below
      const int pn = tt + max(1, d / TP);
      if (l > 0 && pn < tps && tid == 0 && !s_fail) {
        if (!wait_flag_ge(a.flags + (long)b * tps + pn, (unsigned)(a.L - l), a.status, 2u)) s_fail = 1;
      }
      __syncthreads();   // every read of Xp/Xc/ZT/DV/G of this layer is done; part complete; the flag seen
      {
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(a.ocg + (long)l * a.ocls, (short)0, oc_bytes, BUF_DW3);
#pragma unroll
        for (int i = 0; i < NR; ++i) {   // (l = 0: a dead load of valid rows)
          const int e = tid + NT * i, c4 = (e & 7) * 4;
          const int ts = min(t0 + (e >> 3) + d, a.T - 1);
          gl[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(((mb + ts) * 32 + c4) * 4), 0, 16);
        }
      }
      if (tid < 96) {
        float s1 = 0.f;
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) s1 += part[pc * 96 + tid];
        slab[5120 + tid] = s1;
      }
      XSTAMP(12);
      // weight-gradient partials to the slab: with two position halves, each wave parks its
      // partials lane-linear in Xp.. (dead until the next layer's G-build barrier) and waves 0-3
      // sum halves 0 + 1 of their tile / quarter in a fixed order
      if (NH == 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) slab[t4 * 1024 + acc_row(q, lane >> 5) * 32 + (lane & 31)] = accT[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) slab[4096 + (16 * (t4 >> 1) + 4 * g + q) * 32 + 16 * (t4 & 1) + i16] = accR[q];
      } else {
        // (only waves 4-7 park theirs: waves 0-3 add their own half from registers, in the same order)
        if (w >= 4) {
          float* SCR = Xp + (w - 4) * 1280;
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4)
            *(floatx4*)(SCR + (q4 * 64 + lane) * 4) = floatx4{accT[4 * q4], accT[4 * q4 + 1], accT[4 * q4 + 2], accT[4 * q4 + 3]};
          *(floatx4*)(SCR + 1024 + lane * 4) = accR;
        }
        __syncthreads();
        XSTAMP(13);
        if (w < 4) {
          const float* S1 = Xp + w * 1280;
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const floatx4 v = floatx4{accT[4 * q4], accT[4 * q4 + 1], accT[4 * q4 + 2], accT[4 * q4 + 3]} +
                              *(const floatx4*)(S1 + (q4 * 64 + lane) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) slab[w * 1024 + acc_row(4 * q4 + e, lane >> 5) * 32 + (lane & 31)] = v[e];
          }
          const floatx4 v = accR + *(const floatx4*)(S1 + 1024 + lane * 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) slab[4096 + (16 * (w >> 1) + 4 * g + q) * 32 + 16 * (w & 1) + i16] = v[q];
        }
      }
      XSTAMP(6);
    }
#undef XSTAMP
  }
}

}  // namespace

// the 16-position-wave backward chain of NW waves
template <int NW>
static void launch_bwd16(bool tr, int grid, const ChainBK& k, hipStream_t st) {
  void (*f)(ChainBK) = tr ? chain_bwd16_kernel<NW, true> : chain_bwd16_kernel<NW, false>;
  hipLaunchKernelGGL(f, dim3(grid), dim3(64 * NW), 0, st, k);
}

int lbwn_chain_bwd_launch(const lbwn_chain_args& c, hipStream_t st) {
  LBWN_REQUIRE(c.Cr == 32 && c.Cd == 32, "chain bwd: n_res = n_dil = 32 only");
  LBWN_REQUIRE(c.grid >= 1 && c.flags && c.status && c.slab && c.ocg && c.dx0_a && c.dx0_c && c.DZ,
               "chain bwd: bad launch state");
  ChainBK k;
  k.X = c.X; k.xls = c.xls; k.DZ = c.DZ; k.lddz = c.ldz; k.dzls = c.dzls; k.wpack = c.wpack; k.slab = c.slab;
  k.ocg = c.ocg; k.ocls = c.ocls; k.dx0_a = c.dx0_a; k.dx0_c = c.dx0_c;
  k.gc_tab = c.gc_tab; k.gc_ld = c.gc_ld; k.ids = c.ids; k.cond = c.cond; k.ldcond = c.ldcond;
  k.dv_out = c.dv_out; k.lddv = c.lddv; k.gc_dtab = c.gc_dtab; k.tile_gid = c.tile_gid;
  k.dvks = c.dvks;
  k.flags = c.flags; k.status = c.status;
  k.B = c.B; k.T = c.T; k.H = c.H; k.L = c.L; k.nbl = c.nbl; k.Cd = c.Cd;
  k.trace = c.trace ? c.trace + 16L * c.L : nullptr; k.trace_blk = c.trace_blk;
  k.xcd = c.xcd;
  k.Zf = c.Z; k.SG = c.SG; k.sgls = c.sgls; k.bimg = c.bimg;
  const bool x3 = c.bimg && c.SG && c.Z;
  if (x3) LBWN_REQUIRE((((uintptr_t)c.bimg) & 15) == 0 && (((uintptr_t)c.SG) & 15) == 0 && (c.ldz & 3) == 0,
                       "chain bwd x3: misaligned images / rows");
  LBWN_REQUIRE(c.bwd_nw == 0 || ((c.bwd_nw == 4 || c.bwd_nw == 8) && x3),
               "chain bwd: 16-position waves need the bf16-split form, 4 or 8 waves");
  const int tp = lbwn_chain_fwd_tile(c.bwd_nw);
  const int tps = (c.T + tp - 1) / tp;
  // hand-off flags only: the status word is sticky for the whole step
  if (!c.flags_zeroed) {
    if (int e = lbwn_zero_launch(c.flags, ((size_t)c.B * tps * 4 + 15) / 16 * 16, st)) return e;
  }
  LBWN_REQUIRE(x3 == (c.dzls > 0), "chain bwd: the bf16-split chain reads dZ in chain order (dzls), the f32 chain in rows");
  if (c.bwd_nw)   // 32-bit byte offsets of the per-lane row loads (chain_bwd16_kernel load_regs)
    LBWN_REQUIRE(c.dzls * 4 < 0x7fffffffL && c.sgls * 4 < 0x7fffffffL && (long)c.B * c.T * c.ldz * 4 < 0x7fffffffL,
                 "chain bwd: dZ / SG layer or z rows past 2 GiB");
  const bool tr = k.trace != nullptr;
  if (c.bwd_nw == 8) launch_bwd16<8>(tr, c.grid, k, st);
  else if (c.bwd_nw == 4) launch_bwd16<4>(tr, c.grid, k, st);
  else if (x3 && tr) chain_bwd_x3_kernel<true><<<c.grid, 256, 0, st>>>(k);
  else if (x3) chain_bwd_x3_kernel<false><<<c.grid, 256, 0, st>>>(k);
  else chain_bwd_kernel<<<c.grid, 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}
