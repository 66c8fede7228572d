// One WaveNet residual layer, forward and backward (tmodel.py:117-184, :313-325).
//
// Layout: activations are channels-last rows; x_l lives in a per-stream buffer
// [B][H+T][Cr] whose first H rows are a halo: rows [H-d, H) hold SAVE_l, so the dilated
// tap x[t-d] (or SAVE for t<d, tmodel.py:122-127) is simply row H+t-d.  A block owns 128
// consecutive positions of one stream (grid-stride over such tiles); both taps are staged
// into LDS with coalesced 16-B loads (Xp = rows t-d, Xc = rows t), then each wave computes
// a 32-position tile with v_mfma_f32_32x32x2_f32 in the TRANSPOSED orientation (channels on
// MFMA rows, positions on lanes) so that the gate output z is already the B operand of the
// residual / dx products (no lane shuffles):
//   vᵀ[64 × 32pos] = Wcatᵀ[64 out × 64 in] · [x[t-d] | x[t]]ᵀ   (sig rows 0-31, gate 32-63)
//   zᵀ = tanh(v_sig)·σ(v_gate);  x_{l+1}ᵀ = x_lᵀ + RESᵀ·zᵀ + b_res
// Weights arrive pre-packed per layer in the exact padded LDS image (lbwn_pack_layers), so
// staging is a straight 16-B copy.  Channel counts up to 32 are supported (zero-padded).
#include "common.h"
#include "kernels.h"
#include "layer_common.h"

namespace {

// G[r] = g_a[t] + (t+gd < T ? g_c0[t+gd] : 0) for t = t0 + r (rows of [M][C] buffers of stream b)
LBWN_DEV void stage_g(float* G, const float* __restrict__ ga, const float* __restrict__ gc, int gd, long mb,
                      int t0, int T, int C, int tid) {
  if (!ga) {
    for (int e = tid; e < LP * XS; e += 256) G[e] = 0.f;
    return;
  }
  if (C == 32) {
    floatx4 v[4], u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 3, c4 = (e & 7) * 4, t = t0 + r;
      v[i] = *(const floatx4*)(ga + (mb + min(t, T - 1)) * 32 + c4);       // clamped, then select
      u[i] = gc ? *(const floatx4*)(gc + (mb + min(t + gd, T - 1)) * 32 + c4) : floatx4{0.f, 0.f, 0.f, 0.f};
      if (t >= T) v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (t + gd >= T || !gc) u[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      *(floatx4*)(G + (e >> 3) * XS + (e & 7) * 4) = v[i] + u[i];
    }
  } else {
    for (int e = tid; e < LP * 32; e += 256) {
      const int r = e >> 5, c = e & 31, t = t0 + r;
      float v = 0.f;
      if (t < T && c < C) {
        v = ga[(mb + t) * C + c];
        if (gc && t + gd < T) v += gc[(mb + t + gd) * C + c];
      }
      G[r * XS + c] = v;
    }
  }
}

// vᵀ for this wave's 32 positions: acc_s/acc_g rows = out channel, lanes = position.
template <typename K>
LBWN_DEV void conv_tile(const float* Xp, const float* Xc, const float* Ws, const float* bs,
                        const K& a, long m, bool valid, int w, int lane, floatx16& acc_s,
                        floatx16& acc_g) {
  const int pi = lane & 31, h = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc_s[r] = bs[acc_row(r, h)];
    acc_g[r] = bs[32 + acc_row(r, h)];
  }
  if (valid && (a.gc_tab || a.cond)) {
    const float* cs = a.gc_tab ? a.gc_tab + (long)a.ids[m] * a.gc_ld : nullptr;
    const float* cl = a.cond ? a.cond + m * a.ldcond : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = acc_row(r, h);
      if (o < a.Cd) {
        if (cs) { acc_s[r] += cs[o]; acc_g[r] += cs[a.Cd + o]; }
        if (cl) { acc_s[r] += cl[o]; acc_g[r] += cl[a.Cd + o]; }
      }
    }
  }
  const float* xp = Xp + (32 * w + pi) * XS;
  const float* xc = Xc + (32 * w + pi) * XS;
  // operands of group g (8 k values: k = 8g+4h+j) are fetched while group g-1's MFMAs issue
  floatx4 bx[2];
  float ws_[2][4], wg_[2][4];
  auto load = [&](int g, int buf) {
    const float* src = g < 4 ? xp : xc;
    bx[buf] = *(const floatx4*)(src + 8 * (g & 3) + 4 * h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 8 * g + 4 * h + j;
      ws_[buf][j] = Ws[k * WS + pi];
      wg_[buf][j] = Ws[k * WS + 32 + pi];
    }
  };
  load(0, 0);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int cb = g & 1;
    if (g + 1 < 8) load(g + 1, cb ^ 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_s = mfma32(ws_[cb][j], bx[cb][j], acc_s);
      acc_g = mfma32(wg_[cb][j], bx[cb][j], acc_g);
    }
  }
}

// ---- forward ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void layer_fwd_kernel(FwdK a) {
  __shared__ __attribute__((aligned(16))) float sm[2 * LP * XS + WIMG];
  float* Xp = sm;
  float* Xc = Xp + LP * XS;
  float* Ws = Xc + LP * XS;
  float* Rs = Ws + 64 * WS;
  float* bs = Rs + 32 * XS;
  float* br = bs + 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pi = lane & 31, h = lane >> 5;
  const int tps = (a.T + LP - 1) / LP, ntiles = a.B * tps;
  stage_image(Ws, a.wpack, tid);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, t0 = (tile % tps) * LP;
    const float* xb = a.x_in + (long)b * (a.H + a.T) * a.Cr;
    if (tile != (int)blockIdx.x) __syncthreads();  // previous tile's LDS reads done
    stage_rows(Xp, xb, t0, -a.d, a.T, a.H, a.Cr, tid);
    stage_rows(Xc, xb, t0, 0, a.T, a.H, a.Cr, tid);
    __syncthreads();

    const int t = t0 + 32 * w + pi;
    const bool valid = t < a.T;
    const long m = (long)b * a.T + t;
    floatx16 acc_s, acc_g;
    conv_tile(Xp, Xc, Ws, bs, a, m, valid, w, lane, acc_s, acc_g);
    floatx16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = tanhf_(acc_s[r]) * sigmoidf_(acc_g[r]);
    if (a.x_out) {
      floatx16 acc_r;
      const float* xc = Xc + (32 * w + pi) * XS;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 xv = *(const floatx4*)(xc + 8 * q + 4 * h);
        const floatx4 bv = *(const floatx4*)(br + 8 * q + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_r[4 * q + j] = xv[j] + bv[j];
      }
      float ra[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) ra[s] = Rs[acc_row(s, h) * XS + pi];
#pragma unroll
      for (int s = 0; s < 16; ++s) acc_r = mfma32(ra[s], z[s], acc_r);
      if (valid) store_rows16(a.x_out + ((long)b * (a.H + a.T) + a.H + t) * a.Cr, acc_r, a.Cr, h);
    }
    if (valid) store_rows16(a.z + m * a.ldz, z, a.Cd, h);
  }
}

// ---- deferred slab reduction -------------------------------------------------------------

// Destination of slab column c (padded 32-channel layout) in reference layout.
LBWN_DEV void slab_store(const RedK& a, int c, float tot) {
  const int Cr = a.Cr, Cd = a.Cd;
  if (c < 4096) {
    const int cc = c & 2047, tap = cc >> 10, in = (cc >> 5) & 31, o = cc & 31;
    float* dst = c < 2048 ? a.dsig : a.dgate;
    if (in < Cr && o < Cd) dst[(tap * Cr + in) * Cd + o] = tot;
  } else if (c < 5120) {
    const int cc = c - 4096, zc = cc >> 5, o = cc & 31;
    if (zc < Cd && o < Cr) a.dres[zc * Cr + o] = tot;
  } else {
    const int cc = c - 5120, seg = cc >> 5, o = cc & 31;
    if (seg == 0 && a.dbsig && o < Cd) a.dbsig[o] = tot;
    if (seg == 1 && a.dbgate && o < Cd) a.dbgate[o] = tot;
    if (seg == 2 && a.dbres && o < Cr) a.dbres[o] = tot;
  }
}

// Column group `grp` (32 columns) summed over all parts: thread = (part lane p8, column);
// `pre` holds parts p8, p8+8, ... (up to RED_PARTS) loaded earlier.
LBWN_DEV void slab_group_finish(const RedK& a, int grp, const float (&pre)[RED_PARTS], float* scratch,
                                int tid) {
  const int c = grp * 32 + (tid & 31), p8 = tid >> 5;
  float s = 0.f;
  if (c < SLAB) {
#pragma unroll
    for (int j = 0; j < RED_PARTS; ++j) s += pre[j];
    for (int p = p8 + 8 * RED_PARTS; p < a.nparts; p += 8) s += a.slab[(long)p * a.stride + c];
  }
  scratch[tid] = s;
  __syncthreads();
  if (tid < 32 && c < SLAB) {
    float tot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += scratch[j * 32 + tid];
    slab_store(a, c, tot);
  }
  __syncthreads();
}

LBWN_DEV void slab_group_prefetch(const RedK& a, int grp, float (&pre)[RED_PARTS], int tid) {
  const int c = grp * 32 + (tid & 31), p8 = tid >> 5;
#pragma unroll
  for (int j = 0; j < RED_PARTS; ++j) {
    const int p = p8 + 8 * j;
    pre[j] = (c < SLAB && p < a.nparts) ? a.slab[(long)p * a.stride + c] : 0.f;
  }
}

// Sum every layer's slab partials: grid (column groups, L).
// At most 32 VGPRs (22 at this writing, -Rpass-analysis=kernel-resource-usage): it runs on the side stream beside dSKIP's A-in-registers GEMM
// blocks (2 waves of 240 VGPRs per SIMD leave 32), so it must fit in what they leave free or it
// waits for them.  Parts p8, p8 + 8, ... in order (the order of slab_group_prefetch/finish).
__global__ __launch_bounds__(256) void layer_reduce_all_kernel(
    RedK a, long slab_layer, long dsig_l, long dres_l, long db_l) {
  __shared__ float scratch[256];
  const int l = blockIdx.y, tid = threadIdx.x;
  RedK k = a;
  k.slab = a.slab + l * slab_layer;
  k.dsig = a.dsig + l * dsig_l;
  k.dgate = a.dgate + l * dsig_l;
  k.dres = a.dres + l * dres_l;
  k.dbsig = a.dbsig ? a.dbsig + l * db_l : nullptr;
  k.dbgate = a.dbgate ? a.dbgate + l * db_l : nullptr;
  k.dbres = a.dbres ? a.dbres + l * (long)a.Cr : nullptr;
  const int c = blockIdx.x * 32 + (tid & 31), p8 = tid >> 5, cc = min(c, SLAB - 1);
  float s = 0.f;
  // buffer loads: one 32-bit offset per load instead of a 64-bit address (the VGPR budget above);
  // parts past nparts read past the record (0, and the zero is never added: nparts bounds it)
  const int st = (int)k.stride;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(k.slab), (short)0, (int)std::min<long>((long)k.nparts * st * 4, 0x7fffffffL), 0x00020000);
  for (int p0 = p8; p0 < k.nparts; p0 += 64) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, ((p0 + 8 * i) * st + cc) * 4, 0, 0));
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (p0 + 8 * i < k.nparts) ? v[i] : 0.f;
  }
  scratch[tid] = s;
  __syncthreads();
  if (tid < 32 && c < SLAB) {
    float tot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += scratch[j * 32 + tid];
    slab_store(k, c, tot);
  }
}

// ---- backward ----------------------------------------------------------------------------
// LDS (112.5 KB, so that one GEMM block of the concurrent weight-gradient stream fits
// beside it on the CU): Xp | Xc | G | IMG | DV.  After the dx step the weight image is dead
// and holds zᵀ (ZT); RED (dRES cross-wave sum, bias partials) reuses Xp once step 5 is done.
constexpr int BWD_LDS = 3 * LP * XS + WIMG + LP * DS;
static_assert(LP * XS <= WIMG, "ZT must fit in the weight image");
static_assert(4 * 1024 <= LP * XS, "RED must fit in Xp");

__global__ __launch_bounds__(256) void layer_bwd_kernel(BwdK a) {
  __shared__ __attribute__((aligned(16))) float sm[BWD_LDS];
  float* Xp = sm;
  float* Xc = Xp + LP * XS;
  float* G = Xc + LP * XS;
  float* Ws = G + LP * XS;
  float* Rs = Ws + 64 * WS;
  float* bs = Rs + 32 * XS;
  float* DV = Ws + WIMG;             // [LP][DS]   dv (sig | gate), position-major
  float* ZT = Ws;                    // [LP][XS]   z, position-major (after step 4)
  float* RED = Xp;                   // 4 × 1024 / [8][96] (after step 5)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pi = lane & 31, h = lane >> 5;
  const int tps = (a.T + LP - 1) / LP, ntiles = a.B * tps;

  floatx16 accW, accR;  // tile w of dSIG/dGATE (w: 0 sig·prev, 1 sig·cur, 2 gate·prev, 3 gate·cur), dRES part
#pragma unroll
  for (int r = 0; r < 16; ++r) { accW[r] = 0.f; accR[r] = 0.f; }
  float bsum = 0.f;  // bias partial: tid<64 dv column, 64..95 g column

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, t0 = (tile % tps) * LP;
    const long mb = (long)b * a.T;
    const float* xb = a.x_in + (long)b * (a.H + a.T) * a.Cr;
    if (tile != (int)blockIdx.x) __syncthreads();  // previous tile's LDS reads done
    stage_image(Ws, a.wpack, tid);
    stage_rows(Xp, xb, t0, -a.d, a.T, a.H, a.Cr, tid);
    stage_rows(Xc, xb, t0, 0, a.T, a.H, a.Cr, tid);
    stage_g(G, a.g_a, a.g_c0, a.g_d, mb, t0, a.T, a.Cr, tid);
    const int t = t0 + 32 * w + pi;
    const bool valid = t < a.T;
    const long m = mb + t;
    // dZ_skip rows (acc layout: channels 8q+4h..+3 per q)
    floatx16 dz;
    if (a.Cd == 32) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        floatx4 v = *(const floatx4*)(a.dz_skip + (mb + min(t, a.T - 1)) * a.lddz + 8 * q + 4 * h);
        if (!valid) v = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[4 * q + j] = v[j];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = acc_row(r, h);
        dz[r] = (valid && c < a.Cd) ? a.dz_skip[m * a.lddz + c] : 0.f;
      }
    }
    __syncthreads();

    // 1. recompute the gate
    floatx16 acc_s, acc_g;
    conv_tile(Xp, Xc, Ws, bs, a, m, valid, w, lane, acc_s, acc_g);
    floatx16 th, sg;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      th[r] = tanhf_(acc_s[r]);
      sg[r] = sigmoidf_(acc_g[r]);
    }
    // 2. dzᵀ += RES·gᵀ   (dz[pos][c] = dZ[pos][c] + Σ_o g[pos][o]·RES[c][o])
    const float* gp = G + (32 * w + pi) * XS;
    {
      floatx4 gx[4], rx[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        gx[g] = *(const floatx4*)(gp + 8 * g + 4 * h);
        rx[g] = *(const floatx4*)(Rs + pi * XS + 8 * g + 4 * h);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) dz = mfma32(rx[g][j], gx[g][j], dz);
    }
    // 3. dvᵀ, parked position-major for the weight-grad products
    floatx16 dvs, dvg;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dvs[r] = dz[r] * sg[r] * (1.f - th[r] * th[r]);
      dvg[r] = dz[r] * th[r] * sg[r] * (1.f - sg[r]);
    }
    float* dvrow = DV + (32 * w + pi) * DS;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *(floatx4*)(dvrow + 8 * q + 4 * h) = floatx4{dvs[4 * q], dvs[4 * q + 1], dvs[4 * q + 2], dvs[4 * q + 3]};
      *(floatx4*)(dvrow + 32 + 8 * q + 4 * h) = floatx4{dvg[4 * q], dvg[4 * q + 1], dvg[4 * q + 2], dvg[4 * q + 3]};
    }
    // 4. dx: dcurᵀ = W1·dvᵀ (+ g), dprevᵀ = W0·dvᵀ   (rows = in channel)
    floatx16 acc_a, acc_c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const floatx4 gv = *(const floatx4*)(gp + 8 * q + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) { acc_a[4 * q + j] = gv[j]; acc_c[4 * q + j] = 0.f; }
    }
    {
      floatx4 wv[2][4];  // [buf][w0s, w0g, w1s, w1g]
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
    if (valid) {
      store_rows16(a.out_a + m * a.Cr, acc_a, a.Cr, h);
      store_rows16(a.out_c0 + m * a.Cr, acc_c, a.Cr, h);
    }
    __syncthreads();  // DV of every wave visible; nobody reads the weight image any more
    {
      float* zrow = ZT + (32 * w + pi) * XS;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        floatx4 zv;
#pragma unroll
        for (int j = 0; j < 4; ++j) zv[j] = th[4 * q + j] * sg[4 * q + j];
        *(floatx4*)(zrow + 8 * q + 4 * h) = zv;
      }
    }

    // 5. dSIG/dGATE tile w over all LP positions: A[i=in][k=pos] = X[pos][in], B[k][j=o] = DV[pos][o]
    {
      const float* X = (w & 1) ? Xc : Xp;
      const int oc = (w >> 1) * 32 + pi;
      float xa[2][8], da[2][8];
      auto loadb = [&](int bt, int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int p = 2 * (8 * bt + i) + h;
          xa[buf][i] = X[p * XS + pi];
          da[buf][i] = DV[p * DS + oc];
        }
      };
      loadb(0, 0);
#pragma unroll
      for (int bt = 0; bt < LP / 16; ++bt) {
        const int cb = bt & 1;
        if (bt + 1 < LP / 16) loadb(bt + 1, cb ^ 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) accW = mfma32(xa[cb][i], da[cb][i], accW);
      }
    }
    __syncthreads();  // ZT visible; Xp/Xc free for RED
    // 6. dRES part over this wave's 32 positions: A[i=c][k=pos] = z[pos][c], B[k][j=o] = g[pos][o]
    {
      float za[16], ga[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int p = 32 * w + 2 * s2 + h;
        za[s2] = ZT[p * XS + pi];
        ga[s2] = G[p * XS + pi];
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) accR = mfma32(za[s2], ga[s2], accR);
    }
    // bias partials: column sums of DV (64) and G (32) over the tile, 8 position chunks
    {
      float* part = RED;  // [8][96]
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
      __syncthreads();
      if (tid < 96) {
        float s1 = 0.f;
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) s1 += part[pc * 96 + tid];
        bsum += s1;
      }
    }
    // 7. optional dv export (LC grads) and GC table grads
    if (a.dv_out) {
      for (int e = tid; e < LP * 64; e += 256) {
        const int p = e >> 6, o = e & 63, oc = o & 31, tt = t0 + p;
        if (tt < a.T && oc < a.Cd) a.dv_out[(mb + tt) * a.lddv + (o < 32 ? oc : a.Cd + oc)] = DV[p * DS + o];
      }
    }
    if (a.gc_dtab) gc_scatter(a.gc_dtab, a.gc_ld, a.ids + mb, DV, t0, a.T, w, lane, a.Cd, -1);
  }

  // 8. block partial -> slab: tiles 0..3 straight from their wave, dRES summed over waves
  __syncthreads();  // bias partial reads of RED done
  float* slab = a.slab + (long)blockIdx.x * a.slab_stride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    slab[w * 1024 + acc_row(r, h) * 32 + pi] = accW[r];
    RED[w * 1024 + acc_row(r, h) * 32 + pi] = accR[r];
  }
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) slab[4096 + e] = ((RED[e] + RED[1024 + e]) + RED[2048 + e]) + RED[3072 + e];
  if (tid < 96) slab[5120 + tid] = bsum;
}

__global__ __launch_bounds__(256) void layer_reduce_kernel(RedK a) {
  __shared__ float scratch[256];
  float pre[RED_PARTS];
  const int ngroups = (SLAB + 31) / 32;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    slab_group_prefetch(a, grp, pre, threadIdx.x);
    slab_group_finish(a, grp, pre, scratch, threadIdx.x);
  }
}

int grid_fwd(const lbwn_layer_args& a) { return std::min(lbwn_layer_nblocks(a.B, a.T), 512); }
int grid_bwd(const lbwn_layer_args& a) { return std::min(lbwn_layer_nblocks(a.B, a.T), 256); }

FwdK to_fwd(const lbwn_layer_args& a) {
  FwdK k;
  k.x_in = a.x_in; k.x_out = a.x_out; k.z = a.z; k.wpack = a.wpack; k.gc_tab = a.gc_tab; k.ids = a.ids;
  k.cond = a.cond; k.ldz = a.ldz; k.ldcond = a.ldcond; k.gc_ld = a.gc_ld ? a.gc_ld : 2L * a.Cd;
  k.B = a.B; k.T = a.T; k.H = a.H; k.d = a.d; k.Cr = a.Cr; k.Cd = a.Cd;
  return k;
}
BwdK to_bwd(const lbwn_layer_args& a) {
  BwdK k;
  k.x_in = a.x_in; k.wpack = a.wpack; k.dz_skip = a.dz_skip; k.g_a = a.g_a; k.g_c0 = a.g_c0;
  k.out_a = a.out_a; k.out_c0 = a.out_c0; k.slab = a.slab; k.gc_tab = a.gc_tab; k.ids = a.ids; k.cond = a.cond;
  k.dv_out = a.dv_out; k.gc_dtab = a.gc_dtab; k.lddz = a.lddz; k.ldcond = a.ldcond; k.lddv = a.lddv;
  k.gc_ld = a.gc_ld ? a.gc_ld : 2L * a.Cd;
  k.B = a.B; k.T = a.T; k.H = a.H; k.d = a.d; k.Cr = a.Cr; k.Cd = a.Cd; k.g_d = a.g_d; k.slab_stride = a.slab_stride;
  return k;
}

}  // namespace

int lbwn_layer_slab_stride() { return SLAB; }

namespace {
// dL/d(halo buffer) of one layer from its backward's two outputs: out_a[t] = dL/dx[t] (own tap
// and residual) and out_c0[t] = dL/d(dilated tap input at t), which is halo row H + t - d.
__global__ void layer_dx_combine_kernel(const float* __restrict__ a, const float* __restrict__ c0, float* __restrict__ dx,
                                        int B, int T, int H, int d, int C) {
  const long total = (long)B * (H + T) * C;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long br = e / C;
    const int row = (int)(br % (H + T)), b = (int)(br / (H + T));
    const int s = row - H;
    const long mb = (long)b * T;
    float v = 0.f;
    if (s >= 0) v = a[(mb + s) * C + c];
    if (s + d >= 0 && s + d < T) v += c0[(mb + s + d) * C + c];
    dx[e] = v;
  }
}
}  // namespace

int lbwn_layer_dx_combine_launch(const float* out_a, const float* out_c0, float* dx, int B, int T, int H, int d, int C,
                                 hipStream_t st) {
  const long total = (long)B * (H + T) * C;
  layer_dx_combine_kernel<<<(int)std::min<long>((total + 255) / 256, 4096), 256, 0, st>>>(out_a, out_c0, dx, B, T, H,
                                                                                          d, C);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_layer_nblocks(int B, int T) { return B * ((T + LP - 1) / LP); }
int lbwn_layer_bwd_grid(int B, int T) { return std::min(lbwn_layer_nblocks(B, T), 256); }

static int check_layer(const lbwn_layer_args& a) {
  LBWN_REQUIRE(a.Cr >= 1 && a.Cr <= 32 && a.Cd >= 1 && a.Cd <= 32, "layer: n_res/n_dil must be in [1,32]");
  LBWN_REQUIRE(a.d >= 1 && a.d <= a.H, "layer: dilation %d exceeds halo %d", a.d, a.H);
  LBWN_REQUIRE(a.B >= 1 && a.T >= 1, "layer: empty batch");
  LBWN_REQUIRE(a.wpack && (((uintptr_t)a.wpack) & 15) == 0, "layer: packed weight image missing/misaligned");
  if (a.Cr == 32) LBWN_REQUIRE((((uintptr_t)a.x_in) & 15) == 0, "layer: x not 16-B aligned");
  return 0;
}

int lbwn_layer_fwd_launch(const lbwn_layer_args& a, hipStream_t st) {
  if (int e = check_layer(a)) return e;
  layer_fwd_kernel<<<grid_fwd(a), 256, 0, st>>>(to_fwd(a));
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_layer_bwd_launch(const lbwn_layer_args& a, hipStream_t st) {
  if (int e = check_layer(a)) return e;
  LBWN_REQUIRE(a.slab && a.slab_stride >= SLAB, "layer bwd: slab missing");
  layer_bwd_kernel<<<grid_bwd(a), 256, 0, st>>>(to_bwd(a));
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_layer_reduce_launch(const lbwn_layer_red_args& r, hipStream_t st) {
  LBWN_REQUIRE(r.slab && r.nparts >= 1 && r.stride >= SLAB, "layer reduce: bad slab");
  RedK k;
  k.slab = r.slab; k.dsig = r.dsig; k.dgate = r.dgate; k.dres = r.dres;
  k.dbsig = r.dbsig; k.dbgate = r.dbgate; k.dbres = r.dbres;
  k.nparts = r.nparts; k.stride = r.stride; k.Cr = r.Cr; k.Cd = r.Cd;
  layer_reduce_kernel<<<(SLAB + 31) / 32, 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_layer_reduce_all_launch(const lbwn_layer_red_args& r, int L, long slab_layer, hipStream_t st) {
  LBWN_REQUIRE(r.slab && r.nparts >= 1 && r.stride >= SLAB && L >= 1, "layer reduce: bad slab");
  RedK k;
  k.slab = r.slab; k.dsig = r.dsig; k.dgate = r.dgate; k.dres = r.dres;
  k.dbsig = r.dbsig; k.dbgate = r.dbgate; k.dbres = r.dbres;
  k.nparts = r.nparts; k.stride = r.stride; k.Cr = r.Cr; k.Cd = r.Cd;
  layer_reduce_all_kernel<<<dim3((SLAB + 31) / 32, L), 256, 0, st>>>(k, slab_layer, 2L * r.Cr * r.Cd,
                                                                    (long)r.Cd * r.Cr, r.Cd);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_slab_floats() { return SLAB; }

namespace {
// gtab[id][l·64 + c] += Σ over tiles with tile_gid == id (in tile order) of the tile's dv column
// sums slab[l][tile][5120 + c].  Block = (layer, id), thread = column: the block scans the tile ids
// 64 at a time (one per lane, ballot), then adds its matching tiles' partials in tile order
// (deterministic; blocks of ids with no uniform tile only scan).  Side stream beside dSKIP, where
// every dependent round trip is long: few VGPRs, 1,024 tile ids loaded at once (16 per lane) and
// the matching tiles listed in LDS in tile order, then their partials loaded 16 at a time (a
// ballot and a batch of 4 loads per 64 tiles ran 117 us at C4, one load per tile 154 us).
constexpr int GTS_CHUNK = 1024;
__global__ __launch_bounds__(64) void gc_tile_sum_kernel(const float* __restrict__ slab, long slab_layer, long tstride,
                                                         int ntiles, const int* __restrict__ tile_gid, float* gtab,
                                                         long ld) {
  __shared__ int lst[GTS_CHUNK];
  const int l = blockIdx.x, id = blockIdx.y, c = threadIdx.x;
  // the layer's partials through a buffer resource: a load's tile offset is one SGPR (the list
  // entry is wave-uniform), so a batch of 16 costs 16 VGPRs, not 16 64-bit addresses
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(slab + l * slab_layer), (short)0, (int)min(slab_layer * 4, 0x7fffffffL), BUF_DW3);
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int*>(tile_gid), (short)0, ntiles * 4, BUF_DW3);
  float acc = 0.f;
  bool any = false;
  for (int s0 = 0; s0 < ntiles; s0 += GTS_CHUNK) {
    int gid[GTS_CHUNK / 64];
#pragma unroll
    for (int k = 0; k < GTS_CHUNK / 64; ++k)   // past the end: 0 from the range-checked buffer offset, masked below
      gid[k] = (int)__builtin_amdgcn_raw_buffer_load_b32(rg, (s0 + c) * 4 + 256 * k, 0, 0);
    int n = 0;
#pragma unroll
    for (int k = 0; k < GTS_CHUNK / 64; ++k) {
      const int t = s0 + 64 * k + c;
      const bool hit = t < ntiles && gid[k] == id;
      const unsigned long long m = __ballot(hit);
      if (hit) lst[n + __popcll(m & ((1ull << c) - 1ull))] = t;
      n += __popcll(m);
    }
    any |= n > 0;
    __syncthreads();
    for (int i = 0; i < n; i += 16) {   // in tile order
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k)
        v[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            rs, c * 4, __builtin_amdgcn_readfirstlane(lst[min(i + k, n - 1)]) * (int)tstride * 4, 0));
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (i + k < n) acc += v[k];
    }
    __syncthreads();   // the list is rewritten by the next chunk
  }
  if (any) gtab[(long)id * ld + (long)l * 64 + c] += acc;
}
}  // namespace

int lbwn_gc_tile_sum_launch(const float* slab, int L, int ntiles, const int* tile_gid, float* gtab, long ld,
                            int ncat1, hipStream_t st) {
  LBWN_REQUIRE(ncat1 >= 1 && slab && tile_gid && gtab, "gc tile sums: bad arguments");
  // 32-bit byte offset of a tile's partial (the kernel's soffset)
  LBWN_REQUIRE((long)ntiles * SLAB * 4 < 0x7fffffffL, "gc tile sums: a layer's partials past 2 GiB");
  gc_tile_sum_kernel<<<dim3(L, ncat1), 64, 0, st>>>(slab + 5120, (long)ntiles * SLAB, SLAB, ntiles, tile_gid, gtab, ld);
  LBWN_CHECK_LAUNCH();
  return 0;
}
