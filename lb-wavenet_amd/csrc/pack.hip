// Weight-image packers of the layer kernels and chains (the layouts are in layer_common.h), and
// the training step's fused start-of-step launch (step_prologue_kernel), which packs both chains'
// images beside the other start-of-step jobs (prologue.h).
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "layer_common.h"
#include "prologue.h"

namespace {

// ---- weight packing ---------------------------------------------------------------------
// image: Ws[k = tap*32 + in][out (sig 0..31 | gate 32..63)] (row WS), Rs[c][o] (row XS),
//        bs[64] (sig | gate), br[32]

__global__ void pack_layers_kernel(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                                   const float* res, const float* res_b, float* out, int Cr, int Cd) {
  const int l = blockIdx.x;
  const float* ws = sig + (long)l * 2 * Cr * Cd;
  const float* wg = gate + (long)l * 2 * Cr * Cd;
  const float* wr = res + (long)l * Cd * Cr;
  float* img = out + (long)l * WIMG;
  for (int e = threadIdx.x; e < 64 * WS; e += blockDim.x) {
    const int k = e / WS, o = e % WS;
    const int tap = k >> 5, in = k & 31, oc = o & 31;
    float v = 0.f;
    if (o < 64 && in < Cr && oc < Cd) v = (o < 32 ? ws : wg)[(tap * Cr + in) * Cd + oc];
    img[e] = v;
  }
  for (int e = threadIdx.x; e < 32 * XS; e += blockDim.x) {
    const int c = e / XS, o = e % XS;
    img[64 * WS + e] = (c < Cd && o < Cr) ? wr[c * Cr + o] : 0.f;
  }
  if (threadIdx.x < 96) {
    const int i = threadIdx.x;
    float v = 0.f;
    if (i < 64) {
      const float* bb = i < 32 ? sig_b : gate_b;
      if (bb && (i & 31) < Cd) v = bb[(long)l * Cd + (i & 31)];
    } else if (res_b && i - 64 < Cr) {
      v = res_b[(long)l * Cr + (i - 64)];
    }
    img[64 * WS + 32 * XS + i] = v;
  }
}

LBWN_DEV void pack_lc_x3_body(int l, const float* lsig, const float* lgate, unsigned short* out, int Lo, int Cd) {
  unsigned short* img = out + (long)l * LCIMG_US;
  for (int e = threadIdx.x; e < 64 * (LC_ROW / 2); e += blockDim.x) {
    const int o = e / (LC_ROW / 2), kk = 2 * (e % (LC_ROW / 2));
    unsigned short* row = img + o * LC_ROW;
    if (kk >= LC_KP) {   // pad columns (never read) and the plane slots past k: written as part of planes below
      if (kk >= 3 * LC_KP) *(unsigned*)(row + kk) = 0u;
      continue;
    }
    const float* w = (o < 32 ? lsig : lgate) + (long)l * Lo * Cd;
    const int oc = o & 31;
    floatx2 x = {0.f, 0.f};
    if (oc < Cd) {
      if (kk < Lo) x[0] = w[(long)kk * Cd + oc];
      if (kk + 1 < Lo) x[1] = w[(long)(kk + 1) * Cd + oc];
    }
    unsigned hi, mi, lo;
    split2(x, hi, mi, lo);
    *(unsigned*)(row + kk) = hi;
    *(unsigned*)(row + LC_KP + kk) = mi;
    *(unsigned*)(row + 2 * LC_KP + kk) = lo;
  }
}

LBWN_DEV void pack_x3_body(int l, const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                          const float* res, const float* res_b, unsigned short* out, int Cr, int Cd) {
  const float* ws = sig + (long)l * 2 * Cr * Cd;
  const float* wg = gate + (long)l * 2 * Cr * Cd;
  const float* wr = res + (long)l * Cd * Cr;
  unsigned short* img = out + (long)l * XIMG_US;
  // WT: pairs of consecutive input channels
  for (int e = threadIdx.x; e < 64 * 2 * 16; e += blockDim.x) {
    const int o = e >> 5, tap = (e >> 4) & 1, in = 2 * (e & 15), oc = o & 31;
    const float* w = o < 32 ? ws : wg;
    floatx2 x = {0.f, 0.f};
    if (oc < Cd) {
      if (in < Cr) x[0] = w[(tap * Cr + in) * Cd + oc];
      if (in + 1 < Cr) x[1] = w[(tap * Cr + in + 1) * Cd + oc];
    }
    unsigned h, m, lo;
    split2(x, h, m, lo);
    unsigned short* row = img + o * XW_ROW + tap * 96 + in;
    *(unsigned*)(row) = h;
    *(unsigned*)(row + 32) = m;
    *(unsigned*)(row + 64) = lo;
  }
  // RT: kk pairs (kk, kk+1) hold z channels c, c+1 (same j>>2 group)
  for (int e = threadIdx.x; e < 32 * 16; e += blockDim.x) {
    const int o = e >> 4, kk = 2 * (e & 15);
    const int s2 = kk >> 4, hh = (kk >> 3) & 1, j = kk & 7;
    const int c = 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3);
    floatx2 x = {0.f, 0.f};
    if (o < Cr) {
      if (c < Cd) x[0] = wr[c * Cr + o];
      if (c + 1 < Cd) x[1] = wr[(c + 1) * Cr + o];
    }
    unsigned h, m, lo;
    split2(x, h, m, lo);
    unsigned short* row = img + 64 * XW_ROW + o * XR_ROW + kk;
    *(unsigned*)(row) = h;
    *(unsigned*)(row + 32) = m;
    *(unsigned*)(row + 64) = lo;
  }
  if (threadIdx.x < 96) {
    const int i = threadIdx.x;
    float v = 0.f;
    if (i < 64) {
      const float* bb = i < 32 ? sig_b : gate_b;
      if (bb && (i & 31) < Cd) v = bb[(long)l * Cd + (i & 31)];
    } else if (res_b && i - 64 < Cr) {
      v = res_b[(long)l * Cr + (i - 64)];
    }
    ((float*)(img + XB_OFF))[i] = v;
  }
}

LBWN_DEV void pack_lc16_body(int l, const float* lsig, const float* lgate, unsigned short* out, int Lo, int Cd) {
  unsigned short* img = out + (long)l * LC16IMG_US;
  for (int e = threadIdx.x; e < 64 * (LC16_ROW / 2); e += blockDim.x) {
    const int o = e / (LC16_ROW / 2), kk = 2 * (e % (LC16_ROW / 2));
    unsigned short* row = img + o * LC16_ROW;
    if (kk >= LC16_KP) {   // row pad (zero); plane slots are written below
      if (kk >= 3 * LC16_KP) *(unsigned*)(row + kk) = 0u;
      continue;
    }
    const float* w = (o < 32 ? lsig : lgate) + (long)l * Lo * Cd;
    const int oc = o & 31;
    floatx2 x = {0.f, 0.f};
    if (oc < Cd) {
      if (kk < Lo) x[0] = w[(long)kk * Cd + oc];
      if (kk + 1 < Lo) x[1] = w[(long)(kk + 1) * Cd + oc];
    }
    unsigned hi, mi, lo;
    split2(x, hi, mi, lo);
    *(unsigned*)(row + kk) = hi;
    *(unsigned*)(row + LC16_KP + kk) = mi;
    *(unsigned*)(row + 2 * LC16_KP + kk) = lo;
  }
}

LBWN_DEV void pack_bx3_body(int l, const float* sig, const float* gate, const float* res, float* out, int Cr, int Cd) {
  const float* ws = sig + (long)l * 2 * Cr * Cd;
  const float* wg = gate + (long)l * 2 * Cr * Cd;
  const float* wr = res + (long)l * Cd * Cr;
  float* img = out + (long)l * BIMG_F;
  unsigned short* wd = (unsigned short*)img;
  for (int e = threadIdx.x; e < 2 * 32 * 32; e += blockDim.x) {
    const int tap = e >> 10, in = (e >> 5) & 31, kk = 2 * (e & 31);
    floatx2 x = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k2 = kk + u, s2 = k2 >> 4, hh = (k2 >> 3) & 1, j = k2 & 7;
      const int o = 32 * (s2 >> 1) + 16 * (s2 & 1) + 8 * (j >> 2) + 4 * hh + (j & 3), oc = o & 31;
      const float* wk = o < 32 ? ws : wg;
      if (in < Cr && oc < Cd) x[u] = wk[(tap * Cr + in) * Cd + oc];
    }
    unsigned hi, mi, lo;
    split2(x, hi, mi, lo);
    unsigned short* row = wd + (tap * 32 + in) * XW_ROW + kk;
    *(unsigned*)(row) = hi;
    *(unsigned*)(row + 64) = mi;
    *(unsigned*)(row + 128) = lo;
  }
  float* rs = img + BD_US / 2;
  for (int e = threadIdx.x; e < 32 * XS; e += blockDim.x) {
    const int c = e / XS, o = e % XS;
    rs[e] = (c < Cd && o < Cr) ? wr[c * Cr + o] : 0.f;
  }
  for (int e = BD_US / 2 + 32 * XS + threadIdx.x; e < BX_F; e += blockDim.x) img[e] = 0.f;
  unsigned short* rx = (unsigned short*)(img + BX_F);
  for (int e = threadIdx.x; e < 32 * 16; e += blockDim.x) {
    const int c = e >> 4, kk = 2 * (e & 15);
    floatx2 x = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k2 = kk + u, gg = k2 >> 3, ee = k2 & 7, o = 16 * (ee >> 2) + 4 * gg + (ee & 3);
      if (c < Cd && o < Cr) x[u] = wr[c * Cr + o];
    }
    unsigned hi, mi, lo;
    split2(x, hi, mi, lo);
    unsigned short* row = rx + c * RX_ROW + kk;
    *(unsigned*)(row) = hi;
    *(unsigned*)(row + 32) = mi;
    *(unsigned*)(row + 64) = lo;
  }
}

// both chains' images in one launch (blocks [0, L): forward, [L, 2L): backward), and in the
// blocks after them (if skip_b) the skip GEMM's bias Σ_l skip_b[l] (l in order)
LBWN_DEV void pack_fb_x3_block(int l, const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                               const float* res, const float* res_b, unsigned short* fout, float* bout, int L, int Cr,
                               int Cd, const float* skip_b, int Cs, float* bsum, const float* lc_sig,
                               const float* lc_gate, int Lo, unsigned short* lcout, int lc16) {
  const int nlc = lcout ? L : 0;
  if (l < L) {
    pack_x3_body(l, sig, gate, sig_b, gate_b, res, res_b, fout, Cr, Cd);
  } else if (l < 2 * L) {
    pack_bx3_body(l - L, sig, gate, res, bout, Cr, Cd);
  } else if (l < 2 * L + nlc) {
    if (lc16) pack_lc16_body(l - 2 * L, lc_sig, lc_gate, lcout, Lo, Cd);
    else pack_lc_x3_body(l - 2 * L, lc_sig, lc_gate, lcout, Lo, Cd);
  } else {
    const int n = (l - 2 * L - nlc) * 256 + threadIdx.x;
    if (n < Cs) {
      float s = 0.f;
#pragma unroll 10
      for (int k = 0; k < L; ++k) s += skip_b[(long)k * Cs + n];
      bsum[n] = s;
    }
  }
}
__global__ __launch_bounds__(256) void pack_layers_fb_x3_kernel(const float* sig, const float* gate,
                                                                const float* sig_b, const float* gate_b,
                                                                const float* res, const float* res_b,
                                                                unsigned short* fout, float* bout, int L, int Cr,
                                                                int Cd, const float* skip_b, int Cs, float* bsum,
                                                                const float* lc_sig, const float* lc_gate, int Lo,
                                                                unsigned short* lcout, int lc16) {
  pack_fb_x3_block(blockIdx.x, sig, gate, sig_b, gate_b, res, res_b, fout, bout, L, Cr, Cd, skip_b, Cs, bsum, lc_sig,
                   lc_gate, Lo, lcout, lc16);
}

// The step's start-of-step work in ONE launch (lbwn_step_prologue_launch): zero the status word and
// hand-off flags, pre-split the skip/head weight planes, gather the PRE embedding, prepend the
// D-sep state, and pack both chains' images -- five independent jobs that ran as five dependent
// launches of 7-12 us each (profiles/r04_v1_step_timeline.txt).  Block ranges, heavy jobs first.
struct PrologueK {
  lbwn_prologue_args a;
  SplitJobs jb;
  int nz, ns, ne, nd, np;   // blocks: zero, split (per job), embed, D-sep (all layers), pack
  int nl;                   // 1: block 0 forms the masked-position live lists (one block, the longest)
  bool ev4, dv4;            // float4 items: embed, D-sep
};
__global__ __launch_bounds__(256) void step_prologue_kernel(PrologueK k) {
  const lbwn_prologue_args& a = k.a;
  long b = blockIdx.x;
  if (b < k.nl) {
    live_lists_body(a.ids, a.B, a.T, a.tlive, a.klive, a.nklive, a.kpre);
    return;
  }
  b -= k.nl;
  if (b < (long)k.ns * a.njobs) {
    split_planes_body(k.jb, (int)(b / k.ns), b % k.ns, k.ns);
    return;
  }
  b -= (long)k.ns * a.njobs;
  if (b < k.ne) {
    embed_flat_body(b, k.ne, a.q, a.pre, a.pre_b, a.X, a.B, a.T, a.H, a.Cr, a.Q, k.ev4);
    return;
  }
  b -= k.ne;
  if (b < k.nd) {
    dsep_flat_body<true>(b, k.nd, a.X, a.xls, const_cast<float*>(a.save), a.L, a.nbl, a.B, a.T, a.H, a.Cr, k.dv4);
    return;
  }
  b -= k.nd;
  if (b < k.nz) {
    zero_body(b, k.nz, (unsigned*)a.zero, (long)(a.zero_bytes / 4));
    return;
  }
  b -= k.nz;
  pack_fb_x3_block((int)b, a.sig, a.gate, a.sig_b, a.gate_b, a.res, a.res_b, a.fout, a.bout, a.L, a.Cr, a.Cd,
                   a.skip_b, a.Cs, a.bsum, a.lc_sig, a.lc_gate, a.Lo, a.lcout, a.lc16);
}

}  // namespace

int lbwn_layer_image_floats() { return WIMG; }
int lbwn_layer_image_x3_elems() { return XIMG_US; }
int lbwn_lc_image_x3_elems() { return LCIMG_US; }
int lbwn_lc_image16_elems() { return LC16IMG_US; }
int lbwn_lc_in_chain_ok(int Lo) { return Lo > 16 * (LC_K - 1) && Lo <= LC_KP && Lo % 4 == 0; }
int lbwn_layer_image_bx3_floats() { return BIMG_F; }

int lbwn_pack_layers_launch(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                            const float* res, const float* res_b, float* out, int L, int Cr, int Cd, hipStream_t st) {
  pack_layers_kernel<<<L, 256, 0, st>>>(sig, gate, sig_b, gate_b, res, res_b, out, Cr, Cd);
  LBWN_CHECK_LAUNCH();
  return 0;
}

int lbwn_pack_layers_fb_x3_launch(const float* sig, const float* gate, const float* sig_b, const float* gate_b,
                                  const float* res, const float* res_b, unsigned short* fout, float* bout, int L,
                                  int Cr, int Cd, const float* skip_b, int Cs, float* bsum, const float* lc_sig,
                                  const float* lc_gate, int Lo, unsigned short* lcout, hipStream_t st, int lc16) {
  LBWN_REQUIRE(Cr <= 32 && Cd <= 32 && (((uintptr_t)fout) & 15) == 0 && (((uintptr_t)bout) & 15) == 0,
               "pack_layers_fb_x3: bad arguments");
  LBWN_REQUIRE(!lcout || (lc_sig && lc_gate && Lo >= 1 && Lo <= LC_KP && (((uintptr_t)lcout) & 15) == 0),
               "pack_layers_fb_x3: bad LC image arguments");
  const int nsum = (skip_b && bsum) ? (Cs + 255) / 256 : 0;
  const int nlc = lcout ? L : 0;
  pack_layers_fb_x3_kernel<<<2 * L + nlc + nsum, 256, 0, st>>>(sig, gate, sig_b, gate_b, res, res_b, fout, bout, L, Cr,
                                                               Cd, skip_b, Cs, bsum, lc_sig, lc_gate, Lo, lcout,
                                                               lc16);
  LBWN_CHECK_LAUNCH();
  return 0;
}
int lbwn_step_prologue_launch(const lbwn_prologue_args& a, hipStream_t st) {
  LBWN_REQUIRE(a.Cr <= 32 && a.Cd <= 32 && (((uintptr_t)a.fout) & 15) == 0 && (((uintptr_t)a.bout) & 15) == 0,
               "step_prologue: bad pack arguments");
  LBWN_REQUIRE(!a.lcout || (a.lc_sig && a.lc_gate && a.Lo >= 1 && a.Lo <= LC_KP && (((uintptr_t)a.lcout) & 15) == 0),
               "step_prologue: bad LC image arguments");
  LBWN_REQUIRE(a.njobs >= 0 && a.njobs <= 6 && a.zero_bytes % 4 == 0 && a.q && a.pre && a.X && a.save,
               "step_prologue: bad arguments");
  PrologueK k;
  memset(&k, 0, sizeof(k));
  k.a = a;
  long most = 0;
  for (int j = 0; j < a.njobs; ++j) {
    LBWN_REQUIRE(a.W[j] && a.out[j] && a.rows[j] > 0 && a.K[j] > 0, "step_prologue: bad split job");
    k.jb.W[j] = a.W[j]; k.jb.ldw[j] = a.ldw[j]; k.jb.rows[j] = a.rows[j]; k.jb.K[j] = a.K[j];
    k.jb.trans[j] = a.trans[j]; k.jb.out[j] = a.out[j];
    most = std::max(most, (long)a.rows[j] * ((a.K[j] + PLANE_BK - 1) / PLANE_BK) * (PLANE_BK / 2));
  }
  auto blocks = [](long n, long per, long cap) { return (int)std::max(1L, std::min(cap, (n + per - 1) / per)); };
  k.ns = blocks(most, 1024, 256);                                        // 4 pairs per thread
  LBWN_REQUIRE((long)a.B * a.T * a.Cr < (1L << 31) && (long)dsep_rows(a.L, a.nbl, 1) * a.B * a.Cr < (1L << 31),
               "step_prologue: x / SAVE exceed 32-bit indexing");
  k.ev4 = embed_v4(a.pre, a.pre_b, a.X, a.Cr);
  k.dv4 = dsep_v4(a.X, a.xls, a.save, a.Cr);
  k.ne = blocks((long)a.B * a.T * (k.ev4 ? a.Cr / 4 : a.Cr), 256, 2048);   // one item per thread
  k.nd = blocks((long)dsep_rows(a.L, a.nbl, a.B) * (k.dv4 ? a.Cr / 4 : a.Cr), 256, 2048);
  k.nz = a.zero_bytes ? blocks((long)(a.zero_bytes / 4), 1024, 256) : 0;
  k.np = 2 * a.L + (a.lcout ? a.L : 0) + ((a.skip_b && a.bsum) ? (a.Cs + 255) / 256 : 0);
  LBWN_REQUIRE(!a.ids || (a.tlive && a.klive && a.nklive && a.kpre), "step_prologue: bad live-list arguments");
  k.nl = a.ids ? 1 : 0;
  const long grid = (long)k.nl + (long)k.ns * a.njobs + k.ne + k.nd + k.nz + k.np;
  step_prologue_kernel<<<(unsigned)grid, 256, 0, st>>>(k);
  LBWN_CHECK_LAUNCH();
  return 0;
}
