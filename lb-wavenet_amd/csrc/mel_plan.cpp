// Log-mel front end: plan (host-only: configuration checks, filterbank) and C entry points
// (include/lbwn.h, "log-mel front end"; kernels in mel.hip).
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/lbwn.h"
#include "common.h"
#include "kernels.h"

struct lbwn_mel_plan {
  lbwn_mel_cfg cfg;
  lbwn_mel_dims d;
  std::vector<float> fb;       // [nbins][n_mels], what lbwn_mel_filterbank returns
  std::vector<float> fb_pad;   // [ncb*32][nt*32], the device image
  size_t basis_bytes, fb_bytes;
};

static const size_t MEL_LDS_LIMIT = 160 * 1024;   // per workgroup on gfx950

static double mel_hz_to_mel(double f, int htk) {
  if (htk) return 2595.0 * log10(1.0 + f / 700.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}

static double mel_mel_to_hz(double m, int htk) {
  if (htk) return 700.0 * (pow(10.0, m / 2595.0) - 1.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

static size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" {

int lbwn_mel_plan_create(const lbwn_mel_cfg* cfg, lbwn_mel_plan** out) {
  LBWN_REQUIRE(cfg != nullptr && out != nullptr, "mel_plan_create: null argument");
  LBWN_REQUIRE(cfg->struct_size == sizeof(lbwn_mel_cfg), "mel_plan_create: struct_size %zu != %zu (another ABI?)",
               cfg->struct_size, sizeof(lbwn_mel_cfg));
  const lbwn_mel_cfg& c = *cfg;
  LBWN_REQUIRE(c.sample_rate >= 1, "mel_plan_create: sample_rate must be >= 1, got %d", c.sample_rate);
  LBWN_REQUIRE(c.n_fft >= 64 && c.n_fft <= 2048 && c.n_fft % 32 == 0,
               "mel_plan_create: n_fft must be a multiple of 32 in [64, 2048], got %d", c.n_fft);
  LBWN_REQUIRE(c.hop >= 4 && c.hop <= c.n_fft && c.hop % 4 == 0,
               "mel_plan_create: hop must be a multiple of 4 in [4, n_fft], got %d", c.hop);
  LBWN_REQUIRE(c.win_length >= 2 && c.win_length <= c.n_fft,
               "mel_plan_create: win_length must be in [2, n_fft], got %d", c.win_length);
  LBWN_REQUIRE(c.n_mels >= 4 && c.n_mels <= 128 && c.n_mels % 4 == 0,
               "mel_plan_create: n_mels must be a multiple of 4 in [4, 128], got %d", c.n_mels);
  LBWN_REQUIRE(c.fmin >= 0.f && c.fmin < c.fmax, "mel_plan_create: fmin must satisfy 0 <= fmin < fmax, got %g (fmax %g)",
               (double)c.fmin, (double)c.fmax);
  LBWN_REQUIRE(c.fmax <= 0.5f * (float)c.sample_rate, "mel_plan_create: fmax must be <= sample_rate/2, got %g",
               (double)c.fmax);
  LBWN_REQUIRE(c.power == 1 || c.power == 2, "mel_plan_create: power must be 1 or 2, got %d", c.power);
  LBWN_REQUIRE(c.log_floor >= 0.f && c.log_floor <= 3.402823466e38f,
               "mel_plan_create: log_floor must be finite and >= 0, got %g", (double)c.log_floor);

  lbwn_mel_plan* p = new lbwn_mel_plan;
  p->cfg = c;
  lbwn_mel_dims& d = p->d;
  d.n_fft = c.n_fft; d.win = c.win_length; d.hop = c.hop; d.n_mels = c.n_mels; d.power = c.power;
  d.nbins = c.n_fft / 2 + 1; d.ncb = (d.nbins + 31) / 32; d.nt = (c.n_mels + 31) / 32;
  d.log_floor = c.log_floor;
  d.rows = lbwn_mel_lds_bytes(d, 64) <= MEL_LDS_LIMIT ? 64 : lbwn_mel_lds_bytes(d, 32) <= MEL_LDS_LIMIT ? 32 : 0;
  if (!d.rows) {
    const size_t need = lbwn_mel_lds_bytes(d, 32);
    delete p;
    LBWN_REQUIRE(false, "mel_plan_create: n_fft %d with hop %d needs %zu bytes of LDS for a 32-frame tile, the device "
                 "has %zu", c.n_fft, c.hop, need, MEL_LDS_LIMIT);
  }

  // triangles over n_mels + 2 points equally spaced on the mel scale, in double, rounded once
  const int nm = c.n_mels, htk = c.htk ? 1 : 0;
  std::vector<double> pts(nm + 2);
  const double m_lo = mel_hz_to_mel((double)c.fmin, htk), m_hi = mel_hz_to_mel((double)c.fmax, htk);
  for (int i = 0; i < nm + 2; ++i) pts[i] = mel_mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(nm + 1), htk);
  p->fb.assign((size_t)d.nbins * nm, 0.f);
  p->fb_pad.assign((size_t)d.ncb * 32 * d.nt * 32, 0.f);
  for (int j = 0; j < nm; ++j) {
    const double lo = pts[j], ce = pts[j + 1], hi = pts[j + 2];
    const double scale = c.norm ? 2.0 / (hi - lo) : 1.0;
    bool any = false;
    for (int k = 0; k < d.nbins; ++k) {
      const double f = (double)k * (double)c.sample_rate / (double)c.n_fft;
      const double w = fmax(0.0, fmin((f - lo) / (ce - lo), (hi - f) / (hi - ce))) * scale;
      const float wf = (float)w;
      p->fb[(size_t)k * nm + j] = wf;
      p->fb_pad[(size_t)k * d.nt * 32 + j] = wf;
      any = any || wf != 0.f;
    }
    if (!any) {
      delete p;
      LBWN_REQUIRE(false, "mel_plan_create: band %d of n_mels %d (%g..%g Hz) holds no bin of n_fft %d at sample_rate "
                   "%d: an empty filter", j, nm, lo, hi, c.n_fft, c.sample_rate);
    }
  }
  d.cb_lo = d.ncb; d.cb_hi = 0;
  for (int k = 0; k < d.nbins; ++k)
    for (int j = 0; j < nm; ++j)
      if (p->fb[(size_t)k * nm + j] != 0.f) {
        if (k / 32 < d.cb_lo) d.cb_lo = k / 32;
        if (k / 32 + 1 > d.cb_hi) d.cb_hi = k / 32 + 1;
        break;
      }
  p->basis_bytes = round256(lbwn_mel_basis_floats(d) * sizeof(float));
  p->fb_bytes = round256(p->fb_pad.size() * sizeof(float));
  *out = p;
  return 0;
}

void lbwn_mel_plan_destroy(lbwn_mel_plan* plan) { delete plan; }

int64_t lbwn_mel_frames(const lbwn_mel_plan* plan, int64_t n_samples) {
  if (!plan || n_samples <= plan->cfg.n_fft / 2) return 0;
  return n_samples / plan->cfg.hop;
}

size_t lbwn_mel_workspace_bytes(const lbwn_mel_plan* plan) { return plan ? plan->basis_bytes + plan->fb_bytes : 0; }

int lbwn_mel_filterbank(const lbwn_mel_plan* plan, float* host_out) {
  LBWN_REQUIRE(plan != nullptr && host_out != nullptr, "mel_filterbank: null argument");
  memcpy(host_out, plan->fb.data(), plan->fb.size() * sizeof(float));
  return 0;
}

int lbwn_mel_init(const lbwn_mel_plan* plan, void* workspace, void* stream) {
  LBWN_REQUIRE(plan != nullptr && workspace != nullptr, "mel_init: null argument");
  LBWN_REQUIRE(((uintptr_t)workspace & 255) == 0, "mel_init: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int e = lbwn_mel_fwd_prepare(plan->d);   // the forward kernel's LDS limit, here so that the forward is one launch
  if (e) return e;
  e = lbwn_mel_basis_launch(plan->d, (float*)workspace, st);
  if (e) return e;
  LBWN_HIP(hipMemcpyAsync((char*)workspace + plan->basis_bytes, plan->fb_pad.data(),
                          plan->fb_pad.size() * sizeof(float), hipMemcpyHostToDevice, st));
  return 0;
}

int lbwn_mel_forward(const lbwn_mel_plan* plan, const void* workspace, const float* wav, int64_t ld_wav, int batch,
                     int64_t n_samples, float* out, int64_t ld_out_stream, void* stream) {
  LBWN_REQUIRE(plan != nullptr && workspace != nullptr && wav != nullptr && out != nullptr,
               "mel_forward: null argument");
  LBWN_REQUIRE(((uintptr_t)workspace & 255) == 0, "mel_forward: workspace must be 256-byte aligned");
  LBWN_REQUIRE(((uintptr_t)wav & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "mel_forward: wav and out must be 16-byte aligned");
  LBWN_REQUIRE(batch >= 1 && batch <= 65535, "mel_forward: batch must be in [1, 65535], got %d", batch);
  const int64_t F = lbwn_mel_frames(plan, n_samples);
  LBWN_REQUIRE(F >= 1, "mel_forward: n_samples %lld gives no frame (needs n_samples > n_fft/2 = %d and >= hop = %d)",
               (long long)n_samples, plan->cfg.n_fft / 2, plan->cfg.hop);
  LBWN_REQUIRE((F + plan->d.rows - 1) / plan->d.rows < (1LL << 31), "mel_forward: n_samples %lld is too long",
               (long long)n_samples);
  LBWN_REQUIRE(ld_wav % 4 == 0 && ld_wav >= 0 && (batch == 1 || ld_wav >= n_samples),
               "mel_forward: ld_wav must be a multiple of 4 and >= n_samples, got %lld", (long long)ld_wav);
  LBWN_REQUIRE(batch == 1 || ld_out_stream >= F * plan->cfg.n_mels,
               "mel_forward: ld_out_stream must be >= frames * n_mels = %lld, got %lld",
               (long long)(F * plan->cfg.n_mels), (long long)ld_out_stream);
  const float* basis = (const float*)workspace;
  const float* fb = (const float*)((const char*)workspace + plan->basis_bytes);
  return lbwn_mel_fwd_launch(plan->d, basis, fb, wav, (long)ld_wav, batch, (long)n_samples, (long)F, out,
                             (long)ld_out_stream, (hipStream_t)stream);
}

}  // extern "C"
