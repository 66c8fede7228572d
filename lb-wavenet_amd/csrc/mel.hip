// Log-mel front end: wav -> log-mel rows in one launch.
//
// A block owns RT·32 consecutive frames of one stream.  It stages the frames' contiguous signal span
// ((rows-1)·hop + n_fft samples, reflection applied) into LDS once; frame i is then the LDS row that
// starts at sample i·hop.  Its eight waves walk the 32-bin column blocks of the spectrum: a wave forms
// re and im of its block as a product of the frames with the windowed DFT basis on the f32 matrix
// cores (v_mfma_f32_32x32x2_f32), squares them into the power block P [32 frames][32 bins], turns P
// round through a private LDS tile and multiplies it by the filterbank's 32 x n_mels slice into its
// own mel accumulators.  The waves' partial mel sums are added through LDS in wave order, so the
// result does not depend on scheduling.  Neither the spectrum nor P ever leaves the CU.
//
// LDS skew: sample p of the span sits at word p + p/hop.  Frame i, sample j is then word
// i·(hop+1) + j + j/hop; for a fixed j the 32 lanes of a half-wave (i = 0..31) read words that differ
// by multiples of hop+1, which is odd for every accepted hop, so they fall on 32 distinct banks.
#include "common.h"
#include "kernels.h"

#define MEL_WAVES 8
#define MEL_THREADS (MEL_WAVES * 64)
#define MEL_PSCR (32 * 33)   // a wave's P tile, rows padded to 33 words

LBWN_DEV void mel_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static inline int mel_sig_floats(const lbwn_mel_dims& d, int rows) {
  const long span = (long)(rows - 1) * d.hop + d.n_fft;
  return (int)((span + span / d.hop + 4) & ~3L);
}

size_t lbwn_mel_basis_floats(const lbwn_mel_dims& d) { return (size_t)d.ncb * d.n_fft * 64; }

size_t lbwn_mel_lds_bytes(const lbwn_mel_dims& d, int rows) {
  return ((size_t)mel_sig_floats(d, rows) + MEL_WAVES * MEL_PSCR + (size_t)rows * d.nt * 32) * sizeof(float);
}

// basis[cb][m][part][c][e]: sample j = 4m + e, bin k = 32cb + c, part 0 = w[j]·cos(2πjk/n_fft),
// part 1 = w[j]·sin(2πjk/n_fft).  The angle is reduced as the integer (j·k) mod n_fft; window, sine and
// cosine are taken in double and the product is rounded once.
__global__ __launch_bounds__(256) void mel_basis_kernel(lbwn_mel_dims d, float* basis, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int e = (int)(i & 3), c = (int)((i >> 2) & 31), part = (int)((i >> 7) & 1);
  const long mm = i >> 8;
  const int m = (int)(mm % (d.n_fft / 4)), cb = (int)(mm / (d.n_fft / 4));
  const int j = 4 * m + e, k = 32 * cb + c;
  const int jj = j - (d.n_fft - d.win) / 2;
  double v = 0.0;
  if (k < d.nbins && jj >= 0 && jj < d.win) {
    const double w = 0.5 - 0.5 * cospi(2.0 * (double)jj / (double)d.win);
    const long r = ((long)j * k) % d.n_fft;
    const double ang = 2.0 * (double)r / (double)d.n_fft;
    v = w * (part ? sinpi(ang) : cospi(ang));
  }
  basis[i] = (float)v;
}

int lbwn_mel_basis_launch(const lbwn_mel_dims& d, float* basis, hipStream_t st) {
  const long total = (long)lbwn_mel_basis_floats(d);
  mel_basis_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(d, basis, total);
  LBWN_CHECK_LAUNCH();
  return 0;
}

template <int RT, int NT>
__global__ __launch_bounds__(MEL_THREADS) void mel_fwd_kernel(lbwn_mel_dims d, const float* __restrict__ basis,
                                                               const float* __restrict__ fb,
                                                               const float* __restrict__ wav, long ld_wav, long n,
                                                               long frames, float* __restrict__ out, long ld_out) {
  extern __shared__ float lds[];
  constexpr int R = RT * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const int hop = d.hop, nfft = d.n_fft;
  const long t0 = (long)blockIdx.x * R;
  const float* x = wav + (long)blockIdx.y * ld_wav;
  const int span = (R - 1) * hop + nfft;
  const int sigf = (int)(((long)span + span / hop + 4) & ~3L);
  float* sig = lds;
  float* pscr = lds + sigf + wave * MEL_PSCR;
  float* melb = lds + sigf + MEL_WAVES * MEL_PSCR;

  // the tile's signal span, reflected once at either end; rows past the last frame read zeros
  const long g0 = t0 * hop - nfft / 2;
  for (int p = tid; p < span; p += MEL_THREADS) {
    long g = g0 + p;
    if (g < 0) g = -g;
    else if (g >= n) g = 2 * (n - 1) - g;
    const float v = (g >= 0 && g < n) ? x[g] : 0.0f;
    sig[p + p / hop] = v;
  }
  __syncthreads();

  floatx16 mel[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) mel[rt][nt][r] = 0.0f;

  const int nch = nfft / 8;   // 8 samples per chunk: half-wave h takes samples 8ch + 4h .. + 3
  const int rowbase = c * (hop + 1);
  // bins of weight zero in every band (always bin 0 and the Nyquist bin, since 0 <= fmin and fmax <=
  // sample_rate/2; more with a narrower band) add nothing: column blocks made of them alone are skipped
  for (int cb = d.cb_lo + wave; cb < d.cb_hi; cb += MEL_WAVES) {
    floatx16 re[RT], im[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { re[rt][r] = 0.0f; im[rt][r] = 0.0f; }
    const floatx4* bp = reinterpret_cast<const floatx4*>(basis) + (long)cb * (nfft / 4) * 64 + c;
    auto ldb = [&](int ch, floatx4& co, floatx4& si) {
      const int m = 2 * (ch < nch ? ch : nch - 1) + h;
      co = bp[m * 64];
      si = bp[m * 64 + 32];
    };
    auto step = [&](int ch, const floatx4& co, const floatx4& si) {
      const int j = 8 * ch + 4 * h;
      const float* ap = sig + rowbase + j + j / hop;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float* a = ap + rt * 32 * (hop + 1);
        const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
        re[rt] = mfma32(a0, co[0], re[rt]); im[rt] = mfma32(a0, si[0], im[rt]);
        re[rt] = mfma32(a1, co[1], re[rt]); im[rt] = mfma32(a1, si[1], im[rt]);
        re[rt] = mfma32(a2, co[2], re[rt]); im[rt] = mfma32(a2, si[2], im[rt]);
        re[rt] = mfma32(a3, co[3], re[rt]); im[rt] = mfma32(a3, si[3], im[rt]);
      }
    };
    // basis operands two chunks ahead of the products (nch is a multiple of 4)
    floatx4 c0, s0, c1, s1, cn, sn;
    ldb(0, c0, s0);
    ldb(1, c1, s1);
    for (int ch = 0; ch < nch; ch += 2) {
      ldb(ch + 2, cn, sn);
      step(ch, c0, s0);
      c0 = cn; s0 = sn;
      ldb(ch + 3, cn, sn);
      step(ch + 1, c1, s1);
      c1 = cn; s1 = sn;
    }
    // P = |X|^power, turned from the accumulator layout (lane = bin) to the A operand's (lane = frame)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = re[rt][r] * re[rt][r] + im[rt][r] * im[rt][r];
        if (d.power == 1) p = sqrtf(p);
        pscr[acc_row(r, h) * 33 + c] = p;
      }
      mel_wave_sync();
      const float* fp = fb + (long)(cb * 32 + h) * (NT * 32) + c;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const float a = pscr[c * 33 + 2 * kk + h];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          mel[rt][nt] = mfma32(a, fp[(long)(2 * kk) * (NT * 32) + nt * 32], mel[rt][nt]);
      }
      mel_wave_sync();
    }
  }

  // the waves' partial sums, added in wave order
  for (int w = 0; w < MEL_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int idx = (rt * 32 + acc_row(r, h)) * (NT * 32) + nt * 32 + c;
            melb[idx] = (w == 0 ? 0.0f : melb[idx]) + mel[rt][nt][r];
          }
    }
    __syncthreads();
  }

  const int nm = d.n_mels;
  float* o = out + (long)blockIdx.y * ld_out;
  for (int e = tid; e < R * nm; e += MEL_THREADS) {
    const int row = e / nm, band = e - row * nm;
    const long t = t0 + row;
    if (t >= frames) break;
    float v = melb[row * (NT * 32) + band];
    if (d.log_floor > 0.0f) v = logf(fmaxf(v, d.log_floor));
    o[t * nm + band] = v;
  }
}

// prepare: raise the instantiation's dynamic-LDS limit on the current device (lbwn_mel_init; nothing is
// launched), so that the forward is the launch alone.
template <int RT, int NT>
static int mel_fwd_go(bool prepare, const lbwn_mel_dims& d, const float* basis, const float* fb, const float* wav,
                      long ld_wav, int batch, long n, long frames, float* out, long ld_out, hipStream_t st) {
  const size_t lds = lbwn_mel_lds_bytes(d, RT * 32);
  if (prepare) {
    if (lds > 65536)
      LBWN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mel_fwd_kernel<RT, NT>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
  }
  const long tiles = (frames + RT * 32 - 1) / (RT * 32);
  mel_fwd_kernel<RT, NT><<<dim3((unsigned)tiles, (unsigned)batch), dim3(MEL_THREADS), lds, st>>>(
      d, basis, fb, wav, ld_wav, n, frames, out, ld_out);
  LBWN_CHECK_LAUNCH();
  return 0;
}

static int mel_dispatch(bool prepare, const lbwn_mel_dims& d, const float* basis, const float* fb, const float* wav,
                        long ld_wav, int batch, long n, long frames, float* out, long ld_out, hipStream_t st) {
#define MEL_GO(RT, NT) \
  return mel_fwd_go<RT, NT>(prepare, d, basis, fb, wav, ld_wav, batch, n, frames, out, ld_out, st)
  if (d.rows == 64) {
    switch (d.nt) {
      case 1: MEL_GO(2, 1);
      case 2: MEL_GO(2, 2);
      case 3: MEL_GO(2, 3);
      case 4: MEL_GO(2, 4);
    }
  } else if (d.rows == 32) {
    switch (d.nt) {
      case 1: MEL_GO(1, 1);
      case 2: MEL_GO(1, 2);
      case 3: MEL_GO(1, 3);
      case 4: MEL_GO(1, 4);
    }
  }
#undef MEL_GO
  LBWN_REQUIRE(false, "mel_forward: no kernel for %d rows x %d band tiles", d.rows, d.nt);
}

int lbwn_mel_fwd_prepare(const lbwn_mel_dims& d) {
  return mel_dispatch(true, d, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr, 0, nullptr);
}

int lbwn_mel_fwd_launch(const lbwn_mel_dims& d, const float* basis, const float* fb, const float* wav, long ld_wav,
                        int batch, long n, long frames, float* out, long ld_out, hipStream_t st) {
  return mel_dispatch(false, d, basis, fb, wav, ld_wav, batch, n, frames, out, ld_out, st);
}
