// Magnitude terms of auraloss STFTLoss beyond the multi_stft.yaml configuration: the optional mel projection (scale="mel") and the
// weighted spectral-convergence / log-magnitude / linear-magnitude terms under an L1 or L2 distance.  The default configuration
// (SC + L1 log, no scale) keeps stft.hip's stft_sums_kernel / stft_bwd_kernel / stft_total_kernel; these run every other one.
//
// The spectrum is the flat (2*bins, cols) windowed-DFT output of StftPlan.dft: bin k of column c at k*cols + c (imaginary part at
// + bins*cols), cols = 2*rows*frames, x rows in columns [0, rows*frames), y rows after them; column r*frames + f is frame f of row r.
// M = sqrt(clamp(re^2 + im^2, eps)) per bin; with the mel projection M'[m] = sum_k F[m, k] M[k] over filter m's one contiguous bin
// range (a Slaney filterbank: each bin in at most two filters), gathered in the same pass that reads the spectrum -- ~2*bins
// magnitudes per column instead of a dense (n_mels x bins) product.
//
//   stft_terms_fwd_kernel    STFT_TERMS_SPLIT blocks per row: per-row partial sums s0 = sum (M'y - M'x)^2, s1 = sum M'y^2 (SC),
//                            s2 = sum dist(log M'x, log M'y), s3 = sum dist(M'x, M'y); the projected magnitudes of x and y are saved
//                            for the backward.  A term that is not asked for is not evaluated.
//   stft_terms_final_kernel  one wave per row adds the partials in a fixed order (order-deterministic, as stft_sums_final_kernel)
//   stft_terms_bwd_kernel    d loss / d M' per projected element, the adjoint projection as a gather over each bin's <= 2 (filter,
//                            weight) pairs, then (re, im) / M with the forward's clamp: zero where re^2 + im^2 < eps
//   stft_terms_total_kernel  the loss from the sums of every resolution, one wave
#include <cfloat>
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int STFT_TERMS_SPLIT = 32;
constexpr int STFT_TERMS_MAX = 16;
constexpr int TERM_SC = 1, TERM_LOG = 2, TERM_LIN = 4;

__device__ __forceinline__ float terms_mag(float re, float im, float eps) { return sqrtf(fmaxf(re * re + im * im, eps)); }
__device__ __forceinline__ float terms_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }

template <bool MEL>
__global__ __launch_bounds__(256) void stft_terms_fwd_kernel(const float* __restrict__ spec, int rows, int bins, int frames, float eps,
                                                             int n_out, const int* __restrict__ fb_lo, const int* __restrict__ fb_off,
                                                             const float* __restrict__ fb_w, int terms, int l2, float* __restrict__ mags,
                                                             float* __restrict__ partial) {
  __shared__ float red[4];
  const int r = blockIdx.y;
  const long long cols = 2LL * rows * frames, im = (long long)bins * cols;
  const float* sx = spec + (long long)r * frames;
  const float* sy = spec + (long long)(rows + r) * frames;
  const int n = n_out * frames;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += STFT_TERMS_SPLIT * 256) {
    const int m = i / frames, f = i - m * frames;
    float xm, ym;
    if (MEL) {
      xm = 0.f;
      ym = 0.f;
      const int o0 = fb_off[m], o1 = fb_off[m + 1];
      long long e = (long long)fb_lo[m] * cols + f;
      for (int j = o0; j < o1; ++j, e += cols) {
        const float w = fb_w[j];
        xm += w * terms_mag(sx[e], sx[e + im], eps);
        ym += w * terms_mag(sy[e], sy[e + im], eps);
      }
      mags[(long long)r * n + i] = xm;
      mags[(long long)(rows + r) * n + i] = ym;
    } else {
      const long long e = (long long)m * cols + f;
      xm = terms_mag(sx[e], sx[e + im], eps);
      ym = terms_mag(sy[e], sy[e + im], eps);
    }
    if (terms & TERM_SC) {
      const float d = ym - xm;
      s0 += d * d;
      s1 += ym * ym;
    }
    if (terms & TERM_LOG) {
      const float d = logf(xm) - logf(ym);
      s2 += l2 ? d * d : fabsf(d);
    }
    if (terms & TERM_LIN) {
      const float d = xm - ym;
      s3 += l2 ? d * d : fabsf(d);
    }
  }
  s0 = block_sum_256(s0, red);
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  s3 = block_sum_256(s3, red);
  if (threadIdx.x == 0) {
    float* o = partial + ((long long)r * STFT_TERMS_SPLIT + blockIdx.x) * 4;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  }
}

__global__ __launch_bounds__(64) void stft_terms_final_kernel(const float* __restrict__ partial, float* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int k = 0; k < 4; ++k) {
    float v = lane < STFT_TERMS_SPLIT ? partial[((long long)r * STFT_TERMS_SPLIT + lane) * 4 + k] : 0.f;
    v = wave_sum(v);
    if (lane == 0) out[4 * r + k] = v;
  }
}

// d loss / d M'x of one projected element (a = M'x, b = M'y); the coefficients carry the weights, gout and the means' counts
__device__ __forceinline__ float terms_dmag(float a, float b, int terms, int l2, float c_sc, float c_lg, float c_lin) {
  float d = 0.f;
  if (terms & TERM_SC) d += c_sc * (a - b);
  if (terms & TERM_LOG) {
    const float dl = logf(a) - logf(b);
    d += c_lg * (l2 ? 2.f * dl : terms_sign(dl)) / a;
  }
  if (terms & TERM_LIN) {
    const float dd = a - b;
    d += c_lin * (l2 ? 2.f * dd : terms_sign(dd));
  }
  return d;
}

template <bool MEL>
__global__ __launch_bounds__(256) void stft_terms_bwd_kernel(const float* __restrict__ spec, int rows, int bins, int frames, float eps,
                                                             int n_out, const int* __restrict__ bin_m, const float* __restrict__ bin_w,
                                                             const float* __restrict__ mags, int terms, int l2, float w_sc, float w_log,
                                                             float w_lin, const float* __restrict__ sums, const float* __restrict__ gout,
                                                             float scale, float* __restrict__ dspec) {
  const int r = blockIdx.y;
  const long long cols = 2LL * rows * frames, im = (long long)bins * cols;
  const long long xcols = (long long)rows * frames, oim = (long long)bins * xcols;
  const float* sx = spec + (long long)r * frames;
  const float* sy = spec + (long long)(rows + r) * frames;
  const long long per = (long long)n_out * frames;
  const float* mx = MEL ? mags + (long long)r * per : nullptr;
  const float* my = MEL ? mags + (long long)(rows + r) * per : nullptr;
  float* dx = dspec + (long long)r * frames;
  const int n = bins * frames;
  const float g = gout[0] * scale;
  // the FLT_MIN floor: d ||Y - X|| taken as 0 where ||Y - X|| = 0 (a row whose spectra agree exactly), as in stft_bwd_kernel
  const float c_sc = (terms & TERM_SC) ? w_sc * g / ((float)rows * sqrtf(fmaxf(sums[4 * r], FLT_MIN)) * sqrtf(sums[4 * r + 1])) : 0.f;
  const float inv = 1.f / ((float)rows * (float)n_out * (float)frames);
  const float c_lg = w_log * g * inv, c_lin = w_lin * g * inv;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int k = i / frames, f = i - k * frames;
    const long long e = (long long)k * cols + f;
    const float re = sx[e], ie = sx[e + im];
    const float p = re * re + ie * ie;
    const float xm = sqrtf(fmaxf(p, eps));
    float dmag = 0.f;
    if (MEL) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = bin_m[2 * k + q];
        if (m >= 0) {
          const long long o = (long long)m * frames + f;
          dmag += bin_w[2 * k + q] * terms_dmag(mx[o], my[o], terms, l2, c_sc, c_lg, c_lin);
        }
      }
    } else {
      dmag = terms_dmag(xm, terms_mag(sy[e], sy[e + im], eps), terms, l2, c_sc, c_lg, c_lin);
    }
    dmag = p >= eps ? dmag / xm : 0.f;   // d sqrt(clamp(p)) / d(re, im) = (re, im) / M, zero under the clamp
    const long long oe = (long long)k * xcols + f;
    dx[oe] = dmag * re;
    dx[oe + oim] = dmag * ie;
  }
}

struct StftTermsTable { const float* sums[STFT_TERMS_MAX]; float inv_count[STFT_TERMS_MAX]; };
__global__ __launch_bounds__(64) void stft_terms_total_kernel(const StftTermsTable T, int n, int rows, int terms, float w_sc, float w_log,
                                                              float w_lin, float* __restrict__ out) {
  const int lane = threadIdx.x;
  float total = 0.f;
  for (int p = 0; p < n; ++p) {
    const float* s = T.sums[p];
    float sc = 0.f, lg = 0.f, ln = 0.f;
    for (int r = lane; r < rows; r += 64) {
      if (terms & TERM_SC) sc += sqrtf(s[4 * r] / s[4 * r + 1]);
      lg += s[4 * r + 2];
      ln += s[4 * r + 3];
    }
    sc = wave_sum(sc);
    lg = wave_sum(lg);
    ln = wave_sum(ln);
    float term = 0.f;
    if (terms & TERM_SC) term += w_sc * (sc / (float)rows);
    if (terms & TERM_LOG) term += w_log * (lg * T.inv_count[p]);
    if (terms & TERM_LIN) term += w_lin * (ln * T.inv_count[p]);
    total += term;
  }
  if (lane == 0) out[0] = total / (float)n;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" size_t eben_stft_terms_workspace(int rows) { return sizeof(float) * 4 * (size_t)STFT_TERMS_SPLIT * (rows > 0 ? rows : 0); }

extern "C" int eben_stft_terms_fwd(const float* spec, int rows, int bins, int frames, float eps, int n_out, const int* fb_lo,
                                   const int* fb_off, const float* fb_w, int terms, int l2, float* mags, float* partial_ws,
                                   size_t ws_bytes, float* sums, void* stream) {
  EBEN_REQUIRE(spec && sums && partial_ws && rows > 0 && bins > 0 && frames > 0, "bad stft_terms_fwd arguments");
  EBEN_REQUIRE(terms > 0 && terms <= (TERM_SC | TERM_LOG | TERM_LIN), "stft_terms_fwd: terms must be a non-empty mask of 1 | 2 | 4");
  const bool mel = fb_lo != nullptr;
  EBEN_REQUIRE(!mel || (fb_off && fb_w && mags && n_out > 0), "stft_terms_fwd: the mel projection needs its table and a magnitude buffer");
  EBEN_REQUIRE(mel || n_out == bins, "stft_terms_fwd: without a projection n_out must equal bins");
  EBEN_REQUIRE((long long)n_out * frames < (1LL << 31), "stft_terms_fwd: too large");
  if (ws_bytes < eben_stft_terms_workspace(rows)) return fail(EBEN_EWORKSPACE, "stft_terms_fwd needs %zu workspace bytes", eben_stft_terms_workspace(rows));
  float* partial = partial_ws;
  if (mel)
    hipLaunchKernelGGL(stft_terms_fwd_kernel<true>, dim3(STFT_TERMS_SPLIT, rows), dim3(256), 0, as_stream(stream), spec, rows, bins, frames,
                       eps, n_out, fb_lo, fb_off, fb_w, terms, l2, mags, partial);
  else
    hipLaunchKernelGGL(stft_terms_fwd_kernel<false>, dim3(STFT_TERMS_SPLIT, rows), dim3(256), 0, as_stream(stream), spec, rows, bins, frames,
                       eps, n_out, nullptr, nullptr, nullptr, terms, l2, nullptr, partial);
  EBEN_CHECK_LAUNCH("stft_terms_fwd_kernel");
  hipLaunchKernelGGL(stft_terms_final_kernel, dim3(rows), dim3(64), 0, as_stream(stream), partial, sums);
  EBEN_CHECK_LAUNCH("stft_terms_final_kernel");
  return EBEN_OK;
}

extern "C" int eben_stft_terms_bwd(const float* spec, int rows, int bins, int frames, float eps, int n_out, const int* bin_m,
                                   const float* bin_w, const float* mags, int terms, int l2, float w_sc, float w_log, float w_lin,
                                   const float* sums, const float* gout, float scale, float* dspec, void* stream) {
  EBEN_REQUIRE(spec && sums && gout && dspec && rows > 0 && bins > 0 && frames > 0, "bad stft_terms_bwd arguments");
  EBEN_REQUIRE(terms > 0 && terms <= (TERM_SC | TERM_LOG | TERM_LIN), "stft_terms_bwd: terms must be a non-empty mask of 1 | 2 | 4");
  const bool mel = bin_m != nullptr;
  EBEN_REQUIRE(!mel || (bin_w && mags && n_out > 0), "stft_terms_bwd: the mel projection needs its adjoint table and the saved magnitudes");
  EBEN_REQUIRE(mel || n_out == bins, "stft_terms_bwd: without a projection n_out must equal bins");
  EBEN_REQUIRE((long long)bins * frames < (1LL << 31), "stft_terms_bwd: too large");
  const int nb = ceil_div(bins * frames, 256) < 64 ? ceil_div(bins * frames, 256) : 64;
  if (mel)
    hipLaunchKernelGGL(stft_terms_bwd_kernel<true>, dim3(nb, rows), dim3(256), 0, as_stream(stream), spec, rows, bins, frames, eps, n_out,
                       bin_m, bin_w, mags, terms, l2, w_sc, w_log, w_lin, sums, gout, scale, dspec);
  else
    hipLaunchKernelGGL(stft_terms_bwd_kernel<false>, dim3(nb, rows), dim3(256), 0, as_stream(stream), spec, rows, bins, frames, eps, n_out,
                       nullptr, nullptr, nullptr, terms, l2, w_sc, w_log, w_lin, sums, gout, scale, dspec);
  EBEN_CHECK_LAUNCH("stft_terms_bwd_kernel");
  return EBEN_OK;
}

extern "C" int eben_stft_terms_total(const void* const* sums, const float* inv_counts, int n, int rows, int terms, float w_sc, float w_log,
                                     float w_lin, float* out, void* stream) {
  EBEN_REQUIRE(sums && inv_counts && out && n > 0 && n <= STFT_TERMS_MAX && rows > 0, "stft_terms_total: 1..%d resolutions", STFT_TERMS_MAX);
  EBEN_REQUIRE(terms > 0 && terms <= (TERM_SC | TERM_LOG | TERM_LIN), "stft_terms_total: terms must be a non-empty mask of 1 | 2 | 4");
  StftTermsTable T;
  for (int i = 0; i < n; ++i) {
    EBEN_REQUIRE(sums[i], "stft_terms_total: null sums %d", i);
    T.sums[i] = static_cast<const float*>(sums[i]);
    T.inv_count[i] = inv_counts[i];
  }
  hipLaunchKernelGGL(stft_terms_total_kernel, dim3(1), dim3(64), 0, as_stream(stream), T, n, rows, terms, w_sc, w_log, w_lin, out);
  EBEN_CHECK_LAUNCH("stft_terms_total_kernel");
  return EBEN_OK;
}
