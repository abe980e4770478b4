// Multi-rate downsampling of MelganMultiScalesDiscriminator (torchaudio Resample(sample_rate, sample_rate // 2**s,
// "sinc_interp_kaiser") per scale s), forward and adjoint.  With the rates reduced by their gcd to orig / new and the
// kernel table k (new, taps = 2*width + orig) built on the host (vibravox_amd/augment.py), torchaudio's
// _apply_sinc_resample_kernel (zero pad (width, width + orig), conv1d stride orig over the new phases, interleave, crop to
// ceil(new*T/orig)) is
//     y[r, q*new + p] = sum_{j < taps} k[p, j] * x[r, q*orig + j - width]      (x = 0 outside [0, T))
// and its adjoint, in gather form (one thread per input sample, q ascending, then p, fmaf; no atomics):
//     dx[r, i] = sum_{q, p: 0 <= j = i + width - q*orig < taps, q*new + p < t_out} k[p, j] * g[r, q*new + p].
//
// Two paths:
//   * fused (every scale reduces to new = 1, orig = 2^s): one forward launch stages each row's waveform tile and every
//     scale's table in LDS once and writes all downsampled versions; one adjoint launch stages the matching slices of every
//     scale's gradient in LDS and writes d_audio = g_0 + sum_s A_s^T g_s (per-scale partial sums added in scale order).
//   * general rational ratio: the forward is eben_resample (direct.hip); the adjoint is resample_adjoint_kernel below.  For
//     22050 -> 5512 (11025 : 2756, taps 11075) a wave's 64 lanes share one or two q, so their gradient loads are broadcasts
//     and their table loads one coalesced row segment; each thread keeps kRows rows in registers so a table value loaded
//     once feeds kRows FMAs.
#include "common.h"

namespace eben {
namespace {

constexpr int kMaxDown = 5;                    // downsampled scales of the fused path (orig up to 32)
constexpr int kTile = 1024;                    // input samples per fused workgroup
constexpr int kXCap = 1536;                    // LDS floats of the forward waveform tile: kTile + 2 * max width
constexpr int kKCap = 1024;                    // LDS floats of all scales' tables
constexpr int kGCap = 1280;                    // LDS floats of the adjoint's staged gradient slices
constexpr int kRows = 4;                       // rows per thread of the general adjoint

struct MrPlan {
  int nd;                    // downsampled scales (scale s + 1 has orig = 2^(s+1), new = 1)
  int width[kMaxDown];
  int koff[kMaxDown];        // offset of scale s's table in the packed tables
  int t_out[kMaxDown];       // ceil(t_in / orig)
  int ktotal;                // sum of taps
  int wmax;
  float* out[kMaxDown];      // forward outputs (rows, t_out[s])
  const float* g[kMaxDown];  // adjoint inputs (rows, t_out[s])
};

__device__ __forceinline__ int q_first(int num, int orig) { return num <= 0 ? 0 : (num + orig - 1) / orig; }

__global__ __launch_bounds__(256) void multirate_fwd_kernel(const float* __restrict__ x, const float* __restrict__ tables, MrPlan plan,
                                                            int t_in) {
  __shared__ float xs[kXCap];
  __shared__ float ks[kKCap];
  const int r = blockIdx.y;
  const int i0 = blockIdx.x * kTile;
  const int lo = i0 - plan.wmax, span = kTile + 2 * plan.wmax;
  const float* xr = x + (long long)r * t_in;
  for (int u = threadIdx.x; u < span; u += 256) {
    const int i = lo + u;
    xs[u] = (i >= 0 && i < t_in) ? xr[i] : 0.f;
  }
  for (int u = threadIdx.x; u < plan.ktotal; u += 256) ks[u] = tables[u];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kMaxDown; ++s) {   // unrolled: the plan's arrays are indexed by constants (no scratch copy)
    if (s >= plan.nd) break;
    const int orig = 2 << s, w = plan.width[s], taps = 2 * w + orig;
    const float* k = ks + plan.koff[s];
    const int n_lo = i0 / orig, n_hi = min(plan.t_out[s], (i0 + kTile) / orig);
    float* o = plan.out[s] + (long long)r * plan.t_out[s];
    for (int n = n_lo + threadIdx.x; n < n_hi; n += 256) {
      const float* xp = xs + (n * orig - w - lo);
      float acc = 0.f;
      for (int j = 0; j < taps; ++j) acc = fmaf(k[j], xp[j], acc);
      o[n] = acc;
    }
  }
}

__global__ __launch_bounds__(256) void multirate_adj_kernel(const float* __restrict__ g0, const float* __restrict__ tables, MrPlan plan,
                                                            float* __restrict__ dx, int t_in) {
  __shared__ float gs[kGCap];
  __shared__ float ks[kKCap];
  const int r = blockIdx.y;
  const int i0 = blockIdx.x * kTile;
  int qlo[kMaxDown], goff[kMaxDown];
  int off = 0;
#pragma unroll
  for (int s = 0; s < kMaxDown; ++s) {
    if (s >= plan.nd) break;
    const int orig = 2 << s, w = plan.width[s];
    const int a = q_first(i0 - w - orig + 1, orig);
    const int b = min(plan.t_out[s] - 1, (i0 + kTile - 1 + w) / orig);
    qlo[s] = a;
    goff[s] = off - a;
    const float* gr = plan.g[s] + (long long)r * plan.t_out[s];
    for (int u = threadIdx.x; u <= b - a; u += 256) gs[off + u] = gr[a + u];
    off += max(0, b - a + 1);
  }
  for (int u = threadIdx.x; u < plan.ktotal; u += 256) ks[u] = tables[u];
  __syncthreads();
  const float* g0r = g0 ? g0 + (long long)r * t_in : nullptr;
  float* dxr = dx + (long long)r * t_in;
  for (int i = i0 + threadIdx.x; i < min(t_in, i0 + kTile); i += 256) {
    float acc = g0r ? g0r[i] : 0.f;
#pragma unroll
    for (int s = 0; s < kMaxDown; ++s) {
      if (s >= plan.nd) break;
      const int orig = 2 << s, w = plan.width[s], taps = 2 * w + orig;
      const int qa = max(qlo[s], q_first(i + w - taps + 1, orig));
      const int qb = min(plan.t_out[s] - 1, (i + w) / orig);
      const float* k = ks + plan.koff[s] + i + w;
      const float* g = gs + goff[s];
      float part = 0.f;
      for (int q = qa; q <= qb; ++q) part = fmaf(k[-q * orig], g[q], part);
      acc += part;
    }
    dxr[i] = acc;
  }
}

__global__ __launch_bounds__(256) void resample_adjoint_kernel(const float* __restrict__ g, const float* __restrict__ kernels,
                                                               float* __restrict__ dx, int rows, int t_in, int t_out, int orig, int nw,
                                                               int width, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= t_in) return;
  const int r0 = blockIdx.y * kRows;
  const int taps = 2 * width + orig;
  const float* gr[kRows];
#pragma unroll
  for (int u = 0; u < kRows; ++u) gr[u] = g + (long long)min(r0 + u, rows - 1) * t_out;
  float acc[kRows];
#pragma unroll
  for (int u = 0; u < kRows; ++u) acc[u] = 0.f;
  const int qa = q_first(i + width - taps + 1, orig);
  const int qb = min((i + width) / orig, (t_out - 1) / nw);
  for (int q = qa; q <= qb; ++q) {
    const float* k = kernels + (i + width - q * orig);
    const int n0 = q * nw, pn = min(nw, t_out - n0);
    for (int p = 0; p < pn; ++p) {
      const float kv = k[(long long)p * taps];
#pragma unroll
      for (int u = 0; u < kRows; ++u) acc[u] = fmaf(kv, gr[u][n0 + p], acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < kRows; ++u) {
    if (r0 + u >= rows) break;
    float* d = dx + (long long)(r0 + u) * t_in + i;
    *d = accumulate ? *d + acc[u] : acc[u];
  }
}

int make_plan(MrPlan& plan, int t_in, int scales, const int* widths) {
  EBEN_REQUIRE(scales >= 2 && scales - 1 <= kMaxDown, "multirate: scales must be in [2, %d]", kMaxDown + 1);
  EBEN_REQUIRE(widths != nullptr, "multirate: widths is NULL");
  plan.nd = scales - 1;
  plan.ktotal = 0;
  plan.wmax = 0;
  int gtotal = 0;
  for (int s = 0; s < plan.nd; ++s) {
    const int orig = 2 << s, w = widths[s];
    EBEN_REQUIRE(w >= 0 && w <= 4 * orig * 6, "multirate: width %d of scale %d out of range", w, s + 1);
    plan.width[s] = w;
    plan.koff[s] = plan.ktotal;
    plan.ktotal += 2 * w + orig;
    plan.wmax = w > plan.wmax ? w : plan.wmax;
    plan.t_out[s] = (int)(((long long)t_in + orig - 1) / orig);
    gtotal += (kTile - 1 + 2 * w + orig - 1) / orig + 2;   // bound of the staged slice, whatever the tile's alignment
  }
  EBEN_REQUIRE(plan.ktotal <= kKCap, "multirate: %d table floats exceed the LDS budget %d", plan.ktotal, kKCap);
  EBEN_REQUIRE(kTile + 2 * plan.wmax <= kXCap, "multirate: width %d exceeds the waveform tile's halo", plan.wmax);
  EBEN_REQUIRE(gtotal <= kGCap, "multirate: %d staged gradient floats exceed the LDS budget %d", gtotal, kGCap);
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_multirate_down(const float* x, const float* tables, const int* widths, float* const* outs, int rows, int t_in,
                                   int scales, void* stream) {
  EBEN_REQUIRE(x && tables && outs && rows > 0 && rows <= 65535 && t_in > 0, "bad multirate_down arguments");
  MrPlan plan{};
  const int rc = make_plan(plan, t_in, scales, widths);
  if (rc != EBEN_OK) return rc;
  for (int s = 0; s < plan.nd; ++s) {
    EBEN_REQUIRE(outs[s] != nullptr, "multirate_down: output %d is NULL", s + 1);
    plan.out[s] = outs[s];
  }
  hipLaunchKernelGGL(multirate_fwd_kernel, dim3(ceil_div(t_in, kTile), rows), dim3(256), 0, as_stream(stream), x, tables, plan, t_in);
  EBEN_CHECK_LAUNCH("multirate_fwd_kernel");
  return EBEN_OK;
}

extern "C" int eben_multirate_down_adjoint(const float* g0, const float* const* gs, const float* tables, const int* widths, float* dx,
                                           int rows, int t_in, int scales, void* stream) {
  EBEN_REQUIRE(gs && tables && dx && rows > 0 && rows <= 65535 && t_in > 0, "bad multirate_down_adjoint arguments");
  MrPlan plan{};
  const int rc = make_plan(plan, t_in, scales, widths);
  if (rc != EBEN_OK) return rc;
  for (int s = 0; s < plan.nd; ++s) {
    EBEN_REQUIRE(gs[s] != nullptr, "multirate_down_adjoint: gradient %d is NULL", s + 1);
    plan.g[s] = gs[s];
  }
  hipLaunchKernelGGL(multirate_adj_kernel, dim3(ceil_div(t_in, kTile), rows), dim3(256), 0, as_stream(stream), g0, tables, plan, dx, t_in);
  EBEN_CHECK_LAUNCH("multirate_adj_kernel");
  return EBEN_OK;
}

extern "C" int eben_resample_adjoint(const float* g, const float* kernels, float* dx, int rows, int t_in, int t_out, int orig, int nw,
                                     int width, int accumulate, void* stream) {
  EBEN_REQUIRE(g && kernels && dx && rows > 0 && t_in > 0 && t_out > 0 && orig > 0 && nw > 0 && width >= 0, "bad resample_adjoint arguments");
  EBEN_REQUIRE((long long)t_out <= ((long long)nw * t_in + orig - 1) / orig, "resample_adjoint: t_out beyond ceil(new * t_in / orig)");
  EBEN_REQUIRE((long long)nw * (2 * width + orig) < (1ll << 31), "resample_adjoint: table too large");
  EBEN_REQUIRE(ceil_div(rows, kRows) <= 65535, "resample_adjoint: too many rows");
  hipLaunchKernelGGL(resample_adjoint_kernel, dim3(ceil_div(t_in, 256), ceil_div(rows, kRows)), dim3(256), 0, as_stream(stream), g, kernels,
                     dx, rows, t_in, t_out, orig, nw, width, accumulate);
  EBEN_CHECK_LAUNCH("resample_adjoint_kernel");
  return EBEN_OK;
}
