// Per-clip waveform augmentation at a constant batch length (vibravox_amd/augment.py, WaveformDataAugmentation(per_clip=True)).
//
// The batch-level kernels of direct.hip take one speed factor, one pitch step and one mask for the whole padded batch.  Here
// every row carries its own: per-row descriptors travel by value, 48 per launch (as CollateTable does), rows of different
// ratios share a launch, and every stage leaves the batch dense at T samples per row.  The arithmetic of a row is the
// batch-level kernel's on that row alone, operation for operation, so a row is bit-identical to the merged function:
//
//   * resample_clips_kernel   resample_kernel's sum without the taps whose table value is exactly 0: per ratio a band table
//                             band[nw][W] and first[nw]; crop / zero fill to T fused;
//   * vocoder_clips_kernel    phase_vocoder_kernel's walk with rate, frames_out and the output column per row;
//   * ola_clips_kernel        overlap-add (ola_gather's order) times the window envelope 1 / sum_f w^2 (float64 sum, ascending f),
//                             rows of len_stretch samples into a ragged buffer, zero past `valid`;
//   * mask_clips_kernel       zero fill of (first, count) per row.
//
// Streaming kernels: a thread owns the four consecutive samples of one 16-byte line of its row (rows may start anywhere in a
// line; the ragged ends fall back to single stores), so stores along time are coalesced 16-byte ones.
#include "common.h"

#include <vector>

namespace eben {

constexpr int CLIP_CHUNK = 48;

struct ResampleClipTable { EbenClipBand bands[EBEN_CLIP_MAX_BANDS]; EbenResampleClip rows[CLIP_CHUNK]; };
struct VocoderClipTable { EbenVocoderClip rows[CLIP_CHUNK]; };
struct OlaClipTable { EbenOlaClip rows[CLIP_CHUNK]; };
struct MaskClipTable { EbenMaskClip rows[CLIP_CHUNK]; };

// floats between the 16-byte boundary at or below p and p
__device__ __forceinline__ int line_shift(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// samples [n0, n0 + 4) of a row of t samples at o, where o + n0 is 16-byte aligned: one 16-byte store, or single ones at the row's ends
__device__ __forceinline__ void store_line(float* __restrict__ o, int n0, int t, const float v[4]) {
  if (n0 >= 0 && n0 + 4 <= t) {
    *reinterpret_cast<f32x4*>(o + n0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n0 + e >= 0 && n0 + e < t) o[n0 + e] = v[e];
  }
}

// out[n] = sum_j band[p][j] * x[q*orig - width + first[p] + j], n = q*nw + p: one accumulator, fmaf, j ascending, zero outside the row
__device__ __forceinline__ float band_sample(const float* __restrict__ xr, int t_in, const EbenClipBand& B, int n) {
  const int q = n / B.nw, p = n - q * B.nw;
  const float* k = B.band + (long long)p * B.W;
  const long long base = (long long)q * B.orig - B.width + B.first[p];
  float acc = 0.f;
  for (int j = 0; j < B.W; ++j) {
    const long long i = base + j;
    if (i >= 0 && i < t_in) acc = fmaf(k[j], xr[i], acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void resample_clips_kernel(const ResampleClipTable T, const float* __restrict__ x, float* __restrict__ out, int t) {
  const EbenResampleClip row = T.rows[blockIdx.y];
  const EbenClipBand& B = T.bands[row.band];
  const float* xr = x + row.src_offset;
  float* o = out + (long long)row.dst_row * t;
  const long long t_full = ((long long)B.nw * row.t_in + B.orig - 1) / B.orig;   // ceil(new * t_in / orig)
  const int t_out = t_full < t ? (int)t_full : t;
  const int shift = line_shift(o);
  for (int g = blockIdx.x * 256 + threadIdx.x; 4 * g - shift < t; g += gridDim.x * 256) {
    const int n0 = 4 * g - shift;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + e;
      v[e] = (n >= 0 && n < t_out) ? band_sample(xr, row.t_in, B, n) : 0.f;
    }
    store_line(o, n0, t, v);
  }
}

// phase_vocoder_kernel (direct.hip) with the row's rate, frames_out and output column; the walk itself is unchanged
__global__ __launch_bounds__(256) void vocoder_clips_kernel(const VocoderClipTable T, const float* __restrict__ spec, float* __restrict__ out, int row0,
                                                            int nrows, int bins, int frames, long long in_cols, long long out_cols, float hop) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows * bins) return;
  const int r = i / bins, k = i - r * bins;
  const EbenVocoderClip c = T.rows[r];
  const int frames_out = c.frames_out;
  const double rate = c.rate;
  const float* re = spec + (long long)k * in_cols + (long long)(row0 + r) * frames;
  const float* im = re + (long long)bins * in_cols;
  float* ore = out + (long long)k * out_cols + c.col_out;
  float* oim = ore + (long long)bins * out_cols;
  const double two_pi = 6.283185307179586476925286766559;
  const double adv = 3.14159265358979323846264338327950288 * (double)hop * (double)k / (double)(bins - 1);
  double phase = atan2((double)im[0], (double)re[0]);
  double a0 = phase;   // angle(spec[i0]) of the current frame pair, reused while i0 stands still
  int i0_prev = 0;
  for (int f = 0; f < frames_out; ++f) {
    const double ts = (double)f * rate;   // as torch.arange(0, frames, rate) in float64: the frame index must not flip
    const int i0 = (int)ts;
    const double alpha = ts - (double)i0;
    const float r0 = i0 < frames ? re[i0] : 0.f, m0 = i0 < frames ? im[i0] : 0.f;
    const float r1 = i0 + 1 < frames ? re[i0 + 1] : 0.f, m1 = i0 + 1 < frames ? im[i0 + 1] : 0.f;
    const double n0 = sqrt((double)r0 * r0 + (double)m0 * m0), n1 = sqrt((double)r1 * r1 + (double)m1 * m1);
    const double mag = alpha * n1 + (1.0 - alpha) * n0;
    double sn, cs;
    sincos(phase, &sn, &cs);
    ore[f] = (float)(mag * cs);
    oim[f] = (float)(mag * sn);
    if (i0 != i0_prev) { a0 = atan2((double)m0, (double)r0); i0_prev = i0; }
    double d = atan2((double)m1, (double)r1) - a0 - adv;
    d = d - two_pi * rint(d / two_pi);
    phase += d + adv;
  }
}

// frames_buf element (window sample j, frame f of the row) at j*cols + col + f.  Sample u of the row sits at s = u + pad of the
// overlap-added signal: sum over the covering frames in ascending f (ola_gather's order, float32), then times
// float32(1 / sum_f w2[s - f*hop]) with the sum in float64 and the same order (what pitch_shift's host table holds).
__global__ __launch_bounds__(256) void ola_clips_kernel(const OlaClipTable T, const float* __restrict__ buf, const double* __restrict__ w2,
                                                        float* __restrict__ out, long long cols, int win, int hop, int pad) {
  const EbenOlaClip c = T.rows[blockIdx.y];
  const float* bb = buf + c.col;
  float* o = out + c.dst_offset;
  const int shift = line_shift(o);
  for (int g = blockIdx.x * 256 + threadIdx.x; 4 * g - shift < c.len_stretch; g += gridDim.x * 256) {
    const int n0 = 4 * g - shift;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int u = n0 + e;
      v[e] = 0.f;
      if (u >= 0 && u < c.valid) {
        const int s = u + pad;
        int fmax = s / hop;
        if (fmax > c.frames_out - 1) fmax = c.frames_out - 1;
        const int fmin = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
        float acc = 0.f;
        double env = 0.0;
        for (int f = fmin; f <= fmax; ++f) {
          acc += bb[(long long)(s - f * hop) * cols + f];
          env += w2[s - f * hop];
        }
        v[e] = acc * (float)(1.0 / env);
      }
    }
    store_line(o, n0, c.len_stretch, v);
  }
}

__global__ __launch_bounds__(256) void mask_clips_kernel(const MaskClipTable T, float* __restrict__ x, int t) {
  const EbenMaskClip c = T.rows[blockIdx.y];
  float* o = x + (long long)c.row * t + c.first;
  const int shift = line_shift(o);
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  for (int g = blockIdx.x * 256 + threadIdx.x; 4 * g - shift < c.count; g += gridDim.x * 256) store_line(o, 4 * g - shift, c.count, zero);
}

static bool ranges_overlap(const float* a, long long na, const float* b, long long nb) { return a < b + nb && b < a + na; }

}  // namespace eben

using namespace eben;

extern "C" int eben_resample_clips(const float* x, int64_t x_floats, float* out, int out_rows, int t, const EbenClipBand* bands, int nbands,
                                   const EbenResampleClip* rows, int nrows, void* stream) {
  EBEN_REQUIRE(x && out && bands && rows, "resample_clips: null pointer");
  EBEN_REQUIRE(x_floats > 0 && out_rows > 0 && t > 0 && nrows > 0, "resample_clips: %lld input floats, %d output rows of %d samples, %d rows", (long long)x_floats,
               out_rows, t, nrows);
  EBEN_REQUIRE(nbands > 0 && nbands <= EBEN_CLIP_MAX_BANDS, "resample_clips: %d ratios (1..%d a call)", nbands, EBEN_CLIP_MAX_BANDS);
  EBEN_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0, "resample_clips: misaligned pointer");
  EBEN_REQUIRE(!ranges_overlap(x, x_floats, out, (long long)out_rows * t), "resample_clips: out overlaps x");
  for (int i = 0; i < nbands; ++i) {
    const EbenClipBand& b = bands[i];
    if (!b.band || !b.first) return fail(EBEN_EINVAL, "resample_clips: null table of ratio %d", i);
    if (b.orig <= 0 || b.nw <= 0 || b.width < 0 || b.W <= 0 || b.orig > (1 << 20) || b.nw > (1 << 20) || b.W > 2 * b.width + b.orig)
      return fail(EBEN_EINVAL, "resample_clips: ratio %d is %d : %d, width %d, band %d", i, b.orig, b.nw, b.width, b.W);
  }
  std::vector<char> written((size_t)out_rows, 0);
  for (int i = 0; i < nrows; ++i) {
    const EbenResampleClip& r = rows[i];
    if (r.band < 0 || r.band >= nbands) return fail(EBEN_EINVAL, "resample_clips: row %d names ratio %d of %d", i, r.band, nbands);
    if (r.t_in <= 0 || r.t_in > (1 << 30) || r.src_offset < 0 || r.src_offset + r.t_in > x_floats)
      return fail(EBEN_EINVAL, "resample_clips: row %d reads %d samples at %lld of %lld", i, r.t_in, (long long)r.src_offset, (long long)x_floats);
    if (r.dst_row < 0 || r.dst_row >= out_rows) return fail(EBEN_EINVAL, "resample_clips: row %d writes row %d of %d", i, r.dst_row, out_rows);
    if (written[r.dst_row]) return fail(EBEN_EINVAL, "resample_clips: two rows write row %d", r.dst_row);
    written[r.dst_row] = 1;
  }
  int gx = ceil_div(t + 3, 1024);   // 256 threads x one 16-byte line each; + 3: a row may start inside a line
  if (gx > 256) gx = 256;
  for (int p0 = 0; p0 < nrows; p0 += CLIP_CHUNK) {
    const int cnt = nrows - p0 < CLIP_CHUNK ? nrows - p0 : CLIP_CHUNK;
    ResampleClipTable T;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < nbands; ++i) T.bands[i] = bands[i];
    for (int i = 0; i < cnt; ++i) T.rows[i] = rows[p0 + i];
    hipLaunchKernelGGL(resample_clips_kernel, dim3(gx, cnt), dim3(256), 0, as_stream(stream), T, x, out, t);
    EBEN_CHECK_LAUNCH("resample_clips_kernel");
  }
  return EBEN_OK;
}

extern "C" int eben_phase_vocoder_clips(const float* spec, float* out, int bins, int frames, int64_t out_cols, const EbenVocoderClip* rows, int nrows,
                                        float hop, void* stream) {
  EBEN_REQUIRE(spec && out && rows, "phase_vocoder_clips: null pointer");
  EBEN_REQUIRE(nrows > 0 && bins > 1 && frames > 0 && out_cols > 0, "phase_vocoder_clips: %d rows, %d bins, %d frames, %lld output columns", nrows, bins,
               frames, (long long)out_cols);
  EBEN_REQUIRE((long long)nrows * frames < (1ll << 31) && (long long)nrows * bins < (1ll << 31), "phase_vocoder_clips: too many rows");
  long long end = 0;
  for (int i = 0; i < nrows; ++i) {
    const EbenVocoderClip& r = rows[i];
    if (!(r.rate > 0.0) || r.frames_out <= 0) return fail(EBEN_EINVAL, "phase_vocoder_clips: row %d has rate %g, %d output frames", i, r.rate, r.frames_out);
    if (r.col_out < end || (long long)r.col_out + r.frames_out > out_cols)
      return fail(EBEN_EINVAL, "phase_vocoder_clips: row %d writes columns [%d, %lld) of %lld (ascending, disjoint)", i, r.col_out,
                  (long long)r.col_out + r.frames_out, (long long)out_cols);
    end = (long long)r.col_out + r.frames_out;
  }
  for (int p0 = 0; p0 < nrows; p0 += CLIP_CHUNK) {
    const int cnt = nrows - p0 < CLIP_CHUNK ? nrows - p0 : CLIP_CHUNK;
    VocoderClipTable T;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < cnt; ++i) T.rows[i] = rows[p0 + i];
    hipLaunchKernelGGL(vocoder_clips_kernel, dim3(ceil_div(cnt * bins, 256)), dim3(256), 0, as_stream(stream), T, spec, out, p0, cnt, bins, frames,
                       (long long)nrows * frames, (long long)out_cols, hop);
    EBEN_CHECK_LAUNCH("vocoder_clips_kernel");
  }
  return EBEN_OK;
}

extern "C" int eben_overlap_add_clips(const float* frames_buf, int64_t cols, const double* w2, float* out, int64_t out_floats, int win, int hop, int pad,
                                      const EbenOlaClip* rows, int nrows, void* stream) {
  EBEN_REQUIRE(frames_buf && w2 && out && rows, "overlap_add_clips: null pointer");
  EBEN_REQUIRE(cols > 0 && cols < (1ll << 31) && out_floats > 0 && win > 0 && hop > 0 && hop <= win && pad >= 0 && nrows > 0,
               "overlap_add_clips: %lld columns, %lld output floats, window %d, hop %d, pad %d, %d rows", (long long)cols, (long long)out_floats, win, hop,
               pad, nrows);
  EBEN_REQUIRE(((uintptr_t)w2 & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)frames_buf & 3) == 0, "overlap_add_clips: misaligned pointer");
  long long col_end = 0, dst_end = 0;
  int longest = 0;
  for (int i = 0; i < nrows; ++i) {
    const EbenOlaClip& r = rows[i];
    if (r.frames_out <= 0 || r.col < col_end || (long long)r.col + r.frames_out > cols)
      return fail(EBEN_EINVAL, "overlap_add_clips: row %d reads columns [%d, %lld) of %lld (ascending, disjoint)", i, r.col, (long long)r.col + r.frames_out,
                  (long long)cols);
    if (r.len_stretch <= 0 || r.dst_offset < dst_end || r.dst_offset + r.len_stretch > out_floats)
      return fail(EBEN_EINVAL, "overlap_add_clips: row %d writes %d samples at %lld of %lld (ascending, disjoint)", i, r.len_stretch, (long long)r.dst_offset,
                  (long long)out_floats);
    if (r.valid < 0 || r.valid > r.len_stretch || (long long)r.valid + pad > (long long)win + (long long)hop * (r.frames_out - 1))
      return fail(EBEN_EINVAL, "overlap_add_clips: row %d has %d valid samples of %d, %d frames", i, r.valid, r.len_stretch, r.frames_out);
    col_end = (long long)r.col + r.frames_out;
    dst_end = r.dst_offset + r.len_stretch;
    if (r.len_stretch > longest) longest = r.len_stretch;
  }
  int gx = ceil_div(longest + 3, 1024);
  if (gx > 256) gx = 256;
  for (int p0 = 0; p0 < nrows; p0 += CLIP_CHUNK) {
    const int cnt = nrows - p0 < CLIP_CHUNK ? nrows - p0 : CLIP_CHUNK;
    OlaClipTable T;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < cnt; ++i) T.rows[i] = rows[p0 + i];
    hipLaunchKernelGGL(ola_clips_kernel, dim3(gx, cnt), dim3(256), 0, as_stream(stream), T, frames_buf, w2, out, (long long)cols, win, hop, pad);
    EBEN_CHECK_LAUNCH("ola_clips_kernel");
  }
  return EBEN_OK;
}

extern "C" int eben_time_mask_clips(float* x, int rows, int t, const EbenMaskClip* clips, int nclips, void* stream) {
  EBEN_REQUIRE(x && clips, "time_mask_clips: null pointer");
  EBEN_REQUIRE(rows > 0 && t > 0 && nclips > 0, "time_mask_clips: %d rows of %d samples, %d masks", rows, t, nclips);
  EBEN_REQUIRE(((uintptr_t)x & 3) == 0, "time_mask_clips: misaligned pointer");
  int longest = 0;
  for (int i = 0; i < nclips; ++i) {
    const EbenMaskClip& c = clips[i];
    if (c.row < 0 || c.row >= rows) return fail(EBEN_EINVAL, "time_mask_clips: mask %d names row %d of %d", i, c.row, rows);
    if (c.first < 0 || c.count < 0 || (long long)c.first + c.count > t)
      return fail(EBEN_EINVAL, "time_mask_clips: mask %d covers [%d, %lld) of %d samples", i, c.first, (long long)c.first + c.count, t);
    if (c.count > longest) longest = c.count;
  }
  if (longest == 0) return EBEN_OK;
  int gx = ceil_div(longest + 3, 1024);
  if (gx > 256) gx = 256;
  for (int p0 = 0; p0 < nclips; p0 += CLIP_CHUNK) {
    const int cnt = nclips - p0 < CLIP_CHUNK ? nclips - p0 : CLIP_CHUNK;
    MaskClipTable T;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < cnt; ++i) T.rows[i] = clips[p0 + i];
    hipLaunchKernelGGL(mask_clips_kernel, dim3(gx, cnt), dim3(256), 0, as_stream(stream), T, x, t);
    EBEN_CHECK_LAUNCH("mask_clips_kernel");
  }
  return EBEN_OK;
}
