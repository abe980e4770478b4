// Per-row loss sums over ragged buffers: every clip's own value of the losses the test loop logs, from (rows, channels, l_buf)
// tensors whose rows end at lens[r] <= l_buf (ragged.hip: what lies behind a row's end is junk these kernels never read).
//
//   eben_fm_sums_rows         per embedding pair and row: sum |a - b|, sum |a| over the row's valid extent
//   eben_hinge_rows           per logits tensor and row: mean max(0, 1 - target x) over the row's valid extent
//   eben_stft_loss_sums_rows  per row: the three sums of eben_stft_loss_sums_ex over the row's first frames_of_row[r] frames
//   eben_clip_losses          the five per-row loss values from those sums, one launch
//
// Pointer tables travel by value in the kernel arguments; the row lengths stay on the device, so grids are sized from l_buf and the
// blocks past a row's end leave at once.  Every reduction is thread-serial, then block_sum_256, then one wave over the blocks'
// partials in a fixed order -- no atomics, the same bits on every run.  A length outside [0, l_buf] makes the row's result NaN and
// reads nothing.
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int RL_MAX = 32;        // table entries per launch (pairs / hinge terms)
constexpr int FMR_SPLIT = 32;     // blocks per (pair, row)
constexpr int FMR_CHUNK = 4096;   // samples of one channel a block takes at a time: 256 threads x four 16-byte loads per tensor

struct FmRowsTable {
  const float* a[RL_MAX];
  const float* b[RL_MAX];
  const int* lens[RL_MAX];
  int channels[RL_MAX];
  int l_buf[RL_MAX];
};

// block (s, r, p): the units u = s, s + FMR_SPLIT, ... of pair p's row r, a unit being one FMR_CHUNK-sample piece of one channel's valid
// extent.  Rows start anywhere (l_buf is arbitrary), so each piece finds its own 16-byte boundary: up to three scalar samples in front,
// whole f32x4 loads (four per tensor in flight per thread), up to three scalar samples behind -- when a and b are misaligned alike,
// as the two halves of one stacked tensor usually are; a scalar loop otherwise.
__global__ __launch_bounds__(256) void fm_rows_kernel(const FmRowsTable T, int rows, float* __restrict__ partial) {
  __shared__ float red[4];
  const int p = blockIdx.z, r = blockIdx.y, tid = threadIdx.x;
  const int C = T.channels[p], l_buf = T.l_buf[p];
  const int len = T.lens[p][r];
  const bool ok = len >= 0 && len <= l_buf;
  float s1 = 0.f, s2 = 0.f;
  if (ok && len > 0) {
    const int chunks = (len + FMR_CHUNK - 1) / FMR_CHUNK;
    const long long units = (long long)C * chunks;
    const float* a_row = T.a[p] + (long long)r * C * l_buf;
    const float* b_row = T.b[p] + (long long)r * C * l_buf;
    for (long long u = blockIdx.x; u < units; u += FMR_SPLIT) {
      const long long c = u / chunks;
      const int start = (int)(u - c * chunks) * FMR_CHUNK;
      const int n = len - start < FMR_CHUNK ? len - start : FMR_CHUNK;
      const float* pa = a_row + c * l_buf + start;
      const float* pb = b_row + c * l_buf + start;
      const unsigned ma = (unsigned)(reinterpret_cast<unsigned long long>(pa) >> 2) & 3u;
      const unsigned mb = (unsigned)(reinterpret_cast<unsigned long long>(pb) >> 2) & 3u;
      if (ma == mb) {
        int head = (int)((4u - ma) & 3u);
        if (head > n) head = n;
        const int nv = (n - head) >> 2;        // <= 1024
        const int tail0 = head + 4 * nv;
        if (tid < head) { const float av = pa[tid]; s1 += fabsf(av - pb[tid]); s2 += fabsf(av); }
        const f32x4* va = reinterpret_cast<const f32x4*>(pa + head);
        const f32x4* vb = reinterpret_cast<const f32x4*>(pb + head);
        f32x4 xa[4], xb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = tid + 256 * q;
          const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
          xa[q] = i < nv ? va[i] : zero;
          xb[q] = i < nv ? vb[i] : zero;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) { s1 += fabsf(xa[q][e] - xb[q][e]); s2 += fabsf(xa[q][e]); }
        if (tid < n - tail0) { const float av = pa[tail0 + tid]; s1 += fabsf(av - pb[tail0 + tid]); s2 += fabsf(av); }
      } else {
        for (int i = tid; i < n; i += 256) { const float av = pa[i]; s1 += fabsf(av - pb[i]); s2 += fabsf(av); }
      }
    }
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (tid == 0) {
    float* o = partial + (((long long)p * rows + r) * FMR_SPLIT + blockIdx.x) * 2;
    o[0] = ok ? s1 : NAN;
    o[1] = ok ? s2 : NAN;
  }
}

// one wave per (pair, row): the FMR_SPLIT partials in lane order
__global__ __launch_bounds__(64) void fm_rows_final_kernel(const float* __restrict__ partial, float* __restrict__ sums) {
  const long long pr = blockIdx.x;
  const int lane = threadIdx.x;
  float s1 = lane < FMR_SPLIT ? partial[(pr * FMR_SPLIT + lane) * 2 + 0] : 0.f;
  float s2 = lane < FMR_SPLIT ? partial[(pr * FMR_SPLIT + lane) * 2 + 1] : 0.f;
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { sums[2 * pr] = s1; sums[2 * pr + 1] = s2; }
}

struct HingeRowsTable {
  const float* x[RL_MAX];
  const int* lens[RL_MAX];
  int l_buf[RL_MAX];
  float target[RL_MAX];
};

// block (r, i): the logits of a row are a few hundred samples at most -- one block, one pass
__global__ __launch_bounds__(256) void hinge_rows_kernel(const HingeRowsTable T, int rows, float* __restrict__ out) {
  __shared__ float red[4];
  const int i = blockIdx.y, r = blockIdx.x;
  const int l_buf = T.l_buf[i];
  const int len = T.lens[i][r];
  const bool ok = len >= 0 && len <= l_buf;
  const float target = T.target[i];
  float s = 0.f;
  if (ok) {
    const float* x = T.x[i] + (long long)r * l_buf;
    for (int l = threadIdx.x; l < len; l += 256) s += fmaxf(0.f, 1.f - target * x[l]);
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[(long long)i * rows + r] = ok ? s / (float)len : NAN;
}

constexpr int STFTR_SPLIT = 32;   // blocks per row, as eben_stft_loss_sums_ex: a full row walks the same elements in the same order
struct StftRowsLayout { long long row_stride, bin_stride, im_off; };
__device__ __forceinline__ float stft_mag_rows(float re, float im, float eps) { return sqrtf(fmaxf(re * re + im * im, eps)); }

__global__ __launch_bounds__(256) void stft_sums_rows_kernel(const float* __restrict__ sx, const float* __restrict__ sy, int bins,
                                                             StftRowsLayout L, int frames, const int* __restrict__ frames_of_row, float eps,
                                                             float* __restrict__ partial) {
  __shared__ float red[4];
  const int r = blockIdx.y;
  const int fr = frames_of_row[r];
  const bool ok = fr >= 0 && fr <= frames;
  const long long base0 = (long long)r * L.row_stride;
  const long long im_off = L.im_off;
  const int n = ok ? bins * fr : 0;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += STFTR_SPLIT * 256) {
    const int k = i / fr;
    const long long at = base0 + (long long)k * L.bin_stride + (i - k * fr);
    const float xm = stft_mag_rows(sx[at], sx[at + im_off], eps);
    const float ym = stft_mag_rows(sy[at], sy[at + im_off], eps);
    const float d = ym - xm;
    s0 += d * d;
    s1 += ym * ym;
    s2 += fabsf(logf(xm) - logf(ym));
  }
  s0 = block_sum_256(s0, red);
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (threadIdx.x == 0) {
    float* o = partial + ((long long)r * STFTR_SPLIT + blockIdx.x) * 3;
    o[0] = ok ? s0 : NAN; o[1] = ok ? s1 : NAN; o[2] = ok ? s2 : NAN;
  }
}
__global__ __launch_bounds__(64) void stft_sums_rows_final_kernel(const float* __restrict__ partial, float* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    float v = lane < STFTR_SPLIT ? partial[((long long)r * STFTR_SPLIT + lane) * 3 + k] : 0.f;
    v = wave_sum(v);
    if (lane == 0) out[3 * r + k] = v;
  }
}

constexpr int CLIP_RES_MAX = 8;
struct ClipLossTable {
  const float* sums[CLIP_RES_MAX];
  const int* frames[CLIP_RES_MAX];
  int bins[CLIP_RES_MAX];
};

// thread = row: a few dozen divisions each
__global__ __launch_bounds__(64) void clip_losses_kernel(const ClipLossTable T, int n_res, const float* __restrict__ fm_sums, int npairs,
                                                        float fm_inv_count, const float* __restrict__ hinge, int nchains, int rows,
                                                        float* __restrict__ out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  float v = NAN;
  if (n_res > 0) {
    v = 0.f;
    for (int i = 0; i < n_res; ++i) {
      const float* s = T.sums[i] + 3LL * r;
      v += sqrtf(s[0] / s[1]) + s[2] / ((float)T.bins[i] * (float)T.frames[i][r]);
    }
    v /= (float)n_res;
  }
  out[r] = v;
  v = NAN;
  if (npairs > 0) {
    v = 0.f;
    for (int p = 0; p < npairs; ++p) {
      const float* s = fm_sums + ((long long)p * rows + r) * 2;
      v += s[0] / s[1];
    }
    v *= fm_inv_count;
  }
  out[rows + r] = v;
  for (int k = 0; k < 3; ++k) {
    v = NAN;
    if (nchains > 0) {
      v = 0.f;
      for (int c = 0; c < nchains; ++c) v += hinge[(long long)(3 * c + k) * rows + r];
      v /= (float)nchains;
    }
    out[(long long)(2 + k) * rows + r] = v;
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" size_t eben_fm_sums_rows_workspace(int npairs, int rows) {
  return npairs > 0 && rows > 0 ? sizeof(float) * 2 * FMR_SPLIT * (size_t)npairs * (size_t)rows : 0;
}

extern "C" int eben_fm_sums_rows(const void* const* ptrs, const int* channels, const int* l_bufs, const int32_t* const* lens, int npairs,
                                 int rows, float* partial_ws, size_t ws_bytes, float* sums, void* stream) {
  EBEN_REQUIRE(ptrs && channels && l_bufs && lens && partial_ws && sums, "fm_sums_rows: null pointer");
  EBEN_REQUIRE(npairs > 0 && npairs <= RL_MAX, "fm_sums_rows: 1..%d pairs, got %d", RL_MAX, npairs);
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "fm_sums_rows: 1..65535 rows, got %d", rows);
  EBEN_REQUIRE(aligned4(partial_ws) && aligned4(sums), "fm_sums_rows: misaligned pointer");
  if (ws_bytes < eben_fm_sums_rows_workspace(npairs, rows))
    return fail(EBEN_EWORKSPACE, "fm_sums_rows needs %zu workspace bytes", eben_fm_sums_rows_workspace(npairs, rows));
  FmRowsTable T;
  for (int i = 0; i < npairs; ++i) {
    EBEN_REQUIRE(ptrs[2 * i] && ptrs[2 * i + 1] && lens[i], "fm_sums_rows: pair %d has a null pointer", i);
    EBEN_REQUIRE(aligned4(ptrs[2 * i]) && aligned4(ptrs[2 * i + 1]) && aligned4(lens[i]), "fm_sums_rows: pair %d has a misaligned pointer", i);
    EBEN_REQUIRE(channels[i] > 0 && l_bufs[i] > 0, "fm_sums_rows: pair %d has %d channels of %d samples", i, channels[i], l_bufs[i]);
    T.a[i] = static_cast<const float*>(ptrs[2 * i]);
    T.b[i] = static_cast<const float*>(ptrs[2 * i + 1]);
    T.lens[i] = lens[i];
    T.channels[i] = channels[i];
    T.l_buf[i] = l_bufs[i];
  }
  hipLaunchKernelGGL(fm_rows_kernel, dim3(FMR_SPLIT, rows, npairs), dim3(256), 0, as_stream(stream), T, rows, partial_ws);
  EBEN_CHECK_LAUNCH("fm_rows_kernel");
  hipLaunchKernelGGL(fm_rows_final_kernel, dim3((unsigned)npairs * (unsigned)rows), dim3(64), 0, as_stream(stream), partial_ws, sums);
  EBEN_CHECK_LAUNCH("fm_rows_final_kernel");
  return EBEN_OK;
}

extern "C" int eben_hinge_rows(const void* const* xs, const int* l_bufs, const float* targets, const int32_t* const* lens, int n, int rows,
                               float* out, void* stream) {
  EBEN_REQUIRE(xs && l_bufs && targets && lens && out, "hinge_rows: null pointer");
  EBEN_REQUIRE(n > 0 && n <= RL_MAX, "hinge_rows: 1..%d terms, got %d", RL_MAX, n);
  EBEN_REQUIRE(rows > 0, "hinge_rows: %d rows", rows);
  EBEN_REQUIRE(aligned4(out), "hinge_rows: misaligned pointer");
  HingeRowsTable T;
  for (int i = 0; i < n; ++i) {
    EBEN_REQUIRE(xs[i] && lens[i], "hinge_rows: term %d has a null pointer", i);
    EBEN_REQUIRE(aligned4(xs[i]) && aligned4(lens[i]), "hinge_rows: term %d has a misaligned pointer", i);
    EBEN_REQUIRE(l_bufs[i] > 0, "hinge_rows: term %d has rows of %d samples", i, l_bufs[i]);
    T.x[i] = static_cast<const float*>(xs[i]);
    T.lens[i] = lens[i];
    T.l_buf[i] = l_bufs[i];
    T.target[i] = targets[i];
  }
  hipLaunchKernelGGL(hinge_rows_kernel, dim3(rows, n), dim3(256), 0, as_stream(stream), T, rows, out);
  EBEN_CHECK_LAUNCH("hinge_rows_kernel");
  return EBEN_OK;
}

extern "C" size_t eben_stft_loss_sums_rows_workspace(int rows) { return sizeof(float) * 3 * (size_t)STFTR_SPLIT * (rows > 0 ? rows : 0); }

extern "C" int eben_stft_loss_sums_rows(const float* spec_x, const float* spec_y, int rows, int bins, int frames,
                                        const int32_t* frames_of_row, long long row_stride, long long bin_stride, long long im_off, float eps,
                                        float* partial_ws, size_t ws_bytes, float* out, void* stream) {
  EBEN_REQUIRE(spec_x && spec_y && frames_of_row && out && partial_ws, "stft_loss_sums_rows: null pointer");
  EBEN_REQUIRE(aligned4(spec_x) && aligned4(spec_y) && aligned4(frames_of_row) && aligned4(out) && aligned4(partial_ws),
               "stft_loss_sums_rows: misaligned pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && bins > 0 && frames > 0 && bin_stride >= frames && row_stride >= 0 && im_off >= 0,
               "stft_loss_sums_rows: rows %d, bins %d, frames %d, strides %lld / %lld / %lld", rows, bins, frames, row_stride, bin_stride, im_off);
  EBEN_REQUIRE((long long)bins * frames <= 0x7fffffffLL, "stft_loss_sums_rows: %d bins x %d frames", bins, frames);
  if (ws_bytes < eben_stft_loss_sums_rows_workspace(rows))
    return fail(EBEN_EWORKSPACE, "stft_loss_sums_rows needs %zu workspace bytes", eben_stft_loss_sums_rows_workspace(rows));
  const StftRowsLayout L{row_stride, bin_stride, im_off};
  hipLaunchKernelGGL(stft_sums_rows_kernel, dim3(STFTR_SPLIT, rows), dim3(256), 0, as_stream(stream), spec_x, spec_y, bins, L, frames,
                     frames_of_row, eps, partial_ws);
  EBEN_CHECK_LAUNCH("stft_sums_rows_kernel");
  hipLaunchKernelGGL(stft_sums_rows_final_kernel, dim3(rows), dim3(64), 0, as_stream(stream), partial_ws, out);
  EBEN_CHECK_LAUNCH("stft_sums_rows_final_kernel");
  return EBEN_OK;
}

extern "C" int eben_clip_losses(const void* const* stft_sums, const int32_t* const* frames_of_row, const int* bins, int n_res,
                                const float* fm_sums, int npairs, float fm_inv_count, const float* hinge, int nchains, int rows, float* out,
                                void* stream) {
  EBEN_REQUIRE(out && aligned4(out) && rows > 0, "clip_losses: out %p, rows %d", (void*)out, rows);
  EBEN_REQUIRE(n_res >= 0 && n_res <= CLIP_RES_MAX && npairs >= 0 && nchains >= 0, "clip_losses: %d resolutions (<= %d), %d pairs, %d chains",
               n_res, CLIP_RES_MAX, npairs, nchains);
  EBEN_REQUIRE(n_res == 0 || (stft_sums && frames_of_row && bins), "clip_losses: null resolution table");
  EBEN_REQUIRE(npairs == 0 || (fm_sums && aligned4(fm_sums)), "clip_losses: null or misaligned fm_sums");
  EBEN_REQUIRE(nchains == 0 || (hinge && aligned4(hinge)), "clip_losses: null or misaligned hinge");
  ClipLossTable T{};
  for (int i = 0; i < n_res; ++i) {
    EBEN_REQUIRE(stft_sums[i] && frames_of_row[i] && aligned4(stft_sums[i]) && aligned4(frames_of_row[i]) && bins[i] > 0,
                 "clip_losses: resolution %d has a null or misaligned pointer or %d bins", i, bins[i]);
    T.sums[i] = static_cast<const float*>(stft_sums[i]);
    T.frames[i] = frames_of_row[i];
    T.bins[i] = bins[i];
  }
  hipLaunchKernelGGL(clip_losses_kernel, dim3(ceil_div(rows, 64)), dim3(64), 0, as_stream(stream), T, n_res, fm_sums, npairs, fm_inv_count,
                     hinge, nchains, rows, out);
  EBEN_CHECK_LAUNCH("clip_losses_kernel");
  return EBEN_OK;
}
