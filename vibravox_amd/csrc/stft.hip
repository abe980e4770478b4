// stft.hip -- the streaming kernels of the multi-resolution STFT loss (gfx950): framing of the reflect-padded signal (dense and
// folded), the bf16x3 operand split, the magnitude-loss sums / total / gradient of the multi_stft.yaml term set, and the overlap-add
// adjoint of the framing.  The windowed-DFT contractions between them are pw_gemm.hip / the pointwise tap-conv; the weighted / mel /
// L2 term set is stft_terms.hip; the per-row sums over ragged buffers are ragged_losses.hip.
#include "common.h"

#include <cfloat>
#include <cstdlib>

namespace eben {

// ---------------------------------------------------------------------------------------------
// STFT magnitude losses (auraloss STFTLoss: spectral convergence + log-magnitude L1)
// spec: (rows, 2*bins_pad, frames), re in channel k, im in channel bins_pad+k.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float stft_mag(float re, float im, float eps) { return sqrtf(fmaxf(re * re + im * im, eps)); }

// two-level, order-deterministic: STFT_SPLIT blocks per row write partial sums, one wave per row adds them
constexpr int STFT_SPLIT = 32;
// element (row r, bin k, frame f) of a spectrum sits at r*row_stride + k*bin_stride + f (real part; imaginary at + im_off):
// (rows, 2*bins_pad, frames) tensors and the flat (2*bins, rows*frames) GEMM output are both of that form
struct StftLayout { long long row_stride, bin_stride, im_off; };

__global__ __launch_bounds__(256) void stft_sums_kernel(const float* __restrict__ sx, const float* __restrict__ sy, int bins,
                                                        StftLayout L, int frames, float eps, float* __restrict__ partial) {
  __shared__ float red[4];
  const int r = blockIdx.y;
  const long long base0 = (long long)r * L.row_stride;
  const long long im_off = L.im_off;
  const int n = bins * frames;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += STFT_SPLIT * 256) {
    const int k = i / frames;
    const long long base = base0 + (long long)k * (L.bin_stride - frames);   // + i = k*bin_stride + f
    const float xm = stft_mag(sx[base + i], sx[base + im_off + i], eps);
    const float ym = stft_mag(sy[base + i], sy[base + im_off + i], eps);
    const float d = ym - xm;
    s0 += d * d;
    s1 += ym * ym;
    s2 += fabsf(logf(xm) - logf(ym));
  }
  s0 = block_sum_256(s0, red);
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (threadIdx.x == 0) {
    float* o = partial + ((long long)r * STFT_SPLIT + blockIdx.x) * 3;
    o[0] = s0; o[1] = s1; o[2] = s2;
  }
}
__global__ __launch_bounds__(64) void stft_sums_final_kernel(const float* __restrict__ partial, float* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    float v = lane < STFT_SPLIT ? partial[((long long)r * STFT_SPLIT + lane) * 3 + k] : 0.f;
    v = wave_sum(v);
    if (lane == 0) out[3 * r + k] = v;
  }
}

// The loss value from the per-row sums of all resolutions in one launch (auraloss: per resolution mean_r sqrt(s0 / s1) [spectral
// convergence] + sum_r s2 / (rows bins frames) [log magnitude], then the mean over the resolutions): ~8 one-element torch kernels
// per resolution otherwise, on the main stream.  One wave; fixed reduction order.
constexpr int STFT_TOTAL_MAX = 8;
struct StftTotalTable { const float* sums[STFT_TOTAL_MAX]; float inv_count[STFT_TOTAL_MAX]; };
__global__ __launch_bounds__(64) void stft_total_kernel(const StftTotalTable T, int n, int rows, float* __restrict__ out) {
  const int lane = threadIdx.x;
  float total = 0.f;
  for (int p = 0; p < n; ++p) {
    float sc = 0.f, lg = 0.f;
    for (int r = lane; r < rows; r += 64) {
      sc += sqrtf(T.sums[p][3 * r] / T.sums[p][3 * r + 1]);
      lg += T.sums[p][3 * r + 2];
    }
    sc = wave_sum(sc);
    lg = wave_sum(lg);
    total += sc / (float)rows + lg * T.inv_count[p];
  }
  if (lane == 0) out[0] = total / (float)n;
}

__global__ __launch_bounds__(256) void stft_bwd_kernel(const float* __restrict__ sx, const float* __restrict__ sy, int rows, int bins,
                                                       StftLayout L, StftLayout LO, int frames, float eps, const float* __restrict__ sums,
                                                       const float* __restrict__ gout, float scale, float* __restrict__ dsx) {
  const int r = blockIdx.y;
  const long long im_off = L.im_off;
  const int n = bins * frames;
  const float g = gout[0] * scale;
  // d ||Y - X|| is taken as 0 where ||Y - X|| = 0 (a row whose spectra agree exactly), as torch.linalg.vector_norm's backward does:
  // the floor keeps c_sc finite there, so c_sc * (xm - ym = 0) is 0 rather than inf * 0 = NaN; it leaves every sum >= FLT_MIN as it is
  const float c_sc = g / ((float)rows * sqrtf(fmaxf(sums[3 * r], FLT_MIN)) * sqrtf(sums[3 * r + 1]));
  const float c_lg = g / ((float)rows * (float)bins * (float)frames);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int k = i / frames;
    const long long base = (long long)r * L.row_stride + (long long)k * (L.bin_stride - frames);
    const long long obase = (long long)r * LO.row_stride + (long long)k * (LO.bin_stride - frames);
    const float re = sx[base + i], im = sx[base + im_off + i];
    const float p = re * re + im * im;
    const float xm = sqrtf(fmaxf(p, eps));
    const float ym = stft_mag(sy[base + i], sy[base + im_off + i], eps);
    const float dl = logf(xm) - logf(ym);
    const float sg = (dl > 0.f) - (dl < 0.f);
    float dmag = c_sc * (xm - ym) + c_lg * sg / xm;
    dmag = p >= eps ? dmag / xm : 0.f;   // d sqrt(clamp(p)) / dp * 2  -> (re, im) / mag
    dsx[obase + i] = dmag * re;
    dsx[obase + LO.im_off + i] = dmag * im;
  }
}

// ---------------------------------------------------------------------------------------------
// overlap-add: adjoint of framing a reflect-padded signal (STFT backward).
// frames_buf (B, win, frames) holds per-frame sample gradients; padded coordinate q receives
// sum_f buf[q + pad - f*hop, f]; the reflect padding folds q<0 and q>=lx back into [0, lx).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ola_gather(const float* __restrict__ buf, int q, int win, int frames, int hop, int pad, long long j_stride) {
  const int s = q + pad;  // = f*hop + j
  if (s < 0) return 0.f;
  int fmax = s / hop;
  if (fmax > frames - 1) fmax = frames - 1;
  int fmin = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
  float acc = 0.f;
  for (int f = fmin; f <= fmax; ++f) acc += buf[(long long)(s - f * hop) * j_stride + f];
  return acc;
}
// Folded form (eben_stft_frames_folded's adjoint): buf holds 2*(win/2) rows [dE ; dO]; window sample j = h + m gets
// dE[|m|] + sign(m) dO[|m|], the centre dE[0], sample 0 (zero window weight) nothing.
__device__ __forceinline__ float ola_gather_folded(const float* __restrict__ buf, int q, int win, int frames, int hop, int pad, long long j_stride) {
  const int s = q + pad;
  if (s < 0) return 0.f;
  const int h = win >> 1;
  int fmax = s / hop;
  if (fmax > frames - 1) fmax = frames - 1;
  int fmin = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
  float acc = 0.f;
  for (int f = fmin; f <= fmax; ++f) {
    const int j = s - f * hop;
    const int m = j - h, am = m < 0 ? -m : m;
    if (j == 0) continue;
    const float e = buf[(long long)am * j_stride + f];
    const float o = m != 0 ? buf[(long long)(h + am) * j_stride + f] : 0.f;
    acc += m < 0 ? e - o : e + o;
  }
  return acc;
}
__global__ __launch_bounds__(256) void overlap_add_folded_kernel(const float* __restrict__ buf, float* __restrict__ x, int lx, int win,
                                                                 int frames, int hop, int pad, int accumulate,
                                                                 long long row_stride, long long j_stride) {
  const int b = blockIdx.y;
  const float* bb = buf + (long long)b * row_stride;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < lx; u += gridDim.x * 256) {
    float v = ola_gather_folded(bb, u, win, frames, hop, pad, j_stride);
    if (u >= 1 && u <= pad) v += ola_gather_folded(bb, -u, win, frames, hop, pad, j_stride);
    if (u <= lx - 2 && 2 * (lx - 1) - u <= lx - 1 + pad) v += ola_gather_folded(bb, 2 * (lx - 1) - u, win, frames, hop, pad, j_stride);
    const long long i = (long long)b * lx + u;
    if (accumulate) v += x[i];
    x[i] = v;
  }
}

// The same sums from an LDS tile.  The kernel above gathers straight from the buffer with the lanes on consecutive samples, i.e. on
// consecutive ROWS of it (a row = one window sample of every frame): 64 cache lines per load, ten loads per output -- 34-50 us for the
// 20 MB of one resolution.  Here a block owns OLA_U consecutive samples of one item: the frames that reach them (+ the ones the reflected
// ends fold in) are read once, row segment by row segment, unfolded into tile[frame][window sample] = dE[|m|] +- dO[|m|], and every output
// sums its <= win / hop + 1 tile entries (lanes = consecutive samples = consecutive tile entries).  Same terms in the same order: bit-identical.
constexpr int OLA_U = 512;
__device__ __forceinline__ float ola_tile_gather(const float* __restrict__ tile, int q, int win, int frames, int hop, int pad, int f_lo) {
  const int s = q + pad;  // = f*hop + j
  if (s < 0) return 0.f;
  int fmax = s / hop;
  if (fmax > frames - 1) fmax = frames - 1;
  const int fmin = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
  float acc = 0.f;
  for (int f = fmin; f <= fmax; ++f) acc += tile[(f - f_lo) * win + (s - f * hop)];
  return acc;
}
__global__ __launch_bounds__(256) void overlap_add_folded_t_kernel(const float* __restrict__ buf, float* __restrict__ x, int lx, int win,
                                                                   int frames, int hop, int pad, int accumulate, long long row_stride,
                                                                   long long j_stride, int fcap) {
  extern __shared__ __attribute__((aligned(16))) float ola_tile[];   // fcap x win
  const int b = blockIdx.y, u0 = blockIdx.x * OLA_U, tid = threadIdx.x;
  const int h = win >> 1;
  const int qlo = u0, qhi = (u0 + OLA_U < lx ? u0 + OLA_U : lx) - 1;
  int f_lo = qlo <= pad ? 0 : (qlo + pad - win + hop) / hop;   // = ceil((qlo + pad - win + 1) / hop) for a positive numerator
  if (f_lo < 0) f_lo = 0;
  int smax = qhi + pad;
  if (qhi >= lx - 1 - pad) {   // samples whose mirror image past the end folds back onto them
    const int ulo = qlo > lx - 1 - pad ? qlo : lx - 1 - pad;
    const int sm = 2 * (lx - 1) - ulo + pad;
    if (sm > smax) smax = sm;
  }
  int f_hi = smax / hop;
  if (f_hi > frames - 1) f_hi = frames - 1;
  int nf = f_hi - f_lo + 1;
  if (nf > fcap) nf = fcap;   // never (fcap is sized for the worst tile)
  const float* bb = buf + (long long)b * row_stride;
  // unfold: entry (frame fl, m) of the two row blocks -> window samples h + m and h - m of that frame
  // thread = (frame fl = tid % nfp, rows m = tid / nfp, + 256 / nfp, ...), nfp = the power of two >= nf: no division, the loads of four
  // rows in flight together
  int nfp = 1;
  while (nfp < nf) nfp <<= 1;
  const int fl = tid & (nfp - 1), mstep = 256 / nfp;
  if (fl < nf) {
    const float* col = bb + f_lo + fl;
    float* row = ola_tile + fl * win;
    for (int m0 = tid / nfp; m0 < h; m0 += 4 * mstep) {
      float e[4], o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = m0 + k * mstep;
        const int mc = m < h ? m : 0;
        e[k] = col[(long long)mc * j_stride];
        o[k] = col[(long long)(h + mc) * j_stride];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = m0 + k * mstep;
        if (m >= h) continue;
        if (m) { row[h + m] = e[k] + o[k]; row[h - m] = e[k] - o[k]; }
        else { row[h] = e[k] + 0.f; row[0] = 0.f; }   // the centre sample has no odd part; window sample 0 carries no weight
      }
    }
  }
  __syncthreads();
  for (int u = u0 + tid; u <= qhi; u += 256) {
    float v = ola_tile_gather(ola_tile, u, win, frames, hop, pad, f_lo);
    if (u >= 1 && u <= pad) v += ola_tile_gather(ola_tile, -u, win, frames, hop, pad, f_lo);
    if (u <= lx - 2 && 2 * (lx - 1) - u <= lx - 1 + pad) v += ola_tile_gather(ola_tile, 2 * (lx - 1) - u, win, frames, hop, pad, f_lo);
    const long long i = (long long)b * lx + u;
    if (accumulate) v += x[i];
    x[i] = v;
  }
}

// buf element (item b, sample j of the window, frame f) sits at b*row_stride + j*j_stride + f
__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ buf, float* __restrict__ x, int lx, int win,
                                                          int frames, int hop, int pad, int reflect, int accumulate,
                                                          long long row_stride, long long j_stride) {
  const int b = blockIdx.y;
  const float* bb = buf + (long long)b * row_stride;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < lx; u += gridDim.x * 256) {
    float v = ola_gather(bb, u, win, frames, hop, pad, j_stride);
    if (reflect) {
      if (u >= 1 && u <= pad) v += ola_gather(bb, -u, win, frames, hop, pad, j_stride);
      if (u <= lx - 2 && 2 * (lx - 1) - u <= lx - 1 + pad) v += ola_gather(bb, 2 * (lx - 1) - u, win, frames, hop, pad, j_stride);
    }
    const long long i = (long long)b * lx + u;
    if (accumulate) v += x[i];
    x[i] = v;
  }
}

}  // namespace eben

using namespace eben;

extern "C" size_t eben_stft_loss_sums_workspace(int rows) { return sizeof(float) * 3 * (size_t)STFT_SPLIT * (rows > 0 ? rows : 0); }
extern "C" int eben_stft_loss_sums_ex(const float* spec_x, const float* spec_y, int rows, int bins, int frames, long long row_stride,
                                      long long bin_stride, long long im_off, float eps, float* partial_ws, size_t ws_bytes, float* out,
                                      void* stream) {
  EBEN_REQUIRE(spec_x && spec_y && out && partial_ws && rows > 0 && bins > 0 && frames > 0 && bin_stride >= frames, "bad stft_loss arguments");
  if (ws_bytes < eben_stft_loss_sums_workspace(rows)) return fail(EBEN_EWORKSPACE, "stft_loss_sums needs %zu workspace bytes", eben_stft_loss_sums_workspace(rows));
  const StftLayout L{row_stride, bin_stride, im_off};
  hipLaunchKernelGGL(stft_sums_kernel, dim3(STFT_SPLIT, rows), dim3(256), 0, as_stream(stream), spec_x, spec_y, bins, L, frames, eps,
                     partial_ws);
  EBEN_CHECK_LAUNCH("stft_sums_kernel");
  hipLaunchKernelGGL(stft_sums_final_kernel, dim3(rows), dim3(64), 0, as_stream(stream), partial_ws, out);
  EBEN_CHECK_LAUNCH("stft_sums_final_kernel");
  return EBEN_OK;
}
extern "C" int eben_stft_loss_total(const void* const* sums, const float* inv_counts, int n, int rows, float* out, void* stream) {
  EBEN_REQUIRE(sums && inv_counts && out && n > 0 && n <= STFT_TOTAL_MAX && rows > 0, "stft_loss_total: 1..%d resolutions", STFT_TOTAL_MAX);
  StftTotalTable T;
  for (int i = 0; i < n; ++i) {
    EBEN_REQUIRE(sums[i], "stft_loss_total: null sums %d", i);
    T.sums[i] = static_cast<const float*>(sums[i]); T.inv_count[i] = inv_counts[i];
  }
  hipLaunchKernelGGL(stft_total_kernel, dim3(1), dim3(64), 0, as_stream(stream), T, n, rows, out);
  EBEN_CHECK_LAUNCH("stft_total_kernel");
  return EBEN_OK;
}
extern "C" int eben_stft_loss_bwd_ex(const float* spec_x, const float* spec_y, int rows, int bins, int frames, long long row_stride,
                                     long long bin_stride, long long im_off, float eps, const float* sums, const float* gout, float scale,
                                     float* dspec_x, long long out_row_stride, long long out_bin_stride, long long out_im_off, void* stream) {
  EBEN_REQUIRE(spec_x && spec_y && sums && gout && dspec_x && rows > 0 && bins > 0 && frames > 0, "bad stft_loss arguments");
  EBEN_REQUIRE(bin_stride >= frames && out_bin_stride >= frames, "bad stft_loss strides");
  const int nb = grid_for((size_t)bins * frames, 64);
  const StftLayout L{row_stride, bin_stride, im_off}, LO{out_row_stride, out_bin_stride, out_im_off};
  hipLaunchKernelGGL(stft_bwd_kernel, dim3(nb, rows), dim3(256), 0, as_stream(stream), spec_x, spec_y, rows, bins, L, LO, frames,
                     eps, sums, gout, scale, dspec_x);
  EBEN_CHECK_LAUNCH("stft_bwd_kernel");
  return EBEN_OK;
}

extern "C" int eben_overlap_add_ex(const float* frames_buf, float* x, int batch, int lx, int win, int frames, int hop, int pad,
                                   int reflect, int accumulate, long long row_stride, long long j_stride, void* stream) {
  EBEN_REQUIRE(frames_buf && x && batch > 0 && lx > 0 && win > 0 && frames > 0 && hop > 0 && pad >= 0, "bad overlap_add arguments");
  EBEN_REQUIRE(!reflect || pad < lx, "reflect padding must be smaller than the signal");
  hipLaunchKernelGGL(overlap_add_kernel, dim3(grid_for((size_t)lx, 256), batch), dim3(256), 0, as_stream(stream), frames_buf, x, lx,
                     win, frames, hop, pad, reflect, accumulate, row_stride, j_stride);
  EBEN_CHECK_LAUNCH("overlap_add_kernel");
  return EBEN_OK;
}

extern "C" int eben_overlap_add_folded_tiled(int lx, int win, int hop, int pad) {
  static const bool tiled = !(getenv("EBEN_OLA_TILED") && atoi(getenv("EBEN_OLA_TILED")) == 0);
  if (lx <= 0 || win <= 0 || hop <= 0 || pad < 0) return 0;
  const int fcap = OLA_U / hop + win / hop + pad / hop + 4;
  const size_t lds = sizeof(float) * (size_t)fcap * win;
  // fcap <= 256: the tile's unfold spreads its <= fcap frames over the 256 lanes (mstep = 256 / nfp would be 0 past that, at hop 1-2)
  return tiled && fcap <= 256 && lds <= 64 * 1024 && pad < win && lx > 2 * pad;
}
extern "C" int eben_overlap_add_folded(const float* frames_buf, float* x, int batch, int lx, int win, int frames, int hop, int pad,
                                       int accumulate, long long row_stride, long long j_stride, void* stream) {
  EBEN_REQUIRE(frames_buf && x && batch > 0 && lx > 0 && win > 0 && (win & 1) == 0 && frames > 0 && hop > 0 && pad >= 0 && pad < lx,
               "bad overlap_add_folded arguments");
  const int fcap = OLA_U / hop + win / hop + pad / hop + 4;
  const size_t lds = sizeof(float) * (size_t)fcap * win;
  if (eben_overlap_add_folded_tiled(lx, win, hop, pad)) {
    hipLaunchKernelGGL(overlap_add_folded_t_kernel, dim3(ceil_div(lx, OLA_U), batch), dim3(256), lds, as_stream(stream), frames_buf, x, lx, win,
                       frames, hop, pad, accumulate, row_stride, j_stride, fcap);
    EBEN_CHECK_LAUNCH("overlap_add_folded_t_kernel");
    return EBEN_OK;
  }
  hipLaunchKernelGGL(overlap_add_folded_kernel, dim3(grid_for((size_t)lx, 256), batch), dim3(256), 0, as_stream(stream), frames_buf, x,
                     lx, win, frames, hop, pad, accumulate, row_stride, j_stride);
  EBEN_CHECK_LAUNCH("overlap_add_folded_kernel");
  return EBEN_OK;
}

// ---------------------------------------------------------------------------------------------
// STFT framing (im2col of torch.stft(center=True, pad_mode="reflect")): out[j, r*frames + f] = sig[r, reflect(f*hop + j - pad)].
// The (win, rows*frames) matrix makes the windowed DFT ONE dense GEMM over all items' frames (a pointwise tap-conv
// with batch 1): no N-tile padding per item (134 frames per item fill 52 % of two 128-column tiles).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ sig, float* __restrict__ out, int rows, int t,
                                                          int win, int hop, int pad, int frames) {
  const int j = blockIdx.y;
  const long long cols = (long long)rows * frames;
  float* o = out + (long long)j * cols;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cols; c += (long long)gridDim.x * 256) {
    const int r = (int)(c / frames), f = (int)(c - (long long)r * frames);
    int q = f * hop + j - pad;
    q = q < 0 ? -q : q;
    q = q >= t ? 2 * (t - 1) - q : q;
    o[c] = sig[(long long)r * t + q];
  }
}
// Folded framing.  A window symmetric about sample h = win/2 of the frame (hann, periodic: w[0] = 0, w[h+m] = w[h-m]) centred
// in the DFT makes the real part a functional of the EVEN part of the frame about h and the imaginary part one of its ODD part:
//   E[m] = s[h+m] + s[h-m] (m >= 1), E[0] = s[h];  O[m] = s[h+m] - s[h-m], O[0] = 0        (m < h; sample 0 has zero weight)
//   Re X[k] = sum_m basis[k, h+m] E[m],   Im X[k] = sum_m basis[bins+k, h+m] O[m]
// -- a pointwise conv with TWO GROUPS of h channels instead of one of win: half the products.  split = 1 writes each group as
// 3h rows [hi ; lo ; hi] with hi = bf16(v), lo = bf16(v - hi) (both exactly representable in bf16): against weight rows
// [W_hi ; W_hi ; W_lo] a bf16-operand MFMA contraction with fp32 accumulation returns v.W to ~2^-17 relative (the dropped
// lo.lo and residual terms) -- "bf16x3".
__device__ __forceinline__ float bf16_rne(float v) {
  unsigned u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xffff0000u);
}
__global__ __launch_bounds__(256) void stft_frames_folded_kernel(const float* __restrict__ sig, float* __restrict__ out, int rows, int t,
                                                                 int win, int hop, int pad, int frames, int split) {
  const int m = blockIdx.y, h = win >> 1;
  const long long cols = (long long)rows * frames;
  const int nsub = split ? 3 : 1;
  float* oe = out + (long long)m * cols;
  float* oo = out + ((long long)nsub * h + m) * cols;
  const long long sub = (long long)h * cols;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cols; c += (long long)gridDim.x * 256) {
    const int r = (int)(c / frames), f = (int)(c - (long long)r * frames);
    int q1 = f * hop + h + m - pad, q2 = f * hop + h - m - pad;
    q1 = q1 < 0 ? -q1 : q1; q1 = q1 >= t ? 2 * (t - 1) - q1 : q1;
    q2 = q2 < 0 ? -q2 : q2; q2 = q2 >= t ? 2 * (t - 1) - q2 : q2;
    const float a = sig[(long long)r * t + q1], b = sig[(long long)r * t + q2];
    const float e = m ? a + b : a, o = m ? a - b : 0.f;
    if (split) {
      const float eh = bf16_rne(e), oh = bf16_rne(o);
      oe[c] = eh; oe[c + sub] = bf16_rne(e - eh); oe[c + 2 * sub] = eh;
      oo[c] = oh; oo[c + sub] = bf16_rne(o - oh); oo[c + 2 * sub] = oh;
    } else {
      oe[c] = e; oo[c] = o;
    }
  }
}
// The same rows through an LDS transpose (split = 0): the kernel above reads the signal with the lanes on consecutive FRAMES, i.e. hop
// samples apart -- 64 cache lines per load instruction, 30-44 us for the 40 MB of one resolution.  Here a block owns (item, 64 frames, 64
// values of m): its loads run along m (consecutive samples: s[.. + m] ascending, s[.. - m] descending), the sums go through a 64 x 65 tile,
// its stores run along the frames (256 contiguous bytes per row).  Same sums of the same samples: bit-identical.
__global__ __launch_bounds__(256) void stft_frames_folded_t_kernel(const float* __restrict__ sig, float* __restrict__ out, int rows, int t,
                                                                   int win, int hop, int pad, int frames) {
  __shared__ float te[64][65], to[64][65];
  const int h = win >> 1;
  const int f0 = blockIdx.x * 64, m0 = blockIdx.y * 64, r = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cols = (long long)rows * frames;
  const float* s = sig + (long long)r * t;
  const int m = m0 + lane;
  float av[16], bv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {   // the 32 loads of this thread first: all in flight together
    const int f = f0 + wave + 4 * k;
    const bool ok = f < frames && m < h;
    int q1 = f * hop + h + m - pad, q2 = f * hop + h - m - pad;
    q1 = q1 < 0 ? -q1 : q1; q1 = q1 >= t ? 2 * (t - 1) - q1 : q1;
    q2 = q2 < 0 ? -q2 : q2; q2 = q2 >= t ? 2 * (t - 1) - q2 : q2;
    av[k] = ok ? s[q1] : 0.f;
    bv[k] = ok ? s[q2] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int fl = wave + 4 * k;
    te[lane][fl] = m ? av[k] + bv[k] : av[k];
    to[lane][fl] = m ? av[k] - bv[k] : 0.f;
  }
  __syncthreads();
  const int f = f0 + lane;
  if (f >= frames) return;
  float* oe = out + (long long)r * frames + f;
  float* oo = oe + (long long)h * cols;
  for (int ml = wave; ml < 64 && m0 + ml < h; ml += 4) {
    oe[(long long)(m0 + ml) * cols] = te[ml][lane];
    oo[(long long)(m0 + ml) * cols] = to[ml][lane];
  }
}
extern "C" int eben_stft_frames_folded(const float* sig, float* out, int rows, int t, int win, int hop, int pad, int frames, int split,
                                       void* stream) {
  EBEN_REQUIRE(sig && out && rows > 0 && t > 1 && win > 1 && (win & 1) == 0 && hop > 0 && pad >= 0 && pad < t && frames > 0,
               "bad stft_frames_folded arguments");
  EBEN_REQUIRE((frames - 1) * hop + win - 1 - pad <= 2 * (t - 1), "stft_frames_folded: frames reach past the reflected signal");
  static const bool transposed = !(getenv("EBEN_STFT_FRAMES_T") && atoi(getenv("EBEN_STFT_FRAMES_T")) == 0);
  if (!split && transposed && rows <= 65535 && ceil_div(win / 2, 64) <= 65535) {
    hipLaunchKernelGGL(stft_frames_folded_t_kernel, dim3(ceil_div(frames, 64), ceil_div(win / 2, 64), rows), dim3(256), 0, as_stream(stream), sig,
                       out, rows, t, win, hop, pad, frames);
    EBEN_CHECK_LAUNCH("stft_frames_folded_t_kernel");
    return EBEN_OK;
  }
  hipLaunchKernelGGL(stft_frames_folded_kernel, dim3(grid_for((size_t)rows * frames, 64), win / 2), dim3(256), 0, as_stream(stream), sig,
                     out, rows, t, win, hop, pad, frames, split);
  EBEN_CHECK_LAUNCH("stft_frames_folded_kernel");
  return EBEN_OK;
}

// out (groups * 3 * R, cols) = per group [hi ; lo ; hi] of in (groups * R, cols): the bf16x3 operand of a gradient GEMM
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ in, float* __restrict__ out, int R, long long cols) {
  const int row = blockIdx.y;               // g * R + r
  const int g = row / R, r = row - g * R;
  const float* src = in + (long long)row * cols;
  float* dst = out + ((long long)g * 3 * R + r) * cols;
  const long long sub = (long long)R * cols;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cols; c += (long long)gridDim.x * 256) {
    const float v = src[c], hi = bf16_rne(v);
    dst[c] = hi; dst[c + sub] = bf16_rne(v - hi); dst[c + 2 * sub] = hi;
  }
}
extern "C" int eben_split3(const float* in, float* out, int groups, int rows_per_group, long long cols, void* stream) {
  EBEN_REQUIRE(in && out && groups > 0 && rows_per_group > 0 && cols > 0 && (long long)groups * rows_per_group <= 65535, "bad split3 arguments");
  hipLaunchKernelGGL(split3_kernel, dim3(grid_for((size_t)cols, 16), groups * rows_per_group), dim3(256), 0, as_stream(stream), in, out,
                     rows_per_group, cols);
  EBEN_CHECK_LAUNCH("split3_kernel");
  return EBEN_OK;
}

extern "C" int eben_stft_frames(const float* sig, float* out, int rows, int t, int win, int hop, int pad, int frames, void* stream) {
  EBEN_REQUIRE(sig && out && rows > 0 && t > 1 && win > 0 && hop > 0 && pad >= 0 && pad < t && frames > 0, "bad stft_frames arguments");
  EBEN_REQUIRE((frames - 1) * hop + win - 1 - pad <= 2 * (t - 1), "stft_frames: frames reach past the reflected signal");
  hipLaunchKernelGGL(stft_frames_kernel, dim3(grid_for((size_t)rows * frames, 64), win), dim3(256), 0, as_stream(stream), sig, out, rows,
                     t, win, hop, pad, frames);
  EBEN_CHECK_LAUNCH("stft_frames_kernel");
  return EBEN_OK;
}
