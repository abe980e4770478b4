// Validation metrics of base_se.py's common_eval_logging (torchmetrics SI-SDR, classic STOI) on the device.
//
// SI-SDR (torchmetrics scale_invariant_signal_distortion_ratio, zero_mean=False): one workgroup per row, two passes over the
// row with fp64 accumulators -- pass 1 gives sum(p*t), sum(t*t), pass 2 sum((alpha*t - p)^2) exactly as written, so there is
// no closed-form cancellation at high SI-SDR.
//
// STOI (pystoi 0.4.x stoi(x=clean, y=processed, fs), extended=False), batched over rows, no host synchronisation:
//   1. stoi_resample_kernel   polyphase resample_poly(x, p, q, window=h) of both signals to 10 kHz (skipped at fs = 10 kHz)
//   2. stoi_frames_kernel     one workgroup per row: frame energies of the clean signal, max, the -40 dB mask and a
//                             ballot/prefix compaction into the kept-frame index table and its count (kept on the device)
//   3. stoi_bands_kernel      one workgroup per (STFT frame, row): the frame of the overlap-added silence-removed signal is
//                             gathered straight from the kept frames (never materialised), then a direct 512-point DFT of the
//                             bins the third-octave bands cover, folded into the 15 band envelopes
//   4. stoi_corr_kernel       one workgroup per row: the 30-frame segment correlations and d
// Buffers are sized for the all-frames-kept case; rows whose kept count is smaller leave the tail workgroups idle.
//
// Ragged batches (eben_si_sdr_ragged / eben_stoi_ragged): the same kernels with a DEVICE table of row lengths.  Rows are t_max apart,
// grids and buffers are sized for a row of t_max samples, and every kernel derives the row's own shape from its length (stoi_shape_of,
// shared with the host), so a row runs the loops of the dense call on that row alone, in the same order.  The dense entries pass
// lengths == nullptr: every row is t_max long.  A length outside [1, t_max] reads nothing and yields NaN.
//
// The evaluation set on top of these (eben_signal_ratio / eben_estoi / eben_lsd), same conventions -- a nullable DEVICE table of row
// lengths, one value per row, fixed-order fp64 reductions, nothing behind a row's end read:
//   signal_ratio_kernel       SI-SDR or torchmetrics' signal_noise_ratio, optionally after a first pass that forms both fp64 means over
//                             the row's own length (zero_mean; SI-SNR is SI-SDR with it)
//   estoi_seg_kernel          pystoi's extended=True tail on the envelopes of stoi_bands_kernel: one wave per 15 x 30 segment, rows
//   estoi_sum_kernel          then columns centred and normalised in registers, the segment's sum to the workspace; one workgroup
//                             per row adds the row's segments in index order
//   lsd_frames_kernel         one workgroup per (STFT frame, row): the frame of both signals, reflected at the ROW's own ends and
//                             Hann-windowed, as z = preds + i target through one complex radix-2 FFT in LDS (fp64), separated into the
//                             two spectra, log10 of the clamped powers, and sqrt(mean over each band's bins of the squared difference)
//   lsd_mean_kernel           one workgroup per (row, band): the mean over the row's own frames in index order
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int kFs = 10000;
constexpr int kFrame = 256;
constexpr int kHop = 128;
constexpr int kNfft = 512;
constexpr int kBands = 15;
constexpr int kSeg = 30;
constexpr double kDynRange = 40.0;
constexpr double kEps64 = 2.220446049250313e-16;    // float64 machine epsilon (pystoi EPS)
constexpr double kSdrEps = 1.1920928955078125e-07;  // float32 machine epsilon (torchmetrics, fp32 inputs)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over a 256-thread workgroup; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// samples of row r: t_max without a table (the dense entries), else lengths[r], or 0 when that is outside [1, t_max] (uniform over
// the workgroup)
__device__ __forceinline__ int row_length(const int* __restrict__ lengths, long long r, int t_max) {
  if (!lengths) return t_max;
  const int n = lengths[r];
  return n >= 1 && n <= t_max ? n : 0;
}

// ---- SI-SDR -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void si_sdr_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                     const int* __restrict__ lengths, float* __restrict__ out) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int t = row_length(lengths, r, t_max);
  if (t == 0) {
    if (threadIdx.x == 0) out[r] = NAN;
    return;
  }
  const float* p = preds + r * t_max;
  const float* g = target + r * t_max;
  double pt = 0.0, tt = 0.0;
  for (int i = threadIdx.x; i < t; i += 256) {
    const double a = p[i], b = g[i];
    pt = fma(a, b, pt);
    tt = fma(b, b, tt);
  }
  pt = block_sum(pt, red);
  tt = block_sum(tt, red);
  const double alpha = (pt + kSdrEps) / (tt + kSdrEps);
  double nn = 0.0;
  for (int i = threadIdx.x; i < t; i += 256) {
    const double e = alpha * (double)g[i] - (double)p[i];
    nn = fma(e, e, nn);
  }
  nn = block_sum(nn, red);
  if (threadIdx.x == 0) out[r] = (float)(10.0 * log10((alpha * alpha * tt + kSdrEps) / (nn + kSdrEps)));
}

// SI-SDR (kind EBEN_RATIO_SI_SDR) or SNR = 10 log10((sum t^2 + eps) / (sum (t - p)^2 + eps)) (EBEN_RATIO_SNR, torchmetrics
// signal_noise_ratio) of one row per workgroup.  zero_mean: a first pass forms both fp64 means over the row's own length and every
// later pass reads p - mean(p), t - mean(t).  (eben_signal_ratio hands plain SI-SDR to si_sdr_kernel itself.)
__global__ __launch_bounds__(256) void signal_ratio_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                           const int* __restrict__ lengths, int kind, int zero_mean,
                                                           float* __restrict__ out) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int t = row_length(lengths, r, t_max);
  if (t == 0) {
    if (threadIdx.x == 0) out[r] = NAN;
    return;
  }
  const float* p = preds + r * t_max;
  const float* g = target + r * t_max;
  double mp = 0.0, mt = 0.0;
  if (zero_mean) {
    double sp = 0.0, st = 0.0;
    for (int i = threadIdx.x; i < t; i += 256) {
      sp += (double)p[i];
      st += (double)g[i];
    }
    mp = block_sum(sp, red) / (double)t;
    mt = block_sum(st, red) / (double)t;
  }
  if (kind == EBEN_RATIO_SNR) {
    double tt = 0.0, nn = 0.0;
    for (int i = threadIdx.x; i < t; i += 256) {
      const double a = (double)p[i] - mp, b = (double)g[i] - mt;
      const double e = b - a;
      tt = fma(b, b, tt);
      nn = fma(e, e, nn);
    }
    tt = block_sum(tt, red);
    nn = block_sum(nn, red);
    if (threadIdx.x == 0) out[r] = (float)(10.0 * log10((tt + kSdrEps) / (nn + kSdrEps)));
    return;
  }
  double pt = 0.0, tt = 0.0;
  for (int i = threadIdx.x; i < t; i += 256) {
    const double a = (double)p[i] - mp, b = (double)g[i] - mt;
    pt = fma(a, b, pt);
    tt = fma(b, b, tt);
  }
  pt = block_sum(pt, red);
  tt = block_sum(tt, red);
  const double alpha = (pt + kSdrEps) / (tt + kSdrEps);
  double nn = 0.0;
  for (int i = threadIdx.x; i < t; i += 256) {
    const double e = alpha * ((double)g[i] - mt) - ((double)p[i] - mp);
    nn = fma(e, e, nn);
  }
  nn = block_sum(nn, red);
  if (threadIdx.x == 0) out[r] = (float)(10.0 * log10((alpha * alpha * tt + kSdrEps) / (nn + kSdrEps)));
}

// ---- STOI ---------------------------------------------------------------------------------------------------------------
struct StoiShape {
  int p, q, t10, nf, fmax;
};

int gcd_int(int a, int b) {
  while (b) {
    const int c = a % b;
    a = b;
    b = c;
  }
  return a;
}

// a signal of t samples at 10000 q / p Hz (p / q reduced; 1 / 1 at 10 kHz): t10 samples at 10 kHz, nf frames at range(0, t10 - 256, 128),
// at most nf - 1 STFT frames of the silence-removed signal (fmax, >= 1 as a buffer pitch).  The one place host and kernels get it from.
__host__ __device__ inline StoiShape stoi_shape_of(int t, int p, int q) {
  StoiShape s{p, q, 0, 0, 1};
  s.t10 = (int)(((long long)t * p + q - 1) / q);
  s.nf = s.t10 > kFrame ? (s.t10 - kFrame + kHop - 1) / kHop : 0;
  s.fmax = s.nf > 1 ? s.nf - 1 : 1;
  return s;
}

struct StoiBands {
  int lo[kBands];  // [lo, hi) FFT bins of each third-octave band (thirdoct(10000, 512, 15, 150))
  int hi[kBands];
  int bin0, nbins;  // the bins any band covers: [bin0, bin0 + nbins)
};

// out[n] = sum_m x[m] * table[half + n*q - m*p], m in [0, t_in): scipy resample_poly's zero-padded, centred polyphase sum
// (table = up * h, 2*half+1 taps).  blockIdx.z selects the signal (0 clean, 1 processed).  Rows are t_max apart on the way in and
// t10_max apart on the way out; a row of t_in samples produces its own ceil(t_in p / q) outputs.
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ processed,
                                                            const float* __restrict__ table, int half, int p, int q, int t_max,
                                                            const int* __restrict__ lengths, int t10_max, int rows,
                                                            float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const long long r = blockIdx.y;
  const int t_in = row_length(lengths, r, t_max);
  if (t_in == 0 || n >= stoi_shape_of(t_in, p, q).t10) return;
  const float* x = (blockIdx.z ? processed : clean) + r * t_max;
  const long long c = (long long)n * q;
  const long long lo_num = c - half;
  int m0 = lo_num <= 0 ? 0 : (int)((lo_num + p - 1) / p);
  int m1 = (int)((c + half) / p);
  if (m1 > t_in - 1) m1 = t_in - 1;
  float acc = 0.f;
  for (int m = m0; m <= m1; ++m) acc = fmaf(x[m], table[c + half - (long long)m * p], acc);
  out[((long long)blockIdx.z * rows + r) * t10_max + n] = acc;
}

__device__ __forceinline__ double hann258(int j) {  // np.hanning(258)[1:-1][j]
  return 0.5 - 0.5 * cos(2.0 * M_PI * (double)(j + 1) / (double)(kFrame + 1));
}

// one workgroup per row: energies 20*log10(||w*frame|| + EPS) of the clean frames at range(0, t - 256, 128), the mask
// max - 40 - e < 0 and the kept-frame table kept[row, 0:count[row]] in frame order.  `clean` is at 10 kHz, rows pitch10 apart; the
// tables are nf_max apart and the row's own frame count comes from its length (t_max, lengths: at the caller's rate).  A row whose
// length is out of range gets count = -1, which stoi_corr_kernel turns into NaN.
__global__ __launch_bounds__(256) void stoi_frames_kernel(const float* __restrict__ clean, int pitch10, int nf_max, int t_max,
                                                          const int* __restrict__ lengths, int p, int q, double* __restrict__ energy,
                                                          int* __restrict__ kept, int* __restrict__ count) {
  __shared__ double win[kFrame];
  __shared__ double red[4];
  __shared__ int wave_cnt[4];
  const long long r = blockIdx.x;
  const int len = row_length(lengths, r, t_max);
  if (len == 0) {
    if (threadIdx.x == 0) count[r] = -1;
    return;
  }
  const int nf = stoi_shape_of(len, p, q).nf;
  const float* x = clean + r * pitch10;
  double* e = energy + r * nf_max;
  int* k = kept + r * nf_max;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  win[threadIdx.x] = hann258(threadIdx.x);
  __syncthreads();
  double emax = -INFINITY;
  for (int f = wave; f < nf; f += 4) {
    const float* fr = x + (long long)f * kHop;
    double s = 0.0;
#pragma unroll
    for (int j = lane; j < kFrame; j += 64) {
      const double v = win[j] * (double)fr[j];
      s = fma(v, v, s);
    }
    s = wave_sum(s);
    const double en = 20.0 * log10(sqrt(s) + kEps64);
    if (lane == 0) e[f] = en;
    emax = fmax(emax, en);
  }
  // block max (every lane of a wave holds the same value)
  if (lane == 0) red[wave] = emax;
  __syncthreads();
  emax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  int base = 0;
  for (int c0 = 0; c0 < nf; c0 += 256) {
    const int f = c0 + threadIdx.x;
    const bool keep = f < nf && (emax - kDynRange - e[f]) < 0.0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) k[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
    base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) count[r] = base;
}

// one workgroup per (STFT frame i, row).  With kept frames k_0..k_{K-1} (k_m[u] = w[u] * sig[128*kept[m] + u]) the
// overlap-added signal has K+1 hops and K-1 STFT frames; frame i is w * [k_i[0:128] + k_{i-1}[128:256], k_i[128:256] + k_{i+1}[0:128]]
// (k_{-1} = 0).  tob[row, s, band, i] = sqrt(sum over the band's bins of |rfft(frame, 512)|^2).  t and nf are the row pitches of the
// 10 kHz signals and of the kept-frame table; the row's own extent is count[row] (-1: nothing to do).
__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ sx, const float* __restrict__ sy, int t, int nf, const int* __restrict__ kept,
                                                         const int* __restrict__ count, StoiBands bands, int fmax, double* __restrict__ tob) {
  __shared__ float win[kFrame];
  __shared__ float cs[kNfft];
  __shared__ float fr[2][kFrame];
  __shared__ float pw[2][kNfft / 2 + 1];
  const int i = blockIdx.x;
  const long long r = blockIdx.y;
  const int nk = count[r];
  if (i >= nk - 1) return;  // uniform over the workgroup
  const int j = threadIdx.x;
  win[j] = (float)hann258(j);
  cs[j] = (float)cos(2.0 * M_PI * (double)j / kNfft);
  cs[j + 256] = -cs[j];
  __syncthreads();
  const int* k = kept + r * nf;
  const long long cur = (long long)k[i] * kHop;
  const long long nb = j < kHop ? (i > 0 ? (long long)k[i - 1] * kHop + kHop + j : -1) : (long long)k[i + 1] * kHop + (j - kHop);
  const int nu = j < kHop ? j + kHop : j - kHop;  // the neighbour frame's own sample index
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* x = (s ? sy : sx) + r * t;
    float v = win[j] * x[cur + j];
    if (nb >= 0) v += win[nu] * x[nb];
    fr[s][j] = win[j] * v;
  }
  __syncthreads();
  for (int pidx = j; pidx < 2 * bands.nbins; pidx += 256) {
    const int s = pidx >= bands.nbins;
    const int bin = bands.bin0 + pidx - s * bands.nbins;
    const float* f = fr[s];
    float re = 0.f, im = 0.f;
    int ph = 0;  // bin * n mod 512
    for (int n = 0; n < kFrame; ++n) {
      re = fmaf(f[n], cs[ph], re);
      im = fmaf(f[n], cs[(ph - 128) & (kNfft - 1)], im);  // sin(2 pi ph / 512)
      ph = (ph + bin) & (kNfft - 1);
    }
    pw[s][bin] = re * re + im * im;
  }
  __syncthreads();
  if (j < 2 * kBands) {
    const int s = j / kBands, b = j - s * kBands;
    double acc = 0.0;
    for (int q = bands.lo[b]; q < bands.hi[b]; ++q) acc += (double)pw[s][q];
    tob[((r * 2 + s) * kBands + b) * (long long)fmax + i] = sqrt(acc);
  }
}

// one workgroup per row: d = sum over segments m and bands of corr(x_seg, y'_seg) / (J * 15), J = frames - 29
__global__ __launch_bounds__(256) void stoi_corr_kernel(const double* __restrict__ tob, const int* __restrict__ count, int fmax,
                                                        float* __restrict__ out) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int frames = count[r] - 1;
  if (frames < kSeg) {  // uniform over the workgroup; count = -1: the row's length was out of range
    if (threadIdx.x == 0) out[r] = count[r] < 0 ? NAN : 1e-5f;
    return;
  }
  const int J = frames - kSeg + 1;
  const double clip = 1.0 + pow(10.0, 15.0 / 20.0);  // 1 + 10^(-BETA/20)
  double acc = 0.0;
  for (int pidx = threadIdx.x; pidx < J * kBands; pidx += 256) {
    const int m = pidx / kBands, b = pidx - m * kBands;
    const double* x = tob + ((r * 2 + 0) * kBands + b) * (long long)fmax + m;
    const double* y = tob + ((r * 2 + 1) * kBands + b) * (long long)fmax + m;
    double xx = 0.0, yy = 0.0;
    for (int n = 0; n < kSeg; ++n) {
      xx = fma(x[n], x[n], xx);
      yy = fma(y[n], y[n], yy);
    }
    const double c = sqrt(xx) / (sqrt(yy) + kEps64);
    double mx = 0.0, my = 0.0;
    for (int n = 0; n < kSeg; ++n) {
      mx += x[n];
      my += fmin(y[n] * c, x[n] * clip);
    }
    mx /= kSeg;
    my /= kSeg;
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (int n = 0; n < kSeg; ++n) {
      const double a = x[n] - mx, bb = fmin(y[n] * c, x[n] * clip) - my;
      sxy = fma(a, bb, sxy);
      sxx = fma(a, a, sxx);
      syy = fma(bb, bb, syy);
    }
    acc += sxy / ((sqrt(sxx) + kEps64) * (sqrt(syy) + kEps64));
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[r] = (float)(acc / ((double)J * kBands));
}

// sum over the 32 lanes of a wave's half (lanes 0-31 / 32-63); every lane of the half gets it
__device__ __forceinline__ double half_wave_sum(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// pystoi's row_col_normalize on one 15 x 30 segment held by a wave: lane l has frame l % 32 (live below 30) of the bands 2 i + l / 32,
// v[i] for i < 8 (band 15 does not exist: that entry and the dead frames stay 0).  Each band's 30 frames are centred and divided by
// their norm, then each frame's 15 bands; a norm of exactly 0 leaves zeros (no EPS * randn dither, tests/eval_metrics_oracle.py).
__device__ __forceinline__ void row_col_normalise(double (&v)[8], bool live, int half) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool ok = live && 2 * i + half < kBands;
    const double mean = half_wave_sum(v[i]) / kSeg;
    const double c = ok ? v[i] - mean : 0.0;
    const double norm = sqrt(half_wave_sum(c * c));
    v[i] = norm > 0.0 ? c / norm : 0.0;
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];
  s += __shfl_xor(s, 32, 64);
  const double mean = s / kBands;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool ok = live && 2 * i + half < kBands;
    v[i] = ok ? v[i] - mean : 0.0;
    q = fma(v[i], v[i], q);
  }
  q += __shfl_xor(q, 32, 64);
  const double norm = sqrt(q);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = norm > 0.0 ? v[i] / norm : 0.0;
}

// ESTOI (pystoi extended=True), one wave per segment m (4 per workgroup): seg[row, m] = sum over the segment of x_n * y_n, both
// matrices row- and column-normalised.  No clipping and no c normalisation.
__global__ __launch_bounds__(256) void estoi_seg_kernel(const double* __restrict__ tob, const int* __restrict__ count, int fmax,
                                                        double* __restrict__ seg) {
  const long long r = blockIdx.y;
  const int frames = count[r] - 1;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (frames < kSeg || m > frames - kSeg) return;  // uniform over the wave; nothing below synchronises the workgroup
  const int lane = threadIdx.x & 63, n = lane & 31, half = lane >> 5;
  const bool live = n < kSeg;
  double x[8], y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = 2 * i + half;
    const bool ok = live && b < kBands;
    x[i] = ok ? tob[((r * 2 + 0) * kBands + b) * (long long)fmax + m + n] : 0.0;
    y[i] = ok ? tob[((r * 2 + 1) * kBands + b) * (long long)fmax + m + n] : 0.0;
  }
  row_col_normalise(x, live, half);
  row_col_normalise(y, live, half);
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc = fma(x[i], y[i], acc);
  acc = wave_sum(acc);
  if (lane == 0) seg[r * fmax + m] = acc;
}

// one workgroup per row: d = sum over the row's J segments / (30 J), in index order per thread and block_sum's order across threads
__global__ __launch_bounds__(256) void estoi_sum_kernel(const double* __restrict__ seg, const int* __restrict__ count, int fmax,
                                                        float* __restrict__ out) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int frames = count[r] - 1;
  if (frames < kSeg) {  // uniform over the workgroup; count = -1: the row's length was out of range
    if (threadIdx.x == 0) out[r] = count[r] < 0 ? NAN : 1e-5f;
    return;
  }
  const int J = frames - kSeg + 1;
  double acc = 0.0;
  for (int m = threadIdx.x; m < J; m += 256) acc += seg[r * fmax + m];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[r] = (float)(acc / ((double)kSeg * J));
}

// ---- log-spectral distance ------------------------------------------------------------------------------------------------
constexpr int kLsdMaxBands = 4;
constexpr double kLsdFloor = 1e-8;  // clamp(|stft|^2, min = 1e-8)

struct LsdBands {
  int lo[kLsdMaxBands];  // [lo, hi) FFT bins of each band
  int hi[kLsdMaxBands];
  int n;
};

// frames of a row of len samples (torch.stft, center = True): 1 + len / hop, or none when the row cannot be reflect-padded
__host__ __device__ inline int lsd_frames_of(int len, int n_fft, int hop) { return len > n_fft / 2 ? 1 + len / hop : 0; }

// one workgroup per (frame f, row).  The frame covers [f hop - N/2, f hop + N/2) of the row reflected at 0 and at len - 1 (one
// reflection each way suffices for len > N/2), under the periodic Hann window.  z = preds + i target goes through one in-place
// decimation-in-frequency radix-2 FFT in LDS -- fp64 data and twiddles: the bar on LSD is a multiple of what float32 torch.stft loses,
// which a float32 FFT of another factorisation can only meet by luck -- leaving Z[k] at the bit-reversed index of k.  With
// X[k] = (Z[k] + conj Z[N-k]) / 2 and Y[k] = (Z[k] - conj Z[N-k]) / 2i: d2[k] = (log10 max(|X|^2, 1e-8) - log10 max(|Y|^2, 1e-8))^2, and
// dist[band, row, f] = sqrt(sum of d2 over the band's bins / bins), the sum in a fixed order that starts at the band's own first bin
// (so a band's value does not depend on which other bands the launch carries).  LDS: N double2 of data, N/2 of twiddles (reused for d2),
// block_sum's four partial sums.
__global__ __launch_bounds__(256) void lsd_frames_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                         const int* __restrict__ lengths, int n_fft, int log2n, int hop, LsdBands bands,
                                                         int rows, int frames_max, double* __restrict__ dist) {
  extern __shared__ __align__(16) unsigned char lsd_lds[];  // all of the kernel's LDS (the attribute raises the dynamic limit to the CU's)
  double2* z = reinterpret_cast<double2*>(lsd_lds);
  double2* tw = z + n_fft;
  double* d2 = reinterpret_cast<double*>(tw);
  double* red = reinterpret_cast<double*>(tw + (n_fft >> 1));
  const int f = blockIdx.x;
  const long long r = blockIdx.y;
  const int len = row_length(lengths, r, t_max);
  if (f >= lsd_frames_of(len, n_fft, hop)) return;  // uniform over the workgroup
  const int tid = threadIdx.x, nh = n_fft >> 1;
  for (int j = tid; j < nh; j += 256) {  // tw[j] = exp(-2 pi i j / N)
    double sn, cs;
    sincospi(2.0 * (double)j / (double)n_fft, &sn, &cs);
    tw[j] = make_double2(cs, -sn);
  }
  __syncthreads();
  const float* p = preds + r * t_max;
  const float* g = target + r * t_max;
  const int start = f * hop - nh;
  for (int n = tid; n < n_fft; n += 256) {
    long long idx = (long long)start + n;
    if (idx < 0) idx = -idx;
    if (idx >= len) idx = 2ll * (len - 1) - idx;
    const double w = 0.5 - 0.5 * (n < nh ? tw[n].x : -tw[n - nh].x);  // hann_window(N)[n] = 0.5 - 0.5 cos(2 pi n / N)
    z[n] = make_double2(w * (double)p[idx], w * (double)g[idx]);
  }
  for (int half = nh, shift = 0; half >= 1; half >>= 1, ++shift) {
    __syncthreads();
    for (int b = tid; b < nh; b += 256) {
      const int j = b & (half - 1);
      const int i0 = ((b - j) << 1) + j, i1 = i0 + half;
      const double2 a = z[i0], c = z[i1], w = tw[j << shift];
      const double dr = a.x - c.x, di = a.y - c.y;
      z[i0] = make_double2(a.x + c.x, a.y + c.y);
      z[i1] = make_double2(dr * w.x - di * w.y, dr * w.y + di * w.x);
    }
  }
  __syncthreads();
  for (int k = tid; k <= nh; k += 256) {
    const double2 a = z[__brev((unsigned)k) >> (32 - log2n)];
    const double2 c = z[__brev((unsigned)((n_fft - k) & (n_fft - 1))) >> (32 - log2n)];
    const double xr = 0.5 * (a.x + c.x), xi = 0.5 * (a.y - c.y);
    const double yr = 0.5 * (a.y + c.y), yi = -0.5 * (a.x - c.x);
    const double d = log10(fmax(xr * xr + xi * xi, kLsdFloor)) - log10(fmax(yr * yr + yi * yi, kLsdFloor));
    d2[k] = d * d;
  }
  __syncthreads();
  for (int b = 0; b < bands.n; ++b) {
    double s = 0.0;
    for (int k = bands.lo[b] + tid; k < bands.hi[b]; k += 256) s += d2[k];
    s = block_sum(s, red);
    if (tid == 0) dist[((long long)b * rows + r) * frames_max + f] = sqrt(s / (double)(bands.hi[b] - bands.lo[b]));
  }
}

// one workgroup per (row, band): out[band, row] = mean of the row's own frames' distances, NaN for a row that cannot be reflect-padded
// (len <= N/2) or whose length is out of range
__global__ __launch_bounds__(256) void lsd_mean_kernel(const double* __restrict__ dist, int t_max, const int* __restrict__ lengths,
                                                       int n_fft, int hop, int rows, int frames_max, float* __restrict__ out) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int b = blockIdx.y;
  const int frames = lsd_frames_of(row_length(lengths, r, t_max), n_fft, hop);
  if (frames == 0) {
    if (threadIdx.x == 0) out[(long long)b * rows + r] = NAN;
    return;
  }
  const double* d = dist + ((long long)b * rows + r) * frames_max;
  double acc = 0.0;
  for (int f = threadIdx.x; f < frames; f += 256) acc += d[f];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[(long long)b * rows + r] = (float)(acc / (double)frames);
}

StoiShape stoi_shape(int t, int fs) {
  int p = 1, q = 1;
  if (fs != kFs) {
    const int g = gcd_int(kFs, fs);
    p = kFs / g;
    q = fs / g;
  }
  return stoi_shape_of(t, p, q);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct StoiWs {
  size_t sig, energy, kept, count, tob, seg, total;
};

// extended: room behind the classic layout for the per-segment sums of the ESTOI tail
StoiWs stoi_ws(int rows, const StoiShape& s, int fs, bool extended = false) {
  StoiWs w{};
  size_t off = 0;
  w.sig = off;
  off += fs != kFs ? align256(sizeof(float) * 2 * (size_t)rows * s.t10) : 0;
  w.energy = off;
  off += align256(sizeof(double) * (size_t)rows * (s.nf > 0 ? s.nf : 1));
  w.kept = off;
  off += align256(sizeof(int) * (size_t)rows * (s.nf > 0 ? s.nf : 1));
  w.count = off;
  off += align256(sizeof(int) * (size_t)rows);
  w.tob = off;
  off += align256(sizeof(double) * (size_t)rows * 2 * kBands * s.fmax);
  w.seg = off;
  off += extended ? align256(sizeof(double) * (size_t)rows * s.fmax) : 0;
  w.total = off;
  return w;
}

// thirdoct(10000, 512, 15, 150): band edges 150 * 2^((2k -+ 1)/6) Hz, each snapped to the nearest bin of linspace(0, fs, 513)[:257]
// (first bin on a tie, as np.argmin)
StoiBands stoi_bands() {
  StoiBands b{};
  auto nearest = [](double hz) {
    int best = 0;
    double bd = INFINITY;
    for (int k = 0; k <= kNfft / 2; ++k) {
      const double d = (k * (double)kFs / kNfft - hz) * (k * (double)kFs / kNfft - hz);
      if (d < bd) {
        bd = d;
        best = k;
      }
    }
    return best;
  };
  for (int k = 0; k < kBands; ++k) {
    b.lo[k] = nearest(150.0 * pow(2.0, (2.0 * k - 1.0) / 6.0));
    b.hi[k] = nearest(150.0 * pow(2.0, (2.0 * k + 1.0) / 6.0));
  }
  b.bin0 = b.lo[0];
  b.nbins = b.hi[kBands - 1] - b.bin0;
  return b;
}

}  // namespace
}  // namespace eben

using namespace eben;

namespace {

int launch_si_sdr(const float* preds, const float* target, int rows, int t_max, const int* lengths, float* out, void* stream) {
  hipLaunchKernelGGL(si_sdr_kernel, dim3(rows), dim3(256), 0, as_stream(stream), preds, target, t_max, lengths, out);
  EBEN_CHECK_LAUNCH("si_sdr_kernel");
  return EBEN_OK;
}

// the STOI stages over rows t_max apart; lengths == nullptr: every row is t_max long (the dense entry).  out: the classic tail,
// out_ext: the extended one (either may be null, not both) -- one run of resample / frames / bands serves both.
int launch_stoi(const float* clean, const float* processed, int rows, int t_max, const int* lengths, int fs, const float* resample_table,
                int taps, void* workspace, size_t ws_bytes, float* out, float* out_ext, void* stream) {
  const StoiShape s = stoi_shape(t_max, fs);
  const StoiWs w = stoi_ws(rows, s, fs, out_ext != nullptr);
  if (ws_bytes < w.total) return fail(EBEN_EWORKSPACE, "stoi needs %zu workspace bytes", w.total);
  char* ws = static_cast<char*>(workspace);
  const hipStream_t st = as_stream(stream);
  const float* sx = clean;  // both signals at 10 kHz, (rows, t10) each
  const float* sy = processed;
  if (fs != kFs) {
    EBEN_REQUIRE(resample_table && taps > 0 && (taps & 1), "stoi at fs != 10000 needs the odd-length resampling table");
    float* rs = reinterpret_cast<float*>(ws + w.sig);
    hipLaunchKernelGGL(stoi_resample_kernel, dim3(ceil_div(s.t10, 256), rows, 2), dim3(256), 0, st, clean, processed, resample_table,
                       (taps - 1) / 2, s.p, s.q, t_max, lengths, s.t10, rows, rs);
    EBEN_CHECK_LAUNCH("stoi_resample_kernel");
    sx = rs;
    sy = rs + (size_t)rows * s.t10;
  }
  double* energy = reinterpret_cast<double*>(ws + w.energy);
  int* kept = reinterpret_cast<int*>(ws + w.kept);
  int* count = reinterpret_cast<int*>(ws + w.count);
  double* tob = reinterpret_cast<double*>(ws + w.tob);
  hipLaunchKernelGGL(stoi_frames_kernel, dim3(rows), dim3(256), 0, st, sx, s.t10, s.nf, t_max, lengths, s.p, s.q, energy, kept, count);
  EBEN_CHECK_LAUNCH("stoi_frames_kernel");
  if (s.nf > 1) {
    hipLaunchKernelGGL(stoi_bands_kernel, dim3(s.fmax, rows), dim3(256), 0, st, sx, sy, s.t10, s.nf, kept, count, stoi_bands(), s.fmax,
                       tob);
    EBEN_CHECK_LAUNCH("stoi_bands_kernel");
  }
  if (out) {
    hipLaunchKernelGGL(stoi_corr_kernel, dim3(rows), dim3(256), 0, st, tob, count, s.fmax, out);
    EBEN_CHECK_LAUNCH("stoi_corr_kernel");
  }
  if (out_ext) {
    double* seg = reinterpret_cast<double*>(ws + w.seg);
    if (s.fmax >= kSeg) {
      hipLaunchKernelGGL(estoi_seg_kernel, dim3(ceil_div(s.fmax - kSeg + 1, 4), rows), dim3(256), 0, st, tob, count, s.fmax, seg);
      EBEN_CHECK_LAUNCH("estoi_seg_kernel");
    }
    hipLaunchKernelGGL(estoi_sum_kernel, dim3(rows), dim3(256), 0, st, seg, count, s.fmax, out_ext);
    EBEN_CHECK_LAUNCH("estoi_sum_kernel");
  }
  return EBEN_OK;
}

LdsAttrOnce lsd_lds_once;

}  // namespace

extern "C" int eben_si_sdr(const float* preds, const float* target, int rows, int t, float* out, void* stream) {
  EBEN_REQUIRE(preds && target && out && rows > 0 && t > 0, "bad si_sdr arguments");
  return launch_si_sdr(preds, target, rows, t, nullptr, out, stream);
}

extern "C" int eben_si_sdr_ragged(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, float* out,
                                  void* stream) {
  EBEN_REQUIRE(preds && target && lengths && out, "si_sdr_ragged: null pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && t_max > 0, "si_sdr_ragged: rows = %d outside [1, 65535] or t_max = %d <= 0", rows, t_max);
  return launch_si_sdr(preds, target, rows, t_max, lengths, out, stream);
}

extern "C" size_t eben_stoi_workspace(int rows, int t, int fs) {
  if (rows <= 0 || t <= 0 || fs <= 0) return 0;
  return stoi_ws(rows, stoi_shape(t, fs), fs).total;
}

// every row at full length with all frames kept: what the dense call on (rows, t_max) takes
extern "C" size_t eben_stoi_ragged_workspace(int rows, int t_max, int fs) { return eben_stoi_workspace(rows, t_max, fs); }

extern "C" int eben_stoi(const float* clean, const float* processed, int rows, int t, int fs, const float* resample_table, int taps,
                         void* workspace, size_t ws_bytes, float* out, void* stream) {
  EBEN_REQUIRE(clean && processed && out && workspace && rows > 0 && rows <= 65535 && t > 0 && fs > 0, "bad stoi arguments");
  return launch_stoi(clean, processed, rows, t, nullptr, fs, resample_table, taps, workspace, ws_bytes, out, nullptr, stream);
}

extern "C" int eben_stoi_ragged(const float* clean, const float* processed, int rows, int t_max, const int32_t* lengths, int fs,
                                const float* resample_table, int taps, void* workspace, size_t ws_bytes, float* out, void* stream) {
  EBEN_REQUIRE(clean && processed && lengths && out && workspace, "stoi_ragged: null pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && t_max > 0 && fs > 0, "stoi_ragged: rows = %d outside [1, 65535], t_max = %d or fs = %d <= 0", rows,
               t_max, fs);
  return launch_stoi(clean, processed, rows, t_max, lengths, fs, resample_table, taps, workspace, ws_bytes, out, nullptr, stream);
}

extern "C" int eben_signal_ratio(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int kind,
                                 int zero_mean, float* out, void* stream) {
  EBEN_REQUIRE(preds && target && out, "signal_ratio: null pointer");
  EBEN_REQUIRE(rows > 0 && t_max > 0, "signal_ratio: rows = %d or t_max = %d <= 0", rows, t_max);
  EBEN_REQUIRE(kind == EBEN_RATIO_SI_SDR || kind == EBEN_RATIO_SNR, "signal_ratio: kind = %d is neither EBEN_RATIO_SI_SDR nor EBEN_RATIO_SNR", kind);
  EBEN_REQUIRE(zero_mean == 0 || zero_mean == 1, "signal_ratio: zero_mean = %d is neither 0 nor 1", zero_mean);
  if (kind == EBEN_RATIO_SI_SDR && !zero_mean) return launch_si_sdr(preds, target, rows, t_max, lengths, out, stream);
  hipLaunchKernelGGL(signal_ratio_kernel, dim3(rows), dim3(256), 0, as_stream(stream), preds, target, t_max, lengths, kind, zero_mean, out);
  EBEN_CHECK_LAUNCH("signal_ratio_kernel");
  return EBEN_OK;
}

extern "C" size_t eben_estoi_workspace(int rows, int t_max, int fs) {
  if (rows <= 0 || t_max <= 0 || fs <= 0) return 0;
  return stoi_ws(rows, stoi_shape(t_max, fs), fs, true).total;
}

extern "C" int eben_estoi(const float* clean, const float* processed, int rows, int t_max, const int32_t* lengths, int fs,
                          const float* resample_table, int taps, void* workspace, size_t ws_bytes, float* out, float* out_classic,
                          void* stream) {
  EBEN_REQUIRE(clean && processed && out && workspace, "estoi: null pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && t_max > 0 && fs > 0, "estoi: rows = %d outside [1, 65535], t_max = %d or fs = %d <= 0", rows, t_max, fs);
  return launch_stoi(clean, processed, rows, t_max, lengths, fs, resample_table, taps, workspace, ws_bytes, out_classic, out, stream);
}

extern "C" size_t eben_lsd_workspace(int rows, int t_max, int n_fft, int hop, int nbands) {
  if (rows <= 0 || t_max <= 0 || n_fft <= 0 || hop <= 0 || nbands <= 0) return 0;
  return align256(sizeof(double) * (size_t)nbands * rows * (1 + t_max / hop));
}

extern "C" int eben_lsd(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int n_fft, int hop,
                        const int* band_lo, const int* band_hi, int nbands, void* workspace, size_t ws_bytes, float* out, void* stream) {
  EBEN_REQUIRE(preds && target && band_lo && band_hi && workspace && out, "lsd: null pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && t_max > 0, "lsd: rows = %d outside [1, 65535] or t_max = %d <= 0", rows, t_max);
  EBEN_REQUIRE(n_fft >= 256 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0, "lsd: n_fft = %d is not a power of two in [256, 4096]", n_fft);
  EBEN_REQUIRE(hop >= 1 && hop <= n_fft, "lsd: hop = %d outside [1, n_fft = %d]", hop, n_fft);
  EBEN_REQUIRE(nbands >= 1 && nbands <= kLsdMaxBands, "lsd: %d bands outside [1, %d]", nbands, kLsdMaxBands);
  LsdBands bands{};
  bands.n = nbands;
  for (int b = 0; b < nbands; ++b) {
    EBEN_REQUIRE(band_lo[b] >= 0 && band_lo[b] < band_hi[b] && band_hi[b] <= n_fft / 2 + 1, "lsd: band %d = [%d, %d) is empty or outside [0, %d)", b,
                 band_lo[b], band_hi[b], n_fft / 2 + 1);
    bands.lo[b] = band_lo[b];
    bands.hi[b] = band_hi[b];
  }
  const size_t need = eben_lsd_workspace(rows, t_max, n_fft, hop, nbands);
  if (ws_bytes < need) return fail(EBEN_EWORKSPACE, "lsd needs %zu workspace bytes", need);
  int log2n = 0;
  while ((1 << log2n) < n_fft) ++log2n;
  const int frames_max = 1 + t_max / hop;
  const size_t lds = sizeof(double2) * ((size_t)n_fft + n_fft / 2) + 4 * sizeof(double);
  const hipError_t e = lds_attr_once(lsd_lds_once, reinterpret_cast<const void*>(lsd_frames_kernel));
  if (e != hipSuccess) return hip_fail(e, "lsd_frames_kernel: dynamic LDS attribute");
  double* dist = static_cast<double*>(workspace);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(lsd_frames_kernel, dim3(frames_max, rows), dim3(256), lds, st, preds, target, t_max, lengths, n_fft, log2n, hop, bands, rows,
                     frames_max, dist);
  EBEN_CHECK_LAUNCH("lsd_frames_kernel");
  hipLaunchKernelGGL(lsd_mean_kernel, dim3(rows, nbands), dim3(256), 0, st, dist, t_max, lengths, n_fft, hop, rows, frames_max, out);
  EBEN_CHECK_LAUNCH("lsd_mean_kernel");
  return EBEN_OK;
}
