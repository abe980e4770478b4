// Frame-based objective speech measures (Hu & Loizou 2008): segmental SNR, frequency-weighted segmental SNR, the LPC log-likelihood
// ratio and the LPC cepstral distance, on the device, rows of different lengths, no host synchronisation.  The definitions are written
// out in include/eben_hip.h (eben_speech_measures); preds = processed, target = clean.
//
//   measures_tables_kernel    one workgroup: the transform's twiddles and the 25 band filters, to the head of the workspace
//   measures_frames_kernel    one workgroup per (tile of kTileFrames frames, row): segmental SNR and, when LLR or CD is asked, both
//                             frames' autocorrelations, Levinson recursions, quadratic forms and cepstra -- all float64
//   measures_spectral_kernel  the same grid: one float32 complex transform of c / |c| + i p / |p| per frame, the two magnitude spectra, band
//                             energies and the weighted band SNR (sums and everything behind them float64)
//   measures_finish_kernel    one workgroup per row: the means, and for LLR / CD the mean of the smallest 95 % of the non-empty frames
//
// Frames overlap by 75 %: a workgroup stages the span of its 16 consecutive frames (15 S + W samples of each signal, 2280 at 16 kHz)
// once in LDS; a wave then takes four of them one after the other.  A frame's work has one shape whatever the row, and the row's
// reductions run in an order that is a function of its own frame count only -- never of rows, t_max or the row's place in the batch --
// without float atomics: a row of a ragged batch has the bits of the call on that row alone.  Nothing at or behind a row's end is read.
//
// The LPC side keeps no per-lane array: lane (s, k) = (lane >> 5, lane & 31) owns lag k, then coefficient k, of signal s (0 clean,
// 1 processed).  An autocorrelation lag is 480 FMAs over the windowed frame in LDS (x[n] broadcast, x[n + k] conflict-free); Levinson's
// step i is one butterfly sum over the half-wave and one shuffle for a[i - k]; the quadratic forms and the cepstral recursion run the
// same way.  The trimmed mean needs no sort: a radix select over order-preserving 64-bit keys (8 passes of a 256-bin integer histogram)
// finds the K-th smallest value, and the sum of everything below it plus the ties is the sum of the K smallest -- one route for any
// frame count.
#include <climits>
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int kTileFrames = 16;   // frames of one row per workgroup (vibravox_amd/metrics.py MEASURES_TILE_FRAMES)
constexpr int kWaves = 4;
constexpr int kFramesPerWave = kTileFrames / kWaves;
constexpr int kBands = 25;
constexpr int kBandHalf = 16;     // a band's filter is kept for the bins centre - 16 ... centre + 16 (at most 29 of them are non-zero)
constexpr int kBandBins = 2 * kBandHalf + 1;
constexpr int kMaxFft = 1024;
constexpr int kAllMeasures = EBEN_MEASURE_SEG_SNR | EBEN_MEASURE_FW_SEG_SNR | EBEN_MEASURE_LLR | EBEN_MEASURE_CD;
constexpr double kEps = 2.220446049250313e-16;   // 2^-52
// head of the workspace: twiddles (float2[kMaxFft / 2]), band filters (float[kBands][kBandBins]), first bins (int[kBands])
constexpr size_t kTwOff = 0, kBandOff = kMaxFft / 2 * 8, kLoOff = kBandOff + 3328, kTableBytes = kLoOff + 256;
static_assert(kBands * kBandBins * 4 <= 3328 && kBands * 4 <= 256 && kTableBytes % 256 == 0, "speech measures table layout");

__device__ const double kCent[kBands] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372,
                                         703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
                                         1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
__device__ const double kBw[kBands] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724, 86.0056,
                                       95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776,
                                       217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

template <int FS> struct Geom;
template <> struct Geom<16000> { static constexpr int W = 480, S = 120, P = 16, NFFT = 1024; };
template <> struct Geom<8000> { static constexpr int W = 240, S = 60, P = 10, NFFT = 512; };

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__host__ __device__ inline int frames_of(int n, int W, int S) { return n < W ? 0 : (n - W) / S; }

// samples of row r: t_max without a table, else lengths[r], or 0 when that is outside [1, t_max] (uniform over the workgroup)
__device__ __forceinline__ int row_length(const int* __restrict__ lengths, long long r, int t_max) {
  if (!lengths) return t_max;
  const int n = lengths[r];
  return n >= 1 && n <= t_max ? n : 0;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the 32 lanes of a half-wave; every lane of the half gets it
__device__ __forceinline__ double half_sum(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Orders a wave's own LDS traffic where its lanes hand data to each other through a region no other wave touches.  The LDS serves one
// wave's instructions in issue order, so only the compiler has to be kept from moving the accesses: no workgroup barrier, the four
// waves of a workgroup do not wait for each other
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over a 256-thread workgroup; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the span of a tile's frames, clipped at the last frame of the row, once into LDS; zeros behind it
template <int SPAN>
__device__ __forceinline__ void stage_span(const float* __restrict__ g, const float* __restrict__ p, int count, float (*st)[SPAN]) {
  for (int i = threadIdx.x; i < SPAN; i += 256) {
    const bool in = i < count;
    st[0][i] = in ? g[i] : 0.f;
    st[1][i] = in ? p[i] : 0.f;
  }
}

// ---- tables ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void measures_tables_kernel(int fs, int n_fft, float2* __restrict__ tw, float* __restrict__ gb,
                                                              int* __restrict__ lo) {
  const int n2 = n_fft / 2;
  const double nyq = 0.5 * (double)fs;
  for (int t = threadIdx.x; t < n2; t += 256) {
    double s, c;
    sincospi(2.0 * (double)t / (double)n_fft, &s, &c);
    tw[t] = make_float2((float)c, (float)-s);
  }
  const double floor_g = exp(-30.0 / (2.0 * 2.303));
  for (int e = threadIdx.x; e < kBands * kBandBins; e += 256) {
    const int i = e / kBandBins, q = e % kBandBins;
    const int f0 = (int)floor(kCent[i] / nyq * (double)n2);
    const double bwn = kBw[i] / nyq * (double)n2;
    const int j = f0 - kBandHalf + q;
    const double d = (double)(j - f0) / bwn;
    double v = exp(-11.0 * d * d + log(70.0) - log(kBw[i]));
    if (v <= floor_g || j < 0 || j >= n2) v = 0.0;
    gb[e] = (float)v;
    if (q == 0) lo[i] = f0 - kBandHalf;
  }
}

// ---- segmental SNR, LLR and cepstral distance per frame -------------------------------------------------------------------------
// vals: [measure 0 seg, 1 fw, 2 llr, 3 cd][row][f_max] doubles; an empty frame's llr and cd are +inf (no value reaches it)
template <int FS>
__global__ __launch_bounds__(256) void measures_frames_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                              const int* __restrict__ lengths, const double* __restrict__ window, int lpc,
                                                              int f_max, int rows, double* __restrict__ vals) {
  using G = Geom<FS>;
  constexpr int W = G::W, S = G::S, P = G::P;
  constexpr int kSpan = (kTileFrames - 1) * S + W;
  constexpr int kPadW = W + 32;   // 32 zeros behind the frame: x[n + k] of the last lags
  __shared__ float st[2][kSpan];
  __shared__ double win[W];
  __shared__ double fr[kWaves][2][kPadW];
  __shared__ double Rl[kWaves][2][32];
  const long long r = blockIdx.y;
  const int F = frames_of(row_length(lengths, r, t_max), W, S);
  const int f0 = blockIdx.x * kTileFrames;
  if (f0 >= F) return;   // behind the row's last frame (F == 0: every tile)
  const int nf = min(kTileFrames, F - f0);
  const long long base = r * (long long)t_max + (long long)f0 * S;
  stage_span<kSpan>(target + base, preds + base, (nf - 1) * S + W, st);
  for (int i = threadIdx.x; i < W; i += 256) win[i] = window[i];
  for (int i = threadIdx.x; i < kWaves * 2 * 32; i += 256) fr[i >> 6][(i >> 5) & 1][W + (i & 31)] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = lane >> 5, k = lane & 31, half = lane & 32;
  for (int q = 0; q < kFramesPerWave; ++q) {   // from here on a wave touches only its own fr[w] and Rl[w]: no workgroup barrier
    const int fl = w * kFramesPerWave + q;
    if (fl >= nf) break;   // behind the row's last frame (uniform over the wave)
    const float* xc = st[0] + fl * S;
    const float* xp = st[1] + fl * S;
    double cc = 0.0, pp = 0.0, dd = 0.0;
    for (int n = lane; n < W; n += 64) {
      const double c = win[n] * (double)xc[n], p = win[n] * (double)xp[n], d = c - p;
      fr[w][0][n] = c;
      fr[w][1][n] = p;
      cc = fma(c, c, cc);
      pp = fma(p, p, pp);
      dd = fma(d, d, dd);
    }
    cc = wave_sum(cc);
    pp = wave_sum(pp);
    dd = wave_sum(dd);
    const double seg = clip(10.0 * log10(cc / (dd + kEps) + kEps), -10.0, 35.0);
    const bool empty = cc == 0.0 || pp == 0.0;
    double llr = 0.0, cd = 0.0;
    if (lpc) {   // uniform over the workgroup
      wave_sync();
      double R = 0.0;
      if (k <= P) {
        const double* x = fr[w][s];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int n = 0; n < W; n += 4) {   // the products behind n = W - 1 - k meet the zeros
          a0 = fma(x[n], x[n + k], a0);
          a1 = fma(x[n + 1], x[n + 1 + k], a1);
          a2 = fma(x[n + 2], x[n + 2 + k], a2);
          a3 = fma(x[n + 3], x[n + 3 + k], a3);
        }
        R = (a0 + a1) + (a2 + a3);
      }
      Rl[w][s][k] = R;
      wave_sync();
      // Levinson-Durbin: lane (s, k) holds a_k of signal s
      const double* Rs = Rl[w][s];
      double a = 0.0, E = Rs[0];
      for (int i = 1; i <= P; ++i) {
        const bool in = k >= 1 && k < i;
        const double acc = half_sum(in ? a * Rs[(i - k) & 31] : 0.0);
        const double kk = (Rs[i] - acc) / E;
        const double other = __shfl(a, half | ((i - k) & 31), 64);
        if (in) a = fma(-kk, other, a);
        if (k == i) a = kk;
        E *= 1.0 - kk * kk;
      }
      // A T A' with T the Toeplitz matrix of the CLEAN frame's R, for A of the clean (half 0) and of the processed frame (half 1)
      const double A = k == 0 ? 1.0 : (k <= P ? -a : 0.0);
      const double* Rc = Rl[w][0];
      double row = 0.0;
      for (int i = 0; i <= P; ++i) {
        const double Ai = __shfl(A, half | i, 64);
        row = fma(Ai, Rc[i > k ? i - k : k - i], row);
      }
      const double quad = half_sum(A * row);
      const double ratio = log(__shfl(quad, 32, 64) / __shfl(quad, 0, 64));
      llr = ratio > 2.0 ? 2.0 : ratio;
      // cepstra: lane (s, k) holds cep_k
      double cep = k == 1 ? a : 0.0;
      for (int m = 2; m <= P; ++m) {
        const bool in = k >= 1 && k < m;
        const double other = __shfl(a, half | ((m - k) & 31), 64);
        const double sum = half_sum(in ? (double)k * cep * other : 0.0);
        if (k == m) cep = a + sum / (double)m;
      }
      const double dc = cep - __shfl_xor(cep, 32, 64);
      const double ss = half_sum(k >= 1 && k <= P ? dc * dc : 0.0);
      const double dist = 10.0 / log(10.0) * sqrt(2.0 * ss);
      cd = dist > 10.0 ? 10.0 : dist;
    }
    if (lane == 0) {
      const size_t at = (size_t)r * f_max + f0 + fl, plane = (size_t)rows * f_max;
      vals[at] = seg;
      if (lpc) {
        vals[2 * plane + at] = empty ? (double)INFINITY : llr;
        vals[3 * plane + at] = empty ? (double)INFINITY : cd;
      }
    }
    wave_sync();   // the next frame overwrites fr
  }
}

// ---- frequency-weighted segmental SNR per frame -----------------------------------------------------------------------------------
__device__ __forceinline__ int bit_reverse(int j, int bits) { return (int)(__brev((unsigned)j) >> (32 - bits)); }

template <int FS>
__global__ __launch_bounds__(256) void measures_spectral_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                                const int* __restrict__ lengths, const double* __restrict__ window,
                                                                const float2* __restrict__ tw_g, const float* __restrict__ gb_g,
                                                                const int* __restrict__ lo_g, int f_max, double* __restrict__ fw) {
  using G = Geom<FS>;
  constexpr int W = G::W, S = G::S, NFFT = G::NFFT, N2 = NFFT / 2;
  constexpr int kBits = NFFT == 1024 ? 10 : 9;
  constexpr int kSpan = (kTileFrames - 1) * S + W;
  constexpr int kPerLane = N2 / 64, kWinPerLane = (W + 63) / 64;
  static_assert(64 * kWinPerLane <= NFFT, "the frame fits the transform");
  __shared__ float st[2][kSpan];
  __shared__ double win[W];
  __shared__ float2 zs[kWaves][NFFT];
  __shared__ float2 tw[N2];
  __shared__ float gb[kBands * kBandBins];
  __shared__ int lo[kBands];
  const long long r = blockIdx.y;
  const int F = frames_of(row_length(lengths, r, t_max), W, S);
  const int f0 = blockIdx.x * kTileFrames;
  if (f0 >= F) return;
  const int nf = min(kTileFrames, F - f0);
  const long long base = r * (long long)t_max + (long long)f0 * S;
  stage_span<kSpan>(target + base, preds + base, (nf - 1) * S + W, st);
  for (int i = threadIdx.x; i < W; i += 256) win[i] = window[i];
  for (int i = threadIdx.x; i < N2; i += 256) tw[i] = tw_g[i];
  for (int i = threadIdx.x; i < kBands * kBandBins; i += 256) gb[i] = gb_g[i];
  if (threadIdx.x < kBands) lo[threadIdx.x] = lo_g[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = lane >> 5, band = lane & 31;
  float2* z = zs[w];
  for (int q = 0; q < kFramesPerWave; ++q) {   // from here on a wave touches only its own zs[w]: no workgroup barrier
    const int fl = w * kFramesPerWave + q;
    if (fl >= nf) break;   // behind the row's last frame (uniform over the wave)
    const float* xc = st[0] + fl * S;
    const float* xp = st[1] + fl * S;
    double cv[kWinPerLane], pv[kWinPerLane];   // the lane's windowed samples n = lane + 64 e, kept for the packing below
    double cc = 0.0, pp = 0.0;
#pragma unroll
    for (int e = 0; e < kWinPerLane; ++e) {
      const int n = lane + 64 * e;
      const bool in = n < W;
      cv[e] = in ? win[n] * (double)xc[n] : 0.0;
      pv[e] = in ? win[n] * (double)xp[n] : 0.0;
      cc = fma(cv[e], cv[e], cc);
      pp = fma(pv[e], pv[e], pp);
    }
    cc = wave_sum(cc);
    pp = wave_sum(pp);
    const bool empty = cc == 0.0 || pp == 0.0;
    // z = c / |c| + i p / |p|, zeros behind the frame.  Both spectra are divided by their own sums below, so the scales change nothing
    // but the rounding: in one float32 transform the weaker signal carries the stronger one's rounding error, and a quiet clean frame
    // under a loud processed one would lose digits to it
    const double sc = 1.0 / sqrt(cc), sp = 1.0 / sqrt(pp);
#pragma unroll
    for (int e = 0; e < kWinPerLane; ++e) z[lane + 64 * e] = make_float2((float)(cv[e] * sc), (float)(pv[e] * sp));
    for (int n = 64 * kWinPerLane + lane; n < NFFT; n += 64) z[n] = make_float2(0.f, 0.f);
    wave_sync();
    // radix-2 decimation in frequency, in place: X[j] ends at index bit_reverse(j)
    for (int hw = N2, sh = 0; hw >= 1; hw >>= 1, ++sh) {
      for (int b = lane; b < N2; b += 64) {
        const int pos = b & (hw - 1), i = ((b - pos) << 1) + pos, j = i + hw;
        const float2 u = z[i], v = z[j], t = tw[pos << sh];
        const float dx = u.x - v.x, dy = u.y - v.y;
        z[i] = make_float2(u.x + v.x, u.y + v.y);
        z[j] = make_float2(dx * t.x - dy * t.y, dx * t.y + dy * t.x);
      }
      wave_sync();
    }
    // |FFT(c)|[j] = |Z[j] + conj(Z[-j])| / 2, |FFT(p)|[j] = |Z[j] - conj(Z[-j])| / 2
    float mc[kPerLane], mp[kPerLane];
    double sum_c = 0.0, sum_p = 0.0;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
      const int j = lane + 64 * e;
      const float2 a = z[bit_reverse(j, kBits)], b = z[bit_reverse((NFFT - j) & (NFFT - 1), kBits)];
      const float cr = a.x + b.x, ci = a.y - b.y, pr = a.x - b.x, pi = a.y + b.y;
      mc[e] = 0.5f * sqrtf(cr * cr + ci * ci);
      mp[e] = 0.5f * sqrtf(pr * pr + pi * pi);
      sum_c += (double)mc[e];
      sum_p += (double)mp[e];
    }
    sum_c = wave_sum(sum_c);
    sum_p = wave_sum(sum_p);
    wave_sync();
    float* mag = reinterpret_cast<float*>(z);   // [clean, processed][N2]
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
      mag[lane + 64 * e] = mc[e];
      mag[N2 + lane + 64 * e] = mp[e];
    }
    wave_sync();
    // lane (s, band): the band's energy of signal s, normalised by the spectrum's sum
    double energy = 0.0;
    if (band < kBands) {
      const float* m = mag + s * N2;
      const float* g = gb + band * kBandBins;
      const int j0 = lo[band];
      double acc = 0.0;
      for (int e = 0; e < kBandBins; ++e) {
        const int j = min(max(j0 + e, 0), N2 - 1);   // the filter is 0 outside [0, N2)
        acc = fma((double)m[j], (double)g[e], acc);
      }
      energy = acc / (s ? sum_p : sum_c);
    }
    const double ec = energy, ep = __shfl_xor(energy, 32, 64);   // in the clean half: the band's clean and processed energies
    double wgt = 0.0, wsnr = 0.0;
    if (s == 0 && band < kBands) {
      const double d = ec - ep;
      const double err = fmax(d * d, kEps);
      wgt = pow(ec, 0.2);
      wsnr = wgt * clip(10.0 * log10(ec * ec / err), -10.0, 35.0);
    }
    const double num = half_sum(wsnr), den = half_sum(wgt);
    if (lane == 0) fw[(size_t)r * f_max + f0 + fl] = empty ? (double)INFINITY : num / den;
    wave_sync();   // the next frame overwrites z
  }
}

// ---- per row ----------------------------------------------------------------------------------------------------------------------
// order-preserving key of a frame value; NaN sorts behind every number (as numpy sorts it), an empty frame's +inf behind that
constexpr unsigned long long kKeyNan = ~0ull - 1, kKeyEmpty = ~0ull, kSign = 1ull << 63;
__device__ __forceinline__ unsigned long long key_of(double v) {
  if (v != v) return kKeyNan;
  if (v == (double)INFINITY) return kKeyEmpty;
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return b & kSign ? ~b : b | kSign;
}
__device__ __forceinline__ double value_of(unsigned long long key) {
  if (key >= kKeyNan) return NAN;
  return __longlong_as_double((long long)(key & kSign ? key & ~kSign : ~key));
}

// mean of the (95 F' + 50) / 100 smallest of the F' non-empty values of v[0 .. F); NaN without one
__device__ double trimmed_mean(const double* __restrict__ v, int F, unsigned* hist, unsigned long long* sel, double* red) {
  const int tid = threadIdx.x;
  double cnt = 0.0;
  for (int f = tid; f < F; f += 256) cnt += key_of(v[f]) != kKeyEmpty ? 1.0 : 0.0;
  const long long live = (long long)block_sum(cnt, red);   // whole numbers below 2^53: exact
  if (live == 0) return NAN;
  const long long K = (95 * live + 50) / 100;
  if (tid == 0) {
    sel[0] = 0ull;                      // the key's bits found so far
    sel[1] = (unsigned long long)K;     // rank (from 1) among the keys that share them
  }
  for (int pass = 7; pass >= 0; --pass) {
    hist[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = sel[0];
    const int shift = 8 * pass;
    for (int f = tid; f < F; f += 256) {
      const unsigned long long key = key_of(v[f]);
      if (pass == 7 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long rank = sel[1], below = 0ull;
      int b = 0;
      for (; b < 255; ++b) {
        if (below + hist[b] >= rank) break;
        below += hist[b];
      }
      sel[0] = (prefix << 8) | (unsigned long long)b;
      sel[1] = rank - below;
    }
    __syncthreads();
  }
  const unsigned long long kth = sel[0];
  double sum = 0.0, less = 0.0;
  for (int f = tid; f < F; f += 256) {
    const double x = v[f];
    if (key_of(x) < kth) {
      sum += x;
      less += 1.0;
    }
  }
  sum = block_sum(sum, red);
  less = block_sum(less, red);
  return (sum + ((double)K - less) * value_of(kth)) / (double)K;   // the ties at the K-th value fill the count
}

__global__ __launch_bounds__(256) void measures_finish_kernel(int t_max, const int* __restrict__ lengths, int W, int S, int measures, int f_max,
                                                              int rows, const double* __restrict__ vals, float* __restrict__ out) {
  __shared__ double red[4];
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sel[2];
  const long long r = blockIdx.x;
  const int tid = threadIdx.x;
  const int F = frames_of(row_length(lengths, r, t_max), W, S);
  const size_t plane = (size_t)rows * f_max;
  int slot = 0;
  for (int m = 0; m < 4; ++m) {
    if (!(measures & (1 << m))) continue;
    float* dst = out + (size_t)(slot++) * rows + r;
    const double* v = vals + m * plane + (size_t)r * f_max;
    double res;
    if (F < 1) {
      res = NAN;
    } else if (m == 0) {   // every frame counts
      double sum = 0.0;
      for (int f = tid; f < F; f += 256) sum += v[f];
      res = block_sum(sum, red) / (double)F;
    } else if (m == 1) {   // the non-empty frames
      double sum = 0.0, cnt = 0.0;
      for (int f = tid; f < F; f += 256) {
        const double x = v[f];
        if (x != (double)INFINITY) {
          sum += x;
          cnt += 1.0;
        }
      }
      sum = block_sum(sum, red);
      cnt = block_sum(cnt, red);
      res = cnt > 0.0 ? sum / cnt : NAN;
    } else {
      res = trimmed_mean(v, F, hist, sel, red);
    }
    if (tid == 0) *dst = (float)res;
  }
}

bool valid(int rows, int t_max, int fs, int measures) {
  return rows >= 1 && rows <= 65535 && t_max >= 1 && t_max <= INT_MAX - 4096 && (fs == 16000 || fs == 8000) && measures != 0 &&
         (measures & ~kAllMeasures) == 0;
}

int f_max_of(int t_max, int fs) {
  const int W = fs == 16000 ? Geom<16000>::W : Geom<8000>::W, S = fs == 16000 ? Geom<16000>::S : Geom<8000>::S;
  return frames_of(t_max, W, S) > 1 ? frames_of(t_max, W, S) : 1;
}

template <int FS>
int launch(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int measures, const double* window,
           char* ws, float* out, hipStream_t st) {
  using G = Geom<FS>;
  const int f_max = f_max_of(t_max, FS);
  float2* tw = reinterpret_cast<float2*>(ws + kTwOff);
  float* gb = reinterpret_cast<float*>(ws + kBandOff);
  int* lo = reinterpret_cast<int*>(ws + kLoOff);
  double* vals = reinterpret_cast<double*>(ws + kTableBytes);
  const dim3 grid(ceil_div(f_max, kTileFrames), rows);
  const int lpc = (measures & (EBEN_MEASURE_LLR | EBEN_MEASURE_CD)) != 0;
  if (lpc || (measures & EBEN_MEASURE_SEG_SNR)) {
    hipLaunchKernelGGL(measures_frames_kernel<FS>, grid, dim3(256), 0, st, preds, target, t_max, lengths, window, lpc, f_max, rows, vals);
    EBEN_CHECK_LAUNCH("measures_frames_kernel");
  }
  if (measures & EBEN_MEASURE_FW_SEG_SNR) {
    hipLaunchKernelGGL(measures_tables_kernel, dim3(1), dim3(256), 0, st, FS, G::NFFT, tw, gb, lo);
    EBEN_CHECK_LAUNCH("measures_tables_kernel");
    hipLaunchKernelGGL(measures_spectral_kernel<FS>, grid, dim3(256), 0, st, preds, target, t_max, lengths, window, tw, gb, lo, f_max,
                       vals + (size_t)rows * f_max);
    EBEN_CHECK_LAUNCH("measures_spectral_kernel");
  }
  hipLaunchKernelGGL(measures_finish_kernel, dim3(rows), dim3(256), 0, st, t_max, lengths, G::W, G::S, measures, f_max, rows, vals, out);
  EBEN_CHECK_LAUNCH("measures_finish_kernel");
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" size_t eben_speech_measures_workspace(int rows, int t_max, int fs, int measures) {
  if (!valid(rows, t_max, fs, measures)) return 0;
  return kTableBytes + align256(sizeof(double) * 4 * (size_t)rows * f_max_of(t_max, fs));
}

extern "C" int eben_speech_measures(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int fs,
                                    int measures, const double* window, void* workspace, float* out, void* stream) {
  EBEN_REQUIRE(preds && target && window && workspace && out, "speech_measures: null pointer");
  EBEN_REQUIRE(rows >= 1 && rows <= 65535 && t_max >= 1 && t_max <= INT_MAX - 4096,
               "speech_measures: rows = %d outside [1, 65535] or t_max = %d outside [1, %d]", rows, t_max, INT_MAX - 4096);
  EBEN_REQUIRE(fs == 16000 || fs == 8000, "speech_measures: fs = %d is neither 16000 nor 8000", fs);
  EBEN_REQUIRE(measures != 0 && (measures & ~kAllMeasures) == 0, "speech_measures: measures = %d is empty or has bits outside EBEN_MEASURE_*",
               measures);
  char* ws = static_cast<char*>(workspace);
  const hipStream_t st = as_stream(stream);
  return fs == 16000 ? launch<16000>(preds, target, rows, t_max, lengths, measures, window, ws, out, st)
                     : launch<8000>(preds, target, rows, t_max, lengths, measures, window, ws, out, st);
}
