// Integrated loudness of ITU-R BS.1770-4 for one channel, per row of a ragged batch, without ever storing the weighted signal.
//
// K-weighting is two second-order sections in cascade (a high shelf, then a high-pass), both from a zero state at the row's first sample.
// With y the shelf's output and w the high-pass's, the state u[n] = (y[n], y[n-1], w[n], w[n-1]) obeys u[n] = M u[n-1] + f[n] (1, 0, c0, 0),
// f the shelf's FIR part, and M is block lower triangular: [[A, 0], [C, D]] with A and D the two sections' companion matrices.  Every
// power of M keeps that shape, so a transition is 12 numbers, not 16.  The recurrence runs parallel along time exactly as frontend.hip's
// biquad does, with ONE scan over the 4-state instead of two 2-state scans back to back: the second section's input is the first one's
// true output, so two scans would need the first section's chunk carries before the second section's end states could even be formed --
// three passes over the input and two carry kernels where the 4-state scan needs two passes and one.
//
//   1. loud_kernel<false>   (row, chunk): every thread walks its LD_SUB samples from a zero state; a Hillis-Steele scan over the 256 end
//                           states with the host-built powers M^(LD_SUB 2^k); thread 255 stores the chunk's end state.  Skipped when
//                           no row has a second chunk; a row's last chunk hands nothing on and returns at once.
//   2. loud_carry_kernel    one thread per row: S[c+1] = M^LD_CHUNK S[c] + E[c], the state each chunk starts from.
//   3. loud_kernel<true>    the same walk and scan with thread 0 starting from S[chunk]; every thread then knows the state its samples
//                           start from, walks them again and leaves w^2 in LDS (float64).  The chunk's samples are then summed per 100 ms
//                           hop: hop j of chunk c is the piece [max(j h, c LD_CHUNK), min((j+1) h, (c+1) LD_CHUNK)), cut at the exact
//                           sample; a wave sums one piece (lane l takes l, l + 64, ... in ascending order, then the xor butterfly) and
//                           stores it at slot c + j of the row -- pieces lie in time order, and a step to the next piece raises c or j.
//                           Only hops that lie wholly inside the row are summed.  The chunk's max |x| goes to a table as well.
//   4. loud_finish_kernel   one workgroup per row: hop energies from their pieces in ascending chunk order, z_j from four consecutive
//                           hops, the absolute gate, the relative gate, then L, the row's peak and the gain.  Thread-strided loops and
//                           a fixed LDS tree: any block count.
//
// All state, squares and sums are float64; the input is read as float32 and nothing behind a row's end is read.  Every sum has one fixed
// order that depends on the sample's place in its own row and on nothing else: no floating-point atomics, and a row's values are the
// bits of the call on that row alone, wherever it lies in whatever batch and however wide the buffer is.
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int LD_SUB = 16;                        // samples per thread
constexpr int LD_THREADS = 256;
constexpr int LD_CHUNK = LD_THREADS * LD_SUB;     // samples per workgroup
constexpr int LD_LEVELS = 8;                      // log2(LD_THREADS)
constexpr int LD_T_MAX = 0x7fffffff - LD_CHUNK;   // every index plus a chunk stays inside int32

// a power of M as (A00 A01 A10 A11 | C00 C01 C10 C11 | D00 D01 D10 D11)
struct LdMat { double v[12]; };

struct LdParams {
  double b0, b1, b2, a1, a2;   // shelf
  double c0, c1, c2, d1, d2;   // high-pass
  LdMat pw[LD_LEVELS];         // M^(LD_SUB 2^k)
  LdMat pc;                    // M^LD_CHUNK
  int t_max, hop, nchunk, nhop;   // of a row of t_max samples: chunks, whole hops
  long long slots;                // piece slots per row
};

// LDS slot of position p: one pad element per 16, so that the threads of a wave, 16 positions apart, spread over the banks (frontend.hip bq_slot)
__device__ __forceinline__ int ld_slot(int p) { return p + (p >> 4); }

// the row's length, -1 for one outside [0, t_max]
__device__ __forceinline__ int ld_len(const int32_t* lengths, int row, int t_max) {
  if (!lengths) return t_max;
  const int n = lengths[row];
  return n < 0 || n > t_max ? -1 : n;
}

// max that keeps a NaN
__device__ __forceinline__ float ld_max(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ void ld_apply(const LdMat& m, double u0, double u1, double u2, double u3, double* r) {
  r[0] = fma(m.v[0], u0, m.v[1] * u1);
  r[1] = fma(m.v[2], u0, m.v[3] * u1);
  r[2] = fma(m.v[4], u0, fma(m.v[5], u1, fma(m.v[8], u2, m.v[9] * u3)));
  r[3] = fma(m.v[6], u0, fma(m.v[7], u1, fma(m.v[10], u2, m.v[11] * u3)));
}

constexpr int LD_STAGE_DOUBLES = 2184;                     // (LD_CHUNK + 2) floats with their padding, rounded up
constexpr int LD_RAW_DOUBLES = LD_CHUNK + LD_CHUNK / 16;   // the squares with their padding: the larger tenant
static_assert((LD_CHUNK + 2 + (LD_CHUNK + 2) / 16 + 1 + 1) / 2 <= LD_STAGE_DOUBLES, "the staged floats fit their part");
static_assert(LD_STAGE_DOUBLES + 2 * 4 * LD_THREADS <= LD_RAW_DOUBLES, "stage and scan fit under the squares");

template <bool APPLY>
__global__ __launch_bounds__(LD_THREADS) void loud_kernel(const LdParams P, const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                          double* __restrict__ ends, const double* __restrict__ starts,
                                                          double* __restrict__ parts, float* __restrict__ peaks) {
  // one buffer, two tenants: the staged input and the scan first, the squares of the second walk after them
  __shared__ __attribute__((aligned(16))) double raw[LD_RAW_DOUBLES];
  __shared__ float wave_peak[LD_THREADS / 64];
  float* stage = reinterpret_cast<float*>(raw);
  double* scan = raw + LD_STAGE_DOUBLES;   // [2][4][LD_THREADS]
  const int tid = threadIdx.x, row = blockIdx.y, chunk = blockIdx.x;
  const int len = ld_len(lengths, row, P.t_max);
  const long long c0 = (long long)chunk * LD_CHUNK;
  if (c0 >= len) return;                            // the whole block: nothing of this row lies here
  if (!APPLY && c0 + LD_CHUNK >= len) return;       // the row's last chunk hands no state on
  const float* xr = x + (long long)row * P.t_max;
  float pk = 0.f;
  for (int p = tid; p < LD_CHUNK + 2; p += LD_THREADS) {
    const long long n = c0 - 2 + p;
    float v = 0.f;
    if (n >= 0 && n < len) v = xr[n];
    stage[ld_slot(p)] = v;
    pk = ld_max(pk, fabsf(v));
  }
  __syncthreads();
  float xs[LD_SUB + 2];
#pragma unroll
  for (int k = 0; k < LD_SUB + 2; ++k) xs[k] = stage[ld_slot(tid * LD_SUB + k)];
  double f[LD_SUB];
#pragma unroll
  for (int k = 0; k < LD_SUB; ++k) f[k] = fma(P.b0, (double)xs[k + 2], fma(P.b1, (double)xs[k + 1], P.b2 * (double)xs[k]));
  const double na1 = -P.a1, na2 = -P.a2, nd1 = -P.d1, nd2 = -P.d2;
  double y1 = 0.0, y2 = 0.0, w1 = 0.0, w2 = 0.0;
  const long long sc = ((long long)row * P.nchunk + chunk) * 4;
  if (APPLY && tid == 0 && chunk > 0) {
    y1 = starts[sc];
    y2 = starts[sc + 1];
    w1 = starts[sc + 2];
    w2 = starts[sc + 3];
  }
  const double i0 = y1, i1 = y2, i2 = w1, i3 = w2;
#pragma unroll
  for (int k = 0; k < LD_SUB; ++k) {
    const double y = fma(na1, y1, fma(na2, y2, f[k]));
    const double w = fma(P.c0, y, fma(P.c1, y1, fma(P.c2, y2, fma(nd1, w1, nd2 * w2))));
    y2 = y1;
    y1 = y;
    w2 = w1;
    w1 = w;
  }
  // inclusive scan: after level k the state of thread t is the end state of threads t - 2^(k+1) + 1 .. t run from zero
  int buf = 0;
#pragma unroll
  for (int k = 0; k < LD_LEVELS; ++k) {
    double* s = scan + buf * 4 * LD_THREADS;
    s[tid] = y1;
    s[LD_THREADS + tid] = y2;
    s[2 * LD_THREADS + tid] = w1;
    s[3 * LD_THREADS + tid] = w2;
    __syncthreads();
    const int d = 1 << k;
    if (tid >= d) {
      double r[4];
      ld_apply(P.pw[k], s[tid - d], s[LD_THREADS + tid - d], s[2 * LD_THREADS + tid - d], s[3 * LD_THREADS + tid - d], r);
      y1 += r[0];
      y2 += r[1];
      w1 += r[2];
      w2 += r[3];
    }
    buf ^= 1;
  }
  if (!APPLY) {
    if (tid == LD_THREADS - 1) {
      ends[sc] = y1;
      ends[sc + 1] = y2;
      ends[sc + 2] = w1;
      ends[sc + 3] = w2;
    }
    return;
  }
  {
    double* s = scan + buf * 4 * LD_THREADS;
    s[tid] = y1;
    s[LD_THREADS + tid] = y2;
    s[2 * LD_THREADS + tid] = w1;
    s[3 * LD_THREADS + tid] = w2;
    __syncthreads();
    y1 = tid ? s[tid - 1] : i0;
    y2 = tid ? s[LD_THREADS + tid - 1] : i1;
    w1 = tid ? s[2 * LD_THREADS + tid - 1] : i2;
    w2 = tid ? s[3 * LD_THREADS + tid - 1] : i3;
  }
  __syncthreads();   // stage and scan have been read: the squares move in
  double* sq = raw;
#pragma unroll
  for (int k = 0; k < LD_SUB; ++k) {
    const double y = fma(na1, y1, fma(na2, y2, f[k]));
    const double w = fma(P.c0, y, fma(P.c1, y1, fma(P.c2, y2, fma(nd1, w1, nd2 * w2))));
    y2 = y1;
    y1 = y;
    w2 = w1;
    w1 = w;
    sq[ld_slot(tid * LD_SUB + k)] = w * w;
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pk = ld_max(pk, __shfl_xor(pk, o, 64));
  if (lane == 0) wave_peak[wave] = pk;
  __syncthreads();
  if (tid == 0) peaks[(long long)row * P.nchunk + chunk] = ld_max(ld_max(wave_peak[0], wave_peak[1]), ld_max(wave_peak[2], wave_peak[3]));
  // the pieces of the hops that lie wholly inside the row
  const long long whole = (long long)(len / P.hop) * P.hop;
  const long long cend = c0 + LD_CHUNK < whole ? c0 + LD_CHUNK : whole;
  if (cend <= c0) return;
  const long long j0 = c0 / P.hop, j1 = (cend - 1) / P.hop;
  double* pr = parts + (long long)row * P.slots + chunk;
  for (long long j = j0 + wave; j <= j1; j += LD_THREADS / 64) {   // wave-uniform bounds
    const long long a = j * P.hop, b = a + P.hop;
    const int lo = (int)((a > c0 ? a : c0) - c0), hi = (int)((b < cend ? b : cend) - c0);
    double s = 0.0;
    for (int i = lo + lane; i < hi; i += 64) s += sq[ld_slot(i)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) pr[j] = s;
  }
}

__global__ __launch_bounds__(64) void loud_carry_kernel(const LdParams P, int rows, const int32_t* __restrict__ lengths, const double* __restrict__ ends,
                                                        double* __restrict__ starts) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  const int len = ld_len(lengths, row, P.t_max);
  if (len <= 0) return;
  const int nc = (int)(((long long)len + LD_CHUNK - 1) / LD_CHUNK);
  const double* e = ends + (long long)row * P.nchunk * 4;
  double* s = starts + (long long)row * P.nchunk * 4;
  double u[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < nc; ++c) {
    for (int i = 0; i < 4; ++i) s[4 * c + i] = u[i];
    if (c + 1 == nc) break;
    double r[4];
    ld_apply(P.pc, u[0], u[1], u[2], u[3], r);
    for (int i = 0; i < 4; ++i) u[i] = e[4 * c + i] + r[i];
  }
}

// sum over the block in one fixed tree; every thread receives it
__device__ __forceinline__ double ld_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int d = LD_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(LD_THREADS) void loud_finish_kernel(const LdParams P, const int32_t* __restrict__ lengths, const double* __restrict__ parts,
                                                                 const float* __restrict__ peaks, double* __restrict__ hops, double target,
                                                                 double ceiling, float* __restrict__ loudness, float* __restrict__ peak,
                                                                 float* __restrict__ gain) {
  __shared__ double red[LD_THREADS];
  __shared__ float fred[LD_THREADS];
  const int tid = threadIdx.x, row = blockIdx.x;
  const int len = ld_len(lengths, row, P.t_max);
  if (len < 0) {
    if (tid == 0) {
      loudness[row] = nanf("");
      peak[row] = nanf("");
      if (gain) gain[row] = 1.f;
    }
    return;
  }
  const int nc = (int)(((long long)len + LD_CHUNK - 1) / LD_CHUNK);
  float pk = 0.f;
  for (int c = tid; c < nc; c += LD_THREADS) pk = ld_max(pk, peaks[(long long)row * P.nchunk + c]);
  fred[tid] = pk;
  __syncthreads();
  for (int d = LD_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) fred[tid] = ld_max(fred[tid], fred[tid + d]);
    __syncthreads();
  }
  pk = fred[0];
  const int nh = len / P.hop;
  const double* pr = parts + (long long)row * P.slots;
  double* hr = hops + (long long)row * P.nhop;
  for (int j = tid; j < nh; j += LD_THREADS) {
    const long long a = (long long)j * P.hop;
    const int ca = (int)(a / LD_CHUNK), cb = (int)((a + P.hop - 1) / LD_CHUNK);
    double e = 0.0;
    for (int c = ca; c <= cb; ++c) e += pr[(long long)c + j];
    hr[j] = e;
  }
  __syncthreads();   // the block's own stores to hops are visible to it
  const int nb = nh >= 4 ? nh - 3 : 0;
  const double inv_n = 1.0 / (4.0 * (double)P.hop);
  double sum = 0.0, cnt = 0.0;
  for (int j = tid; j < nb; j += LD_THREADS) {
    const double z = ((hr[j] + hr[j + 1]) + (hr[j + 2] + hr[j + 3])) * inv_n;
    if (!(-0.691 + 10.0 * log10(z) <= -70.0)) {   // written so that a NaN block passes and makes the row NaN
      sum += z;
      cnt += 1.0;
    }
  }
  sum = ld_block_sum(sum, red);
  cnt = ld_block_sum(cnt, red);
  double L = -INFINITY;
  if (cnt > 0.0) {
    const double rel = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
    sum = 0.0;
    cnt = 0.0;
    for (int j = tid; j < nb; j += LD_THREADS) {
      const double z = ((hr[j] + hr[j + 1]) + (hr[j + 2] + hr[j + 3])) * inv_n;
      const double l = -0.691 + 10.0 * log10(z);
      if (!(l <= -70.0) && !(l <= rel)) {
        sum += z;
        cnt += 1.0;
      }
    }
    sum = ld_block_sum(sum, red);
    cnt = ld_block_sum(cnt, red);
    if (cnt > 0.0) L = -0.691 + 10.0 * log10(sum / cnt);
  }
  if (tid == 0) {
    loudness[row] = (float)L;
    peak[row] = pk;
    if (gain) {
      double g = 1.0;
      if (isfinite(L) && pk > 0.f && isfinite(pk)) {
        g = pow(10.0, (target - L) / 20.0);
        if (g * (double)pk > ceiling) g = ceiling / (double)pk;
      }
      gain[row] = (float)g;
    }
  }
}

// a * b for two transitions of the block-triangular shape
LdMat ld_mul(const LdMat& a, const LdMat& b) {
  const double *A1 = a.v, *C1 = a.v + 4, *D1 = a.v + 8, *A2 = b.v, *C2 = b.v + 4, *D2 = b.v + 8;
  auto mm = [](const double* p, const double* q, double* o) {
    o[0] = p[0] * q[0] + p[1] * q[2];
    o[1] = p[0] * q[1] + p[1] * q[3];
    o[2] = p[2] * q[0] + p[3] * q[2];
    o[3] = p[2] * q[1] + p[3] * q[3];
  };
  LdMat r;
  double t0[4], t1[4];
  mm(A1, A2, r.v);
  mm(C1, A2, t0);
  mm(D1, C2, t1);
  for (int i = 0; i < 4; ++i) r.v[4 + i] = t0[i] + t1[i];
  mm(D1, D2, r.v + 8);
  return r;
}

bool ld_fs_ok(int fs) { return fs > 0 && fs % 10 == 0; }

struct LdLayout {
  size_t nchunk, nhop, slots;
  size_t ends, starts, parts, hops, peaks, bytes;   // byte offsets, the total
};

LdLayout ld_layout(int rows, int t_max, int fs) {
  LdLayout w;
  const size_t hop = (size_t)fs / 10;
  w.nchunk = ((size_t)t_max + LD_CHUNK - 1) / LD_CHUNK;
  w.nhop = (size_t)t_max / hop;
  w.slots = w.nchunk + w.nhop + 1;
  const size_t r = (size_t)rows;
  w.ends = 0;
  w.starts = w.ends + r * w.nchunk * 4 * sizeof(double);
  w.parts = w.starts + r * w.nchunk * 4 * sizeof(double);
  w.hops = w.parts + r * w.slots * sizeof(double);
  w.peaks = w.hops + r * (w.nhop ? w.nhop : 1) * sizeof(double);
  w.bytes = w.peaks + ((r * w.nchunk * sizeof(float) + 7) & ~(size_t)7);
  return w;
}

inline bool ld_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_k_weighting(int fs, double* coef) {
  EBEN_REQUIRE(coef, "k_weighting: null pointer");
  EBEN_REQUIRE(ld_fs_ok(fs), "k_weighting: fs = %d is not a positive multiple of 10", fs);
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
    coef[0] = (Vh + Vb * K / Q + K * K) / a0;
    coef[1] = 2.0 * (K * K - Vh) / a0;
    coef[2] = (Vh - Vb * K / Q + K * K) / a0;
    coef[3] = 2.0 * (K * K - 1.0) / a0;
    coef[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    coef[5] = 1.0;
    coef[6] = -2.0;
    coef[7] = 1.0;
    coef[8] = 2.0 * (K * K - 1.0) / a0;
    coef[9] = (1.0 - K / Q + K * K) / a0;
  }
  return EBEN_OK;
}

extern "C" size_t eben_loudness_workspace(int rows, int t_max, int fs) {
  if (rows < 1 || rows > 65535 || t_max < 1 || t_max > LD_T_MAX || !ld_fs_ok(fs)) return 0;
  return ld_layout(rows, t_max, fs).bytes;
}

extern "C" int eben_loudness(const float* x, int rows, int t_max, const int32_t* lengths, int fs, double target_lufs, double peak_dbfs, float* loudness,
                             float* peak, float* gain, void* workspace, size_t ws_bytes, void* stream) {
  const char* what = "loudness";
  EBEN_REQUIRE(x && loudness && peak && workspace, "%s: null pointer", what);
  EBEN_REQUIRE(ld_aligned(x, 4) && ld_aligned(lengths, 4) && ld_aligned(loudness, 4) && ld_aligned(peak, 4) && ld_aligned(gain, 4) &&
                   ld_aligned(workspace, 8),
               "%s: misaligned pointer (the workspace to 8 bytes, the others to 4)", what);
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "%s: %d rows (1 ... 65535)", what, rows);
  EBEN_REQUIRE(t_max > 0 && t_max <= LD_T_MAX, "%s: t_max = %d (1 ... %d)", what, t_max, LD_T_MAX);
  EBEN_REQUIRE(ld_fs_ok(fs), "%s: fs = %d is not a positive multiple of 10", what, fs);
  EBEN_REQUIRE(std::isfinite(target_lufs) && std::isfinite(peak_dbfs), "%s: the target (%g LUFS) and the peak ceiling (%g dBFS) must be finite", what,
               target_lufs, peak_dbfs);
  const LdLayout w = ld_layout(rows, t_max, fs);
  EBEN_REQUIRE(ws_bytes >= w.bytes, "%s: a workspace of %zu bytes, eben_loudness_workspace gives %zu", what, ws_bytes, w.bytes);
  double coef[10];
  const int rc = eben_k_weighting(fs, coef);
  if (rc != EBEN_OK) return rc;
  LdParams P;
  P.b0 = coef[0]; P.b1 = coef[1]; P.b2 = coef[2]; P.a1 = coef[3]; P.a2 = coef[4];
  P.c0 = coef[5]; P.c1 = coef[6]; P.c2 = coef[7]; P.d1 = coef[8]; P.d2 = coef[9];
  P.t_max = t_max;
  P.hop = fs / 10;
  P.nchunk = (int)w.nchunk;
  P.nhop = (int)(w.nhop ? w.nhop : 1);
  P.slots = (long long)w.slots;
  LdMat m = {{-P.a1, -P.a2, 1.0, 0.0, P.c1 - P.c0 * P.a1, P.c2 - P.c0 * P.a2, 0.0, 0.0, -P.d1, -P.d2, 1.0, 0.0}};   // M, then M^2, M^4, ... by squaring
  for (int i = 1; i < LD_SUB; i <<= 1) m = ld_mul(m, m);
  for (int k = 0; k < LD_LEVELS; ++k) {
    P.pw[k] = m;
    m = ld_mul(m, m);
  }
  P.pc = m;   // M^(LD_SUB 2^LD_LEVELS)
  static_assert(LD_SUB * (1 << LD_LEVELS) == LD_CHUNK && (LD_SUB & (LD_SUB - 1)) == 0, "powers of M are built by squaring");
  char* base = static_cast<char*>(workspace);
  double* ends = reinterpret_cast<double*>(base + w.ends);
  double* starts = reinterpret_cast<double*>(base + w.starts);
  double* parts = reinterpret_cast<double*>(base + w.parts);
  double* hops = reinterpret_cast<double*>(base + w.hops);
  float* peaks = reinterpret_cast<float*>(base + w.peaks);
  const dim3 grid((unsigned)P.nchunk, (unsigned)rows);
  if (P.nchunk > 1) {
    hipLaunchKernelGGL(loud_kernel<false>, grid, dim3(LD_THREADS), 0, as_stream(stream), P, x, lengths, ends, (const double*)nullptr, (double*)nullptr,
                       (float*)nullptr);
    EBEN_CHECK_LAUNCH("loud_kernel<ends>");
    hipLaunchKernelGGL(loud_carry_kernel, dim3((rows + 63) / 64), dim3(64), 0, as_stream(stream), P, rows, lengths, (const double*)ends, starts);
    EBEN_CHECK_LAUNCH("loud_carry_kernel");
  }
  hipLaunchKernelGGL(loud_kernel<true>, grid, dim3(LD_THREADS), 0, as_stream(stream), P, x, lengths, (double*)nullptr, (const double*)starts, parts, peaks);
  EBEN_CHECK_LAUNCH("loud_kernel<measure>");
  hipLaunchKernelGGL(loud_finish_kernel, dim3(rows), dim3(LD_THREADS), 0, as_stream(stream), P, lengths, (const double*)parts, (const float*)peaks, hops,
                     target_lufs, std::pow(10.0, peak_dbfs / 20.0), loudness, peak, gain);
  EBEN_CHECK_LAUNCH("loud_finish_kernel");
  return EBEN_OK;
}
