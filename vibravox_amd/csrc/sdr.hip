// BSS-eval signal-to-distortion ratio (torchmetrics signal_distortion_ratio, direct-solve branch) on the device, rows of different
// lengths, float64 arithmetic on float32 inputs (a product of two floats is exact in a double), no host synchronisation.
//
// For a row of N samples and a distortion filter of L <= 512 taps: t, p = target, preds (minus their means over the row's own N samples
// with zero_mean), each divided by max(its norm, 1e-6); r[k] = sum_n t[n] t[n+k], b[k] = sum_n t[n] p[n+k] for k < L (linear: nothing
// wraps, 0 for k >= N); r[0] += load_diag; Toeplitz(r) h = b; coh = b . h; out = 10 log10(coh / (1 - coh)).  No eps anywhere.
//
//   sdr_moments_kernel   one workgroup per row: the two means (zero_mean) and the two inverse clamped norms, to the workspace
//   sdr_corr_kernel      one workgroup per (segment of kSegment samples, row): the unnormalised partial r[0..L), b[0..L) over the n of
//                        its segment, to the workspace as [row][segment][2][L]; a segment that starts behind the row's end returns
//   sdr_solve_kernel     one workgroup per row: the row's segment partials added in segment order, the two inverse norms, load_diag, the
//                        Levinson recursion for a general right-hand side, coh and the logarithm
//
// Every sum runs in an order that is a function of the row's own length and of L only -- never of rows, t_max or the row's place in the
// batch -- and there is no atomic: a row of a ragged batch has the bits of the call on that row alone.  Nothing behind a row's end is
// read.  A length outside [1, t_max] gives NaN; so does a silent target (0 / 0 in the recursion's first division).
//
// The correlation loop (2 L N fp64 FMAs per row): a lane owns the 8 consecutive lags k0 = 8 lane .. k0 + 8 of both correlations, 16 fp64
// accumulators, and keeps t[n + k0 .. n + k0 + 16) and p[...] of its window in registers; the loop over n is unrolled by 16 in two halves
// that swap the roles of the window's two halves, so the window never moves registers.  Per 8 steps (128 FMAs) a lane reads 8 doubles of
// each signal and the 8 broadcast t[n] from LDS as 12 ds_read_b128: a quarter of what the LDS could deliver while the FMAs issue.  The 64
// lanes of a wave cover 512 lags (lanes without a lag idle); the block's four waves take a quarter of each staged tile and their
// partials are added through LDS in wave order.  LDS holds the signals as doubles (means subtracted), 8 doubles followed by 2 of padding:
// lanes 8 doubles apart then fall on distinct banks for the 16-byte reads.
#include <climits>
#include <cmath>

#include "common.h"

namespace eben {
namespace {

constexpr int kMaxL = 512;        // taps of the distortion filter, at most
constexpr int kSegment = 8192;    // samples of a row per workgroup of sdr_corr_kernel (vibravox_amd/metrics.py SDR_SEGMENT)
constexpr int kTile = 2048;       // samples staged in LDS at a time; a wave takes kTile / 4 of them
constexpr int kQuarter = kTile / 4;
constexpr int kStage = kTile + kMaxL + 8;      // staged samples at L = 512: the tile, its halo and the window's look-ahead
constexpr int kStagePadded = kStage / 8 * 10;  // 8 doubles + 2 of padding
static_assert(kSegment % kTile == 0 && kQuarter % 16 == 0 && kStage % 8 == 0 && kStagePadded % 2 == 0 &&
              2 * kStagePadded >= 4 * 2 * kMaxL /* the waves' partials reuse both images */, "sdr tile geometry");

__host__ __device__ constexpr int pad_idx(int i) { return i + 2 * (i >> 3); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

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

// samples of row r: t_max without a table, else lengths[r], or 0 when that is outside [1, t_max] (uniform over the workgroup)
__device__ __forceinline__ int row_length(const int* __restrict__ lengths, long long r, int t_max) {
  if (!lengths) return t_max;
  const int n = lengths[r];
  return n >= 1 && n <= t_max ? n : 0;
}

// ---- moments: mom[4 r + (0, 1, 2, 3)] = mean(target), mean(preds) (0 without zero_mean), 1 / max(||target||, 1e-6), the same of preds ----
__global__ __launch_bounds__(256) void sdr_moments_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                          const int* __restrict__ lengths, int zero_mean, double* __restrict__ mom) {
  __shared__ double red[4];
  const long long r = blockIdx.x;
  const int n = row_length(lengths, r, t_max);
  if (n == 0) return;   // sdr_corr_kernel reads nothing of such a row, sdr_solve_kernel writes its NaN
  const float* p = preds + r * t_max;
  const float* g = target + r * t_max;
  double mt = 0.0, mp = 0.0;
  if (zero_mean) {
    double st = 0.0, sp = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
      st += (double)g[i];
      sp += (double)p[i];
    }
    mt = block_sum(st, red) / (double)n;
    mp = block_sum(sp, red) / (double)n;
  }
  double tt = 0.0, pp = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double a = (double)g[i] - mt, b = (double)p[i] - mp;
    tt = fma(a, a, tt);
    pp = fma(b, b, pp);
  }
  tt = block_sum(tt, red);
  pp = block_sum(pp, red);
  if (threadIdx.x == 0) {
    mom[4 * r + 0] = mt;
    mom[4 * r + 1] = mp;
    mom[4 * r + 2] = 1.0 / fmax(sqrt(tt), 1e-6);
    mom[4 * r + 3] = 1.0 / fmax(sqrt(pp), 1e-6);
  }
}

// ---- correlation ------------------------------------------------------------------------------------------------------------------
// 8 staged doubles from sample i (a multiple of 8) of the padded image: four 16-byte reads
__device__ __forceinline__ void load8(const double* __restrict__ s, int i, double (&v)[8]) {
  const double2* q = reinterpret_cast<const double2*>(s + pad_idx(i));
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double2 d = q[c];
    v[2 * c] = d.x;
    v[2 * c + 1] = d.y;
  }
}

// the 8 steps n .. n + 8 on the window (lo, hi) = the signals at n + k0 .. n + k0 + 16: acc[j] += t[n + c] * window[c + j]
__device__ __forceinline__ void step8(const double (&tn)[8], const double (&t_lo)[8], const double (&t_hi)[8], const double (&p_lo)[8],
                                      const double (&p_hi)[8], double (&ar)[8], double (&ab)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = c + j;
      ar[j] = fma(tn[c], q < 8 ? t_lo[q] : t_hi[q - 8], ar[j]);
      ab[j] = fma(tn[c], q < 8 ? p_lo[q] : p_hi[q - 8], ab[j]);
    }
  }
}

__global__ __launch_bounds__(256) void sdr_corr_kernel(const float* __restrict__ preds, const float* __restrict__ target, int t_max,
                                                       const int* __restrict__ lengths, int L, int nseg_max, const double* __restrict__ mom,
                                                       double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[2 * kStagePadded];
  const int seg = blockIdx.x;
  const long long r = blockIdx.y;
  const int N = row_length(lengths, r, t_max);
  const int n0 = seg * kSegment;
  if (n0 >= N) return;   // behind the row's end (N == 0: every segment)
  const float* p = preds + r * t_max;
  const float* g = target + r * t_max;
  const double mt = mom[4 * r + 0], mp = mom[4 * r + 1];
  const int staged = kTile + ((L + 7) & ~7) + 8;
  double* ts = lds;
  double* ps = lds + kStagePadded;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k0 = 8 * lane;
  double ar[8], ab[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ar[j] = ab[j] = 0.0;
  for (int tile = 0; tile < kSegment / kTile; ++tile) {
    const int nt = n0 + tile * kTile;
    if (nt >= N) break;
    __syncthreads();
    for (int i = threadIdx.x; i < staged; i += 256) {   // clipped at the row's own end: zeros behind it
      const int n = nt + i;
      double a = 0.0, b = 0.0;
      if (n < N) {
        a = (double)g[n] - mt;
        b = (double)p[n] - mp;
      }
      ts[pad_idx(i)] = a;
      ps[pad_idx(i)] = b;
    }
    __syncthreads();
    if (k0 < L) {
      const int nb = w * kQuarter;
      const int ne = min(nb + kQuarter, (N - nt + 15) & ~15);   // the steps behind the row's end would add zeros
      double tn[8], tw0[8], tw1[8], pw0[8], pw1[8];
      load8(ts, nb + k0, tw0);
      load8(ps, nb + k0, pw0);
      for (int n = nb; n < ne; n += 16) {
        load8(ts, n, tn);
        load8(ts, n + 8 + k0, tw1);
        load8(ps, n + 8 + k0, pw1);
        step8(tn, tw0, tw1, pw0, pw1, ar, ab);
        load8(ts, n + 8, tn);
        load8(ts, n + 16 + k0, tw0);
        load8(ps, n + 16 + k0, pw0);
        step8(tn, tw1, tw0, pw1, pw0, ar, ab);
      }
    }
  }
  __syncthreads();
  double* red = lds;   // [wave][r, b][kMaxL]
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[(w * 2 + 0) * kMaxL + k0 + j] = ar[j];
    red[(w * 2 + 1) * kMaxL + k0 + j] = ab[j];
  }
  __syncthreads();
  double* out = part + ((size_t)r * nseg_max + seg) * 2 * L;
  for (int j = threadIdx.x; j < 2 * L; j += 256) {
    const int which = j >= L, k = j - which * L;
    out[j] = ((red[(0 + which) * kMaxL + k] + red[(2 + which) * kMaxL + k]) + red[(4 + which) * kMaxL + k]) + red[(6 + which) * kMaxL + k];
  }
}

// ---- solve: Levinson's recursion for Toeplitz(r) x = b with the forward vector y (Golub & Van Loan, Algorithm 4.7.2, r[0] kept) -------
__global__ __launch_bounds__(256) void sdr_solve_kernel(int t_max, const int* __restrict__ lengths, int L, int nseg_max,
                                                        const double* __restrict__ mom, const double* __restrict__ part, double load_diag,
                                                        float* __restrict__ out) {
  __shared__ double rs[kMaxL], bs[kMaxL], xs[kMaxL], ys[kMaxL];
  __shared__ double red[8];
  const long long r = blockIdx.x;
  const int tid = threadIdx.x;
  const int N = row_length(lengths, r, t_max);
  if (N == 0) {
    if (tid == 0) out[r] = NAN;
    return;
  }
  const int nseg = (N - 1) / kSegment + 1;
  const double inv_t = mom[4 * r + 2], inv_p = mom[4 * r + 3];
  const double* mine = part + (size_t)r * nseg_max * 2 * L;
  for (int j = tid; j < 2 * L; j += 256) {
    double s = 0.0;
    for (int seg = 0; seg < nseg; ++seg) s += mine[(size_t)seg * 2 * L + j];
    if (j < L) rs[j] = s * inv_t * inv_t + (j == 0 ? load_diag : 0.0);
    else bs[j - L] = s * inv_t * inv_p;
  }
  __syncthreads();
  const double r0 = rs[0];
  double alpha = L > 1 ? -rs[1] / r0 : 0.0, beta = r0;
  if (tid == 0) {
    xs[0] = bs[0] / r0;
    ys[0] = alpha;
  }
  __syncthreads();
  for (int k = 1; k < L; ++k) {
    beta *= 1.0 - alpha * alpha;
    double dx = 0.0, dy = 0.0;
    for (int i = tid; i < k; i += 256) {
      const double rr = rs[i + 1];
      dx = fma(rr, xs[k - 1 - i], dx);
      dy = fma(rr, ys[k - 1 - i], dy);
    }
    dx = wave_sum(dx);
    dy = wave_sum(dy);
    if ((tid & 63) == 0) {
      red[tid >> 6] = dx;
      red[4 + (tid >> 6)] = dy;
    }
    __syncthreads();
    dx = red[0] + red[1] + red[2] + red[3];
    dy = red[4] + red[5] + red[6] + red[7];
    const double mu = (bs[k] - dx) / beta;
    const bool more = k < L - 1;
    alpha = more ? -(rs[k + 1] + dy) / beta : 0.0;
    double ynew[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = tid + 256 * h;
      if (i < k) {
        const double yr = ys[k - 1 - i];
        xs[i] = fma(mu, yr, xs[i]);
        ynew[h] = fma(alpha, yr, ys[i]);
      }
    }
    __syncthreads();   // every read of the old y and of red is done
    if (more) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = tid + 256 * h;
        if (i < k) ys[i] = ynew[h];
      }
    }
    if (tid == 0) {
      xs[k] = mu;
      if (more) ys[k] = alpha;
    }
    __syncthreads();
  }
  double c = 0.0;
  for (int i = tid; i < L; i += 256) c = fma(bs[i], xs[i], c);
  const double coh = block_sum(c, red);
  if (tid == 0) out[r] = (float)(10.0 * log10(coh / (1.0 - coh)));
}

int nseg_of(int t_max) { return (t_max - 1) / kSegment + 1; }

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" size_t eben_sdr_workspace(int rows, int t_max, int filter_length) {
  if (rows <= 0 || t_max <= 0 || filter_length < 1 || filter_length > kMaxL) return 0;
  return align256(sizeof(double) * 4 * (size_t)rows) + align256(sizeof(double) * 2 * (size_t)filter_length * nseg_of(t_max) * (size_t)rows);
}

extern "C" int eben_sdr(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int filter_length,
                        int zero_mean, double load_diag, void* workspace, float* out, void* stream) {
  EBEN_REQUIRE(preds && target && workspace && out, "sdr: null pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535 && t_max > 0 && t_max <= INT_MAX - 2 * kSegment,
               "sdr: rows = %d outside [1, 65535] or t_max = %d outside [1, %d]", rows, t_max, INT_MAX - 2 * kSegment);
  EBEN_REQUIRE(filter_length >= 1 && filter_length <= kMaxL, "sdr: filter_length = %d outside [1, %d]", filter_length, kMaxL);
  EBEN_REQUIRE(zero_mean == 0 || zero_mean == 1, "sdr: zero_mean = %d is neither 0 nor 1", zero_mean);
  EBEN_REQUIRE(load_diag == load_diag, "sdr: load_diag is NaN");
  const int nseg = nseg_of(t_max);
  double* mom = static_cast<double*>(workspace);
  double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + align256(sizeof(double) * 4 * (size_t)rows));
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sdr_moments_kernel, dim3(rows), dim3(256), 0, st, preds, target, t_max, lengths, zero_mean, mom);
  EBEN_CHECK_LAUNCH("sdr_moments_kernel");
  hipLaunchKernelGGL(sdr_corr_kernel, dim3(nseg, rows), dim3(256), 0, st, preds, target, t_max, lengths, filter_length, nseg, mom, part);
  EBEN_CHECK_LAUNCH("sdr_corr_kernel");
  hipLaunchKernelGGL(sdr_solve_kernel, dim3(rows), dim3(256), 0, st, t_max, lengths, filter_length, nseg, mom, part, load_diag, out);
  EBEN_CHECK_LAUNCH("sdr_solve_kernel");
  return EBEN_OK;
}
