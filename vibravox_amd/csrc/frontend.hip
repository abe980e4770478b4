// Data front end on the device: clip powers, the SNR-controlled noisy collate and the time-parallel biquad.
//
//   eben_clip_powers            mean square of ragged clips, float64 products and sums in a fixed order (vibravox/utils.py:163-164)
//   eben_noisy_collate_scaled   the gather of eben_noisy_collate (direct.hip) with the per-item gain of
//                               mix_speech_and_noise_with_rescaling (utils.py:183-188), every step rounded to float32 as torch does
//   eben_biquad                 one second-order IIR section over each reflect-padded row (torchaudio lfilter / lowpass_biquad as
//                               remove_hf, utils.py:84-116, uses it), parallel along time
//
// The biquad.  With s[n] = (y[n], y[n-1]) the recurrence is s[n] = A s[n-1] + (f[n], 0), A = [[-a1, -a2], [1, 0]], f the FIR part.
// A row is cut into chunks of BQ_CHUNK = 256 * BQ_SUB samples, one 256-thread workgroup per (row, chunk), one thread per BQ_SUB
// consecutive samples:
//   1. biquad_kernel<false>  every thread walks its samples from a zero state; a Hillis-Steele scan over the 256 end states with the
//                            host-built powers A^(BQ_SUB 2^k) gives the chunk's zero-state end state E[row][chunk]
//   2. biquad_carry_kernel   one thread per row: S[c+1] = A^BQ_CHUNK S[c] + E[c], the state each chunk starts from
//   3. biquad_kernel<true>   the same walk and scan with thread 0 starting from S[chunk]; every thread then knows the state its
//                            samples start from, walks them again from that state, clamps and stores
// Rows of one chunk skip 1 and 2.  State, powers of A, FIR part and accumulation are float64 (float32 state is off by 3e-4 at
// 48 kHz / 50 Hz, poles at |z| = 0.995); only x and y are float32.  Pass 3 recomputes the recurrence from the true state instead of
// adding h1[k] s0 + h2[k] s1 to a stored zero-state response: nothing but the two states per chunk is kept between the passes, so no
// response is rounded to float32 on the way and no table has to reach the device.
#include <cmath>

#include "common.h"

// No contraction anywhere in this file: the mixing kernel must round its product before its sum as torch does, and every fused
// multiply-add the other kernels want is written as fma().
#pragma clang fp contract(off)

namespace eben {
namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- clip powers ------------------------------------------------------------------------------------------------------------
constexpr int POW_CHUNK = 48;        // clips per by-value table
constexpr int POW_SEG = 256 * 32;    // samples one workgroup sums at a time
constexpr int POW_PARTS = 64;        // partial sums (workgroups) per clip at the most
struct ClipTable { EbenClip t[POW_CHUNK]; };

__device__ __forceinline__ int pow_parts(long long length) {
  const long long segs = (length + POW_SEG - 1) / POW_SEG;
  return segs < POW_PARTS ? (int)segs : POW_PARTS;
}

// partial[clip][part] = sum of x^2 over the segments part, part + parts, ... of the clip: float4 loads on the 16-byte grid of the
// clip's address (a torch slice may start anywhere), the vectors that straddle an end element by element.
__global__ __launch_bounds__(256) void clip_power_partial_kernel(const ClipTable T, double* __restrict__ partial) {
  __shared__ double red[4];
  const EbenClip c = T.t[blockIdx.y];
  const int parts = pow_parts(c.length);
  if ((int)blockIdx.x >= parts) return;
  const long long mis = (long long)((reinterpret_cast<unsigned long long>(c.data) >> 2) & 3ull);
  const float* base = c.data - mis;                      // 16-byte aligned; element e of the clip is base[e + mis]
  const long long nvec = (c.length + mis + 3) / 4;
  const long long nseg = (nvec + POW_SEG / 4 - 1) / (POW_SEG / 4);
  double acc = 0.0;
  for (long long s = blockIdx.x; s < nseg; s += parts) {
    const long long v1 = (s + 1) * (POW_SEG / 4) < nvec ? (s + 1) * (POW_SEG / 4) : nvec;
    for (long long v = s * (POW_SEG / 4) + threadIdx.x; v < v1; v += 256) {
      const long long e0 = 4 * v - mis;
      if (e0 >= 0 && e0 + 4 <= c.length) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(base + 4 * v);
        acc = fma((double)q[0], (double)q[0], acc);
        acc = fma((double)q[1], (double)q[1], acc);
        acc = fma((double)q[2], (double)q[2], acc);
        acc = fma((double)q[3], (double)q[3], acc);
      } else {
        for (int j = 0; j < 4; ++j) {
          const long long e = e0 + j;
          if (e >= 0 && e < c.length) {
            const double a = c.data[e];
            acc = fma(a, a, acc);
          }
        }
      }
    }
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * POW_PARTS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one wave per clip: lane p holds partial p, a fixed butterfly sums them
__global__ __launch_bounds__(64) void clip_power_final_kernel(const ClipTable T, const double* __restrict__ partial, float* __restrict__ powers) {
  const EbenClip c = T.t[blockIdx.x];
  const int parts = pow_parts(c.length);
  double v = (int)threadIdx.x < parts ? partial[(long long)blockIdx.x * POW_PARTS + threadIdx.x] : 0.0;
  v = wave_sum_f64(v);
  if (threadIdx.x == 0) powers[blockIdx.x] = (float)(v / (double)c.length);
}

// ---- SNR-controlled noisy collate ---------------------------------------------------------------------------------------------
constexpr int COLLATE_CHUNK = 48;
struct CollateTable { EbenCollateItem t[COLLATE_CHUNK]; };

// float32 operations rounded to nearest, formed in float64 and rounded once more: for +, *, / and sqrt the second rounding never
// moves the result (53 >= 2*24 + 2 bits), so the compiler may (and does) narrow them to the float32 instruction where that one is
// correctly rounded; the file's contract(off) keeps the product and the sum from becoming one FMA.
// (hipcc's __fsqrt_rn is the 1-ulp native square root, and its __fmul_rn a plain product that the default contraction fuses.)
__device__ __forceinline__ float rn_mul(float a, float b) { return (float)((double)a * (double)b); }
__device__ __forceinline__ float rn_add(float a, float b) { return (float)((double)a + (double)b); }
__device__ __forceinline__ float rn_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float rn_sqrt(float a) { return (float)sqrt((double)a); }

__global__ __launch_bounds__(256) void noisy_collate_scaled_kernel(const CollateTable T, int samples, const float* __restrict__ speech_power,
                                                                   const float* __restrict__ noise_power, const float* __restrict__ snr_linear,
                                                                   float* __restrict__ bc, float* __restrict__ air, float* __restrict__ ns_out) {
  const EbenCollateItem it = T.t[blockIdx.y];
  // utils.py:184: sqrt(speech_power / (noise_power * snr_linear)), each step a float32 tensor op
  const float g = rn_sqrt(rn_div(speech_power[blockIdx.y], rn_mul(noise_power[blockIdx.y], snr_linear[blockIdx.y])));
  float* obc = bc + (long long)blockIdx.y * samples;
  float* oair = air ? air + (long long)blockIdx.y * samples : nullptr;
  float* ons = ns_out ? ns_out + (long long)blockIdx.y * samples : nullptr;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < samples; t += gridDim.x * 256) {
    const long long u = (long long)t + it.shift;
    float v = 0.f, a = 0.f, n = 0.f;
    if (u >= 0 && u < it.length) {
      n = rn_mul(it.noise[it.noise_start + u], g);   // utils.py:185, then :188 -- never one FMA
      v = rn_add(it.speech[u], n);
      if (it.airborne) a = it.airborne[u];
    }
    obc[t] = v;
    if (oair) oair[t] = a;
    if (ons) ons[t] = n;
  }
}

// ---- biquad -------------------------------------------------------------------------------------------------------------------
constexpr int BQ_SUB = 16;                  // samples per thread
constexpr int BQ_CHUNK = 256 * BQ_SUB;      // samples per workgroup (vibravox_amd/filters.py CHUNK)
constexpr int BQ_LEVELS = 8;                // log2(256)

struct BqParams {
  double b0, b1, b2, a1, a2;
  double pw[BQ_LEVELS][4];   // A^(BQ_SUB 2^k), row major
  double pc[4];              // A^BQ_CHUNK
  int t_in, pad, T, nchunk, reversed, clamp;
};

// LDS slot of staged position p (position 0 = two samples before the chunk): one pad word per 16, so that the 64 threads of a wave,
// 16 positions apart, fall on 64 different banks
__device__ __forceinline__ int bq_slot(int p) { return p + (p >> 4); }

template <bool APPLY>
__global__ __launch_bounds__(256) void biquad_kernel(const BqParams P, const float* __restrict__ x, float* __restrict__ y,
                                                     double* __restrict__ ends, const double* __restrict__ starts) {
  __shared__ float stage[BQ_CHUNK + 2 + (BQ_CHUNK + 2) / 16 + 1];
  __shared__ double scan[2][256][2];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x / P.nchunk;
  const int chunk = blockIdx.x % P.nchunk;
  const float* xr = x + row * P.t_in;
  const long long n0 = (long long)chunk * BQ_CHUNK - 2;   // padded-row step of staged position 0
  // step n of the recurrence reads (and pass 3 writes) padded-row sample m = n, or T-1-n when reversed; sample m of the padded row is
  // x[reflect(m - pad)] as ReflectionPad1d maps it
  for (int p = tid; p < BQ_CHUNK + 2; p += 256) {
    const long long n = n0 + p;
    float v = 0.f;
    if (n >= 0 && n < P.T) {
      long long j = (P.reversed ? P.T - 1 - n : n) - P.pad;
      if (j < 0) j = -j;
      if (j >= P.t_in) j = 2ll * (P.t_in - 1) - j;
      v = xr[j];
    }
    stage[bq_slot(p)] = v;
  }
  __syncthreads();
  float xs[BQ_SUB + 2];
#pragma unroll
  for (int k = 0; k < BQ_SUB + 2; ++k) xs[k] = stage[bq_slot(tid * BQ_SUB + k)];
  double f[BQ_SUB];
#pragma unroll
  for (int k = 0; k < BQ_SUB; ++k) f[k] = fma(P.b0, (double)xs[k + 2], fma(P.b1, (double)xs[k + 1], P.b2 * (double)xs[k]));
  const double na1 = -P.a1, na2 = -P.a2;
  // end state of this thread's samples, from zero (thread 0 of pass 3: from the state the chunk starts with)
  double y1 = 0.0, y2 = 0.0;
  if (APPLY && tid == 0 && chunk > 0) {
    y1 = starts[(row * P.nchunk + chunk) * 2];
    y2 = starts[(row * P.nchunk + chunk) * 2 + 1];
  }
  const double in1 = y1, in2 = y2;
#pragma unroll
  for (int k = 0; k < BQ_SUB; ++k) {
    const double v = fma(na1, y1, fma(na2, y2, f[k]));
    y2 = y1;
    y1 = v;
  }
  // inclusive scan: after level k, (y1, y2) of thread t is the end state of threads t - 2^(k+1) + 1 .. t run from zero
  int buf = 0;
#pragma unroll
  for (int k = 0; k < BQ_LEVELS; ++k) {
    scan[buf][tid][0] = y1;
    scan[buf][tid][1] = y2;
    __syncthreads();
    const int d = 1 << k;
    if (tid >= d) {
      const double u1 = scan[buf][tid - d][0], u2 = scan[buf][tid - d][1];
      y1 += fma(P.pw[k][0], u1, P.pw[k][1] * u2);
      y2 += fma(P.pw[k][2], u1, P.pw[k][3] * u2);
    }
    buf ^= 1;
  }
  if (!APPLY) {
    if (tid == 255) {
      ends[(row * P.nchunk + chunk) * 2] = y1;
      ends[(row * P.nchunk + chunk) * 2 + 1] = y2;
    }
    return;
  }
  scan[buf][tid][0] = y1;
  scan[buf][tid][1] = y2;
  __syncthreads();
  y1 = tid ? scan[buf][tid - 1][0] : in1;
  y2 = tid ? scan[buf][tid - 1][1] : in2;
#pragma unroll
  for (int k = 0; k < BQ_SUB; ++k) {
    const double v = fma(na1, y1, fma(na2, y2, f[k]));
    y2 = y1;
    y1 = v;
    const double o = P.clamp ? fmin(fmax(v, -1.0), 1.0) : v;   // on the output only, never fed back (lfilter clamp=True)
    stage[bq_slot(tid * BQ_SUB + k + 2)] = (float)o;
  }
  __syncthreads();
  float* yr = y + row * P.T;
  for (int p = tid; p < BQ_CHUNK; p += 256) {
    const long long n = (long long)chunk * BQ_CHUNK + p;
    if (n < P.T) yr[P.reversed ? P.T - 1 - n : n] = stage[bq_slot(p + 2)];
  }
}

__global__ __launch_bounds__(64) void biquad_carry_kernel(const BqParams P, int rows, const double* __restrict__ ends, double* __restrict__ starts) {
  const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  const double* e = ends + row * P.nchunk * 2;
  double* s = starts + row * P.nchunk * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int c = 0; c < P.nchunk; ++c) {
    s[2 * c] = s1;
    s[2 * c + 1] = s2;
    const double n1 = e[2 * c] + fma(P.pc[0], s1, P.pc[1] * s2);
    const double n2 = e[2 * c + 1] + fma(P.pc[2], s1, P.pc[3] * s2);
    s1 = n1;
    s2 = n2;
  }
}

void mat2_mul(const double* a, const double* b, double* out) {
  const double r[4] = {a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3]};
  for (int i = 0; i < 4; ++i) out[i] = r[i];
}

}  // namespace

}  // namespace eben

using namespace eben;

extern "C" size_t eben_clip_powers_workspace(int nclips) { return nclips > 0 ? (size_t)nclips * POW_PARTS * sizeof(double) : 0; }

extern "C" int eben_clip_powers(const EbenClip* clips, int nclips, float* powers, void* workspace, size_t ws_bytes, void* stream) {
  EBEN_REQUIRE(clips && nclips > 0 && powers && workspace, "bad clip_powers arguments");
  EBEN_REQUIRE(ws_bytes >= eben_clip_powers_workspace(nclips) && (reinterpret_cast<size_t>(workspace) & 7) == 0,
               "clip_powers workspace too small or misaligned (%zu bytes, eben_clip_powers_workspace gives %zu)", ws_bytes,
               eben_clip_powers_workspace(nclips));
  double* partial = static_cast<double*>(workspace);
  for (int p0 = 0; p0 < nclips; p0 += POW_CHUNK) {
    const int cnt = nclips - p0 < POW_CHUNK ? nclips - p0 : POW_CHUNK;
    ClipTable T;
    int gx = 1;
    for (int i = 0; i < cnt; ++i) {
      T.t[i] = clips[p0 + i];
      if (!T.t[i].data || T.t[i].length < 1 || (reinterpret_cast<size_t>(T.t[i].data) & 3)) return fail(EBEN_EINVAL, "clip %d is malformed", p0 + i);
      const long long segs = (T.t[i].length + POW_SEG - 1) / POW_SEG;
      const int parts = segs < POW_PARTS ? (int)segs : POW_PARTS;
      if (parts > gx) gx = parts;
    }
    hipLaunchKernelGGL(clip_power_partial_kernel, dim3(gx, cnt), dim3(256), 0, as_stream(stream), T, partial + (size_t)p0 * POW_PARTS);
    EBEN_CHECK_LAUNCH("clip_power_partial_kernel");
    hipLaunchKernelGGL(clip_power_final_kernel, dim3(cnt), dim3(64), 0, as_stream(stream), T, partial + (size_t)p0 * POW_PARTS, powers + p0);
    EBEN_CHECK_LAUNCH("clip_power_final_kernel");
  }
  return EBEN_OK;
}

extern "C" int eben_noisy_collate_scaled(const EbenCollateItem* items, int nitems, int samples, const float* speech_power, const float* noise_power,
                                         const float* snr_linear, float* body_conducted, float* airborne, float* noise_scaled, void* stream) {
  EBEN_REQUIRE(items && nitems > 0 && samples > 0 && body_conducted && speech_power && noise_power && snr_linear, "bad scaled collate arguments");
  for (int p0 = 0; p0 < nitems; p0 += COLLATE_CHUNK) {
    const int cnt = nitems - p0 < COLLATE_CHUNK ? nitems - p0 : COLLATE_CHUNK;
    CollateTable T;
    for (int i = 0; i < cnt; ++i) {
      T.t[i] = items[p0 + i];
      if (!T.t[i].speech || !T.t[i].noise || T.t[i].length < 0 || T.t[i].noise_start < 0)
        return fail(EBEN_EINVAL, "collate item %d is malformed (the scaled collate needs a noise clip)", p0 + i);
      if (airborne && !T.t[i].airborne) return fail(EBEN_EINVAL, "collate item %d has no airborne clip", p0 + i);
    }
    int gx = (samples + 255) / 256;
    if (gx > 64) gx = 64;
    const long long o = (long long)p0 * samples;
    hipLaunchKernelGGL(noisy_collate_scaled_kernel, dim3(gx, cnt), dim3(256), 0, as_stream(stream), T, samples, speech_power + p0, noise_power + p0,
                       snr_linear + p0, body_conducted + o, airborne ? airborne + o : nullptr, noise_scaled ? noise_scaled + o : nullptr);
    EBEN_CHECK_LAUNCH("noisy_collate_scaled_kernel");
  }
  return EBEN_OK;
}

extern "C" size_t eben_biquad_workspace(int rows, int t_padded) {
  if (rows <= 0 || t_padded <= 0) return 0;
  const size_t nchunk = ((size_t)t_padded + BQ_CHUNK - 1) / BQ_CHUNK;
  return nchunk > 1 ? (size_t)rows * nchunk * 2 * 2 * sizeof(double) : 0;   // end and start state of every chunk
}

extern "C" int eben_biquad(const float* x, float* y, int rows, int t_in, int pad, const double* coef, int reversed, int clamp, void* workspace,
                           size_t ws_bytes, void* stream) {
  EBEN_REQUIRE(x && y && coef && rows > 0 && t_in > 0 && pad >= 0, "bad biquad arguments");
  EBEN_REQUIRE(pad < t_in, "biquad: reflection padding %d needs a row longer than it (got %d samples)", pad, t_in);
  EBEN_REQUIRE((long long)t_in + 2ll * pad <= 0x7fffffffll, "biquad: padded row too long");
  EBEN_REQUIRE(x != y, "biquad does not run in place");
  BqParams P;
  P.b0 = coef[0]; P.b1 = coef[1]; P.b2 = coef[2]; P.a1 = coef[3]; P.a2 = coef[4];
  EBEN_REQUIRE(std::isfinite(P.b0) && std::isfinite(P.b1) && std::isfinite(P.b2) && std::isfinite(P.a1) && std::isfinite(P.a2),
               "biquad coefficients must be finite");
  P.t_in = t_in; P.pad = pad; P.T = t_in + 2 * pad; P.reversed = reversed != 0; P.clamp = clamp != 0;
  P.nchunk = (P.T + BQ_CHUNK - 1) / BQ_CHUNK;
  EBEN_REQUIRE((long long)rows * P.nchunk <= 0x7fffffffll, "biquad: too many (row, chunk) pairs");
  const size_t need = eben_biquad_workspace(rows, P.T);
  EBEN_REQUIRE(need == 0 || (workspace && ws_bytes >= need && (reinterpret_cast<size_t>(workspace) & 7) == 0),
               "biquad workspace too small or misaligned (%zu bytes, eben_biquad_workspace gives %zu)", ws_bytes, need);
  double m[4] = {-P.a1, -P.a2, 1.0, 0.0};                 // A, then A^2, A^4, ... by squaring
  for (int i = 1; i < BQ_SUB; i <<= 1) mat2_mul(m, m, m);
  for (int k = 0; k < BQ_LEVELS; ++k) {
    for (int i = 0; i < 4; ++i) P.pw[k][i] = m[i];
    mat2_mul(m, m, m);
  }
  for (int i = 0; i < 4; ++i) P.pc[i] = m[i];             // A^(BQ_SUB 2^BQ_LEVELS)
  static_assert(BQ_SUB * (1 << BQ_LEVELS) == BQ_CHUNK && (BQ_SUB & (BQ_SUB - 1)) == 0, "powers of A are built by squaring");
  double* ends = static_cast<double*>(workspace);
  double* starts = ends ? ends + (size_t)rows * P.nchunk * 2 : nullptr;
  const unsigned grid = (unsigned)((long long)rows * P.nchunk);
  if (P.nchunk > 1) {
    hipLaunchKernelGGL(biquad_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), P, x, y, ends, (const double*)nullptr);
    EBEN_CHECK_LAUNCH("biquad_kernel<ends>");
    hipLaunchKernelGGL(biquad_carry_kernel, dim3((rows + 63) / 64), dim3(64), 0, as_stream(stream), P, rows, (const double*)ends, starts);
    EBEN_CHECK_LAUNCH("biquad_carry_kernel");
  }
  hipLaunchKernelGGL(biquad_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), P, x, y, (double*)nullptr, (const double*)starts);
  EBEN_CHECK_LAUNCH("biquad_kernel<apply>");
  return EBEN_OK;
}
