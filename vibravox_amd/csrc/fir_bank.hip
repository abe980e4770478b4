// fir_bank.hip -- tap-tiled FIR banks (gfx950): eben_fir_decimate / eben_fir_interp_sum for the banks the whole-bank-in-LDS kernels of
// direct.hip refuse -- PseudoQMFBanks at its class defaults (32 bands x 1024 taps, pqmf.py:17-232), EBENGenerator(n = 512), anything in
// 1 <= bands <= 64, 1 <= ntaps <= 4096, 1 <= stride <= 64.
//
// Both directions are one contraction D[i][n] = sum_kk A[i][kk] B[kk][n] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation, 64 FLOP / clk / SIMD = the fp32 vector rate, and one LDS dword per operand and lane per 2048 multiply-adds):
//   decimating bank       i = band,                    kk = tap j,                  B = x[(t0 + n) stride + off0 + j]
//   interpolating, summed i = phase r of u - off0      kk = (band k, m), j = r + m stride,   B = y[k][q0 + n - m]     (u = q stride + r + off0)
// A block = 4 waves = 128 columns n (output frames t / input frames q) x one 32-row tile; wave w owns columns 32 w .. 32 w + 31 and ONE
// 32 x 32 accumulator.  The input span of the 128 columns is staged in LDS ONCE and serves every band; the bank is never resident:
// it streams through two LDS buffers in chunks of 64 reduction steps, the next chunk's global loads in flight (8 registers per thread)
// while the current one is contracted, one barrier per chunk.  The reduction runs in ascending kk in every lane whatever the grid:
// no atomics, bitwise reproducible.  Rows past the bank / the stride and reduction steps past its end carry ZERO weights.
//   * decimating: the staged span is skewed by one dword per 32 (index r + r / 32), so that the 32 columns of a half-wave, `stride`
//     dwords apart, fall into distinct banks at stride 32 (and 4, 8, 16; two-way at 64);
//   * interpolating: the input tiles of G bands at a time (all 32 of the default bank: 20 KB), the bands in ascending order over the
//     groups; the 32 x 128 result goes through LDS once so that the stores run along u.
#include "common.h"

namespace eben {

constexpr int FB_P = 128;            // columns per block (4 waves x 32)
constexpr int FB_CHUNK = 64;         // reduction steps per weight chunk = 32 MFMAs per wave
constexpr int FB_ASTR = 33;          // row stride of a staged weight chunk [kk][32 rows] (+1: the transposing writes of the decimating form)
constexpr int FB_A_FLOATS = FB_CHUNK * FB_ASTR;
constexpr int FB_IN_BUDGET = 12288;  // interpolating form: floats of staged input tiles (G bands x TT frames)
static_assert(2 * FB_A_FLOATS >= FB_P * FB_ASTR, "the interpolating epilogue transposes through the two weight buffers");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct FirBankArgs {
  const float* in; const float* w; float* out;
  int lx, ly, bands, ntaps, stride, off0;
  int M, Mp, TT, G;     // interpolating form (FirBankGeom)
  long long qmin;       // interpolating form: first input frame q = floor(-off0 / stride)
};

template <int DIR>
__global__ __launch_bounds__(256) void fir_bank_kernel(const FirBankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // 2 x [64][33]
  float* In = smem + 2 * FB_A_FLOATS;  // staged input
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, h = lane >> 5, n = wv * 32 + col;
  const int b = blockIdx.y, r0 = blockIdx.z * 32;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  float wreg[8];

  if (DIR == 0) {
    const int t0 = blockIdx.x * FB_P;
    const long long q0 = (long long)t0 * a.stride + a.off0;
    const int nch = (a.ntaps + FB_CHUNK - 1) / FB_CHUNK;
    const int span = (FB_P - 1) * a.stride + a.ntaps, span_pad = (FB_P - 1) * a.stride + nch * FB_CHUNK;
    const float* xr = a.in + (long long)b * a.lx;
    for (int r = tid; r < span_pad; r += 256) {
      const long long q = q0 + r;
      In[r + (r >> 5)] = (r < span && q >= 0 && q < a.lx) ? xr[q] : 0.f;
    }
    // chunk c of the bank: thread -> (row e / 64, step e % 64): global reads along the taps, LDS writes [step][row] (banks step + row)
    auto load_w = [&](int c) {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int e = tid + 256 * v, kk = c * FB_CHUNK + (e & 63), band = r0 + (e >> 6);
        wreg[v] = (band < a.bands && kk < a.ntaps) ? a.w[(long long)band * a.ntaps + kk] : 0.f;
      }
    };
    auto store_w = [&](int buf) {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int e = tid + 256 * v;
        As[buf * FB_A_FLOATS + (e & 63) * FB_ASTR + (e >> 6)] = wreg[v];
      }
    };
    load_w(0);
    store_w(0);
    __syncthreads();
    const int bbase = n * a.stride + h;
    for (int c = 0; c < nch; ++c) {
      if (c + 1 < nch) load_w(c + 1);
      const float* Ab = As + (c & 1) * FB_A_FLOATS + h * FB_ASTR + col;
      const int bidx = bbase + c * FB_CHUNK;
      // operands of 8 MFMAs at a time, the next 8 read from LDS while these run
      float av[2][8], bv[2][8];
      auto load_ops = [&](int set, int g) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int st = g * 8 + i, idx = bidx + 2 * st;
          av[set][i] = Ab[st * 2 * FB_ASTR];
          bv[set][i] = In[idx + (idx >> 5)];
        }
      };
      load_ops(0, 0);
#pragma unroll
      for (int g = 0; g < FB_CHUNK / 16; ++g) {
        if (g + 1 < FB_CHUNK / 16) load_ops((g + 1) & 1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][i], bv[g & 1][i], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (c + 1 < nch) store_w((c + 1) & 1);   // the other buffer was last read one chunk (a barrier) back
      __syncthreads();
    }
    // 32x32 D tile: column = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
    const int t = t0 + n;
    if (t < a.ly) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int band = r0 + (v & 3) + 8 * (v >> 2) + 4 * h;
        if (band < a.bands) a.out[((long long)b * a.bands + band) * a.ly + t] = acc[v];
      }
    }
  } else {
    const long long q0 = a.qmin + (long long)blockIdx.x * FB_P;
    const long long tmin = q0 - (a.Mp - 1);
    const int zero_idx = a.G * a.TT;   // one zero word behind the staged tiles
    if (tid == 0) In[zero_idx] = 0.f;
    for (int g0 = 0; g0 < a.bands; g0 += a.G) {
      const int Gc = min(a.G, a.bands - g0);
      for (int kg = 0; kg < Gc; ++kg) {   // (every wave is past the last chunk's barrier: In and both weight buffers are free)
        const float* yr = a.in + ((long long)b * a.bands + g0 + kg) * a.ly;
        for (int tl = tid; tl < a.TT; tl += 256) {
          const long long t = tmin + tl;
          In[kg * a.TT + tl] = (t >= 0 && t < a.ly) ? yr[t] : 0.f;
        }
      }
      const int KT = Gc * a.Mp, nch = (KT + FB_CHUNK - 1) / FB_CHUNK;
      // chunk c: thread -> (step e / 32, phase e % 32): reduction step kk = (band kg, m), tap j = r + m stride: global reads along r
      auto load_w = [&](int c) {
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int e = tid + 256 * v, kk = c * FB_CHUNK + (e >> 5), r = r0 + (e & 31);
          const int kg = kk / a.Mp, m = kk - kg * a.Mp, j = r + m * a.stride;
          wreg[v] = (kg < Gc && r < a.stride && j < a.ntaps) ? a.w[(long long)(g0 + kg) * a.ntaps + j] : 0.f;
        }
      };
      auto store_w = [&](int buf) {
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int e = tid + 256 * v;
          As[buf * FB_A_FLOATS + (e >> 5) * FB_ASTR + (e & 31)] = wreg[v];
        }
      };
      load_w(0);
      store_w(0);
      __syncthreads();
      for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load_w(c + 1);
        const float* Ab = As + (c & 1) * FB_A_FLOATS + h * FB_ASTR + col;
        int kg = (c * FB_CHUNK) / a.Mp, me = c * FB_CHUNK - kg * a.Mp;   // block-uniform (band, even m) of the step: Mp is even
        float av[2][8], bv[2][8];
        auto load_ops = [&](int set, int g) {   // (called in ascending g: kg / me walk the steps)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int m = me + h;
            // frame q0 + n - m; steps past the group's last band (uniform) or the last tap of a phase carry zero weights AND read the zero word
            // (an address select: a value select would wait for every read in turn)
            av[set][i] = Ab[(g * 8 + i) * 2 * FB_ASTR];
            bv[set][i] = In[(kg < Gc && m < a.M) ? kg * a.TT + n + (a.Mp - 1) - m : zero_idx];
            me += 2;
            if (me >= a.Mp) { me = 0; ++kg; }
          }
        };
        load_ops(0, 0);
#pragma unroll
        for (int g = 0; g < FB_CHUNK / 16; ++g) {
          if (g + 1 < FB_CHUNK / 16) load_ops((g + 1) & 1, g + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][i], bv[g & 1][i], acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (c + 1 < nch) store_w((c + 1) & 1);
        __syncthreads();
      }
    }
    // D[r][n] -> LDS [n][r] (both weight buffers are free behind the last barrier) -> stores along u = (q0 + n) stride + r + off0
    float* T = smem;
#pragma unroll
    for (int v = 0; v < 16; ++v) T[n * FB_ASTR + (v & 3) + 8 * (v >> 2) + 4 * h] = acc[v];
    __syncthreads();
    const int rows = min(a.stride - r0, 32);
    float* xo = a.out + (long long)b * a.lx;
    for (int e = tid; e < FB_P * rows; e += 256) {
      const int nn = e / rows, rr = e - nn * rows;
      const long long u = (q0 + nn) * a.stride + r0 + rr + a.off0;
      if (u >= 0 && u < a.lx) xo[u] = T[nn * FB_ASTR + rr];
    }
  }
}

int fir_bank_geom(int bands, int ntaps, int stride, int which, FirBankGeom* g) {
  if (bands < 1 || bands > 64 || ntaps < 1 || ntaps > 4096 || stride < 1 || stride > 64)
    return fail(EBEN_EUNSUPPORTED, "fir bank of %d bands x %d taps at stride %d is outside 1..64 bands, 1..4096 taps, stride 1..64", bands, ntaps, stride);
  *g = FirBankGeom{};
  g->P = FB_P;
  g->chunk = FB_CHUNK;
  if (which == 0) {
    g->rows = bands < 32 ? bands : 32;
    g->row_tiles = ceil_div(bands, 32);
    const int span_pad = (FB_P - 1) * stride + round_up(ntaps, FB_CHUNK);
    g->in_floats = span_pad + (span_pad >> 5) + 1;
  } else {
    g->rows = stride < 32 ? stride : 32;
    g->row_tiles = ceil_div(stride, 32);
    g->Mp = round_up(ceil_div(ntaps, stride), 2);
    g->TT = FB_P + g->Mp - 1;
    g->G = FB_IN_BUDGET / g->TT;   // >= 2: TT <= 128 + 4096 - 1
    if (g->G > bands) g->G = bands;
    g->in_floats = g->G * g->TT + 1;   // + the zero word
  }
  g->lds = sizeof(float) * (size_t)(2 * FB_A_FLOATS + g->in_floats);
  if (g->lds > 160 * 1024) return fail(EBEN_EUNSUPPORTED, "fir bank tile of %zu bytes exceeds the LDS", g->lds);   // (not reachable inside the domain)
  return EBEN_OK;
}

int fir_bank_launch(int which, const float* in, const float* w, float* out, int batch, int lx, int ly, int bands, int ntaps, int stride,
                    int off0, hipStream_t st) {
  FirBankGeom g;
  const int rc = fir_bank_geom(bands, ntaps, stride, which, &g);
  if (rc != EBEN_OK) return rc;
  FirBankArgs a{};
  a.in = in; a.w = w; a.out = out;
  a.lx = lx; a.ly = ly; a.bands = bands; a.ntaps = ntaps; a.stride = stride; a.off0 = off0;
  static LdsAttrOnce once[2];
  const void* kern = which ? (const void*)fir_bank_kernel<1> : (const void*)fir_bank_kernel<0>;
  if (g.lds > 64 * 1024) {
    const hipError_t e = lds_attr_once(once[which], kern);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(fir_bank)");
  }
  if (which == 0) {
    const long long nx = ((long long)ly + FB_P - 1) / FB_P;
    hipLaunchKernelGGL(fir_bank_kernel<0>, dim3((unsigned)nx, batch, g.row_tiles), dim3(256), g.lds, st, a);
  } else {
    // u - off0 = q stride + r covers u = 0 .. lx - 1 for q = floor(-off0 / stride) .. floor((lx - 1 - off0) / stride)
    auto fdiv = [](long long n, long long d) { long long q = n / d; return (n % d != 0 && ((n < 0) != (d < 0))) ? q - 1 : q; };
    const long long qmin = fdiv(-(long long)off0, stride), qmax = fdiv((long long)lx - 1 - off0, stride);
    a.M = ceil_div(ntaps, stride); a.Mp = g.Mp; a.TT = g.TT; a.G = g.G; a.qmin = qmin;
    const long long nx = (qmax - qmin + FB_P) / FB_P;
    hipLaunchKernelGGL(fir_bank_kernel<1>, dim3((unsigned)nx, batch, g.row_tiles), dim3(256), g.lds, st, a);
  }
  EBEN_CHECK_LAUNCH("fir_bank_kernel");
  return EBEN_OK;
}

}  // namespace eben
