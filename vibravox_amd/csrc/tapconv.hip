// tapconv.hip -- the MFMA implicit-GEMM "tap convolution" of libeben_hip.so (gfx950).
//
// One kernel covers the two directions of every Conv1d / ConvTranspose1d of the EBEN generator
// and discriminators (reference call sites: eben_generator.py:112-166,241-249,272-280,295-312;
// eben_discriminator.py:66-157; melgan_discriminator.py:89-156) and the STFT of the
// multi-resolution spectral loss (a strided conv against a windowed DFT basis):
//
//   y[b, g*Mg+m, t*OS+oo] = epi( sum_{c<Cg} sum_{j<J} Wp[j,c,m] * xin(b, g*Cg+c, t*S + off0 + j*dstep) )
//
//   GS ("gather-strided", S = conv stride, OS = 1): Conv1d forward / ConvTranspose1d input-gradient.
//   PS ("phase-scatter",  S = 1, OS = conv stride): Conv1d input-gradient / ConvTranspose1d forward,
//        one stride-1 sub-convolution per output phase r = u mod stride (taps k with
//        (r + pad - k*dil) % stride == 0), so no zero-stuffed MACs are ever issued.
//
// GEMM view per (batch item, group): M = output channels, N = output positions, K = (tap, channel).
// fp32 in / fp32 accumulate on v_mfma_f32_16x16x4_f32 (exact fp32, 157 TFLOP/s chip peak).
//   * the input tile (CI_T channels x receptive span) is staged once per channel chunk in LDS,
//     de-interleaved by stride phase so that the 16 lanes of a B fragment read consecutive
//     dwords whatever the stride (conflict-free ds_read_b32);
//   * weights arrive pre-packed [phase][group][chunk][k][Mpad] (weight-norm scale folded in by
//     the pack kernel), so the A tile is a straight float4 copy, register-prefetched one chunk
//     ahead of the MFMAs;
//   * LeakyReLU on load, bias / LeakyReLU / residual / activation-derivative mask in the epilogue;
//   * blockIdx -> tile mapping is XCD-aware (tiles sharing a weight panel stay on one XCD's L2).
#include "common.h"

#include <cstdlib>

namespace eben {

struct TapArgs {
  const float* x;
  const float* xmask;
  const float* wp;
  const float* bias;
  const float* res;
  const float* emask;
  float* y;
  int B, G, Cg, Mg, Mp, Cx, Cy, Lx, Ly;
  int S, OS, dstep, J, KCpad, CI_T, ncc;
  int mode;              // 0 GS, 1 PS
  int off0, nt;          // GS
  int ps_pad, ps_k, ps_d, ps_kstep;  // PS
  int reflect, in_mode;  // in_mode 0: lrelu(x, in_slope); 1: x * lrelu'(xmask, in_slope)
  float in_slope, out_slope, res_slope, emask_slope;
  int accumulate;
  int res_rows, em_seg, em_map[4];
  int PLEN, CSTRIDE;
  unsigned s_magic;      // ceil(2^32 / S)
  int ntt, nmt, nph;
  long long phase_stride;
};

template <int WAVES_M, int WAVES_N, int FM, int FN>
// second launch-bound = waves per SIMD: an 8-wave block needs 4 (<= 128 VGPRs) for two blocks to share
// a CU -- at 133 VGPRs the 128x128 tile silently ran one block per CU
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64, WAVES_M * WAVES_N == 8 ? 4 : 3) void tapconv_kernel(const TapArgs P) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int BM = WAVES_M * FM * 16;
  constexpr int BN = WAVES_N * FN * 16;
  constexpr int KT = 4096 / BM;         // rows of the staged weight chunk
  constexpr int WSTR = BM + 16;         // +16: the 2 k-rows of a half-wave hit disjoint banks
  constexpr int W4_PER_ROW = BM / 4;
  constexpr int W4_PER_THREAD = KT * BM / 4 / NT;
  static_assert(NT == 256 || NT == 512, "4 or 8 waves per block");
  static_assert(W4_PER_THREAD * NT * 4 == 4096, "weight chunk is 4096 floats");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* koff = reinterpret_cast<int*>(smem);
  const int koff_len = ((P.KCpad + KT - 1) / KT) * KT;   // padded: the k-loop always runs KT/4 steps
  float* Ws = smem + koff_len;                           // multiple of 4 -> 16 B aligned
  float* Xs = Ws + KT * WSTR;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kk = lane >> 4;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // ---- tile decode (XCD-aware) ----
  unsigned id = xcd_remap(blockIdx.x, gridDim.x);
  const int tt = id % P.ntt; id /= P.ntt;
  const int b = id % P.B; id /= P.B;
  const int ph = id % P.nph; id /= P.nph;
  const int mt = id % P.nmt;
  const int g = id / P.nmt;
  const int t0 = tt * BN, m0 = mt * BM;

  // ---- per-phase tap geometry ----
  int J = P.J, off0 = P.off0, nt = P.nt, oo = 0;
  if (P.mode == 1) {
    const int s = P.OS;
    int k0 = -1;
    for (int c = 0; c < P.ps_kstep; ++c) {
      int v = (ph + P.ps_pad - c * P.ps_d) % s;
      if (v < 0) v += s;
      if (v == 0) { k0 = c; break; }
    }
    if (k0 >= 0 && k0 < P.ps_k) {
      J = (P.ps_k - 1 - k0) / P.ps_kstep + 1;
      off0 = (ph + P.ps_pad - k0 * P.ps_d) / s;
    } else {
      J = 0;
      off0 = 0;
    }
    nt = ph < P.Ly ? (P.Ly - ph + s - 1) / s : 0;
    oo = ph;
  }
  if (t0 >= nt) return;  // whole block is outside this phase's range (uniform)
  const int minoff = (P.dstep >= 0 || J == 0) ? off0 : off0 + (J - 1) * P.dstep;
  const int adstep = P.dstep >= 0 ? P.dstep : -P.dstep;
  const int span = J > 0 ? (BN - 1) * P.S + (J - 1) * adstep + 1 : 0;
  const int KC = ((J * P.CI_T + 3) >> 2) << 2;  // flat K entries actually used by this phase

  for (int f = tid; f < koff_len; f += NT) {
    const int j = f / P.CI_T, cl = f - j * P.CI_T;
    int o = 0;
    if (f < P.KCpad && j < J) {
      const int rel = off0 + j * P.dstep - minoff;
      int p = 0, dd = rel;
      if (P.S != 1) { dd = (int)__umulhi((unsigned)rel, P.s_magic); p = rel - dd * P.S; }
      o = cl * P.CSTRIDE + p * P.PLEN + dd;
    }
    koff[f] = o;
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int n = 0; n < FN; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* wbase = P.wp + (long long)ph * P.phase_stride + (long long)g * P.ncc * P.KCpad * P.Mp + m0;
  const int q0 = t0 * P.S + minoff;
  const int nkc = (KC + KT - 1) / KT;

  // ---- main loop.  Both operand streams are software-pipelined through registers:
  //  * weights: one 4096-float chunk ahead, continuously across channel-chunk boundaries (the packed
  //    layout is contiguous in consumption order);
  //  * input tile: when it is small (<= XCAP elements: the k=3..7 layers, which would otherwise
  //    expose a global-load latency every ~100 K-rows) the next channel chunk's tile is fetched into
  //    registers under the current chunk's MFMAs; large tiles (k=41 stride-4 layers) are staged
  //    directly -- there the staging is amortised over ~20 weight chunks.
  constexpr int XR = 10;
  constexpr int XCAP = XR * NT;
  const int xtot = P.CI_T * span;
  const bool xpre = xtot <= XCAP && span < 65536;
  float xreg[XR];
  // tile coordinates of this thread's elements: held in registers by the light variants, recomputed at every use (from a copy of
  // the thread id the compiler cannot see through, so nothing is hoisted back) by the 16-fragment ones, which otherwise spill
  constexpr bool XG_REG = FM * FN < 8;
  const unsigned span_magic = span > 1 ? (unsigned)((0x100000000ull + (unsigned)span - 1) / (unsigned)span) : 0u;
  auto xg_make = [&](int t, int u) -> int {
    const int i = t + u * NT;
    if (!(xpre && i < xtot)) return -1;
    const int c = span > 1 ? (int)__umulhi((unsigned)i, span_magic) : i;
    return (c << 16) | (i - c * span);
  };
  int xg_r[XG_REG ? XR : 1];
  if constexpr (XG_REG) {
#pragma unroll
    for (int u = 0; u < XR; ++u) xg_r[u] = xg_make(tid, u);
  }
  auto opaque_tid = [&]() -> int {
    int t = tid;
    if constexpr (!XG_REG) asm volatile("" : "+v"(t));
    return t;
  };
  auto fetch_x = [&](int r, long long row, bool cv) -> float {
    int q = q0 + r;
    if (P.reflect) {
      q = q < 0 ? -q : q;
      q = q >= P.Lx ? 2 * (P.Lx - 1) - q : q;
    }
    float v = 0.f;
    if (cv && q >= 0 && q < P.Lx) {
      v = P.x[row + q];
      if (P.in_mode == 0) v = lrelu(v, P.in_slope);
      else v *= dlrelu(P.xmask[row + q], P.in_slope);
    }
    return v;
  };
  auto lds_x = [&](int c, int r) -> int {
    int p = 0, i = r;
    if (P.S != 1) { i = (int)__umulhi((unsigned)r, P.s_magic); p = r - i * P.S; }
    return c * P.CSTRIDE + p * P.PLEN + i;
  };
  auto load_x = [&](int cc) {
    const int tq = opaque_tid();
#pragma unroll
    for (int u = 0; u < XR; ++u) {
      float v = 0.f;
      const int g_ = XG_REG ? xg_r[XG_REG ? u : 0] : xg_make(tq, u);
      if (g_ >= 0) {
        const int chan = cc * P.CI_T + (g_ >> 16);
        v = fetch_x(g_ & 0xffff, ((long long)b * P.Cx + (long long)g * P.Cg + chan) * P.Lx, chan < P.Cg);
      }
      xreg[u] = v;
    }
  };
  auto store_x = [&]() {
    const int tq = opaque_tid();
#pragma unroll
    for (int u = 0; u < XR; ++u) {
      const int g_ = XG_REG ? xg_r[XG_REG ? u : 0] : xg_make(tq, u);
      if (g_ >= 0) Xs[lds_x(g_ >> 16, g_ & 0xffff)] = xreg[u];
    }
  };
  auto stage_x_direct = [&](int cc) {
    for (int c = 0; c < P.CI_T; ++c) {
      const int chan = cc * P.CI_T + c;
      const long long row = ((long long)b * P.Cx + (long long)g * P.Cg + chan) * P.Lx;
      for (int r = tid; r < span; r += NT) Xs[lds_x(c, r)] = fetch_x(r, row, chan < P.Cg);
    }
  };
  float4 wreg[W4_PER_THREAD];
  auto prefetch_w = [&](int cc, int kc) {
    const float* wcc = wbase + (long long)cc * P.KCpad * P.Mp;
    const int rows = min(KT, KC - kc * KT);
#pragma unroll
    for (int u = 0; u < W4_PER_THREAD; ++u) {
      const int i4 = tid + u * NT;
      const int rrow = i4 / W4_PER_ROW, c4 = i4 - rrow * W4_PER_ROW;
      wreg[u] = rrow < rows ? *reinterpret_cast<const float4*>(wcc + (long long)(kc * KT + rrow) * P.Mp + c4 * 4)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  if (J > 0) {
    if (xpre) load_x(0);
    prefetch_w(0, 0);
  }
  for (int cc = 0; cc < P.ncc && J > 0; ++cc) {
    __syncthreads();  // previous channel chunk's MFMAs are done with Xs / Ws (and koff is published)
    if (xpre) {
      store_x();
      if (cc + 1 < P.ncc) load_x(cc + 1);
    } else {
      stage_x_direct(cc);
    }
    for (int kc = 0; kc < nkc; ++kc) {
      if (kc > 0) __syncthreads();  // MFMAs of the previous chunk finished reading Ws
#pragma unroll
      for (int u = 0; u < W4_PER_THREAD; ++u) {
        const int i4 = tid + u * NT;
        const int rrow = i4 / W4_PER_ROW, c4 = i4 - rrow * W4_PER_ROW;
        *reinterpret_cast<float4*>(Ws + rrow * WSTR + c4 * 4) = wreg[u];
      }
      __syncthreads();
      if (kc + 1 < nkc) prefetch_w(cc, kc + 1);
      else if (cc + 1 < P.ncc) prefetch_w(cc + 1, 0);
      // fixed-trip k-loop (rows past the chunk end are zero weights against a valid offset 0):
      // tap offsets for the whole chunk are read up front, fragments are loaded one k-step ahead
      // of the MFMAs that consume them.
      const float* wrow = Ws + kk * WSTR + wm * FM * 16 + l15;
      const int* ko = koff + kc * KT + kk;
      const float* xcol = Xs + wn * FN * 16 + l15;
      constexpr int UNR = 4;  // k-steps per unrolled block (16 rows of the weight chunk)
      const int nstep = (min(KT, KC - kc * KT) + 3) >> 2;
      for (int kb = 0; kb < nstep; kb += UNR) {
        int xo[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) xo[u] = ko[(kb + u) * 4];
        float a[2][FM], bv[2][FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) a[0][i] = wrow[(kb * 4) * WSTR + i * 16];
#pragma unroll
        for (int n = 0; n < FN; ++n) bv[0][n] = xcol[xo[0] + n * 16];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int cur = u & 1, nxt = cur ^ 1;
          if (u + 1 < UNR) {
#pragma unroll
            for (int i = 0; i < FM; ++i) a[nxt][i] = wrow[((kb + u + 1) * 4) * WSTR + i * 16];
#pragma unroll
            for (int n = 0; n < FN; ++n) bv[nxt][n] = xcol[xo[u + 1] + n * 16];
          }
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int n = 0; n < FN; ++n)
              acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][i], bv[cur][n], acc[i][n], 0, 0, 0);
        }
      }
    }
  }

  // batched right-hand sides: residual row limit and remapped mask row (wave-uniform)
  const bool use_res = P.res != nullptr && (P.res_rows == 0 || b < P.res_rows);
  const int eb = P.em_seg > 0 ? P.em_map[b / P.em_seg] * P.em_seg + b % P.em_seg : b;
  const long long eoff = (long long)(eb - b) * P.Cy * P.Ly;
  // ---- epilogue: D fragment = 4 consecutive rows (m) x 1 column (t) per lane ----
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm * FM * 16 + i * 16 + kk * 4 + r;
      if (m >= P.Mg) continue;
      const float bias = P.bias ? P.bias[g * P.Mg + m] : 0.f;
      const long long yrow = ((long long)b * P.Cy + (long long)g * P.Mg + m) * P.Ly;
#pragma unroll
      for (int n = 0; n < FN; ++n) {
        const int t = t0 + wn * FN * 16 + n * 16 + l15;
        if (t >= nt) continue;
        const long long idx = yrow + (long long)t * P.OS + oo;
        float v = acc[i][n][r] + bias;
        v = lrelu(v, P.out_slope);
        if (use_res) v += lrelu(P.res[idx], P.res_slope);
        if (P.emask) v *= dlrelu(P.emask[idx + eoff], P.emask_slope);
        if (P.accumulate) v += P.y[idx];
        P.y[idx] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// host side: plan, weight packing, launchers
// ---------------------------------------------------------------------------------------

static int gcd_i(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

struct TapPlan {
  int mode;  // 0 GS, 1 PS
  int Cg, Mg, G, CI_T, ncc, J, KCpad, Mp, cfg, BM, BN;
  int S, OS, dstep, kstep, nph, PLEN, CSTRIDE;
  int Lx, Ly, Cx, Cy, off0, nt, ps_pad;
  int ntt, nmt;
  size_t lds_bytes;
  long long phase_stride;
  size_t packed_floats;
};

// The first-generation kernel is the library's UNIVERSAL fp32 fallback: the shapes no later family takes (one-channel inputs with long
// taps such as the dense STFT form, odd row counts).  One configuration serves them all: 16 x 256 tiles on four waves.  (Rounds 1-2 chose
// among eight tile shapes here; every layer those were tuned for now runs on tapconv2 / tapconv3 / gen_conv / thinconv, and none of
// the other seven was launched by the GPU suite or the bench any more: profiles/r05_kernel_coverage.txt.)
constexpr int kTapBM = 16, kTapBN = 256;

// dir 0: canonical forward direction (GS); dir 1: canonical input-gradient direction (PS).
// For PS with reflect padding the output domain is the padded one (caller folds afterwards).
static void make_plan(const Canon& c, int dir, TapPlan* p) {
  p->mode = dir;
  p->G = c.g;
  if (dir == 0) {
    p->Cg = c.Cin / c.g; p->Mg = c.Cout / c.g;
    p->S = c.s; p->OS = 1; p->dstep = c.d; p->kstep = 1; p->nph = 1; p->J = c.k;
    p->Lx = c.Lin; p->Ly = c.Lout; p->Cx = c.Cin; p->Cy = c.Cout;
    p->off0 = -c.pl; p->nt = c.Lout; p->ps_pad = 0;
  } else {
    p->Cg = c.Cout / c.g; p->Mg = c.Cin / c.g;
    p->S = 1; p->OS = c.s;
    p->kstep = c.s / gcd_i(c.s, c.d);
    p->dstep = -(c.d * p->kstep) / c.s;
    p->nph = c.s;
    p->J = ceil_div(c.k, p->kstep);
    p->Lx = c.Lout; p->Cx = c.Cout; p->Cy = c.Cin;
    p->Ly = c.reflect ? c.Lin + c.pl + c.pr : c.Lin;
    p->ps_pad = c.reflect ? 0 : c.pl;
    p->off0 = 0; p->nt = ceil_div(p->Ly, c.s);
  }
  p->cfg = 3;
  p->BM = kTapBM; p->BN = kTapBN;
  p->Mp = round_up(p->Mg, p->BM);
  p->nmt = p->Mp / p->BM;
  p->ntt = ceil_div(p->nt, p->BN);
  // channel chunk: as many input channels per staged tile as 24 KiB of LDS hold (cap 16), evenly
  // split over the group so that no chunk is mostly padding.  Measured on MI355X (tools/layer_bench.py):
  // the kernel is latency-bound, so a small tile (3-4 resident blocks per CU) beats a large one
  // (48 KiB / 64 channels was 10-35 % slower on every heavy layer).
  const int adstep = p->dstep >= 0 ? p->dstep : -p->dstep;
  const int KT = 4096 / p->BM;
  {
    const int maxd = ((p->J - 1) * adstep) / p->S + 1;
    p->PLEN = p->BN + maxd + 1;
    p->CSTRIDE = round_up(p->S * p->PLEN, 32) + 16;
  }
  static const int env_cap = getenv("EBEN_TAP_CI_CAP") ? atoi(getenv("EBEN_TAP_CI_CAP")) : 0;      // tuning aid
  static const int env_kb = getenv("EBEN_TAP_X_KB") ? atoi(getenv("EBEN_TAP_X_KB")) : 0;          // tuning aid
  int cap = (int)(((env_kb > 0 ? env_kb : 24) * 1024) / (4 * (size_t)p->CSTRIDE));
  if (cap > (env_cap > 0 ? env_cap : 16)) cap = env_cap > 0 ? env_cap : 16;
  if (cap < 1) cap = 1;
  int ci;
  if (p->Cg <= cap) ci = p->Cg;
  else {
    const int nch = ceil_div(p->Cg, cap);
    ci = ceil_div(p->Cg, nch);
  }
  for (;;) {
    p->CI_T = ci;
    p->KCpad = round_up(p->J * ci, 4);
    p->lds_bytes = 4ull * ((size_t)round_up(p->KCpad, KT) + (size_t)KT * (p->BM + 16) + (size_t)ci * p->CSTRIDE);
    if (p->lds_bytes <= 160 * 1024 || ci == 1) break;
    ci = ci / 2 > 0 ? ci / 2 : 1;
  }
  p->ncc = ceil_div(p->Cg, p->CI_T);
  p->phase_stride = (long long)p->G * p->ncc * p->KCpad * p->Mp;
  p->packed_floats = (size_t)p->phase_stride * p->nph;
}

// ---- weight packing -----------------------------------------------------------------------
struct PackArgs {
  const float* w;      // canonical (Cout, Cin/g, k)
  const float* scale;  // per Cout row or null
  float* wp;
  int G, Cg, Mg, Mp, CI_T, ncc, KCpad, J, nph;
  int mode, k, s, d, kstep, ps_pad, Cin_g, Cout_g;
  long long phase_stride;
};

__global__ __launch_bounds__(256) void pack_kernel(const PackArgs P) {
  const long long total = P.phase_stride * P.nph;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    long long r = i;
    const int m = r % P.Mp; r /= P.Mp;
    const int f = r % P.KCpad; r /= P.KCpad;
    const int cc = r % P.ncc; r /= P.ncc;
    const int g = r % P.G;
    const int ph = r / P.G;
    const int j = f / P.CI_T, cl = f - j * P.CI_T;
    const int chan = cc * P.CI_T + cl;
    float v = 0.f;
    if (m < P.Mg && chan < P.Cg && j < P.J) {
      if (P.mode == 0) {
        // reduction channel = conv input channel, m = conv output channel, tap j
        const int co = g * P.Cout_g + m;
        v = P.w[((long long)co * P.Cin_g + chan) * P.k + j];
        if (P.scale) v *= P.scale[co];
      } else {
        int k0 = -1;
        for (int c = 0; c < P.kstep; ++c) {
          int q = (ph + P.ps_pad - c * P.d) % P.s;
          if (q < 0) q += P.s;
          if (q == 0) { k0 = c; break; }
        }
        const int kk = k0 + j * P.kstep;
        if (k0 >= 0 && kk < P.k) {
          const int co = g * P.Cout_g + chan;  // reduction channel = conv output channel
          v = P.w[((long long)co * P.Cin_g + m) * P.k + kk];
          if (P.scale) v *= P.scale[co];
        }
      }
    }
    P.wp[i] = v;
  }
}

static int launch_pack(const Canon& c, const TapPlan& p, const float* w, const float* scale, float* wp, hipStream_t st) {
  PackArgs a;
  a.w = w; a.scale = scale; a.wp = wp;
  a.G = p.G; a.Cg = p.Cg; a.Mg = p.Mg; a.Mp = p.Mp; a.CI_T = p.CI_T; a.ncc = p.ncc; a.KCpad = p.KCpad; a.J = p.J; a.nph = p.nph;
  a.mode = p.mode; a.k = c.k; a.s = c.s; a.d = c.d; a.kstep = p.kstep; a.ps_pad = p.ps_pad;
  a.Cin_g = c.Cin / c.g; a.Cout_g = c.Cout / c.g;
  a.phase_stride = p.phase_stride;
  const long long total = p.phase_stride * p.nph;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, st, a);
  EBEN_CHECK_LAUNCH("pack_kernel");
  return EBEN_OK;
}

// ---- tapconv launcher -----------------------------------------------------------------------
template <int WM, int WN, int FM, int FN>
static int launch_cfg(const TapArgs& a, int nblocks, size_t lds, hipStream_t st) {
  static LdsAttrOnce attr_once;
  auto kern = tapconv_kernel<WM, WN, FM, FN>;
  {
    const hipError_t e = lds_attr_once(attr_once, reinterpret_cast<const void*>(kern));
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(tapconv)");
  }
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(WM * WN * 64), lds, st, a);
  EBEN_CHECK_LAUNCH("tapconv_kernel");
  return EBEN_OK;
}

static int launch_tap(const Canon& c, const TapPlan& p, const TapIO& io, int reflect, hipStream_t st) {
  if (p.lds_bytes > 160 * 1024) return fail(EBEN_EUNSUPPORTED, "tapconv tile needs %zu B of LDS", p.lds_bytes);
  TapArgs a;
  a.x = io.x; a.xmask = io.xmask; a.wp = io.wp; a.bias = io.bias; a.res = io.res; a.emask = io.emask; a.y = io.y;
  a.B = c.B; a.G = p.G; a.Cg = p.Cg; a.Mg = p.Mg; a.Mp = p.Mp; a.Cx = p.Cx; a.Cy = p.Cy; a.Lx = p.Lx; a.Ly = p.Ly;
  a.S = p.S; a.OS = p.OS; a.dstep = p.dstep; a.J = p.J; a.KCpad = p.KCpad; a.CI_T = p.CI_T; a.ncc = p.ncc;
  a.mode = p.mode; a.off0 = p.off0; a.nt = p.nt;
  a.ps_pad = p.ps_pad; a.ps_k = c.k; a.ps_d = c.d; a.ps_kstep = p.kstep;
  a.reflect = reflect; a.in_mode = io.in_mode;
  a.in_slope = io.in_slope; a.out_slope = io.out_slope; a.res_slope = io.res_slope; a.emask_slope = io.emask_slope;
  a.accumulate = io.accumulate;
  a.res_rows = io.res_rows; a.em_seg = io.em_seg;
  for (int i = 0; i < 4; ++i) a.em_map[i] = io.em_map[i];
  a.PLEN = p.PLEN; a.CSTRIDE = p.CSTRIDE;
  a.s_magic = p.S > 1 ? (unsigned)((0x100000000ull + p.S - 1) / p.S) : 0u;
  a.ntt = p.ntt; a.nmt = p.nmt; a.nph = p.nph;
  a.phase_stride = p.phase_stride;
  const long long nb = (long long)p.ntt * c.B * p.nph * p.nmt * p.G;
  if (nb <= 0 || nb > 0x7fffffffLL) return fail(EBEN_EINVAL, "tapconv grid of %lld blocks", nb);
  return launch_cfg<1, 4, 1, 4>(a, (int)nb, p.lds_bytes, st);
}

// Single-output-channel convolution (the logits layers: 1024->1 and 768->1, k=3): a channel
// reduction, not a GEMM.  One block = 64 output positions of one batch item, 16 waves splitting the
// channels; lane = position (coalesced rows, taps hit L1), partial sums combined through LDS in a
// fixed order.  Weights are read from the packed layout (scale already folded in).
__global__ __launch_bounds__(1024) void conv_m1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ bias, float* __restrict__ y, int C, int Lx,
                                                           int Ly, int J, int pad, int dil, int CI_T, int KCpad, int Mp,
                                                           float out_slope) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y, t = blockIdx.x * 64 + lane;
  const float* xb = x + (long long)b * C * Lx;
  float acc = 0.f;
  if (J == 3) {
    // the two logits layers (k = 3): four channels' loads in flight per round trip, addresses clamped instead of branched on,
    // the channel-chunk index carried instead of divided for; same FMA order as the generic loop below
    int q[3], ok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int qq = t - pad + j * dil;
      ok[j] = (int)(qq >= 0) & (int)(qq < Lx);
      q[j] = ok[j] ? qq : 0;
    }
    int cc = w / CI_T, cl = w - cc * CI_T;
    for (int c = w; c < C; c += 64) {
      float xv[4][3], wv[4][3];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cu = c + 16 * u;
        const bool live = cu < C;
        const float* xr = xb + (long long)(live ? cu : w) * Lx;
        const float* wc = wp + ((long long)cc * KCpad + cl) * Mp;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          xv[u][j] = xr[q[j]];
          wv[u][j] = live ? wc[(long long)j * CI_T * Mp] : 0.f;
          if (!ok[j]) xv[u][j] = 0.f;
        }
        cl += 16;
        while (cl >= CI_T) { cl -= CI_T; ++cc; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (c + 16 * u < C) acc = fmaf(wv[u][j], xv[u][j], acc);
    }
  } else {
    for (int c = w; c < C; c += 16) {
      const int cc = c / CI_T, cl = c - cc * CI_T;
      const float* xr = xb + (long long)c * Lx;
      const float* wc = wp + ((long long)cc * KCpad + cl) * Mp;
      for (int j = 0; j < J; ++j) {
        const int q = t - pad + j * dil;
        const float xv = (q >= 0 && q < Lx) ? xr[q] : 0.f;
        acc = fmaf(wc[(long long)j * CI_T * Mp], xv, acc);
      }
    }
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && t < Ly) {
    float s = bias ? bias[0] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += part[i][lane];
    y[(long long)b * Ly + t] = lrelu(s, out_slope);
  }
}

// ---- the family's row of conv1d.hip's table (EBEN_CONV_ROUTE_TAP1) ------------------------------------------------------------
size_t tap1_packed_floats(const Canon& c, int dir) {
  TapPlan p;
  make_plan(c, dir, &p);
  return p.packed_floats;
}

int tap1_pack(const Canon& c, int dir, const float* w, const float* scale, float* wp, hipStream_t st) {
  TapPlan p;
  make_plan(c, dir, &p);
  return launch_pack(c, p, w, scale, wp, st);
}

int tap1_launch(const Canon& c, int dir, const TapIO& io, int reflect, hipStream_t st) {
  TapPlan p;
  make_plan(c, dir, &p);
  if (io.conv1d_fwd && c.Cout == 1 && c.g == 1 && c.s == 1 && !c.reflect && io.in_slope == 1.f && !io.res) {
    hipLaunchKernelGGL(conv_m1_fwd_kernel, dim3(ceil_div(c.Lout, 64), c.B), dim3(1024), 0, st, io.x, io.wp, io.bias, io.y,
                       c.Cin, c.Lin, c.Lout, c.k, c.pl, c.d, p.CI_T, p.KCpad, p.Mp, io.out_slope);
    EBEN_CHECK_LAUNCH("conv_m1_fwd_kernel");
    return EBEN_OK;
  }
  return launch_tap(c, p, io, reflect, st);
}

}  // namespace eben

