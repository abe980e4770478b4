// bl_dx_pr.hip -- "phases as rows": the geometry and the primed weights of a strided bundle-layout Conv1d's input gradient written as ONE
// stride-1 Conv1d (libeben_hip.so, gfx950).  The launch itself is eben_bl_conv1d_bwd_dx_pr[_c] in conv1d.hip, on the primed layer's forward image.
//
// Input gradient of a STRIDED Conv1d as "phases as rows" (melgan_discriminator.py:97-118: k 41, stride 4, 4 groups).  The phase-scatter
// form (tap3 mode 1) runs one stride-1 sub-convolution per output phase: `stride` blocks stage the same window of dy, each with a
// quarter of the taps, and a layer with few channels per group (16 -> 64: four input channels per group) fills an eighth of its MFMA
// rows.  Written for all phases at once,
//     dx[c, S q + ph] = sum_{co, u} W[co, c, ph + pad - S u] dy[co, q + u],
// the input gradient IS a stride-1 Conv1d from the Cout channels of dy to S Cin output rows (ph, c) with taps u = umin .. umax (11 for
// k 41 / S 4) whose result is stored depth-to-space: MelGAN L1 / L2 become grouped 64 -> 64 / 256 -> 256 k 11 convolutions, dy staged
// once, full row tiles.  The primed weights W'[(ph, c)][co][u] are a gather of the layer's weights (pr_weights_kernel), packed as an
// ordinary forward image of the primed layer; tap3's bundle epilogue maps logical bundle -> (physical bundle, phase) (Tap3Args.pr_*).
#include "common.h"

#include <cstdlib>

namespace eben {

static int pr_floordiv(int a, int b) { int q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }

PrGeom pr_geometry(const Canon& c, Canon* cp) {
  PrGeom g{};
  static const int min_s = getenv("EBEN_PR_MIN_STRIDE") ? atoi(getenv("EBEN_PR_MIN_STRIDE")) : 4;
  static const int max_d = getenv("EBEN_PR_MAX_DIL") ? atoi(getenv("EBEN_PR_MAX_DIL")) : 1;
  // stride 2 (the PQMF-band layers) in bundle-major row order on tap3_kernel, up to this dilation (0: off).  [MI355X, 128 rows] the five
  // stride-2 input gradients of a chain at dilation 1: 0.063 / 0.070 / 0.055 / 0.062 / 0.070 -> 0.053 / 0.052 / 0.045 / 0.046 / 0.064 ms,
  // at dilation 2 (7 primed taps for 4 + 3): 0.071 / 0.085 / 0.064 / 0.077 / 0.089 -> 0.061 / 0.063 / 0.050 / 0.057 / 0.085; at dilation
  // 3 (10 primed taps) the extra products cost what the whole-unit epilogue saves: 0.057 / 0.066 / 0.054 / 0.063 / 0.071 -> 0.064 /
  // 0.069 / 0.054 / 0.065 / 0.070
  static const int s2_max_d = getenv("EBEN_PR2_S2_MAX_DIL") ? atoi(getenv("EBEN_PR2_S2_MAX_DIL")) : 2;
  const bool s2 = c.s == 2 && c.d <= s2_max_d;
  if (!c.bl || c.np != 1 || c.reflect || (c.d > max_d && !s2) || c.s < 2 || (c.s < min_s && !s2) || c.s > 8 || (c.k - 1) * c.d + 1 <= c.s || c.pl > (c.k - 1) * c.d) return g;
  const int Cg = c.Cin / c.g;
  if ((c.Cin & 7) || (c.Cout & 7)) return g;
  g.S = c.s;
  // dilation d: tap j sits at offset j d, i.e. W' is nonzero where ph + pad - S u is a multiple of d inside [0, (k - 1) d]
  g.umin = -pr_floordiv((c.k - 1) * c.d - c.pl, c.s);     // ceil((pad - (k - 1) d) / S): phase 0, last tap
  const int umax = pr_floordiv(c.s - 1 + c.pl, c.s);      // phase S - 1, tap 0
  g.kq = umax - g.umin + 1;
  g.Lq = ceil_div(c.Lin, c.s);
  g.fold = (Cg & 7) != 0;                                  // groups that do not start on bundles: one dense (block-diagonal) contraction
  g.cbg = g.fold ? c.Cin / 8 : Cg / 8;
  Canon q = c;
  q.Cin = c.Cout; q.Cout = c.s * c.Cin; q.Lin = c.Lout; q.Lout = g.Lq;
  q.k = g.kq; q.s = 1; q.d = 1; q.g = g.fold ? 1 : c.g;
  q.pl = -g.umin;
  q.pr = g.Lq - c.Lout + g.kq - 1 - q.pl;
  if (q.pl < 0 || q.pr < 0) return g;
  q.reflect = 0; q.xsplit_dir = -1;
  // [MI355X, 128 rows] MelGAN L1 / L2 (4 / 16 channels per group: 64 primed rows per group) 0.336 / 0.310 -> 0.239 / 0.210 ms; L3 / L4 (64 /
  // 256 channels per group: 256 / 1024 primed rows, full row tiles in either form) 0.414 / 0.412 -> 0.531 / 0.524: the form is for the layers
  // whose phases leave row tiles empty
  static const int max_rows = getenv("EBEN_PR_MAX_ROWS") ? atoi(getenv("EBEN_PR_MAX_ROWS")) : 64;
  // Wider layers (MelGAN L3 / L4: 256 / 1024 primed rows per group) take the form on tap4_kernel (bigtap.hip) with the rows ordered
  // (channel bundle, phase, channel in bundle): a 32-row MFMA tile is then ONE bundle at the four phases of a position, i.e. 64
  // contiguous bytes per column -- the phase-scatter form writes (and reads its mask as) 8-byte pieces 64 bytes apart, which a
  // block per CU cannot hide ([MI355X] phase-scatter on tap4: 0.416 / 0.402 -> 0.506 / 0.444 ms)
  static const int big_pr = getenv("EBEN_PR_BIG") ? atoi(getenv("EBEN_PR_BIG")) : 1;
  // ... and the narrow ones (MelGAN L1 / L2: 64 primed rows per group, tap3_kernel) take the same row order: their mask / feature-matching
  // operands and results move as whole units too ([MI355X] those loads were 36-43 % of the order-0 launches)
  static const int small_pr2 = getenv("EBEN_PR2_TAP3") ? atoi(getenv("EBEN_PR2_TAP3")) : 1;
  g.order = (big_pr && c.s == 4 && c.d == 1 && (tap3_is_big(q, 0) || (small_pr2 && (q.Cout / q.g) % 32 == 0))) ? 1 : 0;
  if (s2) {   // two bundles per 32-row tile: whole bundles at both phases, tap3_kernel only
    if (tap3_is_big(q, 0) || (q.Cout / q.g) % 16 != 0) return g;
    g.order = 1;
  }
  if (q.Cout / q.g > max_rows && !g.order) return g;
  if (!tap3_applicable(q, 0)) return g;   // is the PRIMED layer covered -- not a choice of family for `c`
  if (cp) *cp = q;
  g.ok = 1;
  return g;
}

// W'[(g, ph, c)][co][ui] (groups kept) or [(ph, ci)][co][ui] (folded, zero across groups) = scale[co] v[co][c][ph + pad - S (ui + umin)]
__global__ __launch_bounds__(256) void pr_weights_kernel(const float* __restrict__ v, const float* __restrict__ scale, float* __restrict__ wq,
                                                          int Cin, int Cout, int G, int k, int S, int pad, int umin, int kq, int fold, int dil, int order) {
  const int Cg = Cin / G, Mg = Cout / G;
  const int cin_q = fold ? Cout : Mg;                      // input channels per group of the primed layer
  const long long total = (long long)S * Cin * cin_q * kq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ui = (int)(i % kq);
    long long r = i / kq;
    const int cq = (int)(r % cin_q);
    const int row = (int)(r / cin_q);
    int ph, ci, co;
    if (fold && order) { const int lb = row >> 3, cb = lb / S; ph = lb - cb * S; ci = cb * 8 + (row & 7); co = cq; }
    else if (fold) { ph = row / Cin; ci = row - ph * Cin; co = cq; }
    else if (order == 0) { const int g = row / (S * Cg), rr = row - g * S * Cg; ph = rr / Cg; ci = g * Cg + (rr - ph * Cg); co = g * Mg + cq; }
    else {   // (group, channel bundle, phase, channel in bundle)
      const int g = row / (S * Cg), rr = row - g * S * Cg, lb = rr >> 3, cb = lb / S;
      ph = lb - cb * S; ci = g * Cg + cb * 8 + (rr & 7); co = g * Mg + cq;
    }
    const int off = ph + pad - S * (ui + umin);              // = j dil for the tap this entry stands for, if any
    const int j = off / dil;
    float w = 0.f;
    if (off >= 0 && j * dil == off && j < k && co / Mg == ci / Cg) w = v[((long long)co * Cg + (ci % Cg)) * k + j] * (scale ? scale[co] : 1.f);
    wq[i] = w;
  }
}

static void pr_desc_from_canon(const EbenConv1dDesc* d, const Canon& q, EbenConv1dDesc* o) {
  *o = *d;
  o->c_in = q.Cin; o->c_out = q.Cout; o->l_in = q.Lin; o->l_out = q.Lout; o->ksize = q.k; o->stride = 1; o->dilation = 1; o->groups = q.g;
  o->pad_l = q.pl; o->pad_r = q.pr; o->pad_mode = EBEN_PAD_ZERO; o->transposed = 0; o->in_slope = 1.f; o->out_slope = 1.f;
}
}  // namespace eben

using namespace eben;

extern "C" int eben_bl_dx_pr_desc(const EbenConv1dDesc* d, EbenConv1dDesc* primed) {
  Canon c, q;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  if (d->transposed || !pr_geometry(c, &q).ok) return fail(EBEN_EUNSUPPORTED, "eben_bl_dx_pr_desc: the layer's input gradient has no phases-as-rows form");
  EBEN_REQUIRE(primed != nullptr, "null output descriptor");
  pr_desc_from_canon(d, q, primed);
  return EBEN_OK;
}

extern "C" int eben_bl_dx_pr_weights(const EbenConv1dDesc* d, const float* v, const float* scale, float* w_primed, void* stream) {
  Canon c, q;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  const PrGeom g = d->transposed ? PrGeom{} : pr_geometry(c, &q);
  if (!g.ok) return fail(EBEN_EUNSUPPORTED, "eben_bl_dx_pr_weights: the layer's input gradient has no phases-as-rows form");
  EBEN_REQUIRE(v && w_primed, "null pointer in eben_bl_dx_pr_weights");
  const long long total = (long long)q.Cout * (q.Cin / q.g) * q.k;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pr_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), v, scale, w_primed, c.Cin, c.Cout, c.g, c.k, c.s, c.pl,
                     g.umin, g.kq, g.fold, c.d, g.order);
  EBEN_CHECK_LAUNCH("pr_weights_kernel");
  return EBEN_OK;
}
