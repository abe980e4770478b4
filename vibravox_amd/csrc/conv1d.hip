// conv1d.hip -- the conv forward / input-gradient entry points of libeben_hip.so (gfx950): descriptor -> canonical conv (Canon) ->
// conv_route() -> the family's row of kConvFamilies.  The kernels, plans and packed layouts live with their families (tapconv.hip,
// tapconv2.hip, thinconv.hip, tapconv3.hip + bigtap.hip, gen_conv.hip); a new family is one EBEN_CONV_ROUTE_* value, one clause of
// conv_route() and one table row.  The weight-gradient side has the same shape in conv_dw.hip (dw_route()).
#include "common.h"
#include "tap3.h"

#include <cstdlib>

namespace eben {

int canon_from_desc(const EbenConv1dDesc* d, Canon* c) {
  EBEN_REQUIRE(d != nullptr, "null conv descriptor");
  EBEN_REQUIRE(d->batch > 0 && d->c_in > 0 && d->c_out > 0 && d->l_in > 0 && d->l_out > 0, "non-positive conv dims");
  EBEN_REQUIRE(d->ksize > 0 && d->stride > 0 && d->dilation > 0 && d->groups > 0, "non-positive conv params");
  EBEN_REQUIRE(d->c_in % d->groups == 0 && d->c_out % d->groups == 0, "channels not divisible by groups");
  EBEN_REQUIRE(d->stride <= 1024 && d->pad_l >= 0 && d->pad_r >= 0, "bad stride / padding");
  c->B = d->batch; c->k = d->ksize; c->s = d->stride; c->d = d->dilation; c->g = d->groups;
  c->pl = d->pad_l; c->pr = d->pad_r;
  const int math = d->math & ~EBEN_LAYOUT_BL;
  EBEN_REQUIRE(math >= EBEN_MATH_F32 && math <= EBEN_MATH_BF16X6, "unknown math mode %d", d->math);
  c->bl = (d->math & EBEN_LAYOUT_BL) != 0;
  EBEN_REQUIRE(!c->bl || math == EBEN_MATH_BF16 || math == EBEN_MATH_BF16X3, "the bundle layout carries EBEN_MATH_BF16 / EBEN_MATH_BF16X3 only");
  c->bf16 = math != EBEN_MATH_F32;
  c->np = math == EBEN_MATH_BF16X3 ? 2 : (math == EBEN_MATH_BF16X6 ? 3 : 1);
  c->xsplit_dir = math == EBEN_MATH_BF16X2 ? (d->transposed ? 1 : 0) : -1;
  if (!d->transposed) {
    c->Cin = d->c_in; c->Cout = d->c_out; c->Lin = d->l_in; c->Lout = d->l_out;
    c->reflect = d->pad_mode == EBEN_PAD_REFLECT;
    const int expect = (d->l_in + d->pad_l + d->pad_r - d->dilation * (d->ksize - 1) - 1) / d->stride + 1;
    EBEN_REQUIRE(expect == d->l_out, "Conv1d l_out %d does not match the expected %d", d->l_out, expect);
    if (c->reflect) EBEN_REQUIRE(d->pad_l < d->l_in && d->pad_r < d->l_in, "reflect padding must be smaller than the input");
  } else {
    EBEN_REQUIRE(d->pad_mode == EBEN_PAD_ZERO, "ConvTranspose1d only supports zero padding");
    c->Cin = d->c_out; c->Cout = d->c_in; c->Lin = d->l_out; c->Lout = d->l_in;
    c->reflect = 0;
    c->pr = d->pad_l;
    // l_out = (l_in-1)*s - 2p + d(k-1) + output_padding + 1 with 0 <= output_padding < s
    const int base = (d->l_in - 1) * d->stride - 2 * d->pad_l + d->dilation * (d->ksize - 1) + 1;
    EBEN_REQUIRE(d->l_out >= base && d->l_out < base + d->stride, "ConvTranspose1d l_out %d outside [%d,%d)", d->l_out, base, base + d->stride);
  }
  return EBEN_OK;
}

// ---- the route of one (layer, pass) and the family table ------------------------------------------------------------------------
struct ConvRoute {
  int family;    // row of kConvFamilies: EBEN_CONV_ROUTE_NONE .. _GC (the big form is TAP3 with `big`, reported as _TAP4)
  int dir;       // tap direction: 0 gather-strided (the canonical conv), 1 phase-scatter (its adjoint)
  int big;       // TAP3 launches that tap3_launch hands to tap4_kernel (bigtap.hip)
  int reflect;   // the padding the launch itself reflects: a forward's (input gradients fold theirs in a pass of their own)
  int reported() const { return big ? EBEN_CONV_ROUTE_TAP4 : family; }   // eben_conv1d_kernel_generation's answer
};

// THE decision of which family serves a pass (which 0: the layer's forward, 1: its input gradient).  Nothing else flips
// transposed / which into a tap direction or asks a family whether it is applicable in order to choose one.
static ConvRoute conv_route(const Canon& c, int transposed, int which) {
  static const int thin_first = getenv("EBEN_THIN_FIRST") ? atoi(getenv("EBEN_THIN_FIRST")) : 0;
  ConvRoute r{};
  const int dir = r.dir = transposed ? 1 - which : which;
  r.reflect = which == 0 && c.reflect;
  if (which == 0 && gc_applicable(c, dir)) r.family = EBEN_CONV_ROUTE_GC;   // the direct-operand conv serves forwards only
  else if (c.bl) r.family = tap3_applicable(c, dir) ? EBEN_CONV_ROUTE_TAP3 : EBEN_CONV_ROUTE_NONE;   // bundle layout: the bf16 tap-conv or nothing
  else if (c.bf16 && tap3_applicable(c, dir)) r.family = EBEN_CONV_ROUTE_TAP3;   // layers the bf16 kernel does not cover keep their fp32 kernel
  else {
    const int t2 = tap2_applicable(c, dir), th = thin_applicable(c, dir);
    r.family = th && (thin_first || !t2) ? EBEN_CONV_ROUTE_THIN : t2 ? EBEN_CONV_ROUTE_TAP2 : EBEN_CONV_ROUTE_TAP1;
  }
  r.big = r.family == EBEN_CONV_ROUTE_TAP3 && tap3_is_big(c, dir);
  return r;
}

struct ConvFamily {
  size_t (*packed_floats)(const Canon& c, int dir);
  int (*pack)(const Canon& c, int dir, const float* w, const float* scale, float* wp, hipStream_t st);
  int (*launch)(const Canon& c, int dir, const TapIO& io, int reflect, hipStream_t st);
  int has_fm_epilogue;   // the launch forms the feature-matching gradient in its epilogue (TapIO.fm_sums)
};

// gen_conv.hip reads the reflect padding off the canon
static int gc_launch_row(const Canon& c, int dir, const TapIO& io, int, hipStream_t st) { return gc_launch(c, dir, io, st); }
// A bundle-layout layer off the bf16 tap-conv has no kernel (the eben_bl_* entry points say so themselves).  Its image size is
// answered as TAP1's: callers size a buffer before they learn that nothing packs it.
static int none_pack(const Canon&, int, const float*, const float*, float*, hipStream_t) {
  return fail(EBEN_EUNSUPPORTED, "conv1d_pack: no kernel family serves this bundle-layout layer");
}
static int none_launch(const Canon&, int, const TapIO&, int, hipStream_t) {
  return fail(EBEN_EUNSUPPORTED, "conv1d: no kernel family serves this bundle-layout layer");
}

static const ConvFamily kConvFamilies[] = {
    /* EBEN_CONV_ROUTE_NONE */ {tap1_packed_floats, none_pack, none_launch, 0},
    /* EBEN_CONV_ROUTE_TAP1 */ {tap1_packed_floats, tap1_pack, tap1_launch, 0},
    /* EBEN_CONV_ROUTE_TAP2 */ {tap2_packed_floats, tap2_pack, tap2_launch, 0},
    /* EBEN_CONV_ROUTE_THIN */ {thin_packed_floats, thin_pack, thin_launch, 1},
    /* EBEN_CONV_ROUTE_TAP3 */ {tap3_packed_floats, tap3_pack, tap3_launch, 1},
    /* EBEN_CONV_ROUTE_GC   */ {gc_packed_floats, gc_pack, gc_launch_row, 0},
    /* EBEN_CONV_ROUTE_TAP4 */ {tap3_packed_floats, tap3_pack, tap3_launch, 1},   // tap3_launch picks tap4_kernel off its own plan
};
static_assert(sizeof(kConvFamilies) / sizeof(kConvFamilies[0]) == EBEN_CONV_ROUTE_TAP4 + 1, "one row per EBEN_CONV_ROUTE_*");

// reflect-pad fold: dx[u] = D[u+pl] + D[pl-u] (1<=u<=pl) + D[pl+2(L-1)-u] (L-1-pr<=u<=L-2) (+ pre), then mask (+ post)
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ D, const float* __restrict__ mask, float* __restrict__ dx,
                                                   long long rows, int L, int pl, int pr, float slope, int accumulate,
                                                   const float* __restrict__ pre, const float* __restrict__ post) {
  const int Lp = L + pl + pr;
  const long long total = rows * L;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / L;
    const int u = (int)(i - row * L);
    const float* d = D + row * Lp;
    float v = d[u + pl];
    if (u >= 1 && u <= pl) v += d[pl - u];
    if (u >= L - 1 - pr && u <= L - 2) v += d[pl + 2 * (L - 1) - u];
    if (pre) v += pre[i];
    if (mask) v *= dlrelu(mask[i], slope);
    if (post) v += post[i];
    if (accumulate) v += dx[i];
    dx[i] = v;
  }
}

}  // namespace eben

using namespace eben;

extern "C" size_t eben_conv1d_packed_floats(const EbenConv1dDesc* d, int which) {
  Canon c;
  if (canon_from_desc(d, &c) != EBEN_OK) return 0;
  const ConvRoute r = conv_route(c, d->transposed, which);
  return kConvFamilies[r.family].packed_floats(c, r.dir);
}

extern "C" int eben_conv1d_kernel_generation(const EbenConv1dDesc* d, int which) {
  Canon c;
  if (canon_from_desc(d, &c) != EBEN_OK) return EBEN_CONV_ROUTE_NONE;
  return conv_route(c, d->transposed, which).reported();
}

extern "C" int eben_conv1d_variant(const EbenConv1dDesc* d, int which, int mask_on_load, int* out, int n) {
  EBEN_REQUIRE(out && n >= 8 && (which == 0 || which == 1), "eben_conv1d_variant: which 0 / 1 and 8 output slots");
  EBEN_REQUIRE(!mask_on_load || which == 1, "eben_conv1d_variant: the mask is applied on load by input gradients only");
  Canon c;
  const int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  const ConvRoute r = conv_route(c, d->transposed, which);
  out[0] = r.reported();
  if (r.family == EBEN_CONV_ROUTE_GC) {   // gc_kernel<FORM, RT, CT, NP>
    if (gc_variant(c, r.dir, &out[1], &out[2], &out[3], &out[4])) out[7] = EBEN_VARIANT_GC;
    return EBEN_OK;
  }
  if (r.family != EBEN_CONV_ROUTE_TAP3) return EBEN_OK;
  // the launch as the entry points build it
  Tap3Call k{};
  k.bl = c.bl; k.in_mode = mask_on_load ? 1 : 0; k.reflect = r.reflect;
  Tap3Variant v;
  if (const int e = tap3_plan_variant(c, r.dir, k, &v)) return e;
  out[1] = v.FM; out[2] = v.XRB; out[3] = v.IM; out[4] = v.NPW; out[5] = v.NPX; out[6] = v.BL; out[7] = v.kernel;
  return EBEN_OK;
}

extern "C" int eben_conv1d_variant_f32(const EbenConv1dDesc* d, int which, int mask_on_load, int* out, int n) {
  EBEN_REQUIRE(out && n >= 8 && (which == 0 || which == 1), "eben_conv1d_variant_f32: which 0 / 1 and 8 output slots");
  EBEN_REQUIRE(!mask_on_load || which == 1, "eben_conv1d_variant_f32: the mask is applied on load by input gradients only");
  Canon c;
  const int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  const ConvRoute r = conv_route(c, d->transposed, which);
  out[0] = r.reported();
  if (r.family == EBEN_CONV_ROUTE_THIN) return thin_plan_variant(c, r.dir, &out[1]);
  if (r.family == EBEN_CONV_ROUTE_TAP2) return tap2_plan_variant(c, r.dir, mask_on_load ? 1 : 0, &out[1]);
  return EBEN_OK;
}

extern "C" int eben_conv1d_pack(const EbenConv1dDesc* d, const float* v, const float* scale, float* wp_fwd, float* wp_bwd, void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(v != nullptr, "null weight");
  for (int which = 0; which < 2; ++which) {
    float* dst = which == 0 ? wp_fwd : wp_bwd;
    if (!dst) continue;
    const ConvRoute r = conv_route(c, d->transposed, which);
    if ((rc = kConvFamilies[r.family].pack(c, r.dir, v, scale, dst, as_stream(stream)))) return rc;
  }
  return EBEN_OK;
}

extern "C" int eben_conv1d_pack_multi(const EbenPackJob* jobs, int n, void* stream) {
  EBEN_REQUIRE(n >= 0 && (n == 0 || jobs != nullptr), "bad pack job list");
  // images of the bf16 tap-conv family (most of a step's ~150 pack launches) are gathered into launches of 16 jobs; the other
  // families keep their own launches
  constexpr int CAP = 512;
  static thread_local Canon cs[CAP];
  static thread_local int dirs[CAP];
  static thread_local const float* ws[CAP];
  static thread_local const float* scs[CAP];
  static thread_local float* wps[CAP];
  int m = 0;
  auto flush = [&]() -> int {
    const int rc = m ? tap3_pack_multi(cs, dirs, ws, scs, wps, m, as_stream(stream)) : EBEN_OK;
    m = 0;
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    const EbenPackJob& jb = jobs[i];
    Canon c;
    int rc = canon_from_desc(&jb.desc, &c);
    if (rc) return rc;
    EBEN_REQUIRE(jb.v != nullptr, "null weight");
    for (int which = 0; which < 2; ++which) {
      float* dst = which == 0 ? jb.wp_fwd : jb.wp_bwd;
      if (!dst) continue;
      const ConvRoute r = conv_route(c, jb.desc.transposed, which);
      if (r.family == EBEN_CONV_ROUTE_TAP3) {
        if (m == CAP && (rc = flush())) return rc;
        cs[m] = c; dirs[m] = r.dir; ws[m] = jb.v; scs[m] = jb.scale; wps[m] = dst;
        ++m;
      } else if ((rc = kConvFamilies[r.family].pack(c, r.dir, jb.v, jb.scale, dst, as_stream(stream)))) {
        return rc;
      }
    }
  }
  return flush();
}

static int conv1d_fwd_impl(const EbenConv1dDesc* d, const float* x, const float* wp_fwd, const float* bias,
                           const float* residual, float res_slope, float* y, void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(x && wp_fwd && y, "null pointer in conv1d_fwd");
  const ConvRoute r = conv_route(c, d->transposed, 0);
  TapIO io{};
  io.x = x; io.in_mode = 0; io.in_slope = d->in_slope; io.wp = wp_fwd; io.bias = bias;
  io.res = residual; io.res_slope = res_slope; io.emask = nullptr; io.emask_slope = 1.f;
  io.out_slope = d->out_slope; io.y = y; io.accumulate = 0;
  io.conv1d_fwd = !d->transposed;
  return kConvFamilies[r.family].launch(c, r.dir, io, r.reflect, as_stream(stream));
}

extern "C" int eben_conv1d_fwd(const EbenConv1dDesc* d, const float* x, const float* wp_fwd, const float* bias,
                               const float* residual, float* y, void* stream) {
  return conv1d_fwd_impl(d, x, wp_fwd, bias, residual, 1.f, y, stream);
}

extern "C" int eben_conv1d_fwd_res(const EbenConv1dDesc* d, const float* x, const float* wp_fwd, const float* bias,
                                   const float* residual, float res_slope, float* y, void* stream) {
  EBEN_REQUIRE(residual != nullptr, "conv1d_fwd_res without a residual");
  return conv1d_fwd_impl(d, x, wp_fwd, bias, residual, res_slope, y, stream);
}

extern "C" size_t eben_conv1d_bwd_dx_workspace(const EbenConv1dDesc* d) {
  Canon c;
  if (canon_from_desc(d, &c) != EBEN_OK) return 0;
  if (!d->transposed && c.reflect) return sizeof(float) * (size_t)c.B * c.Cin * (c.Lin + c.pl + c.pr);
  return 0;
}

static int conv1d_bwd_dx_impl(const EbenConv1dDesc* d, const float* dy, const float* y, const float* wp_bwd, const float* x,
                              const float* res_pre, const float* res_post, float* dx, int accumulate, void* workspace, size_t ws_bytes,
                              void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(dy && wp_bwd && dx, "null pointer in conv1d_bwd_dx");
  EBEN_REQUIRE(d->out_slope == 1.f || y, "y is required to differentiate the fused output activation");
  EBEN_REQUIRE(d->in_slope == 1.f || x, "x is required to differentiate the fused input activation");
  hipStream_t st = as_stream(stream);
  const ConvRoute r = conv_route(c, d->transposed, 1);
  TapIO io{};
  io.x = dy; io.wp = wp_bwd; io.bias = nullptr; io.res = nullptr; io.res_slope = 1.f; io.out_slope = 1.f;
  if (d->out_slope != 1.f) { io.in_mode = 1; io.xmask = y; io.in_slope = d->out_slope; }
  else { io.in_mode = 0; io.in_slope = 1.f; }
  // a reflect-padded Conv1d: the conv writes the gradient of the PADDED input into the workspace, and the fold pass applies the
  // addends, the mask and `accumulate`; otherwise the conv's own epilogue does and writes dx
  const bool fold = !d->transposed && c.reflect;
  if (fold) {
    const size_t need = eben_conv1d_bwd_dx_workspace(d);
    if (!workspace || ws_bytes < need) return fail(EBEN_EWORKSPACE, "bwd_dx needs %zu workspace bytes, got %zu", need, ws_bytes);
    io.emask = nullptr; io.emask_slope = 1.f; io.y = static_cast<float*>(workspace); io.accumulate = 0;
  } else {
    if (res_post) return fail(EBEN_EUNSUPPORTED, "bwd_dx: an addend behind the input-activation mask needs the reflect-fold pass");
    io.res = res_pre;
    io.emask = d->in_slope != 1.f ? x : nullptr; io.emask_slope = d->in_slope;
    io.y = dx; io.accumulate = accumulate;
  }
  rc = kConvFamilies[r.family].launch(c, r.dir, io, r.reflect, st);
  if (rc || !fold) return rc;
  const long long rows = (long long)c.B * c.Cin;
  long long blocks = (rows * c.Lin + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const float*>(workspace),
                     d->in_slope != 1.f ? x : nullptr, dx, rows, c.Lin, c.pl, c.pr, d->in_slope, accumulate, res_pre, res_post);
  EBEN_CHECK_LAUNCH("fold_kernel");
  return EBEN_OK;
}

extern "C" int eben_conv1d_bwd_dx(const EbenConv1dDesc* d, const float* dy, const float* y, const float* wp_bwd,
                                  const float* x, float* dx, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
  return conv1d_bwd_dx_impl(d, dy, y, wp_bwd, x, nullptr, nullptr, dx, accumulate, workspace, ws_bytes, stream);
}

extern "C" int eben_conv1d_bwd_dx_res(const EbenConv1dDesc* d, const float* dy, const float* y, const float* wp_bwd, const float* x,
                                      const float* res_pre, const float* res_post, float* dx, void* workspace, size_t ws_bytes,
                                      void* stream) {
  return conv1d_bwd_dx_impl(d, dy, y, wp_bwd, x, res_pre, res_post, dx, 0, workspace, ws_bytes, stream);
}

// Batched input gradient for several right-hand sides that share one set of saved activations
// (the discriminator backward of the fused train step: feature-matching, adversarial, fake and real
// seeds stacked along the batch axis):
//   dx[b] = ( conv^T(g[b]) + (b < res_rows ? res[b] : 0) ) * lrelu'(mask[map(b)], mask_slope)
// g is consumed as is: the producer already applied its activation derivative in ITS epilogue, so no
// kernel on this path reads a mask on load.
static int bwd_dx_batched(const EbenConv1dDesc* d, const float* g, const float* wp_bwd, const float* res, int res_rows, const float* fm_sums,
                          float fm_gs, const float* mask, float mask_slope, int seg, const int* seg_map, float* dx, void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(g && wp_bwd && dx, "null pointer in conv1d_bwd_dx_ex");
  EBEN_REQUIRE(!(c.reflect && !d->transposed), "bwd_dx_ex does not fold reflect padding (pad explicitly)");
  EBEN_REQUIRE(seg >= 0 && (seg == 0 || (seg_map && c.B <= 4 * seg)), "bad batch segment map");
  TapIO io{};
  io.x = g; io.in_mode = 0; io.in_slope = 1.f; io.wp = wp_bwd; io.out_slope = 1.f;
  io.res = res; io.res_slope = 1.f; io.res_rows = res_rows;
  io.emask = mask; io.emask_slope = mask_slope; io.em_seg = mask ? seg : 0;
  for (int i = 0; i < 4; ++i) io.em_map[i] = (seg > 0 && seg_map) ? seg_map[i] : i;
  io.y = dx; io.accumulate = 0;
  io.fm_sums = fm_sums; io.fm_gs = fm_gs;
  const ConvRoute r = conv_route(c, d->transposed, 1);
  const ConvFamily& f = kConvFamilies[r.family];
  if (fm_sums && !f.has_fm_epilogue) return fail(EBEN_EUNSUPPORTED, "conv1d_bwd_dx_fm: EBEN_CONV_ROUTE_* %d has no feature-matching epilogue", r.reported());
  return f.launch(c, r.dir, io, r.reflect, as_stream(stream));
}
extern "C" int eben_conv1d_bwd_dx_ex(const EbenConv1dDesc* d, const float* g, const float* wp_bwd, const float* res, int res_rows,
                                     const float* mask, float mask_slope, int seg, const int* seg_map, float* dx, void* stream) {
  return bwd_dx_batched(d, g, wp_bwd, res, res_rows, nullptr, 0.f, mask, mask_slope, seg, seg_map, dx, stream);
}
// The same launch with the feature-matching gradient of the embedding formed in the epilogue instead of read from a buffer a separate
// kernel wrote (feature_loss.py:40-47: d/da [ sum|a - b| / sum|a| ] = sgn(a - b) / s2 - s1 sgn(a) / s2^2):
//   dx[b] = ( conv^T(g[b]) + (b < fm_rows ? fm_gs (sgn(mask[b] - ref[b]) / s2 - s1 sgn(mask[b]) / s2^2) : 0) ) * lrelu'(mask[map(b)])
// with (s1, s2) = fm_sums[0..1] read on the device.  Only the families whose table row says has_fm_epilogue (THIN and TAP3, the
// ones the discriminators' input gradients run on) carry this epilogue: EBEN_EUNSUPPORTED otherwise (use eben_fm_bwd + bwd_dx_ex).
extern "C" int eben_conv1d_bwd_dx_fm(const EbenConv1dDesc* d, const float* g, const float* wp_bwd, const float* ref, int fm_rows,
                                     const float* fm_sums, float fm_gs, const float* mask, float mask_slope, int seg, const int* seg_map,
                                     float* dx, void* stream) {
  EBEN_REQUIRE(ref && fm_sums && mask && fm_rows > 0, "bad feature-matching arguments in conv1d_bwd_dx_fm");
  return bwd_dx_batched(d, g, wp_bwd, ref, fm_rows, fm_sums, fm_gs, mask, mask_slope, seg, seg_map, dx, stream);
}

// ---- bundle layout (EBEN_LAYOUT_BL): the discriminator layers between the chain heads and the logits ------------------------------
namespace eben {
// operands of a bundle-layout batched input gradient (eben_bl_conv1d_bwd_dx_c / eben_bl_conv1d_bwd_dx_pr_c, which name themselves in `who`)
static int bl_dx_io(const char* who, const Canon& c, const void* g_hi, const float* wp, const void* act_hi, const void* act_lo, const void* fm_codes,
                    float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset, const float* fm_sums, float fm_gs, void* dx_hi,
                    void* dx_lo, TapIO* out) {
  EBEN_REQUIRE(g_hi && wp && dx_hi, "null pointer in %s", who);
  EBEN_REQUIRE(seg >= 0 && (seg == 0 || (seg_map && c.B <= 4 * seg)), "bad batch segment map");
  EBEN_REQUIRE(fm_rows == 0 || (fm_sums && act_hi && act_lo && fm_rows > 0), "feature-matching rows need the sums and both planes of the embedding");
  TapIO io{};
  io.in_slope = 1.f; io.wp = wp; io.out_slope = 1.f; io.res_slope = 1.f;
  io.res_rows = fm_rows; io.fm_sums = fm_rows > 0 ? fm_sums : nullptr; io.fm_gs = fm_gs;
  io.emask_slope = mask_slope; io.em_seg = act_hi ? seg : 0;
  for (int i = 0; i < 4; ++i) io.em_map[i] = (seg > 0 && seg_map) ? seg_map[i] : i;
  io.xh = g_hi; io.yh = dx_hi; io.yl = dx_lo; io.eh = act_hi; io.el = act_lo; io.bl_ref_off = ref_row_offset;
  io.ec = fm_rows > 0 ? fm_codes : nullptr;
  *out = io;
  return EBEN_OK;
}
}  // namespace eben

extern "C" int eben_bl_conv1d_bwd_dx_pr(const EbenConv1dDesc* d, const void* g_hi, const float* wp_primed_fwd, const void* act_hi, const void* act_lo,
                                        float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset, const float* fm_sums,
                                        float fm_gs, void* dx_hi, void* dx_lo, void* stream) {
  return eben_bl_conv1d_bwd_dx_pr_c(d, g_hi, wp_primed_fwd, act_hi, act_lo, nullptr, mask_slope, seg, seg_map, fm_rows, ref_row_offset, fm_sums, fm_gs, dx_hi,
                                    dx_lo, stream);
}

extern "C" int eben_bl_conv1d_bwd_dx_pr_c(const EbenConv1dDesc* d, const void* g_hi, const float* wp_primed_fwd, const void* act_hi, const void* act_lo,
                                          const void* fm_codes, float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset,
                                          const float* fm_sums, float fm_gs, void* dx_hi, void* dx_lo, void* stream) {
  Canon c, q;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  const PrGeom g = d->transposed ? PrGeom{} : pr_geometry(c, &q);
  if (!g.ok) return fail(EBEN_EUNSUPPORTED, "eben_bl_conv1d_bwd_dx_pr: the layer's input gradient has no phases-as-rows form");
  TapIO io;
  if ((rc = bl_dx_io("eben_bl_conv1d_bwd_dx_pr", c, g_hi, wp_primed_fwd, act_hi, act_lo, fm_codes, mask_slope, seg, seg_map, fm_rows, ref_row_offset, fm_sums,
                     fm_gs, dx_hi, dx_lo, &io)))
    return rc;
  io.pr_S = g.S; io.pr_cbg = g.cbg; io.pr_Ly = c.Lin; io.pr_CBy = c.Cin / 8; io.pr_order = g.order;
  return tap3_launch(q, 0, io, 0, as_stream(stream));   // the primed layer's forward: pr_geometry vouched for it
}

extern "C" int eben_bl_conv1d_fwd(const EbenConv1dDesc* d, const void* x_hi, const void* x_lo, const float* wp_fwd, const float* bias,
                                  void* y_hi, void* y_lo, void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(c.bl && !d->transposed && d->in_slope == 1.f, "eben_bl_conv1d_fwd: a Conv1d descriptor with EBEN_LAYOUT_BL and no input activation");
  EBEN_REQUIRE(x_hi && wp_fwd && y_hi, "null pointer in eben_bl_conv1d_fwd");
  const ConvRoute r = conv_route(c, 0, 0);
  if (r.family != EBEN_CONV_ROUTE_TAP3) return fail(EBEN_EUNSUPPORTED, "eben_bl_conv1d_fwd: layer not covered by the bundle-layout tap-conv");
  TapIO io{};
  io.in_slope = 1.f; io.wp = wp_fwd; io.bias = bias; io.res_slope = 1.f; io.emask_slope = 1.f; io.out_slope = d->out_slope;
  io.xh = x_hi; io.xl = x_lo; io.yh = y_hi; io.yl = y_lo;
  return kConvFamilies[r.family].launch(c, r.dir, io, 0, as_stream(stream));   // the bundle-layout forward never asks the kernel to reflect
}

extern "C" int eben_bl_conv1d_bwd_dx(const EbenConv1dDesc* d, const void* g_hi, const float* wp_bwd, const void* act_hi, const void* act_lo,
                                     float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset, const float* fm_sums,
                                     float fm_gs, void* dx_hi, void* dx_lo, void* stream) {
  return eben_bl_conv1d_bwd_dx_c(d, g_hi, wp_bwd, act_hi, act_lo, nullptr, mask_slope, seg, seg_map, fm_rows, ref_row_offset, fm_sums, fm_gs, dx_hi, dx_lo,
                                 stream);
}

extern "C" int eben_bl_conv1d_bwd_dx_c(const EbenConv1dDesc* d, const void* g_hi, const float* wp_bwd, const void* act_hi, const void* act_lo,
                                       const void* fm_codes, float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset,
                                       const float* fm_sums, float fm_gs, void* dx_hi, void* dx_lo, void* stream) {
  Canon c;
  int rc = canon_from_desc(d, &c);
  if (rc) return rc;
  EBEN_REQUIRE(c.bl && !d->transposed, "eben_bl_conv1d_bwd_dx: a Conv1d descriptor with EBEN_LAYOUT_BL");
  TapIO io;
  if ((rc = bl_dx_io("eben_bl_conv1d_bwd_dx", c, g_hi, wp_bwd, act_hi, act_lo, fm_codes, mask_slope, seg, seg_map, fm_rows, ref_row_offset, fm_sums, fm_gs,
                     dx_hi, dx_lo, &io)))
    return rc;
  const ConvRoute r = conv_route(c, 0, 1);
  if (r.family != EBEN_CONV_ROUTE_TAP3) return fail(EBEN_EUNSUPPORTED, "eben_bl_conv1d_bwd_dx: layer not covered by the bundle-layout tap-conv");
  return kConvFamilies[r.family].launch(c, r.dir, io, r.reflect, as_stream(stream));
}
