/*
 * eben_hip.h -- C ABI of libeben_hip.so: the MI355X (gfx950) kernels of the EBEN
 * bandwidth-extension GAN train step (vibravox: EBENGenerator +
 * DiscriminatorEBENMultiScales forward/backward, PQMF, feature/hinge/MRSTFT losses, Adam).
 *
 * The reference has no native code: every "kernel" on its hot path is
 * an ATen call site inside a Python nn.Module.  Each entry point below therefore cites the
 * reference *call site* it replaces (file:line relative to the vibravox checkout); the
 * binding a maintainer adds on the reference side is a ctypes stub.
 *
 * Conventions
 *   - all tensors are contiguous float32 (batch, channel, time) device buffers; pointers are
 *     raw device pointers (tensor.data_ptr()); `stream` is a hipStream_t passed as void*.
 *   - every call is asynchronous on `stream`, re-entrant, allocates nothing and never
 *     synchronises; scratch comes from a caller-provided workspace.
 *   - return 0 on success, a negative EBEN_E* code on a bad argument, or a positive
 *     hipError_t from the launch.  eben_last_error() returns a thread-local message.
 *     Nothing throws across the ABI.
 */
#ifndef EBEN_HIP_H
#define EBEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(EBEN_BUILDING)
#define EBEN_API __attribute__((visibility("default")))
#else
#define EBEN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define EBEN_OK 0
#define EBEN_EINVAL (-1)      /* inconsistent descriptor / null pointer */
#define EBEN_EWORKSPACE (-2)  /* workspace too small */
#define EBEN_EUNSUPPORTED (-3)

#define EBEN_PAD_ZERO 0
#define EBEN_PAD_REFLECT 1

/* arithmetic of the contraction (storage, accumulation and the fused element-wise stages are fp32 either way) */
#define EBEN_MATH_F32 0   /* v_mfma_f32_*_f32 / fp32 FMA: bit-exact fp32 products */
#define EBEN_MATH_BF16 1  /* both MFMA operands rounded (RNE) to bf16 -- after the fused input stage (LeakyReLU or its
                           * derivative mask) -- fp32 accumulate; layers the bf16 kernels do not cover run their fp32 kernel */
#define EBEN_MATH_BF16X2 2 /* EBEN_MATH_BF16 with the ACTIVATION operand -- x of the layer's forward and of its weight gradient --
                           * entering as hi + lo, hi = bf16(x), lo = bf16(x - hi): two MFMAs per k-step against the same bf16
                           * weight / gradient fragment, x accurate to ~2^-17.  The discriminator's activations are a large
                           * input-independent component plus a small input-dependent one; rounding them to 8 bits buries the
                           * second, which is all that survives when the fake and real hinge gradients (eben.py:121-125) cancel.
                           * Gradient operands and weights stay single bf16; the input-gradient launch equals EBEN_MATH_BF16. */
#define EBEN_MATH_BF16X3 3 /* fused ResidualUnit launches (eben_ru_*_ex): both operands as hi + lo bf16, three MFMAs per product */
#define EBEN_MATH_BF16X6 4 /* ... as three bf16 pieces each, six MFMAs: every mantissa bit of the fp32 operands, fp32-grade products */
/* OR-ed into EbenConv1dDesc.math (EBEN_MATH_BF16 | EBEN_LAYOUT_BL, EBEN_MATH_BF16X3 | EBEN_LAYOUT_BL): the layer's activations and
 * gradients are at rest in the bf16 BUNDLE LAYOUT (see "bundle layout" below) and the layer is served by the eben_bl_* entry points;
 * the packed weight images come from eben_conv1d_pack / eben_conv1d_packed_floats on the same descriptor. */
#define EBEN_LAYOUT_BL 0x100

/* One Conv1d / ConvTranspose1d layer (nn.Conv1d / nn.ConvTranspose1d semantics).
 * Replaces the F.conv1d / F.conv_transpose1d call sites behind
 *   vibravox/torch_modules/dnn/eben_generator.py:112-166,241-249,272-280,295-312
 *   vibravox/torch_modules/dnn/eben_discriminator.py:66-157
 *   vibravox/torch_modules/dnn/melgan_discriminator.py:89-156
 * weight layout: Conv1d (Cout, Cin/groups, k); ConvTranspose1d (Cin, Cout/groups, k). */
typedef struct EbenConv1dDesc {
  int32_t batch;
  int32_t c_in, c_out;
  int32_t l_in, l_out;      /* l_out must equal the nn.Module's output length */
  int32_t ksize, stride, dilation, groups;
  int32_t pad_l, pad_r;     /* padding on the input (Conv1d) / `padding` of ConvTranspose1d in pad_l */
  int32_t pad_mode;         /* EBEN_PAD_ZERO | EBEN_PAD_REFLECT (Conv1d only) */
  int32_t transposed;       /* 0 Conv1d, 1 ConvTranspose1d */
  float in_slope;           /* LeakyReLU slope fused on the input load (1.0f = none) */
  float out_slope;          /* LeakyReLU slope fused on the output (1.0f = none) */
  int32_t math;             /* EBEN_MATH_F32 | EBEN_MATH_BF16 */
} EbenConv1dDesc;

EBEN_API const char* eben_last_error(void);
/* Bumped whenever a POD structure, an entry point's signature or a table stride changes (2: EbenWnBwdItem.col_perm_k; 3: eben_rubl_*; 4: eben_si_sdr / eben_stoi;
 * 5: eben_multirate_down* / eben_resample_adjoint).  eben_fir_plan was added without a bump: it changes none of those, and a binding
 * that needs it finds out by looking the symbol up.  The same holds for the data front end (eben_clip_powers*, eben_noisy_collate_scaled,
 * eben_biquad*, EbenClip): functions and a new POD type only.
 * eben_version() returns the value the library was built with; bindings compare it with the header they were written against. */
#define EBEN_ABI_VERSION 6
EBEN_API int eben_version(void);
/* fills name with the device's gcnArchName; returns compute-unit count (or negative) */
EBEN_API int eben_device_info(char* name, size_t name_bytes);

/* ---- weight-norm (torch_modules/utils.py:4-9 -> torch._weight_norm, dim=0) -------------- */
/* scale[r] = g[r]/||v[r,:]||, norm[r] = ||v[r,:]||  for r < rows */
EBEN_API int eben_wn_scale(const float* g, const float* v, int rows, int cols, float* scale, float* norm, void* stream);
/* dw given as `nslab` partial slabs of (rows, row_stride) floats (first `cols` of each row are
 * the weight gradient, column `cols` -- if has_bias -- the bias gradient).
 *   g != NULL: dg[r] = sum(dw*v)/norm, dv = (g/norm) dw - (g dg/norm^2) v     (weight-norm)
 *   g == NULL: dv = sum of slabs                                                (plain weight)
 * dbias (nullable) = summed bias column.  The slabs are scratch: slab 0 is overwritten by the sum. */
EBEN_API int eben_wn_bwd(const float* dw_slabs, int nslab, size_t slab_stride, int rows, int cols, int row_stride,
                const float* g, const float* v, const float* norm, float* dg, float* dv, float* dbias, void* stream);

/* Multi-tensor forms of the two calls above: one launch (per 36 items) for every layer of a network.  `items` is a HOST
 * array (device pointers inside), passed to the kernels by value.  Bit-identical results. */
typedef struct EbenWnScaleItem {
  const float* g; const float* v; float* scale; float* norm;
  int32_t rows, cols;
} EbenWnScaleItem;
typedef struct EbenWnBwdItem {
  const float* slabs;                 /* as dw_slabs of eben_wn_bwd: slab 0 is overwritten by the sum */
  const float* g; const float* v; const float* norm;   /* g == NULL: plain weight */
  float* dg; float* dv; float* dbias; /* dbias nullable */
  int64_t slab_stride;                /* floats between slabs */
  int32_t nslab, rows, cols, row_stride;
  int32_t col_perm_k, pad_;           /* k > 0: slab column of weight (c, j) = ((c / 8) k + j) 8 + c % 8, bias column = cols (eben_bl_conv1d_bwd_dw) */
} EbenWnBwdItem;
EBEN_API int eben_wn_scale_multi(const EbenWnScaleItem* items, int n, void* stream);
EBEN_API int eben_wn_bwd_multi(const EbenWnBwdItem* items, int n, void* stream);

/* ---- conv layers ------------------------------------------------------------------------ */
/* floats needed for the packed weights of the forward (which=0) / input-gradient (which=1) pass */
EBEN_API size_t eben_conv1d_packed_floats(const EbenConv1dDesc* d, int which);
/* Many layers' images in few launches (the step rebuilds ~150 images after its two optimiser steps): as eben_conv1d_pack per job
 * (wp_fwd / wp_bwd nullable); `jobs` is a HOST array. */
typedef struct EbenPackJob {
  EbenConv1dDesc desc;
  const float* v; const float* scale;
  float* wp_fwd; float* wp_bwd;
} EbenPackJob;
EBEN_API int eben_conv1d_pack_multi(const EbenPackJob* jobs, int n, void* stream);
/* The kernel family that serves the forward (which = 0) / input-gradient (which = 1) pass of this layer, asked of the host without
 * launching anything (the dispatch's own decision, which eben_conv1d_packed_floats, eben_conv1d_pack and every launch read too):
 * returns EBEN_CONV_ROUTE_*.  The packed layouts differ between routes; pack / fwd / bwd_dx agree by construction. */
#define EBEN_CONV_ROUTE_NONE 0   /* invalid descriptor, or a bundle-layout layer the bf16 tap-conv does not cover */
#define EBEN_CONV_ROUTE_TAP1 1   /* tapconv.hip: fp32 16x16x4 tiles, any shape */
#define EBEN_CONV_ROUTE_TAP2 2   /* tapconv2.hip: fp32 32x32x2 tiles, LDS-DMA weight stream; deep reductions */
#define EBEN_CONV_ROUTE_THIN 3   /* thinconv.hip: VALU, a handful of output channels per group */
#define EBEN_CONV_ROUTE_TAP3 4   /* tapconv3.hip: bf16 operands */
#define EBEN_CONV_ROUTE_GC 5     /* gen_conv.hip: forward only -- the generator's strided / transposed / latent convs under EBEN_MATH_BF16X6 /
                                    EBEN_MATH_BF16X3 (eben_generator.py:241-312) */
#define EBEN_CONV_ROUTE_TAP4 6   /* bigtap.hip: bundle layout only -- the long reductions of melgan_discriminator.py:119-145 /
                                    eben_discriminator.py:118-140 as persistent whole-panel blocks; TAP3's image and entry functions */
EBEN_API int eben_conv1d_kernel_generation(const EbenConv1dDesc* d, int which);
/* The kernel a launch on EBEN_CONV_ROUTE_TAP3 / _TAP4 / _GC runs, asked of the host without launching anything (the dispatch's own
 * decision, for tests).
 * which 0: eben_conv1d_fwd / eben_bl_conv1d_fwd; 1: the input gradient -- eben_conv1d_bwd_dx with mask_on_load = 1 (the fused output
 * activation differentiated as the gradient is staged: out_slope != 1), eben_conv1d_bwd_dx_ex / eben_bl_conv1d_bwd_dx with 0.
 * out[0..7] (n >= 8) = EBEN_CONV_ROUTE_*, then on TAP3 / TAP4: FM, XRB, IM, NPW, NPX, BL (tap3_kernel's template arguments; XRB = 0
 * off tap3_kernel), EBEN_VARIANT_*; on GC (which = 0): FORM, RT, CT, NP (gc_kernel's template arguments, read off the plan
 * the launch dispatches on), 0, 0, EBEN_VARIANT_GC; zeros past out[0] otherwise.  EBEN_EUNSUPPORTED where the launch itself would refuse. */
#define EBEN_VARIANT_TAP3 1      /* tap3_kernel (tapconv3.hip) */
#define EBEN_VARIANT_THIN_BL 2   /* thin_bl_kernel (thin_bl.hip) */
#define EBEN_VARIANT_TAP4 3      /* tap4_kernel (bigtap.hip) */
#define EBEN_VARIANT_GC 4        /* gc_kernel (gen_conv.hip) */
EBEN_API int eben_conv1d_variant(const EbenConv1dDesc* d, int which, int mask_on_load, int* out, int n);
/* The same question for the exact-fp32 families (for tests): the kernel instantiation a launch on EBEN_CONV_ROUTE_THIN / _TAP2 runs and
 * the plan decisions its rarely-taken branches hang on, read off the plan the launch dispatches on.  which / mask_on_load as above.
 * out[0..7] (n >= 8) = EBEN_CONV_ROUTE_*, then
 *   THIN: MT, BN, NP (thin_kernel's template arguments), id_fast (0: the block id is decomposed by division, the grid being too large
 *         for multiply-high), pg_n (stride phases whose geometry the host computed; 0: the kernel computes it, more than 8 phases),
 *         lds_bytes (dynamic LDS of the launch), 0;
 *   TAP2: FM, XR, H16, IMT (tap2_kernel's template arguments after NW = 4; IMT -1: the mask-on-load switch is a run-time one), ncc
 *         (channel chunks), nxbuf (input-tile buffers), and 1 where two buffers suffice only because the tiles change on weight-chunk
 *         boundaries (the aligned hand-over);
 *   zeros past out[0] on every other route (TAP1 has one kernel per launch form and no plan).
 * EBEN_EUNSUPPORTED / EBEN_EINVAL where the launch itself would refuse. */
EBEN_API int eben_conv1d_variant_f32(const EbenConv1dDesc* d, int which, int mask_on_load, int* out, int n);
/* pack v (optionally scaled per dim-0 row: weight-norm) into the MFMA-friendly layouts */
EBEN_API int eben_conv1d_pack(const EbenConv1dDesc* d, const float* v, const float* scale, float* wp_fwd, float* wp_bwd, void* stream);
/* y = lrelu_out( conv(lrelu_in(x)) + bias ) [+ residual] */
EBEN_API int eben_conv1d_fwd(const EbenConv1dDesc* d, const float* x, const float* wp_fwd, const float* bias,
                    const float* residual, float* y, void* stream);
/* ... + lrelu(residual, res_slope): the ResidualUnit's skip when its input is the previous block's output seen through
 * the shared LeakyReLU (eben_generator.py:187-189, 314-316: `x + nl(pointwise(dilated(x)))` with x = nl(previous)) */
EBEN_API int eben_conv1d_fwd_res(const EbenConv1dDesc* d, const float* x, const float* wp_fwd, const float* bias,
                        const float* residual, float res_slope, float* y, void* stream);
/* workspace bytes for bwd_dx (reflect padding only) and bwd_dw (partial slabs) */
EBEN_API size_t eben_conv1d_bwd_dx_workspace(const EbenConv1dDesc* d);
EBEN_API size_t eben_conv1d_bwd_dw_workspace(const EbenConv1dDesc* d, int* nslab, int* row_stride);
/* dx = conv^T( dy * lrelu_out'(y) ) * lrelu_in'(x).  y may be NULL when out_slope==1, x when in_slope==1.
 * accumulate!=0 adds into dx instead of overwriting. */
EBEN_API int eben_conv1d_bwd_dx(const EbenConv1dDesc* d, const float* dy, const float* y, const float* wp_bwd,
                       const float* x, float* dx, int accumulate, void* workspace, size_t ws_bytes, void* stream);
/* dx = ( conv^T( dy * lrelu_out'(y) ) + res_pre ) * lrelu_in'(x) + res_post  (either addend may be NULL; res_post only for
 * reflect-padded Conv1d layers, whose fold pass applies it): the gradient joins of the generator's ResidualUnit / skip
 * connections (eben_generator.py:251-254, 282-284, 314-316) without separate add kernels. */
EBEN_API int eben_conv1d_bwd_dx_res(const EbenConv1dDesc* d, const float* dy, const float* y, const float* wp_bwd, const float* x,
                           const float* res_pre, const float* res_post, float* dx, void* workspace, size_t ws_bytes, void* stream);
/* Batched input gradient for several right-hand sides that share one set of saved activations (rows of
 * g / dx = d->batch):  dx[b] = ( conv^T(g[b]) + (b < res_rows ? res[b] : 0) ) * lrelu'(mask[map(b)], mask_slope)
 * with map(b) = seg_map[b / seg] * seg + b % seg (seg = 0: map(b) = b; seg_map = HOST array of 4 ints).
 * g is used as is (the producer applied its own activation derivative); res / mask may be NULL.
 * Replaces the four separate backward passes through DiscriminatorEBENMultiScales that
 * vibravox/lightning_modules/eben.py:99-128,222-240 triggers (three through the enhanced branch, one
 * through the reference branch) with one pass over stacked gradients. */
EBEN_API int eben_conv1d_bwd_dx_ex(const EbenConv1dDesc* d, const float* g, const float* wp_bwd, const float* res, int res_rows,
                          const float* mask, float mask_slope, int seg, const int* seg_map, float* dx, void* stream);
/* The same launch with the feature-matching gradient of the embedding formed in the epilogue (feature_loss.py:40-47, the term
 * |a - b|.sum() / |a|.sum() of one (enhanced, reference) embedding pair) instead of read from a buffer eben_fm_bwd wrote:
 *   dx[b] = ( conv^T(g[b]) + (b < fm_rows ? fm_gs * (sgn(mask[b] - ref[b]) / s2 - s1 * sgn(mask[b]) / s2^2) : 0) )
 *           * lrelu'(mask[map(b)], mask_slope),      (s1, s2) = fm_sums[0..1] (device memory, written by eben_fm_sums)
 * ref = the reference rows of the embedding whose enhanced rows are mask rows 0 .. fm_rows-1.  Only the thin and the bf16 tap-conv
 * kernels (eben_conv1d_kernel_generation(d, 1) == EBEN_CONV_ROUTE_THIN or _TAP3) carry this epilogue; EBEN_EUNSUPPORTED otherwise. */
EBEN_API int eben_conv1d_bwd_dx_fm(const EbenConv1dDesc* d, const float* g, const float* wp_bwd, const float* ref, int fm_rows,
                          const float* fm_sums, float fm_gs, const float* mask, float mask_slope, int seg, const int* seg_map,
                          float* dx, void* stream);
/* partial weight (+bias) gradients into `slabs` (layout reported by bwd_dw_workspace);
 * finish with eben_wn_bwd. */
EBEN_API int eben_conv1d_bwd_dw(const EbenConv1dDesc* d, const float* dy, const float* y, const float* x, int has_bias,
                       float* slabs, size_t ws_bytes, void* stream);
/* The kernel family eben_conv1d_bwd_dw runs for the layer, asked of the host without launching anything (the dispatch's own decision,
 * which eben_conv1d_bwd_dw_workspace reads too; for tests).  out[0] (n >= 13) = EBEN_DW_ROUTE_*; on the conv_dw3 route out[1..12] =
 * FM, FN, WAVES_M, XRB, SP of conv_dw3_kernel, MT of dw3_pack_a_kernel, then the plan: BKT (time steps per chunk), nsplit (split-K
 * slabs), nchunks ((batch group, time chunk) pairs: block z owns chunks z, z + nsplit, ...), nnt / nmt (column / row tiles), nbg
 * (groups of 16 batch items).  Zeros past out[0] on the other routes. */
#define EBEN_DW_ROUTE_TINY 0       /* tiny_dw_kernel: at most 4 slab columns over a long row */
#define EBEN_DW_ROUTE_ONE_ROW 1    /* m1_dw_kernel: the c_out = 1 logits layers */
#define EBEN_DW_ROUTE_DW3 2        /* conv_dw3.hip: bf16 operands */
#define EBEN_DW_ROUTE_DW2 3        /* conv_dw2.hip: fp32, pre-transposed A image */
#define EBEN_DW_ROUTE_FALLBACK 4   /* conv_dw_kernel (conv_dw.hip) */
EBEN_API int eben_conv1d_bwd_dw_variant(const EbenConv1dDesc* d, int* out, int n);
/* The same question for the exact-fp32 routes, read off the decision their launches dispatch on (for tests).  out[0] (n >= 14) =
 * EBEN_DW_ROUTE_*; then, zero where a route has no such number:
 *   out[1..4]   FM, FN, WAVES_M, XR of conv_dw2_kernel (DW2; the pre-pass is dw_pack_a_kernel<FM, WAVES_M>)
 *   out[5..6]   bk (time steps per chunk: 128 / 64 / 32) of conv_dw_kernel<1, 8, 1, 2> and xfits (1: nch_max * span <= the register
 *               prefetch's capacity; 0: the X tile is staged directly) (FALLBACK)
 *   out[7]      nsplit: the slab count (TINY / ONE_ROW: one slab per batch item)
 *   out[8..12]  nchunks ((batch item, time chunk) pairs: block z owns chunks z, z + nsplit, ...), nnt / nmt (column / row tiles),
 *               nct (time chunks per row), nch_max (input channels per X tile) (DW2, FALLBACK)
 *   out[13]     the slab row stride (columns + 1)
 * On the conv_dw3 route out[0] alone: eben_conv1d_bwd_dw_variant is the authority there. */
EBEN_API int eben_conv1d_bwd_dw_f32_variant(const EbenConv1dDesc* d, int* out, int n);

/* ---- bf16 BUNDLE LAYOUT of the discriminator engine ------------------------------------------------------------------------
 * A (batch, channels, length) tensor, channels a multiple of 8, at rest as bf16 [batch][channels / 8][length][8]: one 16-byte UNIT =
 * 8 consecutive channels at one position = the unit the bf16 tap-conv stages into LDS (no conversion: the input tile is a copy) and
 * the unit the weight-gradient kernel transposes with ds_read_b64_tr_b16.  Two planes: hi = bf16(v) (round to nearest even) and lo =
 * bf16(v - hi) (optional; hi + lo carries 16 mantissa bits).  The batched discriminator passes that replace the autograd graph of
 * vibravox/torch_modules/dnn/eben_discriminator.py:27-51,66-163 and melgan_discriminator.py:89-169 keep every embedding and every
 * stacked gradient between the chain heads and the logits in this form when the plan's contractions are bf16 (BASELINE config 2):
 * the values the MFMA sees are the values it saw with fp32 tensors at rest (the same RNE of the same fp32 number, at the producer's
 * store instead of the consumer's load).  Descriptors carry EBEN_LAYOUT_BL in `math`. */
EBEN_API int eben_bl_from_f32(const float* x, int batch, int channels, int length, void* hi, void* lo /* nullable */, void* stream);
EBEN_API int eben_bl_to_f32(const void* hi, const void* lo /* nullable */, int batch, int channels, int length, float* x, void* stream);
/* y = lrelu(conv(x) + bias): x planes (x_lo required for EBEN_MATH_BF16X3: operands hi + lo, three MFMAs per product), y planes
 * (y_lo nullable).  wp_fwd from eben_conv1d_pack on the same descriptor.  EBEN_EUNSUPPORTED for layers outside the bf16 tap-conv. */
EBEN_API int eben_bl_conv1d_fwd(const EbenConv1dDesc* d, const void* x_hi, const void* x_lo, const float* wp_fwd, const float* bias,
                       void* y_hi, void* y_lo, void* stream);
/* Batched input gradient (cf. eben_conv1d_bwd_dx_fm):
 *   dx[b] = ( conv^T(g[b]) + (b < fm_rows ? fm_gs (sgn(a[b] - a[b + ref_row_offset]) / s2 - s1 sgn(a[b]) / s2^2) : 0) )
 *           * lrelu'(a_hi[map(b)], mask_slope),     a = act_hi + act_lo: the saved embedding at the layer's INPUT (2B rows),
 * map(b) = seg_map[b / seg] * seg + b % seg, (s1, s2) = fm_sums[0..1] on the device.  act_hi NULL: no mask, no feature matching. */
EBEN_API int eben_bl_conv1d_bwd_dx(const EbenConv1dDesc* d, const void* g_hi, const float* wp_bwd, const void* act_hi, const void* act_lo,
                          float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset, const float* fm_sums,
                          float fm_gs, void* dx_hi, void* dx_lo /* nullable */, void* stream);

/* "Phases as rows": the input gradient of a strided bundle-layout Conv1d (stride 4..8 at dilation 1; stride 2 up to dilation 2) as ONE
 * stride-1 Conv1d from the Cout channels of dy to stride x Cin rows, stored depth-to-space (csrc/conv1d.hip; MelGAN layers 1-4,
 * vibravox/torch_modules/dnn/melgan_discriminator.py:97-130, and the stride-2 layers of the PQMF-band discriminators,
 * eben_discriminator.py:86-130).  Rows are (phase, channel) or, at strides 4 and 2, (channel bundle, phase, channel in bundle): a 32-row
 * MFMA tile is then whole 16-byte units at consecutive positions, and mask, feature-matching operands and results move 32 contiguous
 * bytes per lane.  eben_bl_dx_pr_desc writes the descriptor of that primed layer (or returns
 * EBEN_EUNSUPPORTED); eben_bl_dx_pr_weights writes its weights (c_out' x c_in' / groups' x ksize' floats, weight-norm scale folded in), to be
 * packed as the primed layer's FORWARD image with eben_conv1d_pack(primed, w_primed, NULL, image, NULL); eben_bl_conv1d_bwd_dx_pr is
 * eben_bl_conv1d_bwd_dx on that image -- same operands, same epilogue, same results up to the order of the fp32 accumulation. */
EBEN_API int eben_bl_dx_pr_desc(const EbenConv1dDesc* d, EbenConv1dDesc* primed);
EBEN_API int eben_bl_dx_pr_weights(const EbenConv1dDesc* d, const float* v, const float* scale, float* w_primed, void* stream);
EBEN_API int eben_bl_conv1d_bwd_dx_pr(const EbenConv1dDesc* d, const void* g_hi, const float* wp_primed_fwd, const void* act_hi, const void* act_lo,
                                      float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset, const float* fm_sums,
                                      float fm_gs, void* dx_hi, void* dx_lo, void* stream);
/* eben_bl_conv1d_bwd_dx / eben_bl_conv1d_bwd_dx_pr with the feature-matching code plane of the embedding (eben_bl_fm_sums_codes; NULL: the
 * forms above): the rows with a feature-matching term read act_hi and the codes instead of act_hi, act_lo and both planes of the
 * reference rows.  Bit-identical results. */
EBEN_API int eben_bl_conv1d_bwd_dx_c(const EbenConv1dDesc* d, const void* g_hi, const float* wp_bwd, const void* act_hi, const void* act_lo,
                            const void* fm_codes, float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset,
                            const float* fm_sums, float fm_gs, void* dx_hi, void* dx_lo /* nullable */, void* stream);
EBEN_API int eben_bl_conv1d_bwd_dx_pr_c(const EbenConv1dDesc* d, const void* g_hi, const float* wp_primed_fwd, const void* act_hi, const void* act_lo,
                               const void* fm_codes, float mask_slope, int seg, const int* seg_map, int fm_rows, int ref_row_offset,
                               const float* fm_sums, float fm_gs, void* dx_hi, void* dx_lo /* nullable */, void* stream);
/* Weight (+ bias) gradient with both operands in the bundle layout (csrc/bl_dw.hip): the reduction runs along (batch, time) on
 * v_mfma_f32_32x32x16_bf16, both operand tiles arrive in LDS by buffer_load ... lds (descriptor bounds = the zero padding) and are
 * transposed on read -- no packing pre-pass, no conversion.  Slabs [nslab][c_out][row_stride] as eben_conv1d_bwd_dw's, except that
 * with *col_perm_k = k > 0 the column of weight (c, j) inside a row is ((c / 8) k + j) 8 + c % 8 (EbenWnBwdItem.col_perm_k). */
EBEN_API size_t eben_bl_conv1d_bwd_dw_workspace(const EbenConv1dDesc* d, int* nslab, int* row_stride, int* col_perm_k);
EBEN_API int eben_bl_conv1d_bwd_dw(const EbenConv1dDesc* d, const void* dy_hi, const void* x_hi, int has_bias, float* slabs, size_t ws_bytes,
                          void* stream);
/* n weight gradients in as few launches as their tile shapes allow (consecutive problems of one shape share a launch): the same layer
 * index of the three PQMF-band discriminators (vibravox/torch_modules/dnn/eben_discriminator.py:27-28 -- same channels and taps, their own
 * dilation, length, operands and slabs).  Problem i is exactly eben_bl_conv1d_bwd_dw(descs[i], dy_hi[i], x_hi[i], has_bias, slabs[i],
 * ws_bytes[i]): same slabs, bit for bit. */
EBEN_API int eben_bl_conv1d_bwd_dw_multi(const EbenConv1dDesc* const* descs, const void* const* dy_hi, const void* const* x_hi, int has_bias,
                                float* const* slabs, const size_t* ws_bytes, int n, void* stream);
/* The bl_dw kernel the layer's weight gradient runs (host only, the dispatch's own decision): out[0..4] (n >= 5) = FM, FN, XC, WN of
 * bl_dw_kernel<FM, FN, XC, WN>, and 1 when eben_bl_conv1d_bwd_dw_multi groups the problem (bl_dw_multi_kernel<FM, FN>) or 0 when it
 * launches it on its own.  EBEN_EUNSUPPORTED for layers outside the kernel. */
EBEN_API int eben_bl_conv1d_bwd_dw_variant(const EbenConv1dDesc* d, int* out, int n);
/* Chain heads: ReflectionPad1d(reflect_pad) + Conv1d(c_in -> c_out, ksize, dilation, groups = c_in, zero padding `pad`, stride 1)
 * + bias + LeakyReLU(out_slope), fp32 (batch, c_in, l_in) in, bundle planes out (eben_discriminator.py:66-76 layer 0,
 * melgan_discriminator.py:89-98 layer 0).  `jobs` is a HOST array of up to 4 heads run by ONE launch (the three PQMF-band chains
 * read the same bands): forward; input gradient dx (rows, c_in, l_in) = SUM over the jobs of conv^T(g) folded through the
 * reflection (y_hi / y_lo = the gradient planes at the heads' outputs, c_in <= 4); weight gradient of one head (slabs
 * [nslab][c_out][ksize + 1], column ksize = bias) from `rows` gradient rows y_hi and the `rows` input rows x paired with them. */
typedef struct EbenBlHeadJob {
  const float* x;                      /* (batch, c_in, l_in) */
  const float* v; const float* scale;  /* weight direction (c_out, 1, ksize), weight-norm scale g / ||v|| per row (nullable) */
  const float* bias;                   /* nullable */
  void* y_hi; void* y_lo;              /* (batch, c_out, l_out) planes; y_lo nullable */
  int32_t c_in, c_out, l_in, l_out, ksize, dilation, pad, reflect_pad;
  float out_slope; int32_t pad_;
} EbenBlHeadJob;
EBEN_API int eben_bl_head_fwd(const EbenBlHeadJob* jobs, int njobs, int batch, void* stream);
EBEN_API int eben_bl_head_dx(const EbenBlHeadJob* jobs, int njobs, int rows, float* dx, void* stream);
EBEN_API size_t eben_bl_head_dw_workspace(const EbenBlHeadJob* job, int rows, int* nslab, int* row_stride);
EBEN_API int eben_bl_head_dw(const EbenBlHeadJob* job, int rows, float* slabs, size_t ws_bytes, void* stream);
/* Chain tails: the logits layer Conv1d(channels -> 1, ksize <= 8, zero padding, stride 1) (eben_discriminator.py:150-157,
 * melgan_discriminator.py:147-156), v (1, channels, ksize), scale / bias one element (nullable): forward from bundle planes to fp32
 * (batch, 1, l_out); input gradient of `rows` stacked seeds (rows, 1, l_out) with the epilogue of eben_bl_conv1d_bwd_dx (act = the
 * layer's input embedding); weight gradient of `nbranch` hinge branches in one launch -- branch br pairs seed rows and input rows
 * [br rows, (br + 1) rows) of the given pointers -- into slabs [nbranch][nslab][channels ksize + 1] (last column = bias).  The built
 * head shapes are the two of DiscriminatorEBENMultiScales (4 -> 24 k 3, 1 -> 16 k 15): EBEN_EUNSUPPORTED otherwise.  All three tail entry
 * points require pad >= 0 and l_out = length + 2 pad - (ksize - 1) > 0 (EBEN_EINVAL). */
EBEN_API int eben_bl_tail_fwd(const void* x_hi, const void* x_lo, int batch, int channels, int length, int ksize, int pad, const float* v,
                     const float* scale, const float* bias, float out_slope, float* y, void* stream);
EBEN_API int eben_bl_tail_dx(const float* seeds, int rows, int channels, int length, int ksize, int pad, const float* v, const float* scale,
                    const void* act_hi, const void* act_lo, float mask_slope, int seg, const int* seg_map, int fm_rows,
                    int ref_row_offset, const float* fm_sums, float fm_gs, void* g_hi, void* g_lo /* nullable */, void* stream);
EBEN_API size_t eben_bl_tail_dw_workspace(int rows, int channels, int l_out, int ksize, int nbranch, int* nslab, int* row_stride);
EBEN_API int eben_bl_tail_dw(const float* seeds, const void* x_hi, const void* x_lo, int rows, int nbranch, int channels, int length, int ksize, int pad,
                    float* slabs, size_t ws_bytes, void* stream);
/* feature-matching sums (eben_fm_sums) over embeddings in bundle planes: planes = HOST array (hi_0, lo_0, hi_1, lo_1, ...), the
 * enhanced rows are the first units[i] units of pair i's planes and the reference rows the next units[i] (a = hi + lo).  Both planes of
 * every pair are required: a NULL hi or lo plane is EBEN_EINVAL before any launch. */
EBEN_API size_t eben_bl_fm_sums_workspace(int npairs);
EBEN_API int eben_bl_fm_sums(const void* const* planes, const int64_t* units, int npairs, float* partial_ws, size_t ws_bytes, float* sums,
                    void* stream);
/* eben_bl_fm_sums that also writes, for pairs whose codes[p] is not NULL, one byte per element of the pair's enhanced rows:
 * bits 0-1 = sgn(a - r) + 1, bits 2-3 = sgn(a) + 1 (8 bytes per unit, at the unit's index in the hi plane) -- what the feature-matching
 * term of the stacked input gradients needs of the pair (eben_bl_conv1d_bwd_dx_c: one 4-byte load per row quad in place of three
 * 8-byte operand loads).  Same sums. */
EBEN_API int eben_bl_fm_sums_codes(const void* const* planes, const int64_t* units, void* const* codes, int npairs, float* partial_ws,
                                   size_t ws_bytes, float* sums, void* stream);

/* ---- fused ResidualUnit forward (vibravox/torch_modules/dnn/eben_generator.py:287-316) ---------------------------------
 *   y = xin + lrelu( W_pw . ( W_dil (*) xin ), out_slope ),  xin = lrelu(x, in_slope)
 * W_dil (C, C, 3) dilation d with "same" reflect padding, W_pw (C, C, 1), C in {32, 64, 128}, no bias; x, y (batch, C, length).
 * One launch instead of dilated conv + pointwise conv + add: x is read once.  h (nullable) receives W_dil (*) xin and u
 * (nullable) lrelu(z) -- what the backward needs (the pointwise weight gradient, the activation mask).  eben_ru_pack writes
 * the weight image both stages stream (eben_ru_packed_floats(C) floats) from the directions v and the weight-norm scales
 * g/||v|| (eben_wn_scale; NULL = plain weights). */
EBEN_API size_t eben_ru_packed_floats(int channels);
EBEN_API int eben_ru_pack(int channels, const float* v_dil, const float* scale_dil, const float* v_pw, const float* scale_pw, float* wimg,
                 void* stream);
EBEN_API int eben_ru_fwd(int batch, int channels, int length, int dilation, const float* x, float in_slope, float out_slope,
                const float* wimg, float* y, float* h, float* u, void* stream);
/* Input-gradient chain of the same unit in one launch (the reflect padding folds onto the end positions inside the kernel):
 *   g_h = W_pw^T ( g_y * lrelu'(u, out_slope) ),   g_x = ( g_y + fold(W_dil^T (*) g_h) ) * lrelu'(x, in_slope) + post
 * u: the forward's lrelu(z); x: the unit's input (needed when in_slope != 1), post: nullable addend behind the mask (a skip
 * connection's gradient); g_h is written out for the dilated conv's weight gradient.  eben_ru_pack_bwd writes the transposed
 * weight image (eben_ru_packed_floats(C) floats). */
EBEN_API int eben_ru_pack_bwd(int channels, const float* v_dil, const float* scale_dil, const float* v_pw, const float* scale_pw,
                     float* wimg_bwd, void* stream);
EBEN_API int eben_ru_bwd(int batch, int channels, int length, int dilation, const float* gy, const float* u, float out_slope,
                const float* x, float in_slope, const float* post, const float* wimg_bwd, float* gx, float* gh, void* stream);

/* The same two launches on the bf16 matrix pipe with SPLIT operands (csrc/ru_split.hip): every fp32 operand enters as a sum of
 * bf16 pieces and a product is the sum of the piece products that matter.  math:
 *   EBEN_MATH_F32     the exact-fp32 MFMA kernels above;
 *   EBEN_MATH_BF16X6  three pieces per operand, six products: all 24 mantissa bits, dropped terms <= 2^-26 -- fp32 arithmetic at
 *                     6/16 of the fp32 MFMA cost (the generator forward's mode);
 *   EBEN_MATH_BF16X3  two pieces, three products, ~2^-17 per product;   EBEN_MATH_BF16  plain bf16 operands.
 * which: 0 forward image, 1 backward (transposed) image; eben_ru_packed_floats_ex(C, math) floats each.  Dilation <= 9. */
EBEN_API size_t eben_ru_packed_floats_ex(int channels, int math);
EBEN_API int eben_ru_supported(int channels, int dilation, int math);
EBEN_API int eben_ru_pack_ex(int channels, int math, int which, const float* v_dil, const float* scale_dil, const float* v_pw,
                    const float* scale_pw, float* wimg, void* stream);
typedef struct EbenRuPackJob {   /* one image of eben_ru_pack_ex (math != EBEN_MATH_F32); `jobs` is a HOST array */
  int32_t channels, math, which, pad_;
  const float* v_dil; const float* scale_dil; const float* v_pw; const float* scale_pw; float* wimg;
} EbenRuPackJob;
EBEN_API int eben_ru_pack_multi(const EbenRuPackJob* jobs, int n, void* stream);
EBEN_API int eben_ru_fwd_ex(int math, int batch, int channels, int length, int dilation, const float* x, float in_slope, float out_slope,
                   const float* wimg, float* y, float* h, float* u, void* stream);
EBEN_API int eben_ru_bwd_ex(int math, int batch, int channels, int length, int dilation, const float* gy, const float* u, float out_slope,
                   const float* x, float in_slope, const float* post, const float* wimg_bwd, float* gx, float* gh, void* stream);

/* Both weight gradients of the unit in one launch (csrc/ru_dw.hip): split-K slabs [eben_ru_dw_slabs(batch, C, length)][C][C] for the
 * pointwise conv and [..][C][3 C] for the dilated one (row strides C and 3 C), to be summed by eben_wn_bwd / eben_wn_bwd_multi:
 *   dW_pw[m][c] = sum g_z[m] h[c],  g_z = g_y * lrelu'(u, out_slope);   dW_dil[m][c][j] = sum g_h[m] xin[c](. + (j - 1) d, reflected)
 * The reduction runs along time, so the operands are read straight from the (batch, channel, time) tensors (no packing pass).
 * math: EBEN_MATH_BF16 (single bf16 operands) or EBEN_MATH_BF16X6 (three pieces per operand: fp32-grade). */
EBEN_API int eben_ru_dw_slabs(int batch, int channels, int length);
EBEN_API int eben_ru_dw(int math, int batch, int channels, int length, int dilation, const float* gy, const float* u, float out_slope,
               const float* h, const float* gh, const float* x, float in_slope, float* slabs_pw, float* slabs_dil, void* stream);

/* ResidualUnit with what the backward needs AT REST AS bf16 BUNDLES (csrc/ru_bl.hip; the bf16 generator backward of
 * vibravox/torch_modules/dnn/eben_generator.py:287-316).  Bundle plane of a (batch, C, L) tensor: bf16 [batch][C / 8][L][8] (2 batch C L
 * bytes); sign plane: [batch][C / 8][L] bytes, bit e = (value of channel 8 g + e > 0).
 *   eben_rubl_fwd  = eben_ru_fwd_ex (math EBEN_MATH_BF16X6) that writes y (fp32) and, instead of h / u in fp32: xb = bf16(lrelu(x)),
 *                    hb = bf16(h) as bundle planes and umask = the sign plane of u.
 *   eben_rubl_bwd  = eben_ru_bwd_ex (math EBEN_MATH_BF16; wimg_bwd = the EBEN_MATH_BF16 image of eben_ru_pack_ex(which = 1)): g_y fp32 in,
 *                    g_x fp32 out; gzb = bf16(g_y lrelu'(u)) and ghb = bf16(g_h) leave as bundle planes (operands of eben_rubl_dw only).
 *   eben_rubl_dw   = eben_ru_dw on the four bundle planes: slabs [eben_rubl_dw_slabs(batch, C, L)][C][C] and [..][C][3 C] in
 *                    eben_ru_dw's layout. */
EBEN_API int eben_rubl_supported(int channels, int dilation);
EBEN_API int eben_rubl_fwd(int math, int batch, int channels, int length, int dilation, const float* x, float in_slope, float out_slope,
                           const float* wimg, float* y, void* xb, void* hb, void* umask, void* stream);
EBEN_API int eben_rubl_bwd(int batch, int channels, int length, int dilation, const float* gy, const void* umask, float out_slope, const float* x,
                           float in_slope, const float* post, const float* wimg_bwd, float* gx, void* gzb, void* ghb, void* stream);
EBEN_API int eben_rubl_dw_slabs(int batch, int channels, int length);
EBEN_API int eben_rubl_dw(int batch, int channels, int length, int dilation, const void* gzb, const void* hb, const void* ghb, const void* xb,
                          float* slabs_pw, float* slabs_dil, void* stream);
/* The kernel instantiation and the launch geometry of a ResidualUnit launch, asked of the host without launching anything (for tests):
 * the decision the launcher itself dispatches on, the values of its static knobs included (EBEN_RU3_W128; EBEN_RUBL_NW32 / _NW64 / _G128 /
 * _RT64 / _RT128 / _BKT128 / _SEG32 / _SEG64 / _SEG128; EBEN_RUDW_UNROLL / _SEG -- each read once per process).
 * op: EBEN_RU_OP_*; math as the entry point takes it (ignored by the three entry points that take none).
 * out[0 .. EBEN_RU_VARIANT_N - 1] (n >= EBEN_RU_VARIANT_N, else EBEN_EINVAL):
 *   [0]      EBEN_RU_FAMILY_*
 *   [1..5]   the template arguments, 0 past the last: F32 <CT>; SPLIT forward <CT, NW, NP, KSC, BL>, input gradient <CT, NW, NP, G>;
 *            BL_BWD <CT, NW, G>; RU_DW <CT, NP, UN>; RUBL_DW <CT, RT, BKT>
 *   [6]      positions per block (forwards 128 or 64; input gradients BO = 32 NW - 2 dilation; weight gradients the slab length)
 *   [7]      tiles per item (weight gradients: slabs per item)       [8]  blocks of the grid       [9]  dynamic LDS bytes
 *   [10..12] weight gradients: slab length, slabs per item, slabs in all (= eben_ru_dw_slabs / eben_rubl_dw_slabs); 0 otherwise
 * Returns the code of the launch for what the launch refuses (channels, dilation, length <= dilation, a math mode the op lacks). */
#define EBEN_RU_OP_FWD 0      /* eben_ru_fwd_ex */
#define EBEN_RU_OP_BL_FWD 1   /* eben_rubl_fwd */
#define EBEN_RU_OP_BWD 2      /* eben_ru_bwd_ex */
#define EBEN_RU_OP_BL_BWD 3   /* eben_rubl_bwd */
#define EBEN_RU_OP_DW 4       /* eben_ru_dw */
#define EBEN_RU_OP_BL_DW 5    /* eben_rubl_dw */
#define EBEN_RU_FAMILY_F32 1      /* ru_fwd_kernel / ru_bwd_kernel (exact_fp32/ru_fused.hip) */
#define EBEN_RU_FAMILY_SPLIT 2    /* ru3_fwd_kernel / ru3_bwd_kernel (ru_split.hip) */
#define EBEN_RU_FAMILY_BL_BWD 3   /* rubl_bwd_kernel (ru_bl.hip) */
#define EBEN_RU_FAMILY_RU_DW 4    /* ru_dw_kernel (ru_dw.hip) */
#define EBEN_RU_FAMILY_RUBL_DW 5  /* rubl_dw_kernel (ru_bl.hip) */
#define EBEN_RU_VARIANT_N 13
EBEN_API int eben_ru_variant(int op, int math, int batch, int channels, int length, int dilation, int* out, int n);

/* ---- PQMF / FIR banks (vibravox/torch_modules/dsp/pqmf.py:17-232, eben_generator.py:209-211; auraloss FIRFilter) ---------- */
/* Exact fp32 products, fp32 accumulation in a fixed order (bitwise reproducible), any off0 (floor division for negative offsets),
 * any lengths, 64-bit row offsets.  Domain: every bank of 1 <= bands <= 64, 1 <= ntaps <= 4096, 1 <= stride <= 64 -- the class
 * defaults of PseudoQMFBanks (32 bands x 1024 taps) included -- plus the small banks of up to 1024 weights in all that the
 * whole-bank-in-LDS kernels take at other band counts / strides.  Four kernels serve it (eben_fir_plan tells which):
 *   1  the M = 4, N = 32 PQMF banks of every EBEN configuration (1, 2 or 4 bands, stride 4): polyphase form on wave shuffles;
 *   2  one band, stride 1, >= 4 taps (the A-weighting prefilter): register-window FIR;
 *   3  any other bank of <= 1024 weights whose tile fits 64 KB of LDS beside the whole bank;
 *   4  everything else inside the domain: tap-tiled kernels (fir_bank.hip) that stage the input span of 128 output positions once
 *      and stream the bank through LDS in chunks of 64 taps onto v_mfma_f32_32x32x2_f32.
 * Outside the domain: EBEN_EUNSUPPORTED with a message, nothing launched. */
/* decimating FIR bank: y[b,k,t] = sum_j w[k*ntaps+j] * x[b,0,t*stride+off0+j], zero outside [0,lx) */
EBEN_API int eben_fir_decimate(const float* x, const float* w, float* y, int batch, int lx, int ly, int bands, int ntaps,
                      int stride, int off0, void* stream);
/* interpolating FIR bank summed over bands (adjoint of the above):
 *   x[b,0,u] = sum_k sum_{t,j : t*stride+off0+j == u} w[k*ntaps+j] * y[b,k,t], zero outside [0,ly) */
EBEN_API int eben_fir_interp_sum(const float* y, const float* w, float* x, int batch, int lx, int ly, int bands, int ntaps,
                        int stride, int off0, void* stream);
/* The kernel a launch of eben_fir_decimate (which = 0) / eben_fir_interp_sum (which = 1) runs, asked of the host without launching
 * anything (the dispatch's own decision).  out[0..3] (n >= 4) = kernel (1 .. 4 above), output positions per block, taps (reduction
 * steps) per LDS chunk (0 off kernel 4), bands per block (kernel 4, which = 1: bands whose input tile is staged at a time; the block
 * sums them all).  EBEN_EUNSUPPORTED where the launch itself would refuse. */
EBEN_API int eben_fir_plan(int bands, int ntaps, int stride, int which, int* out, int n);

/* ---- elementwise ------------------------------------------------------------------------ */
EBEN_API int eben_lrelu_fwd(const float* x, float* y, size_t n, float slope, void* stream);
EBEN_API int eben_lrelu_bwd(const float* dy, const float* x_or_y, float* dx, size_t n, float slope, void* stream);
/* Grouped GEMM y[g] = W[g] (m x k) * x[g] (k x n), row-major with the n columns contiguous, fp32 in / out, products of split bf16
 * operands on the bf16 MFMA (math: EBEN_MATH_BF16, EBEN_MATH_BF16X3 = hi + lo operands / three products, EBEN_MATH_BF16X6 = three
 * pieces / six products, fp32-grade).  The windowed-DFT contractions of auraloss' STFT (torch.stft inside
 * auraloss.freq.STFTLoss.stft, configs/lightning_module/loss_module/multi_stft.yaml:1-18) and their transposes in the backward:
 * groups = 2 is the folded even / odd form.  w is packed once per basis (eben_gemm_pack -> eben_gemm_packed_floats floats). */
EBEN_API size_t eben_gemm_packed_floats(int math, int groups, int m, int k);
EBEN_API int eben_gemm_pack(int math, int groups, int m, int k, const float* w, float* wp, void* stream);
EBEN_API int eben_gemm_fwd(int math, int groups, int m, int k, long long n, const float* x, const float* wp, float* y, void* stream);
/* Space to depth along time: out[row][r][q] = xp[row][S*q + r + off] (r < S, q < Lq; xp = x continued by reflection or by zeros
 * beyond [0, L)), optionally times lrelu'(mask[row][.], mask_slope).  out: (rows, S, Lq).  Turns a stride-S Conv1d with
 * ksize = kq*S (EncBlock.conv, eben_generator.py:251-254) -- or the input gradient of the matching ConvTranspose1d (DecBlock,
 * eben_generator.py:282-284) -- into a stride-1 conv with kq taps over C*S channels, with the weights viewed as
 * (M, C, kq, S) -> (M, C, S, kq). */
EBEN_API int eben_space_to_depth(const float* x, const float* mask, float mask_slope, float* out, int rows, int L, int S, int off, int Lq,
                        int reflect, void* stream);
EBEN_API int eben_add(const float* a, const float* b, float* out, size_t n, void* stream);
EBEN_API int eben_axpby(const float* a, float alpha, const float* b, float beta, float* out, size_t n, void* stream);
/* bands = tanh(x + lift) where lift has `c_lift` leading channels (eben_generator.py:203-208) */
EBEN_API int eben_tanh_lift_fwd(const float* x, const float* lift, float* out, int batch, int channels, int c_lift, int length, void* stream);
EBEN_API int eben_tanh_bwd(const float* dout, const float* out, float* dx, size_t n, void* stream);
/* nn.ReflectionPad1d (eben_discriminator.py:69, melgan_discriminator.py:92) and its adjoint */
EBEN_API int eben_reflect_pad_fwd(const float* x, float* y, int rows, int lx, int pad_l, int pad_r, void* stream);
EBEN_API int eben_reflect_pad_bwd(const float* dy, float* dx, int rows, int lx, int pad_l, int pad_r, void* stream);

/* ---- losses ----------------------------------------------------------------------------- */
/* feature matching (vibravox/torch_modules/losses/feature_loss.py:37-50): per pair i
 * sums[2i] = sum|a-b|, sums[2i+1] = sum|a| (device floats).  ptrs = HOST array of 2*npairs device
 * pointers (a0,b0,a1,b1,...), numel = HOST array of npairs element counts; they travel to the
 * kernels by value in the kernel-argument segment (no device table, no copy). */
EBEN_API int eben_fm_sums(const void* const* ptrs, const int64_t* numel, int npairs, float* partial_ws, size_t ws_bytes,
                 float* sums, void* stream);
EBEN_API size_t eben_fm_sums_workspace(int npairs);
/* da_i = gout * inv_count * ( sign(a-b)/S2 - S1*sign(a)/S2^2 ); gout is a device scalar */
EBEN_API int eben_fm_bwd(const void* const* ptrs, void* const* da_ptrs, const int64_t* numel, int npairs, const float* sums,
                const float* gout, float inv_count, void* stream);
/* hinge (losses/hinge_loss.py:35-43): out[i] = mean(relu(1 - target*x_i)) ; bwd adds nothing else */
EBEN_API int eben_hinge_fwd(const float* x, size_t n, float target, float* out, void* stream);
/* Dynamic loss balancing of the generator step (vibravox/lightning_modules/eben.py:222-240), the scalar part in one launch:
 * old[i] = init ? *norms[i] : old[i];  if (ema) old[i] = beta * old[i] + one_minus_beta * *norms[i];
 * lambdas[i] = clamp(1 / (old[i] + 1e-4), 0, 1e4);  backprop[0] = sum_i *losses[i] * lambdas[i]   (torch's operation order and
 * roundings; norms / losses: n <= 8 device scalars), and the lambda-weighted sum of n tensors out = sum_i weights[i] * tensors[i]
 * (weights on the device) that seeds the generator backward. */
/* The norms ||dL_i / d(last_conv.weight)|| of the dynamic loss balancing (vibravox/lightning_modules/eben.py:222-229) for n <= 4 losses in
 * one pass, from the seeds s_i = dL_i / d(bands): dW_i = sum s_i (1 - bands^2) (*) reflect_pad(pre), bands = tanh(last_conv(pre) + lift)
 * (eben_generator.py:159-166, 203-208; built for that layer: 32 -> 4, k 3, reflect padding 1).  seeds: HOST array of n device pointers to
 * (batch, 4, length) tensors; norms: n floats on the device; workspace: eben_last_conv_norms_workspace(batch) bytes.  Fixed-order sums. */
EBEN_API size_t eben_last_conv_norms_workspace(int batch);
EBEN_API int eben_last_conv_norms(const void* const* seeds, int n, const float* bands, const float* pre, int batch, int c_in, int c_out, int length,
                                  int ksize, int pad, float* workspace, size_t ws_bytes, float* norms, void* stream);
EBEN_API int eben_balance(const void* const* norms, const void* const* losses, int n, float* old, int init, int ema, float beta,
                 float one_minus_beta, float* lambdas, float* backprop, void* stream);
EBEN_API int eben_weighted_sum(const void* const* tensors, const float* weights, int n, size_t numel, float* out, void* stream);
/* The four discriminator-side loss values of a step from their partial results, one launch: out[0] = inv_count * sum_p s1_p / s2_p
 * (feature_loss.py:37-50, (s1, s2) pairs of eben_fm_sums), out[1 + k] = mean over the sub-discriminators of hinge[3 i + k]
 * (eben.py:99-128: generator-side adversarial, fake, real). */
EBEN_API int eben_disc_losses(const float* fm_sums, int npairs, float inv_count, const float* hinge, int nchains, float* out, void* stream);
/* The MRSTFT loss value from the per-row sums of eben_stft_loss_sums_ex of n <= 8 resolutions (auraloss MultiResolutionSTFTLoss:
 * mean over resolutions of  mean_r sqrt(s0 / s1) + sum_r s2 * inv_counts[i],  inv_counts[i] = 1 / (rows bins_i frames_i)). */
EBEN_API int eben_stft_loss_total(const void* const* sums, const float* inv_counts, int n, int rows, float* out, void* stream);
/* n <= 32 hinge terms in one launch: out[i] = mean(max(0, 1 - targets[i] * xs[i][.])) (the 3 targets x 4 sub-discriminators of one
 * step, eben.py:99-128 through hinge_loss.py:35-43); the single-term kernel's summation order. */
EBEN_API int eben_hinge_fwd_multi(const void* const* xs, const int64_t* numel, const float* targets, int n, float* out, void* stream);
EBEN_API int eben_hinge_bwd(const float* x, size_t n, float target, const float* gout, float scale, float* dx, void* stream);
/* The stacked seeds of the batched discriminator backward (hinge_loss.py:38-43 differentiated three times; rows [fm | adv | fake | real],
 * `per` logits each): seeds[0 .. per) = 0, seeds[per ..) = d hinge(enhanced, +1), [2 per ..) = d hinge(enhanced, -1), [3 per ..) =
 * d hinge(reference, +1), each times gout[0] * scale_x / per -- eben_hinge_bwd's arithmetic, one launch. */
EBEN_API int eben_hinge_bwd_stacked(const float* enhanced_logits, const float* reference_logits, size_t per, const float* gout, float scale_adv,
                                    float scale_fake, float scale_real, float* seeds, void* stream);
/* STFT magnitude losses (auraloss.freq.STFTLoss as configured by multi_stft.yaml; call site
 * vibravox/lightning_modules/eben.py:195-198), |.| = sqrt(clamp(re^2+im^2, eps)):
 * eben_stft_loss_sums_ex, per row r: out[3r] = sum (|Y|-|X|)^2, out[3r+1] = sum |Y|^2, out[3r+2] = sum |log|X| - log|Y||;
 * eben_stft_loss_bwd_ex: dspec_x from d(loss) with loss = mean_rows(sqrt(s0/s1)) + mean(|log X - log Y|); gout device scalar * scale.
 * eben_overlap_add_ex: adjoint of framing a (reflect-)padded signal: x[b,u] (+)= fold( sum_f buf[b, u+pad-f*hop, f] ).  Used by the
 * STFT backward: d(frames) = basis^T . d(spec) is a dense pointwise conv (eben_conv1d_fwd, ksize 1), this kernel scatters it back
 * onto the waveform. */
EBEN_API size_t eben_stft_loss_sums_workspace(int rows);

/* All three take explicit strides -- element (row r, bin k, frame f) of a spectrum at r*row_stride + k*bin_stride + f
 * (imaginary part at + im_off), frame-buffer element (item b, window sample j, frame f) at b*row_stride + j*j_stride + f --
 * so that the windowed DFT of ALL items runs as one dense GEMM over a flat (channels, rows*frames) matrix:
 *   eben_stft_frames: out[j, r*frames + f] = sig[r, reflect(f*hop + j - pad)]   (torch.stft(center=True, pad_mode="reflect") framing)
 *   spec (2*bins, R*frames) = basis (2*bins, win) . frames (win, R*frames)        (eben_conv1d_fwd, ksize 1, batch 1) */
EBEN_API int eben_stft_frames(const float* sig, float* out, int rows, int t, int win, int hop, int pad, int frames, void* stream);
/* Folded framing for a window symmetric about frame sample win/2 (hann): out holds TWO GROUPS of nsub*win/2 rows, the even
 * part E[m] = s[h+m] + s[h-m] (E[0] = s[h]) and the odd part O[m] = s[h+m] - s[h-m] (O[0] = 0) of each frame about h = win/2, so
 * that Re X = basis[:bins, h:] . E and Im X = basis[bins:, h:] . O is a 2-group pointwise conv with half the products of the
 * dense one (auraloss STFTLoss.stft = torch.stft(center=True, hann) as called from eben.py:195-198).  split = 1: nsub = 3, each
 * group written as [hi ; lo ; hi] (hi = bf16(v), lo = bf16(v - hi)) for a bf16-operand contraction against [W_hi ; W_hi ; W_lo]
 * ("bf16x3", ~2^-17 relative); split = 0: nsub = 1, exact fp32.  eben_split3 does the same to the rows of a gradient matrix
 * (groups * R, cols) -> (groups * 3R, cols); eben_overlap_add_folded is the adjoint of the folded framing: buf rows [dE ; dO]. */
EBEN_API int eben_stft_frames_folded(const float* sig, float* out, int rows, int t, int win, int hop, int pad, int frames, int split,
                            void* stream);
EBEN_API int eben_split3(const float* in, float* out, int groups, int rows_per_group, long long cols, void* stream);
/* 1 if eben_overlap_add_folded takes its LDS-tile launch at this geometry (EBEN_OLA_TILED=0 at process start: never), else 0. */
EBEN_API int eben_overlap_add_folded_tiled(int lx, int win, int hop, int pad);
EBEN_API int eben_overlap_add_folded(const float* frames_buf, float* x, int batch, int lx, int win, int frames, int hop, int pad,
                            int accumulate, long long row_stride, long long j_stride, void* stream);
EBEN_API int eben_stft_loss_sums_ex(const float* spec_x, const float* spec_y, int rows, int bins, int frames, long long row_stride,
                           long long bin_stride, long long im_off, float eps, float* partial_ws, size_t ws_bytes, float* out,
                           void* stream);
EBEN_API int eben_stft_loss_bwd_ex(const float* spec_x, const float* spec_y, int rows, int bins, int frames, long long row_stride,
                          long long bin_stride, long long im_off, float eps, const float* sums, const float* gout, float scale,
                          float* dspec_x, long long out_row_stride, long long out_bin_stride, long long out_im_off, void* stream);
EBEN_API int eben_overlap_add_ex(const float* frames_buf, float* x, int batch, int lx, int win, int frames, int hop, int pad,
                        int reflect, int accumulate, long long row_stride, long long j_stride, void* stream);

/* The magnitude terms of auraloss STFTLoss outside multi_stft.yaml's configuration (stft_terms.hip): an optional mel projection
 * (scale="mel") and the weighted SC / log-magnitude / linear-magnitude terms under an L1 or L2 distance.  spec is the flat
 * (2*bins, 2*rows*frames) windowed-DFT output (bin k of column c at k*cols + c, imaginary at + bins*cols; x rows in columns
 * [0, rows*frames), y rows after them); M = sqrt(clamp(re^2 + im^2, eps)).  terms: mask of 1 (SC), 2 (log), 4 (lin); l2 = 0: |.|,
 * 1: (.)^2.  Mel projection M'[m] = sum_j fb_w[j] M[fb_lo[m] + j - fb_off[m]], j in [fb_off[m], fb_off[m+1]), for m < n_out;
 * fb_lo = NULL: no projection, n_out = bins.
 *   eben_stft_terms_fwd: sums[4r .. 4r+3] = sum (M'y - M'x)^2, sum M'y^2, sum dist(log M'x, log M'y), sum dist(M'x, M'y) per row
 *     (terms not in the mask left 0); with the projection, mags receives M'x then M'y as (2, rows, n_out, frames).
 *   eben_stft_terms_bwd: dspec (2*bins, rows*frames) = d loss / d spec_x, loss = sum of the weighted terms (SC: mean over rows;
 *     log / lin: over rows * n_out * frames), times gout[0] * scale; the adjoint projection through each bin's <= 2 (filter, weight)
 *     pairs bin_m[2k + q] (-1: none), bin_w[2k + q]; zero where re^2 + im^2 < eps.
 *   eben_stft_terms_total: out = mean over the n <= 16 resolutions of w_sc mean_r sqrt(s0 / s1) + w_log sum_r s2 * inv_counts[i]
 *     + w_lin sum_r s3 * inv_counts[i]  (inv_counts[i] = 1 / (rows n_out_i frames_i); terms outside the mask are not read). */
EBEN_API size_t eben_stft_terms_workspace(int rows);
EBEN_API int eben_stft_terms_fwd(const float* spec, int rows, int bins, int frames, float eps, int n_out, const int* fb_lo, const int* fb_off,
                                 const float* fb_w, int terms, int l2, float* mags, float* partial_ws, size_t ws_bytes, float* sums,
                                 void* stream);
EBEN_API int eben_stft_terms_bwd(const float* spec, int rows, int bins, int frames, float eps, int n_out, const int* bin_m, const float* bin_w,
                                 const float* mags, int terms, int l2, float w_sc, float w_log, float w_lin, const float* sums,
                                 const float* gout, float scale, float* dspec, void* stream);
EBEN_API int eben_stft_terms_total(const void* const* sums, const float* inv_counts, int n, int rows, int terms, float w_sc, float w_log,
                                   float w_lin, float* out, void* stream);

/* ---- optimiser (torch.optim.Adam as configured by configs/lightning_module/optimizer/adam.yaml) --- */
typedef struct EbenAdamTensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} EbenAdamTensor;
/* `table` is a HOST array of ntensors entries (device pointers inside); it is passed to the
 * kernel by value, 48 tensors per launch. */
EBEN_API int eben_adam_step(const EbenAdamTensor* table, int ntensors, int64_t max_numel, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ---- noisy-BWE batch assembly (vibravox/lightning_datamodules/noisybwe.py:219-291; utils.py:7-81,195-254) ----
 * per item:  body_conducted[i, 0, t] = speech[u] + noise[noise_start + u],  airborne[i, 0, t] = airborne_clip[u],
 * u = t + shift, zero outside [0, length).  shift >= 0: crop offset (set_audio_duration); shift < 0: left zero run
 * of pad_audio; noise / airborne_clip may be NULL (real noisy data: padding only).  `items` is a HOST array (device
 * pointers inside), passed to the kernel by value; outputs are (nitems, 1, samples). */
typedef struct EbenCollateItem {
  const float* speech;
  const float* airborne;
  const float* noise;
  int64_t length;       /* samples of speech (== airborne) */
  int64_t noise_start;  /* first noise sample mixed in */
  int64_t shift;
} EbenCollateItem;
EBEN_API int eben_noisy_collate(const EbenCollateItem* items, int nitems, int samples, float* body_conducted, float* airborne, void* stream);

/* ---- SNR-controlled mixing (mix_speech_and_noise_with_rescaling, vibravox/utils.py:118-193) --------------------------
 * eben_clip_powers: powers[i] = float32(sum(x^2) / length_i) of ragged clips (1 <= length_i); products and sums in float64, per-block
 *   partials and one fixed-order final pass, no atomics: two calls give the same bits.  `clips` is a HOST array (device pointers
 *   inside, 4-byte aligned), passed by value 48 per launch; `workspace` (device, 8-byte aligned) holds
 *   eben_clip_powers_workspace(nclips) bytes.
 * eben_noisy_collate_scaled: eben_noisy_collate with the per-item gain g = sqrt(speech_power / (noise_power * snr_linear)) read
 *   from DEVICE arrays of nitems floats:  ns = noise[noise_start + u] * g,  body_conducted = speech[u] + ns, every step rounded
 *   to float32 (utils.py:183-188; never one FMA).  Every item needs a noise clip.  noise_scaled (nullable) receives ns as
 *   (nitems, 1, samples) with the same zero fill. */
typedef struct EbenClip {
  const float* data;
  int64_t length;
} EbenClip;
EBEN_API size_t eben_clip_powers_workspace(int nclips);
EBEN_API int eben_clip_powers(const EbenClip* clips, int nclips, float* powers, void* workspace, size_t ws_bytes, void* stream);
EBEN_API int eben_noisy_collate_scaled(const EbenCollateItem* items, int nitems, int samples, const float* speech_power, const float* noise_power,
                                       const float* snr_linear, float* body_conducted, float* airborne, float* noise_scaled, void* stream);

/* ---- biquad (torchaudio.functional.lfilter of one second-order section, as lowpass_biquad / remove_hf use it, utils.py:84-116) ----
 * y[r, m] for the padded row xp[r, m] = x[r, reflect(m - pad)], m in [0, t_in + 2*pad) (ReflectionPad1d's index mapping on the
 * read; pad < t_in; nothing is materialised):  v[n] = b0 u[n] + b1 u[n-1] + b2 u[n-2] - a1 v[n-1] - a2 v[n-2] from a zero state,
 * with u[n] = xp[n], y[n] = v[n], or, when `reversed`, u[n] = xp[T-1-n], y[T-1-n] = v[n] (the row is filtered from its last
 * sample to its first and stored in the input's orientation, so no flip is ever made).  coef (HOST) = b0 b1 b2 a1 a2, already
 * divided by a0.  clamp != 0: the STORED value is clamped to [-1, 1], never the state (lfilter clamp=True).  State and
 * accumulation are float64, x and y float32; parallel along time (chunks of 4096 samples, csrc/frontend.hip).  x and y are
 * (rows, t_in) and (rows, t_in + 2*pad), not aliased; `workspace` (device, 8-byte aligned, may be NULL when the query returns
 * 0) holds eben_biquad_workspace(rows, t_in + 2*pad) bytes. */
EBEN_API size_t eben_biquad_workspace(int rows, int t_padded);
EBEN_API int eben_biquad(const float* x, float* y, int rows, int t_in, int pad, const double* coef, int reversed, int clamp, void* workspace,
                         size_t ws_bytes, void* stream);

/* ---- waveform augmentation (vibravox/torch_modules/dsp/data_augmentation.py:38-71) -------------------------------
 * time masking (dsp/time_masking_waveform.py:18-36): x[r, first : first+count] = 0 in place for r < rows;
 * polyphase windowed-sinc resampling (torchaudio.functional.resample as used by T.SpeedPerturbation, restated):
 *   out[r, q*nw + p] = sum_{j < 2*width+orig} kernels[p, j] * xpad[r, q*orig + j], xpad = x with `width` zeros in front;
 *   kernels (nw, 2*width+orig) fp32 on the device; t_out <= ceil(nw * t_in / orig). */
EBEN_API int eben_time_mask(float* x, long long rows, int t, int first, int count, void* stream);
/* phase vocoder of T.PitchShift (torchaudio.functional.phase_vocoder, restated): spec / out are flat (2*bins, rows*frames) /
 * (2*bins, rows*frames_out) spectra (re rows, then im rows), frames_out = ceil(frames / rate), hop = STFT hop length */
EBEN_API int eben_phase_vocoder(const float* spec, float* out, int rows, int bins, int frames, int frames_out, double rate, float hop,
                       void* stream);
EBEN_API int eben_resample(const float* x, const float* kernels, float* out, int rows, int t_in, int t_out, int orig, int nw,
                  int width, void* stream);

/* ---- per-clip waveform augmentation at a constant batch length (csrc/augment_clips.hip; vibravox_amd/augment.py, per_clip=True) ----
 * The kernels above with parameters PER ROW.  Every `rows` / `clips` / `bands` argument is a HOST array (device pointers inside),
 * checked whole before the first launch and passed to the kernels by value, 48 rows a launch.  A row's arithmetic is the
 * batch-level kernel's on that row alone, operation for operation (finite samples: a skipped zero tap does not propagate an
 * inf / NaN the dense sum would).
 * eben_resample_clips: eben_resample's sum over the taps that can be non-zero, the ratio chosen per row:
 *     out[dst_row, n] = sum_{j < W} band[p, j] * x[src_offset + q*orig - width + first[p] + j],  n = q*nw + p < min(ceil(nw*t_in/orig), t)
 *   (one accumulator, fmaf, j ascending, zero outside [0, t_in)), and 0 for the remaining n < t: crop / right padding to t fused.
 *   band (nw, W) fp32 and first (nw) int32 on the device: kernels[p, first[p] + j] of eben_resample's table, every value outside
 *   being exactly 0; W <= 2*width + orig; orig, nw <= 2^20; 1 <= nbands <= EBEN_CLIP_MAX_BANDS; x holds x_floats floats, out is
 *   (out_rows, t), not overlapping x; no two rows share a dst_row.
 * eben_phase_vocoder_clips: eben_phase_vocoder with spec (2*bins, nrows*frames) dense and row i walking rows[i].frames_out frames
 *   at rows[i].rate into columns [col_out, col_out + frames_out) of out (2*bins, out_cols); columns ascending and disjoint.
 * eben_overlap_add_clips: row i = overlap-add of columns [col, col + frames_out) of frames_buf (win, cols) (eben_overlap_add_ex
 *   without reflection, sample u at u + pad) times float32(1 / sum_f w2[u + pad - f*hop]), the sum over the covering frames in
 *   float64 and ascending f (w2: win doubles on the device, the squared window); len_stretch samples at out + dst_offset, zero from
 *   `valid` on; valid <= min(len_stretch, win + hop*(frames_out-1) - pad); rows ascending and disjoint in both buffers.
 * eben_time_mask_clips: x[row, first : first + count] = 0 per clip, x (rows, t); count = 0 allowed. */
#define EBEN_CLIP_MAX_BANDS 16
typedef struct EbenClipBand {
  const float* band;
  const int32_t* first;
  int32_t orig, nw, width, W;
} EbenClipBand;
typedef struct EbenResampleClip {
  int64_t src_offset;   /* floats from x to the row's first sample */
  int32_t t_in;
  int32_t band;         /* index into bands */
  int32_t dst_row;
  int32_t reserved;
} EbenResampleClip;
typedef struct EbenVocoderClip {
  double rate;
  int32_t frames_out;
  int32_t col_out;
} EbenVocoderClip;
typedef struct EbenOlaClip {
  int64_t dst_offset;   /* floats from out to the row's first sample */
  int32_t col;
  int32_t frames_out;
  int32_t len_stretch;
  int32_t valid;
} EbenOlaClip;
typedef struct EbenMaskClip {
  int32_t row, first, count;
} EbenMaskClip;
EBEN_API int eben_resample_clips(const float* x, int64_t x_floats, float* out, int out_rows, int t, const EbenClipBand* bands, int nbands,
                                 const EbenResampleClip* rows, int nrows, void* stream);
EBEN_API int eben_phase_vocoder_clips(const float* spec, float* out, int bins, int frames, int64_t out_cols, const EbenVocoderClip* rows, int nrows,
                                      float hop, void* stream);
EBEN_API int eben_overlap_add_clips(const float* frames_buf, int64_t cols, const double* w2, float* out, int64_t out_floats, int win, int hop, int pad,
                                    const EbenOlaClip* rows, int nrows, void* stream);
EBEN_API int eben_time_mask_clips(float* x, int rows, int t, const EbenMaskClip* clips, int nclips, void* stream);

/* ---- multi-rate downsampling (MelganMultiScalesDiscriminator: torchaudio Resample, "sinc_interp_kaiser") -----------------
 * Same arithmetic as eben_resample: y[r, q*nw + p] = sum_{j < taps} kernels[p, j] * x[r, q*orig + j - width] (zero outside the row).
 * eben_multirate_down: every scale s = 1 .. scales-1 reduces to orig = 2^s, new = 1; tables holds their (1, taps_s =
 *   2*widths[s-1] + 2^s) kernels back to back on the device; widths (host, scales-1 ints); outs (host array of scales-1 device
 *   pointers) receive (rows, ceil(t_in / 2^s)).  One launch for all scales.  2 <= scales <= 6.
 * eben_multirate_down_adjoint: dx = g0 + sum_s A_s^T gs[s-1], one launch, no atomics (g0 nullable = 0).
 * eben_resample_adjoint: dx = A^T g for eben_resample's arguments (accumulate != 0: dx += A^T g); no atomics. */
EBEN_API int eben_multirate_down(const float* x, const float* tables, const int* widths, float* const* outs, int rows, int t_in,
                                 int scales, void* stream);
EBEN_API int eben_multirate_down_adjoint(const float* g0, const float* const* gs, const float* tables, const int* widths, float* dx,
                                         int rows, int t_in, int scales, void* stream);
EBEN_API int eben_resample_adjoint(const float* g, const float* kernels, float* dx, int rows, int t_in, int t_out, int orig, int nw,
                                   int width, int accumulate, void* stream);

/* ---- ragged batches (csrc/ragged.hip): rows of different lengths in one (rows, channels, l_buf) buffer ------------------------
 * In place, one launch for every (row, channel); lens (DEVICE, rows int32) holds each row's own length at this tensor's rate.
 * eben_edge_fill: the `count` samples behind each row's end become what the row's own edge rule supplies to the next layer --
 *   EBEN_FILL_ZERO x[r, c, len + j] = 0, EBEN_FILL_MIRROR x[r, c, len + j] = x[r, c, len - 2 - j] (ReflectionPad1d), j < count.
 *   1 <= count < l_buf, else EBEN_EINVAL before any launch.  The kernel leaves a row alone when len == l_buf (no slack) and
 *   skips it when len + count > l_buf, len < 0 or, mirroring, count > len - 1: a bad table writes nothing out of bounds.
 * eben_edge_zero: the whole slack [len, l_buf) of every row becomes 0 (tensors handed back to the caller).
 * Added without a version bump, like eben_fir_plan: functions only. */
#define EBEN_FILL_ZERO 0
#define EBEN_FILL_MIRROR 1
EBEN_API int eben_edge_fill(float* x, const int32_t* lens, int rows, int channels, int l_buf, int mode, int count, void* stream);
EBEN_API int eben_edge_zero(float* x, const int32_t* lens, int rows, int channels, int l_buf, void* stream);

/* ---- per-row loss sums over ragged buffers (csrc/ragged_losses.hip): every clip's own value of the test-time losses -----------
 * Tables (pointers, channels, l_bufs, targets) are HOST arrays and travel by value in the kernel arguments; every `lens` /
 * `frames_of_row` they name is a DEVICE int32 array of `rows` entries the host never reads.  All reductions are two-level with a
 * fixed order and no atomics: two runs give the same bits.  A lens entry outside [0, l_buf] (a frame count outside [0, frames])
 * makes that row's results NaN and reads nothing; nothing is ever written outside `sums` / `out` and the workspace.
 * eben_fm_sums_rows: npairs <= 32 pairs; ptrs = (a_0, b_0, a_1, b_1, ...), a_i and b_i fp32 (rows, channels[i], l_bufs[i]) at any
 *   4-byte alignment (16-byte loads where a row segment of both allows them, scalar heads and tails elsewhere), lens[i] that pair's
 *   row lengths.  sums[(i * rows + r) * 2 + {0, 1}] = sum |a - b|, sum |a| over c < channels[i], l < lens[i][r].
 * eben_hinge_rows: n <= 32 terms; xs[i] fp32 (rows, 1, l_bufs[i]) logits.  out[i * rows + r] = mean_{l < lens[i][r]} max(0, 1 -
 *   targets[i] x[r, 0, l]) (NaN for an empty row).
 * eben_stft_loss_sums_rows: eben_stft_loss_sums_ex whose row r runs over its first frames_of_row[r] frames only (`frames`: the
 *   frames per row of the buffer, which the strides describe); a row with frames_of_row[r] == frames gets eben_stft_loss_sums_ex's bits.
 * eben_clip_losses: out (5, rows) = per row [MRSTFT, feature matching, adv_loss_gen, real_loss, fake_loss] in one launch:
 *   MRSTFT = mean over the n_res <= 8 resolutions of sqrt(s0 / s1) + s2 / (bins[i] * frames_of_row[i][r]) from stft_sums[i] (rows, 3);
 *   feature matching = fm_inv_count * sum over the pairs of s1 / s2 from fm_sums; the three hinge values the means over the chains
 *   of hinge[(3 * chain + k) * rows + r].  A group whose count is 0 (its pointers may then be NULL) leaves NaN in its rows of out.
 * Added without a version bump: functions only. */
EBEN_API size_t eben_fm_sums_rows_workspace(int npairs, int rows);
EBEN_API int eben_fm_sums_rows(const void* const* ptrs, const int* channels, const int* l_bufs, const int32_t* const* lens, int npairs,
                               int rows, float* partial_ws, size_t ws_bytes, float* sums, void* stream);
EBEN_API int eben_hinge_rows(const void* const* xs, const int* l_bufs, const float* targets, const int32_t* const* lens, int n, int rows,
                             float* out, void* stream);
EBEN_API size_t eben_stft_loss_sums_rows_workspace(int rows);
EBEN_API int eben_stft_loss_sums_rows(const float* spec_x, const float* spec_y, int rows, int bins, int frames,
                                      const int32_t* frames_of_row, long long row_stride, long long bin_stride, long long im_off, float eps,
                                      float* partial_ws, size_t ws_bytes, float* out, void* stream);
EBEN_API int eben_clip_losses(const void* const* stft_sums, const int32_t* const* frames_of_row, const int* bins, int n_res,
                              const float* fm_sums, int npairs, float fm_inv_count, const float* hinge, int nchains, int rows, float* out,
                              void* stream);

/* ---- streaming inference (csrc/stream.hip): a layer's input for this push from the previous push's buffer and fresh output ------
 * dst[rc, j] = prev[rc, prev_off + j] for j < n_carry; dst[rc, n_carry + j] = src[rc, src_off + j] (+ add[rc, add_off + j]) for
 * j < n_new; rc < rows_channels.  fp32 [row][C][L] tensors, each with its own row pitch (in floats); offsets and counts are
 * arbitrary.  prev may be NULL when n_carry == 0, src when n_new == 0, add always (no second source).  EBEN_EINVAL before any launch
 * for a null or misaligned-to-4 pointer, a negative offset or count, n_carry + n_new == 0, an offset plus its count past its pitch,
 * n_carry + n_new past dst_pitch, or a dst extent (rows_channels * dst_pitch floats) that overlaps the extent of a source in use.
 * Added without a version bump: a function only. */
EBEN_API int eben_stream_splice(float* dst, int dst_pitch, const float* prev, int prev_pitch, int prev_off, int n_carry, const float* src,
                                int src_pitch, int src_off, int n_new, const float* add, int add_pitch, int add_off, int rows_channels,
                                void* stream);

/* eben_stream_splice_rows: the splice with a slot dimension, for independent sessions that share one state (streaming.StreamPool).
 * rows_channels = slots * channels, slots <= EBEN_STREAM_MAX_SLOTS.  `active`: (slots + 63) / 64 HOST words, bit r of the mask = slot r
 * advances in this call; the entry copies them into a by-value kernel argument (no device mask, no copy engine: the caller may reuse
 * its words at once).  With a = popcount(active bits below r):
 *   active slot r:   what eben_stream_splice does for that row: prev is read at row r; src and add at row a when src_compact (they
 *                    hold one row per ACTIVE slot, in slot order), else at row r; dst is written at row a when dst_compact, else at r;
 *   inactive slot r: dst_compact: writes nothing; else with idle != NULL: dst[r, c, j] = idle[r, c, j] for j < n_carry + n_new (the
 *                    slot's state moves to the twin buffer unchanged); else writes nothing.
 * idle (nullable) has its own pitch and is not prev: a tensor rewritten whole every push (n_carry == 0) still holds a session's state.
 * EBEN_EINVAL before any launch, nothing written, for: what eben_stream_splice refuses; a null `active`; a null or misaligned idle;
 * n_carry + n_new past idle_pitch; channels <= 0 or rows_channels % channels != 0; more than EBEN_STREAM_MAX_SLOTS slots; a set bit
 * at or above `slots`; dst's extent overlapping prev, src, add or idle (a compact tensor's extent counts the active slots only).
 * No bit set with idle (and dst not compact) copies every slot; no bit set and nothing to write returns EBEN_OK without a launch.
 *
 * eben_copy_segments: dst[i][0 : floats) = src[i][0 : floats) for `count` <= EBEN_COPY_MAX_SEGMENTS segments read from HOST memory
 * (passed to the kernel by value), one launch.  EBEN_EINVAL before any launch for a null or misaligned-to-4 pointer, a negative count
 * of segments or of floats, more than EBEN_COPY_MAX_SEGMENTS segments, or a dst extent overlapping any src extent or another dst.
 * Segments of 0 floats are legal; nothing to copy returns EBEN_OK without a launch.
 * Added without a version bump: functions only. */
#define EBEN_STREAM_MAX_SLOTS 256
#define EBEN_COPY_MAX_SEGMENTS 64
typedef struct EbenCopySegment {
  float* dst;
  const float* src;
  long long floats;
} EbenCopySegment;
EBEN_API int eben_stream_splice_rows(float* dst, int dst_pitch, const float* prev, int prev_pitch, int prev_off, int n_carry, const float* src,
                                     int src_pitch, int src_off, int n_new, const float* add, int add_pitch, int add_off, const float* idle,
                                     int idle_pitch, int rows_channels, int channels, const unsigned long long* active, int src_compact,
                                     int dst_compact, void* stream);
EBEN_API int eben_copy_segments(const EbenCopySegment* segments, int count, void* stream);

/* ---- input at the recording's rate (csrc/rate.hip): eben_resample's arithmetic on ragged rows and on a stream's tape -----------------
 * y[q * nw + p] = sum_{j < taps} kernels[p][j] * x[q * orig + j - width], taps = 2 * width + orig, fp32 fmaf in ascending j, every
 * index outside the signal skipped: a row's or a stream's result is bit for bit eben_resample's on the whole signal alone.
 * A row's buffer holds the samples [pos0, pos0 + len) of a signal that starts at stream position 0 (pos0 stays with the caller); all
 * indices handed over are buffer-relative.  Indices below 0 and at or behind len read as zero; len is clamped into [0, row pitch], so
 * nothing outside a row's buffer is read whatever a length table holds.
 *   eben_resample_ragged  rows of l_in_buf floats with lens[r] samples each (int32 device table) -> rows of l_out_buf floats: row r gets
 *     its ceil(nw * len / orig) outputs, exact zeros behind them up to l_out_buf, and that count in out_lens[r] (int32 device table).
 *   eben_resample_stream  a tape [carry | chunk] of len samples per row (pitch tape_pitch) -> out[r, first_out + n], n < n_out.  Output n
 *     has phase (p0 + n) % nw and its tap 0 at buffer index base0 + ((p0 + n) / nw) * orig, base0 = q0 * orig - width - pos0.  end != 0:
 *     the tape's right end is the signal's own (zeros behind it); else every tap of every output must lie inside the tape.
 *   eben_resample_plan    the tile of a ratio, without launching: out[0..3] (n >= 4) = values of q per block, outputs per block, floats
 *     of the input window staged in LDS, 1 when the table is staged too (nw * taps floats fit its budget) else 0 (read through L2).
 * EBEN_EINVAL before any launch for a null or misaligned-to-4 pointer, rows outside 1 ... 65535, a ratio whose taps fit no tile,
 * l_out_buf below ceil(nw * l_in_buf / orig), a length or a range of outputs past its pitch, a phase outside [0, nw), or n_out reaching
 * past what the tape can serve.  n_out == 0 returns EBEN_OK without a launch.  Added without a version bump: functions only. */
EBEN_API int eben_resample_plan(int orig, int nw, int width, int* out, int n);
EBEN_API int eben_resample_ragged(const float* x, const int32_t* lens, const float* kernels, float* out, int32_t* out_lens, int rows,
                                  int l_in_buf, int l_out_buf, int orig, int nw, int width, void* stream);
EBEN_API int eben_resample_stream(const float* tape, const float* kernels, float* out, int rows, int tape_pitch, int len, int out_pitch,
                                  int first_out, int n_out, int p0, int base0, int end, int orig, int nw, int width, void* stream);

/* The same two steps of a stream -- splice, then resample -- for independent sessions in the slots of one state
 * (streaming.StreamPool with input_rates): every slot has its own counts, phase, ratio and parity.  The state is two tapes and two
 * FIFO buffers of `slots` rows each (row pitches tape_pitch / fifo_pitch floats); a descriptor names its slot and which of the two it
 * writes.  Descriptors are read from HOST memory, validated, and passed to the kernel by value (nothing is uploaded; the caller may
 * reuse its table at once): at most EBEN_RATE_MAX_SPLICES splices or EBEN_RATE_MAX_PIECES pieces (two per splice) per call, one launch.  Slots that no descriptor names are not touched.
 *   eben_rate_splice_slots  per descriptor, with out = tapes[tape] and in = tapes[1 - tape] (a slot never reads the tape it writes):
 *     out[slot][0 : n_carry + n_new) = [ in[slot][prev_off : prev_off + n_carry) | src[src_row][0 : n_new) ]; src holds src_rows rows
 *     of src_pitch floats (NULL when no descriptor has n_new > 0).
 *   eben_resample_slots     per piece what eben_resample_stream does on one row: the tape tapes[tape][slot] of `len` samples with the
 *     ratio ratios[ratio] (at most EBEN_RATE_MAX_RATIOS; `kernels` its (nw, 2 * width + orig) device table), p0, base0 and end, the
 *     n_out outputs to fifos[fifo][slot][first_out + n].  Pieces of different ratios share the launch: the grid is (tiles of the
 *     largest piece, pieces), each ratio with the tile eben_resample_plan states.  A push whose outputs straddle two FIFO buffers is
 *     two pieces.  Pieces with n_out == 0 are checked and dropped.
 * EBEN_EINVAL before any launch, nothing written, for: a null or misaligned-to-4 pointer; slots outside 1 ... EBEN_STREAM_MAX_SLOTS;
 * a negative count or more descriptors than the call's cap (a null table with count > 0); a slot, src_row, tape, fifo or ratio
 * index outside its range; per descriptor what eben_stream_splice / eben_resample_stream refuse (negative offsets or counts,
 * n_carry + n_new == 0 or past tape_pitch, prev_off + n_carry past tape_pitch, n_new past src_pitch, a ratio that fits no tile, len
 * past tape_pitch, first_out + n_out past fifo_pitch, a phase outside [0, nw), n_out past what the tape serves); two splices on one
 * slot; two pieces whose outputs overlap on one (fifo, slot); the extents of the two tapes, the two FIFO buffers, src and the ratio
 * tables in use overlapping where one of them is written.  An empty list returns EBEN_OK without a launch.
 * Added without a version bump: functions and POD types only. */
#define EBEN_RATE_MAX_SPLICES 64
#define EBEN_RATE_MAX_PIECES 128
#define EBEN_RATE_MAX_RATIOS 8
typedef struct EbenRateSplice {
  int slot, src_row, prev_off, n_carry, n_new, tape;
} EbenRateSplice;
typedef struct EbenRateRatio {
  const float* kernels;
  int orig, nw, width, reserved;
} EbenRateRatio;
typedef struct EbenRatePiece {
  int len, p0, base0, n_out, end, first_out;
  unsigned char slot, ratio, tape, fifo;   /* 28 bytes: a steady push of every one of 64 slots, two pieces each, is one call */
} EbenRatePiece;
EBEN_API int eben_rate_splice_slots(float* tape0, float* tape1, int tape_pitch, int slots, const float* src, int src_pitch, int src_rows,
                                    const EbenRateSplice* splices, int count, void* stream);
EBEN_API int eben_resample_slots(const float* tape0, const float* tape1, int tape_pitch, float* fifo0, float* fifo1, int fifo_pitch, int slots,
                                 const EbenRateRatio* ratios, int n_ratios, const EbenRatePiece* pieces, int count, void* stream);

/* ---- recordings to resident clips (csrc/corpus.hip): the `data` chunks of WAVE files, as they lie on disk, to rows of float32 -----------
 * `data` is one DEVICE byte buffer of data_bytes bytes (16-byte aligned) holding many files' interleaved frames; row r is one channel of
 * one file, described by an EbenPcmRow: its frames start at data + byte_offset (a multiple of 16), `frames` of them, `channels` samples
 * each, of which sample `channel` is taken.  Conversions, each exact: EBEN_PCM_S16 x / 2^15, EBEN_PCM_S24 (packed 3-byte little-endian,
 * sign-extended) x / 2^23, EBEN_PCM_S32 float(x) * 2^-31 with float(x) rounded to nearest once, EBEN_PCM_F32 a copy.
 * The table is handed over twice: rows_host (HOST memory, validated here before anything is launched) and rows_dev (its upload, what
 * the kernel reads; typically both travel with the bytes in one copy).  A row of rows_dev whose numbers would reach outside the byte
 * buffer or the output is treated as empty.  Two output forms:
 *   padded  out_offsets_host == out_offsets_dev == NULL: out is (rows, out_extent) floats, row r gets its samples, exact zeros behind
 *           them up to the pitch out_extent, and their count in out_lens[r] (int32 DEVICE table, required) -- the buffers
 *           eben_resample_ragged takes and writes.
 *   flat    out_offsets_* (HOST and DEVICE copies of `rows` int64 offsets in floats): row r's samples go to out[out_offsets[r] + n] and
 *           nothing else is written; out_extent is the size of the whole store in floats; the rows' ranges must ascend without overlap.
 *           out_lens is optional.
 *   eben_pcm_decode_ragged    row r = its `frames` converted samples.
 *   eben_pcm_resample_ragged  row r = its ceil(nw * frames / orig) resampled samples: eben_resample_ragged's kernel with its staging
 *     replaced by the converting, channel-strided load -- the tile of eben_resample_plan, the same ascending-j fmaf order -- so the
 *     outputs are bit for bit those of eben_resample_ragged on the decoded row.  `kernels`: the (nw, 2 * width + orig) device table.
 * Mono EBEN_PCM_S16 rows take 16-byte loads per lane; other rows are read sample by sample.
 * EBEN_EINVAL before any launch, nothing written, for: a null or misaligned pointer (data to 16 bytes, tables to 8, out / out_lens /
 * kernels to 4); only one of the two offset tables; rows outside 1 ... 65535; an unknown format; channels outside 1 ... 65535;
 * channel >= channels; negative frames or more than 0x7fff0000 samples a row; a byte_offset that is negative or no multiple of 16; a
 * row reaching past data_bytes; a pitch too small for its row; a flat range past out_extent or not behind the previous row's; a
 * ratio whose taps fit no tile.  Added without a version bump: functions and a POD type only. */
#define EBEN_PCM_S16 0
#define EBEN_PCM_S24 1
#define EBEN_PCM_S32 2
#define EBEN_PCM_F32 3
typedef struct EbenPcmRow {
  long long byte_offset;
  int frames, channels, channel, format;   /* 24 bytes */
} EbenPcmRow;
EBEN_API int eben_pcm_decode_ragged(const void* data, long long data_bytes, const EbenPcmRow* rows_host, const EbenPcmRow* rows_dev,
                                    const long long* out_offsets_host, const long long* out_offsets_dev, float* out, int32_t* out_lens, int rows,
                                    long long out_extent, void* stream);
EBEN_API int eben_pcm_resample_ragged(const void* data, long long data_bytes, const EbenPcmRow* rows_host, const EbenPcmRow* rows_dev,
                                      const float* kernels, const long long* out_offsets_host, const long long* out_offsets_dev, float* out,
                                      int32_t* out_lens, int rows, long long out_extent, int orig, int nw, int width, void* stream);

/* ---- rows of float32 to the bytes of WAVE files (csrc/pcm_encode.hip): the decoder's way back ---------------------------------------------
 * `src` is one DEVICE buffer of src_floats floats; row r, described by an EbenPcmEncRow, is the `samples` floats from src + src_offset
 * (any offset: a row of a padded buffer at r * pitch and a clip inside a flat store are the same case).  Its mono little-endian samples
 * go to image + byte_offset (a multiple of 16) of a flat DEVICE byte image of image_bytes bytes (16-byte aligned): `samples` * 2 / 3
 * (packed) / 4 / 4 bytes and not one more -- headers, the gaps between rows and everything else in the image stay as they are.
 * Conversions, deterministic, no dither, each the inverse of the decoder's: with b the bit depth and v = rint(x * 2^(b-1)), half to
 * even in float32 (the product is exact), EBEN_PCM_S16 / S24 / S32 store v clamped to [-2^(b-1), 2^(b-1) - 1] and 0 for a NaN;
 * EBEN_PCM_F32 stores the bits of x.  clipped[r] (int32 DEVICE table, required; set to zero by a memset on `stream` in front of the
 * launch) receives the number of samples of row r with v >= 2^(b-1), v < -2^(b-1) or x a NaN -- an integer sum, the same on every run;
 * EBEN_PCM_F32 never clips.
 * The table is handed over twice, as for the decoder: rows_host is validated here before anything is launched, the kernel reads
 * rows_dev and treats a row whose numbers would reach outside src or the image as empty.  EBEN_PCM_S16 rows convert into LDS and
 * store 16 bytes (8 samples) per lane, whatever the alignment of the source row, the last partial vector sample by sample; the other
 * formats store sample by sample.  A block owns eben_pcm_encode_plan's out[0] consecutive samples of one row (n >= 1; no launch).
 * EBEN_EINVAL before any launch, nothing written, for: a null or misaligned pointer (image to 16 bytes, tables to 8, src and clipped
 * to 4); rows outside 1 ... 65535; an unknown format; negative samples or more than 0x7fff0000 a row; a negative src_offset or a row
 * reaching past src_floats; a byte_offset that is negative or no multiple of 16; a row reaching past image_bytes; two rows whose byte
 * ranges overlap (in any order).  Added without a version bump: functions and a POD type only. */
typedef struct EbenPcmEncRow {
  long long src_offset;    /* of the row's sample 0 in src, in floats */
  long long byte_offset;   /* of its first byte in the image */
  int samples, format;     /* 24 bytes */
} EbenPcmEncRow;
EBEN_API int eben_pcm_encode_plan(int* out, int n);
EBEN_API int eben_pcm_encode_ragged(const float* src, long long src_floats, const EbenPcmEncRow* rows_host, const EbenPcmEncRow* rows_dev, void* image,
                                    long long image_bytes, int32_t* clipped, int rows, void* stream);
/* eben_pcm_encode_ragged with a factor per row: gains is a DEVICE float32 table of `rows` entries (required, 4-byte aligned), and sample
 * n of row r is converted from v = x[n] * gains[r], rounded to float32 first -- the same kernel body, tile, rounding, clamp, NaN rule and
 * clipped count (a NaN gain makes every sample of its row a NaN); EBEN_PCM_F32 stores the bits of v.  With every gain exactly 1.0 the
 * image is that of eben_pcm_encode_ragged (a signalling NaN in an EBEN_PCM_F32 row aside: the product quiets it).  The table is read by
 * the kernel alone, so it may come from a launch queued in front of this one (eben_loudness) without a host wait.  Refusals as above,
 * plus a null or misaligned gains.  Added without a version bump: a function only. */
EBEN_API int eben_pcm_encode_ragged_gain(const float* src, long long src_floats, const EbenPcmEncRow* rows_host, const EbenPcmEncRow* rows_dev,
                                         void* image, long long image_bytes, int32_t* clipped, const float* gains, int rows, void* stream);

/* ---- live sessions in and out as PCM at the caller's rate (csrc/stream_pcm.hip): the pool's front and back end, one launch each ----------
 * eben_stream_pcm_out: the back end of all sessions of one run -- what eben_rate_splice_slots, eben_resample_slots and
 * eben_pcm_encode_ragged do one after the other, per slot, without the float FIFO between them.  The state is two tapes of `slots` rows
 * (row pitch tape_pitch floats) as in eben_rate_splice_slots; `src` holds src_rows rows of src_pitch floats (the model-rate samples a run
 * emitted, one row per session); `image` is a flat DEVICE byte image of image_bytes < 2^31 bytes (16-byte aligned).  Pieces are read from
 * HOST memory, validated, and passed to the kernel by value: at most EBEN_STREAM_PCM_MAX_PIECES per call, one launch.  Per piece:
 *   tape     with out = tapes[tape] and in = tapes[1 - tape]: out[slot][0 : n_carry + n_new) = [ in[slot][prev_off : prev_off + n_carry) |
 *            src[src_row][0 : n_new) ], exactly what eben_rate_splice_slots leaves behind -- also when n_out == 0 (a push below the
 *            look-ahead completes no output);
 *   outputs  output n < n_out is what eben_resample_stream computes on that tape (len = n_carry + n_new) with ratios[ratio] (`kernels` its
 *            (nw, 2 * width + orig) device table), p0, base0 and end: acc = 0, acc = fmaf(k[j], x[j], acc) in ascending j over all taps,
 *            taps outside [0, len) reading zero -- bit for bit the outputs of eben_resample_slots;
 *   store    each output converted by the rules of eben_pcm_encode_ragged (rint(x * 2^(b-1)) half to even, clamped, a NaN as 0;
 *            EBEN_PCM_F32 the bits) to image + byte_offset + n * bytes per sample, byte_offset a multiple of 16; clipped[slot] (int32
 *            DEVICE table of `slots` entries, accumulated and never cleared here) grows by the count eben_pcm_encode_ragged would report.
 *   ratio == -1 (the session leaves at the model's rate): output n = src[src_row][n], n_out == n_new, n_carry == 0; no tape is touched
 *            (both tapes may be NULL when no piece resamples).
 * The blocks of a piece read only tapes[1 - tape] and src and write only tapes[tape] and the image: no launch reads what it writes.
 * The grid is (tiles of the largest piece, pieces), 256 threads, consecutive lanes consecutive outputs; the window is staged in LDS from
 * its two sources, the table beside it when it fits (else read through L2); stores go out sample by sample.
 *   eben_stream_pcm_plan  the tile of a ratio, without a launch: out[0..2] (n >= 3) = outputs per block, floats of the input window staged
 *     in LDS, the table's route (0 through L2, 1 in LDS, 2 in LDS with one value per tap for every output).  orig == nw == 1 with width 0
 *     states the tile of ratio == -1.
 * EBEN_EINVAL before any launch, nothing written, for: a null or misaligned pointer (image to 16 bytes, the others to 4); slots outside
 * 1 ... EBEN_STREAM_MAX_SLOTS; a negative count or more than EBEN_STREAM_PCM_MAX_PIECES pieces; image_bytes negative or not below 2^31;
 * a slot, src_row, tape, ratio, format or end outside its range; per piece what eben_rate_splice_slots, eben_resample_slots and
 * eben_pcm_encode_ragged refuse (negative offsets or counts, n_carry + n_new == 0 or past tape_pitch, prev_off + n_carry past tape_pitch,
 * n_new past src_pitch, a ratio that fits no tile, a phase outside [0, nw), n_out past what the tape serves, a byte_offset that is
 * negative or no multiple of 16, bytes past image_bytes); ratio == -1 with n_carry != 0 or n_out != n_new; two pieces on one slot; two
 * pieces whose byte ranges overlap; the extents of the tapes, src, the image, clipped and the tables in use overlapping where one of
 * them is written.  An empty list returns EBEN_OK without a launch.
 *
 * eben_pcm_chunks_in: the front of all sessions of a tick.  Chunk i is `n` mono samples of `format` at the DEVICE pointer `bytes` (any
 * alignment: a frame inside a network buffer), converted exactly as eben_pcm_decode_ragged converts them, to dst[dst_row][0 : n) of a
 * (rows, pitch) float32 buffer; nothing else is written.  Descriptors are read from HOST memory, validated and passed by value: at most
 * EBEN_PCM_MAX_CHUNKS per call, one launch; a block owns EBEN_PCM_CHUNK_TILE consecutive samples of one chunk.  EBEN_EINVAL before any
 * launch, nothing written, for: a null table, a null or misaligned-to-4 dst, a negative count or more than EBEN_PCM_MAX_CHUNKS chunks,
 * rows or pitch below 1, null bytes with n > 0, negative n or n past the pitch, an unknown format, a dst_row outside [0, rows), two
 * chunks on one row, a chunk's bytes overlapping dst's extent.  Chunks of 0 samples are legal; nothing to convert returns EBEN_OK
 * without a launch.  Added without a version bump: functions and POD types only. */
#define EBEN_STREAM_PCM_MAX_PIECES 64
#define EBEN_PCM_MAX_CHUNKS 64
#define EBEN_PCM_CHUNK_TILE 1024
typedef struct EbenStreamPcmPiece {
  int prev_off, n_carry, n_new, p0, base0, n_out, byte_offset;
  unsigned short src_row;
  unsigned char slot, tape;
  signed char ratio;                     /* -1: no resampling */
  unsigned char format, end, reserved;   /* 36 bytes: 64 pieces and the ratios stay below eben_resample_slots' piece table */
} EbenStreamPcmPiece;
typedef struct EbenPcmChunk {
  const void* bytes;
  int n, format, dst_row;   /* 24 bytes with the tail padding */
} EbenPcmChunk;
EBEN_API int eben_stream_pcm_plan(int orig, int nw, int width, int* out, int n);
EBEN_API int eben_stream_pcm_out(float* tape0, float* tape1, int tape_pitch, int slots, const float* src, int src_pitch, int src_rows,
                                 const EbenRateRatio* ratios, int n_ratios, void* image, long long image_bytes, int32_t* clipped,
                                 const EbenStreamPcmPiece* pieces, int count, void* stream);
EBEN_API int eben_pcm_chunks_in(const EbenPcmChunk* chunks, int count, float* dst, int rows, int pitch, void* stream);

/* ---- many tensors to one byte image and back (csrc/snapshot.hip): the device half of a checkpoint ------------------------------------
 * Entry i is the nbytes bytes at the DEVICE pointer `tensor` (any alignment for kind 0; kind 1 is float32: pointer and nbytes multiples
 * of 4) and the bytes [image_offset, image_offset + nbytes) of a flat DEVICE image of image_bytes bytes (pointer and size multiples of
 * 16).  Every offset is a multiple of 16; nbytes 0 is legal and copies nothing.  The copies move bits (NaN payloads, -0.0 and denormals
 * survive): a block owns eben_pack_plan's *block_bytes consecutive bytes of one entry; one that lies wholly inside its tensor with the
 * tensor on the 16-byte grid moves 16-byte vectors, all loads before the first store, every other block goes byte by byte.
 *   eben_pack_tensors    tensors -> image.  The table is in the image's order (offsets ascending, no overlap).  The padding in front of
 *                        the first entry, between one entry's end and the next one's offset and behind the last up to image_bytes is
 *                        written as zeros, so every byte of the image is written.  nonfinite[i] (n counters, zeroed here on the stream;
 *                        may be null without a kind-1 entry) receives the number of infinities and NaNs of entry i when it is kind 1:
 *                        integer sums, one atomicAdd per block that found any.  `reserved` is ignored.
 *   eben_unpack_tensors  image -> tensors, the entries in any order (no overlap in the image).  Only the entries' own bytes are written.
 *   eben_pack_plan       no launch: *blocks = the blocks eben_pack_tensors launches for the table (the last entry counted up to the
 *                        next multiple of 16), *block_bytes = a block's bytes.  Either output may be null, and so may the table with n 0.
 * The whole table is checked before the first launch: EBEN_EINVAL, nothing launched or written, for a null table, tensor or image,
 * n < 1, a kind other than 0 / 1, negative nbytes, a float32 entry off the 4-byte grid, a misaligned or negative offset, an entry
 * reaching past image_bytes, overlapping entries, and -- pack -- offsets that do not ascend or float32 entries without counters.
 * Added without a version bump: functions and a POD type only. */
typedef struct EbenPackEntry {
  void* tensor;
  long long image_offset;
  long long nbytes;
  int kind;       /* 0 bytes, 1 float32 */
  int reserved;   /* 32 bytes */
} EbenPackEntry;
EBEN_API int eben_pack_tensors(const EbenPackEntry* table, int n, void* image, long long image_bytes, unsigned* nonfinite, void* stream);
EBEN_API int eben_unpack_tensors(const EbenPackEntry* table, int n, const void* image, long long image_bytes, void* stream);
EBEN_API int eben_pack_plan(const EbenPackEntry* table, int n, long long* blocks, int* block_bytes);

/* ---- misc ------------------------------------------------------------------------------- */
/* out[0] = sqrt(sum x^2) (torch.norm at eben.py:226); `out` must hold 257 floats (scratch) */
EBEN_API int eben_l2norm(const float* x, size_t n, float* out, void* stream);

/* ---- validation metrics (base_se.py common_eval_logging: torchmetrics SI-SDR and STOI) ------------------------------
 * eben_si_sdr: out[r] = scale_invariant_signal_distortion_ratio(preds[r, :], target[r, :], zero_mean=False), fp64 sums.
 * eben_stoi: out[r] = pystoi stoi(x = clean[r, :], y = processed[r, :], fs), extended=False (torchmetrics' call order).
 *   fs != 10000: both signals are first resampled to 10 kHz as scipy resample_poly(x, p, q, window=h), p/q = 10000/fs reduced;
 *   resample_table holds `up * h` (taps = 2*half+1 floats, on the device), built by the caller once per fs.  At fs == 10000
 *   the table is ignored.  `workspace` (device, eben_stoi_workspace(rows, t, fs) bytes) holds the resampled signals, frame
 *   energies, the kept-frame tables and band envelopes; no host synchronisation.  Rows left with fewer than 30 STFT frames
 *   after silence removal get 1e-5. */
EBEN_API int eben_si_sdr(const float* preds, const float* target, int rows, int t, float* out, void* stream);
EBEN_API size_t eben_stoi_workspace(int rows, int t, int fs);
EBEN_API int eben_stoi(const float* clean, const float* processed, int rows, int t, int fs, const float* resample_table, int taps,
              void* workspace, size_t ws_bytes, float* out, void* stream);

/* ---- the same metrics over rows of different lengths (corpus evaluation in ragged batches) ------------------------------------
 * Rows are t_max floats apart; row r is the signal [0, lengths[r]) and what lies behind it is never read.  lengths (DEVICE, rows
 * int32) is never seen by the host: grids and the workspace are sized from t_max (eben_stoi_ragged_workspace(rows, t_max, fs) bytes,
 * every row at full length with all frames kept) and a row's surplus workgroups return at once.  out[r] has the bits of the dense
 * entry on row r alone (preds[r, :lengths[r]] as a (1, lengths[r]) call): the same kernels with the row's own length, loop order and
 * reduction order.  A lengths[r] outside [1, t_max] cannot be refused by the host: that row reads nothing and gets out[r] = NaN, the
 * other rows are unaffected.  EBEN_EINVAL before any launch for a null pointer, rows outside [1, 65535], t_max <= 0, fs <= 0 or, at
 * fs != 10000, a missing or even-length table; EBEN_EWORKSPACE for a short workspace.  Any 4-byte-aligned base and any t_max.
 * Added without a version bump: functions only. */
EBEN_API int eben_si_sdr_ragged(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, float* out,
                                void* stream);
EBEN_API size_t eben_stoi_ragged_workspace(int rows, int t_max, int fs);
EBEN_API int eben_stoi_ragged(const float* clean, const float* processed, int rows, int t_max, const int32_t* lengths, int fs,
                              const float* resample_table, int taps, void* workspace, size_t ws_bytes, float* out, void* stream);

/* ---- evaluation metrics beyond the two base_se.py logs: zero-mean SI-SDR / SI-SNR, SNR, ESTOI, log-spectral distance ---------------
 * The conventions of the ragged entries above, with a NULLABLE lengths (null: every row is t_max long): one value per row, fp64
 * reductions in a fixed order, so out[r] has the bits of the call on row r alone; a lengths[r] outside its valid range makes that row
 * NaN and touches nothing else; nothing behind a row's end is read; no host synchronisation.
 * eben_signal_ratio: kind EBEN_RATIO_SI_SDR is torchmetrics scale_invariant_signal_distortion_ratio(preds, target, zero_mean),
 *   EBEN_RATIO_SNR its signal_noise_ratio(preds, target, zero_mean) = 10 log10((sum t^2 + eps) / (sum (t - p)^2 + eps)), eps the float32
 *   machine epsilon.  zero_mean = 1 subtracts each signal's fp64 mean over the row's own length first; SI-SNR is SI_SDR with it.
 * eben_estoi: pystoi stoi(clean, processed, fs, extended=True) -- the front end of eben_stoi (resample, silence removal, third-octave
 *   envelopes), then per 15 x 30 segment both matrices' rows, then columns, centred and normalised, d = sum x_n y_n / (30 J).  No
 *   EPS * randn dither; a row or column whose centred norm is exactly 0 contributes 0.  Fewer than 30 frames: 1e-5.  out_classic
 *   (nullable) also receives what eben_stoi[_ragged] writes, from the same envelopes: one front end, two tails.
 *   Workspace: eben_estoi_workspace(rows, t_max, fs) bytes (eben_stoi's plus a double per possible segment).
 * eben_lsd: P(s) = clamp(|torch.stft(s, n_fft, hop, win_length = n_fft, hann_window(n_fft), center = True, "reflect")|^2, min = 1e-8),
 *   D[f] = sqrt(mean over the band's bins of (log10 P(preds) - log10 P(target))^2), out[band * rows + r] = mean of D over the row's own
 *   1 + len / hop frames, reflected at the row's own end.  n_fft a power of two in [256, 4096], 1 <= hop <= n_fft, 1 <= nbands <= 4,
 *   band b the bins [band_lo[b], band_hi[b]) inside [0, n_fft / 2 + 1) (HOST arrays).  A row with len <= n_fft / 2 cannot be
 *   reflect-padded: NaN.  Workspace: eben_lsd_workspace(rows, t_max, n_fft, hop, nbands) bytes.
 * EBEN_EINVAL before any launch for a null pointer (other than lengths / out_classic) or an argument outside the ranges above,
 * EBEN_EWORKSPACE for a short workspace.  Added without a version bump: functions only, and a binding that needs them finds out by
 * looking the symbols up. */
#define EBEN_RATIO_SI_SDR 0
#define EBEN_RATIO_SNR 1
EBEN_API int eben_signal_ratio(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int kind,
                               int zero_mean, float* out, void* stream);
EBEN_API size_t eben_estoi_workspace(int rows, int t_max, int fs);
EBEN_API int eben_estoi(const float* clean, const float* processed, int rows, int t_max, const int32_t* lengths, int fs,
                        const float* resample_table, int taps, void* workspace, size_t ws_bytes, float* out, float* out_classic,
                        void* stream);
EBEN_API size_t eben_lsd_workspace(int rows, int t_max, int n_fft, int hop, int nbands);
EBEN_API int eben_lsd(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int n_fft, int hop,
                      const int* band_lo, const int* band_hi, int nbands, void* workspace, size_t ws_bytes, float* out, void* stream);

/* ---- BSS-eval signal-to-distortion ratio (torchmetrics signal_distortion_ratio, direct-solve branch; csrc/sdr.hip) -------------------
 * The conventions of the evaluation metrics above: rows t_max floats apart, a NULLABLE device lengths, one float per row, fp64 sums in
 * an order that depends on the row's own length and on filter_length only, so out[r] has the bits of the call on row r alone; nothing
 * behind a row's end is read; no host synchronisation.  Per row of N samples, in float64: t, p = target, preds (zero_mean = 1: minus
 * their means over the N samples), each divided by max(its norm, 1e-6); r[k] = sum_n t[n] t[n + k] and b[k] = sum_n t[n] p[n + k] for
 * k < filter_length (linear correlations, 0 for k >= N); r[0] += load_diag (0.0 for torchmetrics' None); Toeplitz(r) h = b by Levinson's
 * recursion; coh = b . h; out[r] = 10 log10(coh / (1 - coh)).  There is no eps: a silent target gives NaN, preds proportional to
 * target whatever 1 - coh leaves (a very large value, +inf or NaN); a lengths[r] outside [1, t_max] gives NaN.  With filter_length = 1
 * this is SI-SDR without its eps.  workspace: eben_sdr_workspace(rows, t_max, filter_length) bytes on the device (two means and two
 * inverse norms per row, then 2 filter_length doubles per row and segment of 8192 samples of t_max); the entry trusts its size.
 * EBEN_EINVAL before any launch for a null pointer (other than lengths), rows outside [1, 65535], t_max outside [1, INT_MAX - 16384],
 * filter_length outside [1, 512], zero_mean neither 0 nor 1 or a NaN load_diag; eben_sdr_workspace returns 0 for such arguments.
 * Added without a version bump: functions only. */
EBEN_API size_t eben_sdr_workspace(int rows, int t_max, int filter_length);
EBEN_API int eben_sdr(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int filter_length,
                      int zero_mean, double load_diag, void* workspace, float* out, void* stream);

/* ---- frame-based objective speech measures (Hu & Loizou 2008: segmental SNR, frequency-weighted segmental SNR, LPC log-likelihood
 * ratio, LPC cepstral distance; csrc/speech_measures.hip) -----------------------------------------------------------------------------
 * The conventions of the evaluation metrics above: rows t_max floats apart, a NULLABLE device lengths, one float per row and measure,
 * every reduction in an order that depends on the row's own length only, so a value has the bits of the call on its row alone; nothing
 * at or behind a row's end is read; no host synchronisation.  preds = processed, target = clean.  The definitions restate the published
 * code (parity unpinned):
 *   fs 16000 or 8000; W = floor(0.030 fs + 0.5) (480 / 240), S = W / 4, F = (N - W) / S frames for a row of N >= W samples (one fewer
 *   than would fit), frame f = samples [f S, f S + W).  window: W DOUBLES on the device, w[n] = 0.5 (1 - cos(2 pi (n + 1) / (W + 1))),
 *   computed by the caller.  c = w * target frame, p = w * preds frame, in float64.  eps = 2^-52.  A frame is EMPTY when sum c^2 == 0 or
 *   sum p^2 == 0.
 *   EBEN_MEASURE_SEG_SNR     mean over all F frames of clip(10 log10(sum c^2 / (sum (c - p)^2 + eps) + eps), -10, 35)
 *   EBEN_MEASURE_FW_SEG_SNR  n_fft = 1024 / 512, n2 = n_fft / 2; C[j] = |FFT(c)|[j] for j < n2 divided by its sum over j, P likewise
 *                            (one float32 complex transform of c / |c| + i p / |p|); 25 critical bands with Gaussian-shaped filters
 *                            g_i[j] = exp(-11 ((j - floor(cent_i / (fs / 2) n2)) / (bw_i / (fs / 2) n2))^2 + ln 70 - ln bw_i), set to 0
 *                            where <= exp(-30 / 4.606) (centres 50 ... 3597.63 Hz and bandwidths 70 ... 346.136 Hz: the table in
 *                            speech_measures.hip); Ec_i = sum_j C[j] g_i[j], Ep_i likewise; snr_i = clip(10 log10(Ec_i^2 /
 *                            max((Ec_i - Ep_i)^2, eps)), -10, 35); frame value sum_i Ec_i^0.2 snr_i / sum_i Ec_i^0.2; the mean over
 *                            the non-empty frames
 *   LPC of order 16 / 10: R[k] = sum_n x[n] x[n + k], Levinson-Durbin, A = [1, -a_1 ... -a_P], float64.
 *   EBEN_MEASURE_LLR         per non-empty frame min(2, ln((A_p T A_p') / (A_c T A_c'))), T the Toeplitz matrix of the clean frame's R
 *   EBEN_MEASURE_CD          cep_1 = a_1, cep_m = a_m + (1 / m) sum_{k < m} k cep_k a_{m - k}; per non-empty frame
 *                            min(10, (10 / ln 10) sqrt(2 sum_m (cep_c[m] - cep_p[m])^2))
 *   LLR and CD of a row: the mean of the (95 F' + 50) / 100 smallest of its F' non-empty frames' values.
 * measures: a non-empty mask of EBEN_MEASURE_*; out: one plane of `rows` floats per set bit, in bit order.  A row with F < 1 (N < W + S,
 * or a lengths[r] outside [1, t_max]) is NaN in every plane; a row without a non-empty frame is NaN in all but the SEG_SNR plane.
 * workspace: eben_speech_measures_workspace(rows, t_max, fs, measures) bytes on the device (the transform's twiddles and the band
 * filters, then one double per row, possible frame and measure); the entry trusts its size.  EBEN_EINVAL before any launch for a null
 * pointer (other than lengths), rows outside [1, 65535], t_max outside [1, INT_MAX - 4096], an fs other than the two or a mask that is
 * empty or has other bits; eben_speech_measures_workspace returns 0 for such arguments.  Added without a version bump: functions only. */
#define EBEN_MEASURE_SEG_SNR 1
#define EBEN_MEASURE_FW_SEG_SNR 2
#define EBEN_MEASURE_LLR 4
#define EBEN_MEASURE_CD 8
EBEN_API size_t eben_speech_measures_workspace(int rows, int t_max, int fs, int measures);
EBEN_API int eben_speech_measures(const float* preds, const float* target, int rows, int t_max, const int32_t* lengths, int fs,
                                  int measures, const double* window, void* workspace, float* out, void* stream);

/* ---- integrated loudness of ITU-R BS.1770-4, one channel, per row (csrc/loudness.hip) ------------------------------------------------------
 * Restated from the recommendation (parity with pyloudnorm / libebur128 unpinned).  x: (rows, t_max) float32 on the device; row r is its
 * first lengths[r] samples (lengths: DEVICE int32, or NULL: every row has t_max), nothing behind them is read.
 *   K-weighting  two second-order sections in cascade from a zero state at the row's first sample, coefficients for `fs` in float64 on the
 *                host (eben_k_weighting: coef = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2).  Shelf: f0 = 1681.974450955533,
 *                G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *                a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2)/a0, 2(K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0], a = [1, 2(K^2 - 1)/a0,
 *                (1 - K/Q + K^2)/a0].  High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a as above with its own
 *                K and a0.  At 48 kHz these are the recommendation's printed coefficients.
 *   blocks       n = 0.4 fs samples every h = 0.1 fs, only those wholly inside the row; z_j = the mean square of block j's weighted samples,
 *                l_j = -0.691 + 10 log10 z_j.
 *   gates        absolute: l_j > -70; relative: Gr = -0.691 + 10 log10(mean of the z_j kept by the absolute gate) - 10;
 *                loudness[r] = -0.691 + 10 log10(mean of the z_j with l_j > -70 and l_j > Gr), -inf when no block is left (or there is none).
 *   peak[r]      max |x| over the row's own samples (sample peak), 0 for an empty row.
 *   gain[r]      (gain may be NULL) g = 10^((target_lufs - L) / 20), L before its rounding to float32; if g * peak > 10^(peak_dbfs / 20)
 *                then g = 10^(peak_dbfs / 20) / peak; g = 1 when L is not finite or the peak is 0.  Formed in float64, stored as float32.
 * Filter state, squares and every sum are float64 on the float32 input; each sum has one fixed order that depends only on a sample's
 * place in its own row (no floating-point atomics), so a row's three values are the bits of the call on that row alone, in any batch,
 * at any position and buffer width.  A lengths[r] outside [0, t_max] makes loudness[r] and peak[r] NaN and gain[r] 1; NaN samples make
 * them NaN as well.  The weighted signal is never stored: the workspace (eben_loudness_workspace bytes on the device, 8-byte aligned)
 * holds a state per 4096-sample chunk, a sum per (chunk, hop) piece and per hop, and a peak per chunk.  Launches: two passes over the
 * input with a carry between them (one pass when t_max <= 4096) and one workgroup per row for the gates.
 * EBEN_EINVAL before any launch for: a null pointer (other than lengths and gain) or a misaligned one (workspace to 8 bytes, the others to
 * 4); rows outside [1, 65535]; t_max outside [1, INT_MAX - 4096]; an fs that is no positive multiple of 10; a non-finite target_lufs or
 * peak_dbfs; ws_bytes below eben_loudness_workspace(rows, t_max, fs), which returns 0 for arguments that would be refused.
 * Added without a version bump: functions only. */
EBEN_API int eben_k_weighting(int fs, double* coef /* 10 values, HOST */);
EBEN_API size_t eben_loudness_workspace(int rows, int t_max, int fs);
EBEN_API int eben_loudness(const float* x, int rows, int t_max, const int32_t* lengths, int fs, double target_lufs, double peak_dbfs, float* loudness,
                           float* peak, float* gain, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBEN_HIP_H */
