"""GPU: every launch of the gen_conv case table (tests/test_gen_conv_variants.py) through the C ABI -- eben_wn_scale, eben_conv1d_pack,
eben_conv1d_fwd / eben_conv1d_fwd_res, as the generator's forward drives them -- against float64.  Before each launch the case's
gc_kernel<FORM, RT, CT, NP> is asserted through eben_conv1d_variant, so a case a retuned gc_plan moved elsewhere fails by name instead of
passing on another kernel.

(a) same operands: the float64 sum of exactly the bf16 piece products the kernel forms (pieces p0 = bf16(v), p1 = bf16(v - p0),
    p2 = bf16(v - p0 - p1) of lrelu(x, in_slope) and of the fp32 product w * scale, scale read back from the device; products (qw, qx)
    with qw + qx <= NP - 1), epilogue in float64.  Kernel and reference differ by the fp32 accumulation and its order only: 3e-6 of
    max |ref|, the bar test_generator_direct_operand_convs holds for the same accumulation.
(b) exact operands: oracle.eben_oracle.conv_layer on doubles.  NP = 3: 3e-6.  NP = 2: per element
    |y - y64| <= 3 * 2^-16 (|w| (*) |lrelu(x)|) + 3e-6 max |y64| on the pre-activation sum (3 * 2^-16 per product: the dropped lo x lo
    term and the rounding of the lo pieces, PRODUCT_REL of tests/test_gpu_stft.py); the slopes are <= 1, so the bound carries through
    the output activation, and the residual is added exactly.
(c) the inputs discriminate: reference (a) with the hi x lo or the lo x hi product left out differs from the full one by more than
    10 x the bar of (a) on the case's data -- a kernel that dropped or mispaired a cross term would fail (a), not pass on lucky inputs.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from formula import formula_tensor
from oracle import eben_oracle as O
from tests.test_gen_conv_variants import CASES, gc_tuple

pytestmark = pytest.mark.gpu
BAR_A = 3e-6            # (a), and (b) at NP = 3
PRODUCT_REL_X3 = 3 * 2.0 ** -16
RES_SLOPE = 0.3


def pieces(v, n):
    """The kernel's split (gc_split / gc_pack_kernel): piece q = bf16_rne(v - p0 - .. - p(q-1)), every residual exact in fp32."""
    assert v.dtype == torch.float32
    out, t = [], v.clone()
    for _ in range(n):
        p = t.to(torch.bfloat16).to(torch.float32)
        out.append(p.double())
        t = t - p
    return out


def lrelu32(x, slope):
    return torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32)) if slope != 1.0 else x


def conv64(x, w, spec):
    """The layer's contraction on float64 operands, padding included; no bias, no activation."""
    if spec.transposed:
        return F.conv_transpose1d(x, w, None, stride=spec.stride, padding=spec.pad_l)
    if spec.pad_l or spec.pad_r:
        x = F.pad(x, (spec.pad_l, spec.pad_r), mode="reflect" if spec.reflect else "constant")
    return F.conv1d(x, w, None, stride=spec.stride)


def max_rel(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("name", list(CASES))
def test_gc_instantiation_against_float64(hip, name):
    """Each case of the table on its own instantiation against the three comparisons of the module docstring.
    [MI355X] worst over the table: (a) 6.54e-07 of max |ref| (bar 3e-6; f2_r1c1_x6_s2_b1, the longest reduction); (b) NP = 3 6.40e-07
    (bar 3e-6), NP = 2 0.188 of the per-element bound (f2_r2c2_x3_s2); (c) the smallest effect of a dropped cross term is 142 x the
    bar of (a) (f2_r2c1_x6_s8; asked: > 10 x)."""
    from vibravox_amd._lib import check, ptr, stream

    lib = hip
    case = CASES[name]
    spec = case.spec()
    form, rt, ct, np_ = gc_tuple(lib, name, case)
    assert (form, rt, ct, np_) == case.expect, f"{name}: runs gc_kernel{(form, rt, ct, np_)}, the case is written for {case.expect}"
    batch, length, l_out = case.batch, case.length, spec.out_len(case.length)
    wshape = spec.weight_shape()
    v = formula_tensor(f"gcv/{name}/w", wshape, 1 / math.sqrt(wshape[1] * wshape[2]))
    g = formula_tensor(f"gcv/{name}/g", (wshape[0], 1, 1)).abs() + 0.5
    bias = formula_tensor(f"gcv/{name}/b", (spec.c_out,), 0.1) if case.bias else None
    x = formula_tensor(f"gcv/{name}/x", (batch, spec.c_in, length))
    res = formula_tensor(f"gcv/{name}/r", (batch, spec.c_out, l_out)) if case.res else None

    dev = torch.device("cuda")
    d = case.desc()
    vd, gd = v.to(dev), g.to(dev)
    if case.offset:   # rows that are 4-byte but not 16-byte aligned
        buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
        xd = buf[1:].view(x.shape)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = x.to(dev)
    scale = torch.full((wshape[0],), float("nan"), dtype=torch.float32, device=dev)
    norm = torch.empty_like(scale)
    check(lib.eben_wn_scale(ptr(gd), ptr(vd), wshape[0], wshape[1] * wshape[2], ptr(scale), ptr(norm), stream()), "wn_scale")
    wp = torch.full((lib.eben_conv1d_packed_floats(ctypes.byref(d), 0),), float("nan"), dtype=torch.float32, device=dev)
    check(lib.eben_conv1d_pack(ctypes.byref(d), ptr(vd), ptr(scale), ptr(wp), None, stream()), "pack")
    y = torch.full((batch, spec.c_out, l_out), float("nan"), dtype=torch.float32, device=dev)
    bd = None if bias is None else bias.to(dev)
    if res is None:
        check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(xd), ptr(wp), ptr(bd), None, ptr(y), stream()), "fwd")
    else:
        rd = res.to(dev)
        check(lib.eben_conv1d_fwd_res(ctypes.byref(d), ptr(xd), ptr(wp), ptr(bd), ptr(rd), RES_SLOPE, ptr(y), stream()), "fwd_res")
    torch.cuda.synchronize()
    assert torch.isfinite(wp).all() and torch.isfinite(y).all()
    got = y.double().cpu()

    def epilogue(pre):
        t = pre if bias is None else pre + bias.double().reshape(1, -1, 1)
        t = F.leaky_relu(t, spec.out_slope) if spec.out_slope != 1.0 else t
        return t if res is None else t + F.leaky_relu(res.double(), RES_SLOPE)

    # ---- (a): the kernel's own operands ----
    w32 = v * scale.cpu().reshape(-1, 1, 1)                # the fp32 product gc_pack_kernel splits
    x32 = lrelu32(x, spec.in_slope)                        # the fp32 activation gc_kernel splits
    wq, xq = pieces(w32, np_), pieces(x32, np_)
    hi_lo, lo_hi = conv64(xq[1], wq[0], spec), conv64(xq[0], wq[1], spec)
    pre = sum(conv64(sum(xq[: np_ - q]), wq[q], spec) for q in range(np_))
    ref_a = epilogue(pre)
    err_a = max_rel(got, ref_a)

    # ---- (c): a dropped cross term shows on this data ----
    drop = min(max_rel(epilogue(pre - hi_lo), ref_a), max_rel(epilogue(pre - lo_hi), ref_a))

    # ---- (b): exact operands ----
    okw = {k: val for k, val in case.kw.items() if k not in ("c_in", "c_out", "ksize")}
    exact_pre = O.conv_layer(x.double(), v.double(), g.double(), None if bias is None else bias.double(), **{**okw, "out_slope": 1.0})
    exact = F.leaky_relu(exact_pre, spec.out_slope) + (0 if res is None else F.leaky_relu(res.double(), RES_SLOPE))
    if np_ == 3:
        err_b = max_rel(got, exact)
        bar_b = BAR_A
    else:
        w_exact = O.weight_norm(g.double(), v.double())
        mag = conv64(F.leaky_relu(x.double(), spec.in_slope).abs(), w_exact.abs(), spec)
        bound = PRODUCT_REL_X3 * mag + 3e-6 * exact_pre.abs().max()
        err_b = float(((got - exact).abs() / bound).max())   # fraction of the per-element bound
        bar_b = 1.0
    print(f"[gc] {name} gc_kernel{(form, rt, ct, np_)}: (a) {err_a:.3g}  (b) {err_b:.3g} of {bar_b:g}  (c) {drop / BAR_A:.3g} x bar")
    assert drop > 10 * BAR_A, f"{name}: a dropped cross term moves the reference by {drop:.3g} only"
    assert err_a < BAR_A, f"{name} (gc_kernel{(form, rt, ct, np_)}): {err_a:.3g} against float64 on the kernel's own piece products"
    assert err_b < bar_b, f"{name} (gc_kernel{(form, rt, ct, np_)}): {err_b:.3g} (bar {bar_b:g}) against float64 on the exact operands"
