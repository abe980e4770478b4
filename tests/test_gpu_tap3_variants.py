"""GPU: every launch of the variant table (tests/test_tap3_variants.py) through the C ABI against a float64 conv of exactly the
operands the MFMAs multiply.  Before each launch the case's instantiation is asserted through eben_conv1d_variant, so a case that a
retuned plan moved elsewhere fails by name instead of passing on another kernel.

Bounds (max |got - ref| / max |ref|) and reference operands are those of the existing test of each mode:
  EBEN_MATH_BF16    bf16 (RNE) x and w                3e-5   (test_bf16_math_forward_and_batched_input_gradient)
  ... bundle layout bf16 x and w                      2e-5 forward, 3e-5 input gradient   (test_bundle_conv_forward / _input_gradient)
  EBEN_MATH_BF16X2  exact x, bf16 w                   3e-5   (test_bf16x2_math_keeps_the_activation_operand)
  EBEN_MATH_BF16X3  exact x and w                     1e-4   (test_split_bf16_math_forward_and_batched_input_gradient)
  ... bundle layout hi + lo planes of x and of w       3e-5   (test_bundle_conv_forward)
  EBEN_MATH_BF16X6  exact x and w                     3e-5
  bl_dw weight gradients: bf16 operands               1e-4
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from formula import formula_tensor
from tests.test_tap3_variants import BF16, BF16X2, BF16X3, BF16X6, BL, CASES, DW_CASES, DX, FWD, TAP3, dw_variant, variant
from vibravox_amd.ops import CONV_ROUTE_TAP3

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = {BF16: 3e-5, BF16X2: 3e-5, BF16X3: 1e-4, BF16X6: 3e-5}
TOL_BL = {(BF16, FWD): 2e-5, (BF16, DX): 3e-5, (BF16X3, FWD): 3e-5}


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def hilo(t):
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi.double() + (t - hi).to(torch.bfloat16).double()


def conv_t(g, w, spec, length):
    """Adjoint of the forward conv in float64 (the input gradient), output cut / padded to `length`."""
    l_out = g.shape[-1]
    op = length - ((l_out - 1) * spec.stride - spec.pad_l - spec.pad_r + spec.dilation * (spec.ksize - 1) + 1)
    xr = torch.zeros(g.shape[0], spec.c_in, length, dtype=torch.float64, requires_grad=True)
    F.conv1d(F.pad(xr, (spec.pad_l, spec.pad_r)), w, stride=spec.stride, dilation=spec.dilation, groups=spec.groups).mul(g).sum().backward()
    assert op >= 0
    return xr.grad


def conv(x, w, spec, bias=None):
    return F.conv1d(F.pad(x, (spec.pad_l, spec.pad_r)), w, bias, stride=spec.stride, dilation=spec.dilation, groups=spec.groups)


def assert_variant(lib, name, case):
    rc, v = variant(lib, case)
    assert rc == 0, (name, lib.eben_last_error())
    assert v[0] == CONV_ROUTE_TAP3 and v[7] == TAP3, (name, v)
    assert v[1:7] == case.expect, f"{name}: runs tap3_kernel{v[1:7]}, the case is written for {case.expect}"
    return v[1:7]


def _plain(hip, name, case):
    import dataclasses

    from vibravox_amd import ops
    from vibravox_amd._lib import check, ptr, stream

    slope = 0.2
    spec = dataclasses.replace(case.spec(), out_slope=slope if (case.direction == FWD or case.mask_on_load) else 1.0)
    d = case.desc(spec)
    fm, xrb, im, npw, npx, bl = assert_variant(hip, name, case)
    B, L, l_out = case.batch, case.length, spec.out_len(case.length)
    wshape = spec.weight_shape()
    w = formula_tensor(f"t3v/{name}/w", wshape, 1 / math.sqrt(wshape[1] * wshape[2]))
    wd = w.to(DEV)
    mm = case.math
    # the operands the MFMAs multiply: bf16 pieces of the exact values (split forms: every piece, i.e. the exact value)
    rw = bf if mm in (BF16, BF16X2) else (lambda t: t.double())
    ra = bf if mm == BF16 or (mm == BF16X2 and case.direction == DX) else (lambda t: t.double())
    which = case.direction
    wp = torch.empty(hip.eben_conv1d_packed_floats(ctypes.byref(d), which), dtype=torch.float32, device=DEV)
    check(hip.eben_conv1d_pack(ctypes.byref(d), ptr(wd), None, ptr(wp) if which == 0 else None, ptr(wp) if which == 1 else None, stream()), "pack")
    if which == FWD:
        x = formula_tensor(f"t3v/{name}/x", (B, spec.c_in, L))
        bias = formula_tensor(f"t3v/{name}/b", (spec.c_out,), 0.1)
        res = formula_tensor(f"t3v/{name}/r", (B, spec.c_out, l_out), 0.5)
        xd, bd, rd = x.to(DEV), bias.to(DEV), res.to(DEV)
        y = torch.full((B, spec.c_out, l_out), float("nan"), dtype=torch.float32, device=DEV)
        check(hip.eben_conv1d_fwd(ctypes.byref(d), ptr(xd), ptr(wp), ptr(bd), ptr(rd), ptr(y), stream()), "fwd")
        ref = F.leaky_relu(conv(ra(x), rw(w), spec, bias.double()), slope) + res.double()
        got = y
    elif case.mask_on_load:
        # autograd's input gradient: dy * lrelu'(y) formed as dy is staged, rounded after the mask; accumulate into a non-zero dx
        # on the even tile heights
        accumulate = 1 if fm % 2 == 0 else 0
        dy = formula_tensor(f"t3v/{name}/dy", (B, spec.c_out, l_out))
        yv = formula_tensor(f"t3v/{name}/y", (B, spec.c_out, l_out))
        dx0 = formula_tensor(f"t3v/{name}/dx0", (B, spec.c_in, L))
        dyd, yd = dy.to(DEV), yv.to(DEV)
        got = dx0.to(DEV).clone()
        check(hip.eben_conv1d_bwd_dx(ctypes.byref(d), ptr(dyd), ptr(yd), ptr(wp), None, ptr(got), accumulate, None, 0, stream()), "bwd_dx")
        masked = dy.double() * torch.where(yv.double() > 0, 1.0, slope)
        ref = conv_t(ra(masked), rw(w), spec, L) + (dx0.double() if accumulate else 0.0)
    else:
        # the batched input gradient's epilogue: + residual on the first rows, x lrelu'(activation)
        g = formula_tensor(f"t3v/{name}/g", (B, spec.c_out, l_out))
        rows = (B + 1) // 2
        res = formula_tensor(f"t3v/{name}/res", (rows, spec.c_in, L))
        act = formula_tensor(f"t3v/{name}/act", (B, spec.c_in, L))
        gd, rd, ad = g.to(DEV), res.to(DEV), act.to(DEV)
        got = torch.full((B, spec.c_in, L), float("nan"), dtype=torch.float32, device=DEV)
        check(hip.eben_conv1d_bwd_dx_ex(ctypes.byref(d), ptr(gd), ptr(wp), ptr(rd), rows, ptr(ad), slope, 0, None, ptr(got), stream()), "bwd_dx_ex")
        ref = conv_t(ra(g), rw(w), spec, L)
        ref[:rows] += res.double()
        ref = ref * torch.where(act.double() > 0, 1.0, slope)
    torch.cuda.synchronize()
    err = rel_err(got, ref)
    assert err < TOL[mm], f"{name} (tap3_kernel{(fm, xrb, im, npw, npx, bl)}): error {err:.3g} against float64"


def _bundle(hip, name, case):
    import dataclasses

    from vibravox_amd import ops
    from vibravox_amd._lib import check
    from vibravox_amd.disc_engine_bl import Planes

    slope = 0.2
    spec = dataclasses.replace(case.spec(), out_slope=slope if case.direction == FWD else 1.0)
    d = case.desc(spec)
    fm, xrb, im, npw, npx, bl = assert_variant(hip, name, case)
    B, L, l_out = case.batch, case.length, spec.out_len(case.length)
    wshape = spec.weight_shape()
    v = formula_tensor(f"t3v/{name}/w", wshape, 1 / math.sqrt(wshape[1] * wshape[2])).to(DEV)
    scale = (1 + 0.3 * formula_tensor(f"t3v/{name}/s", (wshape[0],))).to(DEV)
    w = (v * scale.reshape(-1, 1, 1)).cpu()
    which = case.direction
    wp = torch.empty(hip.eben_conv1d_packed_floats(ctypes.byref(d), which), dtype=torch.float32, device=DEV)
    ops.conv1d_pack(d, v, scale, wp if which == 0 else None, wp if which == 1 else None)
    st = torch.cuda.current_stream().cuda_stream
    x3 = case.math == BF16X3
    if which == FWD:
        x = formula_tensor(f"t3v/{name}/x", (B, spec.c_in, L))
        xp = Planes.from_f32(x.to(DEV), True)
        bias = formula_tensor(f"t3v/{name}/b", (spec.c_out,), 0.1).to(DEV)
        y = Planes(B, spec.c_out, l_out, DEV)
        check(hip.eben_bl_conv1d_fwd(ctypes.byref(d), xp.hi.data_ptr(), xp.lo.data_ptr() if x3 else None, wp.data_ptr(), bias.data_ptr(),
                                     y.hi.data_ptr(), y.lo.data_ptr(), st), "bl_conv1d_fwd")
        xin, wq = (xp.to_f32().cpu().double(), hilo(w)) if x3 else (bf(x), bf(w))
        ref = F.leaky_relu(conv(xin, wq, spec, bias.cpu().double()), slope)
        got = y.to_f32()
    else:
        assert not x3, "eben_bl_conv1d_bwd_dx takes one gradient plane"
        g = formula_tensor(f"t3v/{name}/g", (B, spec.c_out, l_out))
        gp = Planes.from_f32(g.to(DEV), False)
        act = Planes.from_f32(formula_tensor(f"t3v/{name}/act", (B, spec.c_in, L)).to(DEV), True)
        dx = Planes(B, spec.c_in, L, DEV)
        check(hip.eben_bl_conv1d_bwd_dx(ctypes.byref(d), gp.hi.data_ptr(), wp.data_ptr(), act.hi.data_ptr(), act.lo.data_ptr(), slope, 0, None, 0, 0,
                                        None, 0.0, dx.hi.data_ptr(), dx.lo.data_ptr(), st), "bl_conv1d_bwd_dx")
        a_hi = act.hi.permute(0, 1, 3, 2).reshape(B, spec.c_in, L).double().cpu()
        ref = conv_t(bf(g), bf(w), spec, L) * torch.where(a_hi > 0, 1.0, slope)
        got = dx.to_f32()
    torch.cuda.synchronize()
    err = rel_err(got, ref)
    assert err < TOL_BL[(case.math, which)], f"{name} (tap3_kernel{(fm, xrb, im, npw, npx, bl)}): error {err:.3g} against float64"


@pytest.mark.parametrize("name", list(CASES))
def test_tap3_instantiation_against_float64(hip, name):
    case = CASES[name]
    assert not case.env, "cases with knobs run in a child process"
    (_bundle if case.layout == BL else _plain)(hip, name, case)


def _dw_setup(name, case):
    from vibravox_amd.disc_engine_bl import Planes

    spec = case.spec()
    l_out = spec.out_len(case.length)
    dy = formula_tensor(f"t3v/{name}/dy", (case.batch, spec.c_out, l_out))
    x = formula_tensor(f"t3v/{name}/xw", (case.batch, spec.c_in, case.length))
    return spec, dy, x, Planes.from_f32(dy.to(DEV), False), Planes.from_f32(x.to(DEV), False)


def _dw_reduce(hip, d, slabs, spec):
    from vibravox_amd import ops

    nslab, rs, perm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    hip.eben_bl_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(rs), ctypes.byref(perm))
    wshape = spec.weight_shape()
    dv, dbias = torch.empty(wshape, dtype=torch.float32, device=DEV), torch.empty(wshape[0], dtype=torch.float32, device=DEV)
    ops.wn_bwd_multi([ops.wn_job(slabs, nslab.value, rs.value, dv, None, None, (dv, None, dbias), col_perm_k=perm.value)])
    return dv, dbias


@pytest.mark.parametrize("name", list(DW_CASES))
def test_bl_dw_instantiation_against_float64(hip, name):
    """eben_bl_conv1d_bwd_dw and, for the problems it groups, eben_bl_conv1d_bwd_dw_multi (bl_dw_multi_kernel) on two copies of the
    problem: both against float64 on the bf16 operands."""
    from vibravox_amd._lib import check

    case = DW_CASES[name]
    rc, v = dw_variant(hip, case)
    assert rc == 0 and v == case.expect, f"{name}: runs bl_dw {v}, the case is written for {case.expect}"
    spec, dy, x, dyp, xp = _dw_setup(name, case)
    d = case.desc()
    nbytes = hip.eben_bl_conv1d_bwd_dw_workspace(ctypes.byref(d), None, None, None)
    st = torch.cuda.current_stream().cuda_stream
    wshape = spec.weight_shape()
    wr = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(wshape[0], dtype=torch.float64, requires_grad=True)
    (conv(bf(x), wr, spec, br) * bf(dy)).sum().backward()
    outs = []
    slabs = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    check(hip.eben_bl_conv1d_bwd_dw(ctypes.byref(d), dyp.hi.data_ptr(), xp.hi.data_ptr(), 1, slabs.data_ptr(), nbytes, st), "bl_conv1d_bwd_dw")
    outs.append(_dw_reduce(hip, d, slabs, spec))
    # the same problem twice through _multi: grouped into one bl_dw_multi_kernel launch, or two launches of its own
    k = 2
    descs = (ctypes.POINTER(type(d)) * k)(ctypes.pointer(d), ctypes.pointer(d))
    many = [torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(k)]
    dys, xs = (ctypes.c_void_p * k)(*[dyp.hi.data_ptr()] * k), (ctypes.c_void_p * k)(*[xp.hi.data_ptr()] * k)
    sl, nbs = (ctypes.c_void_p * k)(*[m.data_ptr() for m in many]), (ctypes.c_size_t * k)(*[nbytes] * k)
    check(hip.eben_bl_conv1d_bwd_dw_multi(descs, dys, xs, 1, sl, nbs, k, st), "bl_conv1d_bwd_dw_multi")
    outs += [_dw_reduce(hip, d, m, spec) for m in many]
    torch.cuda.synchronize()
    for i, (dv, dbias) in enumerate(outs):
        assert rel_err(dv, wr.grad) < 1e-4, (name, i, rel_err(dv, wr.grad))
        assert rel_err(dbias, br.grad) < 1e-4, (name, i)
