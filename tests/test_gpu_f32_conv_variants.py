"""GPU: every launch of the fp32 variant table (tests/test_f32_conv_variants.py) through the C ABI, into NaN-filled outputs, against a
float64 torch.nn.functional conv of the same operands (these kernels multiply fp32: the operands are exact).  Before each launch the
case's instantiation is asserted through eben_conv1d_variant_f32, so a case that a retuned plan moved elsewhere fails by name
instead of passing on another kernel.

Launch forms (spread over the table: every instantiation sees one, every family all of them):
  fwd      eben_conv1d_fwd, bias, fused in_slope / out_slope (reflect padding in the launch where the layer has it)
  fwd_res  eben_conv1d_fwd_res, res_slope != 1
  dx       eben_conv1d_bwd_dx, the mask on load (out_slope != 1), accumulate = 1 into a non-zero dx, the reflect-fold workspace
  dx_res   eben_conv1d_bwd_dx_res, an addend before the input-activation mask and (reflect-padded layers) one after it
  dx_ex    eben_conv1d_bwd_dx_ex, res_rows < B and a seg_map that is not the identity
  dx_fm    eben_conv1d_bwd_dx_fm (thin only) against the expression of conv1d.hip's eben_conv1d_bwd_dx_fm in float64
ConvTranspose1d layers run fwd and dx (the autograd input gradient with a fused output activation: mask on load at tap direction 0).

Bound: max |got - ref| / max |ref| < 3e-5, the project's bound for fp32 conv kernels against fp64 (tests/test_gpu_ops.py).
Two bit-identity checks need no knob: every NP = 4 launch against the same layer on its first 2 batch items (NP = 1: thinconv.hip
keeps the FMA order per output), and the id_fast = 0 launch against the same layer at batch 8 (id_fast = 1).

[MI355X] worst error per family over the 55 cases: thin_kernel 5.3e-07, tap2_kernel 1.1e-06, tapconv_kernel 6.3e-07 (bound 3e-5); both
bit-identity checks exact.  With `n * BN` dropped from thin_kernel's LDS read the five NP = 4 cases fail and no other; with the
`cc % nxbuf` buffer rotation dropped from pack2_kernel's offset table the 17 tap2 cases with more than one input-tile buffer fail.
"""
import ctypes
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from formula import formula_tensor
from tests.test_f32_conv_variants import CASES, DX, FWD, ID_SLOW_CASE, ID_SLOW_SMALL_BATCH, NP4_CASES, TAP1, TAP2, THIN, answer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 3e-5
FAMILY = {TAP1: "tapconv_kernel", TAP2: "tap2_kernel", THIN: "thin_kernel"}
WORST = {}
# (in_slope, out_slope) of each form unless the case's own ConvSpec kwargs set them; dx forms take out_slope only with a mask on load
SLOPES = {"fwd": (0.3, 0.2), "fwd_res": (1.0, 0.2), "dx": (1.0, 0.2), "dx_res": (0.01, 0.2), "dx_ex": (1.0, 1.0), "dx_fm": (1.0, 1.0)}
RES_SLOPE, MASK_SLOPE = 0.3, 0.2
SEG_MAP = (0, 0, 0, 1)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def lin64(x, w, spec):
    """The layer's linear part in float64: zero or reflect padding and Conv1d, or ConvTranspose1d."""
    if spec.transposed:
        return F.conv_transpose1d(x, w, None, stride=spec.stride, padding=spec.pad_l, output_padding=spec.output_padding, groups=spec.groups,
                                  dilation=spec.dilation)
    xp = F.pad(x, (spec.pad_l, spec.pad_r), mode="reflect" if spec.reflect else "constant")
    return F.conv1d(xp, w, None, stride=spec.stride, dilation=spec.dilation, groups=spec.groups)


def adjoint64(g, w, spec, length):
    """Adjoint of lin64 by autograd (the input gradient, reflect fold included)."""
    xr = torch.zeros(g.shape[0], spec.c_in, length, dtype=torch.float64, requires_grad=True)
    lin64(xr, w, spec).mul(g).sum().backward()
    return xr.grad


def dlrelu(t, slope):
    return torch.where(t.double() > 0, 1.0, slope)


def case_spec(case):
    i, o = SLOPES[case.form]
    if case.direction == DX and not case.mask_on_load:
        o = 1.0
    return dataclasses.replace(case.spec(), in_slope=case.kw.get("in_slope", i), out_slope=case.kw.get("out_slope", o))


def seg_rows(batch):
    """eben_conv1d_bwd_dx_ex's mask row of every batch item for `seg` items per segment and SEG_MAP."""
    seg = -(-batch // 4)
    return seg, [SEG_MAP[b // seg] * seg + b % seg for b in range(batch)]


def operands(name, case, spec):
    """The CPU operands of the case's launch form and its float64 reference."""
    B, L, l_out = case.batch, case.length, spec.out_len(case.length)
    wshape = spec.weight_shape()
    v = formula_tensor(f"f32v/{name}/w", wshape, 1 / math.sqrt(wshape[1] * wshape[2]))
    scale = 1 + 0.3 * formula_tensor(f"f32v/{name}/s", (wshape[0],))
    w = v.double() * scale.double().reshape(-1, 1, 1)
    t = {"v": v, "scale": scale}
    xs, ys = (B, spec.c_in, L), (B, spec.c_out, l_out)
    if case.form in ("fwd", "fwd_res"):
        t["x"], t["bias"] = formula_tensor(f"f32v/{name}/x", xs), formula_tensor(f"f32v/{name}/b", (spec.c_out,), 0.1)
        ref = F.leaky_relu(lin64(F.leaky_relu(t["x"].double(), spec.in_slope), w, spec) + t["bias"].double().reshape(1, -1, 1), spec.out_slope)
        if case.form == "fwd_res":
            t["res"] = formula_tensor(f"f32v/{name}/r", ys, 0.5)
            ref = ref + F.leaky_relu(t["res"].double(), RES_SLOPE)
    elif case.form in ("dx", "dx_res"):
        t["dy"] = formula_tensor(f"f32v/{name}/dy", ys)
        masked = t["dy"].double()
        if spec.out_slope != 1.0:
            t["y"] = formula_tensor(f"f32v/{name}/y", ys)
            masked = masked * dlrelu(t["y"], spec.out_slope)
        ref = adjoint64(masked, w, spec, L)
        if case.form == "dx":
            t["dx0"] = formula_tensor(f"f32v/{name}/dx0", xs)
            ref = ref + t["dx0"].double()
        else:
            t["pre"], t["x"] = formula_tensor(f"f32v/{name}/pre", xs), formula_tensor(f"f32v/{name}/x", xs)
            ref = (ref + t["pre"].double()) * dlrelu(t["x"], spec.in_slope)
            if spec.reflect and not spec.transposed:   # an addend behind the mask is the fold pass's
                t["post"] = formula_tensor(f"f32v/{name}/post", xs)
                ref = ref + t["post"].double()
    else:
        t["g"] = formula_tensor(f"f32v/{name}/g", ys)
        ref = adjoint64(t["g"].double(), w, spec, L)
        seg, rows = seg_rows(B)
        t["act"] = formula_tensor(f"f32v/{name}/act", (2 * seg, spec.c_in, L))
        if case.form == "dx_ex":
            t["rows"] = (B + 1) // 2
            t["res"] = formula_tensor(f"f32v/{name}/res", (t["rows"], spec.c_in, L))
            ref[:t["rows"]] += t["res"].double()
        else:
            # conv1d.hip, eben_conv1d_bwd_dx_fm: rows b < fm_rows receive fm_gs (sgn(a - b) / s2 - s1 sgn(a) / s2^2) with a = the mask's
            # first fm_rows rows, b = the reference rows, (s1, s2) = (sum |a - b|, sum |a|); fm_gs sized so that the addend is O(1)
            assert B % 4 == 0
            a64, b64 = t["act"].double()[:seg], t["act"].double()[seg:]
            s1, s2 = (a64 - b64).abs().sum(), a64.abs().sum()
            t["gs"] = 0.25 * a64.numel()
            ref[:seg] += t["gs"] * (torch.sign(a64 - b64) / s2 - s1 * torch.sign(a64) / s2 ** 2)
        ref = ref * dlrelu(t["act"][rows], MASK_SLOPE)
    return t, ref


def launch(hip, case, spec, t, batch=None):
    """The case's launch on the first `batch` items of its operands (all of them by default); returns the output on the device."""
    from vibravox_amd._lib import check, ptr, stream

    B = batch or case.batch
    sub = B != case.batch
    L, l_out = case.length, spec.out_len(case.length)
    d = case.desc(spec, B)
    which = case.direction
    keep = {k: (x[:B] if k not in ("v", "scale", "bias", "act") else x).contiguous().to(DEV) for k, x in t.items() if torch.is_tensor(x)}
    p = lambda k: ptr(keep[k]) if k in keep else None   # noqa: E731
    wp = torch.empty(hip.eben_conv1d_packed_floats(ctypes.byref(d), which), dtype=torch.float32, device=DEV)
    check(hip.eben_conv1d_pack(ctypes.byref(d), p("v"), p("scale"), ptr(wp) if which == 0 else None, ptr(wp) if which == 1 else None, stream()), "pack")
    shape = (B, spec.c_out, l_out) if which == FWD else (B, spec.c_in, L)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    ws_bytes = hip.eben_conv1d_bwd_dx_workspace(ctypes.byref(d)) if which == DX else 0
    ws = torch.full((max(1, ws_bytes // 4),), float("nan"), dtype=torch.float32, device=DEV)
    if case.form == "fwd":
        check(hip.eben_conv1d_fwd(ctypes.byref(d), p("x"), ptr(wp), p("bias"), None, ptr(out), stream()), "fwd")
    elif case.form == "fwd_res":
        check(hip.eben_conv1d_fwd_res(ctypes.byref(d), p("x"), ptr(wp), p("bias"), p("res"), RES_SLOPE, ptr(out), stream()), "fwd_res")
    elif case.form == "dx":
        out = keep["dx0"].clone()
        check(hip.eben_conv1d_bwd_dx(ctypes.byref(d), p("dy"), p("y"), ptr(wp), None, ptr(out), 1, ptr(ws), ws_bytes, stream()), "bwd_dx")
    elif case.form == "dx_res":
        check(hip.eben_conv1d_bwd_dx_res(ctypes.byref(d), p("dy"), p("y"), ptr(wp), p("x"), p("pre"), p("post"), ptr(out), ptr(ws), ws_bytes,
                                         stream()), "bwd_dx_res")
    else:
        # the first items of a launch keep their own mask rows and (dx_ex) their residual rows: the short launch names them directly
        seg, _ = seg_rows(case.batch)
        assert not sub or B <= seg
        act = keep["act"][:B].contiguous() if sub else keep["act"]
        seg_arg, seg_map = (0, None) if sub else (seg, (ctypes.c_int * 4)(*SEG_MAP))
        if case.form == "dx_ex":
            rows = min(t["rows"], B)
            check(hip.eben_conv1d_bwd_dx_ex(ctypes.byref(d), p("g"), ptr(wp), p("res"), rows, ptr(act), MASK_SLOPE, seg_arg, seg_map, ptr(out),
                                            stream()), "bwd_dx_ex")
        else:
            assert not sub
            a, b = keep["act"][:seg], keep["act"][seg:]
            sums = torch.stack(((a - b).abs().sum(), a.abs().sum())).to(torch.float32).contiguous()
            check(hip.eben_conv1d_bwd_dx_fm(ctypes.byref(d), p("g"), ptr(wp), ptr(b), seg, ptr(sums), t["gs"], ptr(act), MASK_SLOPE, seg_arg, seg_map,
                                            ptr(out), stream()), "bwd_dx_fm")
    torch.cuda.synchronize()
    return out


def assert_variant(hip, name, case, batch=None):
    v = answer(hip, case, batch=batch)
    if batch is None:
        assert (v[0], v[1:]) == (case.route, case.expect), f"{name}: runs {FAMILY.get(v[0], v[0])}{v[1:]}, the case is written for {case.expect}"
    return v


@pytest.mark.parametrize("name", list(CASES))
def test_f32_instantiation_against_float64(hip, name):
    case = CASES[name]
    spec = case_spec(case)
    v = assert_variant(hip, name, case)
    t, ref = operands(name, case, spec)
    got = launch(hip, case, spec, t)
    err = rel_err(got, ref)
    WORST[case.route] = max(WORST.get(case.route, 0.0), err)
    print(f"[f32 variants] {name} ({FAMILY[case.route]}{v[1:]}): error {err:.3g} against float64; worst so far "
          + ", ".join(f"{FAMILY[r]} {e:.3g}" for r, e in sorted(WORST.items())))
    assert err < TOL, f"{name} ({FAMILY[case.route]}{v[1:]}): error {err:.3g} against float64"
    # bit identity of the first items with a launch that takes the other path: NP = 1 instead of 4, id_fast = 1 instead of 0
    small = 2 if name in NP4_CASES else ID_SLOW_SMALL_BATCH if name == ID_SLOW_CASE else 0
    if small:
        u = assert_variant(hip, name, case, batch=small)
        assert u[:3] == v[:3] and (u[3], u[4]) == ((1, 1) if name in NP4_CASES else (v[3], 1)), (name, u)
        assert (v[3], v[4]) == ((4, 1) if name in NP4_CASES else (1, 0)), (name, v)
        again = launch(hip, case, spec, t, batch=small)
        assert torch.equal(again, got[:small]), f"{name}: {FAMILY[case.route]}{u[1:]} on {small} items differs from {v[1:]} in bits"
