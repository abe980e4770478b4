"""GPU: every launch of the ResidualUnit variant table (tests/test_ru_variants.py) through the C ABI against float64.  Before a case
is compared, the instantiation and geometry it ran with are asserted through eben_ru_variant (asked in the process that launched), so a
case that a retuned plan moved elsewhere fails by name instead of passing on another kernel.

Buffers: every output lies between two guards of 64 elements filled with a sentinel that must survive the launch (the fp32 tensors, the
bf16 bundle planes and the sign bytes alike) and is prefilled with NaN (the sign plane with 0xAA) so that a column nobody wrote shows;
cases with offset 1 place every fp32 operand one float past a 16-byte boundary (the scalar staging paths).

Bounds (max |got - ref| / max |ref|):
  * forward (y, h, u) and input gradient (g_x, g_h) against float64 of the weight-normalised unit / its autograd: RU_TOL[math] of
    tests/test_gpu_ops.py (3e-5 exact fp32 and three pieces, 1e-4 two pieces, 2e-2 one piece);
  * EBEN_MATH_BF16 (one piece) also against float64 ON THE OPERANDS THE KERNEL MULTIPLIES, at the fp32-accumulation bound RU_TOL[0]: the
    weights are bf16 (RNE) of the fp32 product v * scale (rs_pack_bf16 in the pack kernels), the first stage's activations bf16 of the fp32
    lrelu(x) / g_y lrelu'(u), the second stage's bf16 of the kernel's OWN fp32 h / g_h output (ru3_fwd_kernel splits its stage-1
    accumulators, ru3_bwd_kernel the g_h it wrote back to LDS: the values it stores).  Every operand's rounding can be rebuilt from the
    tensors the kernels write, so no stage keeps RU_TOL[1] here; this is the check that sees a dropped or doubled tap at an edge column.
    For eben_rubl_bwd the g_h plane is bf16 already (the operand itself); its stage A is checked on the fp32 g_h of eben_ru_bwd_ex, to
    which the plane must be bit-identical;
  * weight-gradient slab sums against the float64 contraction of the same operands: 2e-6 (bf16 operands: exact products, fp32
    accumulation), 3e-5 for three pieces; for every third case dv / dg through eben_wn_bwd against float64 autograd at 2 RU_TOL
    (4e-2 for the bundle kernels) -- the bounds of test_fused_residual_unit_weight_gradients / test_bundle_layout_residual_unit.

Measured on an MI355X at 128 channels: one piece against float64 4e-3 (forward), 3e-3 (input gradient); on the kernel's operands 3e-7 and
2e-7; slab sums 3e-7; dv / dg 3.5e-3.  A left-fold source column shifted by one in ru3_bwd_kernel puts g_x of every one-piece case
0.10 .. 0.37 off in both comparisons.

Cases with knobs run in one child process per knob set (the knobs are read once per process): the child performs only the launches and
writes what they produced to a file; the references and every comparison stay here.  A child that fails fails its cases; nothing retries.
"""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from formula import formula_tensor
from tests.test_gpu_ops import RU_TOL, _from_bundles, _sign_plane, _to_bundles
from tests.test_ru_variants import BF16, BF16X3, BF16X6, BL_BWD, BL_DW, BL_FWD, BWD, CASES, DW, F32, FWD, KNOBS, N_OUT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = {torch.float32: 1234.5, torch.bfloat16: 7.0, torch.uint8: 0x5C}
UNWRITTEN = {torch.float32: float("nan"), torch.bfloat16: float("nan"), torch.uint8: 0xAA}
OUT_SLOPE = 0.01
DW_CASES = [n for n, c in CASES.items() if c.op in (DW, BL_DW)]
WN_CASES = set(DW_CASES[::3])   # the cases that also go through eben_wn_bwd


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), "shape mismatch or a value nobody wrote"
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


# ---- inputs and the float64 unit (CPU) -------------------------------------------------------------------------------------------
_weights = {}


def weights(c):
    """Directions and gains of the two weight-normalised convs, g != ||v||."""
    if c not in _weights:
        vd = formula_tensor(f"ruv/{c}/vd", (c, c, 3), 1 / math.sqrt(3 * c))
        vp = formula_tensor(f"ruv/{c}/vp", (c, c, 1), 1 / math.sqrt(c))
        gd = vd.reshape(c, -1).norm(dim=1).reshape(c, 1, 1) * (1 + 0.3 * formula_tensor(f"ruv/{c}/gd", (c, 1, 1)))
        gp = vp.reshape(c, -1).norm(dim=1).reshape(c, 1, 1) * (1 + 0.3 * formula_tensor(f"ruv/{c}/gp", (c, 1, 1)))
        _weights[c] = dict(vd=vd, vp=vp, gd=gd, gp=gp)
    return _weights[c]


_refs = {}


def unit_ref(case):
    """float64 forward and autograd of the unit on the case's inputs; shared by the cases of one (channels, dilation, length, batch, slope)."""
    c, d, L, B = case.channels, case.dilation, case.length, case.batch
    key = (c, d, L, B, case.slope)
    if key in _refs:
        return _refs[key]
    w = weights(c)
    x = formula_tensor(f"ruv/{c}/{d}/{L}/{B}/x", (B, c, L))
    gy = formula_tensor(f"ruv/{c}/{d}/{L}/{B}/gy", (B, c, L))
    pt = formula_tensor(f"ruv/{c}/{d}/{L}/{B}/post", (B, c, L))
    rvd, rvp, rgd, rgp = (w[k].double().requires_grad_(True) for k in ("vd", "vp", "gd", "gp"))
    wd = rvd * (rgd / rvd.flatten(1).norm(dim=1).reshape(c, 1, 1))
    wp = rvp * (rgp / rvp.flatten(1).norm(dim=1).reshape(c, 1, 1))
    xr = x.double().requires_grad_(True)
    xin = F.leaky_relu(xr, case.slope)
    h = F.conv1d(F.pad(xin, (d, d), mode="reflect"), wd, dilation=d)
    h.retain_grad()
    u = F.leaky_relu(F.conv1d(h, wp), OUT_SLOPE)
    ((xin + u) * gy.double()).sum().backward()
    r = dict(x=x, gy=gy, post=pt, xin=xin.detach(), h=h.detach(), u=u.detach(), y=(xin + u).detach(), gh=h.grad, gx=xr.grad,
             dvd=rvd.grad, dvp=rvp.grad, dgd=rgd.grad, dgp=rgp.grad)
    # what the backward launches are given of the forward: fp32 copies of the float64 tensors
    r["u32"], r["h32"], r["gh32"] = r["u"].float(), r["h"].float(), r["gh"].float()
    if len(_refs) > 64:
        _refs.clear()
    _refs[key] = r
    return r


def launch_inputs(case):
    """The fp32 tensors a case's launches read (CPU): what a child process is handed."""
    r = unit_ref(case)
    keys = {FWD: ("x",), BL_FWD: ("x",), BWD: ("x", "gy", "post", "u32"), BL_BWD: ("x", "gy", "post", "u32"),
            DW: ("x", "gy", "u32", "h32", "gh32"), BL_DW: ("x", "gy", "u32", "h32", "gh32")}[case.op]
    return {k: r[k] for k in keys}


# ---- the launches (this process or a child) ---------------------------------------------------------------------------------------
def guarded(shape, dtype, dev, offset=0):
    """A tensor of `shape` prefilled as unwritten, `offset` elements past a 16-byte boundary, between two sentinel guards."""
    n = int(math.prod(shape))
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
    view = buf[GUARD + offset: GUARD + offset + n].view(shape)
    view.fill_(UNWRITTEN[dtype])
    assert view.data_ptr() % 16 == (offset * view.element_size()) % 16
    return buf, view


def guards_intact(buf, view, offset):
    n = view.numel()
    s = SENTINEL[buf.dtype]
    return bool((buf[:GUARD + offset] == s).all()) and bool((buf[GUARD + offset + n:] == s).all())


def placed(t, dev, offset):
    buf = torch.empty(GUARD + offset + t.numel(), dtype=t.dtype, device=dev)
    view = buf[GUARD + offset:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * 4) % 16
    return view


class Device:
    """Per process: the weight-norm scales and the packed images of each channel count."""

    def __init__(self, lib):
        self.lib, self.dev, self.w, self.img = lib, torch.device("cuda"), {}, {}

    def scales(self, c):
        from vibravox_amd._lib import check, ptr, stream

        if c not in self.w:
            w = {k: v.to(self.dev) for k, v in weights(c).items()}
            for key, cols in (("d", 3 * c), ("p", c)):
                w["s" + key], w["n" + key] = torch.empty(c, device=self.dev), torch.empty(c, device=self.dev)
                check(self.lib.eben_wn_scale(ptr(w["g" + key]), ptr(w["v" + key]), c, cols, ptr(w["s" + key]), ptr(w["n" + key]), stream()), "wn_scale")
            self.w[c] = w
        return self.w[c]

    def image(self, c, mm, which):
        from vibravox_amd._lib import check, ptr, stream

        if (c, mm, which) not in self.img:
            w = self.scales(c)
            img = torch.empty(self.lib.eben_ru_packed_floats_ex(c, mm), dtype=torch.float32, device=self.dev)
            check(self.lib.eben_ru_pack_ex(c, mm, which, ptr(w["vd"]), ptr(w["sd"]), ptr(w["vp"]), ptr(w["sp"]), ptr(img), stream()), "ru_pack_ex")
            self.img[(c, mm, which)] = img
        return self.img[(c, mm, which)]


def run_case(D, case, inp):
    """Only launches: returns what they wrote (CPU tensors), whether every guard survived, and what eben_ru_variant says here."""
    from vibravox_amd._lib import check, stream

    lib, dev = D.lib, D.dev
    c, d, L, B, off, mm = case.channels, case.dilation, case.length, case.batch, case.offset, case.math
    vout = (ctypes.c_int * N_OUT)()
    rc = lib.eben_ru_variant(case.op, mm, B, c, L, d, vout, N_OUT)
    out = {"variant": (rc, tuple(vout))}
    w = D.scales(c)
    out["sd"], out["sp"] = w["sd"].cpu(), w["sp"].cpu()
    st = stream()
    shape = (B, c, L)
    held, held_in = {}, []

    def new(name, dtype=torch.float32, shp=shape, offset=off):
        held[name] = guarded(shp, dtype, dev, offset if dtype is torch.float32 else 0) + (offset if dtype is torch.float32 else 0,)
        return held[name][1].data_ptr()

    def fin(name):
        held_in.append(placed(inp[name], dev, off))   # kept alive until the launches are done
        return held_in[-1]

    x = fin("x")
    xp = x.data_ptr() if case.slope != 1.0 else None
    plane = (B, c // 8, L, 8)
    if case.op == FWD:
        check(lib.eben_ru_fwd_ex(mm, B, c, L, d, x.data_ptr(), case.slope, OUT_SLOPE, D.image(c, mm, 0).data_ptr(), new("y"), new("h"), new("u"), st), "ru_fwd_ex")
    elif case.op == BL_FWD:
        img = D.image(c, mm, 0).data_ptr()
        check(lib.eben_ru_fwd_ex(mm, B, c, L, d, x.data_ptr(), case.slope, OUT_SLOPE, img, new("y0"), new("h0"), new("u0"), st), "ru_fwd_ex")
        check(lib.eben_rubl_fwd(mm, B, c, L, d, x.data_ptr(), case.slope, OUT_SLOPE, img, new("y"), new("xb", torch.bfloat16, plane),
                                new("hb", torch.bfloat16, plane), new("um", torch.uint8, (B, c // 8, L)), st), "rubl_fwd")
    elif case.op in (BWD, BL_BWD):
        gy, u32 = fin("gy"), fin("u32")
        post = fin("post").data_ptr() if case.post else None
        m1 = BF16 if case.op == BL_BWD else mm
        img = D.image(c, m1, 1).data_ptr()
        check(lib.eben_ru_bwd_ex(m1, B, c, L, d, gy.data_ptr(), u32.data_ptr(), OUT_SLOPE, xp, case.slope, post, img, new("gx"), new("gh"), st), "ru_bwd_ex")
        if case.op == BL_BWD:
            um = _sign_plane(u32.contiguous())
            check(lib.eben_rubl_bwd(B, c, L, d, gy.data_ptr(), um.data_ptr(), OUT_SLOPE, xp, case.slope, post, img, new("gx1"),
                                    new("gzb", torch.bfloat16, plane), new("ghb", torch.bfloat16, plane), st), "rubl_bwd")
    else:
        nslab = (lib.eben_ru_dw_slabs if case.op == DW else lib.eben_rubl_dw_slabs)(B, c, L)
        out["nslab"] = nslab
        assert 0 < nslab <= 4096
        if case.op == DW:
            gy, u32, h32, gh32 = fin("gy"), fin("u32"), fin("h32"), fin("gh32")
            check(lib.eben_ru_dw(mm, B, c, L, d, gy.data_ptr(), u32.data_ptr(), OUT_SLOPE, h32.data_ptr(), gh32.data_ptr(), x.data_ptr(), case.slope,
                                 new("slab_p", shp=(nslab, c, c)), new("slab_d", shp=(nslab, c, c, 3)), st), "ru_dw")
        else:
            gy, u32, h32, gh32 = (inp[k].to(dev) for k in ("gy", "u32", "h32", "gh32"))
            planes = [_to_bundles(t) for t in (gy * torch.where(u32 > 0, 1.0, OUT_SLOPE), h32, gh32, F.leaky_relu(inp["x"].to(dev), case.slope))]
            out["planes"] = [p.cpu() for p in planes]
            check(lib.eben_rubl_dw(B, c, L, d, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(),
                                   new("slab_p", shp=(nslab, c, c)), new("slab_d", shp=(nslab, c, c, 3)), st), "rubl_dw")
        torch.cuda.synchronize()
        if case.name in WN_CASES:   # eben_wn_bwd sums the slabs in place: on aligned copies, after the slabs themselves are kept
            for key, cols in (("p", c), ("d", 3 * c)):
                slabs = held["slab_" + key][1].clone()
                dv, dg = torch.empty_like(w["v" + key]), torch.empty_like(w["g" + key])
                check(lib.eben_wn_bwd(slabs.data_ptr(), nslab, c * cols, c, cols, cols, w["g" + key].data_ptr(), w["v" + key].data_ptr(),
                                      w["n" + key].data_ptr(), dg.data_ptr(), dv.data_ptr(), None, st), "wn_bwd")
                out["dv" + key], out["dg" + key] = dv.cpu(), dg.cpu()
    torch.cuda.synchronize()
    out["guards"] = {k: guards_intact(buf, view, o) for k, (buf, view, o) in held.items()}
    for k, (buf, view, o) in held.items():
        out[k] = view.cpu().clone()
    return out


def child_main(path_in, path_out):
    """Entry of a knob set's child process: the launches of every case in `path_in`, their outputs to `path_out`."""
    from vibravox_amd import _lib

    D = Device(_lib.load())
    todo = torch.load(path_in)
    torch.save({name: run_case(D, CASES[name], inp) for name, inp in todo.items()}, path_out)


_CHILD = ("import sys; sys.path[:0] = [%r, %r]\n"
          "import tests.test_gpu_ru_variants as m\n"
          "m.child_main(sys.argv[1], sys.argv[2])\n" % (ROOT, os.path.join(ROOT, "tests", "golden")))
_children = {}


def child_outputs(knobs):
    """The outputs of every case of one knob set, from ONE child process started once (a failure is kept, not retried)."""
    if knobs not in _children:
        _children[knobs] = None
        names = [n for n, c in CASES.items() if c.knobs == knobs]
        with tempfile.TemporaryDirectory() as td:
            pin, pout = os.path.join(td, "in.pt"), os.path.join(td, "out.pt")
            torch.save({n: launch_inputs(CASES[n]) for n in names}, pin)
            r = subprocess.run([sys.executable, "-c", _CHILD, pin, pout], env={**os.environ, **KNOBS[knobs]}, timeout=300, capture_output=True, text=True)
            assert r.returncode == 0, f"child of knob set {knobs} exited with {r.returncode}: {r.stderr[-3000:]}"
            _children[knobs] = torch.load(pout)
    assert _children[knobs] is not None, f"the child process of knob set {knobs} failed earlier"
    return _children[knobs]


_device = []


def outputs_of(hip, case):
    if case.knobs:
        return child_outputs(case.knobs)[case.name]
    if not _device:
        _device.append(Device(hip))
    return run_case(_device[0], case, launch_inputs(case))


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------
def effective_weights(case, out):
    """fp32 v * scale as the pack kernels form it (scale = the device's g / ||v||)."""
    w = weights(case.channels)
    return w["vd"] * out["sd"].reshape(-1, 1, 1), w["vp"] * out["sp"].reshape(-1, 1, 1)


def assert_errors(case, rows):
    """rows of (tensor name, what it is compared with, error, bound): every figure is printed before the first one is asserted."""
    for k, what, err, bound in rows:
        print(f"{case.name}: {k} {err:.3g} against {what} (bound {bound})")
    for k, what, err, bound in rows:
        assert err < bound, (case.name, k, what, err, bound)


def check_forward(case, out, r, mm):
    got = {k: out[k if case.op == FWD else k + "0"] for k in ("y", "h", "u")}
    rows = [(k, "float64", rel_err(got[k], r[k]), RU_TOL[mm]) for k in ("y", "h", "u")]
    if mm == BF16:
        wd32, wp32 = effective_weights(case, out)
        d = case.dilation
        xin32 = F.leaky_relu(r["x"], case.slope)
        h_same = F.conv1d(F.pad(bf(xin32), (d, d), mode="reflect"), bf(wd32), dilation=d)
        u_same = F.leaky_relu(F.conv1d(bf(got["h"]), bf(wp32)), OUT_SLOPE)
        rows += [(k, "float64 on the kernel's operands", rel_err(got[k], ref), RU_TOL[F32])
                 for k, ref in (("h", h_same), ("u", u_same), ("y", xin32.double() + u_same))]
    assert_errors(case, rows)


def fold_conv_t(gh, wd, d):
    """W_dil^T (*) g_h folded through the reflect padding, float64."""
    xz = torch.zeros_like(gh, requires_grad=True)
    (F.conv1d(F.pad(xz, (d, d), mode="reflect"), wd, dilation=d) * gh).sum().backward()
    return xz.grad


def check_backward(case, out, r, mm):
    gx_ref = r["gx"] + (r["post"].double() if case.post else 0.0)
    rows = [(k, "float64 autograd", rel_err(out[k], ref), RU_TOL[mm]) for k, ref in (("gh", r["gh"]), ("gx", gx_ref))]
    if mm == BF16:
        wd32, wp32 = effective_weights(case, out)
        gz32 = r["gy"] * torch.where(r["u32"] > 0, 1.0, OUT_SLOPE)
        gh_same = torch.einsum("mc,bmt->bct", bf(wp32)[:, :, 0], bf(gz32))
        gx_same = r["gy"].double() + fold_conv_t(bf(out["gh"]), bf(wd32), case.dilation)
        if case.slope != 1.0:
            gx_same = gx_same * torch.where(r["x"] > 0, 1.0, case.slope).double()
        if case.post:
            gx_same = gx_same + r["post"].double()
        rows += [(k, "float64 on the kernel's operands", rel_err(out[k], ref), RU_TOL[F32]) for k, ref in (("gh", gh_same), ("gx", gx_same))]
    assert_errors(case, rows)


def check_weight_gradients(case, out, r):
    c, d, L = case.channels, case.dilation, case.length
    nslab = out["nslab"]
    assert out["variant"][1][12] == nslab, (case.name, out["variant"], nslab)
    if case.op == BL_DW:
        gz, h, gh, xin = (_from_bundles(p).double() for p in out["planes"])
        tol, tol_wn = 2e-6, 4e-2
    elif case.math == BF16:
        gz, h, gh, xin = bf(r["gy"] * torch.where(r["u32"] > 0, 1.0, OUT_SLOPE)), bf(r["h32"]), bf(r["gh32"]), bf(F.leaky_relu(r["x"], case.slope))
        tol, tol_wn = 2e-6, 2 * RU_TOL[BF16]
    else:
        gz, h, gh, xin = ((r["gy"] * torch.where(r["u32"] > 0, 1.0, OUT_SLOPE)).double(), r["h32"].double(), r["gh32"].double(),
                          F.leaky_relu(r["x"], case.slope).double())
        tol, tol_wn = 3e-5, 2 * RU_TOL[BF16X6]
    dwp = torch.einsum("bmt,bct->mc", gz, h)
    xpad = F.pad(xin, (d, d), mode="reflect")
    dwd = torch.stack([torch.einsum("bmt,bct->mc", gh, xpad[:, :, j * d: j * d + L]) for j in range(3)], dim=2)
    rows = [(k, "the float64 contraction of the same operands", rel_err(out[k].double().sum(0), ref), tol) for k, ref in (("slab_p", dwp), ("slab_d", dwd))]
    if case.name in WN_CASES:
        rows += [(k, "float64 autograd", rel_err(out[k], r[k]), tol_wn) for k in ("dvp", "dgp", "dvd", "dgd")]
    assert_errors(case, rows)


@pytest.mark.parametrize("name", list(CASES))
def test_ru_instantiation_against_float64(hip, name):
    case = CASES[name]
    out = outputs_of(hip, case)
    rc, v = out["variant"]
    assert rc == 0 and v == case.expect, f"{name}: ran family {v[0]} <{v[1:6]}> geometry {v[6:]}, the case is written for {case.expect}"
    assert all(out["guards"].values()), (name, "written outside the tensor", [k for k, ok in out["guards"].items() if not ok])
    r = unit_ref(case)
    if case.op == FWD:
        check_forward(case, out, r, case.math)
    elif case.op == BL_FWD:
        check_forward(case, out, r, case.math)
        # the bundle forward: y of eben_ru_fwd_ex bit for bit; the planes are bf16 of lrelu(x) and of THAT kernel's h, the sign bits of its u
        assert torch.equal(out["y"], out["y0"]), name
        assert torch.equal(out["xb"], _to_bundles(F.leaky_relu(r["x"], case.slope))), name
        assert torch.equal(out["hb"], _to_bundles(out["h0"])), name
        assert torch.equal(out["um"], _sign_plane(out["u0"])), name
    elif case.op == BWD:
        check_backward(case, out, r, case.math)
    elif case.op == BL_BWD:
        # eben_ru_bwd_ex (one piece) carries the float64 and the same-operand checks; the bundle kernel equals it bit for bit
        check_backward(case, out, r, BF16)
        assert torch.equal(out["gx1"], out["gx"]), name
        assert torch.equal(out["gzb"], _to_bundles(r["gy"] * torch.where(r["u32"] > 0, 1.0, OUT_SLOPE))), name
        assert torch.equal(out["ghb"], _to_bundles(out["gh"])), name
        assert rel_err(_from_bundles(out["ghb"]), r["gh"]) < RU_TOL[BF16]
        # stage B on the plane itself: bf16 g_h is the operand
        wd32, _ = effective_weights(case, out)
        gx_same = r["gy"].double() + fold_conv_t(_from_bundles(out["ghb"]).double(), bf(wd32), case.dilation)
        if case.slope != 1.0:
            gx_same = gx_same * torch.where(r["x"] > 0, 1.0, case.slope).double()
        if case.post:
            gx_same = gx_same + r["post"].double()
        assert rel_err(out["gx1"], gx_same) < RU_TOL[F32], (name, rel_err(out["gx1"], gx_same))
    else:
        check_weight_gradients(case, out, r)


# ---- the multi-tensor entry points -----------------------------------------------------------------------------------------------------
def test_ru_pack_multi_images_are_those_of_pack_ex(hip):
    """eben_ru_pack_multi: both images of all three split maths at 32 / 64 / 128 channels in ONE job list, one job without weight-norm
    scales -- bit-identical to eben_ru_pack_ex job by job."""
    from vibravox_amd._lib import EbenRuPackJob, check, stream

    D = Device(hip)
    jobs, want = [], []
    for c in (32, 64, 128):
        w = D.scales(c)
        for mm in (BF16, BF16X3, BF16X6):
            for which in (0, 1):
                plain = (c, mm, which) == (64, BF16X3, 1)
                sd, sp = (None, None) if plain else (w["sd"].data_ptr(), w["sp"].data_ptr())
                n = hip.eben_ru_packed_floats_ex(c, mm)
                one = torch.full((n,), float("nan"), dtype=torch.float32, device=D.dev)
                check(hip.eben_ru_pack_ex(c, mm, which, w["vd"].data_ptr(), sd, w["vp"].data_ptr(), sp, one.data_ptr(), stream()), "ru_pack_ex")
                buf, view = guarded((n,), torch.float32, D.dev)
                jobs.append(EbenRuPackJob(c, mm, which, 0, w["vd"].data_ptr(), sd, w["vp"].data_ptr(), sp, view.data_ptr()))
                want.append((one, buf, view, (c, mm, which)))
    arr = (EbenRuPackJob * len(jobs))(*jobs)
    check(hip.eben_ru_pack_multi(arr, len(jobs), stream()), "ru_pack_multi")
    torch.cuda.synchronize()
    for one, buf, view, key in want:
        assert guards_intact(buf, view, 0), key
        assert torch.equal(view.view(torch.int32), one.view(torch.int32)), key
    bad = EbenRuPackJob(64, F32, 0, 0, jobs[0].v_dil, None, jobs[0].v_pw, None, jobs[0].wimg)
    assert hip.eben_ru_pack_multi((EbenRuPackJob * 1)(bad), 1, stream()) < 0   # the fp32 MFMA image is eben_ru_pack's


def test_wn_multi_forms_are_the_single_tensor_forms(hip):
    """eben_wn_scale_multi / eben_wn_bwd_multi on three tensors of different shapes (one plain weight, one with a bias column):
    bit-identical to eben_wn_scale / eben_wn_bwd."""
    from vibravox_amd._lib import EbenWnBwdItem, EbenWnScaleItem, check, stream

    dev = torch.device("cuda")
    shapes = [(32, 96, 3, False, True), (64, 64, 1, True, True), (128, 384, 5, False, False)]   # rows, cols, slabs, bias column, weight norm
    sitems, bitems, single, keep = [], [], [], []
    for i, (rows, cols, nslab, bias, wn) in enumerate(shapes):
        v = formula_tensor(f"ruv/wn/{i}/v", (rows, cols), 1 / math.sqrt(cols)).to(dev)
        g = (v.norm(dim=1) * (1 + 0.3 * formula_tensor(f"ruv/wn/{i}/g", (rows,)).to(dev))).contiguous()
        rs = cols + (1 if bias else 0)
        slabs = formula_tensor(f"ruv/wn/{i}/slabs", (nslab, rows, rs)).to(dev)
        s1, n1, s2, n2 = (torch.full((rows,), float("nan"), device=dev) for _ in range(4))
        check(hip.eben_wn_scale(g.data_ptr(), v.data_ptr(), rows, cols, s1.data_ptr(), n1.data_ptr(), stream()), "wn_scale")
        sitems.append(EbenWnScaleItem(g.data_ptr(), v.data_ptr(), s2.data_ptr(), n2.data_ptr(), rows, cols))
        outs = []
        for _ in range(2):
            dg, dv, db = torch.full((rows,), float("nan"), device=dev), torch.full((rows, cols), float("nan"), device=dev), torch.full((rows,), float("nan"), device=dev)
            outs.append((slabs.clone(), dg, dv, db))
        a, b = outs
        gp, np_ = (g.data_ptr(), n1.data_ptr()) if wn else (None, None)
        check(hip.eben_wn_bwd(a[0].data_ptr(), nslab, rows * rs, rows, cols, rs, gp, v.data_ptr(), np_, a[1].data_ptr() if wn else None, a[2].data_ptr(),
                              a[3].data_ptr() if bias else None, stream()), "wn_bwd")
        bitems.append(EbenWnBwdItem(b[0].data_ptr(), gp, v.data_ptr(), np_, b[1].data_ptr() if wn else None, b[2].data_ptr(), b[3].data_ptr() if bias else None,
                                    rows * rs, nslab, rows, cols, rs, 0, 0))
        single.append((s1, n1, s2, n2, a, b, bias, wn))
        keep.append((v, g, slabs))
    check(hip.eben_wn_scale_multi((EbenWnScaleItem * 3)(*sitems), 3, stream()), "wn_scale_multi")
    check(hip.eben_wn_bwd_multi((EbenWnBwdItem * 3)(*bitems), 3, stream()), "wn_bwd_multi")
    torch.cuda.synchronize()
    for i, (s1, n1, s2, n2, a, b, bias, wn) in enumerate(single):
        assert torch.isfinite(s1).all() and torch.equal(s1, s2) and torch.equal(n1, n2), i
        assert torch.isfinite(a[2]).all() and torch.equal(a[2], b[2]), i
        assert not wn or (torch.isfinite(a[1]).all() and torch.equal(a[1], b[1])), i
        assert not bias or (torch.isfinite(a[3]).all() and torch.equal(a[3], b[3])), i
