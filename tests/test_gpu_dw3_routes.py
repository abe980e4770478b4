"""GPU: every case of the table of tests/test_dw3_variants.py -- the generator's conv forms under the bf16-mixed plan, one per
conv_dw3_kernel / dw3_pack_a_kernel instantiation and plan edge -- through the C ABI (eben_conv1d_bwd_dw_workspace,
eben_conv1d_bwd_dw, eben_wn_bwd) against the float64 index-formula oracle of tests/dw_oracle.py on the operands as the kernel rounds
them.  The bound is the one tests/test_gpu_ops.py holds this kernel to (1e-4 of max|ref|: fp32 accumulation of exact bf16 products);
tests/test_dw_oracle.py shows that each case's inputs put a wrong reflection or a shifted tap more than 10x that bound away.  The
workspace -- split-K slabs and the packed gradient image behind them -- is NaN before every launch: whatever the kernels leave
unwritten and the reduction then reads fails the finiteness check of rel_err.
"""
import ctypes
import math

import pytest
import torch

from tests import dw_oracle
from tests.test_dw3_variants import BF16, BF16X2, CASES, DW3, FALL_THROUGH, dw_variant
from tests.test_gpu_ops import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4          # dv, dbias against the oracle on the rounded operands
FAR = 10 * TOL      # how far the oracle WITHOUT a mask / an activation must be for the comparison to show it
FP32_TOL = 3e-5     # test_conv_layer_fwd_bwd's bound for the exact-fp32 kernels (2x for dv)

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def inputs(name, case):
    return memo(("in", name), lambda: dw_oracle.case_inputs(name, case.spec(), case.batch, case.length))


def oracle(name, case, **how):
    """(dw, dbias) of the float64 oracle, computed once per (case, variant) and shared."""
    key = ("ref", name) + tuple(sorted(how.items()))
    return memo(key, lambda: dw_oracle.weight_gradient(case.spec(), *inputs(name, case), math=case.math, **how))


def dev(t):
    return None if t is None else t.to("cuda")


def launch(lib, d, dy, y, x, has_bias, wshape):
    """eben_conv1d_bwd_dw into a NaN workspace, then the slab sum: (dv, dbias or None)."""
    from vibravox_amd._lib import check, ptr, stream

    nslab, row_stride = ctypes.c_int(0), ctypes.c_int(0)
    ws_bytes = lib.eben_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(row_stride))
    rows, cols = wshape[0], wshape[1] * wshape[2]
    assert ws_bytes >= 4 * nslab.value * rows * row_stride.value and row_stride.value == cols + 1
    ws = torch.full(((ws_bytes + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.eben_conv1d_bwd_dw(ctypes.byref(d), ptr(dy), ptr(y), ptr(x), has_bias, ptr(ws), ws_bytes, stream()), "bwd_dw")
    dv = torch.full(wshape, float("nan"), dtype=torch.float32, device="cuda")
    dbias = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda") if has_bias else None
    check(lib.eben_wn_bwd(ptr(ws), nslab.value, rows * row_stride.value, rows, cols, row_stride.value, None, None, None, None,
                          ptr(dv), ptr(dbias), stream()), "wn_bwd")
    torch.cuda.synchronize()
    return dv, dbias


def run_case(lib, name):
    """The case's weight gradient on the device, once: dict(dv, dbias, dv_nobias, dv_direct)."""
    def make():
        from vibravox_amd import ops
        from vibravox_amd._lib import check, ptr, stream

        case = CASES[name]
        spec = case.spec()
        x, dy, y = (dev(t) for t in inputs(name, case))
        wshape = spec.weight_shape()
        out = {}
        if case.premasked():
            # ops.weight_grads masks the gradient by one element-wise launch and hands the layer over without its activation
            v = torch.zeros(wshape, dtype=torch.float32, device="cuda")
            full = ops.conv_desc(spec, case.batch, case.length, case.math)
            out["dv"], _, _ = ops.weight_grads(full, dy, y, x, v, None, None, None)
            gm = torch.empty_like(dy)
            check(lib.eben_lrelu_bwd(ptr(dy), ptr(y), ptr(gm), dy.numel(), spec.out_slope, stream()), "lrelu_bwd")
            out["dv_direct"], _ = launch(lib, case.dw_desc(), gm, None, x, 0, wshape)
            torch.cuda.synchronize()
            return out
        out["dv"], out["dbias"] = launch(lib, case.dw_desc(), dy, y, x, 1 if case.bias else 0, wshape)
        if case.bias:
            out["dv_nobias"], _ = launch(lib, case.dw_desc(), dy, y, x, 0, wshape)
        return out
    return memo(("gpu", name), make)


@pytest.mark.parametrize("name", list(CASES))
def test_dw3_case_against_the_float64_oracle(hip, name):
    case = CASES[name]
    spec = case.spec()
    rc, v = dw_variant(hip, case.dw_desc())
    assert rc == 0 and v[0] == DW3 and v == case.expect, (name, v)
    got = run_case(hip, name)
    dw, dbias = oracle(name, case)
    e_dv = rel_err(got["dv"], dw)
    print(f"[dw3] {name}: dv {e_dv:.3e}", end="")
    assert e_dv < TOL, (name, e_dv)
    if not spec.transposed:
        assert case.bias
        e_db = rel_err(got["dbias"], dbias)
        print(f" dbias {e_db:.3e}", end="")
        assert e_db < TOL, (name, e_db)
        # without the bias column the weight gradient is the same, bit for bit
        assert torch.equal(got["dv_nobias"], got["dv"]), name
    if case.premasked():
        e_direct = rel_err(got["dv_direct"], dw)
        print(f" direct {e_direct:.3e}", end="")
        assert torch.equal(got["dv"], got["dv_direct"]), name
        assert e_direct < TOL
    # a kernel that ignored the mask of the fused output activation, or the activation applied on load, would be far off
    if spec.out_slope != 1.0:
        far = rel_err(oracle(name, case, mask=False)[0], dw)
        print(f" | no mask {far:.3e}", end="")
        assert far > FAR, (name, far)
    if spec.in_slope != 1.0:
        far = rel_err(oracle(name, case, in_act=False)[0], dw)
        print(f" | no input activation {far:.3e}", end="")
        assert far > FAR, (name, far)
    print()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.math == BF16X2])
def test_split_activation_operand_is_closer_to_the_unrounded_one(hip, name):
    """EBEN_MATH_BF16X2 keeps the layer's activations as hi + lo tiles: against the float64 contraction of the UNROUNDED X (the gradient
    operand rounded as both runs round it) it must be strictly closer than the EBEN_MATH_BF16 run of the same layer."""
    plain = name[:-3]
    assert name.endswith("_x2") and CASES[plain].math == BF16 and CASES[plain].kw == CASES[name].kw
    assert (CASES[plain].batch, CASES[plain].length) == (CASES[name].batch, CASES[name].length)
    case = CASES[name]
    # same inputs for both runs: the split case's
    exact = memo(("exact", name), lambda: dw_oracle.weight_gradient(case.spec(), *inputs(name, case), math=case.math, rounded=(True, False)))[0]
    split = run_case(hip, name)["dv"]
    x, dy, y = (dev(t) for t in inputs(name, case))
    from vibravox_amd import ops

    d1 = ops.conv_desc(case.spec(), case.batch, case.length, BF16)
    assert dw_variant(hip, d1)[1] == CASES[plain].expect
    single, _ = launch(hip, d1, dy, y, x, 1, case.spec().weight_shape())
    e2, e1 = rel_err(split, exact), rel_err(single, exact)
    print(f"[dw3] {name}: against the unrounded activations: bf16x2 {e2:.3e}, bf16 {e1:.3e}")
    assert e2 < e1, (name, e2, e1)
    assert rel_err(split, oracle(name, case)[0]) < TOL


@pytest.mark.parametrize("name", ["enc_s4", "dec_s4", "rows96"])
def test_weight_norm_layer_backward_on_dw3(hip, name):
    """One case per route family (reflect strided, transposed, zero-padded) through ops.conv_layer under ops.backward_math(MATH_BF16):
    dv, dg, dbias against float64 autograd of the weight normalisation applied to the oracle's gradient on the rounded operands."""
    from vibravox_amd import ops

    case = CASES[name]
    spec = case.spec()
    assert spec.out_slope == 1.0   # the saved output's signs are then no part of the comparison
    d = ops.conv_desc(spec, case.batch, case.length, BF16)
    assert dw_variant(hip, d)[1][0] == DW3
    x, dy, _ = inputs(name, case)
    wshape = spec.weight_shape()
    v = dw_oracle.formula_tensor(f"dw3/{name}/v", wshape, 1 / math.sqrt(wshape[1] * wshape[2]))
    g = v.reshape(wshape[0], -1).norm(dim=1).reshape(-1, 1, 1) * (1 + 0.3 * dw_oracle.formula_tensor(f"dw3/{name}/g", (wshape[0], 1, 1)))
    bias = dw_oracle.formula_tensor(f"dw3/{name}/b", (spec.c_out,), 0.1) if case.bias else None

    dw, dbias = oracle(name, case)
    rv, rg = v.double().requires_grad_(True), g.double().requires_grad_(True)
    w = rg * rv / rv.reshape(wshape[0], -1).norm(dim=1).reshape(-1, 1, 1)
    (w * dw).sum().backward()

    vd, gd = dev(v).requires_grad_(True), dev(g).requires_grad_(True)
    bd = dev(bias).requires_grad_(True) if case.bias else None
    with ops.backward_math(ops.MATH_BF16):
        y = ops.conv_layer(dev(x), vd, gd, bd, spec)
    (y * dev(dy)).sum().backward()
    torch.cuda.synchronize()
    errs = {"dv": rel_err(vd.grad, rv.grad), "dg": rel_err(gd.grad, rg.grad)}
    if case.bias:
        errs["dbias"] = rel_err(bd.grad, dbias)
    print(f"[dw3] {name} through conv_layer: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert all(e < 2 * TOL for e in errs.values()), (name, errs)


@pytest.mark.parametrize("name", list(FALL_THROUGH))
def test_layer_refused_by_dw3_still_gets_its_gradient(hip, name):
    """bf16-math layers outside conv_dw3 take the exact-fp32 kernels: the fp32 bound against the oracle on the unrounded operands."""
    from vibravox_amd import ops

    case = FALL_THROUGH[name]
    spec = case.spec()
    d = ops.conv_desc(spec, case.batch, case.length, case.math)
    rc, v = dw_variant(hip, d)
    assert rc == 0 and v == case.expect and v[0] != DW3
    x, dy, y = dw_oracle.case_inputs("fall/" + name, spec, case.batch, case.length)
    dw, dbias = dw_oracle.weight_gradient(spec, x, dy, y, case.math, rounded=False)
    has_bias = 1 if (case.bias and not spec.transposed) else 0
    dv, db = launch(hip, d, dev(dy), dev(y), dev(x), has_bias, spec.weight_shape())
    e_dv = rel_err(dv, dw)
    e_db = rel_err(db, dbias) if has_bias else 0.0
    print(f"[dw3] fall-through {name} (route {v[0]}): dv {e_dv:.3e} dbias {e_db:.3e}")
    assert e_dv < 2 * FP32_TOL and e_db < FP32_TOL, (name, e_dv, e_db)
