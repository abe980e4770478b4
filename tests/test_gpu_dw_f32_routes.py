"""GPU: every case of the table of tests/test_dw_f32_variants.py -- one per conv_dw2_kernel / dw_pack_a_kernel instantiation, the
chunk lengths and the direct X staging of conv_dw_kernel, tiny_dw_kernel, m1_dw_kernel and the plan edges listed there -- through
the C ABI (eben_conv1d_bwd_dw_workspace, eben_conv1d_bwd_dw, eben_wn_bwd) against the float64 index-formula oracle of
tests/dw_oracle.py on the unrounded operands.  The bound is the one tests/test_gpu_ops.py (test_conv_layer_fwd_bwd) holds these
exact-fp32 kernels to: 3e-5 of max|ref| for dbias, twice that for dv; tests/test_dw_f32_oracle.py shows that each case's inputs put a
wrong reflection, a shifted tap or a dropped mask or activation more than 10x that bound away.  The workspace -- split-K slabs and
the packed gradient image behind them -- is NaN before every launch: whatever the kernels leave unwritten and the reduction then
reads fails the finiteness check of rel_err.  The split-K hand-over cases run a second time into a workspace of 1e30s and must give
the same bits: a read of an unwritten buffer that happens to be finite would not.
"""
import ctypes
import math

import pytest
import torch

from tests import dw_oracle
from tests.test_dw_f32_variants import CASES, DW2, F32, FALLBACK, FIELDS, HAND_OVER, ONE_ROW, TINY, f32_variant
from tests.test_gpu_dw3_routes import FP32_TOL, dev, memo
from tests.test_gpu_ops import rel_err

pytestmark = pytest.mark.gpu

ROUTE_NAMES = {TINY: "tiny", ONE_ROW: "one_row", DW2: "dw2", FALLBACK: "fallback"}


def inputs(name, case):
    return memo(("f32/in", name), lambda: dw_oracle.case_inputs("f32/" + name, case.spec(), case.batch, case.length))


def oracle(name, case):
    """(dw, dbias) of the float64 oracle on the unrounded operands, computed once per case and shared."""
    return memo(("f32/ref", name), lambda: dw_oracle.weight_gradient(case.spec(), *inputs(name, case), math=case.math, rounded=False))


def launch(lib, d, dy, y, x, has_bias, wshape, fill=float("nan")):
    """tests/test_gpu_dw3_routes.py's launch with the workspace's prefill a parameter: eben_conv1d_bwd_dw, then the slab sum."""
    from vibravox_amd._lib import check, ptr, stream

    nslab, row_stride = ctypes.c_int(0), ctypes.c_int(0)
    ws_bytes = lib.eben_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(row_stride))
    rows, cols = wshape[0], wshape[1] * wshape[2]
    assert ws_bytes >= 4 * nslab.value * rows * row_stride.value and row_stride.value == cols + 1
    ws = torch.full(((ws_bytes + 3) // 4,), fill, dtype=torch.float32, device="cuda")
    check(lib.eben_conv1d_bwd_dw(ctypes.byref(d), ptr(dy), ptr(y), ptr(x), has_bias, ptr(ws), ws_bytes, stream()), "bwd_dw")
    dv = torch.full(wshape, float("nan"), dtype=torch.float32, device="cuda")
    dbias = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda") if has_bias else None
    check(lib.eben_wn_bwd(ptr(ws), nslab.value, rows * row_stride.value, rows, cols, row_stride.value, None, None, None, None,
                          ptr(dv), ptr(dbias), stream()), "wn_bwd")
    torch.cuda.synchronize()
    return dv, dbias


def run_case(lib, name):
    """The case's weight gradient on the device, once: dict(dv, dbias, dv_nobias)."""
    def make():
        case = CASES[name]
        x, dy, y = (dev(t) for t in inputs(name, case))
        wshape = case.spec().weight_shape()
        out = {}
        out["dv"], out["dbias"] = launch(lib, case.desc(), dy, y, x, 1 if case.has_bias() else 0, wshape)
        if case.has_bias():
            out["dv_nobias"], _ = launch(lib, case.desc(), dy, y, x, 0, wshape)
        return out
    return memo(("f32/gpu", name), make)


@pytest.mark.parametrize("name", list(CASES))
def test_f32_case_against_the_float64_oracle(hip, name):
    case = CASES[name]
    rc, v = f32_variant(hip, case.desc())
    assert rc == 0 and v == case.expect, (name, dict(zip(FIELDS, v)))
    got = run_case(hip, name)
    dw, dbias = oracle(name, case)
    e_dv = rel_err(got["dv"], dw)
    print(f"[dw_f32] {name} ({ROUTE_NAMES[v[0]]}): dv {e_dv:.3e}", end="")
    assert e_dv < 2 * FP32_TOL, (name, e_dv)
    assert case.has_bias() == (not case.spec().transposed)
    if case.has_bias():
        e_db = rel_err(got["dbias"], dbias)
        print(f" dbias {e_db:.3e}", end="")
        assert e_db < FP32_TOL, (name, e_db)
        # without the bias column the weight gradient is the same, bit for bit
        assert torch.equal(got["dv_nobias"], got["dv"]), name
    print()


@pytest.mark.parametrize("name", HAND_OVER)
def test_hand_over_case_reads_nothing_it_did_not_write(hip, name):
    """Blocks that own several chunks: the same bits whether the workspace held NaN or 1e30 before the launch."""
    case = CASES[name]
    p = case.plan()
    assert p["nsplit"] < p["nchunks"]
    x, dy, y = (dev(t) for t in inputs(name, case))
    first = run_case(hip, name)
    dv, dbias = launch(hip, case.desc(), dy, y, x, 1, case.spec().weight_shape(), fill=1e30)
    assert torch.equal(dv, first["dv"]) and torch.equal(dbias, first["dbias"]), name
    assert rel_err(dv, oracle(name, case)[0]) < 2 * FP32_TOL


@pytest.mark.parametrize("name", ["dw2_64_x32", "fb_rows3", "tiny_pqmf_l0", "m1_96"])
def test_weight_norm_layer_backward_on_the_f32_routes(hip, name):
    """One case per route through ops.conv_layer at the default (fp32) backward math: dv, dg, dbias against float64 autograd of the
    weight normalisation applied to the oracle's gradient."""
    from vibravox_amd import ops

    case = CASES[name]
    spec = case.spec()
    assert spec.out_slope == 1.0 and case.math == F32   # the saved output's signs are then no part of the comparison
    assert {CASES[n].expect[0] for n in ("dw2_64_x32", "fb_rows3", "tiny_pqmf_l0", "m1_96")} == {DW2, FALLBACK, TINY, ONE_ROW}
    assert f32_variant(hip, ops.conv_desc(spec, case.batch, case.length, F32))[1] == case.expect
    x, dy, _ = inputs(name, case)
    wshape = spec.weight_shape()
    v = dw_oracle.formula_tensor(f"f32/{name}/v", wshape, 1 / math.sqrt(wshape[1] * wshape[2]))
    g = v.reshape(wshape[0], -1).norm(dim=1).reshape(-1, 1, 1) * (1 + 0.3 * dw_oracle.formula_tensor(f"f32/{name}/g", (wshape[0], 1, 1)))
    bias = dw_oracle.formula_tensor(f"f32/{name}/b", (spec.c_out,), 0.1)

    dw, dbias = oracle(name, case)
    rv, rg = v.double().requires_grad_(True), g.double().requires_grad_(True)
    w = rg * rv / rv.reshape(wshape[0], -1).norm(dim=1).reshape(-1, 1, 1)
    (w * dw).sum().backward()

    vd, gd, bd = (dev(t).requires_grad_(True) for t in (v, g, bias))
    y = ops.conv_layer(dev(x), vd, gd, bd, spec)
    (y * dev(dy)).sum().backward()
    torch.cuda.synchronize()
    errs = {"dv": rel_err(vd.grad, rv.grad), "dg": rel_err(gd.grad, rg.grad), "dbias": rel_err(bd.grad, dbias)}
    print(f"[dw_f32] {name} through conv_layer: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert all(e < 2 * FP32_TOL for e in errs.values()), (name, errs)
