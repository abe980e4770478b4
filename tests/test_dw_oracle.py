"""CPU: the float64 weight-gradient oracle of tests/dw_oracle.py against float64 torch.autograd, for every case of the table of
tests/test_dw3_variants.py -- and that each case's inputs SHOW the errors the GPU test is after: a reflect layer computed with zero
padding or with the mirror moved by one sample, a transposed layer computed one tap off, each more than 10x the GPU tolerance away."""
import pytest
import torch
import torch.nn.functional as F

from tests import dw_oracle
from tests.test_dw3_variants import CASES, FALL_THROUGH

GPU_TOL = 1e-4   # tests/test_gpu_dw3_routes.py


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def autograd_dw(spec, A, X):
    """d/dw of sum(conv(X; w) * A) -- for a transposed layer sum(conv_transpose(A; w) * X): the layer is linear in w."""
    w = torch.zeros(spec.weight_shape(), dtype=torch.float64, requires_grad=True)
    if spec.transposed:
        out = F.conv_transpose1d(A, w, None, spec.stride, spec.pad_l, spec.output_padding, spec.groups, spec.dilation)
        (out * X).sum().backward()
    else:
        xp = F.pad(X, (spec.pad_l, spec.pad_r), mode="reflect") if spec.reflect else F.pad(X, (spec.pad_l, spec.pad_r))
        (F.conv1d(xp, w, None, spec.stride, 0, spec.dilation, spec.groups) * A).sum().backward()
    return w.grad


@pytest.mark.parametrize("name", list(CASES) + ["fall/" + n for n in FALL_THROUGH])
def test_oracle_equals_float64_autograd_on_unrounded_operands(name):
    case = FALL_THROUGH[name[5:]] if name.startswith("fall/") else CASES[name]
    spec = case.spec()
    x, dy, y = dw_oracle.case_inputs(name, spec, case.batch, case.length)
    A, X = dw_oracle.operands(spec, x, dy, y, case.math, rounded=False)
    dw, dbias = dw_oracle.contract(spec, A, X)
    assert dw.shape == spec.weight_shape()
    assert rel(dw, autograd_dw(spec, A, X)) < 1e-12
    if not spec.transposed:
        assert rel(dbias, A.sum(dim=(0, 2))) < 1e-12 and dbias.shape == (spec.c_out,)
    # the operands themselves: the mask and the activations sit where the layer has them
    gm = dy.double() * torch.where(y.double() > 0, 1.0, spec.out_slope) if y is not None else dy.double()
    xa = F.leaky_relu(x.double(), spec.in_slope) if spec.in_slope != 1.0 else x.double()
    a_ref, x_ref = (xa, gm) if spec.transposed else (gm, xa)
    assert rel(A, a_ref) < 1e-6 and rel(X, x_ref) < 1e-6   # formed in fp32


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.spec().reflect])
def test_reflect_case_shows_a_wrong_padding(name):
    case = CASES[name]
    spec = case.spec()
    A, X = dw_oracle.operands(spec, *dw_oracle.case_inputs(name, spec, case.batch, case.length), case.math)
    true = dw_oracle.contract(spec, A, X)[0]
    assert rel(dw_oracle.contract(spec, A, X, pad="zero")[0], true) > 10 * GPU_TOL
    assert rel(dw_oracle.contract(spec, A, X, reflect_offset=1)[0], true) > 10 * GPU_TOL


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.spec().transposed])
def test_transposed_case_shows_a_one_tap_shift(name):
    case = CASES[name]
    spec = case.spec()
    A, X = dw_oracle.operands(spec, *dw_oracle.case_inputs(name, spec, case.batch, case.length), case.math)
    true = dw_oracle.contract(spec, A, X)[0]
    assert rel(dw_oracle.contract(spec, A, X, tap_shift=1)[0], true) > 10 * GPU_TOL
    assert rel(dw_oracle.contract(spec, A, X, tap_shift=-1)[0], true) > 10 * GPU_TOL


def test_rounded_operands_are_bf16_values_and_the_split_restores_the_activation():
    case = CASES["enc_s2_x2"]
    spec = case.spec()
    x, dy, y = dw_oracle.case_inputs("enc_s2_x2", spec, case.batch, case.length)
    A, X1 = dw_oracle.operands(spec, x, dy, y, dw_oracle.ops.MATH_BF16)
    _, X2 = dw_oracle.operands(spec, x, dy, y, dw_oracle.ops.MATH_BF16X2)
    assert torch.equal(A, A.to(torch.bfloat16).double()) and torch.equal(X1, X1.to(torch.bfloat16).double())
    e1, e2 = float((X1 - x.double()).abs().max()), float((X2 - x.double()).abs().max())
    assert 0 < e2 < e1 * 2.0 ** -7     # 8 more mantissa bits
    # rounded AFTER the mask: bf16(dy * lrelu'(y)), not bf16(dy) * lrelu'(y)
    case = CASES["latent_up"]
    spec = case.spec()
    x, dy, y = dw_oracle.case_inputs("latent_up", spec, case.batch, case.length)
    A, _ = dw_oracle.operands(spec, x, dy, y)
    mask = torch.where(y > 0, 1.0, spec.out_slope)
    assert torch.equal(A, (dy * mask).to(torch.bfloat16).double())
    assert not torch.equal(A, dy.to(torch.bfloat16).double() * mask.double())
