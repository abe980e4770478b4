"""CPU: the float64 weight-gradient oracle of tests/dw_oracle.py on the UNROUNDED operands (what the exact-fp32 routes compute) against
float64 torch.autograd, for every case of the table of tests/test_dw_f32_variants.py -- and that each case's inputs SHOW the errors
tests/test_gpu_dw_f32_routes.py is after: a reflect layer computed with zero padding or with the mirror moved by one sample, a
transposed layer computed one tap off, a masked or activated layer computed without its mask or activation, each more than 10x the
GPU bound away."""
import pytest
import torch

from tests import dw_oracle
from tests.test_dw_f32_variants import CASES
from tests.test_dw_oracle import autograd_dw, rel

GPU_TOL = 2 * 3e-5   # tests/test_gpu_dw_f32_routes.py: dv
FAR = 10 * GPU_TOL

_memo = {}


def operands(name):
    if name not in _memo:
        case = CASES[name]
        spec = case.spec()
        A, X = dw_oracle.operands(spec, *dw_oracle.case_inputs("f32/" + name, spec, case.batch, case.length), case.math, rounded=False)
        _memo[name] = (A, X, dw_oracle.contract(spec, A, X)[0])
    return _memo[name]


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_float64_autograd(name):
    spec = CASES[name].spec()
    A, X, dw = operands(name)
    assert dw.shape == spec.weight_shape()
    assert rel(dw, autograd_dw(spec, A, X)) < 1e-12


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.spec().reflect])
def test_reflect_case_shows_a_wrong_padding(name):
    spec = CASES[name].spec()
    A, X, true = operands(name)
    assert rel(dw_oracle.contract(spec, A, X, pad="zero")[0], true) > FAR
    assert rel(dw_oracle.contract(spec, A, X, reflect_offset=1)[0], true) > FAR


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.spec().transposed])
def test_transposed_case_shows_a_one_tap_shift(name):
    spec = CASES[name].spec()
    A, X, true = operands(name)
    assert rel(dw_oracle.contract(spec, A, X, tap_shift=1)[0], true) > FAR
    assert rel(dw_oracle.contract(spec, A, X, tap_shift=-1)[0], true) > FAR


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.spec().out_slope != 1.0 or c.spec().in_slope != 1.0])
def test_masked_or_activated_case_shows_a_dropped_mask_or_activation(name):
    case = CASES[name]
    spec = case.spec()
    ins = dw_oracle.case_inputs("f32/" + name, spec, case.batch, case.length)
    true = operands(name)[2]
    if spec.out_slope != 1.0:
        assert rel(dw_oracle.weight_gradient(spec, *ins, math=case.math, rounded=False, mask=False)[0], true) > FAR
    if spec.in_slope != 1.0:
        assert rel(dw_oracle.weight_gradient(spec, *ins, math=case.math, rounded=False, in_act=False)[0], true) > FAR
