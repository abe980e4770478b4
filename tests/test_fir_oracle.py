"""CPU: the float64 FIR-bank reference of the GPU tests (tests/fir_oracle.py) against a triple-loop evaluation of the two definitions,
and its two independently written halves against each other (interp_sum is the adjoint of decimate: float64 autograd of <A x, s>).
Tiny shapes, off0 of both signs, ly running past the input, a window that never meets the input's interior.  Everything is float64:
the bound is a few ulps of sums of <= 30 products of magnitude <= 1."""
import pytest
import torch

from tests import fir_oracle
from formula import formula_tensor

TOL = 1e-13

# (bands, ntaps, stride, off0, batch, lx, ly)
SHAPES = [(3, 10, 3, 5, 2, 40, 17), (2, 7, 4, -6, 1, 30, 12), (3, 5, 2, -20, 1, 9, 14), (1, 4, 1, 3, 1, 5, 5)]


def tensors(bands, ntaps, stride, off0, batch, lx, ly):
    tag = f"fir_oracle/{bands}/{ntaps}/{stride}/{off0}/{batch}/{lx}/{ly}"
    return (formula_tensor(tag + "/x", (batch, 1, lx)).double(), formula_tensor(tag + "/w", (bands, ntaps)).double(),
            formula_tensor(tag + "/s", (batch, bands, ly)).double())


def loops(x, w, s, stride, off0):
    """A x and A^T s term by term from the definitions."""
    (batch, _, lx), (bands, ntaps), ly = x.shape, w.shape, s.shape[2]
    ax, ats = torch.zeros(batch, bands, ly, dtype=torch.float64), torch.zeros(batch, 1, lx, dtype=torch.float64)
    for b in range(batch):
        for k in range(bands):
            for t in range(ly):
                for j in range(ntaps):
                    u = t * stride + off0 + j
                    if 0 <= u < lx:
                        ax[b, k, t] += w[k, j] * x[b, 0, u]
                        ats[b, 0, u] += w[k, j] * s[b, k, t]
    return ax, ats


@pytest.mark.parametrize("bands,ntaps,stride,off0,batch,lx,ly", SHAPES)
def test_oracle_against_the_definitions_and_its_own_adjoint(bands, ntaps, stride, off0, batch, lx, ly):
    x, w, s = tensors(bands, ntaps, stride, off0, batch, lx, ly)
    ax_ref, ats_ref = loops(x, w, s, stride, off0)
    assert ats_ref.abs().max() > 0 and ax_ref.abs().max() > 0
    ax = fir_oracle.decimate(x, w, ly, stride, off0)
    ats = fir_oracle.interp_sum(s, w, lx, stride, off0)
    assert ax.shape == ax_ref.shape and ats.shape == ats_ref.shape and ax.dtype == ats.dtype == torch.float64
    xg = x.clone().requires_grad_(True)
    (fir_oracle.decimate(xg, w, ly, stride, off0) * s).sum().backward()
    errs = {"decimate vs loops": float((ax - ax_ref).abs().max()), "interp_sum vs loops": float((ats - ats_ref).abs().max()),
            "interp_sum vs autograd of decimate": float((ats - xg.grad).abs().max())}
    print((bands, ntaps, stride, off0, batch, lx, ly), errs)
    assert max(errs.values()) < TOL, errs
