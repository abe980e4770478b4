"""Float64 oracle of a conv layer's weight gradient, written from the index formula of csrc/conv_dw3.hip (no autograd):

    dw[co, c, j] = sum_{b, t} A(b, co, t) * X(b, c, refl(t * S - pad_l + j * d)),      dbias[co] = sum_{b, t} A(b, co, t)

A (the small side, l_out long for a Conv1d) and X (the big side) are the operands AS THE KERNEL FORMS THEM (`operands`):
  Conv1d            A = dy * lrelu'(y) (the fused output activation differentiated on load),  X = lrelu(x, in_slope)
  ConvTranspose1d   the adjoint: A = lrelu(x, in_slope) (rows = the layer's c_in), X = dy * lrelu'(y) (columns = c_out / groups),
                    S / pad_l / d those of the layer, zero outside the row -- canon_from_desc and the dispatcher's operand swap
formed in fp32 as on the device, then rounded to bf16 (EBEN_MATH_BF16); EBEN_MATH_BF16X2 keeps X as hi + lo, hi = bf16(x),
lo = bf16(x - hi).  The contraction itself runs in float64 on those values.  `contract` also takes the WRONG paddings and taps the
sensitivity checks of tests/test_dw_oracle.py substitute (zero for reflect, the reflection moved by one sample, a one-tap shift).
"""
import torch

from formula import formula_tensor
from vibravox_amd import ops


def bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> float64."""
    assert t.dtype is torch.float32
    return t.to(torch.bfloat16).to(torch.float64)


def lrelu(t: torch.Tensor, slope: float) -> torch.Tensor:
    return t if slope == 1.0 else torch.where(t > 0, t, t * slope)


def lrelu_derivative(y: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


def case_inputs(name, spec, batch, length):
    """(x, dy, y) of a table case: fp32 formula tensors; y (the saved output, read for its signs only) when out_slope != 1."""
    l_out = spec.out_len(length)
    x = formula_tensor(f"dw3/{name}/x", (batch, spec.c_in, length))
    dy = formula_tensor(f"dw3/{name}/dy", (batch, spec.c_out, l_out))
    y = formula_tensor(f"dw3/{name}/y", (batch, spec.c_out, l_out)) if spec.out_slope != 1.0 else None
    return x, dy, y


def operands(spec, x, dy, y=None, math=ops.MATH_BF16, rounded=True, mask=True, in_act=True, split=None):
    """(A, X) of the layer in float64.  x / dy / y: fp32 layer input, output gradient and (for out_slope != 1) saved output.
    rounded False: the fp32 operands unrounded; (True, False): A rounded, X not.  mask / in_act False drop the output-activation mask /
    the input activation (what a kernel that ignored them would compute).  split: hi + lo X (default: Conv1d under BF16X2)."""
    ra, rx = rounded if isinstance(rounded, tuple) else (rounded, rounded)
    gm = dy * lrelu_derivative(y, spec.out_slope) if (mask and spec.out_slope != 1.0) else dy
    xa = lrelu(x, spec.in_slope) if in_act else x
    a, xo = (xa, gm) if spec.transposed else (gm, xa)
    if split is None:
        split = math == ops.MATH_BF16X2 and not spec.transposed
    A = bf16(a) if ra else a.double()
    if not rx:
        X = xo.double()
    elif split:
        hi = xo.to(torch.bfloat16).to(torch.float32)
        X = hi.double() + bf16(xo - hi)
    else:
        X = bf16(xo)
    return A, X


def contract(spec, A, X, pad="layer", reflect_offset=0, tap_shift=0):
    """(dw in the layer's weight shape, dbias or None for a transposed layer) from the index formula.
    pad "layer": the layer's own (single reflection / zero outside the row); "zero": zero even for a reflect layer.
    reflect_offset 1: the mirror moved by one sample (the edge sample repeated); tap_shift 1: tap j reads where tap j + 1 belongs."""
    B, Ca, La = A.shape
    _, Cx, Lx = X.shape
    G, k, S, d = spec.groups, spec.ksize, spec.stride, spec.dilation
    Mg, Cg = Ca // G, Cx // G
    reflect = spec.reflect and not spec.transposed and pad == "layer"
    dw = torch.zeros(Ca, Cg, k, dtype=torch.float64)
    t = torch.arange(La)
    for j in range(k):
        p = t * S - spec.pad_l + (j + tap_shift) * d
        if reflect:
            p = torch.where(p < 0, -p - reflect_offset, p)
            p = torch.where(p >= Lx, 2 * (Lx - 1) - p + reflect_offset, p)
        ok = (p >= 0) & (p < Lx)
        xj = X[:, :, p.clamp(0, Lx - 1)] * ok.to(torch.float64)   # (B, Cx, La)
        for g in range(G):
            dw[g * Mg:(g + 1) * Mg, :, j] = torch.einsum("bmt,bct->mc", A[:, g * Mg:(g + 1) * Mg], xj[:, g * Cg:(g + 1) * Cg])
    return dw, (None if spec.transposed else A.sum(dim=(0, 2)))


def weight_gradient(spec, x, dy, y=None, math=ops.MATH_BF16, **how):
    """operands + contract: keyword arguments of either."""
    c_kw = {key: how.pop(key) for key in ("pad", "reflect_offset", "tap_shift") if key in how}
    A, X = operands(spec, x, dy, y, math, **how)
    return contract(spec, A, X, **c_kw)
