"""float64 restatement of the two FIR-bank operations of the library (test-only): eben_fir_decimate and eben_fir_interp_sum, the
operators behind PQMF analysis / synthesis, the A-weighting prefilter and their adjoints.

    decimate     y[b,k,t] = sum_j w[k,j] x[b,0,t stride + off0 + j]                       x zero outside [0, lx)
    interp_sum   x[b,0,u] = sum_k sum_{t stride + off0 + j = u} w[k,j] y[b,k,t]           y zero outside [0, ly)

for any sign of off0 and any lx, ly (outputs may run past the input on either side).  The two are written independently of each
other -- a strided convolution and a transposed convolution plus cropping -- so that either checks the other (tests/test_fir_oracle.py);
neither goes through autograd.  Tensors are CPU float64: x (batch, 1, lx), w (bands, ntaps), y (batch, bands, ly)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def decimate(x: torch.Tensor, w: torch.Tensor, ly: int, stride: int, off0: int) -> torch.Tensor:
    lx, ntaps = x.shape[2], w.shape[1]
    left = max(0, -off0)
    start = off0 + left                                  # index of sample off0 in the padded signal (>= 0)
    right = max(0, start + (ly - 1) * stride + ntaps - (left + lx))
    padded = F.pad(x, (left, right))[..., start:]
    return F.conv1d(padded, w[:, None, :], stride=stride)[..., :ly]


def interp_sum(y: torch.Tensor, w: torch.Tensor, lx: int, stride: int, off0: int) -> torch.Tensor:
    # full[v] = sum_k sum_{t stride + j = v} w[k,j] y[k,t], v = 0 .. (ly - 1) stride + ntaps - 1; x[u] = full[u - off0] where that exists
    full = F.conv_transpose1d(y, w[:, None, :], stride=stride)
    x = torch.zeros(y.shape[0], 1, lx, dtype=y.dtype)
    lo, hi = max(0, off0), min(lx, full.shape[2] + off0)
    if hi > lo:
        x[..., lo:hi] = full[..., lo - off0:hi - off0]
    return x
