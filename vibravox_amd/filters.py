"""Biquad filtering on the device: ``lowpass_biquad`` and the zero-phase 4th-order low-pass ``remove_hf``.

Counterpart of ``vibravox.utils.remove_hf`` (vibravox/utils.py:84-116): reflection padding, ``torchaudio.functional.lowpass_biquad``
forward, then backward, then the crop -- the standard way to simulate band-limited input from clean speech.  The IIR recurrence is
``eben_biquad`` (csrc/frontend.hip): parallel along time (chunks of ``CHUNK`` samples, states carried across chunks), float64 state
and accumulation, float32 storage.  The padding and the time reversal are index mapping inside the kernel: no padded copy and no
``torch.flip`` is made.

torchaudio is not installed here, so ``lowpass_biquad_coefficients`` / ``lowpass_biquad`` restate it (parity unpinned); the float64
test oracle is ``scipy.signal.lfilter``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Tuple

import torch

from ._lib import EbenError, check, load, ptr, stream

#: samples per workgroup of eben_biquad (csrc/frontend.hip BQ_CHUNK): rows longer than this carry their state across chunks
CHUNK = 4096
#: samples per thread inside a chunk (BQ_SUB)
SUBCHUNK = 16


def lowpass_biquad_coefficients(sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> Tuple[float, float, float, float, float]:
    """(b0, b1, b2, a1, a2), already divided by a0, of ``torchaudio.functional.lowpass_biquad`` -- restated, parity unpinned
    (torchaudio is not installed here).  Formed as torchaudio forms them for a float32 waveform: every step on float32 CPU tensors,
    in its order, and each coefficient divided by a0 in float32 (``biquad`` -> ``lfilter``)."""
    f32 = torch.float32
    w0 = 2 * math.pi * torch.as_tensor(cutoff_freq, dtype=f32) / sample_rate
    alpha = torch.sin(w0) / 2 / torch.as_tensor(Q, dtype=f32)
    b0 = (1 - torch.cos(w0)) / 2
    b1 = 1 - torch.cos(w0)
    b2 = b0
    a0 = 1 + alpha
    a1 = -2 * torch.cos(w0)
    a2 = 1 - alpha
    return tuple(float(c.to(f32) / a0.to(f32)) for c in (b0, b1, b2, a1, a2))


def _biquad(x2: torch.Tensor, pad: int, coef, reversed_: bool, clamp: bool) -> torch.Tensor:
    """eben_biquad on a contiguous (rows, t) float32 device tensor -> (rows, t + 2*pad)."""
    lib = load()
    rows, t = x2.shape
    out = torch.empty((rows, t + 2 * pad), dtype=torch.float32, device=x2.device)
    nbytes = lib.eben_biquad_workspace(rows, t + 2 * pad)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x2.device) if nbytes else None
    c = (ctypes.c_double * 5)(*coef)
    check(lib.eben_biquad(ptr(x2), ptr(out), rows, t, pad, c, int(reversed_), int(clamp), ws.data_ptr() if ws is not None else None, nbytes,
                          stream()), "biquad")
    return out


def _rows(waveform: torch.Tensor) -> torch.Tensor:
    if not isinstance(waveform, torch.Tensor) or not waveform.is_cuda:
        raise EbenError(f"vibravox_amd filters run only on an MI355X HIP device (got '{getattr(waveform, 'device', type(waveform))}'); "
                        "there is no CPU path -- the CPU oracle is test-only.")
    if waveform.dtype is not torch.float32:
        raise EbenError(f"expected a float32 waveform, got {waveform.dtype}")
    if waveform.dim() < 1 or waveform.numel() == 0:
        raise ValueError(f"expected a non-empty (..., time) waveform, got shape {tuple(waveform.shape)}")
    return waveform.contiguous().reshape(-1, waveform.shape[-1])   # a non-contiguous view is copied once


def lowpass_biquad(waveform: torch.Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> torch.Tensor:
    """``torchaudio.functional.lowpass_biquad`` (restated, parity unpinned) on a (..., time) float32 device tensor: one forward
    pass from a zero state, the output clamped to [-1, 1] as ``lfilter(clamp=True)`` does."""
    x2 = _rows(waveform)
    return _biquad(x2, 0, lowpass_biquad_coefficients(sample_rate, cutoff_freq, Q), False, True).reshape(waveform.shape)


def remove_hf(waveform: torch.Tensor, sample_rate: int, cutoff_freq: float, padding_length: int = 3000) -> torch.Tensor:
    """``vibravox.utils.remove_hf``: low-pass of the fourth order with zero phase shift, (..., time) float32 on the device in, same
    shape out.  A forward pass over the reflect-padded rows, a time-reversed pass over that (float32, clamped) result, the crop
    ``[padding_length : -padding_length]``.

    ``padding_length >= time`` raises ``RuntimeError`` as ``ReflectionPad1d`` does.  ``padding_length = 0`` raises ``ValueError``:
    the reference's ``[0:-0]`` crop would return an empty tensor, which nobody means."""
    padding_length = int(padding_length)
    if padding_length <= 0:
        raise ValueError("remove_hf needs padding_length >= 1: the reference's crop [padding_length:-padding_length] is empty at 0")
    x2 = _rows(waveform)
    t = x2.shape[-1]
    if padding_length >= t:
        raise RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding ({padding_length}, "
                           f"{padding_length}) at dimension -1 of input {list(waveform.shape)}")
    coef = lowpass_biquad_coefficients(sample_rate, cutoff_freq)
    fwd = _biquad(x2, padding_length, coef, False, True)
    bwd = _biquad(fwd, 0, coef, True, True)
    return bwd[:, padding_length:-padding_length].contiguous().reshape(waveform.shape)   # the crop, as one copy: a contiguous result
