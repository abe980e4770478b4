"""Float64 restatement of the evaluation metrics beyond the two ``base_se.py`` logs (test-only): ESTOI, zero-mean SI-SDR / SI-SNR,
SNR and the log-spectral distance.

* ESTOI: ``pystoi.stoi(clean, processed, fs, extended=True)``.  The front end (resampling to 10 kHz, silence removal, STFT, third-octave
  matrix) is the one of ``tests/metrics_oracle.py``; the tail is pystoi's ``row_col_normalize`` branch.  It is restated from pystoi's
  published source and is NOT pinned against pystoi: neither pystoi nor torchmetrics is installed here.  What a later pin could need to
  flip is a named switch in ``CONVENTIONS``.
* ``si_sdr(..., zero_mean)`` / ``snr(..., zero_mean)``: torchmetrics' ``scale_invariant_signal_distortion_ratio`` and
  ``signal_noise_ratio`` with their ``eps`` of the float32 inputs the device receives; ``si_snr`` is SI-SDR with ``zero_mean=True``.
* ``lsd``: through float64 ``torch.stft`` -- an implementation that shares nothing with the kernel's gather and FFT, as the MRSTFT
  tests use it.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import metrics_oracle as M

CONVENTIONS = dict(
    dither=False,            # pystoi adds EPS * randn before each normalisation (so that no norm is 0); not reproduced: it is random
    zero_norm_value=0.0,     # a row or column whose centred norm is exactly 0 contributes this instead of 0 / 0
    min_frames_value=1e-5,   # pystoi's return value when fewer than N STFT frames are left
)
LSD_FLOOR = 1e-8


def _normalise(x, axis):
    x = x - x.mean(axis, keepdims=True)
    norm = np.sqrt((x * x).sum(axis, keepdims=True))
    safe = np.where(norm > 0, norm, 1.0)
    return np.where(norm > 0, x / safe, CONVENTIONS["zero_norm_value"])


def row_col_normalize(seg):
    """(J, bands, N): every band's N frames centred and scaled to unit norm, then every frame's bands."""
    assert not CONVENTIONS["dither"]
    return _normalise(_normalise(seg, 2), 1)


def envelopes(x, y, fs):
    """Third-octave envelopes (bands, frames) of clean x and processed y after resampling and silence removal."""
    x, y = M.resample(np.asarray(x, np.float64), fs), M.resample(np.asarray(y, np.float64), fs)
    x, y = M.remove_silent_frames(x, y)
    xs, ys = M.stft(x).T, M.stft(y).T
    obm, _ = M.thirdoct()
    return np.sqrt(obm @ np.abs(xs) ** 2), np.sqrt(obm @ np.abs(ys) ** 2)


def segments(env):
    return np.array([env[:, m - M.N:m] for m in range(M.N, env.shape[1] + 1)])


def estoi_from_envelopes(xt, yt):
    if xt.shape[-1] < M.N:
        return CONVENTIONS["min_frames_value"]
    xn, yn = row_col_normalize(segments(xt)), row_col_normalize(segments(yt))
    return float((xn * yn / M.N).sum() / xn.shape[0])


def estoi_clip(x, y, fs):
    """pystoi.stoi(x=clean, y=processed, fs, extended=True), float64."""
    return estoi_from_envelopes(*envelopes(x, y, fs))


def estoi(preds, target, fs):
    """torchmetrics argument order: (..., T) -> (...), float64."""
    p = np.asarray(preds, np.float64)
    t = np.asarray(target, np.float64)
    lead = p.shape[:-1]
    p2, t2 = p.reshape(-1, p.shape[-1]), t.reshape(-1, t.shape[-1])
    return np.array([estoi_clip(t2[i], p2[i], fs) for i in range(p2.shape[0])]).reshape(lead)


def _centred(preds, target, zero_mean):
    p = np.asarray(preds, np.float64)
    t = np.asarray(target, np.float64)
    if zero_mean:
        p = p - p.mean(-1, keepdims=True)
        t = t - t.mean(-1, keepdims=True)
    return p, t


def si_sdr(preds, target, zero_mean=False):
    p, t = _centred(preds, target, zero_mean)
    return M.si_sdr(p, t)


def si_snr(preds, target):
    return si_sdr(preds, target, zero_mean=True)


def snr(preds, target, zero_mean=False):
    p, t = _centred(preds, target, zero_mean)
    eps = float(np.finfo(np.float32).eps)
    noise = t - p
    return 10 * np.log10(((t * t).sum(-1) + eps) / ((noise * noise).sum(-1) + eps))


def log_power(x, n_fft, hop, dtype=torch.float64):
    """log10 clamp(|stft|^2, 1e-8) of a 1-D signal: (n_fft // 2 + 1, 1 + len // hop), in ``dtype`` throughout."""
    s = torch.as_tensor(np.asarray(x)).to(dtype)
    spec = torch.stft(s, n_fft, hop, n_fft, torch.hann_window(n_fft, dtype=dtype), center=True, pad_mode="reflect", return_complex=True)
    return spec.abs().square().clamp(min=LSD_FLOOR).log10()


def lsd(preds, target, n_fft=2048, hop=512, bins=None, dtype=torch.float64):
    """LSD of one pair of 1-D signals over the bins [k_lo, k_hi) (None: all), as a float."""
    lo, hi = (0, n_fft // 2 + 1) if bins is None else bins
    d = (log_power(preds, n_fft, hop, dtype) - log_power(target, n_fft, hop, dtype))[lo:hi]
    return float(d.square().mean(0).sqrt().mean().double())
