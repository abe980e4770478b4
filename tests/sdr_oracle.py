"""Float64 restatement of the BSS-eval signal-to-distortion ratio (test-only), per row alone, and the inputs of its tests.

The quantity is torchmetrics 1.x ``signal_distortion_ratio(preds, target, use_cg_iter=None, filter_length=512, zero_mean=False,
load_diag=None)``, direct-solve branch, restated from memory of its published source: torchmetrics is NOT installed here, so the
restatement is unpinned (like the pystoi and auraloss restatements of the neighbouring oracles).  For one row of N samples:

1. ``t = target``, ``p = preds``; with ``zero_mean`` each minus its mean over the row's own N samples.
2. ``t <- t / max(||t||, 1e-6)``, ``p <- p / max(||p||, 1e-6)``.
3. ``r[k] = sum_n t[n] t[n + k]`` and ``b[k] = sum_n t[n] p[n + k]`` for k = 0 .. L - 1: linear correlations, 0 for k >= N.
4. ``r[0] += load_diag`` when it is given.
5. ``Toeplitz(r) h = b``, ``coh = b . h``, value ``10 log10(coh / (1 - coh))``.

Two routes that share nothing past step 2: ``"fft"`` forms the correlations by a zero-padded ``rfft`` long enough not to wrap (as
torchmetrics does) and solves the dense Toeplitz matrix with ``numpy.linalg.solve``; ``"direct"`` forms them as plain sums and solves
with ``scipy.linalg.solve_toeplitz`` (Levinson).  ``oracle_spread`` is their largest disagreement in dB on the inputs of the GPU tests:
the oracle's own error, which the tests' bar is built from.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.linalg
import scipy.signal

FILTER_LENGTHS = (1, 7, 16, 64, 512)
SETTINGS = ((False, None), (True, None), (False, 1e-3))     # (zero_mean, load_diag)
KINDS = ("fir", "speech")
DC = 0.3                       # offset of the rows scored with zero_mean
COMPARED = (-30.0, 60.0)       # dB: rows whose oracle value lies inside are held to the bar


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def prepare(preds, target, zero_mean=False):
    """Steps 1 and 2."""
    t, p = np.asarray(target, np.float64), np.asarray(preds, np.float64)
    if zero_mean:
        t, p = t - t.mean(), p - p.mean()
    return p / max(math.sqrt(float((p * p).sum())), 1e-6), t / max(math.sqrt(float((t * t).sum())), 1e-6)


def correlations_fft(p, t, L):
    n_fft = 1 << max(0, math.ceil(math.log2(len(t) + L - 1)))
    tf, pf = np.fft.rfft(t, n_fft), np.fft.rfft(p, n_fft)
    r = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n_fft)[:L]
    b = np.fft.irfft(np.conj(tf) * pf, n_fft)[:L]
    return r, b


def correlations_direct(p, t, L):
    n = len(t)
    r, b = np.zeros(L), np.zeros(L)
    for k in range(min(L, n)):
        r[k] = np.dot(t[: n - k], t[k:])
        b[k] = np.dot(t[: n - k], p[k:])
    return r, b


def sdr(preds, target, filter_length=512, zero_mean=False, load_diag=None, route="fft"):
    """The five steps on one row; NaN / inf where the arithmetic gives them (no eps anywhere)."""
    p, t = prepare(preds, target, zero_mean)
    L = int(filter_length)
    with np.errstate(all="ignore"):
        if route == "fft":
            r, b = correlations_fft(p, t, L)
        else:
            r, b = correlations_direct(p, t, L)
        if load_diag is not None:
            r = r.copy()
            r[0] += load_diag
        if r[0] == 0 or not np.isfinite(r).all():
            return float("nan")
        if route == "fft":
            h = np.linalg.solve(scipy.linalg.toeplitz(r), b)
        else:
            h = scipy.linalg.solve_toeplitz(r, b)
        coh = float(np.dot(b, h))
        return float(10.0 * np.log10(np.float64(coh) / np.float64(1.0 - coh)))


def si_sdr_no_eps(preds, target, zero_mean=False):
    """Closed form of L = 1: coh = rho^2, so 10 log10(rho^2 / (1 - rho^2)) -- written as SI-SDR's projection, without its eps."""
    t, p = np.asarray(target, np.float64), np.asarray(preds, np.float64)
    if zero_mean:
        t, p = t - t.mean(), p - p.mean()
    alpha = np.dot(p, t) / np.dot(t, t)
    e = p - alpha * t
    return float(10.0 * np.log10(alpha * alpha * np.dot(t, t) / np.dot(e, e)))


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------------
def row_lengths(L, S):
    """1, a row shorter than 512 lags, the segment boundary, the halo that crosses it and the row's end, and a third segment; repeats
    dropped."""
    out = []
    for n in (1, 300, S - 1, S, S + 1, S + L - 1, S + L, 2 * S + 5):
        if n not in out:
            out.append(n)
    return out


def _speech(rng, n):
    """White noise through a 4th-order low-pass at 0.08 of Nyquist plus 1e-3 of the noise: the Toeplitz matrix of 512 lags has a
    condition number around 3e5."""
    w = rng.randn(n)
    bb, aa = scipy.signal.butter(4, 0.08)
    return scipy.signal.lfilter(bb, aa, w) + 1e-3 * w


@functools.lru_cache(maxsize=None)
def inputs(kind, L, S, dc=0.0):
    """(targets, preds): one float64 array of float32 values per row of ``row_lengths(L, S)``.
    "fir": white-noise targets, preds the target through a random decaying FIR of min(L, 8) taps plus white noise at 0.1 of its scale.
    "speech": low-passed noise, preds 0.7 of the target rolled by one sample plus 0.05 of another such signal."""
    targets, preds = [], []
    for i, n in enumerate(row_lengths(L, S)):
        rng = np.random.RandomState(1000 * KINDS.index(kind) + 10 * FILTER_LENGTHS.index(L) + i)
        if kind == "fir":
            t = rng.randn(n)
            taps = min(L, 8)
            fir = rng.randn(taps) * 0.6 ** np.arange(taps)
            p = np.convolve(t, fir)[:n] + 0.1 * rng.randn(n)
        else:
            t = _speech(rng, n)
            t /= max(float(np.abs(t).max()), 1e-12)
            other = _speech(rng, n)
            other /= max(float(np.abs(other).max()), 1e-12)
            p = 0.7 * np.roll(t, 1) + 0.05 * other
        targets.append(_f32(t + dc))
        preds.append(_f32(p + dc))
    return targets, preds


def case_inputs(kind, L, S, zero_mean):
    return inputs(kind, L, S, DC if zero_mean else 0.0)


@functools.lru_cache(maxsize=None)
def case(kind, L, S, zero_mean, load_diag):
    """(fft route, direct route): the oracle of every row alone, two (rows,) float64 arrays."""
    targets, preds = case_inputs(kind, L, S, zero_mean)
    both = [[sdr(p, t, L, zero_mean, load_diag, route) for p, t in zip(preds, targets)] for route in ("fft", "direct")]
    return np.array(both[0]), np.array(both[1])


def compared(values):
    with np.errstate(invalid="ignore"):
        return np.isfinite(values) & (values >= COMPARED[0]) & (values <= COMPARED[1])


@functools.lru_cache(maxsize=None)
def oracle_spread(S):
    """The largest |fft route - direct route| in dB over every compared row of every case of the GPU tests."""
    worst = 0.0
    for kind in KINDS:
        for L in FILTER_LENGTHS:
            for zero_mean, load_diag in SETTINGS:
                a, b = case(kind, L, S, zero_mean, load_diag)
                keep = compared(a) & compared(b)
                if keep.any():
                    worst = max(worst, float(np.abs(a[keep] - b[keep]).max()))
    return worst


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
