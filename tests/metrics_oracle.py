"""Float64 NumPy/SciPy restatement of the two validation metrics ``base_se.py`` logs (test-only).

* SI-SDR: ``torchmetrics.functional.scale_invariant_signal_distortion_ratio(preds, target, zero_mean=False)``.
* STOI: ``torchmetrics.functional.short_time_objective_intelligibility(preds, target, fs, extended=False)``, which calls
  ``pystoi.stoi(target, preds, fs)`` per clip (clean = target).  The pystoi 0.4.x conventions are restated from its
  published source; pystoi is not installed here, so this is NOT a pin against pystoi.  Every convention that a later
  pin could need to flip is a named switch in ``CONVENTIONS``.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME = 256
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40
EPS = np.finfo(np.float64).eps

CONVENTIONS = dict(
    frame_end_exclusive=True,     # frames start at range(0, len(x) - N_FRAME, hop): the end bound is excluded
    resample_gain_up=True,        # resample_poly multiplies an array window by `up` before filtering
    min_frames_value=1e-5,        # pystoi's return value when fewer than N STFT frames are left
)


def si_sdr(preds, target):
    """(..., T) -> (...), float64."""
    p = np.asarray(preds, np.float64)
    t = np.asarray(target, np.float64)
    eps = float(np.finfo(np.float32).eps)
    alpha = ((p * t).sum(-1, keepdims=True) + eps) / ((t * t).sum(-1, keepdims=True) + eps)
    ts = alpha * t
    noise = ts - p
    return 10 * np.log10(((ts * ts).sum(-1) + eps) / ((noise * noise).sum(-1) + eps))


def hanning_window(n=N_FRAME):
    return np.hanning(n + 2)[1:-1]


def resample_filter(fs):
    """(h, p, q): pystoi ``resample_oct(x, FS, fs)``'s Kaiser-windowed sinc, normalised to unit sum; p/q reduced."""
    g = math.gcd(FS, int(fs))
    p, q = FS // g, int(fs) // g
    stopband = 1.0 / (2 * max(p, q))
    roll_off = stopband / 10
    rejection_db = 60.0
    L = math.ceil((rejection_db - 8) / (28.714 * roll_off))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stopband * np.sinc(2 * stopband * t)
    beta = 0.1102 * (rejection_db - 8.7)
    h = np.kaiser(2 * L + 1, beta) * ideal
    return h / h.sum(), p, q


def resample(x, fs):
    """pystoi resample_oct: scipy.signal.resample_poly(x, p, q, window=h)."""
    if int(fs) == FS:
        return np.asarray(x, np.float64)
    h, p, q = resample_filter(fs)
    if not CONVENTIONS["resample_gain_up"]:
        h = h / p   # resample_poly multiplies by p again
    return resample_poly(np.asarray(x, np.float64), p, q, window=h)


def resample_direct(x, fs):
    """The same resampling written as the polyphase sum the kernel evaluates: out[n] = sum_m x[m] * p*h[L + n*q - m*p]."""
    h, p, q = resample_filter(fs)
    x = np.asarray(x, np.float64)
    L = (len(h) - 1) // 2
    n_out = -(-len(x) * p // q)
    out = np.zeros(n_out)
    for n in range(n_out):
        m = np.arange(max(0, -(-(n * q - L) // p)), min(len(x) - 1, (n * q + L) // p) + 1)
        out[n] = np.dot(x[m], p * h[L + n * q - m * p])
    return out


def frame_starts(length, framelen=N_FRAME, hop=N_FRAME // 2):
    end = length - framelen if CONVENTIONS["frame_end_exclusive"] else length - framelen + 1
    return list(range(0, max(end, 0), hop))


def kept_frames(x, dyn_range=DYN_RANGE, framelen=N_FRAME, hop=N_FRAME // 2):
    """Indices of the frames of the clean signal that survive silence removal."""
    w = hanning_window(framelen)
    starts = frame_starts(len(x), framelen, hop)
    if not starts:
        return np.zeros(0, np.int64)
    e = np.array([20 * np.log10(np.linalg.norm(w * x[i:i + framelen]) + EPS) for i in starts])
    return np.nonzero((e.max() - dyn_range - e) < 0)[0]


def overlap_add(frames, hop=N_FRAME // 2):
    """pystoi's _overlap_and_add (reshape form)."""
    num_frames, framelen = frames.shape
    segments = -(-framelen // hop)
    f = np.pad(frames, ((0, segments), (0, segments * hop - framelen)))
    f = f.reshape((num_frames + segments, segments, hop)).transpose((1, 0, 2)).reshape((-1, hop))[:-segments]
    return f.reshape((segments, num_frames + segments - 1, hop)).sum(0).reshape((-1,))


def overlap_add_loop(frames, hop=N_FRAME // 2):
    num_frames, framelen = frames.shape
    out = np.zeros((num_frames - 1) * hop + framelen)
    for i in range(num_frames):
        out[i * hop:i * hop + framelen] += frames[i]
    return out


def remove_silent_frames(x, y):
    w = hanning_window()
    keep = kept_frames(x)
    starts = frame_starts(len(x))
    xf = np.array([w * x[starts[k]:starts[k] + N_FRAME] for k in keep]).reshape(-1, N_FRAME)
    yf = np.array([w * y[starts[k]:starts[k] + N_FRAME] for k in keep]).reshape(-1, N_FRAME)
    return overlap_add(xf), overlap_add(yf)


def stft(x):
    w = hanning_window()
    starts = frame_starts(len(x))
    return np.array([np.fft.rfft(w * x[i:i + N_FRAME], n=NFFT) for i in starts]).reshape(-1, NFFT // 2 + 1)


def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """(obm (bands, nfft/2+1), edges (bands, 2) as [lo, hi) bin indices)."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi = min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    edges = np.zeros((num_bands, 2), np.int64)
    for i in range(num_bands):
        a = int(np.argmin(np.square(f - lo[i])))
        b = int(np.argmin(np.square(f - hi[i])))
        obm[i, a:b] = 1
        edges[i] = a, b
    return obm, edges


def stoi_clip(x, y, fs):
    """pystoi.stoi(x=clean, y=processed, fs, extended=False), float64."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if x.shape != y.shape:
        raise ValueError("x and y should have the same length")
    x, y = resample(x, fs), resample(y, fs)
    x, y = remove_silent_frames(x, y)
    xs, ys = stft(x).T, stft(y).T
    if xs.shape[-1] < N:
        return CONVENTIONS["min_frames_value"]
    obm, _ = thirdoct()
    xt = np.sqrt(obm @ np.abs(xs) ** 2)
    yt = np.sqrt(obm @ np.abs(ys) ** 2)
    xseg = np.array([xt[:, m - N:m] for m in range(N, xt.shape[1] + 1)])
    yseg = np.array([yt[:, m - N:m] for m in range(N, xt.shape[1] + 1)])
    c = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
    yp = np.minimum(yseg * c, xseg * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(2, keepdims=True)
    xseg = xseg - xseg.mean(2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xseg = xseg / (np.linalg.norm(xseg, axis=2, keepdims=True) + EPS)
    J, M = xseg.shape[0], xseg.shape[1]
    return float((yp * xseg).sum() / (J * M))


def stoi(preds, target, fs):
    """torchmetrics argument order: (..., T) -> (...), float64."""
    p = np.asarray(preds, np.float64)
    t = np.asarray(target, np.float64)
    lead = p.shape[:-1]
    p2, t2 = p.reshape(-1, p.shape[-1]), t.reshape(-1, t.shape[-1])
    return np.array([stoi_clip(t2[i], p2[i], fs) for i in range(p2.shape[0])]).reshape(lead)


def speech_like(key, rows, t, fs, seed=0):
    """Formula-hash 'speech': noise under per-row syllable envelopes with silent stretches, so that silence removal keeps
    a different number of frames on every row.  Deterministic, no RNG state."""
    n = np.arange(t, dtype=np.float64)
    out = np.zeros((rows, t))
    for r in range(rows):
        h = (np.sin(n * 12.9898 + (r + 1) * 78.233 + seed * 3.7 + len(key)) * 43758.5453) % 1.0 - 0.5
        car = np.sin(2 * np.pi * (180 + 23 * r) * n / fs) + 0.6 * np.sin(2 * np.pi * (730 + 41 * r) * n / fs) + 0.8 * h
        syl = 0.5 + 0.5 * np.sin(2 * np.pi * (2.1 + 0.37 * r) * n / fs + r)
        gate = (np.sin(2 * np.pi * (0.45 + 0.11 * r) * n / fs + 0.7 * r) > -0.2 + 0.02 * (r % 7)).astype(np.float64)
        out[r] = 0.3 * car * syl ** 2 * gate + 1e-5 * h
    return out
