"""Float64 restatement of the frame-based objective speech measures (test-only), one row at a time, and the inputs of their tests.

Segmental SNR, frequency-weighted segmental SNR, LPC log-likelihood ratio and LPC cepstral distance after Hu & Loizou (2008), the
``pysepm`` set without WSS and the composites.  pysepm is NOT installed here: the definitions written out at ``eben_speech_measures`` in
``include/eben_hip.h`` are the contract and this file restates them in numpy (parity with pysepm unpinned).  preds = processed,
target = clean.

Two LPC routes that share nothing past the windowed frame: ``"direct"`` forms R[k] as plain sums and runs the Levinson-Durbin
recursion; ``"toeplitz"`` takes R from a zero-padded FFT and solves the normal equations with ``scipy.linalg.solve_toeplitz``.
``oracle_spread()`` is their largest disagreement per measure over the rows of the GPU tests, ``fw_f32_spread()`` the largest change of
``fw_seg_snr`` when transform, normalisation and band sums are rounded to float32 (``scipy.fft`` transforms complex64 in float32): the
oracle's own errors, which the tests' bars are built from.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.fft
import scipy.linalg
import scipy.signal

EPS = 2.0 ** -52
RATES = (16000, 8000)
KINDS = ("mix", "tilt", "bwe")
NAMES = ("seg_snr", "fw_seg_snr", "llr", "cd")
TILE_FRAMES = 16      # frames of a row per workgroup of the frame kernels (mirrored: vibravox_amd.metrics.MEASURES_TILE_FRAMES)
CENT = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
        1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63)
BW = (70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457,
      199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def geometry(fs):
    """(W, S, P, n_fft)"""
    assert fs in RATES
    w = int(math.floor(0.030 * fs + 0.5))
    return w, w // 4, 16 if fs == 16000 else 10, 1 << int(math.ceil(math.log2(2 * w)))


def frame_count(n, fs):
    w, s, _, _ = geometry(fs)
    return 0 if n < w else (n - w) // s


def window(fs):
    w = geometry(fs)[0]
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, w + 1) / (w + 1)))


@functools.lru_cache(maxsize=None)
def band_filters(fs):
    """(25, n2) float64: the Gaussian-shaped critical-band filters, zero where they fall to exp(-30 / 4.606) or below."""
    n2 = geometry(fs)[3] // 2
    j = np.arange(n2, dtype=np.float64)
    out = np.zeros((len(CENT), n2))
    floor_g = math.exp(-30.0 / (2.0 * 2.303))
    for i, (cent, bw) in enumerate(zip(CENT, BW)):
        f0 = math.floor(cent / (fs / 2) * n2)
        bwn = bw / (fs / 2) * n2
        g = np.exp(-11.0 * ((j - f0) / bwn) ** 2 + math.log(70.0) - math.log(bw))
        g[g <= floor_g] = 0.0
        out[i] = g
    return out


def autocorr_direct(x, order):
    n = len(x)
    return np.array([np.dot(x[: n - k], x[k:]) for k in range(order + 1)])


def autocorr_fft(x, order):
    n_fft = 1 << int(math.ceil(math.log2(2 * len(x))))
    f = np.fft.rfft(x, n_fft)
    return np.fft.irfft(f.real ** 2 + f.imag ** 2, n_fft)[: order + 1]


def levinson(r, order):
    """Predictor coefficients a_1 .. a_P of the Levinson-Durbin recursion."""
    a = np.zeros(order + 1)
    e = r[0]
    for i in range(1, order + 1):
        acc = 0.0
        for j in range(1, i):
            acc += a[j] * r[i - j]
        k = (r[i] - acc) / e
        prev = a.copy()
        for j in range(1, i):
            a[j] = prev[j] - k * prev[i - j]
        a[i] = k
        e *= 1.0 - k * k
    return a[1:]


def lpc(x, order, route):
    """(R[0 .. P], a_1 .. a_P)"""
    if route == "direct":
        r = autocorr_direct(x, order)
        return r, levinson(r, order)
    r = autocorr_fft(x, order)
    return r, scipy.linalg.solve_toeplitz(r[:order], r[1 : order + 1])


def cepstrum(a):
    order = len(a)
    cep = np.zeros(order + 1)
    cep[1] = a[0]
    for m in range(2, order + 1):
        acc = 0.0
        for k in range(1, m):
            acc += k * cep[k] * a[m - k - 1]
        cep[m] = a[m - 1] + acc / m
    return cep[1:]


def fw_frame(c, p, fs, f32=False):
    """(frame value, the 25 band SNRs before the weighting)"""
    n_fft = geometry(fs)[3]
    n2 = n_fft // 2
    g = band_filters(fs)
    if f32:
        cs = np.abs(scipy.fft.fft(c.astype(np.float32), n_fft)[:n2]).astype(np.float32)
        ps = np.abs(scipy.fft.fft(p.astype(np.float32), n_fft)[:n2]).astype(np.float32)
        assert cs.dtype == np.float32
        cs = cs / cs.sum(dtype=np.float32)
        ps = ps / ps.sum(dtype=np.float32)
        g32 = g.astype(np.float32)
        ec = (g32 * cs[None]).sum(axis=1, dtype=np.float32).astype(np.float64)
        ep = (g32 * ps[None]).sum(axis=1, dtype=np.float32).astype(np.float64)
    else:
        cs = np.abs(np.fft.fft(c, n_fft)[:n2])
        ps = np.abs(np.fft.fft(p, n_fft)[:n2])
        cs = cs / cs.sum()
        ps = ps / ps.sum()
        ec = g @ cs
        ep = g @ ps
    err = np.maximum((ec - ep) ** 2, EPS)
    with np.errstate(divide="ignore"):
        snr = np.clip(10.0 * np.log10(ec ** 2 / err), -10.0, 35.0)
    wgt = ec ** 0.2
    return float((wgt * snr).sum() / wgt.sum()), snr


def trimmed_mean(values):
    """Mean of the (95 F' + 50) // 100 smallest; NaN without a value."""
    if len(values) == 0:
        return float("nan")
    k = (95 * len(values) + 50) // 100
    return float(np.mean(np.sort(np.asarray(values, np.float64))[:k]))


def measures(preds, target, fs, route="direct", fw_f32=False, which=NAMES):
    """The four values of one row (the keys of ``which``) and ``"_clamped"``: the fraction of frames at a seg_snr / llr / cd clamp and of
    (frame, band) values at a fw_seg_snr clamp, ``(seg, fw, llr, cd)``.  A row without a frame is NaN everywhere."""
    w, s, order, _ = geometry(fs)
    x, y = np.asarray(target, np.float64), np.asarray(preds, np.float64)
    assert x.shape == y.shape and x.ndim == 1
    nf = frame_count(len(x), fs)
    out = {name: float("nan") for name in which}
    out["_clamped"] = (0.0, 0.0, 0.0, 0.0)
    if nf < 1:
        return out
    win = window(fs)
    seg, fw, llr, cd = [], [], [], []
    fw_hits, fw_all = 0, 0
    for f in range(nf):
        c, p = win * x[f * s : f * s + w], win * y[f * s : f * s + w]
        cc, pp, dd = float(np.dot(c, c)), float(np.dot(p, p)), float(np.dot(c - p, c - p))
        seg.append(float(np.clip(10.0 * np.log10(cc / (dd + EPS) + EPS), -10.0, 35.0)))
        if cc == 0.0 or pp == 0.0:
            continue
        if "fw_seg_snr" in which:
            value, snr = fw_frame(c, p, fs, fw_f32)
            fw.append(value)
            fw_hits += int(((snr <= -10.0) | (snr >= 35.0)).sum())
            fw_all += snr.size
        if "llr" in which or "cd" in which:
            r_c, a_c = lpc(c, order, route)
            _, a_p = lpc(p, order, route)
            t = scipy.linalg.toeplitz(r_c)
            big_c, big_p = np.concatenate([[1.0], -a_c]), np.concatenate([[1.0], -a_p])
            with np.errstate(all="ignore"):
                llr.append(float(np.minimum(2.0, np.log((big_p @ t @ big_p) / (big_c @ t @ big_c)))))
                d = cepstrum(a_c) - cepstrum(a_p)
                cd.append(float(np.minimum(10.0, 10.0 / math.log(10.0) * math.sqrt(2.0 * float(np.dot(d, d))))))
    seg_a, llr_a, cd_a = np.array(seg), np.array(llr), np.array(cd)
    out["_clamped"] = (float(((seg_a <= -10.0) | (seg_a >= 35.0)).mean()), fw_hits / max(fw_all, 1),
                       float((llr_a >= 2.0).mean()) if len(llr) else 0.0, float((cd_a >= 10.0).mean()) if len(cd) else 0.0)
    if "seg_snr" in which:
        out["seg_snr"] = float(np.mean(seg_a))
    if "fw_seg_snr" in which:
        out["fw_seg_snr"] = float(np.mean(fw)) if fw else float("nan")
    if "llr" in which:
        out["llr"] = trimmed_mean(llr)
    if "cd" in which:
        out["cd"] = trimmed_mean(cd)
    return out


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------------
def row_lengths(fs):
    """F = 1 (the shortest row), the last length with one frame, F = 2, F = 10 (nothing trimmed), F = 11 (the first trimmed frame), the
    last length of one full tile, the first with a frame in a second tile and one more, and two seconds and a bit."""
    w, s, _, _ = geometry(fs)
    edge = w + (TILE_FRAMES + 1) * s
    return [w + s, w + 2 * s - 1, w + 2 * s, w + 10 * s + 7, w + 11 * s, edge - 1, edge, edge + 1, 2 * fs + 13]


def speech(seed, n, fs):
    """A 120 Hz pulse train plus 0.3 of white noise through four resonators (500 / 1500 / 2500 / 3500 Hz, 150 / 200 / 300 / 400 Hz wide),
    a 3 Hz tremolo, peak-normalised, plus 1e-3 of white noise; float32 values."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / fs
    x = 0.3 * rng.randn(n)
    period = fs / 120.0
    x[np.unique(np.floor(np.arange(0, n / period) * period).astype(int).clip(0, n - 1))] += 1.0
    for f, bw in ((500.0, 150.0), (1500.0, 200.0), (2500.0, 300.0), (3500.0, 400.0)):
        r = math.exp(-math.pi * bw / fs)
        x = scipy.signal.lfilter([1.0], [1.0, -2.0 * r * math.cos(2.0 * math.pi * f / fs), r * r], x)
    x = x * (0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t))
    x = x / max(float(np.abs(x).max()), 1e-12)
    return _f32(x + 1e-3 * rng.randn(n))


def degrade(kind, t, o, seed):
    """``mix``: 0.8 t + 0.2 o.  ``tilt``: t through the FIR [1, -0.3] plus 3e-4 of white noise.  ``bwe``: a 4th-order Butterworth low-pass
    of t at half Nyquist plus half of what the same low-pass leaves of o."""
    rng = np.random.RandomState(seed)
    if kind == "mix":
        return _f32(0.8 * t + 0.2 * o)
    if kind == "tilt":
        return _f32(scipy.signal.lfilter([1.0, -0.3], [1.0], t) + 3e-4 * rng.randn(len(t)))
    b, a = scipy.signal.butter(4, 0.5)
    return _f32(scipy.signal.lfilter(b, a, t) + 0.5 * (o - scipy.signal.lfilter(b, a, o)))


@functools.lru_cache(maxsize=None)
def inputs(fs):
    """(targets, preds, labels): one float64 array of float32 values per (kind, length) of the tests, kinds outermost."""
    targets, preds, labels = [], [], []
    for ki, kind in enumerate(KINDS):
        for i, n in enumerate(row_lengths(fs)):
            seed = 7000 + 100 * RATES.index(fs) * len(KINDS) + 100 * ki + i
            t, o = speech(seed, n, fs), speech(seed + 50, n, fs)
            targets.append(t)
            preds.append(degrade(kind, t, o, seed + 77))
            labels.append((kind, n))
    return targets, preds, labels


@functools.lru_cache(maxsize=None)
def table(fs, route="direct", fw_f32=False):
    """The oracle of every row of ``inputs(fs)`` alone: a list of ``measures`` dicts."""
    targets, preds, _ = inputs(fs)
    which = NAMES if not fw_f32 else ("fw_seg_snr",)
    return [measures(p, t, fs, route, fw_f32, which) for t, p in zip(targets, preds)]


@functools.lru_cache(maxsize=None)
def oracle_spread():
    """{measure: the largest |direct route - toeplitz route| over every row of the GPU tests, both rates}"""
    worst = {name: 0.0 for name in NAMES}
    for fs in RATES:
        for a, b in zip(table(fs, "direct"), table(fs, "toeplitz")):
            for name in NAMES:
                worst[name] = max(worst[name], abs(a[name] - b[name]))
    return worst


@functools.lru_cache(maxsize=None)
def fw_f32_spread():
    """The largest change of a row's fw_seg_snr when transform, normalisation and band sums are rounded to float32."""
    return max(abs(a["fw_seg_snr"] - b["fw_seg_snr"]) for fs in RATES for a, b in zip(table(fs), table(fs, "direct", True)))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bar(name, oracle):
    """|device - oracle| allowed: one float32 ulp of the value (the output is a float32) plus the oracle's own error -- a hundred times
    the two routes' disagreement (a third summation order), for fw_seg_snr four times the float32 spread (the kernel's transform is
    float32 in another butterfly order than pocketfft's)."""
    own = 4.0 * fw_f32_spread() if name == "fw_seg_snr" else 100.0 * oracle_spread()[name]
    return ulp32(oracle) + own
