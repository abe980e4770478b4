"""Float64 oracle of the integrated loudness of ITU-R BS.1770-4 (one channel), every row alone, with numpy and ``scipy.signal.lfilter``;
test code, imported by ``tests/test_loudness_oracle.py`` (CPU) and the GPU tests of ``csrc/loudness.hip``.

Two routes through the K-weighting: ``"cascade"`` filters section after section, ``"single"`` filters once with the two sections'
polynomials convolved into one fourth-order filter.  Their disagreement over the rows the GPU tests use is ``oracle_spread()``, the unit
the GPU tests build their bar from.  The coefficient formulas are written out here a second time, on their own, from the definition in
``include/eben_hip.h`` (``metrics.k_weighting_coefficients`` is checked against them)."""
import functools
import math

import numpy as np
from scipy.signal import lfilter

RATES = (16000, 44100, 48000)
CHUNK = 4096          # csrc/loudness.hip LD_CHUNK
ABSOLUTE_GATE = -70.0

#: the coefficients the recommendation prints for 48 kHz (BS.1770-4, tables 1 and 2): b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high-pass
TABLE_48K_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
TABLE_48K_HIGHPASS = (-1.99004745483398, 0.99007225036621)


def coefficients(fs):
    """``(b, a)`` of the shelf and of the high-pass, float64."""
    f0, g, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = np.tan(np.pi * f0 / fs)
    vh = np.power(10.0, g / 20.0)
    vb = np.power(vh, 0.4996667741545416)
    a0 = 1.0 + k / q + k * k
    shelf = (np.array([(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0]),
             np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]))
    f0, q = 38.13547087602444, 0.5003270373238773
    k = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]))
    return shelf, highpass


def weighted(x, fs, route="cascade"):
    x = np.asarray(x, dtype=np.float64)
    (b1, a1), (b2, a2) = coefficients(fs)
    if route == "cascade":
        return lfilter(b2, a2, lfilter(b1, a1, x))
    assert route == "single"
    return lfilter(np.convolve(b1, b2), np.convolve(a1, a2), x)


def block_count(n, fs):
    h = fs // 10
    return max(0, (n - 4 * h) // h + 1)


def blocks(x, fs, route="cascade"):
    """``z_j`` of every block that lies wholly inside ``x``."""
    h = fs // 10
    y = weighted(x, fs, route) if len(x) else np.zeros(0)
    return np.array([np.mean(np.square(y[j * h : j * h + 4 * h])) for j in range(block_count(len(x), fs))], dtype=np.float64)


def lk(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def gated(z):
    """``(L, l_j, relative gate, kept mask)`` of the block energies ``z``."""
    l = lk(z)
    above = l > ABSOLUTE_GATE
    if not above.any():
        return -math.inf, l, math.nan, above
    rel = float(lk(np.mean(z[above]))) - 10.0
    kept = above & (l > rel)
    return (float(lk(np.mean(z[kept]))) if kept.any() else -math.inf), l, rel, kept


def loudness(x, fs, route="cascade"):
    return gated(blocks(x, fs, route))[0]


def peak(x):
    return float(np.max(np.abs(np.asarray(x, dtype=np.float32)))) if len(x) else 0.0


def gain(level, pk, target=-23.0, ceiling_db=-1.0):
    """The float64 formula, before its rounding to float32."""
    if not math.isfinite(level) or pk == 0.0:
        return 1.0
    g = 10.0 ** ((target - level) / 20.0)
    ceiling = 10.0 ** (ceiling_db / 20.0)
    return ceiling / pk if g * pk > ceiling else g


def ulp32(v):
    """One float32 unit in the last place at the magnitude of ``v`` (float64 array)."""
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def row_lengths(fs):
    """The smallest lengths at which each loop of the kernels can go wrong: one sample short of a block, one block, around the second,
    the first chunk's edge (no block yet at these rates: the peak alone), the first chunk edge behind a whole block, about a second
    (several chunks, the carry) and three seconds (both gates drop blocks)."""
    h = fs // 10
    n = 4 * h
    edge = -(-n // CHUNK) * CHUNK
    return [n - 1, n, n + h - 1, n + h, CHUNK - 1, CHUNK, CHUNK + 1, edge - 1, edge, edge + 1, fs + 37, 3 * fs]


def gated_noise(n, fs, seed):
    """Seeded float32 noise at 0.1 rms with, where the row is long enough for them, one stretch 85 dB down (under the absolute gate) and
    one 24 dB down (under the relative gate), each 0.7 s: every block that meets a stretch's edge stays clear of both gates."""
    x = (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    if n >= 3 * fs:
        a, b, w = int(0.6 * fs), int(1.8 * fs), int(0.7 * fs)
        x[a : a + w] *= np.float32(10.0 ** (-85.0 / 20.0))
        x[b : b + w] *= np.float32(10.0 ** (-24.0 / 20.0))
    return x


@functools.lru_cache(maxsize=None)
def inputs(fs):
    """The rows of the GPU tests at ``fs``: float32 arrays, one per entry of ``row_lengths``."""
    return tuple(gated_noise(n, fs, 1000 + fs % 997 + r) for r, n in enumerate(row_lengths(fs)))


@functools.lru_cache(maxsize=None)
def table(fs, route="cascade"):
    """Per row of ``inputs(fs)``: ``(L, peak)``."""
    return tuple((loudness(x, fs, route), peak(x)) for x in inputs(fs))


@functools.lru_cache(maxsize=None)
def oracle_spread():
    """The largest disagreement of the two routes over every row of every rate whose loudness is finite, in LU."""
    worst = 0.0
    for fs in RATES:
        for (a, _), (b, _) in zip(table(fs, "cascade"), table(fs, "single")):
            if math.isfinite(a) or math.isfinite(b):
                worst = max(worst, abs(a - b))
    return worst


def bar(oracle):
    """``ulp32(oracle) + 100 * ORACLE_SPREAD``: the result is the float32 rounding of a float64 value, computed in a third order."""
    return ulp32(oracle) + 100.0 * oracle_spread()
