"""The sample conversions of the PCM encoder in numpy: the oracle of the export tests (no GPU, nothing of vibravox_amd).

With b the bit depth and v = rint(x * 2^(b-1)), rounded half to even in float32 (the product is an exact power-of-two scaling):
PCM16 / PCM24 / PCM32 store v clamped to [-2^(b-1), 2^(b-1) - 1] and 0 for a NaN, little-endian, PCM24 packed in 3 bytes; FLOAT32
stores the bits of x.  A sample counts as clipped when v >= 2^(b-1), v < -2^(b-1) or x is a NaN; FLOAT32 never clips."""
import numpy as np

BITS = {"PCM16": 16, "PCM24": 24, "PCM32": 32, "FLOAT32": 32}
BYTES = {"PCM16": 2, "PCM24": 3, "PCM32": 4, "FLOAT32": 4}


def to_int(x: np.ndarray, fmt: str):
    """``(stored integers as int64, clipped count)`` of the float32 samples ``x`` for one of the three PCM formats."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    scale = np.float32(2.0 ** (BITS[fmt] - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(x * scale)
    assert v.dtype == np.float32
    nan = np.isnan(x)
    high = v >= scale
    low = v < -scale
    wide = v.astype(np.float64)
    wide[nan] = 0.0
    wide = np.clip(wide, -float(scale), float(scale) - 1.0)   # float64 holds every 32-bit bound exactly
    return wide.astype(np.int64), int(np.count_nonzero(nan | high | low))


def encode(x: np.ndarray, fmt: str):
    """``(bytes of the data chunk, clipped count)`` of the float32 samples ``x``."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if fmt == "FLOAT32":
        return x.astype("<f4", copy=False).view(np.uint8).tobytes(), 0
    ints, clipped = to_int(x, fmt)
    if fmt == "PCM16":
        return ints.astype("<i2").tobytes(), clipped
    if fmt == "PCM32":
        return ints.astype("<i4").tobytes(), clipped
    u = (ints & 0xFFFFFF).astype("<u4")
    return u.view(np.uint8).reshape(-1, 4)[:, :3].tobytes(), clipped


def decode(data: bytes, fmt: str) -> np.ndarray:
    """The decoder's conversion of a mono data chunk, float32: x / 2^15, x / 2^23, float32(x) * 2^-31, or the bits."""
    raw = np.frombuffer(data, dtype=np.uint8)
    if fmt == "FLOAT32":
        return raw.view("<f4").copy()
    if fmt == "PCM16":
        return raw.view("<i2").astype(np.float32) / np.float32(32768)
    if fmt == "PCM32":
        return raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    b = raw.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    return v.astype(np.float32) / np.float32(1 << 23)
