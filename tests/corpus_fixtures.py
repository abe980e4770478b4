"""WAVE files written with struct.pack and their numpy conversion: the fixtures and the oracle of the corpus tests (no GPU, nothing
of vibravox_amd).  A file's content is an integer (PCM) or float32 (FLOAT32) array of shape (frames, channels)."""
import os
import struct

import numpy as np

BITS = {"PCM16": 16, "PCM24": 24, "PCM32": 32, "FLOAT32": 32}
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def samples(fmt: str, frames: int, channels: int, seed: int) -> np.ndarray:
    """Seeded content covering the format's whole range; the extremes come first when there is room."""
    rng = np.random.default_rng(seed)
    if fmt == "FLOAT32":
        x = rng.standard_normal((frames, channels)).astype(np.float32)
        edge = [np.float32(-1.0), np.float32(1.0), np.float32(1e-30), np.float32(-0.0)]
    else:
        b = BITS[fmt]
        x = rng.integers(-(1 << (b - 1)), 1 << (b - 1), size=(frames, channels), dtype=np.int64)
        edge = [-(1 << (b - 1)), (1 << (b - 1)) - 1, -1, 0, (1 << (b - 1)) - 129]   # the last: a PCM32 value that float32 must round
    flat = x.reshape(-1)
    flat[:min(len(edge), flat.size)] = edge[:flat.size]
    return x


def encode(x: np.ndarray, fmt: str) -> bytes:
    if fmt == "FLOAT32":
        return x.astype("<f4").tobytes()
    if fmt == "PCM16":
        return x.astype("<i2").tobytes()
    if fmt == "PCM32":
        return x.astype("<i4").tobytes()
    u = (x.reshape(-1).astype(np.int64) & 0xFFFFFF).astype("<u4")
    return u.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def oracle(x: np.ndarray, fmt: str, channel: int) -> np.ndarray:
    """The conversions the issue states, in numpy: float32 of one channel."""
    c = x[:, channel]
    if fmt == "FLOAT32":
        return c.astype(np.float32)
    if fmt == "PCM16":
        return c.astype(np.float32) / np.float32(32768)
    if fmt == "PCM24":
        return c.astype(np.float32) / np.float32(1 << 23)
    return c.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -31)


def write_wav(path, x: np.ndarray, fmt: str, rate: int, *, extensible: bool = False, before_data=(), data_size=None, tag=None, bits=None,
              riff: bytes = b"RIFF") -> str:
    """``before_data``: (id, payload) chunks between fmt and data (an odd payload gets its pad byte); ``data_size``: the size field of the
    data chunk when it is to lie (0, 0xFFFFFFFF); ``tag`` / ``bits``: overrides for files the reader must refuse."""
    frames, channels = x.shape
    body = encode(x, fmt) if fmt in BITS else x.tobytes()
    bits = bits if bits is not None else BITS[fmt]
    tag = tag if tag is not None else (3 if fmt == "FLOAT32" else 1)
    block = channels * bits // 8
    core = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        core += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + _GUID_TAIL
    chunks = b"fmt " + struct.pack("<I", len(core)) + core
    for cid, payload in before_data:
        chunks += cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    chunks += b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body
    os.makedirs(os.path.dirname(os.fspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(riff + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return os.fspath(path)
