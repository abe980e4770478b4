"""CPU (no GPU): the WAVE header writer and the image plan of vibravox_amd.corpus, the properties of the export oracle itself, and the
argument checks of eben_pcm_encode_ragged."""
import ctypes
import io
import os
import wave

import numpy as np
import pytest

from tests import corpus_fixtures as F
from tests import export_oracle as O
from vibravox_amd import corpus


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


# ---- wav_header -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", corpus.FORMATS)
@pytest.mark.parametrize("frames", [0, 1, 37])
def test_wav_header_is_read_back_by_wav_info_and_by_the_wave_module(tmp_path, fmt, frames):
    x = F.samples(fmt, frames, 1, 3)
    head = corpus.wav_header(22050, frames, fmt)
    assert len(head) == corpus.HEADER_BYTES == 44
    body = F.encode(x, fmt)
    p = tmp_path / "a.wav"
    p.write_bytes(head + body)
    assert corpus.wav_info(p) == (22050, 1, frames, fmt, 44, frames * corpus.BYTES_PER_SAMPLE[fmt])
    assert head == open(F.write_wav(tmp_path / "b.wav", x, fmt, 22050), "rb").read()[:44]   # the fixtures' struct.pack header
    if fmt != "FLOAT32":   # the standard library reads PCM only
        with wave.open(io.BytesIO(head + body)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, corpus.BYTES_PER_SAMPLE[fmt], 22050, frames)
            assert w.readframes(frames) == body


def test_wav_header_refuses_what_does_not_fit_32_bits():
    most = (0xFFFFFFFF - 36) // 2
    head = corpus.wav_header(16000, most, "PCM16")
    assert head[4:8] == (36 + 2 * most).to_bytes(4, "little") and head[40:44] == (2 * most).to_bytes(4, "little")
    with pytest.raises(ValueError, match="32-bit"):
        corpus.wav_header(16000, most + 1, "PCM16")
    with pytest.raises(ValueError, match="32-bit"):
        corpus.wav_header(16000, 1 << 30, "FLOAT32")
    with pytest.raises(ValueError, match="format"):
        corpus.wav_header(16000, 10, "PCM8")
    with pytest.raises(ValueError):
        corpus.wav_header(0, 10, "PCM16")
    with pytest.raises(ValueError):
        corpus.wav_header(16000, -1, "PCM16")


# ---- plan_image -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", corpus.FORMATS)
def test_image_plan_aligns_every_data_start_and_keeps_the_budget(fmt):
    counts = [100, 3, 0, 50, 16, 200, 1, 7, 129]
    width = corpus.BYTES_PER_SAMPLE[fmt]
    budget = 48 + 200 * width + 300
    groups = corpus.plan_image(counts, fmt, budget)
    assert len(groups) > 1
    assert groups[0].lo == 0 and groups[-1].hi == len(counts) and all(a.hi == b.lo for a, b in zip(groups, groups[1:]))
    for g in groups:
        assert len(g.starts) == g.hi - g.lo and g.nbytes <= budget and g.nbytes % 16 == 0
        end = 0
        for start, n in zip(g.starts, counts[g.lo:g.hi]):
            assert (start + corpus.HEADER_BYTES) % 16 == 0          # where the encoder writes
            assert start >= end                                     # disjoint and in order
            end = start + corpus.HEADER_BYTES + n * width
        assert end <= g.nbytes
    one = corpus.plan_image(counts, fmt, 1 << 20)
    assert len(one) == 1 and (one[0].lo, one[0].hi) == (0, len(counts))
    assert corpus.plan_image([], fmt, 1 << 20) == []
    with pytest.raises(ValueError, match="staging"):
        corpus.plan_image([10, 1000, 10], fmt, 48 + 1000 * width - 1)
    assert len(corpus.plan_image([1000], fmt, 48 + corpus._up(1000 * width))) == 1   # exactly fits alone


# ---- the oracle's own properties ------------------------------------------------------------------------------------------------------------
def test_oracle_round_trips_every_pcm16_and_pcm24_code():
    for fmt, bits in (("PCM16", 16), ("PCM24", 24)):
        codes = np.arange(-(1 << (bits - 1)), 1 << (bits - 1), dtype=np.int64).reshape(-1, 1)
        raw = F.encode(codes, fmt)
        x = F.oracle(codes, fmt, 0)
        assert np.array_equal(x, O.decode(raw, fmt))       # the two decoders agree
        again, clipped = O.encode(x, fmt)
        assert again == raw and clipped == 0


def test_oracle_pcm32_decode_encode_decode_is_decode():
    codes = F.samples("PCM32", 200000, 1, 11)
    x = F.oracle(codes, "PCM32", 0)
    raw, clipped = O.encode(x, "PCM32")
    # a code within 64 of the top decodes to 1.0, which does not fit PCM32 again: it clips to the largest code, which decodes to 1.0
    assert clipped == int(np.count_nonzero(x == np.float32(1.0)))
    assert np.array_equal(O.decode(raw, "PCM32"), x)


def test_oracle_rounds_half_way_cases_to_even():
    k = np.array([-32768, -32767, -3, -2, -1, 0, 1, 2, 3, 100, 101, 32765, 32766], dtype=np.int64)
    x = ((k.astype(np.float64) + 0.5) / 32768).astype(np.float32)          # exact in float32
    assert np.array_equal(x.astype(np.float64) * 32768, k + 0.5)
    ints, clipped = O.to_int(x, "PCM16")
    want = np.where(k % 2 == 0, k, k + 1)                                   # the even neighbour of k + 0.5
    assert np.array_equal(ints, want) and clipped == 0
    ints, clipped = O.to_int(np.array([(32767 + 0.5) / 32768], dtype=np.float32), "PCM16")   # rounds to 32768: out of range
    assert ints.tolist() == [32767] and clipped == 1


SPECIAL = np.array([1.0, -1.0, np.inf, -np.inf, np.nan, -0.0, 1e-45], dtype=np.float32)   # the last: the smallest denormal


@pytest.mark.parametrize("fmt", ["PCM16", "PCM24", "PCM32"])
def test_oracle_special_values(fmt):
    b = O.BITS[fmt]
    top, bottom = (1 << (b - 1)) - 1, -(1 << (b - 1))
    ints, clipped = O.to_int(SPECIAL, fmt)
    assert ints.tolist() == [top, bottom, top, bottom, 0, 0, 0]
    assert clipped == 4                                                     # 1.0, +inf, -inf and the NaN; -1.0 is a code
    raw, n = O.encode(SPECIAL, fmt)
    assert n == 4 and len(raw) == len(SPECIAL) * O.BYTES[fmt]


def test_oracle_float32_keeps_the_bits():
    raw, clipped = O.encode(SPECIAL, "FLOAT32")
    assert clipped == 0 and raw == SPECIAL.view(np.uint8).tobytes()
    assert np.array_equal(O.decode(raw, "FLOAT32").view(np.uint32), SPECIAL.view(np.uint32))


# ---- the entry point's argument checks ---------------------------------------------------------------------------------------------------
def _table(*rows):
    t = np.zeros(len(rows), dtype=corpus.ENC_ROW_DTYPE)
    for k, r in enumerate(rows):
        t[k] = r
    return t


def test_encode_tile_is_exposed_without_gpu(lib):
    from vibravox_amd import _lib

    tile = _lib.pcm_encode_tile()
    assert tile >= 8 and tile % 8 == 0
    assert lib.eben_pcm_encode_plan(None, 1) == -1 and lib.eben_pcm_encode_plan((ctypes.c_int * 1)(), 0) == -1


def test_encode_refuses_bad_arguments_without_gpu(lib):
    """Every call is refused on the host (EBEN_EINVAL and a message) before any launch: the device pointers are made up and never
    dereferenced, only the host table is read."""
    from vibravox_amd._lib import PCM_F32, PCM_S16, PCM_S24, PCM_S32, EbenPcmEncRow

    assert ctypes.sizeof(EbenPcmEncRow) == corpus.ENC_ROW_DTYPE.itemsize == 24
    P = ctypes.c_void_p
    # (src_offset, byte_offset, samples, format): rows in shuffled image order, sources anywhere on the 4-byte grid
    ok_rows = _table((1, 512, 100, PCM_S16), (103, 0, 30, PCM_S24), (135, 96, 7, PCM_F32), (150, 128, 50, PCM_S32))
    good = dict(src=P(0x10000), src_floats=200, rows=ok_rows, rows_dev=P(0x20000), image=P(0x30000), image_bytes=712, clipped=P(0x40000), n=4)

    def call(**kw):
        a = dict(good, **kw)
        rows_host = a["rows"].ctypes.data if isinstance(a["rows"], np.ndarray) else a["rows"]
        return lib.eben_pcm_encode_ragged(a["src"], a["src_floats"], rows_host, a["rows_dev"], a["image"], a["image_bytes"], a["clipped"], a["n"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in lib.eben_last_error(), (kw, lib.eben_last_error())

    for name in ("src", "rows", "rows_dev", "image", "clipped"):
        refused(b"null", **{name: None})
    for name, bad in (("image", 0x30008), ("rows_dev", 0x20004), ("src", 0x10002), ("clipped", 0x40002)):
        refused(b"misaligned", **{name: P(bad)})
    for n in (0, -1, 65536):
        refused(b"rows", n=n)
    refused(b"unknown format", rows=_table((0, 0, 10, 4)), n=1)
    refused(b"unknown format", rows=_table((0, 0, 10, -1)), n=1)
    refused(b"samples", rows=_table((0, 0, -1, PCM_S16)), n=1)
    refused(b"multiple of 16", rows=_table((0, 8, 10, PCM_S16)), n=1)               # a misaligned byte offset
    refused(b"multiple of 16", rows=_table((0, -16, 10, PCM_S16)), n=1)
    refused(b"source of 200", rows=_table((191, 0, 10, PCM_S16)), n=1)              # a row past the source
    refused(b"source of 200", rows=_table((-1, 0, 10, PCM_S16)), n=1)
    refused(b"source of 199", src_floats=199)                                       # the last row of the good table ends at float 200
    refused(b"image of 712", rows=_table((0, 704, 5, PCM_S16)), n=1)                # 10 bytes from 704: a row past the image
    refused(b"image of 711", image_bytes=711)                                       # the first row of the good table ends at byte 712
    refused(b"overlap", rows=_table((0, 16, 10, PCM_S16), (10, 0, 9, PCM_S16)), n=2)     # bytes [16, 36) and [0, 18), given out of order
    refused(b"overlap", rows=_table((0, 0, 9, PCM_S32), (10, 32, 10, PCM_S16)), n=2)     # bytes [0, 36) and [32, 52)
    refused(b"overlap", rows=_table((0, 0, 10, PCM_S16), (0, 0, 10, PCM_S16)), n=2)      # the same place twice
