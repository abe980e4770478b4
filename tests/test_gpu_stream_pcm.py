"""Live sessions in and out as PCM at the caller's rate, on the device.  Every criterion is equality: ``eben_stream_pcm_out`` against the
three merged kernels it stands for, ``eben_pcm_chunks_in`` against the corpus decoder, and the drivers against the unchanged drivers with
``augment.resample`` and the merged encoder behind them."""
import functools

import numpy as np
import pytest
import torch

from formula import formula_audio
from tests import export_oracle as E
from tests import pool_oracle as P
from tests import pool_rate_oracle as PR
from tests import ragged_oracle as R
from tests.test_gpu_stream import body, fenced, fences_intact, same_bits
from vibravox_amd import augment, corpus, rate, streaming

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAN, INF = float("nan"), float("inf")
OUT_FREQS = (48000, 44100, 24000, 8000)   # 1:3, 160:441 (its table is read through L2), 2:3 and 2:1 from 16 kHz
FORMATS = corpus.FORMATS
BYTES = (2, 3, 4, 4)
GUARD, FILL = 64, 0xA5


# ---- the raw back end -------------------------------------------------------------------------------------------------------------------
def back_cases():
    """(ratio or -1, prev_off, n_carry, n_new, p0, base0, n_out, end): per ratio the left edge (base0 < 0), a steady odd phase behind a
    carry, end = 1 on a tail of one sample, a single output, no output at all (the tape is still written) and one output more than the
    tile ``eben_stream_pcm_plan`` states; without a ratio 1, 77, 300 and a tile plus one."""
    out = []
    for i, f in enumerate(OUT_FREQS):
        orig, new, width = rate.ratio(16000, f)
        taps = 2 * width + orig
        tile = rate.tile_of_back(orig, new, width)["outputs_per_block"]

        def served(p0, base0, n_out):   # the shortest tape whose right end is not the signal's that serves the piece
            return base0 + ((p0 + n_out - 1) // new) * orig + taps

        p0 = 7 if new == 441 else 1 if new > 1 else 0
        out.append((i, 0, 0, served(0, -width, 200), 0, -width, 200, 0))
        out.append((i, 3, 11, served(p0, 5, 255) + 3 - 11, p0, 5, 255, 0))
        out.append((i, 0, 0, 1, 0, -width, -(-new // orig), 1))
        out.append((i, 9, served(p0, 2, 1) - 1, 1, p0, 2, 1, 0))
        out.append((i, 2, 4, 3, p0, 0, 0, 0))
        out.append((i, 1, 5, served(0, -width, tile + 1) - 5, 0, -width, tile + 1, 0))
    assert rate.tile_of_back(1, 1, 0)["outputs_per_block"] == 1024
    for n in (1, 77, 300, 1025):
        out.append((-1, 0, 0, n, 0, 0, n, 0))
    return out


def source(tag, pieces, sp):
    """Row j is piece j's emitted samples: formula audio scaled by 1.5 (it clamps), with +-1.0 and ties at (m + 0.5) / 2^15 planted; a
    NaN and both infinities too where the bytes do not depend on which NaN an fmaf hands on (integer formats, or no resampling)."""
    x = (formula_audio(tag, len(pieces), sp, amp=1.0) * 1.5).reshape(len(pieces), sp).contiguous()
    for j, p in enumerate(pieces):
        n = p["n_new"]
        for k, v in ((8, 1.0), (9, -1.0), (12, 1000.5 / 32768), (13, -1001.5 / 32768), (14, 32766.5 / 32768), (15, -32768.5 / 32768)):
            if k < n:
                x[j, k] = v
        if n >= 60 and (p["format"] != 3 or p["ratio"] < 0):
            x[j, 30], x[j, 45], x[j, n - 2] = NAN, INF, -INF
    return x


def guarded(nbytes):
    base = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    view = base[GUARD : GUARD + nbytes]
    assert view.data_ptr() % 16 == 0
    return base, view


@pytest.mark.parametrize("slots", [3, 70])
def test_stream_pcm_out_equals_splice_resample_and_encode(hip, slots):
    from vibravox_amd._lib import EbenRatePiece, EbenRateRatio, EbenRateSplice, check, stream

    tiles = [rate.tile_of_back(*rate.ratio(16000, f)) for f in OUT_FREQS]
    assert [t["table_route"] for t in tiles] == [1, 0, 1, 2] and tiles[1]["outputs_per_block"] == 882
    cases = back_cases()
    tp = sp = fp = 2100
    assert max(c[2] + c[3] for c in cases) <= tp and max(c[1] + c[2] for c in cases) <= tp and max(c[6] for c in cases) <= fp
    tables = [rate._table(16000, f, DEV)[0] for f in OUT_FREQS]
    ratios = (EbenRateRatio * 4)(*[EbenRateRatio(t.data_ptr(), *rate.ratio(16000, f), 0) for t, f in zip(tables, OUT_FREQS)])
    per_call = min(slots, 64)
    named = set(range(slots)) if slots == 3 else {(11 * j + 1) % slots for j in range(len(cases))}
    mine = [poisoned(slots, tp, f"pcm_out/{slots}/tape{k}", named) for k in (0, 1)]      # what the new call runs on ...
    theirs = [poisoned(slots, tp, f"pcm_out/{slots}/tape{k}", named) for k in (0, 1)]    # ... and the three merged ones
    fifo = [torch.zeros(slots, fp, device=DEV) for _ in (0, 1)]
    clipped = torch.full((slots,), 5, dtype=torch.int32, device=DEV)
    want_clipped = torch.full((slots,), 5, dtype=torch.int64)
    seen = set()
    for g in range(0, len(cases), per_call):
        pieces, at = [], 0
        for j, c in enumerate(cases[g : g + per_call], start=g):
            slot = j % 3 if slots == 3 else (11 * j + 1) % slots
            fmt = j % 4
            at = -(-at // 16) * 16 + 16 * (j % 2)   # every other piece leaves a gap in front
            pieces.append(dict(slot=slot, src_row=len(pieces), ratio=c[0], tape=(j // 3) % 2, prev_off=c[1], n_carry=c[2], n_new=c[3], p0=c[4], base0=c[5],
                               n_out=c[6], end=bool(c[7]), format=fmt, byte_offset=at))
            at += c[6] * BYTES[fmt]
            seen.add((c[0], fmt))
        src = source(f"pcm_out/{slots}/{g}", pieces, sp).to(DEV)
        base, image = guarded(at + 16)
        want_base, want_image = guarded(at + 16)
        table = rate.pack_back_pieces([rate.BackPiece(**p) for p in pieces])
        check(hip.eben_stream_pcm_out(mine[0][2].data_ptr(), mine[1][2].data_ptr(), tp, slots, src.data_ptr(), sp, len(pieces), ratios, 4, image.data_ptr(),
                                      image.numel(), clipped.data_ptr(), table, len(pieces), stream()), "stream_pcm_out")
        # the same pieces through eben_rate_splice_slots -> eben_resample_slots -> eben_pcm_encode_ragged
        rated = [p for p in pieces if p["ratio"] >= 0]
        if rated:
            t = (EbenRateSplice * len(rated))(*[EbenRateSplice(p["slot"], p["src_row"], p["prev_off"], p["n_carry"], p["n_new"], p["tape"]) for p in rated])
            check(hip.eben_rate_splice_slots(theirs[0][2].data_ptr(), theirs[1][2].data_ptr(), tp, slots, src.data_ptr(), sp, len(pieces), t, len(rated),
                                             stream()), "rate_splice_slots")
            t = (EbenRatePiece * len(rated))(*[EbenRatePiece(len=p["n_carry"] + p["n_new"], p0=p["p0"], base0=p["base0"], n_out=p["n_out"], end=int(p["end"]),
                                                             first_out=0, slot=p["slot"], ratio=p["ratio"], tape=p["tape"], fifo=0) for p in rated])
            check(hip.eben_resample_slots(theirs[0][2].data_ptr(), theirs[1][2].data_ptr(), tp, fifo[0].data_ptr(), fifo[1].data_ptr(), fp, slots, ratios, 4, t,
                                          len(rated), stream()), "resample_slots")
        for group, buf, offset in ((rated, fifo[0], lambda p: p["slot"] * fp), ([p for p in pieces if p["ratio"] < 0], src, lambda p: p["src_row"] * sp)):
            if group:
                rows = np.array([(offset(p), p["byte_offset"], p["n_out"], p["format"]) for p in group], dtype=corpus.ENC_ROW_DTYPE)
                counts = corpus.rows_to_pcm(buf, rows, want_image).cpu()
                for p, c in zip(group, counts):
                    want_clipped[p["slot"]] += int(c)
        assert torch.equal(base.cpu(), want_base.cpu()), g                                   # the bytes, the gaps and the guards
        assert bool((base[:GUARD] == FILL).all()) and bool((base[-GUARD:] == FILL).all())
        for k in (0, 1):
            got = mine[k][1].cpu()
            assert same_bits(got, theirs[k][1].cpu()) and fences_intact(got), (g, k)          # un-named slots and the rest of each pitch included
        assert torch.equal(clipped.cpu().long(), want_clipped), g
    assert seen >= {(r, f) for r in range(4) for f in range(4)} | {(-1, f) for f in range(4)}
    assert int(want_clipped.sum()) > 5 * slots + 20                                           # the data did clamp
    assert not same_bits(mine[0][1].cpu(), mine[0][0]) and not same_bits(mine[1][1].cpu(), mine[1][0])


def poisoned(slots, pitch, tag, named):
    """``fenced`` rows with NaN in every slot that is not named."""
    flat, dev, view = fenced(slots, pitch, tag)
    for r in range(slots):
        if r not in named:
            body(flat, slots, pitch)[r] = NAN
            view[r] = NAN
    return flat, dev, view


def test_stream_pcm_out_refuses_bad_arguments_and_writes_nothing(hip):
    from vibravox_amd._lib import EbenRateRatio, stream

    slots, tp, sp = 4, 200, 60
    t = [fenced(slots, tp, f"pcm_out/bad/tape{k}") for k in (0, 1)]
    fs, ds, vs = fenced(2, sp, "pcm_out/bad/src")
    k = rate._table(16000, 48000, DEV)[0]
    orig, new, width = rate.ratio(16000, 48000)
    assert (orig, new, width) == (1, 3, 7)
    ratios = (EbenRateRatio * 1)(EbenRateRatio(k.data_ptr(), orig, new, width, 0))
    base, image = guarded(4096)
    clipped = torch.full((slots,), 3, dtype=torch.int32, device=DEV)
    # a tape of 100 samples: while it goes on, output n reads up to index (n // 3) + 14, so 255 outputs are served and 259 are not; as the signal's
    # end it serves the outputs whose centre (n // 3) + 7 lies inside it: 279, not 280
    good = dict(slot=1, src_row=0, ratio=0, tape=1, prev_off=10, n_carry=40, n_new=60, p0=0, base0=0, n_out=255, end=False, format=1, byte_offset=16)
    plain = dict(slot=2, src_row=1, ratio=-1, tape=0, prev_off=0, n_carry=0, n_new=50, p0=0, base0=0, n_out=50, end=False, format=0, byte_offset=1024)

    def call(descs, count=None, slots=slots, rows=2, n_ratios=1, nbytes=4096, **ptrs):
        table = rate.pack_back_pieces([rate.BackPiece(**d) for d in descs]) if descs else None
        p = dict(tape0=t[0][2].data_ptr(), tape1=t[1][2].data_ptr(), src=vs.data_ptr(), image=image.data_ptr(), clipped=clipped.data_ptr())
        p.update(ptrs)
        return hip.eben_stream_pcm_out(p["tape0"], p["tape1"], tp, slots, p["src"], sp, rows, ratios, n_ratios, p["image"], nbytes, p["clipped"], table,
                                       len(descs) if count is None else count, stream())

    bad = [[dict(good, slot=4)], [dict(good, src_row=2)], [dict(good, tape=2)], [dict(good, ratio=1)], [dict(good, ratio=-2)], [dict(good, format=4)],
           [dict(good, n_new=61)], [dict(good, prev_off=161)], [dict(good, n_carry=141)], [dict(good, n_carry=0, n_new=0, n_out=0)], [dict(good, p0=3)],
           [dict(good, p0=-1)], [dict(good, n_out=259)], [dict(good, n_out=-1)], [dict(good, end=True, n_out=280)], [good, dict(plain, slot=1)],
           [good, dict(plain, byte_offset=512)], [dict(good, byte_offset=24)], [dict(good, byte_offset=-16)], [dict(good, byte_offset=3344)],
           [dict(plain, n_carry=1)], [dict(plain, n_out=49)], [dict(plain, n_new=61, n_out=61)], [dict(good, slot=i % 4) for i in range(65)]]
    for descs in bad:
        assert call(descs) == -1 and hip.eben_last_error(), descs
    assert call([good], nbytes=-1) == -1 and call([good], nbytes=1 << 31) == -1 and call([good], slots=257) == -1 and call([good], count=-1) == -1
    for name in ("tape0", "tape1", "src", "image", "clipped"):
        assert call([good], **{name: None}) == -1 and b"null" in hip.eben_last_error(), name
        assert call([good], **{name: image.data_ptr() + 2050}) == -1 and b"misaligned" in hip.eben_last_error(), name
    assert call([good], tape1=t[0][2].data_ptr()) == -1 and b"two tapes overlap" in hip.eben_last_error()
    assert call([good], src=t[1][2].data_ptr()) == -1 and b"overlaps src" in hip.eben_last_error()
    assert call([good], image=t[0][1].data_ptr() + 512) == -1 and b"image overlaps" in hip.eben_last_error()
    assert call([good], clipped=image.data_ptr() + 2048) == -1 and b"clipped table overlaps" in hip.eben_last_error()
    assert call([good], image=k.data_ptr()) == -1 and b"table of ratio 0 overlaps" in hip.eben_last_error()
    assert call([], 0) == 0 and call([good], 0) == 0 and call([dict(plain, n_new=0, n_out=0)]) == 0   # nothing to do: no launch
    torch.cuda.synchronize()
    for flat, dev, _ in t:
        assert same_bits(dev.cpu(), flat)               # nothing was written
    assert bool((base == FILL).all()) and clipped.tolist() == [3] * slots
    assert call([good, plain]) == 0 and call([dict(good, tape=0, end=True, n_out=279)]) == 0   # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert not same_bits(t[1][1].cpu(), t[1][0]) and not same_bits(t[0][1].cpu(), t[0][0]) and all(fences_intact(dev.cpu()) for _, dev, _ in t)
    assert not bool((image[16 : 16 + 3 * 255] == FILL).all()) and not bool((image[1024:1124] == FILL).all())
    assert bool((base[:GUARD] == FILL).all()) and bool((base[-GUARD:] == FILL).all()) and bool((image[1124:] == FILL).all())


# ---- the raw front ------------------------------------------------------------------------------------------------------------------------
def test_pcm_chunks_in_equals_the_corpus_decoder(hip):
    from vibravox_amd._lib import PCM_CHUNK_TILE, EbenPcmChunk, stream

    rows, pitch = 14, PCM_CHUNK_TILE + 40
    flat, dev, view = fenced(rows, pitch, "chunks_in/dst")
    want = flat.clone()
    chunks, keep = [], []
    cases = [(f, n) for f in range(4) for n in (1, 300, PCM_CHUNK_TILE + 1)]
    for j, (f, n) in enumerate(cases):
        raw = ((np.arange(n * BYTES[f], dtype=np.int64) * (37 + 2 * j) + 11 * j + 5) % 256).astype(np.uint8)
        if f == 0:
            raw[:4] = (0x00, 0x80, 0xFF, 0x7F)[: len(raw)]   # -32768 and 32767
        off = 1 + j % 3                                      # the bytes start at an odd address, or 2 or 3 off the 4-byte grid
        buf = torch.zeros(off + len(raw) + 3, dtype=torch.uint8)
        buf[off : off + len(raw)] = torch.from_numpy(raw)
        buf = buf.to(DEV)
        keep.append(buf)
        assert (buf.data_ptr() + off) % 4 == off
        row = (5 * j + 2) % rows
        chunks.append(EbenPcmChunk(buf.data_ptr() + off, n, f, row))
        decoded = torch.from_numpy(E.decode(raw.tobytes(), FORMATS[f]))
        # the merged decoder on the same bytes, where it wants them: at a multiple of 16
        data = torch.zeros(-(-len(raw) // 16) * 16, dtype=torch.uint8)
        data[: len(raw)] = torch.from_numpy(raw)
        merged, lens = corpus.pcm_to_rows(data.to(DEV), np.array([(0, n, 1, 0, f)], dtype=corpus.ROW_DTYPE))
        assert int(lens[0]) == n and same_bits(merged[0, :n].cpu(), decoded), (f, n)
        body(want, rows, pitch)[row, :n] = decoded
    assert len({c.dst_row for c in chunks}) == len(chunks) == 12
    table = (EbenPcmChunk * len(chunks))(*chunks)
    good = lambda: hip.eben_pcm_chunks_in(table, len(chunks), view.data_ptr(), rows, pitch, stream())   # noqa: E731
    one = lambda **kw: (EbenPcmChunk * 1)(EbenPcmChunk(**dict(dict(bytes=keep[0].data_ptr() + 1, n=1, format=0, dst_row=0), **kw)))   # noqa: E731
    two = (EbenPcmChunk * 2)(chunks[0], chunks[0])
    many = (EbenPcmChunk * 65)(*[EbenPcmChunk(keep[0].data_ptr(), 0, 0, i % rows) for i in range(65)])
    bad = [(one(format=4), 1), (one(format=-1), 1), (one(n=-1), 1), (one(n=pitch + 1), 1), (one(dst_row=rows), 1), (one(dst_row=-1), 1), (one(bytes=None), 1),
           (two, 2), (many, 65), (one(), -1), (None, 1), (one(bytes=view.data_ptr() + 1), 1)]
    for t, count in bad:
        assert hip.eben_pcm_chunks_in(t, count, view.data_ptr(), rows, pitch, stream()) == -1 and hip.eben_last_error(), count
    for dst, r, p in ((None, rows, pitch), (view.data_ptr() + 2, rows, pitch), (view.data_ptr(), 0, pitch), (view.data_ptr(), rows, 0)):
        assert hip.eben_pcm_chunks_in(table, len(chunks), dst, r, p, stream()) == -1 and hip.eben_last_error()
    assert hip.eben_pcm_chunks_in(table, 0, view.data_ptr(), rows, pitch, stream()) == 0 and hip.eben_pcm_chunks_in(one(n=0), 1, view.data_ptr(), rows, pitch,
                                                                                                              stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(dev.cpu(), flat)                    # nothing was written
    assert good() == 0
    got = dev.cpu()
    assert same_bits(got, want) and fences_intact(got)   # each chunk its row's bits; the rest of every pitch and the other rows as they were


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generator():
    return R.formula_generator(2, 32)[0].to(DEV)


def encoded(x, fmt):
    """The merged encoder on the rows of ``x`` (rows, 1, T): (bytes (rows, T * bytes per sample) on the host, clipped counts)."""
    rows, _, t = x.shape
    f = FORMATS.index(fmt)
    pitch = -(-(t * BYTES[f]) // 16) * 16
    image = torch.zeros(rows * pitch, dtype=torch.uint8, device=DEV)
    table = np.array([(r * t, r * pitch, t, f) for r in range(rows)], dtype=corpus.ENC_ROW_DTYPE)
    counts = corpus.rows_to_pcm(x.contiguous(), table, image)
    return image.view(rows, pitch)[:, : t * BYTES[f]].cpu(), counts.cpu()


@pytest.mark.parametrize("r,fmt", [(48000, "PCM16"), (44100, "PCM24"), (8000, "FLOAT32")])
def test_the_enhancer_leaves_as_the_whole_result_resampled_and_encoded(hip, r, fmt):
    gen = generator()
    n_in = 768
    x = formula_audio(f"stream_pcm/enhancer/{r}", 2, 9 * n_in + 101).to(DEV)
    with torch.no_grad():
        def drive(enhancer):
            res = [enhancer.push(x[:, :, i * n_in : (i + 1) * n_in]) for i in range(9)]
            return res + [enhancer.finish(x[:, :, 9 * n_in :])]

        plain = torch.cat(drive(streaming.StreamingEnhancer(gen, 256, streams=2, input_rate=48000)), dim=2)
        want, counts = encoded(augment.resample(plain, 16000, r), fmt)
        enhancer = streaming.StreamingEnhancer(gen, 256, streams=2, input_rate=48000, output_rate=r, output_format=fmt)
        assert enhancer.input_chunk_samples == n_in and enhancer.output_lookahead == rate.Schedule(16000, r).lookahead
        res = drive(enhancer)
        assert all(o.dtype is torch.uint8 and o.dim() == 2 and o.shape[0] == 2 for o in res) and res[0].shape[1] == 0
        got = torch.cat(res, dim=1).cpu()
        assert got.shape == want.shape and torch.equal(got, want)
        assert torch.equal(enhancer.clipped.cpu(), counts)
        # only a rate: the FLOAT32 route, viewed
        floats = drive(streaming.StreamingEnhancer(gen, 256, streams=2, input_rate=48000, output_rate=r))
        assert all(o.dtype is torch.float32 and o.dim() == 3 for o in floats)
        assert same_bits(torch.cat(floats, dim=2).cpu(), augment.resample(plain, 16000, r).cpu())
        # a second stream on the same enhancer repeats the bytes and starts its count again
        enhancer.reset()
        assert torch.equal(torch.cat(drive(enhancer), dim=1).cpu(), want) and torch.equal(enhancer.clipped.cpu(), counts)


def test_seventy_rows_leave_in_two_calls_and_enhance_stream_joins_them(hip, monkeypatch):
    from tests.test_gpu_pool_rate import Counted
    from vibravox_amd import _lib, inference

    gen = generator()
    x = formula_audio("stream_pcm/rows70", 70, 2500).to(DEV)
    with torch.no_grad():
        plain = inference.enhance_stream(gen, x, 256)[0]
        want, _ = encoded(augment.resample(plain, 16000, 8000), "PCM16")
        counted = Counted(hip)
        monkeypatch.setattr(_lib, "_lib", counted)
        got = inference.enhance_stream(gen, x, 256, output_rate=8000, format="PCM16")
        runs = sum(1 for c in counted.calls if c == "eben_stream_pcm_out")
        assert runs % 2 == 0 and runs >= 2                       # 64 rows and 6 rows of every run that emitted
        assert got.dtype is torch.uint8 and torch.equal(got.cpu(), want)
        floats = inference.enhance_stream(gen, x[:3], 256, output_rate=8000)
        assert same_bits(floats.cpu(), augment.resample(plain[:3], 16000, 8000).cpu())


WAYS = (dict(output_rate=48000, output_format="PCM16"), dict(output_rate=44100, output_format="PCM24"), dict(output_rate=16000, output_format="PCM32"),
        dict(output_rate=8000, output_format="FLOAT32"), dict())


class Leaving:
    """A pool whose k-th ``open`` leaves the k-th way of ``WAYS``, for the scenario drivers that know ``open(rate)`` only."""

    def __init__(self, pool):
        self.pool, self.opened = pool, 0

    def open(self, r):
        self.opened += 1
        return self.pool.open(r, **WAYS[(self.opened - 1) % len(WAYS)])

    def __getattr__(self, name):
        return getattr(self.pool, name)


def pool_pointers(pool):
    return ([t.data_ptr() for pair in pool.state.buffers.values() for t in pair] + [t.data_ptr() for t in pool.tapes.tapes + pool.tapes.fifo]
            + [t.data_ptr() for t in pool.back.tapes + [pool.back.clipped]] + [t.data_ptr() for st in pool.private.values() for pair in st.buffers.values() for t in pair])


def test_pool_sessions_leave_as_the_unchanged_pools_results_resampled_and_encoded(hip):
    gen = generator()
    spec = PR.rated_scenario(P.SCENARIO_256, PR.RATES_256)
    clips = {name: formula_audio(f"stream_pcm/pool/{name}", 1, total).to(DEV) for name, total, _, _, _ in spec}
    rates = sorted({r for *_, r in spec})
    with torch.no_grad():
        plain_outs, _, _ = PR.run_rated_scenario(streaming.StreamPool(gen, 256, slots=4, input_rates=rates), clips, spec)
        pool = streaming.StreamPool(gen, 256, slots=4, input_rates=rates, output_rates=(48000, 44100, 8000)).prepare(DEV, private=4)
        for t in pool.back.tapes:
            t.fill_(NAN)
        ptrs = pool_pointers(pool)
        outs, _, sessions = PR.run_rated_scenario(Leaving(pool), clips, spec)
        assert sorted(WAYS.index(dict(output_rate=s.output_rate, output_format=s.output_format) if s.egress else {}) for s in sessions.values()) == [0, 1, 2, 3, 4]
        got = {}
        for name, s in sessions.items():
            whole = torch.cat(plain_outs[name], dim=2)
            got[name] = torch.cat(outs[name], dim=-1).cpu()
            if not s.egress:
                assert s.clipped is None and same_bits(got[name], whole.cpu()), name
                continue
            at_rate = whole if s.output_rate == 16000 else augment.resample(whole, 16000, s.output_rate)
            want, counts = encoded(at_rate, s.output_format)
            assert all(o.dtype is torch.uint8 and o.dim() == 1 for o in outs[name]), name
            assert got[name].shape == want[0].shape and torch.equal(got[name], want[0]), (name, s.output_rate, s.output_format)
            assert int(s.clipped) == int(counts[0]), name
        # a second scenario on the same pool allocates nothing and repeats the bytes
        again, _, _ = PR.run_rated_scenario(Leaving(pool), clips, spec)
        assert pool_pointers(pool) == ptrs
        for name in got:
            assert torch.equal(torch.cat(again[name], dim=-1).cpu(), got[name]), name
        # isolation: the others push NaN audio, and no byte of this session changes
        for k, keep in enumerate(("A", "D")):
            noisy = {name: c if name == keep else torch.full_like(c, NAN) for name, c in clips.items()}
            lonely = Leaving(pool)
            lonely.opened = 0
            res, _, _ = PR.run_rated_scenario(lonely, noisy, spec)
            assert torch.equal(torch.cat(res[keep], dim=-1).cpu(), got[keep]), keep


def test_pcm16_bytes_pushed_give_the_bits_of_their_decoded_samples(hip):
    gen = generator()
    n_in, pushes = 768, 11
    x = formula_audio("stream_pcm/ingress", 1, pushes * n_in + 55)
    raw = E.encode(x.numpy(), "PCM16")[0]
    data = torch.frombuffer(bytearray(b"\x00" + raw), dtype=torch.uint8).to(DEV)[1:]     # the bytes at an odd address
    floats = torch.from_numpy(E.decode(raw, "PCM16")).reshape(1, 1, -1).to(DEV)
    assert data.data_ptr() % 2 == 1 and floats.shape == x.shape
    with torch.no_grad():
        pool = streaming.StreamPool(gen, 256, slots=2, input_rates=(48000,))
        a, b = pool.open(48000, input_format="PCM16"), pool.open(48000)
        res = [pool.step({a: data[2 * n_in * i : 2 * n_in * (i + 1)], b: floats[:, :, n_in * i : n_in * (i + 1)]}) for i in range(pushes)]
        got = torch.cat([r[a] for r in res] + [pool.close(a, data[2 * n_in * pushes :])], dim=2)
        want = torch.cat([r[b] for r in res] + [pool.close(b, floats[:, :, n_in * pushes :])], dim=2)
        assert got.shape == want.shape and got.shape[2] > 2048 and same_bits(got.cpu(), want.cpu())
        c = pool.open(48000, input_format="PCM16")
        with pytest.raises(ValueError, match="1536"):
            pool.step({c: data[:1534]})
        with pytest.raises(ValueError, match="uint8"):
            pool.step({c: floats[:, :, :n_in]})
        # the enhancer's rows take the same bytes
        one = streaming.StreamingEnhancer(gen, 256, streams=1, input_rate=48000, input_format="PCM16")
        rows = [one.push(data[2 * n_in * i : 2 * n_in * (i + 1)].reshape(1, -1)) for i in range(pushes)] + [one.finish(data[2 * n_in * pushes :].reshape(1, -1))]
        ref = streaming.StreamingEnhancer(gen, 256, streams=1, input_rate=48000)
        ref_rows = [ref.push(floats[:, :, n_in * i : n_in * (i + 1)]) for i in range(pushes)] + [ref.finish(floats[:, :, n_in * pushes :])]
        assert same_bits(torch.cat(rows, dim=2).cpu(), torch.cat(ref_rows, dim=2).cpu())


# ---- library calls ------------------------------------------------------------------------------------------------------------------------
def steady_tick_calls(counted, gen, n, pool_kw, open_kw):
    """The library calls of one tick in which ``n`` pooled sessions of a 64-slot pool push (after every session has reached its slot)."""
    pool = streaming.StreamPool(gen, 256, slots=64, **pool_kw).prepare(DEV, private=1)
    sessions = [pool.open(**open_kw) for _ in range(n)]
    s0 = sessions[0]
    chunk = torch.zeros(2 * s0.input_chunk_samples, dtype=torch.uint8, device=DEV) if s0.input_format else torch.zeros(1, 1, s0.input_chunk_samples, device=DEV)
    for s in sessions:   # one by one through the same private state
        while s.phase != "pooled":
            pool.step({s: chunk})
    pool.step({s: chunk for s in sessions})
    counted.calls.clear()
    out = pool.step({s: chunk for s in sessions})
    calls = list(counted.calls)
    want = (1536,) if s0.output_format == "PCM16" and s0.output_rate == 48000 else (1, 1, 256)
    assert all(tuple(o.shape) == want for o in out.values())
    return calls


def test_a_tick_in_and_out_as_pcm_costs_one_library_call_on_each_side(hip, monkeypatch):
    from tests.test_gpu_pool_rate import Counted
    from vibravox_amd import _lib

    counted = Counted(hip)
    monkeypatch.setattr(_lib, "_lib", counted)
    gen = generator()
    out, front = "eben_stream_pcm_out", "eben_pcm_chunks_in"
    leave = dict(output_rate=48000, output_format="PCM16")
    with torch.no_grad():
        for n in (1, 64):
            today = steady_tick_calls(counted, gen, n, {}, {})
            assert len(today) > 20 and out not in today and front not in today
            assert steady_tick_calls(counted, gen, n, dict(output_rates=(48000,)), leave) == today + [out], n
            assert steady_tick_calls(counted, gen, n, dict(output_rates=(48000,)), dict(leave, input_format="PCM16")) == [front] + today + [out], n
            if n > 1:   # the two below do not depend on how many sessions push: once
                continue
            assert steady_tick_calls(counted, gen, n, dict(output_rates=(48000, 44100)), {}) == today       # declared, not used: today's calls in today's order
            # frames at 48 kHz on both sides: the PCM front, the rate front, today's tick, the way out
            both = steady_tick_calls(counted, gen, n, dict(input_rates=(48000,), output_rates=(48000,)), dict(leave, input_rate=48000, input_format="PCM16"))
            assert both == [front, "eben_rate_splice_slots", "eben_resample_slots"] + today + [out], n
            print(f"{n} sessions: {len(today)} library calls a tick in float at the model's rate, {len(both)} with 48 kHz PCM16 on both sides")
