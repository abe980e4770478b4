"""The way out of a live session, on the host: ``rate.SlotBack`` turns "slot s emitted k samples" into the pieces of one
``eben_stream_pcm_out`` call.  Every piece is checked by brute force over stream positions -- each tap of each output must find its own
sample in the tape the piece describes, or lie outside the tape exactly where the signal has no sample -- as ``test_pool_rate_plan.py``
does for the front.  No GPU: the library is loaded for its symbols only."""
import ctypes
import json

import pytest

from tests import ragged_oracle as R
from vibravox_amd import rate, streaming
from vibravox_amd.inference import resampled_length

MODEL = 16000
RATES = (48000, 44100, 24000, 8000, 16000)
CHUNK = 256


def emissions(total):
    """A stream of ``total`` model-rate samples as a pool hands it over: nothing during warm-up, whole chunks, then the rest at the end."""
    out = [(0, False), (0, False)]
    done = 0
    while total - done > CHUNK + 37:   # the end hands over more than a chunk at once, as a finish does
        out.append((CHUNK, False))
        done += CHUNK
    out.append((total - done, True))
    return out


def lengths(r):
    taps = rate.Schedule(MODEL, r).taps if r != MODEL else 13
    return (1, taps, 3 * CHUNK + 1, 5 * CHUNK + 255, 2 * CHUNK + 37)


@pytest.mark.parametrize("r", RATES)
def test_every_piece_keeps_the_tape_invariants_the_kernel_validates(r):
    for total in lengths(r):
        back = rate.SlotBack(CHUNK, 3, RATES, MODEL, max_emit=2 * CHUNK)
        back.open(1, r, "PCM16")
        orig, new, width = rate.ratio(MODEL, r)
        taps = 2 * width + orig
        tape, pushed, emitted = [], 0, 0   # the stream positions the slot's current tape holds
        parity = 0
        for k, final in emissions(total):
            pieces, ranges, nbytes = back.emit([(1, 0, k, final)])
            if not pieces:
                assert ranges[1][1] == 0 and (k == 0 or r == MODEL), (r, total, k)
                continue
            (p,) = pieces
            assert ranges[1] == (p.byte_offset, p.n_out) and nbytes == p.byte_offset + 2 * p.n_out and p.byte_offset % 16 == 0
            assert p.slot == 1 and p.src_row == 0 and p.format == 0 and p.n_new == k and p.end == final
            if r == MODEL:
                assert p.ratio == -1 and p.n_carry == 0 and p.n_out == k
                emitted += k
                pushed += k
                continue
            assert p.ratio == back.rates.index(r) and p.tape == parity ^ 1, (r, total)
            parity ^= 1
            # the tape: the carried samples come from the tape of the push before, and end where the new ones begin
            assert 0 <= p.prev_off and p.prev_off + p.n_carry <= len(tape) and p.n_carry <= taps - 1
            assert 0 < p.n_carry + p.n_new <= back.tape_samples
            tape = tape[p.prev_off : p.prev_off + p.n_carry] + list(range(pushed, pushed + k))
            pushed += k
            assert tape == list(range(pushed - len(tape), pushed)), (r, total)
            assert 0 <= p.p0 < new
            for n in range(p.n_out):
                g = emitted + n
                q, ph = divmod(g, new)
                ql, pl = divmod(p.p0 + n, new)
                assert pl == ph, (r, total, n)
                for j in range(taps):
                    pos, idx = q * orig - width + j, p.base0 + ql * orig + j
                    if 0 <= pos < pushed:
                        assert 0 <= idx < len(tape) and tape[idx] == pos, (r, total, n, j)
                    else:   # in front of the signal, or behind its end: the tape has no such index, the kernel reads a zero
                        assert (idx < 0 or idx >= len(tape)) and (pos < 0 or final), (r, total, n, j)
            emitted += p.n_out
            # what the entry point checks of the last output (rate.hip's check_piece)
            if p.n_out:
                ql, pl = divmod(p.p0 + p.n_out - 1, new)
                base_last = p.base0 + ql * orig
                if final:
                    assert (base_last + width) * new + pl * orig < new * len(tape)
                else:
                    assert base_last + taps <= len(tape)
        assert pushed == total
        assert emitted == (total if r == MODEL else resampled_length(total, orig, new)), (r, total)


def test_a_push_below_the_lookahead_still_writes_its_tape():
    back = rate.SlotBack(CHUNK, 1, (48000,), MODEL)
    back.open(0, 48000, "PCM24")
    assert back.lookahead(0) == rate.Schedule(MODEL, 48000).lookahead > 0
    pieces, ranges, nbytes = back.emit([(0, 0, 3, False)])
    assert len(pieces) == 1 and pieces[0].n_out == 0 and pieces[0].n_new == 3 and ranges[0] == (0, 0) and nbytes == 0
    pieces, ranges, nbytes = back.emit([(0, 0, 0, True)])
    assert pieces[0].n_out == 9 and pieces[0].n_new == 0 and pieces[0].n_carry == 3 and pieces[0].end and nbytes == 27


def test_byte_ranges_are_16_aligned_and_disjoint():
    back = rate.SlotBack(CHUNK, 8, RATES, MODEL)
    formats = ("PCM16", "PCM24", "PCM32", "FLOAT32", "PCM24", None)
    rates = (48000, 44100, 16000, 8000, None, 24000)
    for slot, (r, f) in enumerate(zip(rates, formats)):
        back.open(slot + 1, r, f)
    for k in (255, 1, CHUNK, 77):
        pieces, ranges, nbytes = back.emit([(slot + 1, 5 - slot, k, False) for slot in range(6)])
        spans = sorted((p.byte_offset, p.byte_offset + p.nbytes) for p in pieces)
        assert all(lo % 16 == 0 for lo, _ in spans)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] == nbytes)
        for p in pieces:
            assert ranges[p.slot] == (p.byte_offset, p.n_out) and p.src_row == 6 - p.slot
            assert p.nbytes == p.n_out * rate.PCM_BYTES[p.format]
    with pytest.raises(RuntimeError, match="named twice"):
        back.emit([(1, 0, 4, False), (1, 1, 4, False)])
    with pytest.raises(RuntimeError, match="not open"):
        back.emit([(0, 0, 4, False)])
    with pytest.raises(RuntimeError, match="sized for"):
        back.emit([(1, 0, back.max_emit + 1, False)])


def test_the_piece_table_is_packed_as_the_header_lays_it_out():
    from vibravox_amd._lib import EbenPcmChunk, EbenStreamPcmPiece

    assert ctypes.sizeof(EbenStreamPcmPiece) == 36 and ctypes.sizeof(EbenPcmChunk) == 24
    piece = rate.BackPiece(slot=255, src_row=65535, ratio=-1, tape=1, prev_off=2, n_carry=3, n_new=4, p0=5, base0=-6, n_out=7, end=True, format=3,
                           byte_offset=1 << 30)
    t = rate.pack_back_pieces([piece, piece._replace(ratio=7, end=False, slot=0)])
    got = t[0]
    assert (got.prev_off, got.n_carry, got.n_new, got.p0, got.base0, got.n_out, got.byte_offset) == (2, 3, 4, 5, -6, 7, 1 << 30)
    assert (got.src_row, got.slot, got.tape, got.ratio, got.format, got.end) == (65535, 255, 1, -1, 3, 1)
    assert (t[1].ratio, t[1].end, t[1].slot) == (7, 0, 0)


def test_the_tile_is_stated_without_a_launch():
    for r in (48000, 44100, 24000, 8000):
        orig, new, width = rate.ratio(MODEL, r)
        front, mine = rate.tile(orig, new, width), rate.tile_of_back(orig, new, width)
        assert mine["outputs_per_block"] == front["outputs_per_block"] and mine["window_floats"] == front["window_floats"]
        assert (mine["table_route"] > 0) == front["table_in_lds"] and (mine["table_route"] == 2) == (new == 1)
    assert rate.tile_of_back(*rate.ratio(MODEL, 44100))["table_route"] == 0
    assert rate.tile_of_back(1, 1, 0) == dict(outputs_per_block=1024, window_floats=1024, table_route=2)


def test_open_refuses_an_undeclared_rate_and_an_unknown_format_by_name():
    gen = R.formula_generator(2, 32)[0]
    book = streaming.PoolBook(gen, CHUNK, 4, output_rates=(48000, 8000))
    with pytest.raises(ValueError, match="44100"):
        book.open(output_rate=44100)
    with pytest.raises(ValueError, match="PCM16, PCM24, PCM32, FLOAT32.*'PCM8'"):
        book.open(output_rate=48000, output_format="PCM8")
    with pytest.raises(ValueError, match="'ULAW'"):
        book.open(input_format="ULAW")
    assert book.free_slots == [0, 1, 2, 3]   # a refusal takes no slot
    s = book.open(output_rate=48000, output_format="PCM16", input_format="PCM16")
    assert (s.output_rate, s.output_format, s.input_format, s.egress) == (48000, "PCM16", "PCM16", True)
    assert s.output_lookahead == rate.Schedule(MODEL, 48000).lookahead
    plain = book.open(output_rate=16000)
    assert not plain.egress and plain.output_rate == 16000 and plain.output_format is None and plain.output_lookahead == 0
    at_model = streaming.PoolBook(gen, CHUNK, 4).open(output_format="PCM32")   # the model's rate needs no declaration
    assert at_model.egress and at_model.output_rate == 16000 and at_model.output_lookahead == 0


def test_a_pool_that_declares_output_rates_and_uses_none_makes_todays_lists():
    from tests.golden import make_pool_entries_golden as G

    gen = R.formula_generator(2, 32)[0]
    with open(G.PATH) as f:
        today = json.load(f)
    for book in (streaming.PoolBook(gen, 256, 4, output_rates=(48000, 44100)), streaming.PoolBook(gen, 256, 4, input_rates=(48000,), output_rates=(8000,))):
        got = json.loads(json.dumps(G.record(book)))
        assert got == today


def test_the_two_entries_refuse_bad_arguments_before_they_touch_a_device():
    """Every check of ``eben_stream_pcm_out`` and ``eben_pcm_chunks_in`` comes before the launch: with made-up device addresses a refusal is
    all that can happen here.  ``tests/test_gpu_stream_pcm.py`` repeats them on real buffers and shows that nothing was written."""
    from vibravox_amd._lib import EbenPcmChunk, EbenRateRatio, load

    lib = load()
    tape0, tape1, src, image, clipped, table = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    ratios = (EbenRateRatio * 1)(EbenRateRatio(table, 1, 3, 7, 0))
    good = rate.BackPiece(slot=1, src_row=0, ratio=0, tape=1, prev_off=10, n_carry=40, n_new=60, p0=0, base0=0, n_out=255, end=False, format=1, byte_offset=16)

    def call(pieces, count=None, **kw):
        a = dict(tape0=tape0, tape1=tape1, tp=200, slots=4, src=src, sp=60, rows=2, n_ratios=1, image=image, nbytes=4096, clipped=clipped)
        a.update(kw)
        t = rate.pack_back_pieces(pieces) if pieces else None
        return lib.eben_stream_pcm_out(a["tape0"], a["tape1"], a["tp"], a["slots"], a["src"], a["sp"], a["rows"], ratios, a["n_ratios"], a["image"], a["nbytes"],
                                       a["clipped"], t, len(pieces) if count is None else count, None)

    assert call([], 0) == 0 and call([good], 0) == 0                                   # an empty list: no launch
    refused = [([good._replace(slot=4)], {}), ([good._replace(ratio=1)], {}), ([good._replace(format=4)], {}), ([good._replace(tape=2)], {}),
               ([good._replace(p0=3)], {}), ([good._replace(n_out=259)], {}), ([good._replace(end=True, n_out=280)], {}), ([good._replace(byte_offset=8)], {}),
               ([good._replace(byte_offset=4080)], {}), ([good._replace(n_new=61)], {}), ([good._replace(prev_off=161)], {}),
               ([good, good._replace(byte_offset=2048)], {}), ([good, good._replace(slot=2, src_row=1, byte_offset=512)], {}),
               ([good._replace(ratio=-1)], {}), ([good] * 65, {}), ([good], dict(image=image + 8)), ([good], dict(tape0=tape0 + 2)), ([good], dict(clipped=None)),
               ([good], dict(tape1=tape0 + 16)), ([good], dict(image=tape0)), ([good], dict(nbytes=1 << 31)), ([good], dict(slots=0)), ([good], dict(tp=99))]
    for pieces, kw in refused:
        assert call(pieces, **kw) == -1 and lib.eben_last_error(), (pieces, kw)
    chunk = lambda **kw: (EbenPcmChunk * 1)(EbenPcmChunk(**dict(dict(bytes=src + 1, n=10, format=0, dst_row=0), **kw)))   # noqa: E731
    assert lib.eben_pcm_chunks_in(None, 0, tape0, 4, 200, None) == 0
    for t, dst, rows in ((chunk(format=4), tape0, 4), (chunk(n=201), tape0, 4), (chunk(dst_row=4), tape0, 4), (chunk(bytes=None), tape0, 4), (chunk(), None, 4),
                         (chunk(), tape0 + 2, 4), (chunk(), tape0, 0), (chunk(bytes=tape0 + 5), tape0, 4)):
        assert lib.eben_pcm_chunks_in(t, 1, dst, rows, 200, None) == -1 and lib.eben_last_error()
