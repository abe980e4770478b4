"""CPU: ``StreamPool`` sessions at a recording rate -- ``rate.SlotFront``'s per-slot lists executed in float64 on NaN-poisoned tapes and
FIFO buffers (``tests/pool_rate_oracle.py``), ``PoolBook`` with rated sessions through the float64 pool oracle, and the refusals of the
pool and of the two host entries ``eben_rate_splice_slots`` / ``eben_resample_slots``.

Bounds: what the front hands on is compared with ``rate_oracle.direct`` of the whole signal for EQUALITY (the same float64 products in
the same order); the pool's outputs with the float64 generator of the float64-resampled clip within 1e-12, the bar of
test_stream_pool_plan.py."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests import pool_oracle as P
from tests import pool_rate_oracle as PR
from tests import ragged_oracle as R
from tests import rate_oracle as RO
from vibravox_amd import augment, ragged, rate, streaming


@functools.lru_cache(maxsize=None)
def generator(p):
    return R.formula_generator(p, 32)


def whole(x64, r, model_rate=16000):
    """``rate_oracle.direct`` of (T,) float64 at ``r`` Hz."""
    orig, new, width = rate.ratio(r, model_rate)
    return RO.direct(x64[None], augment.sinc_resample_kernel(r, model_rate)[0].numpy(), orig, new, width)[0][0]


# ---- the front alone ------------------------------------------------------------------------------------------------------------------
# (rate, opening tick, ticks skipped, pushes, tail): tails of 0, 1 and input_chunk_samples - 1; one session closes after a single push, one
# after none; "-1" stands for input_chunk_samples - 1
FRONT_CASES = {
    1280: (6, [(48000, 0, (2,), 5, 1), (44100, 1, (3, 4), 4, -1), (24000, 0, (), 1, 7), (8000, 2, (5,), 4, 0), (16000, 0, (), 0, 0), (48000, 3, (), 0, 100)]),
    256: (4, [(48000, 0, (1,), 6, -1), (32000, 2, (4, 5), 5, 0), (8000, 1, (), 1, 1), (8000, 0, (), 0, 40)]),
}


@pytest.mark.parametrize("chunk", [1280, 256])
def test_front_alone_hands_on_the_whole_signal_exactly(chunk):
    slots, cases = FRONT_CASES[chunk]
    front = rate.SlotFront(chunk, slots, [c[0] for c in cases], 16000, 256)
    assert 16000 not in front.rates and front.tape_samples == max(2 * w + o - 1 + n for (o, _, w), n in zip(front.ratios, front.input_chunk))
    tapes = PR.OracleTapes(front)
    g = np.random.default_rng(chunk)
    live = {}
    for slot, (r, start, skips, pushes, tail) in enumerate(cases):
        if r == 16000:
            continue   # a slot at the model's rate has no front: it stays NaN throughout
        n_in = front.input_chunk[front.rates.index(r)]
        tail = n_in - 1 if tail < 0 else tail
        live[slot] = dict(rate=r, start=start, skips=skips, pushes=pushes, tail=tail, n_in=n_in, x=g.standard_normal(pushes * n_in + tail), pos=0, got=[],
                          done=0, open=False)
    for tick in range(40):
        feed = []
        for slot, s in live.items():
            if tick == s["start"]:
                front.open(slot, s["rate"])
                s["open"] = True
            if s["open"] and tick not in s["skips"] and s["done"] < s["pushes"]:
                feed.append(slot)
        if feed:
            splices, pieces, chunks = front.feed([(slot, live[slot]["n_in"]) for slot in feed])
            tapes.run(splices, pieces, {slot: live[slot]["x"][live[slot]["pos"] : live[slot]["pos"] + live[slot]["n_in"]] for slot in feed})
            assert len({(s.n_new, s.src_row) for s in splices}) == len(splices) == len(feed)
            for slot in feed:
                s = live[slot]
                assert len(chunks[slot]) == (0 if s["done"] == 0 else 1) and all(c.samples == chunk for c in chunks[slot])
                s["got"] += [tapes.chunk(c) for c in chunks[slot]]
                s["pos"], s["done"] = s["pos"] + s["n_in"], s["done"] + 1
        for slot, s in live.items():   # a session whose pushes are done closes in a tick of its own
            if s["open"] and s["done"] == s["pushes"] and tick not in s["skips"] and slot not in feed:
                splices, pieces, chunks = front.feed([(slot, s["tail"])], final=True)
                tapes.run(splices, pieces, {slot: s["x"][s["pos"] :]})
                sizes = [c.samples for c in chunks[slot]]
                rest = front.outputs_after(slot, 0) - chunk * s["pushes"]
                # after at least one push the FIFO completes one more whole chunk at the close, whatever the tail
                assert sizes == ([chunk] if s["pushes"] else []) + ([rest] if rest else []), (slot, sizes, rest)
                s["got"] += [tapes.chunk(c) for c in chunks[slot]]
                s["open"] = False
                front.release(slot)
    assert not any(s["open"] for s in live.values())
    for slot, s in live.items():
        got, want = np.concatenate(s["got"]), whole(s["x"], s["rate"])
        assert got.shape == want.shape and not np.isnan(got).any(), slot
        assert np.array_equal(got, want), (slot, s["rate"], float(np.abs(got - want).max()))
    # the slot at the model's rate was never touched
    for slot, c in enumerate(cases):
        if c[0] == 16000:
            assert np.isnan(tapes.tapes[:, slot]).all() and np.isnan(tapes.fifo[:, slot]).all()


def _plain(entry):
    return {k: v for k, v in entry._asdict().items() if k not in ("tape", "fifo")}


NEAR, LATER, TAIL = 4, 4, 5   # pushes before the jump, pushes after it (both parities twice), samples of the final push


def _drive(chunk, r, far, replay, count):
    """One slot: NEAR pushes, a jump of the slot's ``Schedule`` past 2^33 when ``far``, LATER pushes and a final one of TAIL samples.
    With ``replay`` the front is left to itself; without, its ``steady`` is held at None, so that every push is ``Schedule.push``'s own
    numbers (``count`` tells how many were).  Returns (the NEAR + LATER + 1 results of ``feed``, the schedule at the end)."""
    front = rate.SlotFront(chunk, 3, [r], 16000, 256)
    n_in = front.input_chunk[0]
    front.open(1, r)
    st, out = front.slot[1], []
    before = count[0]

    def push(n, final=False):
        out.append(front.feed([(1, n)], final=final))
        if not replay:
            assert st.lazy == 0 and not st.replay
            st.steady = None

    for _ in range(NEAR):
        push(n_in)
    if far:
        assert n_in % st.schedule.orig == 0
        st.schedule.advance(((1 << 33) // (2 * n_in) + 1) * 2 * n_in)   # an even number of pushes: the parities stay
        assert st.schedule.pushed > 1 << 33
    for _ in range(LATER):
        push(n_in)
    push(TAIL, final=True)
    sch = st.schedule
    return out, (sch.pushed, sch.emitted, sch.start, sch.finished), count[0] - before


@pytest.mark.parametrize("chunk,r", [(1280, 48000), (1280, 44100), (1280, 24000), (1280, 8000), (256, 48000), (256, 32000), (256, 8000)])
def test_steady_descriptors_repeat_also_past_2_to_the_33(chunk, r, monkeypatch):
    """The expected lists come from ``Schedule.push`` at every push (a front whose replay is switched off), near position 0 and past
    2^33; the front that replays its steady push must return the same splices, pieces and chunks, field for field, at both parities
    and at the final push."""
    count, real = [0], rate.Schedule.push

    def counted(self, n_in, final=False):
        count[0] += 1
        return real(self, n_in, final)

    monkeypatch.setattr(rate.Schedule, "push", counted)
    total = NEAR + LATER + 1
    want, end, calls = _drive(chunk, r, False, False, count)
    assert calls == total                                   # the expectation never replays
    want_far, end_far, calls = _drive(chunk, r, True, False, count)
    assert calls == total and end_far[0] > 1 << 33 and end_far[3]
    # what Schedule.push gives: from the first steady push on the numbers repeat, with period 2 in the parities, wherever the stream stands
    assert want[0][2][1] == [] and all(len(run[2][1]) == 1 for run in want[1:-1])
    steady = want[2]   # the carry no longer starts at position 0
    for run in want[3:-1] + want_far[3:-1]:
        assert [_plain(s) for s in run[0]] == [_plain(s) for s in steady[0]] and [_plain(p) for p in run[1]] == [_plain(p) for p in steady[1]]
    for runs in (want, want_far):
        assert all(runs[k] == runs[k + 2] and runs[k] != runs[k + 1] for k in range(2, total - 3))
    assert len(steady[1]) == 2 and sum(p.n_out for p in steady[1]) == chunk   # a steady push straddles two FIFO buffers
    assert want_far == want                                 # the final push too: splices, pieces (p0, base0, length, end) and chunks
    orig, new, _ = rate.ratio(r, 16000)
    tape_samples = rate.SlotFront(chunk, 3, [r], 16000, 256).tape_samples
    for run in want_far:
        for p in run[1]:
            assert abs(p.base0) < 4096 and 0 <= p.p0 < new and p.length <= tape_samples
    last = want_far[-1]
    assert [c.samples for c in last[2][1]] == [chunk, -(-TAIL * new // orig)] and all(p.end for p in last[1]) and len(last[0]) == 1
    # the front as it ships: it replays (fewer calls of Schedule.push) and returns those very lists, and leaves the schedule where the
    # pushes would have
    for far, expect, expect_end in ((False, want, end), (True, want_far, end_far)):
        got, got_end, calls = _drive(chunk, r, far, True, count)
        assert calls < total, calls
        assert len(got) == len(expect)
        for k, (g, w) in enumerate(zip(got, expect)):
            assert [s._asdict() for s in g[0]] == [s._asdict() for s in w[0]], (far, k)
            assert [p._asdict() for p in g[1]] == [p._asdict() for p in w[1]], (far, k)
            assert g[2] == w[2], (far, k)
        assert got_end == expect_end, far


# ---- the book with rated sessions, in float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,chunk,slots,lengths,rates", [(2, 256, 4, P.SCENARIO_256, PR.RATES_256), (1, 1280, 5, PR.SCENARIO_1280, PR.RATES_1280)])
def test_rated_pool_sessions_equal_their_own_resampled_clips(p, chunk, slots, lengths, rates):
    gen, sd = generator(p)
    spec = PR.rated_scenario(lengths, rates)
    clips = {name: formula_audio(f"pool_rate/{name}", 1, total).double() for name, total, _, _, _ in spec}
    pool = PR.RatedOraclePool(gen, sd, chunk, slots, input_rates=sorted(set(rates)))
    outs, slot_of, sessions = PR.run_rated_scenario(pool, clips, spec)
    assert slot_of["E"] == slot_of["A"]   # E inherits A's slot, with another rate's leftovers in its tapes at chunk 1280
    worst = 0.0
    for name, total, _, _, r in spec:
        x = clips[name][0, 0].numpy()
        at_model = torch.from_numpy(x if r == 16000 else whole(x, r)).reshape(1, 1, -1)
        cut = ragged.cut_length(gen, at_model.shape[2])
        o_enh, o_bands = O.generator_forward(sd, at_model[:, :, :cut], p)
        enhanced, bands = torch.cat([o[0] for o in outs[name]], dim=2), torch.cat([o[1] for o in outs[name]], dim=2)
        assert enhanced.shape == o_enh.shape == (1, 1, cut) and bands.shape == o_bands.shape, name
        assert not torch.isnan(enhanced).any() and not torch.isnan(bands).any(), name
        err = max(float((enhanced - o_enh).abs().max()), float((bands - o_bands).abs().max()))
        assert err < 1e-12, (name, err)
        worst = max(worst, err)
        sizes = [o[0].shape[2] for o in outs[name][:-1]]
        first = next((i for i, k in enumerate(sizes) if k), len(sizes))
        assert all(k == 0 for k in sizes[:first]) and all(k == chunk for k in sizes[first:]), (name, sizes)
        s = sessions[name]
        assert s.input_rate == r and s.input_chunk_samples * 16000 == chunk * r
        if r != 16000:
            orig, new, _ = rate.ratio(r, 16000)
            assert s.input_latency == s.input_chunk_samples + -(-pool.book.plan.latency * orig // new)
            for k in range(first, len(sizes)):   # pushed - emitted * orig / new at every steady tick
                assert (k + 1) * s.input_chunk_samples - (k + 1 - first) * chunk * orig // new == s.input_latency, (name, k)
        else:
            assert s.input_latency == pool.book.plan.latency
    runs = [e for e in pool.log if isinstance(e, streaming.PooledRun)]
    fronts = [e for e in pool.log if isinstance(e, streaming.FrontRun)]
    assert any(len(run.order) >= 2 for run in runs) and any(len({s.input_rate for s in run.order}) >= 2 for run in runs)
    assert any(len({sp.n_new for sp in f.splices}) >= 2 for f in fronts)   # chunks of different lengths in one tick
    assert pool.book.free_slots == list(range(slots)) and all(st is None for st in pool.book.front.slot)
    print(f"p {p} chunk {chunk}: worst |rated pool - float64 whole clip| {worst:.1e}, {len(runs)} pooled runs, {len(fronts)} front runs")


# ---- refusals and API -----------------------------------------------------------------------------------------------------------------
def test_a_pool_without_rated_sessions_makes_todays_lists():
    """Today's lists are a recording: ``tests/golden/pool_entries_256.json`` was written by the commit before ``PoolBook`` knew
    ``input_rates`` (tests/golden/make_pool_entries_golden.py), every ``tick`` and ``close`` of the scenario field by field."""
    from tests.golden import make_pool_entries_golden as G

    gen, _ = generator(2)
    with open(G.PATH) as f:
        today = json.load(f)
    assert len(today) > 30 and {name for entries in today for name, _ in entries} == {"PooledRun", "PrivatePush", "Move"}

    def same(lists, what):
        lists = json.loads(json.dumps(lists))   # tuples as the file holds them
        assert len(lists) == len(today), what
        for k, (got, want) in enumerate(zip(lists, today)):
            assert [name for name, _ in got] == [name for name, _ in want], (what, k)
            for (_, g), (name, w) in zip(got, want):
                assert g == w, (what, k, name, {f: (g.get(f), w.get(f)) for f in set(g) | set(w) if g.get(f) != w.get(f)})

    same(G.record(streaming.PoolBook(gen, 256, 4)), "no input_rates")
    same(G.record(streaming.PoolBook(gen, 256, 4, input_rates=(), model_rate=16000)), "input_rates=()")
    book = streaming.PoolBook(gen, 256, 4, input_rates=(48000, 16000))
    same(G.record(book), "declared, but every session opens at the model's rate")
    book = streaming.PoolBook(gen, 256, 4, input_rates=(48000,))
    same(G.record(book, lambda: book.open(16000)), "open(model_rate)")
    assert streaming.PoolBook(gen, 256, 4).front is None and streaming.PoolBook(gen, 256, 4, input_rates=(16000,)).front is None


def test_prepare_refuses_another_device_while_rated_sessions_are_open(monkeypatch):
    """The front's schedules and parities belong to the tapes they were made on."""
    gen, _ = generator(2)
    pool = streaming.StreamPool(gen, 256, slots=2, input_rates=(48000,))
    here, there = types.SimpleNamespace(device="here"), types.SimpleNamespace(device="there")
    pool.state, pool.tapes = here, here

    def allocate(device, rows):   # what _allocate does when the device is another one
        pool.state = there
        return True

    monkeypatch.setattr(pool, "_allocate", allocate)
    s = pool.open(48000)
    with pytest.raises(RuntimeError, match="recording rate are open on here.*'there'"):
        pool.prepare("there")
    assert pool.state is here and pool.tapes is here and pool.book.front.slot[s.slot] is not None


def test_the_rated_pool_refuses_misuse_before_it_touches_a_device():
    gen, _ = generator(2)
    with pytest.raises(ValueError, match="smallest chunk_samples that works is 1280"):
        streaming.StreamPool(gen, 256, input_rates=(44100,))
    with pytest.raises(ValueError, match="positive"):
        streaming.StreamPool(gen, 256, input_rates=(0,))
    pool = streaming.StreamPool(gen, 256, slots=3, input_rates=(48000,))
    with pytest.raises(ValueError, match=r"22050.*48000"):
        pool.open(input_rate=22050)
    assert pool.book.free_slots == [0, 1, 2]                 # the refusal took no slot
    plain, same, s = pool.open(), pool.open(16000), pool.open(input_rate=48000)
    assert not plain.rated and not same.rated and s.rated
    assert (plain.input_rate, plain.input_chunk_samples, plain.input_latency) == (16000, 256, pool.latency)
    assert (s.input_rate, s.input_chunk_samples, s.input_latency) == (48000, 768, 768 + 3 * pool.latency)
    ref = streaming.StreamingEnhancer(gen, 256, input_rate=48000)
    assert (s.input_chunk_samples, s.input_latency) == (ref.input_chunk_samples, ref.input_latency)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"expects a float32 \(1, 1, 768\)"):
            pool.step({s: torch.zeros(1, 1, 256)})            # a chunk at the model's rate for a 48 kHz session
        with pytest.raises(ValueError, match=r"\(1, 1, 256\)"):
            pool.step({plain: torch.zeros(1, 1, 768)})
        with pytest.raises(ValueError, match=r"\(1, 1, 768\).*shorter"):
            pool.close(s, torch.zeros(1, 1, 768))             # a whole chunk is a step
        from vibravox_amd._lib import EbenError

        with pytest.raises(EbenError, match="no CPU path"):
            pool.step({s: torch.zeros(1, 1, 768)})
    with pytest.raises(RuntimeError, match="no backward"):
        pool.step({s: torch.zeros(1, 1, 768)})
    assert s.phase == "warming" and pool.book.front.slot[s.slot].schedule.pushed == 0


def test_a_close_below_the_shortest_clip_leaves_the_session_and_its_front():
    gen, _ = generator(2)
    book = streaming.PoolBook(gen, 256, 2, input_rates=(48000,))
    s = book.open(48000)
    st = book.front.slot[s.slot]

    def where():
        return (st.tape, st.fifo, st.held, st.schedule.pushed, st.schedule.emitted, st.schedule.start, st.schedule.finished, s.phase, s.pushes, s.private,
                s.schedule.pushed, tuple(book.free_slots))

    before = where()
    with pytest.raises(ValueError, match="too short"):
        book.close(s, 100)
    assert where() == before
    entries = book.tick([s])
    assert [type(e).__name__ for e in entries] == ["FrontRun"]      # the first push completes nothing: the generator's schedule stays
    assert s.schedule.pushed == 0 and s.pushes == 0 and s.pooled_pushes == 0
    before = where()
    with pytest.raises(ValueError, match="too short"):
        book.close(s, 10)                                     # 778 samples at 48 kHz: 260 at the model's rate
    with pytest.raises(ValueError, match="fewer"):
        book.close(s, 768)
    assert where() == before and book.front.slot[s.slot] is st
    for _ in range(8):
        book.tick([s])
    kinds = [type(e).__name__ for e in book.close(s, 10)]
    assert kinds[0] == "FrontRun" and kinds.count("Hand") == 2 and s.phase == "closed" and book.front.slot[s.slot] is None
    with pytest.raises(RuntimeError, match="closed"):
        book.close(s)


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


A0, A1, SRC, F0, F1, TAB = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000   # never dereferenced: every call below is refused
V = ctypes.c_void_p


def test_rate_splice_slots_argument_errors_without_gpu(lib):
    from vibravox_amd._lib import EbenRateSplice

    good = dict(slot=1, src_row=0, prev_off=10, n_carry=40, n_new=60, tape=1)

    def call(splices=None, count=None, t0=A0, t1=A1, pitch=200, slots=4, src=SRC, sp=60, rows=2, null_table=False, **change):
        splices = [dict(good, **change)] if splices is None else splices
        table = None if null_table else (EbenRateSplice * max(1, len(splices)))(*[EbenRateSplice(**s) for s in splices])
        return lib.eben_rate_splice_slots(V(t0), V(t1), pitch, slots, V(src), sp, rows, table, len(splices) if count is None else count, None)

    msg = lib.eben_last_error
    assert call(splices=[], count=0) == 0 and call(count=0, null_table=True) == 0       # an empty list: no launch
    assert call(null_table=True) == -1 and b"null" in msg()
    assert call(t0=0) == -1 and b"null" in msg() and call(t1=0) == -1 and call(src=0) == -1 and b"null src" in msg()
    for k in ("t0", "t1", "src"):
        assert call(**{k: 0x700002}) == -1 and b"misaligned" in msg(), k
    assert call(count=-1) == -1 and b"at most 64" in msg()
    assert call(splices=[dict(good, slot=i) for i in range(65)], slots=70) == -1 and b"at most 64" in msg()
    assert call(slots=0) == -1 and call(slots=257) == -1 and b"slots" in msg()
    assert call(slot=4) == -1 and b"names slot 4 of 4" in msg() and call(slot=-1) == -1
    assert call(src_row=2) == -1 and b"src row 2 of 2" in msg() and call(src_row=-1) == -1
    assert call(tape=2) == -1 and b"tape 2" in msg()
    assert call(n_carry=-1) == -1 and call(n_new=-1) == -1 and call(n_carry=0, n_new=0) == -1 and b"carry 0, new 0" in msg()
    assert call(prev_off=-1) == -1 and call(prev_off=161) == -1 and b"prev offset" in msg()
    assert call(n_new=61) == -1 and b"past src's pitch" in msg()
    assert call(pitch=99) == -1 and b"past the tape's pitch" in msg()
    assert call(splices=[good, dict(good, src_row=1)]) == -1 and b"two splices on slot 1" in msg()
    assert call(t1=A0 + 4 * (4 * 200 - 1)) == -1 and b"tapes overlap" in msg()          # the last float of tape 0's extent
    assert call(src=A1 - 4 * (2 * 60 - 1)) == -1 and b"overlaps src" in msg()           # the last float of src's extent
    assert call(src=A0 + 4 * 10) == -1 and b"overlaps src" in msg()


def test_descriptor_tables_are_packed_as_the_header_lays_them_out(lib):
    """``SlotTapes.run`` packs its tables as bytes: they must be the ctypes structures' bytes, field for field."""
    from vibravox_amd._lib import RATE_MAX_PIECES, RATE_MAX_SPLICES, EbenRatePiece, EbenRateSplice

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eben_hip.h")).read()
    assert f"#define EBEN_RATE_MAX_SPLICES {RATE_MAX_SPLICES}\n" in header and f"#define EBEN_RATE_MAX_PIECES {RATE_MAX_PIECES}\n" in header
    assert ctypes.sizeof(EbenRateSplice) == rate._SPLICE_POD.size == 24 and ctypes.sizeof(EbenRatePiece) == rate._PIECE_POD.size == 28
    s = rate.SlotSplice(slot=3, src_row=2, prev_off=11, n_carry=40, n_new=768, tape=1)
    assert bytes(EbenRateSplice(**s._asdict())) == rate._SPLICE_POD.pack(*s)
    p = rate.SlotPiece(slot=200, ratio=7, tape=1, length=808, p0=2, base0=-19, n_out=249, end=True, fifo=1, first_out=7)
    want = EbenRatePiece(len=p.length, p0=p.p0, base0=p.base0, n_out=p.n_out, end=1, first_out=p.first_out, slot=p.slot, ratio=p.ratio, tape=p.tape, fifo=p.fifo)
    assert bytes(want) == rate._PIECE_POD.pack(p.length, p.p0, p.base0, p.n_out, p.end, p.first_out, p.slot, p.ratio, p.tape, p.fifo)


def test_resample_slots_argument_errors_without_gpu(lib):
    from vibravox_amd._lib import EbenRatePiece, EbenRateRatio

    # 3:1 (width 19, 41 taps): a tape of 100 samples serves outputs up to q = 19 when its right end is not the signal's
    good = dict(slot=1, ratio=0, tape=0, len=100, p0=0, base0=0, n_out=20, end=0, fifo=1, first_out=5)

    def call(pieces=None, count=None, t0=A0, t1=A1, tp=200, f0=F0, f1=F1, fp=64, slots=4, ratios=((TAB, 3, 1, 19),), n_ratios=None, null_table=False, **change):
        pieces = [dict(good, **change)] if pieces is None else pieces
        table = None if null_table else (EbenRatePiece * max(1, len(pieces)))(*[EbenRatePiece(**p) for p in pieces])
        rt = (EbenRateRatio * max(1, len(ratios)))(*[EbenRateRatio(k, o, n, w, 0) for k, o, n, w in ratios])
        return lib.eben_resample_slots(V(t0), V(t1), tp, V(f0), V(f1), fp, slots, rt, len(ratios) if n_ratios is None else n_ratios, table,
                                       len(pieces) if count is None else count, None)

    msg = lib.eben_last_error
    assert call(pieces=[], count=0) == 0 and call(count=0, null_table=True) == 0
    assert call(n_out=0) == 0                                                            # checked and dropped: no launch
    assert call(null_table=True) == -1 and b"null" in msg()
    for k in ("t0", "t1", "f0", "f1"):
        assert call(**{k: 0}) == -1 and b"null" in msg(), k
        assert call(**{k: 0x700002}) == -1 and b"misaligned" in msg(), k
    assert call(ratios=((0, 3, 1, 19),)) == -1 and b"table of ratio 0" in msg() and call(ratios=((TAB + 2, 3, 1, 19),)) == -1
    assert call(count=-1) == -1 and call(pieces=[dict(good, first_out=0, n_out=0)] * 129) == -1 and b"at most 128" in msg()
    assert call(slots=0) == -1 and call(slots=257) == -1 and b"slots" in msg()
    assert call(slot=4) == -1 and b"names slot 4 of 4" in msg() and call(slot=-1) == -1
    assert call(ratio=1) == -1 and b"ratio 1 of 1" in msg() and call(ratio=-1) == -1
    assert call(n_ratios=9, ratios=((TAB, 3, 1, 19),) * 9) == -1 and b"ratios" in msg() and call(n_ratios=0) == -1
    assert call(tape=2) == -1 and call(fifo=-1) == -1 and b"0 or 1" in msg()
    assert call(ratios=((TAB, 5000, 1, 6),)) == -1 and b"fits no tile" in msg()
    assert call(ratios=((TAB, 0, 1, 19),)) == -1 and call(ratios=((TAB, 3, 1, -1),)) == -1
    assert call(len=201) == -1 and call(len=-1) == -1 and b"a tape of" in msg()
    assert call(first_out=45) == -1 and b"past the pitch" in msg() and call(first_out=-1) == -1 and call(n_out=-1) == -1
    assert call(p0=1) == -1 and b"phase 1 of 1" in msg() and call(p0=-1) == -1
    assert call(base0=0x7fff0001) == -1 and b"base index" in msg()
    assert call(n_out=21) == -1 and b"not the signal's end" in msg()                     # q = 20 reads index 100
    assert call(n_out=41, end=1) == -1 and b"reach past the signal" in msg()             # output 40 sits at input 120 >= 100
    two = [good, dict(good, first_out=24, n_out=10)]
    assert call(pieces=two) == -1 and b"another piece writes too" in msg()               # [5, 25) and [24, 34) of one (FIFO buffer, slot)
    assert call(f1=F0 + 4 * (4 * 64 - 1)) == -1 and b"FIFO buffers overlap" in msg()
    assert call(f0=A1 + 4 * (4 * 200 - 1)) == -1 and b"overlaps a tape" in msg()
    assert call(f1=A0 - 4 * (4 * 64 - 1)) == -1 and b"overlaps a tape" in msg()
    assert call(ratios=((F1 + 4 * (4 * 64 - 1), 3, 1, 19),)) == -1 and b"overlaps the table" in msg()
