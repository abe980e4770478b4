"""GPU: ``StreamPool`` sessions at a recording rate -- ``eben_rate_splice_slots`` and ``eben_resample_slots`` through their raw entry points
(against torch indexing and against ``eben_resample_stream`` on each row alone, bit for bit), ``rate.SlotFront`` / ``rate.SlotTapes``
against ``augment.resample`` of the whole clip, and ``streaming.StreamPool(input_rates=...)`` against an unrated pool fed the resampled
clip -- all for EQUALITY: the per-slot kernels run the arithmetic of the kernels they stand beside, and the generator behind the front
gets the bits it would get from ``augment.resample``."""
import functools

import pytest
import torch

from formula import formula_audio
from tests import pool_oracle as P
from tests import pool_rate_oracle as PR
from tests import ragged_oracle as R
from tests.test_gpu_stream import body, fenced, fences_intact, same_bits
from vibravox_amd import augment, rate, streaming

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAN = float("nan")
FREQS = (48000, 44100, 24000, 8000, 32000)   # 3:1, 441:160, 3:2, 1:2, 2:1 to 16 kHz: all three table routes


def poisoned(slots, pitch, tag, named):
    """``fenced`` rows with NaN in every slot that is not named."""
    flat, dev, view = fenced(slots, pitch, tag)
    for r in range(slots):
        if r not in named:
            body(flat, slots, pitch)[r] = NAN
            view[r] = NAN
    return flat, dev, view


# ---- the splice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [3, 70])
def test_splice_slots_equals_torch_indexing(hip, slots):
    from vibravox_amd._lib import EbenRateSplice, check, stream

    pitch, sp, rows = 700, 300, 5
    # (slot, src_row, prev_off, n_carry, n_new, tape): every count its own; a carry alone, new samples alone, the whole pitch, one sample
    descs = [(0, 4, 3, 40, 257, 1), (slots - 1, 0, 0, 0, 300, 0), (1, 2, 699, 1, 0, 1)]
    if slots > 3:
        descs += [(7, 1, 100, 400, 300, 0), (64, 3, 17, 0, 1, 1), (33, 0, 0, 474, 226, 0)]
    named = {d[0] for d in descs}
    f0, d0, v0 = poisoned(slots, pitch, f"slots/{slots}/tape0", named)
    f1, d1, v1 = poisoned(slots, pitch, f"slots/{slots}/tape1", named)
    fs, ds, vs = fenced(rows, sp, f"slots/{slots}/src")
    table = (EbenRateSplice * len(descs))(*[EbenRateSplice(*d) for d in descs])
    check(hip.eben_rate_splice_slots(v0.data_ptr(), v1.data_ptr(), pitch, slots, vs.data_ptr(), sp, rows, table, len(descs), stream()), "rate_splice_slots")
    want = [f0.clone(), f1.clone()]
    before = [body(f0, slots, pitch), body(f1, slots, pitch)]
    for slot, row, po, nc, nn, tape in descs:
        w = body(want[tape], slots, pitch)
        w[slot, :nc] = before[1 - tape][slot, po : po + nc]
        w[slot, nc : nc + nn] = body(fs, rows, sp)[row, :nn]
    for got, w in ((d0.cpu(), want[0]), (d1.cpu(), want[1])):
        assert same_bits(got, w) and fences_intact(got)      # un-named slots, the rest of each pitch and the fences included
    assert same_bits(ds.cpu(), fs)


# ---- the resampling -------------------------------------------------------------------------------------------------------------------
def piece_cases():
    """(ratio index, len, p0, base0, n_out, end) of the launches one call makes: per ratio the left edge, a steady position with an odd
    phase, the signal's end with a tail of one sample; n_out of 1, 256 and 1280; a small push split at every point."""
    out = []
    for i, f in enumerate(FREQS):
        orig, new, width = rate.ratio(f, 16000)
        taps = 2 * width + orig

        def served(p0, base0, n_out):   # the shortest tape whose right end is not the signal's that serves the launch
            return base0 + ((p0 + n_out - 1) // new) * orig + taps

        out.append((i, served(0, -width, 256), 0, -width, 256, 0))                       # the left edge: base0 < 0
        p0 = 7 if new == 160 else 1 if new > 1 else 0
        out.append((i, served(p0, 5, 256) + 3, p0, 5, 256, 0))                           # steady, odd phase where the ratio has phases
        out.append((i, 1, 0, -width, -(-new // orig), 1))                                # end = 1 on a tail of 1 sample
        out.append((i, served(p0, 2, 1), p0, 2, 1, 0))                                   # a single output
    for i in (0, 1):   # 1280 outputs: 3:1 crosses its 1024-output tile, 441:160 its 960-output tile
        orig, new, width = rate.ratio(FREQS[i], 16000)
        out.append((i, 1 + ((1 + 1279) // new) * orig + 2 * width + orig, 1 if new > 1 else 0, 1, 1280, 0))
    orig, new, width = rate.ratio(24000, 16000)   # 3:2: a push of 9 outputs at p0 = 1, whole and split at every point
    push = rate.RatePush(0, 0, 0, 1, 4, 9, False)
    length = 4 + ((1 + 8) // new) * orig + 2 * width + orig
    assert length == SPLIT_LEN
    out.append((2, length, 1, 4, 9, 0))
    for k in range(1, 9):
        out.append((2, length, 1, 4, k, 0))
        out.append((2, length, *push.piece(k, orig, new), 9 - k, 0))
    return out


SPLIT_LEN = 39   # the tape length of the split push: no other case of its ratio has it


@pytest.mark.parametrize("slots", [3, 70])
def test_resample_slots_equals_resample_stream_on_each_row(hip, slots):
    from vibravox_amd._lib import EbenRatePiece, EbenRateRatio, check, stream

    tiles = [rate.tile(*rate.ratio(f, 16000)) for f in FREQS]
    assert [t["outputs_per_block"] for t in tiles[:2]] == [1024, 960] and [t["table_in_lds"] for t in tiles] == [True, False, True, True, True]
    cases = piece_cases()
    tp, fp = 4100, 1300 if slots > 3 else 3400
    assert max(c[1] for c in cases) <= tp
    # a (slot, FIFO buffer, first_out) per piece: spread over the slots, ranges of one (slot, buffer) 3 apart
    used, pieces = {}, []
    order = sorted(range(len(cases)), key=lambda i: -cases[i][4])
    for n, i in enumerate(order):
        ratio, length, p0, base0, n_out, end = cases[i]
        split = ratio == 2 and length == SPLIT_LEN   # the split push and its halves read one tape row
        slot, tape = (slots - 1, 1) if split else ((11 * n + 1) % slots, (n // 3) % 2)
        fifo = n % 2
        first = used.get((slot, fifo), 2)
        used[(slot, fifo)] = first + n_out + 3
        assert first + n_out <= fp
        pieces.append(dict(slot=slot, ratio=ratio, tape=tape, len=length, p0=p0, base0=base0, n_out=n_out, end=end, fifo=fifo, first_out=first))
    assert len(pieces) <= 64 and {p["ratio"] for p in pieces} == set(range(5))
    named = {p["slot"] for p in pieces}
    tapes = [poisoned(slots, tp, f"pieces/{slots}/tape{k}", named) for k in (0, 1)]
    fifos = [poisoned(slots, fp, f"pieces/{slots}/fifo{k}", named) for k in (0, 1)]
    tables = [rate._table(f, 16000, DEV)[0] for f in FREQS]
    ratios = (EbenRateRatio * 5)(*[EbenRateRatio(t.data_ptr(), *rate.ratio(f, 16000), 0) for t, f in zip(tables, FREQS)])
    table = (EbenRatePiece * len(pieces))(*[EbenRatePiece(**p) for p in pieces])
    check(hip.eben_resample_slots(tapes[0][2].data_ptr(), tapes[1][2].data_ptr(), tp, fifos[0][2].data_ptr(), fifos[1][2].data_ptr(), fp, slots, ratios, 5,
                                  table, len(pieces), stream()), "resample_slots")
    want = [fifos[0][0].clone(), fifos[1][0].clone()]
    for p in pieces:
        orig, new, width = rate.ratio(FREQS[p["ratio"]], 16000)
        row = tapes[p["tape"]][2][p["slot"]]
        alone = torch.full((p["n_out"] + 2,), NAN, device=DEV)
        check(hip.eben_resample_stream(row.data_ptr(), tables[p["ratio"]].data_ptr(), alone.data_ptr(), 1, tp, p["len"], p["n_out"] + 2, 1, p["n_out"], p["p0"],
                                       p["base0"], p["end"], orig, new, width, stream()), "resample_stream")
        alone = alone.cpu()
        assert not torch.isnan(alone[1:-1]).any() and torch.isnan(alone[0]) and torch.isnan(alone[-1]), p
        body(want[p["fifo"]], slots, fp)[p["slot"], p["first_out"] : p["first_out"] + p["n_out"]] = alone[1:-1]
    for k in (0, 1):
        got = fifos[k][1].cpu()
        assert same_bits(got, want[k]) and fences_intact(got), k   # each piece its row's bits; everything else as it was
        assert same_bits(tapes[k][1].cpu(), tapes[k][0])
    # the two halves of every split push are the whole push's bits
    got = [body(fifos[k][1].cpu(), slots, fp) for k in (0, 1)]
    wrote = lambda p: got[p["fifo"]][p["slot"], p["first_out"] : p["first_out"] + p["n_out"]]
    split = [p for p in pieces if p["ratio"] == 2 and p["len"] == SPLIT_LEN]
    whole_push = [p for p in split if p["n_out"] == 9]
    assert len(split) == 17 and len(whole_push) == 1
    for k in range(1, 9):
        first = [p for p in split if p["n_out"] == k and (p["p0"], p["base0"]) == (1, 4)]
        second = [p for p in split if p["n_out"] == 9 - k and (p["p0"], p["base0"]) != (1, 4)]
        assert len(first) == len(second) == 1, k
        assert same_bits(torch.cat([wrote(first[0]), wrote(second[0])]), wrote(whole_push[0])), k


def test_slot_entries_refuse_bad_arguments_and_write_nothing(hip):
    from vibravox_amd._lib import EbenRatePiece, EbenRateRatio, EbenRateSplice, stream

    slots, tp, fp = 4, 200, 64
    t = [fenced(slots, tp, f"slots/bad/tape{k}") for k in (0, 1)]
    f = [fenced(slots, fp, f"slots/bad/fifo{k}") for k in (0, 1)]
    fs, ds, vs = fenced(2, 60, "slots/bad/src")
    k = rate._table(48000, 16000, DEV)[0]
    ratios = (EbenRateRatio * 1)(EbenRateRatio(k.data_ptr(), 3, 1, 19, 0))
    sgood = dict(slot=1, src_row=0, prev_off=10, n_carry=40, n_new=60, tape=1)
    pgood = dict(slot=1, ratio=0, tape=0, len=100, p0=0, base0=0, n_out=20, end=0, fifo=1, first_out=5)

    def splice(descs, count=None, slots=slots, rows=2):
        table = (EbenRateSplice * len(descs))(*[EbenRateSplice(**d) for d in descs])
        return hip.eben_rate_splice_slots(t[0][2].data_ptr(), t[1][2].data_ptr(), tp, slots, vs.data_ptr(), 60, rows, table, len(descs) if count is None else count,
                                          stream())

    def pieces(descs, count=None, n_ratios=1, f1=None):
        table = (EbenRatePiece * len(descs))(*[EbenRatePiece(**d) for d in descs])
        return hip.eben_resample_slots(t[0][2].data_ptr(), t[1][2].data_ptr(), tp, f[0][2].data_ptr(), f[1][2].data_ptr() if f1 is None else f1, fp, slots, ratios,
                                       n_ratios, table, len(descs) if count is None else count, stream())

    bad_splices = [[dict(sgood, slot=4)], [dict(sgood, src_row=2)], [sgood, dict(sgood, src_row=1)], [dict(sgood, n_new=61)], [dict(sgood, prev_off=161)],
                   [dict(sgood, tape=2)], [dict(sgood, n_carry=0, n_new=0)], [dict(sgood, slot=i % 4) for i in range(65)]]
    for descs in bad_splices:
        assert splice(descs) == -1 and hip.eben_last_error(), descs
    bad_pieces = [[dict(pgood, slot=4)], [dict(pgood, ratio=1)], [pgood, dict(pgood, first_out=24, n_out=10)], [dict(pgood, n_out=21)], [dict(pgood, p0=1)],
                  [dict(pgood, len=201)], [dict(pgood, first_out=45)], [dict(pgood, fifo=2)], [dict(pgood, n_out=0)] * 129]
    for descs in bad_pieces:
        assert pieces(descs) == -1 and hip.eben_last_error(), descs
    assert pieces([pgood], f1=t[0][2].data_ptr()) == -1 and b"overlaps a tape" in hip.eben_last_error()
    assert splice([], 0) == 0 and pieces([pgood], 0) == 0 and pieces([dict(pgood, n_out=0)]) == 0   # nothing to do: no launch
    torch.cuda.synchronize()
    for flat, dev, _ in t + f:
        assert same_bits(dev.cpu(), flat)             # nothing was written
    assert splice([sgood]) == 0 and pieces([pgood]) == 0   # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert not same_bits(t[1][1].cpu(), t[1][0]) and not same_bits(f[1][1].cpu(), f[1][0]) and same_bits(t[0][1].cpu(), t[0][0])
    assert all(fences_intact(dev.cpu()) for _, dev, _ in t + f)


# ---- the front on the device -------------------------------------------------------------------------------------------------------------
def drive_front(front, tapes, signals, plan):
    """``plan``: slot -> (rate, opening tick, ticks skipped).  Every slot pushes whole chunks of its (1, 1, T) signal while it has one, then
    ends with its tail.  Returns slot -> the chunks handed on, concatenated."""
    got, pos, ended = {s: [] for s in plan}, {s: 0 for s in plan}, set()
    for tick in range(40):
        feed = []
        for slot, (r, start, skips) in plan.items():
            if tick == start:
                front.open(slot, r)
            n_in = front.input_chunk[front.rates.index(r)]
            if tick >= start and tick not in skips and slot not in ended:
                if signals[slot].shape[2] - pos[slot] >= n_in:
                    feed.append((slot, n_in))
                else:
                    splices, pieces, chunks = front.feed([(slot, signals[slot].shape[2] - pos[slot])], final=True)
                    tapes.run(splices, pieces, {slot: signals[slot][:, :, pos[slot] :].contiguous()})
                    got[slot] += [tapes.chunk(c).clone() for c in chunks[slot]]
                    ended.add(slot)
                    front.release(slot)
        if feed:
            splices, pieces, chunks = front.feed(feed)
            tapes.run(splices, pieces, {slot: signals[slot][:, :, pos[slot] : pos[slot] + n].contiguous() for slot, n in feed})
            for slot, n in feed:
                got[slot] += [tapes.chunk(c).clone() for c in chunks[slot]]
                pos[slot] += n
    assert ended == set(plan)
    return {s: torch.cat(v, dim=2) for s, v in got.items()}


@pytest.mark.parametrize("chunk,freqs", [(1280, (48000, 44100, 24000, 8000)), (256, (48000, 32000, 8000))])
def test_front_hands_on_augment_resample_of_the_whole_clip(hip, chunk, freqs):
    front = rate.SlotFront(chunk, len(freqs) + 2, freqs, 16000, 256)
    tapes = rate.SlotTapes(front, DEV)
    plan = {slot + 1: (r, slot % 3, (slot + 3,)) for slot, r in enumerate(freqs)}   # slots 0 and the last one hold no session
    signals = {}
    for slot, (r, _, _) in plan.items():
        n_in = front.input_chunk[front.rates.index(r)]
        signals[slot] = formula_audio(f"front/{chunk}/{r}", 1, 3 * n_in + (0, 1, n_in - 1, 40)[slot % 4]).to(DEV)

    def poison():
        for t in tapes.tapes + tapes.fifo:
            t.fill_(NAN)

    poison()
    ptrs = [t.data_ptr() for t in tapes.tapes + tapes.fifo]
    clean = drive_front(front, tapes, signals, plan)
    for slot, (r, _, _) in plan.items():
        want = augment.resample(signals[slot], r, 16000)
        assert clean[slot].shape == want.shape and torch.equal(clean[slot], want), (slot, r)
    for t in tapes.tapes + tapes.fifo:   # the slots without a session were never written
        assert torch.isnan(t[0]).all() and torch.isnan(t[-1]).all()
    for keep in plan:                    # the others push NaN audio: no bit of this session changes
        poison()
        noisy = {s: x if s == keep else torch.full_like(x, NAN) for s, x in signals.items()}
        assert same_bits(drive_front(front, tapes, noisy, plan)[keep], clean[keep]), keep
    assert ptrs == [t.data_ptr() for t in tapes.tapes + tapes.fifo]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(chunk):
    """The mixed-rate scenario of a chunk size: generator, spec, clips at their own rates and ``augment.resample`` of each."""
    p, slots, lengths, rates = (2, 4, P.SCENARIO_256, PR.RATES_256) if chunk == 256 else (1, 5, PR.SCENARIO_1280, PR.RATES_1280)
    gen = R.formula_generator(p, 32)[0].to(DEV)
    spec = PR.rated_scenario(lengths, rates)
    clips = {name: formula_audio(f"pool_rate/{name}", 1, total).to(DEV) for name, total, _, _, _ in spec}
    at_model = {name: clips[name] if r == 16000 else augment.resample(clips[name], r, 16000) for name, _, _, _, r in spec}
    return gen, slots, spec, clips, at_model


def joined(outs):
    return {name: tuple(torch.cat([o[k] for o in res], dim=2) for k in (0, 1)) for name, res in outs.items()}


def state_pointers(pool):
    return ([t.data_ptr() for pair in pool.state.buffers.values() for t in pair] + [t.data_ptr() for t in pool.tapes.tapes + pool.tapes.fifo]
            + [t.data_ptr() for st in pool.private.values() for pair in st.buffers.values() for t in pair])


@pytest.mark.parametrize("chunk", [256, 1280])
def test_rated_sessions_equal_unrated_sessions_on_the_resampled_clip(hip, chunk):
    gen, slots, spec, clips, at_model = case(chunk)
    rates = sorted({r for *_, r in spec})
    with torch.no_grad():
        pool = streaming.StreamPool(gen, chunk, slots=slots, return_bands=True, input_rates=rates).prepare(DEV, private=slots)
        for t in pool.tapes.tapes + pool.tapes.fifo:
            t.fill_(NAN)
        ptrs = state_pointers(pool)
        outs, slot_of, sessions = PR.run_rated_scenario(pool, clips, spec)
        plain_spec = tuple((name, at_model[name].shape[2], start, skips, None) for name, _, start, skips, _ in spec)
        plain = streaming.StreamPool(gen, chunk, slots=slots, return_bands=True)
        plain_outs, _, _ = PR.run_rated_scenario(plain, at_model, plain_spec)
        got, want = joined(outs), joined(plain_outs)
        for name, _, _, _, r in spec:
            for a, b in zip(got[name], want[name]):
                assert a.shape == b.shape and not torch.isnan(a).any() and torch.equal(a, b), (name, r)
            sizes, plain_sizes = [o[0].shape[2] for o in outs[name][:-1]], [o[0].shape[2] for o in plain_outs[name][:-1]]
            first = next((i for i, k in enumerate(sizes) if k), len(sizes))
            assert all(k == 0 for k in sizes[:first]) and all(k == chunk for k in sizes[first:]), (name, sizes)
            s = sessions[name]
            if r != 16000:
                orig, new, _ = rate.ratio(r, 16000)
                plain_first = next((i for i, k in enumerate(plain_sizes) if k), len(plain_sizes))
                if plain_first < len(plain_sizes) and first < len(sizes):
                    assert first == plain_first + 1, (name, first, plain_first)   # the FIFO in front: one push later
                for k in range(first, len(sizes)):
                    assert (k + 1) * s.input_chunk_samples - (k + 1 - first) * chunk * orig // new == s.input_latency, (name, k)
                # printed, not asserted: a stream of its own through StreamingEnhancer(input_rate=r), and the whole-clip forward
                alone = streaming.StreamingEnhancer(gen, chunk, 1, True, input_rate=r)
                n_in, x = alone.input_chunk_samples, clips[name]
                res = [alone.push(x[:, :, i : i + n_in]) for i in range(0, x.shape[2] - n_in + 1, n_in)]
                res.append(alone.finish(x[:, :, len(res) * n_in :]))
                assert [o[0].shape[2] for o in res[:-1]] == sizes, name            # the return sizes are StreamingEnhancer's
                single = torch.cat([o[0] for o in res], dim=2)
                whole = gen(gen.cut_to_valid_length(at_model[name]))
                whole = whole[0] if isinstance(whole, tuple) else whole
                print(f"chunk {chunk} {name} at {r} Hz: max|pool - StreamingEnhancer| {float((got[name][0] - single).abs().max()):.1e}, "
                      f"max|pool - whole clip| {float((got[name][0] - whole).abs().max()):.1e}")
        # a second scenario on the same pool allocates nothing and gives a fresh pool's results
        again, _, _ = PR.run_rated_scenario(pool, clips, spec)
        assert state_pointers(pool)[: len(ptrs)] == ptrs and len(state_pointers(pool)) == len(ptrs)
        for name, pair in joined(again).items():
            assert all(torch.equal(a, b) for a, b in zip(pair, got[name])), name


# ---- library calls ------------------------------------------------------------------------------------------------------------------------
class Counted:
    """The library handle with every ``eben_*`` call written down."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("eben_") or name == "eben_last_error":
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)

        return counted


def steady_tick_calls(counted, gen, n, input_rates, input_rate):
    """The library calls of one tick in which ``n`` pooled sessions of a 64-slot pool push (after every session has reached its slot)."""
    pool = streaming.StreamPool(gen, 256, slots=64, input_rates=input_rates).prepare(DEV, private=1)
    sessions = [pool.open(input_rate) for _ in range(n)]
    chunk = torch.zeros(1, 1, sessions[0].input_chunk_samples, device=DEV)
    for s in sessions:   # one by one through the same private state
        while s.phase != "pooled":
            pool.step({s: chunk})
    pool.step({s: chunk for s in sessions})
    counted.calls.clear()
    out = pool.step({s: chunk for s in sessions})
    calls = list(counted.calls)
    assert all(o.shape == (1, 1, 256) for o in out.values())
    return calls


def test_a_rated_tick_costs_two_library_calls_more(hip, monkeypatch):
    from vibravox_amd import _lib

    counted = Counted(hip)
    monkeypatch.setattr(_lib, "_lib", counted)
    gen = case(256)[0]
    new = ["eben_rate_splice_slots", "eben_resample_slots"]
    with torch.no_grad():
        for n in (1, 64):
            today = steady_tick_calls(counted, gen, n, (), None)
            assert len(today) > 20 and not set(today) & set(new)
            assert steady_tick_calls(counted, gen, n, (48000,), None) == today         # declared, not used: today's calls in today's order
            rated = steady_tick_calls(counted, gen, n, (48000,), 48000)
            assert rated == new + today, (n, len(rated), len(today))                    # the front first, then exactly today's tick
            print(f"{n} sessions: {len(today)} library calls a tick at the model's rate, {len(rated)} at 48 kHz")


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_the_rated_pool_checks_its_arguments(hip):
    from vibravox_amd._lib import EbenError

    gen = case(256)[0]
    pool = streaming.StreamPool(gen, 256, slots=2, input_rates=(48000,))
    s = pool.open(48000)
    with torch.no_grad():
        with pytest.raises(ValueError, match="768"):
            pool.step({s: torch.zeros(1, 1, 256, device=DEV)})
        with pytest.raises(EbenError, match="no CPU path"):
            pool.step({s: torch.zeros(1, 1, 768)})
    with pytest.raises(RuntimeError, match="no backward"):
        pool.step({s: torch.zeros(1, 1, 768, device=DEV)})
    with torch.no_grad():
        with pytest.raises(ValueError, match="too short"):
            pool.close(s, torch.zeros(1, 1, 100, device=DEV))
        assert s.phase == "warming"
        x = formula_audio("pool_rate/args", 1, 768 * 12 + 5).to(DEV)
        res = [pool.step({s: x[:, :, i * 768 : (i + 1) * 768]})[s] for i in range(12)]
        res.append(pool.close(s, x[:, :, 12 * 768 :]))
        want = gen(gen.cut_to_valid_length(augment.resample(x, 48000, 16000)))
        want = want[0] if isinstance(want, tuple) else want
        got = torch.cat(res, dim=2)
        assert res[0].shape == (1, 1, 0) and got.shape == want.shape and float((got - want).abs().max()) < 2e-5
        with pytest.raises(RuntimeError, match="closed"):
            pool.step({s: x[:, :, :768]})
        with pytest.raises(RuntimeError, match="closed"):
            pool.close(s)
