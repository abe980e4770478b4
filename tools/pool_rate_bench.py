"""Streaming sessions at the recording's rate: what a tick of `StreamPool(input_rates=(48000,))` costs with N sessions at 48 kHz pushing,
next to the three other ways of serving them.

    python tools/pool_rate_bench.py [--active 1,16,64] [--slots 64] [--chunk 256] [--ticks 16] [--iters 5] [--out FILE]

The default generator EBENGenerator(4, 32, 2) on noise, a pool of `--slots` slots with every slot holding a pooled session.  Per number N
of sessions that push in a tick:
  (rated) `pool.step` of N sessions at 48 kHz: the front (one splice launch, one resampling launch) and the masked steady run;
  (a) a pool of the same declaration (`input_rates=(48000,)`, so `tick` looks for rated sessions there too) ticking N sessions opened at
      the model's rate on audio resampled beforehand: the floor;
  (b) N `StreamingEnhancer(streams=1, input_rate=48000)`, one push each;
  (c) a `rate.StreamResampler` per stream in front of an unrated pool: N pushes of a resampler, then that pool's tick;
  (front) the front of (rated) alone -- `SlotFront.feed` and `SlotTapes.run` for N slots: its two launches and their host work;
  (feed), (book rated), (book plain): host work alone, nothing enqueued -- `SlotFront.feed` for N slots, and `PoolBook.tick` of N pooled
      sessions at 48 kHz and at the model's rate.  `book rated - book plain - feed` is what the book adds around the front (its list
      of rated sessions, a `FrontRun` and a `Hand` per session).
A pass is `--ticks` ticks, timed with HIP events around it and with the host's clock around its enqueue; the paths alternate within one
session, medians of `--iters` passes with their min and max.  Library calls are counted during one tick, on a handle that writes every
`eben_*` call down.  Prints one JSON line per N and a summary."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE, FS = 48000, 16000


class CountedLibrary:
    """The library handle with every `eben_*` call counted."""

    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("eben_") or name == "eben_last_error":
            return fn

        def counted(*args):
            self.n += 1
            return fn(*args)

        return counted


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--active", default="1,16,64")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import _lib, rate
    from vibravox_amd.streaming import PoolBook, StreamingEnhancer, StreamPool
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "pool_rate_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    chunk, slots, ticks = args.chunk, args.slots, args.ticks
    counted = CountedLibrary(_lib.load())
    _lib._lib = counted

    def calls(fn):
        fn()   # right behind a call of the same path: a change of batch shape rebuilds packed weight images, which is not the tick's
        counted.n = 0
        fn()
        return counted.n

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        t0.record()
        fn()
        t1.record()
        h1 = time.perf_counter()
        t1.synchronize()
        return t0.elapsed_time(t1), 1e3 * (h1 - h0)

    def medians(paths):
        got = {name: [] for name, _ in paths}
        for _ in range(args.iters):
            for name, fn in paths:
                got[name].append(timed(fn))
        return {name: dict(ms=statistics.median(d for d, _ in v) / ticks, host_ms=statistics.median(h for _, h in v) / ticks,
                           min_ms=min(d for d, _ in v) / ticks, max_ms=max(d for d, _ in v) / ticks) for name, v in got.items()}

    lines = []
    with torch.no_grad():
        rated = StreamPool(gen, chunk, slots=slots, input_rates=(RATE,)).prepare(dev, private=1)
        floor = StreamPool(gen, chunk, slots=slots, input_rates=(RATE,)).prepare(dev, private=1)
        plain = StreamPool(gen, chunk, slots=slots).prepare(dev, private=1)
        r_sessions, a_sessions, p_sessions = [rated.open(RATE) for _ in range(slots)], [floor.open() for _ in range(slots)], [plain.open() for _ in range(slots)]
        n_in = r_sessions[0].input_chunk_samples
        wide, narrow = 0.1 * torch.randn(1, 1, n_in, device=dev), 0.1 * torch.randn(1, 1, chunk, device=dev)
        for pool, sessions, x in ((rated, r_sessions, wide), (floor, a_sessions, narrow), (plain, p_sessions, narrow)):
            for s in sessions:   # one after the other to the steady state: a single private state serves them all
                while s.phase != "pooled":
                    pool.step({s: x})
        # the books alone (host only): every slot holds a pooled session
        books = {}
        for name, r in (("book_rated", RATE), ("book_plain", None)):
            book = PoolBook(gen, chunk, slots, rated.plan, (RATE,), FS)
            sessions = [book.open(r) for _ in range(slots)]
            for s in sessions:
                while s.phase != "pooled":
                    book.tick([s])
            books[name] = (book, sessions)
        for n in (int(a) for a in args.active.split(",")):
            assert 1 <= n <= slots
            r_feed = {s: 0.1 * torch.randn(1, 1, n_in, device=dev) for s in r_sessions[:: slots // n][:n]}
            p_sess = p_sessions[:: slots // n][:n]
            a_feed = {s: 0.1 * torch.randn(1, 1, chunk, device=dev) for s in a_sessions[:: slots // n][:n]}
            alone = [StreamingEnhancer(gen, chunk, input_rate=RATE) for _ in range(n)]
            resamplers = [rate.StreamResampler(RATE, FS, 1, n_in) for _ in range(n)]
            for _ in range(rated.plan.warmup_pushes + 3):
                for e, r in zip(alone, resamplers):
                    e.push(wide)
                    r.push(wide)
            front = rate.SlotFront(chunk, slots, (RATE,), FS, gen.multiple)
            tapes = rate.SlotTapes(front, dev)
            f_slots = [s.slot for s in r_feed]
            for slot in f_slots:
                front.open(slot, RATE)
            f_in = {slot: wide for slot in f_slots}

            feed_only = rate.SlotFront(chunk, slots, (RATE,), FS, gen.multiple)
            for slot in f_slots:
                feed_only.open(slot, RATE)
            feed_arg = [(slot, n_in) for slot in f_slots]
            book_ticks = {name: (lambda book=book, some=sessions[:: slots // n][:n]: book.tick(some)) for name, (book, sessions) in books.items()}

            def front_tick():
                splices, pieces, _ = front.feed([(slot, n_in) for slot in f_slots])
                tapes.run(splices, pieces, f_in)

            def resampled_tick():
                outs = {s: r.push(wide) for s, r in zip(p_sess, resamplers)}
                plain.step(outs)

            def alone_tick():
                for e in alone:
                    e.push(wide)

            ticks_of = dict(rated=lambda: rated.step(r_feed), a=lambda: floor.step(a_feed), b=alone_tick, c=resampled_tick, front=front_tick,
                            feed=lambda: feed_only.feed(feed_arg), **book_ticks)
            for fn in ticks_of.values():
                fn(), fn()
            assert all(v.shape == (1, 1, chunk) for v in rated.step(r_feed).values())
            launches = {name: calls(fn) for name, fn in ticks_of.items()}
            m = medians([(name, (lambda fn=fn: [fn() for _ in range(ticks)])) for name, fn in ticks_of.items()])
            line = dict(measure="rated_tick", chunk=chunk, slots=slots, active=n, input_rate=RATE, chunk_ms=round(1e3 * chunk / FS, 2))
            for name, v in m.items():
                line[name] = {k: round(x, 3) for k, x in v.items()}
                line[name]["library_calls"] = launches[name]
            line["rated_minus_a_ms"] = round(m["rated"]["ms"] - m["a"]["ms"], 3)
            line["rated_minus_a_host_ms"] = round(m["rated"]["host_ms"] - m["a"]["host_ms"], 3)
            line["a_spread_ms"] = round(m["a"]["max_ms"] - m["a"]["min_ms"], 3)
            line["book_beyond_feed_host_ms"] = round(m["book_rated"]["host_ms"] - m["book_plain"]["host_ms"] - m["feed"]["host_ms"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del alone, resamplers, front, tapes, feed_only

    names = (("rated", "rated tick"), ("a", "(a) resampled before"), ("b", "(b) N enhancers"), ("c", "(c) N resamplers + pool"), ("front", "front alone"))
    summary = [f"pool_rate_bench on {torch.cuda.get_device_properties(0).name}: EBENGenerator(4, 32, 2), chunk {chunk} ({1e3 * chunk / FS:.0f} ms), {slots} slots, "
               f"N sessions at {RATE} Hz push; medians of {args.iters} alternated passes of {ticks} ticks: device ms [min, max] / host ms of the enqueue "
               f"/ library calls, per tick"]
    for l in lines:
        summary.append(f"  N = {l['active']}")
        for key, title in names:
            v = l[key]
            summary.append(f"    {title:<24} {v['ms']:>8.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}] / {v['host_ms']:<8.3f} / {v['library_calls']}")
        summary.append(f"    rated - (a): {l['rated_minus_a_ms']:.3f} ms device, {l['rated_minus_a_host_ms']:.3f} ms host; (a)'s own spread {l['a_spread_ms']:.3f} ms")
        rest = l["rated_minus_a_ms"] - l["front"]["ms"] - l["book_beyond_feed_host_ms"]
        summary.append(f"      measured parts: the front alone (feed, two descriptor tables, the stacked input, two launches) {l['front']['ms']:.3f} ms, of it "
                       f"feed {l['feed']['host_ms']:.3f} ms host; PoolBook.tick host-only {l['book_rated']['host_ms']:.3f} ms rated, "
                       f"{l['book_plain']['host_ms']:.3f} ms at the model's rate: the book beyond feed {l['book_beyond_feed_host_ms']:.3f} ms")
        summary.append(f"      not measured: the remaining {rest:.3f} ms (a difference of medians; supposed: the FIFO views StreamPool._execute hands over per session)")
    summary.append("  every path is bound by the host's enqueue (device time by events = host time), so what a rated tick costs over (a) is host work that "
                   "grows with N, not the two launches: those are the front alone at N = 1")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
