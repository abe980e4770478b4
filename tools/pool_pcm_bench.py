"""Live sessions in and out as PCM at the caller's rate: what a tick of 64 sessions costs with 48 kHz PCM16 frames on both sides, next to
the float pool and next to the same service put together from the merged library calls.

    python tools/pool_pcm_bench.py [--slots 64] [--chunk 256] [--ticks 16] [--iters 7] [--out profiles/pool_pcm_bench.txt]

The benchmark's generator EBENGenerator(4, 32, 2) on noise, a pool of `--slots` slots with every slot holding a pooled session that pushes in
every tick:
  (a) today's float pool at the model's rate;
  (b) today's `StreamPool(input_rates=(48000,))`: float32 in at 48 kHz, float32 out at 16 kHz;
  (c) 48 kHz PCM16 in and out through the new path: `open(48000, output_rate=48000, output_format="PCM16", input_format="PCM16")` --
      one `eben_pcm_chunks_in` in front of (b)'s tick, one `eben_stream_pcm_out` behind it;
  (d) the same service from merged calls only: `eben_pcm_decode_ragged` in front of (b)'s tick; behind it the results stacked,
      `eben_rate_splice_slots`, `eben_resample_slots` and `eben_pcm_encode_ragged`, driven by the same `rate.SlotBack` numbers.
(c) and (d) get the same frames from the first tick on and run the same number of ticks, and the bytes of their last
tick are asserted equal.  A pass is `--ticks` ticks, timed with HIP events around it and with the host's clock around its enqueue; the
four paths alternate within one run, medians of `--iters` passes with their min and max.  Library calls are counted during one tick."""
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
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=16)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from vibravox_amd import _lib, corpus, rate
    from vibravox_amd._lib import EbenRatePiece, EbenRateRatio, EbenRateSplice, check, ptr, stream
    from vibravox_amd.streaming import StreamPool
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "pool_pcm_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    chunk, slots, ticks = args.chunk, args.slots, args.ticks
    counted = CountedLibrary(_lib.load())
    _lib._lib = counted

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

    with torch.no_grad():
        pools = dict(a=StreamPool(gen, chunk, slots=slots), b=StreamPool(gen, chunk, slots=slots, input_rates=(RATE,)),
                     c=StreamPool(gen, chunk, slots=slots, input_rates=(RATE,), output_rates=(RATE,)), d=StreamPool(gen, chunk, slots=slots, input_rates=(RATE,)))
        for p in pools.values():
            p.prepare(dev, private=1)
        ways = dict(a={}, b=dict(input_rate=RATE), c=dict(input_rate=RATE, output_rate=RATE, output_format="PCM16", input_format="PCM16"), d=dict(input_rate=RATE))
        sessions = {k: [pools[k].open(**ways[k]) for _ in range(slots)] for k in pools}
        n_in = sessions["b"][0].input_chunk_samples
        # one tick's frames: every session its own 48 kHz PCM16 frame, all in one byte buffer (a frame is a multiple of 16 bytes)
        assert (2 * n_in) % 16 == 0
        frames = (0.1 * torch.randn(slots, n_in)).clamp(-1, 1).mul(32767).round().to(torch.int16)
        data = frames.view(torch.uint8).reshape(-1).to(dev)
        wide = (frames.to(torch.float32) / 32768).to(dev)            # the same frames decoded, for (b)
        narrow = 0.1 * torch.randn(slots, 1, 1, chunk, device=dev)   # ... and model-rate noise for (a)
        feeds = dict(a={s: narrow[i] for i, s in enumerate(sessions["a"])}, b={s: wide[i].view(1, 1, n_in) for i, s in enumerate(sessions["b"])},
                     c={s: data[2 * n_in * i : 2 * n_in * (i + 1)] for i, s in enumerate(sessions["c"])})
        # (d): the merged decoder in front, the three merged kernels behind
        dec_rows = np.array([(2 * n_in * i, n_in, 1, 0, 0) for i in range(slots)], dtype=corpus.ROW_DTYPE)
        stage = torch.zeros(slots, n_in, device=dev)
        stage_views = [stage[i].view(1, 1, n_in) for i in range(slots)]
        back = rate.SlotBack(chunk, slots, (RATE,), FS, pools["c"].book.back.max_emit)
        orig, new, width = back.ratios[0]
        table = rate._table(FS, RATE, dev)[0]
        ratios = (EbenRateRatio * 1)(EbenRateRatio(table.data_ptr(), orig, new, width, 0))
        d_tapes = [torch.zeros(slots, back.tape_samples, device=dev) for _ in range(2)]
        fifo_pitch = new * back.max_emit // orig + new
        d_fifo = [torch.zeros(slots, fifo_pitch, device=dev) for _ in range(2)]
        d_last = {}
        for s in sessions["d"]:
            back.open(s.slot, RATE, "PCM16")

        def d_tick():
            corpus.pcm_to_rows(data, dec_rows, out=stage, pitch=n_in)
            outs = pools["d"].step({s: stage_views[i] for i, s in enumerate(sessions["d"])})
            k = outs[sessions["d"][0]].shape[2]
            if k == 0:
                return
            src = torch.cat([outs[s] for s in sessions["d"]], dim=0)
            pieces, ranges, nbytes = back.emit([(s.slot, i, k, False) for i, s in enumerate(sessions["d"])])
            lib = _lib.load()
            t = (EbenRateSplice * len(pieces))(*[EbenRateSplice(p.slot, p.src_row, p.prev_off, p.n_carry, p.n_new, p.tape) for p in pieces])
            check(lib.eben_rate_splice_slots(ptr(d_tapes[0]), ptr(d_tapes[1]), back.tape_samples, slots, ptr(src), k, slots, t, len(pieces), stream()),
                  "rate_splice_slots")
            t = (EbenRatePiece * len(pieces))(*[EbenRatePiece(p.n_carry + p.n_new, p.p0, p.base0, p.n_out, int(p.end), 0, p.slot, p.ratio, p.tape, 0) for p in pieces])
            check(lib.eben_resample_slots(ptr(d_tapes[0]), ptr(d_tapes[1]), back.tape_samples, ptr(d_fifo[0]), ptr(d_fifo[1]), fifo_pitch, slots, ratios, 1, t,
                                          len(pieces), stream()), "resample_slots")
            image = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            rows = np.array([(p.slot * fifo_pitch, p.byte_offset, p.n_out, 0) for p in pieces], dtype=corpus.ENC_ROW_DTYPE)
            d_last["image"], d_last["clipped"], d_last["nbytes"] = image, corpus.rows_to_pcm(d_fifo[0], rows, image), nbytes

        c_last = {}

        def c_tick():
            c_last["out"] = pools["c"].step(feeds["c"])

        tick_of = dict(a=lambda: pools["a"].step(feeds["a"]), b=lambda: pools["b"].step(feeds["b"]), c=c_tick, d=d_tick)
        # to the steady state: all sessions of a pool together (the private states are allocated once, before anything is timed)
        warm = pools["a"].plan.warmup_pushes + 4
        for _ in range(warm):
            for fn in tick_of.values():
                fn()
        assert all(s.phase == "pooled" for group in sessions.values() for s in group)
        calls = {}
        for name, fn in tick_of.items():
            fn()
            counted.n = 0
            fn()
            calls[name] = counted.n
        got = {name: [] for name in tick_of}
        for _ in range(args.iters):
            for name, fn in tick_of.items():
                got[name].append(timed(lambda fn=fn: [fn() for _ in range(ticks)]))
        # (c) and (d) saw the same frames for the same number of ticks: the same bytes
        torch.cuda.synchronize()
        n = d_last["nbytes"]
        assert n == 2 * 3 * chunk * slots and torch.equal(pools["c"].image[:n].cpu(), d_last["image"][:n].cpu()), "(c) and (d) differ in their bytes"
        for i, s in enumerate(sessions["c"]):
            assert torch.equal(c_last["out"][s].cpu(), d_last["image"][2 * 3 * chunk * i : 2 * 3 * chunk * (i + 1)].cpu())
        m = {name: dict(ms=statistics.median(d for d, _ in v) / ticks, host_ms=statistics.median(h for _, h in v) / ticks, min_ms=min(d for d, _ in v) / ticks,
                        max_ms=max(d for d, _ in v) / ticks, library_calls=calls[name]) for name, v in got.items()}

    line = dict(measure="pcm_tick", chunk=chunk, slots=slots, active=slots, rate=RATE, format="PCM16", chunk_ms=round(1e3 * chunk / FS, 2), bytes_equal=True)
    for name, v in m.items():
        line[name] = {k: round(x, 3) if isinstance(x, float) else x for k, x in v.items()}
    spread = lambda k: m[k]["max_ms"] - m[k]["min_ms"]   # noqa: E731
    line["c_minus_b_ms"] = round(m["c"]["ms"] - m["b"]["ms"], 3)
    line["c_minus_d_ms"] = round(m["c"]["ms"] - m["d"]["ms"], 3)
    line["spread_ms"] = {k: round(spread(k), 3) for k in m}
    faster = m["d"]["ms"] - m["c"]["ms"] > max(spread("c"), spread("d"))
    line["c_faster_than_d_beyond_spread"] = bool(faster)
    titles = dict(a="(a) float pool, 16 kHz", b="(b) float in at 48 kHz", c="(c) PCM16 in and out, 48 kHz", d="(d) the same, merged calls")
    summary = [f"pool_pcm_bench on {torch.cuda.get_device_properties(0).name}: EBENGenerator(4, 32, 2), chunk {chunk} ({1e3 * chunk / FS:.0f} ms), {slots} live "
               f"sessions push in every tick; medians of {args.iters} alternated passes of {ticks} ticks: device ms [min, max] / host ms of the enqueue / "
               f"library calls, per tick"]
    for k, title in titles.items():
        v = m[k]
        summary.append(f"    {title:<30} {v['ms']:>8.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}] / {v['host_ms']:<8.3f} / {v['library_calls']}")
    summary.append(f"  (c) - (b): {line['c_minus_b_ms']:.3f} ms a tick for PCM on both sides and the way back to 48 kHz; (c) - (d): {line['c_minus_d_ms']:.3f} ms; "
                   f"spreads (max - min of the passes): (c) {spread('c'):.3f} ms, (d) {spread('d'):.3f} ms")
    summary.append("  (c) is faster than (d) beyond the run's own spread" if faster else
                   "  (c) is NOT faster than (d) beyond the run's own spread: the single launch is not shown to pay here")
    summary.append("  the bytes of (c) and (d) were equal at the last tick, session by session")
    print(json.dumps(line), flush=True)
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
