"""Streaming sessions: what a tick of `vibravox_amd.streaming.StreamPool` costs, next to the two ways of serving N live streams without it.

    python tools/pool_bench.py [--active 1,16,64] [--slots 64] [--chunk 256] [--ticks 16] [--iters 5] [--out FILE]

The default generator EBENGenerator(4, 32, 2) on noise at 16 kHz, a pool of `--slots` slots with every slot holding a pooled session.
Per number N of sessions that push in a tick:
  (a) `pool.step` with N of the pooled sessions (one masked run of the steady-state list over all slots);
  (b) N `StreamingEnhancer(streams=1)`, one push each: the only correct way to serve N independent streams without the pool;
  (c) one lockstep `StreamingEnhancer(streams=N)` push: the floor -- the pool issues the same launches plus a mask;
  (d) `GeneratorEngine.stream_run_pooled` alone on a stacked input made once: (a) without the pool's per-session host work.
Then a tick in which one session warms up beside `slots - 1` pooled ones, and the move of a session into its slot and out of it.
A pass is `--ticks` ticks, timed with HIP events around it and with the host's clock around its enqueue; the paths alternate within one
session, medians of `--iters` passes.  Launches are counted as calls into libeben_hip.so during one tick.  Prints one JSON line per
measurement and a summary."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
FS = 16000


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

    from enhance_bench import LaunchCounter
    from vibravox_amd import gen_engine
    from vibravox_amd.streaming import StreamingEnhancer, StreamPool
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "pool_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    chunk, slots, ticks = args.chunk, args.slots, args.ticks
    noise = lambda rows: 0.1 * torch.randn(rows, 1, chunk, device=dev)

    def timed(fn):
        """(device ms, host ms of the enqueue) of one call."""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        t0.record()
        fn()
        t1.record()
        h1 = time.perf_counter()
        t1.synchronize()
        return t0.elapsed_time(t1), 1e3 * (h1 - h0)

    def medians(paths, per):
        """Alternates the paths `--iters` times; per path the medians (device, host) in ms per `per` calls of its unit."""
        got = {name: [] for name, _ in paths}
        for _ in range(args.iters):
            for name, fn in paths:
                got[name].append(timed(fn))
        return {name: (statistics.median(d for d, _ in v) / per, statistics.median(h for _, h in v) / per, min(d for d, _ in v) / per,
                       max(d for d, _ in v) / per) for name, v in got.items()}

    lines = []
    with torch.no_grad():
        pool = StreamPool(gen, chunk, slots=slots).prepare(dev, private=1)
        plan = pool.plan
        sessions = [pool.open() for _ in range(slots)]
        one = noise(1)
        for s in sessions:            # one after the other to the steady state: a single private state serves them all
            while s.phase != "pooled":
                pool.step({s: one})
        assert all(s.phase == "pooled" for s in sessions) and len(pool.private) == 1
        for n in (int(a) for a in args.active.split(",")):
            assert 1 <= n <= slots
            feed = {s: noise(1) for s in sessions[:: slots // n][:n]}
            alone = [StreamingEnhancer(gen, chunk) for _ in range(n)]
            lock = StreamingEnhancer(gen, chunk, streams=n)
            rows = noise(n)
            for _ in range(plan.warmup_pushes + 2):
                for e in alone:
                    e.push(one)
                lock.push(rows)
            assert all(v.shape == (1, 1, chunk) for v in pool.step(feed).values()) and lock.push(rows).shape == (n, 1, chunk)
            torch.cuda.synchronize()
            # each count right behind a call of the same path: the first forward after one of another batch shape rebuilds the packed
            # weight images, and those launches are not the tick's
            pool.step(feed)
            with LaunchCounter() as c_pool:
                pool.step(feed)
            lock.push(rows)
            with LaunchCounter() as c_lock:
                lock.push(rows)

            def pool_pass():
                for _ in range(ticks):
                    pool.step(feed)

            # the masked run alone, without the pool's per-session work (checks, the stacked input, a row view and a dict entry each)
            engine = gen_engine.engine_of(gen)
            compact = torch.cat(list(feed.values()), dim=0)
            mask = [0] * ((slots + 63) // 64)
            for s in feed:
                mask[s.slot >> 6] |= 1 << (s.slot & 63)

            def run_pass():
                for _ in range(ticks):
                    engine.stream_run_pooled(pool.state, plan.steady, compact, tuple(mask), n)

            def alone_pass():
                for _ in range(ticks):
                    for e in alone:
                        e.push(one)

            def lock_pass():
                for _ in range(ticks):
                    lock.push(rows)

            m = medians((("pool", pool_pass), ("run", run_pass), ("alone", alone_pass), ("lockstep", lock_pass)), ticks)
            line = dict(measure="tick", chunk=chunk, slots=slots, active=n, pool_ms=round(m["pool"][0], 3), pool_host_ms=round(m["pool"][1], 3),
                        pool_min_ms=round(m["pool"][2], 3), pool_max_ms=round(m["pool"][3], 3), masked_run_ms=round(m["run"][0], 3), masked_run_host_ms=round(m["run"][1], 3), enhancers_ms=round(m["alone"][0], 3),
                        enhancers_host_ms=round(m["alone"][1], 3), lockstep_ms=round(m["lockstep"][0], 3), lockstep_host_ms=round(m["lockstep"][1], 3),
                        pool_over_lockstep=round(m["pool"][0] / m["lockstep"][0], 3), enhancers_over_pool=round(m["alone"][0] / m["pool"][0], 2),
                        pool_launches=c_pool.n, lockstep_launches=c_lock.n, chunk_ms=round(1e3 * chunk / FS, 2))
            print(json.dumps(line), flush=True)
            lines.append(line)
            del alone, lock

        # one session warming up beside slots - 1 pooled ones: its private push and the pooled run in one tick
        pool.close(sessions.pop())
        rest = {s: noise(1) for s in sessions}
        warm_ticks = plan.warmup_pushes

        def warming_pass():
            s = pool.open()
            for _ in range(warm_ticks):
                pool.step({**rest, s: one})
            assert s.phase == "warming"
            pool.close(s)

        def pooled_pass():
            for _ in range(warm_ticks):
                pool.step(rest)

        warming_pass()
        m = medians((("warming", warming_pass), ("pooled", pooled_pass)), warm_ticks)
        line = dict(measure="warming_tick", chunk=chunk, pooled=slots - 1, warming=1, tick_ms=round(m["warming"][0], 3),
                    tick_host_ms=round(m["warming"][1], 3), pooled_only_ms=round(m["pooled"][0], 3), pooled_only_host_ms=round(m["pooled"][1], 3),
                    note="the warming pass also opens and closes its session once per pass")
        print(json.dumps(line), flush=True)
        lines.append(line)

        # the move of a session's state into a slot and out of it: one eben_copy_segments launch each
        private = pool._private_state(0)
        names, reps = pool.book.moved, 64
        engine.stream_move(pool.state, slots - 1, private, names, False)   # the private state at its steady lengths

        def moves(into_pool):
            return lambda: [engine.stream_move(pool.state, slots - 1, private, names, into_pool) for _ in range(reps)]

        def torch_copies():
            for _ in range(reps):
                for name in names:
                    pool.state.view(name)[slots - 1].copy_(private.view(name)[0])

        m = medians((("in", moves(True)), ("out", moves(False)), ("torch", torch_copies)), reps)
        floats = sum(private.view(name).numel() for name in names)
        line = dict(measure="move", tensors=len(names), floats=floats, move_in_us=round(1e3 * m["in"][0], 1), move_in_host_us=round(1e3 * m["in"][1], 1),
                    move_out_us=round(1e3 * m["out"][0], 1), move_out_host_us=round(1e3 * m["out"][1], 1),
                    torch_copies_us=round(1e3 * m["torch"][0], 1), torch_copies_host_us=round(1e3 * m["torch"][1], 1))
        print(json.dumps(line), flush=True)
        lines.append(line)

    summary = [f"pool_bench on {torch.cuda.get_device_properties(0).name}: EBENGenerator(4, 32, 2) at 16 kHz, chunk {chunk}, {slots} slots, medians of "
               f"{args.iters} alternated passes of {ticks} ticks (device ms by HIP events / host ms of the enqueue)",
               f"  {'active':>6} {'pool tick':>16} {'masked run alone':>16} {'N enhancers':>16} {'lockstep streams=N':>19} {'pool/lockstep':>13} {'enhancers/pool':>14} {'launches':>9}"]
    for l in lines:
        if l["measure"] == "tick":
            summary.append(f"  {l['active']:>6} {l['pool_ms']:>8.3f}/{l['pool_host_ms']:<7.3f} {l['masked_run_ms']:>8.3f}/{l['masked_run_host_ms']:<7.3f} {l['enhancers_ms']:>8.3f}/{l['enhancers_host_ms']:<7.3f} "
                           f"{l['lockstep_ms']:>10.3f}/{l['lockstep_host_ms']:<8.3f} {l['pool_over_lockstep']:>13.3f} {l['enhancers_over_pool']:>14.2f} "
                           f"{l['pool_launches']:>4}/{l['lockstep_launches']:<4}")
        elif l["measure"] == "warming_tick":
            summary.append(f"  one session warming beside {l['pooled']} pooled: {l['tick_ms']:.3f} ms per tick (host {l['tick_host_ms']:.3f}); the {l['pooled']} "
                           f"pooled alone: {l['pooled_only_ms']:.3f} ms (host {l['pooled_only_host_ms']:.3f})")
        else:
            summary.append(f"  move of a session ({l['tensors']} tensors, {l['floats']} floats): in {l['move_in_us']:.1f} us (host {l['move_in_host_us']:.1f}), out "
                           f"{l['move_out_us']:.1f} us (host {l['move_out_host_us']:.1f}); the same as {l['tensors']} torch copies: {l['torch_copies_us']:.1f} us "
                           f"(host {l['torch_copies_host_us']:.1f})")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
