"""Streaming enhancement: what a steady-state push of `vibravox_amd.streaming.StreamingEnhancer` costs, next to the whole-clip forward.

    python tools/stream_bench.py [--chunks 256,1024,4096,16128] [--streams 1,8,64] [--iters 5] [--out FILE]

Per (chunk, streams), the default generator EBENGenerator(4, 32, 2) on noise at 16 kHz:
  (a) `pushes` steady-state pushes of one enhancer (warmed up first, the stream simply goes on from pass to pass);
  (b) `gen(cut_to_valid_length(.))` of the same `streams x pushes x chunk` samples in one piece.
Each pass is timed with HIP events around all of its pushes; the two paths alternate within one session, medians of `--iters` passes.
Launches are counted as calls into libeben_hip.so (every one of them is one kernel launch) during one push.  The real-time factor is
the chunk's duration over the time of one push.  Prints one JSON line per configuration and a summary."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
FS = 16000


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="256,1024,4096,16128")   # 16128: 16000 rounded to the generator's multiple
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from enhance_bench import LaunchCounter
    from vibravox_amd.streaming import Splice, StreamingEnhancer
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "stream_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    lines = []
    for chunk in (int(c) for c in args.chunks.split(",")):
        for streams in (int(s) for s in args.streams.split(",")):
            pushes = max(4, min(64, 65536 // chunk))
            audio = 0.1 * torch.randn(streams, 1, pushes * chunk, device=dev)
            pieces = [audio[:, :, i * chunk : (i + 1) * chunk].contiguous() for i in range(pushes)]
            enhancer = StreamingEnhancer(gen, chunk, streams=streams)
            plan = enhancer.plan

            def stream_pass():
                with torch.no_grad():
                    return [enhancer.push(x) for x in pieces]

            def whole_pass():
                with torch.no_grad():
                    return gen(gen.cut_to_valid_length(audio))[0]

            with torch.no_grad():
                for _ in range(plan.warmup_pushes + 2):   # to the steady state: from here on every push returns a chunk
                    enhancer.push(pieces[0])
            assert all(o.shape[2] == chunk for o in stream_pass())
            whole_pass()
            torch.cuda.synchronize()
            with LaunchCounter() as c:
                with torch.no_grad():
                    enhancer.push(pieces[0])
            splices = sum(1 for o in plan.steady if isinstance(o, Splice) and o.n_carry + o.n_new)
            with LaunchCounter() as cw:
                whole_pass()
            times = {"stream": [], "whole": []}
            for _ in range(args.iters):
                for name, fn in (("stream", stream_pass), ("whole", whole_pass)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    t1.record()
                    t1.synchronize()
                    times[name].append(t0.elapsed_time(t1))
            ms_push = statistics.median(times["stream"]) / pushes
            ms_whole = statistics.median(times["whole"])
            audio_s = streams * pushes * chunk / FS
            line = dict(chunk=chunk, streams=streams, pushes=pushes, ms_per_push=round(ms_push, 3),
                        min_ms_per_push=round(min(times["stream"]) / pushes, 3), max_ms_per_push=round(max(times["stream"]) / pushes, 3),
                        launches_per_push=c.n, splices_per_push=splices, chunk_ms=round(1e3 * chunk / FS, 2),
                        real_time_factor=round(chunk / FS / (ms_push * 1e-3), 2),
                        stream_audio_seconds_per_second=round(audio_s / (ms_push * pushes * 1e-3), 0), whole_clip_ms=round(ms_whole, 3),
                        whole_clip_launches=cw.n, whole_clip_audio_seconds_per_second=round(audio_s / (ms_whole * 1e-3), 0),
                        latency_samples=plan.latency, lookahead_samples=plan.lookahead, state_bytes_per_stream=4 * plan.state_floats)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del enhancer, audio, pieces
    summary = [f"stream_bench on {torch.cuda.get_device_properties(0).name}: EBENGenerator(4, 32, 2) at 16 kHz, steady-state pushes against the whole-clip "
               f"forward of the same audio, medians of {args.iters} alternated passes",
               f"  {'chunk':>6} {'streams':>7} {'ms/push':>9} {'launches':>8} {'x real time':>11} {'audio-s/s':>10} {'whole clip audio-s/s':>21} {'state/stream':>13}"]
    for l in lines:
        summary.append(f"  {l['chunk']:>6} {l['streams']:>7} {l['ms_per_push']:>9.3f} {l['launches_per_push']:>8} {l['real_time_factor']:>11.2f} "
                       f"{l['stream_audio_seconds_per_second']:>10.0f} {l['whole_clip_audio_seconds_per_second']:>21.0f} "
                       f"{l['state_bytes_per_stream'] / 2 ** 20:>9.2f} MiB")
    one = next((l for l in lines if l["chunk"] == 256 and l["streams"] == 1), None)
    if one is not None:
        verdict = "less" if one["ms_per_push"] < one["chunk_ms"] else "NOT less"
        summary.append(f"  a 256-sample push on one stream takes {one['ms_per_push']:.3f} ms, {verdict} than the {one['chunk_ms']:.0f} ms it represents")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
