"""Input at the recording's rate: what resampling inside the inference calls costs, against resampling clip by clip in front of them.

    python tools/rate_bench.py [--clips 256] [--iters 7] [--kernel-iters 50] [--push-iters 200] [--out FILE]

(a) Corpus: `--clips` clips with lengths uniform in 1 .. 12 s at 48 kHz (seed 0, the distribution of tools/enhance_bench.py) through
    EBENGenerator(4, 32, 2): `enhance_clips(clips, input_rate=48000)` against a loop of `augment.resample(c, 48000, 16000)` followed by
    `enhance_clips` -- what the package offered before.  The two alternate within one session; medians of `--iters` passes, HIP events
    around a whole pass.
(b) The ragged kernel alone on that corpus, the padded 48 kHz buffers packed ahead of time -- once as the batches `enhance_clips` makes
    (one launch each) and once as one buffer with a row per clip (one launch: the launch overhead paid once): bytes read (the rows' own
    samples) plus bytes written (the whole output buffers, zeros included) per second, medians of `--kernel-iters` passes; next to each
    a device-to-device torch copy of the same byte count, timed in the same run, the two alternating.
(c) A stream: one push of 768 samples with `StreamingEnhancer(gen, 256, input_rate=48000)` against one push of 256 samples at the
    model's rate, in the steady state; `--push-iters` pushes each per round, alternating rounds, HIP events around a round.
Prints one JSON line per measurement and a summary; `--out` writes both to a file."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IN, MODEL = 48000, 16000


def timed(torch, fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--push-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import augment, ragged, rate
    from vibravox_amd.inference import MAX_BATCH_SAMPLES, enhance_clips, resampled_length
    from vibravox_amd.streaming import StreamingEnhancer
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "rate_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1 * IN, 12 * IN + 1, size=args.clips)]
    clips = [(0.1 * torch.randn(1, 1, t)).to(dev) for t in lengths]
    at_model = [resampled_length(t, IN, MODEL) for t in lengths]
    audio_s = sum(lengths) / IN
    lines = []

    # ---- (a) the corpus ----------------------------------------------------------------------------------------------------------------
    def inside():
        return enhance_clips(gen, clips, input_rate=IN)

    def in_front():
        return enhance_clips(gen, [augment.resample(c, IN, MODEL) for c in clips])

    paths = [("resample_loop_then_enhance_clips", in_front), ("enhance_clips_input_rate", inside)]
    outs = {name: fn() for name, fn in paths}   # warm-up: weight images, allocator, code objects
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for a, b in zip(*outs.values()))
    del outs
    times = {name: [] for name, _ in paths}
    for _ in range(args.iters):
        for name, fn in paths:
            times[name].append(timed(torch, fn))
    for name, _ in paths:
        ms = statistics.median(times[name])
        lines.append(dict(part="a", path=name, clips=args.clips, audio_seconds=round(audio_s, 1), median_ms=round(ms, 2), min_ms=round(min(times[name]), 2),
                          max_ms=round(max(times[name]), 2), audio_seconds_per_second=round(audio_s / (ms * 1e-3), 0), results_equal=equal))
        print(json.dumps(lines[-1]), flush=True)

    # ---- (b) the ragged kernel alone -----------------------------------------------------------------------------------------------------
    def pack(groups):
        """[(raw, lens, out)] per group of clip indices, and the bytes a pass reads (the rows' own samples) plus writes (whole buffers)."""
        packed, nbytes = [], 0
        for idx, l_buf in groups:
            raw_lengths = [lengths[i] for i in idx]
            raw = torch.zeros((len(idx), 1, max(raw_lengths)), device=dev)
            for r, i in enumerate(idx):
                raw[r, 0, : raw_lengths[r]] = clips[i][0, 0]
            out = torch.empty((len(idx), 1, max(l_buf, resampled_length(raw.shape[2], IN, MODEL))), device=dev)
            packed.append((raw, torch.tensor(raw_lengths, dtype=torch.int32, device=dev), out))
            nbytes += 4 * (sum(raw_lengths) + out.numel())
        return packed, nbytes

    batches, _ = ragged.compose_batches(gen, at_model, MAX_BATCH_SAMPLES)
    layouts = [("batches_of_enhance_clips", [(idx, ragged.plan(gen, [at_model[i] for i in idx]).l_buf) for idx in batches]),
               ("whole_corpus_one_launch", [(list(range(args.clips)), 0)])]   # every clip a row of one buffer: the launch overhead paid once
    for layout, groups in layouts:
        packed, nbytes = pack(groups)
        src = torch.empty(nbytes // 8, device=dev)   # a copy reads and writes: half the bytes each way
        dst = torch.empty_like(src)

        def kernel_pass():
            for raw, lens, out in packed:
                rate.resample_ragged(raw, lens, IN, MODEL, out=out)

        def copy_pass():
            dst.copy_(src)

        for fn in (kernel_pass, copy_pass):
            fn()
        torch.cuda.synchronize()
        kt, ct = [], []
        for _ in range(args.kernel_iters):
            kt.append(timed(torch, kernel_pass))
            ct.append(timed(torch, copy_pass))
        for name, ts, launches in (("resample_ragged_kernel", kt, len(packed)), ("torch_device_copy_same_bytes", ct, 1)):
            ms = statistics.median(ts)
            lines.append(dict(part="b", layout=layout, path=name, bytes_read_plus_written=nbytes, launches=launches, median_ms=round(ms, 4),
                              min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), gigabytes_per_second=round(nbytes / (ms * 1e-3) / 1e9, 1)))
            print(json.dumps(lines[-1]), flush=True)

    # ---- (c) one push of a stream --------------------------------------------------------------------------------------------------------
    rated = StreamingEnhancer(gen, 256, input_rate=IN).prepare(dev)
    plain = StreamingEnhancer(gen, 256).prepare(dev)
    chunk48, chunk16 = 0.1 * torch.randn(1, 1, 768, device=dev), 0.1 * torch.randn(1, 1, 256, device=dev)
    with torch.no_grad():
        for _ in range(64):   # into the steady state
            rated.push(chunk48)
            plain.push(chunk16)

        def pushes(enhancer, chunk):
            for _ in range(args.push_iters):
                enhancer.push(chunk)

        torch.cuda.synchronize()
        pt = {"push_768_input_rate_48000": [], "push_256_model_rate": []}
        for _ in range(args.iters):
            pt["push_256_model_rate"].append(timed(torch, lambda: pushes(plain, chunk16)) / args.push_iters)
            pt["push_768_input_rate_48000"].append(timed(torch, lambda: pushes(rated, chunk48)) / args.push_iters)
    for name, ts in pt.items():
        ms = statistics.median(ts)
        lines.append(dict(part="c", path=name, pushes_per_round=args.push_iters, median_ms_per_push=round(ms, 4), min_ms_per_push=round(min(ts), 4),
                          max_ms_per_push=round(max(ts), 4), real_time_factor=round(16.0 / ms, 1)))
        print(json.dumps(lines[-1]), flush=True)

    a0, a1, b0, b1, b2, b3, c0, c1 = lines
    summary = [
        f"rate_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} clips of 1-12 s at 48 kHz ({audio_s:.0f} s of audio), EBENGenerator(4, 32, 2)",
        f"  (a) resample loop, then enhance_clips : {a0['median_ms']:9.2f} ms  (min {a0['min_ms']}, max {a0['max_ms']}; medians of {args.iters} alternated passes)",
        f"      enhance_clips(input_rate=48000)   : {a1['median_ms']:9.2f} ms  (min {a1['min_ms']}, max {a1['max_ms']}): {a0['median_ms'] / a1['median_ms']:.3f}x the loop's "
        f"speed; results equal: {equal}",
    ]
    for k, c in ((b0, b1), (b2, b3)):
        summary += [
            f"  (b) ragged kernel alone, {k['layout']}, {k['launches']} launch(es): {k['median_ms']:9.4f} ms  {k['gigabytes_per_second']:8.1f} GB/s read + "
            f"written ({k['bytes_read_plus_written']} bytes; medians of {args.kernel_iters}, HIP events around the pass, host enqueue included)",
            f"      torch copy of the same byte count : {c['median_ms']:9.4f} ms  {c['gigabytes_per_second']:8.1f} GB/s: the kernel runs at "
            f"{c['median_ms'] / k['median_ms']:.2f}x the copy's rate"]
    summary += [
        f"  (c) push of 256 at the model's rate   : {c1['median_ms_per_push']:9.4f} ms per push",
        f"      push of 768 with input_rate=48000 : {c0['median_ms_per_push']:9.4f} ms per push: {c0['median_ms_per_push'] - c1['median_ms_per_push']:+.4f} ms "
        f"({c0['median_ms_per_push'] / c1['median_ms_per_push']:.3f}x) for a chunk of 16 ms",
    ]
    if a1["median_ms"] >= a0["median_ms"]:
        summary.append("  (a) does NOT beat resampling in front: the interface and the stream route stand on their own")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
