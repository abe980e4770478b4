"""Enhancing a corpus of utterances of different lengths: the loop of batch-1 generator forwards against ragged batches.

    python tools/enhance_bench.py [--clips 256] [--iters 5] [--budgets 1048576,4194304] [--out FILE]

Workload: `--clips` clips with lengths uniform in 1 .. 12 s at 16 kHz (seed 0) through the default generator EBENGenerator(4, 32, 2).
  (a) for every clip `gen(cut_to_valid_length(clip))` -- the evaluation path, one forward per clip;
  (b) `vibravox_amd.inference.enhance_clips`, once per `max_batch_samples` budget.
Each pass is timed with HIP events around the whole corpus; the paths alternate within one session, one warm-up pass each, medians of
`--iters` passes.  The batches of the last budget are also timed packed ahead of time, through `forward_ragged` and through the plain
batched forward (the same launches without the fills): what the fills and what packing and unpacking cost.  Launches are counted as calls into libeben_hip.so (every one of them is one kernel launch); the copies torch makes
to pack and unpack the clips are listed beside them.  Prints one JSON line per path and a summary."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 16000


class LaunchCounter:
    """Counts the library calls made through `check` in the modules on the generator's forward path."""

    def __init__(self):
        from vibravox_amd import gen_engine, ops

        self.modules, self.n = (gen_engine, ops), 0
        self.orig = [m.check for m in self.modules]

    def __enter__(self):
        def counting(rc, what="", _orig=self.orig[0]):
            self.n += 1
            return _orig(rc, what)

        for m in self.modules:
            m.check = counting
        return self

    def __exit__(self, *exc):
        for m, f in zip(self.modules, self.orig):
            m.check = f


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--budgets", default="1048576,4194304")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import ragged
    from vibravox_amd.inference import enhance_clips
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "enhance_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1 * FS, 12 * FS + 1, size=args.clips)]
    clips = [(0.1 * torch.randn(1, 1, t)).to(dev) for t in lengths]
    cut = [ragged.cut_length(gen, t) for t in lengths]
    audio_s = sum(cut) / FS
    budgets = [int(b) for b in args.budgets.split(",")]

    def loop_of_forwards():
        with torch.no_grad():
            return [gen(gen.cut_to_valid_length(c))[0] for c in clips]

    paths = [("batch1_loop", loop_of_forwards)] + [
        (f"enhance_clips_{b}", lambda b=b: enhance_clips(gen, clips, max_batch_samples=b)) for b in budgets]
    # where the time goes: the same batches packed ahead of time, through forward_ragged (fills, no packing) and through the plain
    # batched forward (the same launches without the fills; its edges are the buffer's, it is here for its time only)
    b = budgets[-1]
    packed = []
    for idx in ragged.compose_batches(gen, lengths, b)[0]:
        p = ragged.plan(gen, [lengths[i] for i in idx])
        buf = torch.zeros((len(idx), 1, p.l_buf), device=dev)
        for r, i in enumerate(idx):
            buf[r, 0, : p.cut[r]] = clips[i][0, 0, : p.cut[r]]
        packed.append((buf, p.lengths))

    def packed_ragged():
        with torch.no_grad():
            return [gen.forward_ragged(buf, lens)[0] for buf, lens in packed]

    def packed_plain():
        with torch.no_grad():
            return [gen(buf)[0] for buf, _ in packed]

    paths += [(f"packed_ragged_{b}", packed_ragged), (f"packed_plain_{b}", packed_plain)]

    for _, fn in paths:   # warm-up: weight images, allocator
        fn()
    torch.cuda.synchronize()
    launches = {}
    for name, fn in paths:
        with LaunchCounter() as c:
            fn()
        launches[name] = c.n
    ref = paths[0][1]()
    worst = {}
    for name, fn in paths[1 : 1 + len(budgets)]:
        worst[name] = max(float((a.reshape(-1) - b.reshape(-1)).abs().max()) for a, b in zip(fn(), ref))
    del ref
    times = {name: [] for name, _ in paths}
    for _ in range(args.iters):
        for name, fn in paths:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))

    lines = []
    for name, _ in paths:
        ms = statistics.median(times[name])
        line = dict(path=name, clips=args.clips, audio_seconds=round(audio_s, 1), median_ms=round(ms, 2), min_ms=round(min(times[name]), 2),
                    max_ms=round(max(times[name]), 2), audio_seconds_per_second=round(audio_s / (ms * 1e-3), 0), library_launches=launches[name])
        if name.startswith("enhance_clips"):
            b = int(name.rsplit("_", 1)[1])
            batches, _ = ragged.compose_batches(gen, lengths, b)
            plans = [ragged.plan(gen, [lengths[i] for i in idx]) for idx in batches]
            pad = [1.0 - sum(p.cut) / (len(p.cut) * p.l_buf) for p in plans]
            line.update(batches=len(batches), rows_per_batch=[len(p.cut) for p in plans], padding_share=[round(x, 3) for x in pad],
                        padding_share_total=round(1.0 - sum(cut) / sum(len(p.cut) * p.l_buf for p in plans), 3),
                        fill_launches=sum(len(p.fills) for p in plans), torch_copies=2 * args.clips + len(batches),
                        max_abs_vs_batch1=worst[name])
        print(json.dumps(line), flush=True)
        lines.append(line)
    base = lines[0]
    summary = [f"enhance_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} clips of 1-12 s at 16 kHz ({audio_s:.0f} s of audio), "
               f"EBENGenerator(4, 32, 2), medians of {args.iters} alternated passes",
               f"  {'batch-1 loop':>24}: {base['median_ms']:9.2f} ms  {base['audio_seconds_per_second']:9.0f} audio-s/s  {base['library_launches']} launches"]
    for l in lines[1 + len(budgets):]:
        summary.append(f"  {l['path']:>24}: {l['median_ms']:9.2f} ms  {l['audio_seconds_per_second']:9.0f} audio-s/s  {l['library_launches']} launches")
    for l in lines[1 : 1 + len(budgets)]:
        summary.append(f"  {l['path']:>24}: {l['median_ms']:9.2f} ms  {l['audio_seconds_per_second']:9.0f} audio-s/s  {l['library_launches']} launches "
                       f"({l['fill_launches']} of them fills) + {l['torch_copies']} torch copies, {l['batches']} batches, padding "
                       f"{100 * l['padding_share_total']:.1f} %, {base['median_ms'] / l['median_ms']:.2f}x the loop, max|diff| {l['max_abs_vs_batch1']:.1e}")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
