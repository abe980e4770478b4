"""What measuring integrated loudness costs on an enhanced split: the one ragged `metrics.loudness_gain` call against the same values
composed from calls the package already had, a device copy of the same bytes, and `inference.enhance_to_pcm` with and without
`loudness=`.

    python tools/loudness_bench.py [--clips 256] [--reps 20] [--rates 16000 48000] [--out profiles/loudness_bench.txt]

Workload per rate: `--clips` clips with lengths uniform in 1 .. 12 s (seed 0) of the speech-like signal of tools/eval_bench.py, in one
zero-padded (clips, longest) float32 batch on the device.

  (a) ragged    one `metrics.loudness_gain(x, fs, lengths)` call: two passes over the input with the 4-state scan, the chunk carry, the
                per-row gates (csrc/loudness.hip).  Nothing of the batch's size is written.
  (b) composed  the same definition from merged calls: two `eben_biquad` passes over the padded batch (`filters._biquad`, shelf then
                high-pass: the weighted signal is written twice, as float32), then torch: squares and hop sums in float64, blocks as
                four consecutive hops, both gates with masks, in chunks of 32 rows.  Its float32 hand-over between the sections makes
                its values differ from (a)'s in the last digits; the largest difference is reported, not held to a bar.
  (c) copy      `x.clone()`: reading and writing the batch's bytes once, the bandwidth floor of anything that touches every sample.
  (d) export    `enhance_to_pcm` through EBENGenerator(4, 32, 2), PCM16, with and without `loudness=-23` (at 48 kHz: clips in at
                48 kHz, files out at 48 kHz), the generator drained; wall clock around the whole call, the device idle before and after.

(a), (b), (c) are timed with HIP events around one whole call; every path runs `--reps` times after two warm-up calls, the paths
alternating within one session; medians with min .. max as the run-to-run spread.  No expectation is fixed in advance."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eval_bench import speech_like  # noqa: E402  (tools/ is the script's directory)


def composed(x, lens, fs, coefficients, chunk=32):
    """Integrated loudness of every row of a zero-padded batch from eben_biquad and torch; (rows,) float32."""
    import torch

    from vibravox_amd import filters

    shelf, highpass = coefficients
    y = filters._biquad(filters._biquad(x, 0, tuple(shelf), False, False), 0, tuple(highpass), False, False)
    rows, t = y.shape
    h = fs // 10
    nh = t // h
    out = torch.full((rows,), float("-inf"), dtype=torch.float32, device=x.device)
    if nh < 4:
        return out
    for r0 in range(0, rows, chunk):
        e = y[r0 : r0 + chunk, : nh * h].double().pow(2).reshape(-1, nh, h).sum(-1)
        z = e.unfold(1, 4, 1).sum(-1) / (4 * h)
        blocks = torch.clamp(lens[r0 : r0 + chunk].long() // h - 3, min=0)
        live = torch.arange(z.shape[1], device=x.device)[None, :] < blocks[:, None]
        l = -0.691 + 10.0 * torch.log10(z)
        keep = live & (l > -70.0)
        zero = torch.zeros_like(z)
        rel = -0.691 + 10.0 * torch.log10(torch.where(keep, z, zero).sum(-1) / keep.sum(-1)) - 10.0
        keep = keep & (l > rel[:, None])
        out[r0 : r0 + chunk] = (-0.691 + 10.0 * torch.log10(torch.where(keep, z, zero).sum(-1) / keep.sum(-1))).float()
    return torch.where(torch.isnan(out), torch.full_like(out, float("-inf")), out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 48000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import metrics as M
    from vibravox_amd.inference import enhance_to_pcm
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "loudness_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    lines, summary = [], []
    for fs in args.rates:
        rng = np.random.RandomState(0)
        seconds = rng.uniform(1.0, 12.0, size=args.clips)
        lengths = [int(s * fs) for s in seconds]
        t_max = max(lengths)
        host = torch.zeros((args.clips, t_max))
        for r, t in enumerate(lengths):
            host[r, :t] = torch.from_numpy(speech_like(r, t, fs).astype(np.float32))
        x = host.to(dev)
        clips = [x[r, :t].clone() for r, t in enumerate(lengths)]
        lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
        coefficients = M.k_weighting_coefficients(fs)
        rated = dict(input_rate=fs, output_rate=fs) if fs != 16000 else {}

        def export(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in enhance_to_pcm(gen, clips, format="PCM16", **rated, **kw):
                pass
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        paths = [("ragged", lambda: M.loudness_gain(x, fs, lens)[0]), ("composed", lambda: composed(x, lens, fs, coefficients)),
                 ("copy", lambda: x.clone())]
        results = {}
        for name, fn in paths:   # warm-up (code objects, allocator)
            fn()
            results[name] = fn()
        export()
        export(loudness=-23.0)
        torch.cuda.synchronize()
        a, b = results["ragged"].double(), results["composed"].double()
        both = torch.isfinite(a) & torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)) and both.any(), "(a) and (b) disagree on which clips have a loudness"
        worst = float((a - b)[both].abs().max())
        times = {name: [] for name in ("ragged", "composed", "copy", "export_plain", "export_loudness")}
        for _ in range(args.reps):
            for name, fn in paths:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
            times["export_plain"].append(export())
            times["export_loudness"].append(export(loudness=-23.0))
        audio = sum(lengths) / fs
        by = {}
        for name, v in times.items():
            by[name] = dict(path=name, fs=fs, clips=args.clips, audio_seconds=round(audio, 1), reps=args.reps, median_ms=round(statistics.median(v), 3),
                            min_ms=round(min(v), 3), max_ms=round(max(v), 3))
            lines.append(by[name])
            print(json.dumps(by[name]), flush=True)
        ra, co, cp, ep, el = (by[k] for k in ("ragged", "composed", "copy", "export_plain", "export_loudness"))
        faster = "faster than" if ra["median_ms"] < co["median_ms"] else "NOT faster than"
        summary += [
            f"loudness_bench on {torch.cuda.get_device_properties(0).name} at {fs} Hz: {args.clips} clips of 1-12 s ({audio:.0f} s of audio, longest {t_max} "
            f"samples, {x.numel() * 4 / 2 ** 20:.0f} MiB padded), medians of {args.reps} alternated calls (min .. max)"]
        summary += [f"  {l['path']:>16}: {l['median_ms']:9.3f} ms  ({l['min_ms']:.3f} .. {l['max_ms']:.3f})" for l in (ra, co, cp, ep, el)]
        summary += [
            f"  (a) / (b) = {ra['median_ms'] / co['median_ms']:.3f}: the ragged call is {faster} the composition of merged calls; their values differ by at "
            f"most {worst:.2e} LU (the composition hands float32 from one section to the next)",
            f"  (a) / (c) = {ra['median_ms'] / cp['median_ms']:.1f}: {ra['median_ms']:.3f} ms against {cp['median_ms']:.3f} ms for a device copy of the batch "
            f"(two reads of the input and float64 recurrences against one read and one write)",
            f"  (d) loudness=-23 adds {el['median_ms'] - ep['median_ms']:.3f} ms to enhance_to_pcm's {ep['median_ms']:.3f} ms "
            f"({100.0 * (el['median_ms'] - ep['median_ms']) / ep['median_ms']:.1f} %; the plain call's own spread {ep['max_ms'] - ep['min_ms']:.3f} ms)"]
        del x, clips, host
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
