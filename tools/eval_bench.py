"""Scoring a test split of utterances of different lengths: the loop of batch-1 forwards and dense metric calls against
`inference.evaluate_clips` (ragged forwards, SI-SDR / STOI kernels with a length per row).

    python tools/eval_bench.py [--clips 256] [--iters 5] [--budgets 1048576,4194304] [--out FILE]

Workload: `--clips` (corrupted, reference) pairs with lengths uniform in 1 .. 12 s at 16 kHz (seed 0, the corpus of tools/enhance_bench.py)
through the default generator EBENGenerator(4, 32, 2).  The references are noise under syllable envelopes with silent stretches (the
construction of the metric tests' `speech_like`, restated below), so STOI's silence removal keeps a different share of every clip; the
corrupted clips are the references plus white noise at 5 dB.
  (a) per clip `gen(cut_to_valid_length(c))`, then dense `si_sdr` and `stoi` on that one row -- the reference's batch-1 test loop;
  (b) `inference.evaluate_clips`, once per `max_batch_samples` budget;
  (c) `inference.enhance_clips` alone at the same budgets: what of (b) is not the metrics;
  (d) the metrics alone on the same enhanced signals: dense calls clip by clip, and the ragged calls on the packed buffers of the last
      budget -- whether a length per row costs the kernels anything.
Each pass is timed with HIP events around the whole corpus; the paths alternate within one session, one warm-up pass each, medians of
`--iters` passes with every sample printed.  Launches are counted as calls into libeben_hip.so (each is one kernel launch, a STOI call four).  Prints one
JSON line per path, max |(b) - (a)| per metric and whether (b) beats (a) by more than the spread of (a)'s own samples."""
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


def speech_like(r: int, t: int, fs: int = FS) -> np.ndarray:
    """Clip `r`: two tones and hashed noise under a syllable envelope, gated into stretches of speech and silence."""
    n = np.arange(t, dtype=np.float64)
    k = r % 16
    h = (np.sin(n * 12.9898 + (r + 1) * 78.233) * 43758.5453) % 1.0 - 0.5
    car = np.sin(2 * np.pi * (180 + 23 * k) * n / fs) + 0.6 * np.sin(2 * np.pi * (730 + 41 * k) * n / fs) + 0.8 * h
    syl = 0.5 + 0.5 * np.sin(2 * np.pi * (2.1 + 0.37 * k) * n / fs + r)
    gate = (np.sin(2 * np.pi * (0.45 + 0.11 * k) * n / fs + 0.7 * r) > -0.2 + 0.02 * (r % 7)).astype(np.float64)
    return 0.3 * car * syl ** 2 * gate + 1e-5 * h


class LaunchCounter:
    """Counts the library calls made through `check` in the modules on the evaluation path."""

    def __init__(self):
        from vibravox_amd import augment, gen_engine, metrics, ops

        self.modules, self.n = (gen_engine, ops, metrics, augment), 0
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
    from vibravox_amd.inference import enhance_clips, evaluate_clips
    from vibravox_amd.metrics import si_sdr, stoi
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "eval_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1 * FS, 12 * FS + 1, size=args.clips)]
    reference, corrupted = [], []
    for r, t in enumerate(lengths):
        x = speech_like(r, t)
        noise = rng.randn(t)
        noise *= np.sqrt((x ** 2).mean() / (noise ** 2).mean()) * 10 ** (-5.0 / 20)
        reference.append(torch.from_numpy(x.astype(np.float32)).reshape(1, 1, t).to(dev))
        corrupted.append(torch.from_numpy((x + noise).astype(np.float32)).reshape(1, 1, t).to(dev))
    cut = [ragged.cut_length(gen, t) for t in lengths]
    audio_s = sum(cut) / FS
    budgets = [int(b) for b in args.budgets.split(",")]

    def batch1_loop():
        sdr, sti = [], []
        with torch.no_grad():
            for c, g in zip(corrupted, reference):
                e = gen(gen.cut_to_valid_length(c))[0]
                g = gen.cut_to_valid_length(g)
                sdr.append(si_sdr(e, g).reshape(1))
                sti.append(stoi(e, g, FS).reshape(1))
        return {"si_sdr": torch.cat(sdr), "stoi": torch.cat(sti)}

    paths = [("batch1_loop", batch1_loop)]
    paths += [(f"evaluate_clips_{b}", lambda b=b: evaluate_clips(gen, corrupted, reference, max_batch_samples=b)) for b in budgets]
    paths += [(f"enhance_clips_{b}", lambda b=b: enhance_clips(gen, corrupted, max_batch_samples=b)) for b in budgets]

    # (d) the metrics alone, on the enhanced clips of the last budget: clip by clip, and on the packed buffers with a length per row
    b = budgets[-1]
    enhanced = enhance_clips(gen, corrupted, max_batch_samples=b)
    cut_refs = [g[..., :n].contiguous() for g, n in zip(reference, cut)]
    packed = []
    for idx in ragged.compose_batches(gen, lengths, b)[0]:
        p = ragged.plan(gen, [lengths[i] for i in idx])
        e_buf, g_buf = torch.zeros((len(idx), p.l_buf), device=dev), torch.zeros((len(idx), p.l_buf), device=dev)
        for r, i in enumerate(idx):
            e_buf[r, : p.cut[r]] = enhanced[i].reshape(-1)
            g_buf[r, : p.cut[r]] = cut_refs[i].reshape(-1)
        packed.append((e_buf, g_buf, torch.tensor(p.cut, dtype=torch.int32, device=dev)))

    def metrics_dense_loop():
        return [(si_sdr(e, g), stoi(e, g, FS)) for e, g in zip(enhanced, cut_refs)]

    def metrics_ragged():
        return [(si_sdr(e, g, lens), stoi(e, g, FS, lens)) for e, g, lens in packed]

    paths += [("metrics_dense_loop", metrics_dense_loop), (f"metrics_ragged_{b}", metrics_ragged)]

    for _, fn in paths:   # warm-up: weight images, resampling table, allocator
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
        got = fn()
        worst[name] = {k: float((got[k] - ref[k]).abs().max()) for k in ("si_sdr", "stoi")}
    stoi_scored = int((ref["stoi"] != 1e-5).sum())
    stoi_range = (float(ref["stoi"].min()), float(ref["stoi"].max()))
    sdr_range = (float(ref["si_sdr"].min()), float(ref["si_sdr"].max()))
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
        line = dict(path=name, clips=args.clips, audio_seconds=round(audio_s, 1), median_ms=round(ms, 2), samples_ms=[round(x, 2) for x in times[name]],
                    audio_seconds_per_second=round(audio_s / (ms * 1e-3), 0), library_launches=launches[name])
        if name.startswith("evaluate_clips"):
            line.update(batches=len(ragged.compose_batches(gen, lengths, int(name.rsplit("_", 1)[1]))[0]), max_abs_vs_batch1=worst[name])
        print(json.dumps(line), flush=True)
        lines.append(line)
    by = {l["path"]: l for l in lines}
    base = by["batch1_loop"]
    spread = max(base["samples_ms"]) - min(base["samples_ms"])
    summary = [f"eval_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} pairs of 1-12 s at 16 kHz ({audio_s:.0f} s of audio), "
               f"EBENGenerator(4, 32, 2), medians of {args.iters} alternated passes; STOI scores {stoi_scored} of {args.clips} clips "
               f"(the others keep fewer than 30 frames) in [{stoi_range[0]:.3f}, {stoi_range[1]:.3f}], SI-SDR in [{sdr_range[0]:.1f}, {sdr_range[1]:.1f}] dB"]
    for l in lines:
        extra = ""
        if l["path"].startswith("evaluate_clips"):
            extra = (f", {l['batches']} batches, {base['median_ms'] / l['median_ms']:.2f}x the loop, max|diff| si_sdr "
                     f"{l['max_abs_vs_batch1']['si_sdr']:.1e} dB stoi {l['max_abs_vs_batch1']['stoi']:.1e}")
        summary.append(f"  {l['path']:>24}: {l['median_ms']:9.2f} ms  samples {l['samples_ms']}  {l['library_launches']} launches{extra}")
    ok = True
    for bb in budgets:
        e, c = by[f"evaluate_clips_{bb}"], by[f"enhance_clips_{bb}"]
        gain = base["median_ms"] - e["median_ms"]
        ok = ok and gain > spread
        summary.append(f"  budget {bb}: the metrics' share of evaluate_clips is {e['median_ms'] - c['median_ms']:.2f} ms of {e['median_ms']:.2f}; "
                       f"evaluate_clips is {gain:.2f} ms faster than the loop (spread of the loop's own samples {spread:.2f} ms)")
    d, g = by["metrics_dense_loop"], by[f"metrics_ragged_{b}"]
    summary.append(f"  metrics alone: dense clip by clip {d['median_ms']:.2f} ms ({d['library_launches']} launches), ragged on the packed buffers "
                   f"{g['median_ms']:.2f} ms ({g['library_launches']} launches): the ragged calls are "
                   f"{'SLOWER than' if g['median_ms'] > d['median_ms'] else 'faster than'} the sum of the dense ones on the same rows")
    summary.append(f"  speed bar (evaluate_clips faster than the loop by more than the loop's own spread, at every budget): {'met' if ok else 'NOT MET'}")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
