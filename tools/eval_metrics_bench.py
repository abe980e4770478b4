"""What the evaluation metrics cost on a test split: `inference.evaluate_clips` with its default two metrics (SI-SDR, STOI) against the
same call with all seven (ESTOI, SI-SNR, SNR, LSD and high-band LSD on top), and each metric call alone on the packed buffers.

    python tools/eval_metrics_bench.py [--clips 256] [--reps 20] [--budget 4194304] [--cutoff 4000] [--default-only] [--out FILE]

Workload: the corpus of tools/eval_bench.py -- `--clips` (corrupted, reference) pairs with lengths uniform in 1 .. 12 s at 16 kHz (seed 0)
through EBENGenerator(4, 32, 2).  Every path is timed with HIP events around one whole pass, `--reps` passes after two warm-up passes,
the paths alternating within one session; medians with min .. max as the run-to-run spread.  Launches are counted as calls into
libeben_hip.so from `vibravox_amd.metrics` (a STOI call is four kernel launches, ESTOI five, STOI + ESTOI six, LSD two).

`--default-only` times nothing but the default call and touches none of the new entry points: the same script on the commit before them
gives the yardstick the default call has to stay within."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eval_bench import FS, speech_like  # noqa: E402  (tools/ is the script's directory)

ALL = ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=int, default=1 << 22)
    ap.add_argument("--cutoff", type=float, default=4000.0)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import metrics as M
    from vibravox_amd import ragged
    from vibravox_amd.inference import enhance_clips, evaluate_clips
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "eval_metrics_bench times the device path: it needs an MI355X"
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
    audio_s = sum(ragged.cut_length(gen, t) for t in lengths) / FS

    paths = [("evaluate_clips_default", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget))]
    if not args.default_only:
        paths.append(("evaluate_clips_all_seven", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget, metrics=ALL,
                                                                         lsd_hf_cutoff_hz=args.cutoff)))
        # every metric call alone, on the packed enhanced / reference buffers evaluate_clips hands them
        enhanced = enhance_clips(gen, corrupted, max_batch_samples=args.budget)
        packed = []
        for idx in ragged.compose_batches(gen, lengths, args.budget)[0]:
            p = ragged.plan(gen, [lengths[i] for i in idx])
            e_buf, g_buf = torch.zeros((len(idx), p.l_buf), device=dev), torch.zeros((len(idx), p.l_buf), device=dev)
            for r, i in enumerate(idx):
                e_buf[r, : p.cut[r]] = enhanced[i].reshape(-1)
                g_buf[r, : p.cut[r]] = reference[i].reshape(-1)[: p.cut[r]]
            packed.append((e_buf, g_buf, torch.tensor(p.cut, dtype=torch.int32, device=dev)))
        hf = (args.cutoff, FS // 2)
        alone = dict(si_sdr=lambda e, g, n: M.si_sdr(e, g, n), stoi=lambda e, g, n: M.stoi(e, g, FS, n),
                     estoi=lambda e, g, n: M.stoi(e, g, FS, n, extended=True), stoi_and_estoi=lambda e, g, n: M.stoi_and_estoi(e, g, FS, n),
                     si_snr=lambda e, g, n: M.si_snr(e, g, n), snr=lambda e, g, n: M.snr(e, g, n), lsd=lambda e, g, n: M.lsd(e, g, FS, n),
                     lsd_hf=lambda e, g, n: M.lsd(e, g, FS, n, band_hz=hf), lsd_both=lambda e, g, n: M.lsd(e, g, FS, n, band_hz=[None, hf]))
        paths += [(f"alone_{k}", lambda f=f: [f(e, g, n) for e, g, n in packed]) for k, f in alone.items()]

    launches = {}
    for name, fn in paths:   # warm-up (weight images, resampling table, allocator), then the library calls of one pass
        fn()
        fn()
        seen, real = [], M.check
        M.check = lambda rc, what="", _s=seen, _r=real: (_s.append(what), _r(rc, what))[1]
        try:
            fn()
        finally:
            M.check = real
        launches[name] = len(seen)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for _ in range(args.reps):
        for name, fn in paths:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))

    lines = []
    for name, _ in paths:
        s = times[name]
        lines.append(dict(path=name, clips=args.clips, audio_seconds=round(audio_s, 1), reps=args.reps, median_ms=round(statistics.median(s), 3),
                          min_ms=round(min(s), 3), max_ms=round(max(s), 3), metric_library_calls=launches[name]))
        print(json.dumps(lines[-1]), flush=True)
    by = {l["path"]: l for l in lines}
    summary = [f"eval_metrics_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} pairs of 1-12 s at 16 kHz ({audio_s:.0f} s of audio), "
               f"EBENGenerator(4, 32, 2), max_batch_samples {args.budget}, medians of {args.reps} alternated passes (min .. max)"]
    for l in lines:
        summary.append(f"  {l['path']:>26}: {l['median_ms']:9.3f} ms  ({l['min_ms']:.3f} .. {l['max_ms']:.3f})  {l['metric_library_calls']} metric calls")
    if not args.default_only:
        d, a = by["evaluate_clips_default"], by["evaluate_clips_all_seven"]
        added = {k: by[f"alone_{k}"]["median_ms"] for k in ("stoi_and_estoi", "si_snr", "snr", "lsd_both")}
        added["stoi_and_estoi"] -= by["alone_stoi"]["median_ms"]     # what the second tail adds to the STOI the default call runs anyway
        top = max(added, key=added.get)
        summary.append(f"  all seven metrics add {a['median_ms'] - d['median_ms']:.3f} ms to the default call's {d['median_ms']:.3f} ms "
                       f"(its own spread {d['max_ms'] - d['min_ms']:.3f} ms); of the calls they add, alone: " +
                       ", ".join(f"{k} {v:.3f} ms" for k, v in added.items()) + f" -- {top} dominates")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
