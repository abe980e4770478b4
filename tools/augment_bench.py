"""Waveform augmentation: what the batch-level transforms cost, what the per-clip mode costs, and what each does to the step's length.

    python tools/augment_bench.py [--batch 32] [--samples 40000] [--iters 9] [--kernel-iters 50] [--fit-steps 50] [--skip-fit] [--out FILE]

At the benchmark's batch (32 x 40 000 samples at 16 kHz, two waveforms), HIP events around each call, one warm-up call first, the
compared paths alternating within a round, medians with min / max of `--iters` rounds:
(a) the batch-level `speed`, `pitch_shift` and `time_masking_` of vibravox_amd/augment.py, each alone on both waveforms; for
    `pitch_shift` every one of the ten default steps: the first call (which builds the step's dense table in float64 on the host and
    uploads it) and the steady state, then the bytes of device memory the dense tables hold once all ten have occurred;
(b) `WaveformDataAugmentation(per_clip=True)`: every clip drawing speed, pitch and mask; the probabilities and lists of `light.yaml`;
    and one stage at a time (host planning and descriptor tables included: this is the call the collator makes);
(c) one `augment.resample_clips` call (the cached bands looked up, the descriptor tables built with ctypes, two launches for the 64
    rows): bytes read (the rows' samples) plus written per second for the speed ratios and for the pitch ratios, next to a device
    copy of the same byte count.  The events enclose the host work, so the figure is a lower bound on the kernel's own rate;
(d) a `--fit-steps`-step `Trainer.fit` on the synthetic datamodule with `per_clip.yaml` against the batch mode with the same
    probabilities: the distinct batch lengths T the train step was given.
Prints one JSON line per measurement and a summary; `--out` writes both to a file."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE = 16000
STEP_MS = 8.5   # the train step the augmentation has to keep up with (README)


def timed(torch, fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def config_kwargs(name: str) -> dict:
    """The constructor arguments of configs/lightning_datamodule/data_augmentation/<name>.yaml (Hydra's tuples resolved by hand)."""
    import yaml

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "lightning_datamodule", "data_augmentation", name + ".yaml")))
    return {k: (tuple(v["_args_"][0]) if isinstance(v, dict) else v) for k, v in cfg.items() if k not in ("_target_", "sample_rate")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=40000)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--fit-steps", type=int, default=50)
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import augment, collate

    assert torch.cuda.is_available(), "augment_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    B, T = args.batch, args.samples
    g = torch.Generator().manual_seed(0)
    w1, w2 = (0.1 * torch.randn(B, 1, T, generator=g)).to(dev), (0.1 * torch.randn(B, 1, T, generator=g)).to(dev)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def rounds(paths, iters):
        """{name: [ms]} of `iters` rounds with the paths alternating inside a round, after one warm-up call each."""
        for _, fn in paths:
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in paths}
        for _ in range(iters):
            for name, fn in paths:
                ts[name].append(timed(torch, fn))
        return ts

    # ---- (a) the batch-level transforms ------------------------------------------------------------------------------------------------
    default = augment.WaveformDataAugmentation(RATE)
    mask_buf = torch.cat((w1, w2)).clone()
    paths = [(f"speed_{f}", (lambda f=f: (augment.speed(w1, RATE, f), augment.speed(w2, RATE, f)))) for f in (0.7, 0.95, 1.3)]
    paths.append(("time_masking_8pct", lambda: augment.time_masking_(mask_buf, 8)))
    for name, ts in rounds(paths, args.iters).items():
        emit(part="a", path=name, waveforms=2, **stats(ts))
    first, tables = {}, {}
    for s in default.pitch_shift_steps:   # the first call of each step: its dense table built on the host and uploaded
        t0 = time.perf_counter()
        augment.pitch_shift(w1, RATE, s)
        torch.cuda.synchronize()
        first[s] = (time.perf_counter() - t0) * 1e3
        tables[s] = next(v[0] for k, v in augment._kernel_cache.items() if k[:2] == (int(RATE / 2.0 ** (-s / 12)), RATE)).numel()
    paths = [(s, (lambda s=s: (augment.pitch_shift(w1, RATE, s), augment.pitch_shift(w2, RATE, s)))) for s in default.pitch_shift_steps]
    for s, ts in rounds(paths, args.iters).items():   # the steady state, the ten steps alternating, all ten tables resident
        emit(part="a", path=f"pitch_shift_{s}", waveforms=2, first_call_one_waveform_ms=round(first[s], 1), table_floats=tables[s], **stats(ts))
    dense = sum(v[0].numel() * 4 for k, v in augment._kernel_cache.items() if k[0] != k[1] and v[0].shape[1] > 100)
    emit(part="a", path="pitch_shift_dense_tables", device_bytes=dense)
    augment._kernel_cache.clear()   # give the dense tables back before the rest
    torch.cuda.empty_cache()

    # ---- (b) the per-clip module -------------------------------------------------------------------------------------------------------
    light = config_kwargs("light")
    variants = {
        "every_clip_speed_pitch_mask": dict(p_data_augmentation=1, p_speed_perturbation=1, p_pitch_shift=1, p_time_masking=1),
        "light_probabilities": light,
        "speed_only": dict(p_data_augmentation=1, p_speed_perturbation=1, p_pitch_shift=0, p_time_masking=0),
        "pitch_only": dict(p_data_augmentation=1, p_speed_perturbation=0, p_pitch_shift=1, p_time_masking=0),
        "mask_only": dict(p_data_augmentation=1, p_speed_perturbation=0, p_pitch_shift=0, p_time_masking=1),
    }
    mods = {k: augment.WaveformDataAugmentation(RATE, per_clip=True, **kw) for k, kw in variants.items()}
    torch.manual_seed(0)
    touched = {k: [] for k in mods}

    def run(k):
        out = mods[k](w1, w2)
        touched[k].append(len(mods[k].last_plan))
        return out

    for name, ts in rounds([(k, (lambda k=k: run(k))) for k in mods], args.iters).items():
        emit(part="b", path="per_clip_" + name, waveforms=2, clips_touched_mean=round(statistics.mean(touched[name]), 1), **stats(ts))
    per_clip_light = next(l["median_ms"] for l in lines if l.get("path") == "per_clip_light_probabilities")

    # ---- (c) one resample_clips call ----------------------------------------------------------------------------------------------------
    rows_n = 2 * B
    flat = torch.cat((w1, w2)).reshape(-1)
    out = torch.empty((rows_n, T), device=dev)
    layouts = {"speed_ratios": [int(default.speed_perturbation_factors[i % 10] * RATE) for i in range(rows_n)],
               "pitch_ratios": [int(RATE / 2.0 ** (-default.pitch_shift_steps[i % 10] / 12)) for i in range(rows_n)]}
    for layout, origs in layouts.items():
        # a row reads what its T outputs reach: min(T, ceil(T * orig / new)) of its samples
        rows = [(i * T, T, o, RATE, i) for i, o in enumerate(origs)]
        nbytes = 4 * (sum(min(T, -(-T * o // RATE)) for o in origs) + out.numel())
        src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)
        ts = rounds([("resample_clips_call", lambda: augment.resample_clips(flat, rows, out)), ("torch_device_copy_same_bytes", lambda: dst.copy_(src))], args.kernel_iters)
        for name, t in ts.items():
            emit(part="c", layout=layout, path=name, rows=rows_n, bytes_read_plus_written=nbytes, gigabytes_per_second=round(nbytes / (statistics.median(t) * 1e-3) / 1e9, 1),
                 **stats(t))

    # ---- (d) the lengths a fit's step sees ---------------------------------------------------------------------------------------------
    if not args.skip_fit:
        sys.path.insert(0, ROOT)
        from bench import build_module
        from vibravox_amd.fit import Trainer
        from vibravox_amd.synthetic import SyntheticBWEDataModule

        class Augmented:
            """The synthetic batches through the collator's augmentation hook."""

            def __init__(self, aug):
                self.inner, self.aug, self.lengths = SyntheticBWEDataModule(RATE, B, T * 1000 // RATE, device="cuda"), aug, []

            def train_dataloader(self):
                for batch in self.inner.train_dataloader():
                    bc, ab = collate._augment(self.aug, False, batch["audio_body_conducted"], batch["audio_airborne"])
                    self.lengths.append(int(bc.shape[-1]))
                    yield {"audio_body_conducted": bc, "audio_airborne": ab}

        kw = config_kwargs("per_clip")
        for mode in ("per_clip", "batch"):
            dm = Augmented(augment.WaveformDataAugmentation(RATE, **dict(kw, per_clip=mode == "per_clip")))
            torch.manual_seed(0)
            mod = build_module(dev, 1234)
            error = None
            t0 = time.perf_counter()
            try:
                Trainer(max_steps=args.fit_steps, limit_train_batches=args.fit_steps, log_every_n_steps=args.fit_steps).fit(mod, dm)
                torch.cuda.synchronize()
            except Exception as e:   # a length the step refuses is a result here, not a crash of the bench
                error = f"{type(e).__name__}: {e}"[:300]
            emit(part="d", mode=mode, steps_served=len(dm.lengths), distinct_T=len(set(dm.lengths)), lengths=sorted(set(dm.lengths)),
                 wall_seconds=round(time.perf_counter() - t0, 1), error=error)
            del mod
            torch.cuda.empty_cache()

    summary = [f"augment_bench on {torch.cuda.get_device_properties(0).name}: {B} x {T} samples at {RATE} Hz, two waveforms; medians of {args.iters} alternated rounds ((c): of {args.kernel_iters})"]
    for l in lines:
        if l["part"] == "a" and "median_ms" in l:
            extra = f"; first call {l['first_call_one_waveform_ms']} ms for one waveform, table of {l['table_floats'] / 1e6:.0f} M floats" if "table_floats" in l else ""
            summary.append(f"  (a) batch-level {l['path']:<22}: {l['median_ms']:10.3f} ms (min {l['min_ms']}, max {l['max_ms']}){extra}")
        elif l["part"] == "a":
            summary.append(f"  (a) dense pitch tables held on the device after all ten steps: {l['device_bytes'] / 1e9:.2f} GB")
        elif l["part"] == "b":
            summary.append(f"  (b) {l['path']:<38}: {l['median_ms']:10.3f} ms (min {l['min_ms']}, max {l['max_ms']}); {l['clips_touched_mean']} of {B} clips touched")
        elif l["part"] == "c":
            summary.append(f"  (c) {l['layout']:<13} {l['path']:<29}: {l['median_ms']:8.4f} ms  {l['gigabytes_per_second']:8.1f} GB/s read + written ({l['bytes_read_plus_written']} bytes)")
            if l["path"] == "resample_clips_call":
                summary[-1] += "; host tables and 2 launches included: a lower bound on the kernel's rate"
        elif l["part"] == "d":
            summary.append(f"  (d) fit, {l['mode']:<8}: {l['distinct_T']} distinct T over {l['steps_served']} batches {l['lengths'][:12]} in {l['wall_seconds']} s"
                           + (f"; stopped by {l['error']}" if l["error"] else ""))
    ratio = per_clip_light / STEP_MS
    summary.append(f"  per-clip at light's probabilities costs {per_clip_light:.3f} ms a batch = {ratio:.2f} of the {STEP_MS} ms train step"
                   + (": MORE than a step" if ratio > 1 else ""))
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
