"""The complete test log of a split of utterances of different lengths -- SI-SDR, STOI and the five atomic losses per utterance: the
loop of batch-1 `test_step` + `on_test_batch_end` against `EBENLightningModule.evaluate_clips(losses=True)` (ragged generator and
discriminators, per-row feature-matching / hinge / MRSTFT sums), and against `evaluate_clips` without the losses.

    python tools/eval_losses_bench.py [--clips 256] [--iters 5] [--budget 4194304] [--out profiles/eval_losses_bench.txt]

Workload: the corpus of tools/eval_bench.py (`--clips` pairs with lengths uniform in 1 .. 12 s at 16 kHz, seed 0) through
EBENGenerator(4, 32, 2), DiscriminatorEBENMultiScales(3, 24) and the multi_stft.yaml MRSTFT with A-weighting, random initial weights.
Each pass is timed with HIP events around the whole corpus; the three paths alternate within one session, one warm-up pass each,
medians of `--iters` passes with every sample printed.  Prints one JSON line per path and the largest relative difference of every
loss between the ragged pass and the loop.  No ratio is promised: the numbers are what the device gives."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FS = 16000
LOSSES = ("generator/reconstructive_loss_freq", "generator/feature_matching_loss", "generator/adv_loss_gen", "discriminator/real_loss",
          "discriminator/fake_loss")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--budget", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from eval_bench import speech_like
    from vibravox_amd import ragged
    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    assert torch.cuda.is_available(), "eval_losses_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    opt = partial(FusedAdam, lr=3e-4)
    mod = EBENLightningModule(
        sample_rate=FS, generator=EBENGenerator(m=4, n=32, p=2).to(dev).eval(), discriminator=DiscriminatorEBENMultiScales(q=3, min_channels=24).to(dev).eval(),
        generator_optimizer=opt, discriminator_optimizer=opt,
        reconstructive_loss_freq_fn=MultiResolutionSTFTLoss(sample_rate=FS, perceptual_weighting=True).to(dev),
        feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales(), adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales())
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1 * FS, 12 * FS + 1, size=args.clips)]
    reference, corrupted = [], []
    for r, t in enumerate(lengths):
        x = speech_like(r, t)
        noise = rng.randn(t)
        noise *= np.sqrt((x ** 2).mean() / (noise ** 2).mean()) * 10 ** (-5.0 / 20)
        reference.append(torch.from_numpy(x.astype(np.float32)).reshape(1, 1, t).to(dev))
        corrupted.append(torch.from_numpy((x + noise).astype(np.float32)).reshape(1, 1, t).to(dev))
    audio_s = sum(ragged.cut_length(mod.generator, t) for t in lengths) / FS
    margin = ragged.loss_margin(mod.discriminator, 4, mod.reconstructive_loss_freq_fn)

    def batch1_loop():
        """The reference's test loop: per utterance the logged values, kept on the device."""
        rows = {k: [] for k in LOSSES}
        for i, (c, g) in enumerate(zip(corrupted, reference)):
            batch = {"audio_body_conducted": c, "audio_airborne": g}
            mod.on_test_batch_end(mod.test_step(batch, i), batch, i)
            for k in LOSSES:
                rows[k].append(mod.logged[f"test/{k}"].reshape(1))
        return {k: torch.cat(v) for k, v in rows.items()}

    paths = [("batch1_test_loop", batch1_loop),
             ("evaluate_clips_losses", lambda: mod.evaluate_clips(corrupted, reference, max_batch_samples=args.budget, losses=True)),
             ("evaluate_clips_metrics_only", lambda: mod.evaluate_clips(corrupted, reference, max_batch_samples=args.budget))]
    for _, fn in paths:   # warm-up: weight images, DFT bases, resampling table, allocator
        fn()
    torch.cuda.synchronize()
    loop, got = paths[0][1](), paths[1][1]()
    worst = {k: float(((got[k] - loop[k]).abs() / loop[k].abs()).max()) for k in LOSSES}
    del loop, got
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
                    audio_seconds_per_second=round(audio_s / (ms * 1e-3), 0))
        if name == "evaluate_clips_losses":
            line.update(batches=len(ragged.compose_batches(mod.generator, lengths, args.budget, margin)[0]), margin=margin, max_rel_vs_loop=worst)
        print(json.dumps(line), flush=True)
        lines.append(line)
    by = {l["path"]: l for l in lines}
    base, full, bare = by["batch1_test_loop"], by["evaluate_clips_losses"], by["evaluate_clips_metrics_only"]
    spread = max(base["samples_ms"]) - min(base["samples_ms"])
    gain = base["median_ms"] - full["median_ms"]
    summary = [f"eval_losses_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} pairs of 1-12 s at 16 kHz ({audio_s:.0f} s of audio), "
               f"EBENGenerator(4, 32, 2), DiscriminatorEBENMultiScales(3, 24), MRSTFT of multi_stft.yaml, budget {args.budget} buffer samples, "
               f"medians of {args.iters} alternated passes"]
    for l in lines:
        summary.append(f"  {l['path']:>28}: {l['median_ms']:9.2f} ms  samples {l['samples_ms']}")
    summary.append(f"  evaluate_clips(losses=True): {full['batches']} batches at a margin of {margin} samples, {base['median_ms'] / full['median_ms']:.2f}x the "
                   f"batch-1 test loop ({gain:.2f} ms {'faster' if gain > 0 else 'SLOWER'}; spread of the loop's own samples {spread:.2f} ms), "
                   f"{full['median_ms'] / bare['median_ms']:.2f}x the cost of evaluate_clips without the losses")
    summary.append("  largest relative difference to the loop's value, per loss: " + ", ".join(f"{k.split('/')[1]} {v:.1e}" for k, v in worst.items()))
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
