"""What the BSS-eval SDR costs on a test split: the one ragged `metrics.sdr` call against the torch route on the same device and the same
padded batch, and `inference.evaluate_clips` with its default metrics against the same call with "sdr" added.

    python tools/sdr_bench.py [--clips 256] [--reps 20] [--filter-length 512] [--budget 4194304] [--out profiles/sdr_bench.txt]

Workload: the corpus of tools/eval_metrics_bench.py -- `--clips` (corrupted, reference) pairs with lengths uniform in 1 .. 12 s at 16 kHz
(seed 0).  The SDR paths score the corrupted clips against their references in one zero-padded (clips, longest) batch.

  (a) hip         one `metrics.sdr(preds, target, lengths)` call: eben_sdr's three kernels.
      hip_solve   the same call with every length 1: a moments kernel and a correlation grid with next to nothing to do, and the whole
                  Levinson solve (which has no data-dependent branch) -- the solve's share of (a); (a) minus it is what the moments
                  and correlation kernels take on the real rows.  (The three kernel times proper come from a kernel trace in a run of
                  its own: `rocprofv3 --kernel-trace -- python tools/sdr_bench.py --only-hip`.)
  (b) torch       float64 on the same padded batch: zero-padded `rfft` correlations as torchmetrics forms them, the dense Toeplitz
                  matrices and `torch.linalg.solve`.  The reference for the time; its values are checked against (a) row by row within the bar of
                  tests/test_gpu_sdr.py taken twice (both sides are float32 roundings): 2 float32 ulp + 1e-7 dB.
  (c) evaluate_clips through EBENGenerator(4, 32, 2) with the default metrics, and with "sdr" added.

Every path is timed with HIP events around one whole call, `--reps` calls after two warm-up calls, the paths alternating within one
session; medians with min .. max as the run-to-run spread.  Workspace: eben_sdr_workspace for (a), the peak of torch's allocator over one
call for (b)."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eval_bench import FS, speech_like  # noqa: E402  (tools/ is the script's directory)

FP64_FMA_PER_S = 256 * 4 * 16 * 2.4e9     # 256 CUs x 4 SIMDs x 16 fp64 FMA lanes per clock x 2.4 GHz: the vector-fp64 peak


def torch_sdr(preds, target, filter_length):
    """torchmetrics' direct-solve route on a zero-padded batch, float64: zero padding behind a row changes nothing."""
    import torch

    p, t = preds.double(), target.double()
    t = t / torch.clamp(torch.linalg.norm(t, dim=-1, keepdim=True), min=1e-6)
    p = p / torch.clamp(torch.linalg.norm(p, dim=-1, keepdim=True), min=1e-6)
    n_fft = 2 ** math.ceil(math.log2(p.shape[-1] + t.shape[-1] - 1))
    tf = torch.fft.rfft(t, n=n_fft, dim=-1)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n_fft)[..., :filter_length]
    b = torch.fft.irfft(tf.conj() * torch.fft.rfft(p, n=n_fft, dim=-1), n=n_fft)[..., :filter_length]
    k = torch.arange(filter_length, device=r.device)
    mat = r[..., (k[:, None] - k[None, :]).abs()]
    h = torch.linalg.solve(mat, b)
    coh = (b * h).sum(-1)
    return (10.0 * torch.log10(coh / (1.0 - coh))).float()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--budget", type=int, default=1 << 22)
    ap.add_argument("--only-hip", action="store_true", help="three calls of (a) and nothing else: the program of a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import metrics as M
    from vibravox_amd._lib import load
    from vibravox_amd.inference import DEFAULT_EVAL_METRICS, evaluate_clips
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "sdr_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
    L = args.filter_length
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1 * FS, 12 * FS + 1, size=args.clips)]
    t_max = max(lengths)
    reference, corrupted = [], []
    target, preds = torch.zeros((args.clips, t_max)), torch.zeros((args.clips, t_max))
    for r, t in enumerate(lengths):
        x = speech_like(r, t)
        noise = rng.randn(t)
        noise *= np.sqrt((x ** 2).mean() / (noise ** 2).mean()) * 10 ** (-5.0 / 20)
        target[r, :t] = torch.from_numpy(x.astype(np.float32))
        preds[r, :t] = torch.from_numpy((x + noise).astype(np.float32))
        reference.append(target[r, :t].reshape(1, 1, t).to(dev))
        corrupted.append(preds[r, :t].reshape(1, 1, t).to(dev))
    target, preds = target.to(dev), preds.to(dev)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ones = torch.ones_like(lens)
    fmas = 2 * sum(L * t - L * (L - 1) // 2 if t >= L else t * (t + 1) // 2 for t in lengths)   # both correlations, lags 0 .. L - 1
    floor_ms = 1e3 * fmas / FP64_FMA_PER_S

    if args.only_hip:
        for _ in range(3):
            M.sdr(preds, target, lens, filter_length=L)
        torch.cuda.synchronize()
        return

    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    with_sdr = tuple(DEFAULT_EVAL_METRICS) + ("sdr",)
    paths = [("hip", lambda: M.sdr(preds, target, lens, filter_length=L)),
             ("hip_solve", lambda: M.sdr(preds, target, ones, filter_length=L)),
             ("torch", lambda: torch_sdr(preds, target, L)),
             ("evaluate_clips_default", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget)),
             ("evaluate_clips_with_sdr", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget, metrics=with_sdr,
                                                                sdr_filter_length=L))]
    results = {}
    for name, fn in paths:   # warm-up (code objects, FFT plans, solver handles, allocator)
        fn()
        results[name] = fn()
    torch.cuda.synchronize()
    # the values: (b) against (a) per row -- one float32 ulp for each of the two float32 roundings, and 1e-7 dB for two float64 routes
    a, b = results["hip"].double(), results["torch"].double()
    ulp = torch.from_numpy(np.spacing(np.abs(a.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(dev)
    worst = float(((a - b).abs() / ulp).max())
    assert torch.isfinite(a).all() and ((a - b).abs() <= 2.0 * ulp + 1e-7).all(), f"(a) and (b) differ by up to {worst} float32 ulp"
    # the workspaces
    ws_hip = int(load().eben_sdr_workspace(args.clips, t_max, L))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch_sdr(preds, target, L)
    torch.cuda.synchronize()
    ws_torch = int(torch.cuda.max_memory_allocated() - base)

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
        lines.append(dict(path=name, clips=args.clips, filter_length=L, audio_seconds=round(sum(lengths) / FS, 1), reps=args.reps,
                          median_ms=round(statistics.median(s), 3), min_ms=round(min(s), 3), max_ms=round(max(s), 3)))
        print(json.dumps(lines[-1]), flush=True)
    by = {l["path"]: l for l in lines}
    hip, solve, ref = by["hip"], by["hip_solve"], by["torch"]
    corr_ms = hip["median_ms"] - solve["median_ms"]
    d, w = by["evaluate_clips_default"], by["evaluate_clips_with_sdr"]
    summary = [f"sdr_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} pairs of 1-12 s at 16 kHz ({sum(lengths) / FS:.0f} s of audio, "
               f"longest {t_max} samples), filter_length {L}, medians of {args.reps} alternated calls (min .. max)"]
    for l in lines:
        summary.append(f"  {l['path']:>26}: {l['median_ms']:9.3f} ms  ({l['min_ms']:.3f} .. {l['max_ms']:.3f})")
    summary += [
        f"  (a) / (b) = {hip['median_ms'] / ref['median_ms']:.3f}: the ragged HIP call takes {hip['median_ms']:.3f} ms, the torch route {ref['median_ms']:.3f} ms; "
        f"values agree within {worst:.2f} float32 ulp of (a) on every row",
        f"  (a) apart: the solve {solve['median_ms']:.3f} ms (the call with every length 1), moments + correlation {corr_ms:.3f} ms by difference; "
        f"the correlations are {fmas:.3e} fp64 FMAs = {floor_ms:.3f} ms at the vector-fp64 peak: the two passes over the samples take "
        f"{corr_ms / floor_ms:.2f} x that floor",
        f"  workspace: (a) {ws_hip} bytes ({ws_hip / 2 ** 20:.1f} MiB), (b) {ws_torch} bytes at torch's allocator peak ({ws_torch / 2 ** 20:.1f} MiB)",
        f"  evaluate_clips: \"sdr\" adds {w['median_ms'] - d['median_ms']:.3f} ms to the default call's {d['median_ms']:.3f} ms "
        f"(its own spread {d['max_ms'] - d['min_ms']:.3f} ms)"]
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
