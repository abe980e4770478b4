"""Time the device data front end (vibravox_amd.collate / vibravox_amd.filters) against the same work done the reference's way on
the host: the per-item loops of the float64 CPU restatement (tests/frontend_oracle.py) with 16 threads.

    python tools/frontend_bench.py [--threads 16] [--iters 50] [--out FILE]

Cases (16 kHz): bwe_collate of 32 clips of 3-6 s to 2.5 s; the SNR-controlled noisy collate of the same clips with 30 s noise clips;
remove_hf at (32, 32 000) and at (1, 1 024 000) -- the same number of samples, so the ratio of the two times shows whether time is
parallel.  Two more lines time the kernels alone at 256 x 160 000 samples (one biquad call, the clip powers), where the launches no
longer set the time.  Device time is host wall time around `iters` calls ending in a synchronise (after warm-up), so it includes the planner's
draws and the launches; "hbm_fraction" is each case's algorithmic bytes / time as a fraction of 8 TB/s.  Prints one JSON line per
case and a summary.  Measured-once figures: no threshold hangs on them."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12   # bytes / s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from tests import frontend_oracle as F
    from vibravox_amd.collate import bwe_collate, noisy_bwe_collate
    from vibravox_amd.filters import remove_hf

    assert torch.cuda.is_available(), "frontend_bench times the device path: it needs an MI355X"
    torch.set_num_threads(args.threads)
    fs, strategy, snr = 16000, "constant_length-2500-ms", (-3.0, 5.0)
    g = torch.Generator().manual_seed(0)
    lengths = [int(n) for n in torch.randint(3 * fs, 6 * fs + 1, (32,), generator=g)]
    batch = [{"audio_body_conducted": torch.rand(n, generator=g) - 0.5, "audio_airborne": torch.rand(n, generator=g) - 0.5,
              "audio_body_conducted_speechless_noisy": (torch.rand(30 * fs, generator=g) - 0.5) * 0.3} for n in lengths]
    dev_batch = [{k: v.cuda() for k, v in b.items()} for b in batch]
    t_out = int(fs * 2.5)

    def timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def host(fn, reps=3):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    lines = []

    def record(case, dev_ms, cpu_ms, nbytes, **extra):
        line = dict(case=case, device_ms=round(dev_ms, 4), host_oracle_ms=round(cpu_ms, 2), host_threads=args.threads,
                    speedup=round(cpu_ms / dev_ms, 1), algorithmic_mb=round(nbytes / 1e6, 2),
                    hbm_fraction=round(nbytes / (dev_ms * 1e-3) / PEAK, 4), **extra)
        print(json.dumps(line), flush=True)
        lines.append(line)

    record("bwe_collate 32 x (3-6 s) -> 2.5 s", timed(lambda: bwe_collate(dev_batch, fs, strategy), args.iters),
           host(lambda: F.bwe_collate(batch, fs, strategy, False)), 32 * t_out * 4 * 4)
    record("snr collate 32 x (3-6 s), 30 s noise -> 2.5 s", timed(lambda: noisy_bwe_collate(dev_batch, fs, strategy, snr_range=snr), args.iters),
           host(lambda: F.noisy_bwe_collate_snr(batch, fs, strategy, False, snr)), (sum(lengths) + 32 * 30 * fs) * 4 + 32 * t_out * 4 * 5)
    with ThreadPoolExecutor(args.threads) as pool:
        times = {}
        for rows, t in ((32, 32000), (1, 1024000)):
            x = (0.5 * (2 * np.random.RandomState(1).rand(rows, t) - 1)).astype(np.float32)
            xd = torch.from_numpy(x).cuda()
            dev_ms = timed(lambda: remove_hf(xd, fs, 4000), args.iters)
            cpu_ms = host(lambda: list(pool.map(lambda r: F.remove_hf(r, fs, 4000), list(x))))
            err = float(np.abs(remove_hf(xd, fs, 4000).cpu().numpy() - F.remove_hf(x, fs, 4000)).max())
            times[(rows, t)] = dev_ms
            record(f"remove_hf ({rows}, {t})", dev_ms, cpu_ms, rows * t * 4 * 2, max_abs_err=err)
    # the kernels alone at sizes where the launches no longer set the time (no host counterpart is timed for these)
    from vibravox_amd.collate import clip_powers
    from vibravox_amd.filters import lowpass_biquad

    big = torch.rand(256, 160000, device="cuda") - 0.5
    ms = timed(lambda: lowpass_biquad(big, fs, 4000), 20)
    stream_lines = [dict(case="lowpass_biquad (256, 160000): one eben_biquad call of three passes", device_ms=round(ms, 4),
                         algorithmic_mb=round(big.numel() * 8 / 1e6, 1), hbm_fraction=round(big.numel() * 8 / (ms * 1e-3) / PEAK, 4),
                         moved_mb=round(big.numel() * 12 / 1e6, 1), hbm_fraction_moved=round(big.numel() * 12 / (ms * 1e-3) / PEAK, 4))]
    clips = [big[i] for i in range(256)]
    ms = timed(lambda: clip_powers(clips), 20)
    stream_lines.append(dict(case="clip_powers 256 x 160000", device_ms=round(ms, 4), algorithmic_mb=round(big.numel() * 4 / 1e6, 1),
                             hbm_fraction=round(big.numel() * 4 / (ms * 1e-3) / PEAK, 4)))
    for l in stream_lines:
        print(json.dumps(l), flush=True)
    ratio = times[(1, 1024000)] / times[(32, 32000)]
    dev = torch.cuda.get_device_properties(0).name
    summary = [f"frontend_bench on {dev}: device front end vs the float64 CPU restatement's per-item loops on {args.threads} threads "
               f"(measured once, {args.iters} calls per case)"]
    for l in lines:
        summary.append(f"  {l['case']:>46}: device {l['device_ms']:.3f} ms ({100 * l['hbm_fraction']:.2f} % of 8 TB/s on {l['algorithmic_mb']} MB), "
                       f"host {l['host_oracle_ms']:.1f} ms ({l['speedup']}x)")
    summary.append(f"  remove_hf (1, 1 024 000) / (32, 32 000) time ratio: {ratio:.2f} (1 = time is as parallel as rows)")
    for l in stream_lines:
        moved = f"; {100 * l['hbm_fraction_moved']:.1f} % on the {l['moved_mb']} MB it moves" if "moved_mb" in l else ""
        summary.append(f"  {l['case']}: device {l['device_ms']:.3f} ms ({100 * l['hbm_fraction']:.1f} % of 8 TB/s on {l['algorithmic_mb']} MB{moved})")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines + stream_lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
