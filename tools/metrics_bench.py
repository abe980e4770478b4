"""Time the device SI-SDR + STOI (vibravox_amd.metrics) against the float64 CPU restatement (tests/metrics_oracle.py) run the
way torchmetrics runs pystoi -- a device->host copy, then one clip at a time -- spread over a pool of CPU worker processes.

    python tools/metrics_bench.py [--workers 16] [--iters 20] [--out FILE]

Shapes: a validation batch of 32 x 2 s and a batch of 8 x 10 s, 16 kHz.  Device time is host wall time around `iters` calls
ending in a synchronise (after warm-up); CPU time is the wall time of one pass over the batch, copy included.  Prints one
JSON line per shape and a summary."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cpu_clip(args):
    from tests import metrics_oracle as M

    p, t, fs = args
    return M.stoi_clip(t, p, fs), float(M.si_sdr(p, t))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from tests import metrics_oracle as M
    from vibravox_amd.metrics import si_sdr, stoi

    assert torch.cuda.is_available(), "metrics_bench times the device path: it needs an MI355X"
    fs = 16000
    lines = []
    with ProcessPoolExecutor(args.workers) as pool:
        list(pool.map(_cpu_clip, [(np.ones(4000), np.ones(4000), 10000)] * args.workers))   # start the workers
        for name, rows, seconds in (("val_32x2s", 32, 2), ("8x10s", 8, 10)):
            t = fs * seconds
            clean = M.speech_like(name, rows, t, fs).astype(np.float32)
            noisy = (clean + 0.05 * np.random.RandomState(0).randn(rows, t)).astype(np.float32)
            p, g = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
            for _ in range(3):
                si_sdr(p, g), stoi(p, g, fs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                a, d = si_sdr(p, g), stoi(p, g, fs)
            torch.cuda.synchronize()
            dev_ms = (time.perf_counter() - t0) * 1e3 / args.iters
            t0 = time.perf_counter()
            pc, gc = p.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
            res = list(pool.map(_cpu_clip, [(pc[i], gc[i], fs) for i in range(rows)]))
            cpu_ms = (time.perf_counter() - t0) * 1e3
            d_err = float(np.abs(d.cpu().numpy() - np.array([r[0] for r in res])).max())
            s_err = float(np.abs(a.cpu().numpy() - np.array([r[1] for r in res])).max())
            line = dict(shape=name, rows=rows, samples=t, fs=fs, device_ms=round(dev_ms, 3), cpu_oracle_ms=round(cpu_ms, 1),
                        cpu_workers=args.workers, speedup=round(cpu_ms / dev_ms, 1), max_abs_stoi_err=d_err, max_abs_si_sdr_err_db=s_err)
            print(json.dumps(line), flush=True)
            lines.append(line)
    dev = torch.cuda.get_device_properties(0).name
    summary = [f"metrics_bench on {dev}: device SI-SDR + STOI vs the float64 CPU restatement on {args.workers} worker processes"]
    for l in lines:
        summary.append(f"  {l['shape']:>10}: device {l['device_ms']:.3f} ms, CPU {l['cpu_oracle_ms']:.1f} ms ({l['speedup']}x), "
                       f"max|dSTOI| {l['max_abs_stoi_err']:.1e}, max|dSI-SDR| {l['max_abs_si_sdr_err_db']:.1e} dB")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
