"""Time MelganMultiScalesDiscriminator's multi-rate downsampling and the whole module on the device.

    python tools/melgan_ms_bench.py [--reps 50] [--warmup 10] [--out profiles/melgan_ms_bench.txt]

Rows:
  * the fused forward launch (eben_multirate_down) and the fused adjoint launch (eben_multirate_down_adjoint) alone, 16 kHz,
    3 scales, against the HBM bytes they must move (read the waveform / write every downsampled version, and the reverse);
  * the module's forward + backward (hinge(+1) + feature matching against a detached second forward, as a discriminator
    step does) at 32 x 31968 and at the reference fixture's 4 x 15679.
Each rep is timed alone with a pair of HIP events after `warmup` untimed reps; the median and the 10th / 90th percentiles are
reported (min / max as well).  One JSON line per row, then a summary."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    import numpy as np
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = np.percentile(ms, [0, 10, 50, 90, 100])
    return dict(min_ms=round(q[0], 4), p10_ms=round(q[1], 4), median_ms=round(q[2], 4), p90_ms=round(q[3], 4), max_ms=round(q[4], 4))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melgan_ms_bench.txt"))
    args = ap.parse_args()

    import torch

    from vibravox_amd import ops
    from vibravox_amd._lib import check, load, ptr, stream
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import MelganMultiScalesDiscriminator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales

    assert torch.cuda.is_available(), "melgan_ms_bench times the device path: it needs an MI355X"
    dev, sr, scales = torch.device("cuda"), 16000, 3
    lib = load()
    packed, widths = ops._fused_plan(sr, scales, dev)
    lines = []
    for rows, t in ((32, 31968), (4, 15679)):
        x = torch.randn(rows, t, device=dev)
        outs = [torch.empty(rows, -(-t // 2 ** s), device=dev) for s in range(1, scales)]
        gs = [torch.randn_like(o) for o in outs]
        dx = torch.empty_like(x)
        down_bytes = 4 * (x.numel() + sum(o.numel() for o in outs))
        fwd = timed(lambda: check(lib.eben_multirate_down(ptr(x), ptr(packed), widths, ops._ptr_array(outs), rows, t, scales, stream())),
                    args.reps, args.warmup)
        adj = timed(lambda: check(lib.eben_multirate_down_adjoint(ptr(x), ops._ptr_array(gs), ptr(packed), widths, ptr(dx), rows, t, scales,
                                                                  stream())), args.reps, args.warmup)
        for name, r, nbytes in (("fused_forward", fwd, down_bytes), ("fused_adjoint", adj, down_bytes + 4 * x.numel())):
            lines.append(dict(row=name, rows=rows, samples=t, hbm_bytes=nbytes, gb_per_s_at_median=round(nbytes / r["median_ms"] / 1e6, 1), **r))

        torch.manual_seed(0)
        disc = MelganMultiScalesDiscriminator(sr, scales=scales).to(dev)
        fm, hinge = FeatureLossForDiscriminatorMelganMultiScales(), HingeLossForDiscriminatorMelganMultiScales()
        audio, other = torch.randn(rows, 1, t, device=dev), torch.randn(rows, 1, t, device=dev)
        audio.requires_grad_(True)

        def step():
            with torch.no_grad():
                e_b = disc(other)
            e_a = disc(audio)
            (fm(e_a, e_b) + hinge(embeddings=e_a, target=1)).backward()

        lines.append(dict(row="module_fwd_bwd", rows=rows, samples=t, **timed(step, max(10, args.reps // 5), max(3, args.warmup // 2))))
    for line in lines:
        print(json.dumps(line), flush=True)
    name = torch.cuda.get_device_properties(0).name
    summary = [f"melgan_ms_bench on {name} ({sr} Hz, {scales} scales); median [p10, p90] of per-rep HIP-event times"]
    for l in lines:
        extra = f", {l['hbm_bytes'] / 1e6:.1f} MB -> {l['gb_per_s_at_median']} GB/s" if "hbm_bytes" in l else ""
        summary.append(f"  {l['row']:>15} {l['rows']:>2} x {l['samples']}: {l['median_ms']:.4f} ms [{l['p10_ms']:.4f}, {l['p90_ms']:.4f}]{extra}")
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
