"""What the frame-based speech measures cost on a test split: the one ragged `metrics.speech_measures` call against the same definitions
in batched float64 torch on the same device and the same padded batch, each measure alone, the frame kernel against a device copy of the
two buffers, and `inference.evaluate_clips` with its default metrics against the same call with the four keys added.

    python tools/measures_bench.py [--clips 256] [--reps 20] [--budget 4194304] [--out profiles/measures_bench.txt]

Workload: the corpus of tools/eval_metrics_bench.py -- `--clips` (corrupted, reference) pairs with lengths uniform in 1 .. 12 s at 16 kHz
(seed 0), the corrupted clip its reference plus white noise at 5 dB.  The measure paths score the corrupted clips against their references
in one zero-padded (clips, longest) batch.

  (a) hip_all     one `metrics.speech_measures(preds, target, 16000, lengths)` call, all four measures: the frame kernel (segmental SNR,
                  autocorrelations, Levinson, LLR, cepstra; float64), the table and spectral kernels (one float32 complex transform per
                  frame, band sums float64) and the per-row finish.
      hip_<name>  the same call with `which=(<name>,)`; hip_frames is `which=("seg_snr", "llr", "cd")`: the frame kernel and the finish,
                  no spectral kernel.  (Kernel times proper come from a kernel trace in a run of its own:
                  `rocprofv3 --kernel-trace --stats -- python tools/measures_bench.py --only-hip`.)
  (b) torch_all   the same definitions on the same padded batch in float64 torch: `unfold` frames under the window, `torch.fft.rfft`,
                  the band filters as a matrix, autocorrelations as 17 shifted products, a 16-step batched Levinson recursion, Toeplitz
                  quadratic forms, a sort for the trimmed means; in chunks of 32 rows (the frames of 256 rows in float64 would take 6 GB a
                  signal).  The reference for the time; its values are compared with (a) row by row: seg_snr, llr and cd within
                  2 float32 ulp + 1e-7 (both sides are float32 roundings of float64 routes), fw_seg_snr within 2 float32 ulp + 2e-5 dB
                  (a float32 transform moves a row by a few 1e-6 dB; measured on the CPU by tests/test_measures_oracle.py).
      copy        `preds.clone(); target.clone()`: what reading and writing the two buffers once costs.
  (c) evaluate_clips through EBENGenerator(4, 32, 2) with the default metrics, and with the four keys added.

Every path is timed with HIP events around one whole call, `--reps` calls after two warm-up calls, the paths alternating within one
session; medians with min .. max as the run-to-run spread."""
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

NAMES = ("seg_snr", "fw_seg_snr", "llr", "cd")
EPS = 2.0 ** -52
CENT = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
        1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63)
BW = (70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457,
      199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)


def band_matrix(fs, n2):
    j = np.arange(n2, dtype=np.float64)
    out = np.zeros((len(CENT), n2))
    for i, (cent, bw) in enumerate(zip(CENT, BW)):
        g = np.exp(-11.0 * ((j - np.floor(cent / (fs / 2) * n2)) / (bw / (fs / 2) * n2)) ** 2 + np.log(70.0) - np.log(bw))
        g[g <= np.exp(-30.0 / (2.0 * 2.303))] = 0.0
        out[i] = g
    return out


def torch_measures(preds, target, lens, fs, window, bands, geometry, chunk=32):
    """The four measures of every row of a zero-padded batch, float64 torch; (4, rows) float32."""
    import torch

    w, s, order, n_fft = geometry
    rows, t_max = preds.shape
    f_max = (t_max - w) // s
    out = torch.empty((4, rows), dtype=torch.float32, device=preds.device)
    inf = float("inf")
    for r0 in range(0, rows, chunk):
        p = preds[r0 : r0 + chunk].double().unfold(-1, w, s)[:, :f_max] * window
        c = target[r0 : r0 + chunk].double().unfold(-1, w, s)[:, :f_max] * window
        nf = torch.clamp((lens[r0 : r0 + chunk].long() - w) // s, min=0)
        live = torch.arange(f_max, device=preds.device)[None, :] < nf[:, None]
        cc, pp, dd = (c * c).sum(-1), (p * p).sum(-1), ((c - p) ** 2).sum(-1)
        seg = torch.clamp(10.0 * torch.log10(cc / (dd + EPS) + EPS), -10.0, 35.0)
        full = live & (cc != 0) & (pp != 0)
        # frequency-weighted segmental SNR
        cs, ps = torch.fft.rfft(c, n=n_fft)[..., : n_fft // 2].abs(), torch.fft.rfft(p, n=n_fft)[..., : n_fft // 2].abs()
        ec = (cs / cs.sum(-1, keepdim=True)) @ bands.T
        ep = (ps / ps.sum(-1, keepdim=True)) @ bands.T
        snr = torch.clamp(10.0 * torch.log10(ec ** 2 / torch.clamp((ec - ep) ** 2, min=EPS)), -10.0, 35.0)
        wgt = ec ** 0.2
        fw = (wgt * snr).sum(-1) / wgt.sum(-1)
        # LPC
        def lpc(x):
            r = torch.stack([(x[..., : w - k] * x[..., k:]).sum(-1) for k in range(order + 1)], dim=-1)
            a = torch.zeros_like(r)
            e = r[..., 0].clone()
            for i in range(1, order + 1):
                acc = (a[..., 1:i] * r[..., 1:i].flip(-1)).sum(-1) if i > 1 else torch.zeros_like(e)
                k = (r[..., i] - acc) / e
                if i > 1:
                    a[..., 1:i] = a[..., 1:i] - k[..., None] * a[..., 1:i].flip(-1)
                a[..., i] = k
                e = e * (1.0 - k * k)
            return r, a[..., 1:]

        def cepstrum(a):
            cep = torch.zeros(a.shape[:-1] + (order + 1,), dtype=a.dtype, device=a.device)
            cep[..., 1] = a[..., 0]
            ks = torch.arange(1, order + 1, device=a.device, dtype=a.dtype)
            for m in range(2, order + 1):
                acc = (ks[: m - 1] * cep[..., 1:m] * a[..., : m - 1].flip(-1)).sum(-1)
                cep[..., m] = a[..., m - 1] + acc / m
            return cep[..., 1:]

        r_c, a_c = lpc(c)
        _, a_p = lpc(p)
        idx = torch.arange(order + 1, device=preds.device)
        toep = r_c[..., (idx[:, None] - idx[None, :]).abs()]
        one = torch.ones_like(a_c[..., :1])
        big_c, big_p = torch.cat([one, -a_c], -1), torch.cat([one, -a_p], -1)
        quad = lambda v: ((v[..., None, :] @ toep) @ v[..., :, None])[..., 0, 0]
        llr = torch.clamp(torch.log(quad(big_p) / quad(big_c)), max=2.0)
        d = cepstrum(a_c) - cepstrum(a_p)
        cd = torch.clamp(10.0 / np.log(10.0) * torch.sqrt(2.0 * (d * d).sum(-1)), max=10.0)
        # per row
        zero = torch.zeros_like(seg)
        count = full.sum(-1)
        out[0, r0 : r0 + chunk] = (torch.where(live, seg, zero).sum(-1) / nf).float()
        out[1, r0 : r0 + chunk] = (torch.where(full, fw, zero).sum(-1) / count).float()
        keep = (95 * count + 50) // 100
        first = torch.arange(f_max, device=preds.device)[None, :] < keep[:, None]
        for k, v in ((2, llr), (3, cd)):
            ordered = torch.sort(torch.where(full, v, torch.full_like(v, inf)), dim=-1).values
            out[k, r0 : r0 + chunk] = (torch.where(first, ordered, zero).sum(-1) / keep).float()
    return out


def summarise_trace(db_path, out) -> None:
    """Per-kernel times of the speech-measure kernels in a `rocprofv3 --kernel-trace` database of `--only-hip` (three calls of (a))."""
    import sqlite3

    rows = sqlite3.connect(db_path).execute(
        "select name, count(*), min(duration), avg(duration), max(duration) from kernels where name like '%measures_%' group by name "
        "order by avg(duration) desc").fetchall()
    assert rows, f"no speech-measure kernel in {db_path}"
    lines = ["kernel trace of `measures_bench.py --only-hip` (rocprofv3 --kernel-trace, a run of its own; times under tracing, in us): "
             "calls, min, mean, max"]
    for name, calls, lo, mean, hi in rows:
        short = name[name.index("measures_"):].split("(")[0].split("<")[0] + ("<16000>" if "<16000" in name else "")
        lines.append(f"  {short:>34}: {calls:3d}  {lo / 1e3:9.1f} {mean / 1e3:9.1f} {hi / 1e3:9.1f}")
    lines.append(f"  sum of the means: {sum(r[3] for r in rows) / 1e3:.1f} us")
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=int, default=1 << 22)
    ap.add_argument("--only-hip", action="store_true", help="three calls of (a) and nothing else: the program of a kernel trace")
    ap.add_argument("--trace-db", default=None, help="the rocpd database a kernel trace of --only-hip left: write its per-kernel times to --out and stop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_db:
        summarise_trace(args.trace_db, args.out)
        return

    import torch

    from vibravox_amd import metrics as M
    from vibravox_amd.inference import DEFAULT_EVAL_METRICS, EVAL_METRICS_FRAMED, evaluate_clips
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "measures_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda")
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
    geometry = M.measures_geometry(FS)
    w, s, _, n_fft = geometry
    frames = sum((t - w) // s for t in lengths)

    def hip(which):
        got = M.speech_measures(preds, target, FS, lens, which)
        return torch.stack([got[name] for name in which])

    if args.only_hip:
        for _ in range(3):
            hip(NAMES)
        torch.cuda.synchronize()
        return

    window = torch.from_numpy(M.measures_window(FS)).to(dev)
    bands = torch.from_numpy(band_matrix(FS, n_fft // 2)).to(dev)
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    with_framed = tuple(DEFAULT_EVAL_METRICS) + tuple(EVAL_METRICS_FRAMED)
    paths = [("hip_all", lambda: hip(NAMES)), ("torch_all", lambda: torch_measures(preds, target, lens, FS, window, bands, geometry))]
    paths += [(f"hip_{name}", (lambda name: lambda: hip((name,)))(name)) for name in NAMES]
    paths += [("hip_frames", lambda: hip(("seg_snr", "llr", "cd"))), ("copy", lambda: (preds.clone(), target.clone())),
              ("evaluate_clips_default", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget)),
              ("evaluate_clips_with_framed", lambda: evaluate_clips(gen, corrupted, reference, max_batch_samples=args.budget, metrics=with_framed))]
    results = {}
    for name, fn in paths:   # warm-up (code objects, FFT plans, allocator)
        fn()
        results[name] = fn()
    torch.cuda.synchronize()
    a, b = results["hip_all"].double(), results["torch_all"].double()
    ulp = torch.from_numpy(np.spacing(np.abs(a.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(dev)
    diff = (a - b).abs()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    worst = {name: (float(diff[k].max()), float((diff[k] / ulp[k]).max())) for k, name in enumerate(NAMES)}
    for k, name in enumerate(NAMES):
        own = 2e-5 if name == "fw_seg_snr" else 1e-7
        assert (diff[k] <= 2.0 * ulp[k] + own).all(), f"(a) and (b) differ in {name} by up to {worst[name][0]:.3e} ({worst[name][1]:.2f} float32 ulp)"

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
        v = times[name]
        lines.append(dict(path=name, clips=args.clips, audio_seconds=round(sum(lengths) / FS, 1), frames=frames, reps=args.reps,
                          median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)))
        print(json.dumps(lines[-1]), flush=True)
    by = {l["path"]: l for l in lines}
    hip_all, ref, fr, cp = by["hip_all"], by["torch_all"], by["hip_frames"], by["copy"]
    d, f = by["evaluate_clips_default"], by["evaluate_clips_with_framed"]
    summary = [f"measures_bench on {torch.cuda.get_device_properties(0).name}: {args.clips} pairs of 1-12 s at 16 kHz ({sum(lengths) / FS:.0f} s of audio, "
               f"{frames} frames, longest {t_max} samples), medians of {args.reps} alternated calls (min .. max)"]
    for l in lines:
        summary.append(f"  {l['path']:>27}: {l['median_ms']:9.3f} ms  ({l['min_ms']:.3f} .. {l['max_ms']:.3f})")
    summary += [
        f"  (a) / (b) = {hip_all['median_ms'] / ref['median_ms']:.4f}: the ragged HIP call takes {hip_all['median_ms']:.3f} ms, the float64 torch route "
        f"{ref['median_ms']:.3f} ms",
        "  values, largest |(a) - (b)| over the rows: " + ", ".join(f"{name} {worst[name][0]:.2e} ({worst[name][1]:.2f} float32 ulp)" for name in NAMES),
        f"  frame kernel + finish (hip_frames) {fr['median_ms']:.3f} ms against {cp['median_ms']:.3f} ms for a device copy of the two buffers: "
        f"{fr['median_ms'] / cp['median_ms']:.1f} x the copy ({1e3 * fr['median_ms'] / frames:.3f} us a frame; the work is float64 arithmetic on "
        f"frames that overlap fourfold, not traffic)",
        f"  evaluate_clips: the four keys add {f['median_ms'] - d['median_ms']:.3f} ms to the default call's {d['median_ms']:.3f} ms "
        f"(its own spread {d['max_ms'] - d['min_ms']:.3f} ms)"]
    print("\n".join(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(l) for l in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
