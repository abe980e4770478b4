"""The PQMF filter-bank kernels alone on the device at BASELINE config 2 (batch 32 x 31968 samples, 4 bands, 32 taps): us per launch and the
achieved HBM rate of each shape (vibravox/torch_modules/dsp/pqmf.py:194-213 -- analysis = `pqmf_analysis_kernel`, synthesis + band sum =
`pqmf_synthesis_kernel`: the polyphase forms on wave shuffles; EBEN_PQMF_SHUFFLE=0 selects the LDS forms `fir_decimate_kernel` /
`fir_interp_sum_kernel`) and of their adjoints (the backward of the generator's synthesis / the balancing seeds).
Algorithmic bytes: every input sample read once, every output sample written once (4 B each).  Peak 8 TB/s (6.3 measured for a copy).
Usage: python tools/pqmf_bench.py [--iters 50]

With --bank M N: the M-band x N-tap bank instead (the tap-tiled kernels of csrc/fir_bank.hip; PseudoQMFBanks' class defaults are 32 1024),
at --batch x (1024 M - N) samples = 1024 frames: analysis, synthesis + band sum and their two adjoints as ONE launch each, with the fraction
of the fp32 roof (2 M N frames batch FLOP at 157.3 TFLOP/s) and of the byte roof, beside the baseline a library without those kernels is
left with -- M single-band launches of the whole-bank-in-LDS kernels (plus one add of the M outputs for the band sum).  --baseline-only
times only that baseline and needs nothing newer than the single-band launches."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=50); ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--bank", type=int, nargs=2, metavar=("M", "N"), default=None); ap.add_argument("--baseline-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda")
pq = PseudoQMFBanks(decimation=4, kernel_size=32).to(dev)
B, T = args.batch, 31968


def timed(fn):
    for _ in range(5): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3


def bank_rows(m, n):
    """One large bank: (name, us of the one-launch form or None, us of the m-launch baseline) per direction."""
    from vibravox_amd import ops
    pqb = PseudoQMFBanks(decimation=m, kernel_size=n).to(dev)
    frames, off = 1024, -(n - 1)
    t = frames * m - n
    wa, ws = (w.detach().reshape(m, n).contiguous() for w in (pqb.analysis_weights, pqb.synthesis_weights))
    x = 0.1 * torch.randn(B, 1, t, device=dev)
    y = 0.1 * torch.randn(B, m, frames, device=dev)
    ys = [y[:, k:k + 1].contiguous() for k in range(m)]
    rows = []
    with torch.no_grad():
        for name, w in (("analysis", wa), ("synthesis adjoint (analysis-form kernel)", ws)):
            wk = [w[k:k + 1].contiguous() for k in range(m)]
            base = timed(lambda: [ops._fir_decimate(x, wk[k], frames, 1, n, m, off) for k in range(m)])
            one = None if args.baseline_only else timed(lambda: ops._fir_decimate(x, w, frames, m, n, m, off))
            rows.append((f"{name} ({B},1,{t}) -> ({B},{m},{frames})", one, base))
        for name, w in (("synthesis + band sum", ws), ("analysis adjoint (synthesis-form kernel)", wa)):
            wk = [w[k:k + 1].contiguous() for k in range(m)]
            base = timed(lambda: torch.stack([ops._fir_interp_sum(ys[k], wk[k], t, 1, n, m, off) for k in range(m)]).sum(0))
            one = None if args.baseline_only else timed(lambda: ops._fir_interp_sum(y, w, t, m, n, m, off))
            rows.append((f"{name} ({B},{m},{frames}) -> ({B},1,{t})", one, base))
    flop, nbytes = 2.0 * m * n * frames * B, 4.0 * (B * t + B * m * frames + m * n)
    print(f"bank {m} x {n}, {B} x {t} samples = {frames} frames: {flop / 1e9:.2f} GFLOP = {flop / 157.3e6:.1f} us at 157.3 TFLOP/s fp32, "
          f"{nbytes / 1e6:.1f} MB = {nbytes / 8e6:.1f} us at 8 TB/s")
    print(f"{'launch':72s} {'us':>8s} {'of fp32':>8s} {'of 8TB/s':>8s} {f'{m} launches us':>15s} {'ratio':>6s}")
    for name, one, base in rows:
        if one is None:
            print(f"{name:72s} {'-':>8s} {'-':>8s} {'-':>8s} {base:15.1f} {'-':>6s}")
        else:
            print(f"{name:72s} {one:8.1f} {flop / 157.3e6 / one:8.3f} {nbytes / 8e6 / one:8.3f} {base:15.1f} {base / one:6.2f}")


if args.bank:
    bank_rows(*args.bank)
    if args.baseline_only:
        sys.exit(0)
    print()
x = 0.1 * torch.randn(B, 1, T, device=dev)
print(f"{'launch':64s} {'us':>7s} {'MB':>7s} {'TB/s':>6s} {'of 8':>5s}")
rows = []
from vibravox_amd import ops
n = pq.kernel_size
wa = pq.analysis_weights.detach().reshape(4, 32).contiguous()
ws = pq.synthesis_weights.detach().reshape(4, 32).contiguous()
with torch.no_grad():   # the launches themselves (ops._fir_*): through the module + autograd.Function a call costs ~13 us of host time
    for bands in (2, 4):
        y = pq(x, "analysis", bands=bands)
        wb = wa[:bands].contiguous()
        us = timed(lambda: ops._fir_decimate(x, wb, y.shape[2], bands, n, 4, -(n - 1)))
        rows.append((f"analysis, {bands} bands ({B},1,{T}) -> {tuple(y.shape)}", us, (x.numel() + y.numel()) * 4))
    bands4 = pq(x, "analysis", bands=4)
    out = pq.synthesis_sum(bands4)
    us = timed(lambda: ops._fir_interp_sum(bands4, ws, T, 4, n, 4, -(n - 1)))
rows.append((f"synthesis + band sum {tuple(bands4.shape)} -> {tuple(out.shape)}", us, (bands4.numel() + out.numel()) * 4))
# the adjoints as the kernels autograd launches for them (ops._FirInterpSumFn.backward = eben_fir_decimate, ops._FirDecimateFn.backward =
# eben_fir_interp_sum), HIP events around the launches -- not around torch.autograd.grad, whose ~40 us of host time the round-4 row timed
w4 = ws
g = torch.randn_like(out)
with torch.no_grad():
    us = timed(lambda: ops._fir_decimate(g, w4, bands4.shape[2], 4, n, 4, -(n - 1)))
rows.append((f"synthesis adjoint (analysis-form kernel) {tuple(out.shape)} -> {tuple(bands4.shape)}", us, (out.numel() + bands4.numel()) * 4))
gb = torch.randn_like(bands4)
with torch.no_grad():
    us = timed(lambda: ops._fir_interp_sum(gb, wa, T, 4, n, 4, -(n - 1)))
rows.append((f"analysis adjoint (synthesis-form kernel) {tuple(bands4.shape)} -> ({B}, 1, {T})", us, (gb.numel() + B * T) * 4))
for name, us, nb in rows:
    r = nb / us / 1e6
    assert r / 8 <= 1.0
    print(f"{name:64s} {us:7.1f} {nb / 1e6:7.1f} {r:6.2f} {r / 8:5.2f}")
