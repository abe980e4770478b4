"""MRSTFT loss alone on the device: forward and forward + backward time at the bench shape, and the kernels of one pass.

    python tools/mrstft_time.py [stft_math] [--mel N_BINS] [--batch B] [--length T]

``--mel N`` times the reference's commented-out option (multi_stft.yaml: scale "mel", n_bins N) instead of the default configuration;
run it with and without to set the two side by side."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("stft_math", nargs="?", default="folded_x3")
ap.add_argument("--mel", type=int, default=0, help="n_bins of scale='mel' (0: the default configuration, no scale)")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--length", type=int, default=32000)
args = ap.parse_args()

dev = torch.device("cuda", 0)
mod = bench.build_module(dev, 1234)
fn = mod.reconstructive_loss_freq_fn
if args.mel:
    fn = MultiResolutionSTFTLoss(fft_sizes=fn.fft_sizes, hop_sizes=fn.hop_sizes, win_lengths=fn.win_lengths, sample_rate=16000,
                                 perceptual_weighting=True, scale="mel", n_bins=args.mel).to(dev)
fn.stft_math = args.stft_math
config = f"mel {args.mel}" if args.mel else "default"
batch = bench.synthetic_batch(args.batch, args.length, 1234, dev)
y = batch["audio_airborne"] if "audio_airborne" in batch else list(batch.values())[0]
x = (y * 0.9 + 0.01 * torch.randn_like(y)).requires_grad_(True)
def fwd():
    return fn(x, y)
def both():
    x.grad = None
    fn(x, y).backward()
for f, name in ((fwd, "forward"), (both, "forward + backward")):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record(); torch.cuda.synchronize()
    print(f"{name}: {e0.elapsed_time(e1) / 20:.3f} ms ({fn.stft_math}, {config}, {args.batch} x {args.length})")
from torch.profiler import profile, ProfilerActivity
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    both(); torch.cuda.synchronize()
evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
evs.sort(key=lambda e: e.time_range.start)
t0 = evs[0].time_range.start
for e in evs:
    print(f"{(e.time_range.start - t0):8.1f} us  {e.time_range.end - e.time_range.start:7.1f} us  {e.name[:100]}")
