"""Multi-resolution STFT loss on the HIP tap-conv (windowed-DFT GEMM) and reduction kernels.

Stands in for ``auraloss.freq.MultiResolutionSTFTLoss`` as instantiated by
``configs/lightning_module/loss_module/multi_stft.yaml:1-18`` and called at
``vibravox/lightning_modules/eben.py:195-198`` (``loss(enhanced, reference)``).  auraloss is a
third-party dependency that is not vendored in the reference (pyproject.toml:21, unpinned; 0.4.0
semantics restated: per-item spectral convergence, log-magnitude L1, A-weighting FIR prefilter,
mean over resolutions) -- parity for this term is therefore *unpinned* (see DESIGN.md).

Per resolution the STFT is a framing pass + one dense GEMM: hann(win) centred in n_fft and center=True
reflect padding reduce to frames of ``win`` samples at hop ``hop`` over the signal reflect-padded by
``n_fft//2 - (n_fft - win)//2`` (``win/2`` when both are even), multiplied by the 2*(n_fft/2+1) rows
[w cos ; -w sin] of the windowed DFT basis.  Any ``win <= n_fft`` is accepted, as by torch.stft.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from ... import ops


_DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "data")


def a_weighting_taps(fs: float, ntaps: int = 101) -> torch.Tensor:
    """The A-weighting FIR of auraloss ``FIRFilter("aw")``.  For the reference's configuration (16 kHz, 101 taps:
    multi_stft.yaml:15,18) the committed table is loaded -- the design runs through scipy's ``firls`` and must not move with
    the scipy installed on the box; ``tests/test_oracle_golden.py`` checks that it still regenerates to 1e-7."""
    path = os.path.join(_DATA, f"a_weighting_fir_{int(fs)}_{int(ntaps)}.npy")
    if float(fs) == int(fs) and os.path.exists(path):
        return torch.from_numpy(np.load(path).astype("float32"))
    return design_a_weighting_taps(fs, ntaps)


def design_a_weighting_taps(fs: float, ntaps: int = 101) -> torch.Tensor:
    """IEC A-weighting prototype -> bilinear -> freqz(512) -> firls(ntaps) (auraloss FIRFilter 'aw')."""
    import scipy.signal

    f1, f2, f3, f4, a1000 = 20.598997, 107.65265, 737.86223, 12194.217, 1.9997
    num = [(2 * np.pi * f4) ** 2 * (10 ** (a1000 / 20)), 0, 0, 0, 0]
    den = np.polymul([1, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    den = np.polymul(np.polymul(den, [1, 2 * np.pi * f3]), [1, 2 * np.pi * f2])
    b, a = scipy.signal.bilinear(num, den, fs=fs)
    w, h = scipy.signal.freqz(b, a, worN=512, fs=fs)
    return torch.tensor(scipy.signal.firls(ntaps, w, abs(h), fs=fs).astype("float32"))


def windowed_dft_basis(n_fft: int, win: int) -> torch.Tensor:
    """(2*bins, 1, win): rows k<bins  w[j] cos(2 pi k (j+lp)/n_fft), rows bins+k  -w[j] sin(...)."""
    bins = n_fft // 2 + 1
    window = torch.hann_window(win, dtype=torch.float64)
    lp = (n_fft - win) // 2
    n = torch.arange(win, dtype=torch.float64) + lp
    k = torch.arange(bins, dtype=torch.float64).unsqueeze(1)
    ang = 2 * math.pi * k * n / n_fft
    basis = torch.cat((torch.cos(ang) * window, -torch.sin(ang) * window), dim=0)
    return basis.to(torch.float32).unsqueeze(1).contiguous()


class MultiResolutionSTFTLoss(torch.nn.Module):
    def __init__(self, fft_sizes: Sequence[int] = (1024, 2048, 512), hop_sizes: Sequence[int] = (120, 240, 50),
                 win_lengths: Sequence[int] = (600, 1200, 240), window: str = "hann_window", w_sc: float = 1.0,
                 w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0, sample_rate: Optional[float] = None,
                 scale: Optional[str] = None, n_bins: Optional[int] = None, perceptual_weighting: bool = False,
                 scale_invariance: bool = False, eps: float = 1e-8, **kwargs):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        for n_fft, win in zip(fft_sizes, win_lengths):
            if not 0 < win <= n_fft:
                raise ValueError(f"win_length must satisfy 0 < win_length <= n_fft, got win_length={win}, n_fft={n_fft}")
        if window != "hann_window" or w_sc != 1.0 or w_log_mag != 1.0 or w_lin_mag or w_phs or scale or scale_invariance:
            raise NotImplementedError("only the configuration of configs/lightning_module/loss_module/multi_stft.yaml is built")
        if perceptual_weighting and sample_rate is None:
            raise ValueError("`sample_rate` must be supplied when `perceptual_weighting = True`.")
        self.eps = eps
        self.fft_sizes, self.hop_sizes, self.win_lengths = tuple(fft_sizes), tuple(hop_sizes), tuple(win_lengths)
        self.register_buffer("fir", a_weighting_taps(sample_rate) if perceptual_weighting else None, persistent=False)
        self._plans = None
        for i, (n_fft, win) in enumerate(zip(self.fft_sizes, self.win_lengths)):
            basis = windowed_dft_basis(n_fft, win).squeeze(1)                       # (2*bins, win)
            self.register_buffer(f"basis_{i}", basis.unsqueeze(-1).contiguous(), persistent=False)            # (2*bins, win, 1)
            self.register_buffer(f"basis_t_{i}", basis.t().contiguous().unsqueeze(-1), persistent=False)      # (win, 2*bins, 1)

    def _build_plans(self):
        plans = []
        for i, (n_fft, hop, win) in enumerate(zip(self.fft_sizes, self.hop_sizes, self.win_lengths)):
            bins = n_fft // 2 + 1
            # hann(win) centred in n_fft (torch.stft puts it (n_fft - win)//2 samples into the frame) + center=True reflect
            # padding of n_fft//2 == frames of length `win` taken at reflect padding n_fft//2 - (n_fft - win)//2 (the window is
            # zero outside its `win` samples); win/2 when n_fft and win are both even
            plans.append(ops.StftPlan(n_fft=n_fft, hop=hop, win=win, bins=bins, pad=n_fft // 2 - (n_fft - win) // 2,
                                      spec_f=ops.ConvSpec(c_in=win, c_out=2 * bins, ksize=1), basis_f=getattr(self, f"basis_{i}"),
                                      spec_t=ops.ConvSpec(c_in=2 * bins, c_out=win, ksize=1), basis_t=getattr(self, f"basis_t_{i}"),
                                      cache_fwd=ops.PackedWeights(), cache_bwd=ops.PackedWeights()))
        return plans

    #: arithmetic of the windowed-DFT contractions: "folded" (exact fp32 on the even / odd parts of the frames: half the products
    #: of "dense"), "dense" (one win-channel GEMM), "bf16x3" (folded, hi / lo bf16 operand splits on the bf16 MFMA, ~2^-17
    #: relative per product), "folded_x6" / "folded_x3" (folded, the tap-conv's split bf16 operands: three pieces per operand =
    #: fp32-grade products at 6/16 of the fp32 MFMA's cost / two pieces, ~2^-17 -- EBENLightningModule.stft_math)
    stft_math: str = os.environ.get("EBEN_STFT_MATH", "folded")

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if self.stft_math not in ("folded", "dense", "bf16x3", "folded_x3", "folded_x6"):
            raise ValueError(f"unknown STFT math {self.stft_math!r}")
        if self._plans is None or self._plans[0].basis_f.device != x.device or self._plans[0].basis_f.data_ptr() != self.basis_0.data_ptr():
            self._plans = self._build_plans()
        for p in self._plans:
            p.math = self.stft_math
        return ops.mrstft(x, y, self.fir, self._plans, self.eps)
