"""float64 restatement of MultiResolutionSTFTLoss with every option it builds (auraloss 0.4.x MultiResolutionSTFTLoss / STFTLoss,
restated: neither auraloss nor librosa is installed, so this pins the module to its own reading of them, not to them).

Per resolution: optional A-weighting FIR on both signals, torch.stft(center=True, reflect) in float64 with
``getattr(torch, window)(win)`` (float32, as auraloss builds it), M = sqrt(clamp(re^2 + im^2, eps)), optionally M <- F . M with the module's float32 mel table
(mrstft_loss.mel_filterbank, used in float64), then

    w_sc * mean_rows ||My - Mx||_F / ||My||_F  +  w_log_mag * dist(log Mx, log My)  +  w_lin_mag * dist(Mx, My)

with dist the mean of |.| (L1) or (.)^2 (L2) over rows x bins x frames; a zero weight's term is not evaluated.  The loss is the mean
over the resolutions."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F


def stft_magnitudes(s: torch.Tensor, n_fft: int, hop: int, win: int, window: str, eps: float, noise=None) -> torch.Tensor:
    """noise = (rel, generator): adds seeded complex noise of rel x (max|s| sqrt(win)) to the spectrum -- the scale of an fp32 windowed
    DFT's rounding at rel = 2^-24 (the conditioning model of tests/test_gpu_stft.py)."""
    w = getattr(torch, window)(win).double()    # auraloss' window: torch's float32 default
    spec = torch.stft(s, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
    if noise is not None:
        rel, g = noise
        scale = float(s.detach().abs().max()) * win ** 0.5 * rel
        spec = spec + scale * torch.complex(torch.randn(spec.shape, generator=g, dtype=torch.float64),
                                            torch.randn(spec.shape, generator=g, dtype=torch.float64))
    return torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=eps))


def mrstft_terms_loss(x: torch.Tensor, y: torch.Tensor, fft_sizes: Sequence[int], hop_sizes: Sequence[int], win_lengths: Sequence[int],
                      window: str = "hann_window", w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0,
                      mag_distance: str = "L1", scale: Optional[str] = None, n_bins: Optional[int] = None, sample_rate: float = 16000,
                      fir: Optional[torch.Tensor] = None, eps: float = 1e-8, noise_rel: Optional[float] = None) -> torch.Tensor:
    """x, y (batch, channels, t) float64; fir: the A-weighting taps when perceptual_weighting (None: no prefilter); noise_rel: perturb
    every spectrum at that relative scale (seeded), see ``stft_magnitudes``."""
    from vibravox_amd.torch_modules.losses.mrstft_loss import mel_filterbank

    b, c, t = x.shape
    if fir is not None:
        k = fir.double().view(1, 1, -1)
        x = F.conv1d(x.reshape(b * c, 1, t), k, padding=k.shape[-1] // 2).view(b, c, t)
        y = F.conv1d(y.reshape(b * c, 1, t), k, padding=k.shape[-1] // 2).view(b, c, t)
    dist = (lambda d: d.abs().mean()) if mag_distance == "L1" else (lambda d: (d ** 2).mean())
    noise = None if noise_rel is None else (noise_rel, torch.Generator().manual_seed(1))
    total = 0.0
    for n_fft, hop, win in zip(fft_sizes, hop_sizes, win_lengths):
        xm = stft_magnitudes(x.reshape(-1, t), n_fft, hop, win, window, eps, noise)
        ym = stft_magnitudes(y.reshape(-1, t), n_fft, hop, win, window, eps, noise)
        if scale == "mel":
            fb = torch.from_numpy(mel_filterbank(sample_rate, n_fft, n_bins)).double()
            xm, ym = torch.matmul(fb, xm), torch.matmul(fb, ym)
        term = 0.0
        if w_sc:
            term = term + w_sc * (torch.norm(ym - xm, p="fro", dim=[-1, -2]) / torch.norm(ym, p="fro", dim=[-1, -2])).mean()
        if w_log_mag:
            term = term + w_log_mag * dist(torch.log(xm) - torch.log(ym))
        if w_lin_mag:
            term = term + w_lin_mag * dist(xm - ym)
        total = total + term
    return total / len(fft_sizes)
