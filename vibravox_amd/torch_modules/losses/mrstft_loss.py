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

Beyond multi_stft.yaml, auraloss' other options are built too (0.4.x semantics restated, like everything here, and *unpinned*:
neither auraloss nor librosa is installed): ``window`` (``getattr(torch, window)(win_length)``, periodic, for hann / hamming /
blackman / bartlett / kaiser), ``w_sc`` / ``w_log_mag`` / ``w_lin_mag`` (a zero weight's term is not computed), ``mag_distance``
L1 / L2, and ``scale="mel"`` with ``n_bins`` -- the magnitudes projected by ``librosa.filters.mel(sr=sample_rate, n_fft=n_fft,
n_mels=n_bins)`` with its defaults (Slaney scale and norm, fmin 0, fmax sr/2), restated in ``mel_filterbank``.  Per resolution:
M = sqrt(clamp(re^2 + im^2, eps)) [-> F . M], then w_sc mean_rows ||My - Mx||_F / ||My||_F + w_log_mag dist(log Mx, log My) +
w_lin_mag dist(Mx, My), the mean over the resolutions.  The multi_stft.yaml configuration keeps its own kernels (stft._YamlTerms);
every other one runs stft._WeightedTerms (stft_terms.hip).  ``scale="chroma"``, ``w_phs``, ``scale_invariance`` and non-default
``reduction`` / ``output`` are not built and raise NotImplementedError.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Optional, Sequence

import numpy as np
import torch

from ... import ops, stft


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


#: the torch window functions auraloss' ``get_window(window, win_length)`` reaches that are built (periodic, torch's defaults)
WINDOWS = ("hann_window", "hamming_window", "blackman_window", "bartlett_window", "kaiser_window")


def window_samples(window: str, win: int) -> torch.Tensor:
    """float64 ``getattr(torch, window)(win)``: periodic, kaiser at torch's default beta 12."""
    if window not in WINDOWS:
        raise NotImplementedError(f"window {window!r} is not built; one of {', '.join(WINDOWS)}")
    return getattr(torch, window)(win, dtype=torch.float64)


def window_foldable(window: str, win: int) -> bool:
    """Whether the folded STFT forms (even / odd parts about the window centre h = win/2, sample 0 dropped) compute this window's DFT:
    its float32 sample 0 is exactly 0 and w[h + m] == w[h - m] in float32 (hann, blackman, bartlett -- not hamming or kaiser)."""
    if win % 2:
        return False
    w = window_samples(window, win).to(torch.float32)
    h = win // 2
    m = torch.arange(1, h)
    return float(w[0]) == 0.0 and bool((w[h + m] == w[h - m]).all())


def windowed_dft_basis(n_fft: int, win: int, window: str = "hann_window") -> torch.Tensor:
    """(2*bins, 1, win): rows k<bins  w[j] cos(2 pi k (j+lp)/n_fft), rows bins+k  -w[j] sin(...)."""
    bins = n_fft // 2 + 1
    w = window_samples(window, win)
    lp = (n_fft - win) // 2
    n = torch.arange(win, dtype=torch.float64) + lp
    k = torch.arange(bins, dtype=torch.float64).unsqueeze(1)
    ang = 2 * math.pi * k * n / n_fft
    basis = torch.cat((torch.cos(ang) * w, -torch.sin(ang) * w), dim=0)
    return basis.to(torch.float32).unsqueeze(1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# mel filterbank: librosa.filters.mel(sr, n_fft, n_mels) with its defaults (fmin 0, fmax sr/2, htk False, norm "slaney"), restated
# ------------------------------------------------------------------------------------------------------------------------------
_MEL_F_SP = 200.0 / 3            # Hz per mel below the break
_MEL_MIN_LOG_HZ = 1000.0         # the break: mel 15
_MEL_MIN_LOG_MEL = _MEL_MIN_LOG_HZ / _MEL_F_SP
_MEL_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney mel scale: linear at 200/3 Hz per mel below 1000 Hz (mel 15), logarithmic with step log(6.4)/27 above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / _MEL_F_SP
    log = _MEL_MIN_LOG_MEL + np.log(np.maximum(f, _MEL_MIN_LOG_HZ) / _MEL_MIN_LOG_HZ) / _MEL_LOGSTEP
    return np.where(f >= _MEL_MIN_LOG_HZ, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = _MEL_F_SP * m
    log = _MEL_MIN_LOG_HZ * np.exp(_MEL_LOGSTEP * (np.maximum(m, _MEL_MIN_LOG_MEL) - _MEL_MIN_LOG_MEL))
    return np.where(m >= _MEL_MIN_LOG_MEL, log, lin)


def mel_filterbank(sample_rate: float, n_fft: int, n_mels: int) -> np.ndarray:
    """(n_mels, n_fft//2 + 1) float32 Slaney-normalised triangles: band edges n_mels + 2 points evenly spaced in mel over [0, sr/2],
    bin frequencies rfftfreq(n_fft, 1/sr), triangle max(0, min(lower, upper)) stored into a float32 table and scaled in place by
    2 / (f[m+2] - f[m]) -- the ramps in float64, each of the two steps rounded to float32 as librosa's float32 ``weights`` array does.
    Warns as librosa does when a filter comes out empty."""
    sr = float(sample_rate)
    weights = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    if not np.all((mel_f[:-2] == 0) | (weights.max(axis=1) > 0)):
        warnings.warn("Empty filters detected in mel frequency basis. Some channels will produce empty responses. Try increasing your "
                      "sampling rate (and fmax) or reducing n_mels.", stacklevel=2)
    return weights


def mel_bands(fb: np.ndarray):
    """The banded forms of a filterbank the kernels read: forward, filter m covers bins [lo[m], lo[m] + off[m+1] - off[m]) with
    weights w[off[m] ..]; adjoint, bin k's <= 2 (filter, weight) pairs (bin_m[k, q] = -1: none).  Raises if a bin lies in more than
    two filters' ranges (not a triangle bank)."""
    n_mels, bins = fb.shape
    lo, off, w = np.zeros(n_mels, np.int32), np.zeros(n_mels + 1, np.int32), []
    bin_m, bin_w = np.full((bins, 2), -1, np.int32), np.zeros((bins, 2), np.float32)
    used = np.zeros(bins, np.int32)
    for m in range(n_mels):
        nz = np.flatnonzero(fb[m] != 0)
        a, b = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        lo[m], off[m + 1] = a, off[m] + (b - a)
        w.append(fb[m, a:b])
        for k in range(a, b):
            if used[k] == 2:
                raise ValueError(f"bin {k} lies in more than two mel filters")
            bin_m[k, used[k]], bin_w[k, used[k]] = m, fb[m, k]
            used[k] += 1
    w = np.concatenate(w) if off[-1] else np.zeros(1, np.float32)
    return (torch.from_numpy(lo), torch.from_numpy(off), torch.from_numpy(w.astype(np.float32)), torch.from_numpy(bin_m.reshape(-1)),
            torch.from_numpy(bin_w.reshape(-1)))


#: auraloss STFTLoss keyword arguments MultiResolutionSTFTLoss forwards (**kwargs), with the values that are built
_STFT_KWARGS = {"reduction": ("mean",), "mag_distance": ("L1", "L2"), "output": ("loss",), "device": None}


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
        for key, value in kwargs.items():
            if key not in _STFT_KWARGS:
                raise TypeError(f"MultiResolutionSTFTLoss got an unexpected keyword argument {key!r}")
            if _STFT_KWARGS[key] is not None and value not in _STFT_KWARGS[key]:
                if key == "mag_distance":
                    raise ValueError(f"Invalid distance: '{value}'.")
                raise NotImplementedError(f"{key}={value!r} is not built (only {_STFT_KWARGS[key][0]!r})")
        mag_distance = kwargs.get("mag_distance", "L1")
        if window not in WINDOWS:
            raise NotImplementedError(f"window {window!r} is not built; one of {', '.join(WINDOWS)}")
        if w_phs:
            raise NotImplementedError("the phase term (w_phs != 0) is not built")
        if scale_invariance:
            raise NotImplementedError("scale_invariance=True is not built")
        if scale not in (None, "mel"):
            raise NotImplementedError(f"scale={scale!r} is not built (only None and 'mel')")
        if not (w_sc or w_log_mag or w_lin_mag):
            raise NotImplementedError("at least one of w_sc, w_log_mag, w_lin_mag must be non-zero")
        if scale == "mel":
            if sample_rate is None:
                raise ValueError("`sample_rate` must be supplied when `scale = 'mel'`.")
            if n_bins is None or not 0 < n_bins <= min(fft_sizes):
                raise ValueError(f"scale='mel' needs 0 < n_bins <= n_fft of every resolution, got n_bins={n_bins}")
        if perceptual_weighting and sample_rate is None:
            raise ValueError("`sample_rate` must be supplied when `perceptual_weighting = True`.")
        #: the multi_stft.yaml configuration (hann, SC + L1 log-magnitude, no scale) keeps stft._YamlTerms; every other runs stft._WeightedTerms
        self.default_terms = (window == "hann_window" and w_sc == 1.0 and w_log_mag == 1.0 and not w_lin_mag and mag_distance == "L1"
                              and scale is None)
        if not self.default_terms and len(fft_sizes) > 16:
            raise NotImplementedError("at most 16 resolutions outside the default configuration")
        self.window, self.scale, self.n_bins, self.mag_distance = window, scale, n_bins, mag_distance
        self.w_sc, self.w_log_mag, self.w_lin_mag = float(w_sc), float(w_log_mag), float(w_lin_mag)
        self.eps = eps
        self.fft_sizes, self.hop_sizes, self.win_lengths = tuple(fft_sizes), tuple(hop_sizes), tuple(win_lengths)
        self.register_buffer("fir", a_weighting_taps(sample_rate) if perceptual_weighting else None, persistent=False)
        self._plans = None
        for i, (n_fft, win) in enumerate(zip(self.fft_sizes, self.win_lengths)):
            basis = windowed_dft_basis(n_fft, win, window).squeeze(1)              # (2*bins, win)
            self.register_buffer(f"basis_{i}", basis.unsqueeze(-1).contiguous(), persistent=False)            # (2*bins, win, 1)
            self.register_buffer(f"basis_t_{i}", basis.t().contiguous().unsqueeze(-1), persistent=False)      # (win, 2*bins, 1)
            if scale == "mel":
                fb = mel_filterbank(sample_rate, n_fft, n_bins)
                self.register_buffer(f"fb_{i}", torch.from_numpy(fb), persistent=False)                      # (n_bins, bins)
                for name, t in zip(("lo", "off", "w", "bin_m", "bin_w"), mel_bands(fb)):
                    self.register_buffer(f"mel_{name}_{i}", t, persistent=False)

    def _build_plans(self):
        plans = []
        for i, (n_fft, hop, win) in enumerate(zip(self.fft_sizes, self.hop_sizes, self.win_lengths)):
            mel = None
            if self.scale == "mel":
                mel = (self.n_bins,) + tuple(getattr(self, f"mel_{name}_{i}") for name in ("lo", "off", "w", "bin_m", "bin_w"))
            plans.append(stft.StftPlan.build(n_fft, hop, win, getattr(self, f"basis_{i}"), getattr(self, f"basis_t_{i}"),
                                             foldable=window_foldable(self.window, win), mel=mel))
        return plans

    #: arithmetic of the windowed-DFT contractions: "folded" (exact fp32 on the even / odd parts of the frames: half the products
    #: of "dense"), "dense" (one win-channel GEMM), "bf16x3" (folded, hi / lo bf16 operand splits on the bf16 MFMA, ~2^-17
    #: relative per product), "folded_x6" / "folded_x3" (folded, the tap-conv's split bf16 operands: three pieces per operand =
    #: fp32-grade products at 6/16 of the fp32 MFMA's cost / two pieces, ~2^-17 -- EBENLightningModule.stft_math); a window the
    #: folded forms cannot fold (hamming, kaiser) takes "dense" in every mode.  The mel projection and the terms run in fp32 always.
    stft_math: str = os.environ.get("EBEN_STFT_MATH", "folded")

    def _current_plans(self, x: torch.Tensor):
        """The plans on x's device and the buffers' current storage, set to ``stft_math``."""
        if self.stft_math not in ("folded", "dense", "bf16x3", "folded_x3", "folded_x6"):
            raise ValueError(f"unknown STFT math {self.stft_math!r}")
        if self._plans is None or self._plans[0].basis_f.device != x.device or self._plans[0].basis_f.data_ptr() != self.basis_0.data_ptr():
            self._plans = self._build_plans()
        for p in self._plans:
            p.math = self.stft_math
        return self._plans

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        plans = self._current_plans(x)
        if self.default_terms:
            return stft.mrstft(x, y, self.fir, plans, self.eps)
        return stft.mrstft_terms(x, y, self.fir, plans, self.eps, (self.w_sc, self.w_log_mag, self.w_lin_mag), self.mag_distance == "L2")

    def ragged_sums(self, x: torch.Tensor, y: torch.Tensor, lengths: Sequence[int]):
        """The per-row sums behind ``forward_ragged``: per resolution (sums (rows, 3), frames_of_row (rows,) int32 on the device, bins),
        what ``ops.clip_losses`` takes.  Checks everything ``forward_ragged`` refuses before anything runs."""
        plans = self._current_plans(x)   # host work only: nothing is launched before the checks below
        if not (self.w_sc == 1.0 and self.w_log_mag == 1.0 and not self.w_lin_mag and self.mag_distance == "L1" and self.scale is None):
            raise NotImplementedError(
                f"forward_ragged is built for the multi_stft.yaml term set (w_sc = w_log_mag = 1, L1, no scale; any window), not for w_sc="
                f"{self.w_sc}, w_log_mag={self.w_log_mag}, w_lin_mag={self.w_lin_mag}, mag_distance={self.mag_distance!r}, scale={self.scale!r}")
        if len(self.fft_sizes) > 8:
            raise NotImplementedError("forward_ragged: at most 8 resolutions")
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            raise RuntimeError("MultiResolutionSTFTLoss.forward_ragged has no backward; its inputs must not require grad")
        if x.dim() != 3 or x.shape[1] != 1 or x.shape != y.shape or x.dtype is not torch.float32 or y.dtype is not torch.float32:
            raise ValueError(f"forward_ragged: expected two float32 (rows, 1, l_buf) buffers, got {tuple(x.shape)} and {tuple(y.shape)}")
        rows, _, l_buf = x.shape
        lengths = [int(t) for t in lengths]
        if len(lengths) != rows:
            raise ValueError(f"forward_ragged: {len(lengths)} lengths for {rows} rows")
        pad = max(p.pad for p in plans)
        for r, t in enumerate(lengths):
            if t < pad + 1:
                raise ValueError(f"clip {r} ({t} samples) is too short: the STFT reflect-pads {pad} samples")
            if t > l_buf or (t < l_buf and t + pad > l_buf):
                raise ValueError(f"clip {r} ({t} samples) needs {pad} samples of slack behind it in a buffer of {l_buf}, or none at all")
        with torch.no_grad():
            host = torch.tensor([lengths + lengths] + [[p.frames(t) for t in lengths] * 2 for p in plans], dtype=torch.int32)
            table = host.to(x.device, non_blocking=True)   # the one upload: row lengths, then every resolution's frames per row
            frames = [table[1 + i, :rows] for i in range(len(plans))]
            fill = pad if any(t < l_buf for t in lengths) else 0
            sums = stft.mrstft_sums_rows(x.contiguous(), y.contiguous(), table[0], frames, self.fir, plans, self.eps, fill)
        return [(s, f, p.bins) for s, f, p in zip(sums, frames, plans)]

    def forward_ragged(self, x: torch.Tensor, y: torch.Tensor, lengths: Sequence[int]) -> torch.Tensor:
        """(rows,) float32: row r is ``forward(x[r:r+1, :, :lengths[r]], y[r:r+1, :, :lengths[r]])``, all rows in one pass.  ``x`` and ``y``
        are (rows, 1, l_buf) and zero behind every row; a row shorter than the buffer needs the largest reflect pad of slack behind it.
        Inference only: no gradient is returned and inputs that require grad are refused.  Built for the multi_stft.yaml term set (SC +
        log-magnitude L1, linear scale) at any resolutions and ``perceptual_weighting``; every other term set raises NotImplementedError."""
        terms = self.ragged_sums(x, y, lengths)
        with torch.no_grad():
            return ops.clip_losses(x.shape[0], x.device, stft=terms)[0]
