"""Speech-quality validation metrics on the device (the SI-SDR and STOI of ``base_se.py``'s ``common_eval_logging``).

* ``si_sdr(preds, target)``: ``torchmetrics.functional.scale_invariant_signal_distortion_ratio(preds, target, zero_mean=False)``,
  one HIP launch (``eben_si_sdr``) with fp64 sums and a second pass for the noise energy.
* ``stoi(preds, target, fs)``: ``torchmetrics.functional.short_time_objective_intelligibility(preds, target, fs)``, i.e. pystoi
  0.4.x ``stoi(target, preds, fs, extended=False)`` per clip, restated as four HIP launches (``eben_stoi``) over the whole batch:
  resampling to 10 kHz, silence removal, third-octave band envelopes, segment correlations.  pystoi is not installed here,
  so its conventions are restated from its published source (parity unpinned, like the auraloss / torchaudio restatements).

Beyond those two, for scoring a bandwidth-extension model: ``si_sdr(..., zero_mean=True)`` / ``si_snr`` and ``snr`` (torchmetrics'
``scale_invariant_signal_noise_ratio`` and ``signal_noise_ratio``; ``eben_signal_ratio``), ``stoi(..., extended=True)`` (ESTOI: pystoi's
row- and column-normalised tail on the same envelopes, without its ``EPS * randn`` dither; ``eben_estoi``) and ``lsd`` (log-spectral
distance over the whole band or over ``band_hz`` ranges; ``eben_lsd``).  ``sdr`` is the BSS-eval signal-to-distortion ratio (torchmetrics'
``signal_distortion_ratio``, direct solve: up to 512 lags of both correlations and a Toeplitz solve per row, float64; ``eben_sdr``), restated
from torchmetrics 1.x without the package at hand (parity unpinned).

``speech_measures`` (and ``seg_snr``, ``fw_seg_snr``, ``llr``, ``cepstral_distance`` on top of it) are the classic frame-based objective
measures of Hu & Loizou (2008), the ``pysepm`` set without WSS and the PESQ composites: segmental SNR, frequency-weighted segmental SNR,
the LPC log-likelihood ratio and the LPC cepstral distance over 30 ms frames (``eben_speech_measures``; LPC and sums float64, the
transform float32).  pysepm is not installed here either: the definitions are restated from the published code (parity unpinned).

``integrated_loudness`` / ``loudness_gain`` measure one signal's level as a listener perceives it: the integrated loudness of ITU-R
BS.1770-4 (K-weighting, gated 400 ms blocks; ``eben_loudness``), its sample peak and the gain to a target level under a peak ceiling --
what ``inference.enhance_to_pcm(loudness=)`` normalises its files with.  Restated from the recommendation (parity unpinned).

All take ``(..., T)`` float tensors on a HIP device and return ``(...)`` float32 on that device, with torchmetrics' argument
order (preds first).  There is no CPU path: a CPU tensor raises ``EbenError`` (the float64 restatement used to check these
kernels is test code under ``tests/``).

``ScaleInvariantSignalDistortionRatio`` and ``ShortTimeObjectiveIntelligibility`` mirror the torchmetrics classes
(``update`` / ``compute`` / ``reset``; ``forward`` returns the batch mean and accumulates).  Their running sum and count
live on the device as plain attributes, not buffers, so a module that holds them keeps its ``state_dict`` keys.

Rows of different lengths: every entry point takes ``lengths``, one value per row of the flattened leading dimensions.  Row ``r`` is
then the signal ``[..., :lengths[r]]`` -- what lies behind it is never read -- and its value has the bits of the call on that row
alone (``eben_si_sdr_ragged`` / ``eben_stoi_ragged``: the same kernels with a length per row; the newer entries take a nullable table).  A sequence of ints or a CPU integer
tensor is validated (``ValueError`` naming the row) and uploaded; an ``int32`` tensor on the signals' device is used as it is, without
synchronisation, and a value outside ``[1, T]`` in it makes that row NaN (for ``lsd`` also a value ``<= n_fft // 2``: such a row cannot
be reflect-padded).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import EbenError, check, load, ptr, stream

STOI_FS = 10000


Lengths = Union[None, Sequence[int], torch.Tensor]


def _host_lengths(lengths, rows: int, t: int, what: str, least: int = 1) -> Optional[torch.Tensor]:
    """A host-side ``lengths`` checked and as a CPU int32 tensor; None for a device tensor (``_device_lengths`` takes those)."""
    if torch.is_tensor(lengths):
        if lengths.is_cuda:
            return None
        if lengths.dtype in (torch.bool,) or lengths.is_floating_point() or lengths.is_complex():
            raise ValueError(f"{what}: lengths must be integers, got a {lengths.dtype} tensor")
        values = [int(v) for v in lengths.reshape(-1).tolist()]
    else:
        values = []
        for r, v in enumerate(lengths):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{what}: lengths[{r}] = {v!r} is not an integer")
            values.append(int(v))
    if len(values) != rows:
        raise ValueError(f"{what}: {len(values)} lengths for {rows} rows")
    for r, v in enumerate(values):
        if not least <= v <= t:
            raise ValueError(f"{what}: row {r} has length {v}, outside [{least}, {t}]")
    return torch.tensor(values, dtype=torch.int32)


def _device_lengths(lengths: torch.Tensor, rows: int, lead: Tuple[int, ...], dev: torch.device, what: str) -> torch.Tensor:
    """A ``lengths`` that already lives on a device: taken as it is (nobody reads its values on the host)."""
    if lengths.device != dev:
        raise ValueError(f"{what}: lengths is on '{lengths.device}', the signals are on '{dev}'")
    if lengths.dtype is not torch.int32:
        raise ValueError(f"{what}: a device lengths tensor must be int32, got {lengths.dtype}")
    if tuple(lengths.shape) not in ((rows,), lead):
        raise ValueError(f"{what}: a device lengths tensor must have shape {(rows,)} or {lead}, got {tuple(lengths.shape)}")
    return lengths.contiguous().reshape(-1)


def _rows(preds: torch.Tensor, target: torch.Tensor, what: str, lengths: Lengths = None, least: int = 1):
    """(preds, target) as contiguous float32 (rows, T), the leading shape and ``lengths`` as a device int32 (rows,) tensor or None."""
    if preds.shape != target.shape:
        raise ValueError(f"{what}: preds and target must have the same shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if preds.dim() < 1 or preds.shape[-1] < 1:
        raise ValueError(f"{what}: expected (..., time) signals, got shape {tuple(preds.shape)}")
    lead = tuple(preds.shape[:-1])
    t = preds.shape[-1]
    rows = math.prod(lead)
    host = _host_lengths(lengths, rows, t, what, least) if lengths is not None else None   # refused before anything touches a device
    for x in (preds, target):
        if not x.is_cuda:
            raise EbenError(f"{what} runs only on an MI355X HIP device (got a tensor on '{x.device}'); there is no CPU path")
    p2 = preds.detach().to(torch.float32).contiguous().reshape(-1, t)
    g2 = target.detach().to(torch.float32).contiguous().reshape(-1, t)
    if lengths is None:
        return p2, g2, lead, None
    if host is not None:
        return p2, g2, lead, host.to(p2.device, non_blocking=True)
    return p2, g2, lead, _device_lengths(lengths, rows, lead, p2.device, what)


def _lens_ptr(lens: Optional[torch.Tensor]) -> Optional[int]:
    return None if lens is None else lens.data_ptr()


RATIO_SI_SDR, RATIO_SNR = 0, 1   # include/eben_hip.h EBEN_RATIO_*


def _signal_ratio(preds, target, lengths, kind: int, zero_mean: bool, what: str) -> torch.Tensor:
    p2, g2, lead, lens = _rows(preds, target, what, lengths)
    out = torch.empty(p2.shape[0], dtype=torch.float32, device=p2.device)
    check(load().eben_signal_ratio(ptr(p2), ptr(g2), p2.shape[0], p2.shape[1], _lens_ptr(lens), kind, int(bool(zero_mean)), ptr(out), stream()), what)
    return out.reshape(lead)


def si_sdr(preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None, zero_mean: bool = False) -> torch.Tensor:
    """Scale-invariant SDR in dB per signal: (..., T) -> (...); with ``lengths``, of ``[..., :lengths[r]]`` per row.  ``zero_mean``
    subtracts each signal's mean over its own length first."""
    if zero_mean:
        return _signal_ratio(preds, target, lengths, RATIO_SI_SDR, True, "si_sdr")
    p2, g2, lead, lens = _rows(preds, target, "si_sdr", lengths)
    out = torch.empty(p2.shape[0], dtype=torch.float32, device=p2.device)
    if lens is None:
        check(load().eben_si_sdr(ptr(p2), ptr(g2), p2.shape[0], p2.shape[1], ptr(out), stream()), "si_sdr")
    else:
        check(load().eben_si_sdr_ragged(ptr(p2), ptr(g2), p2.shape[0], p2.shape[1], lens.data_ptr(), ptr(out), stream()), "si_sdr_ragged")
    return out.reshape(lead)


def si_snr(preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None) -> torch.Tensor:
    """torchmetrics ``scale_invariant_signal_noise_ratio``: SI-SDR of the zero-mean signals."""
    return _signal_ratio(preds, target, lengths, RATIO_SI_SDR, True, "si_snr")


def snr(preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None, zero_mean: bool = False) -> torch.Tensor:
    """torchmetrics ``signal_noise_ratio`` in dB per signal: 10 log10((sum t^2 + eps) / (sum (t - p)^2 + eps))."""
    return _signal_ratio(preds, target, lengths, RATIO_SNR, zero_mean, "snr")


SDR_SEGMENT = 8192      # samples of a row per workgroup of the correlation kernel (csrc/sdr.hip kSegment)
SDR_MAX_FILTER = 512    # taps of the distortion filter, at most


def sdr_filter_length(value, what: str) -> int:
    """``value`` as the taps of the distortion filter; ``ValueError`` unless it is an integer in [1, SDR_MAX_FILTER]."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or int(value) != value \
            or not 1 <= int(value) <= SDR_MAX_FILTER:
        raise ValueError(f"{what} must be an integer in [1, {SDR_MAX_FILTER}], got {value!r}")
    return int(value)


def sdr(preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None, filter_length: int = 512, zero_mean: bool = False,
        load_diag: Optional[float] = None, use_cg_iter: Optional[int] = None) -> torch.Tensor:
    """BSS-eval signal-to-distortion ratio in dB per signal, torchmetrics ``signal_distortion_ratio`` (direct solve): the estimate is
    allowed a ``filter_length``-tap distortion filter before what is left counts as distortion.  (..., T) -> (...); with ``lengths``, of
    ``[..., :lengths[r]]`` per row, each value the bits of the call on that row alone.  float64 throughout (``eben_sdr``: ragged
    correlations and a Levinson solve per row); there is no eps, so a silent target gives NaN.  The conjugate-gradient branch
    (``use_cg_iter``) is not built."""
    if use_cg_iter is not None:
        raise NotImplementedError("sdr: the conjugate-gradient solver (use_cg_iter) is not built; pass None for the direct solve")
    taps = sdr_filter_length(filter_length, "sdr: filter_length")
    diag = 0.0 if load_diag is None else float(load_diag)   # the ABI's 0.0 adds nothing
    if diag != diag:
        raise ValueError("sdr: load_diag is NaN")
    p2, g2, lead, lens = _rows(preds, target, "sdr", lengths)
    rows, t = p2.shape
    lib = load()
    ws = torch.empty(lib.eben_sdr_workspace(rows, t, taps), dtype=torch.uint8, device=p2.device)
    out = torch.empty(rows, dtype=torch.float32, device=p2.device)
    check(lib.eben_sdr(ptr(p2), ptr(g2), rows, t, _lens_ptr(lens), taps, int(bool(zero_mean)), diag, ws.data_ptr(), ptr(out),
                       stream()), "sdr")
    return out.reshape(lead)


def stoi_resample_table(fs: int) -> Tuple[np.ndarray, int, int]:
    """(up * h as float64, up, down) of pystoi's ``resample_oct(x, 10000, fs)``: a Kaiser-windowed sinc (60 dB rejection,
    roll-off a tenth of the cut-off) normalised to unit sum; resample_poly scales an array window by ``up``."""
    g = math.gcd(STOI_FS, int(fs))
    up, down = STOI_FS // g, int(fs) // g
    cutoff = 1.0 / (2 * max(up, down))
    rejection_db = 60.0
    half = math.ceil((rejection_db - 8) / (28.714 * cutoff / 10))
    n = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (rejection_db - 8.7)) * (2 * up * cutoff * np.sinc(2 * cutoff * n))
    return up * h / h.sum(), up, down


_tables: Dict[Tuple[int, torch.device], torch.Tensor] = {}


def _stoi_table(fs: int, dev: torch.device):
    if fs == STOI_FS:
        return None, 0
    key = (fs, dev)
    if key not in _tables:
        _tables[key] = torch.from_numpy(stoi_resample_table(fs)[0]).to(torch.float32).to(dev)
    return _tables[key], _tables[key].numel()


def _estoi(preds, target, fs: int, lengths: Lengths, with_classic: bool, what: str):
    """ESTOI per row, and with ``with_classic`` also classic STOI from the same envelopes (one front end, two tails)."""
    p2, g2, lead, lens = _rows(preds, target, what, lengths)
    fs = int(fs)
    if fs <= 0:
        raise ValueError(f"{what}: fs must be positive, got {fs}")
    rows, t = p2.shape
    dev = p2.device
    lib = load()
    table, taps = _stoi_table(fs, dev)
    ws_bytes = lib.eben_estoi_workspace(rows, t, fs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((2 if with_classic else 1, rows), dtype=torch.float32, device=dev)
    classic = out[1].data_ptr() if with_classic else None
    check(lib.eben_estoi(ptr(g2), ptr(p2), rows, t, _lens_ptr(lens), fs, ptr(table), taps, ws.data_ptr(), ws_bytes, out[0].data_ptr(), classic,
                         stream()), what)
    return (out[0].reshape(lead), out[1].reshape(lead)) if with_classic else out[0].reshape(lead)


def stoi_and_estoi(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(classic STOI, ESTOI) per signal from one run of the resampling, silence-removal and band-envelope kernels; each has the bits of
    its own ``stoi`` call."""
    estoi, classic = _estoi(preds, target, fs, lengths, True, "stoi_and_estoi")
    return classic, estoi


def stoi(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None, extended: bool = False) -> torch.Tensor:
    """STOI per signal (target = clean reference): (..., T) -> (...); with ``lengths``, of ``[..., :lengths[r]]`` per row.  ``extended``
    selects ESTOI."""
    if extended:
        return _estoi(preds, target, fs, lengths, False, "estoi")
    p2, g2, lead, lens = _rows(preds, target, "stoi", lengths)
    fs = int(fs)
    if fs <= 0:
        raise ValueError(f"stoi: fs must be positive, got {fs}")
    rows, t = p2.shape
    dev = p2.device
    lib = load()
    table, taps = _stoi_table(fs, dev)
    ws_bytes = lib.eben_stoi_workspace(rows, t, fs) if lens is None else lib.eben_stoi_ragged_workspace(rows, t, fs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(rows, dtype=torch.float32, device=dev)
    if lens is None:
        check(lib.eben_stoi(ptr(g2), ptr(p2), rows, t, fs, ptr(table), taps, ws.data_ptr(), ws_bytes, ptr(out), stream()), "stoi")
    else:
        check(lib.eben_stoi_ragged(ptr(g2), ptr(p2), rows, t, lens.data_ptr(), fs, ptr(table), taps, ws.data_ptr(), ws_bytes, ptr(out),
                                   stream()), "stoi_ragged")
    return out.reshape(lead)


LSD_MAX_BANDS = 4   # bands per eben_lsd launch


def lsd_band_bins(band_hz, fs: int, n_fft: int) -> Tuple[int, int]:
    """The bin range [k_lo, k_hi) of ``band_hz = (lo, hi)``: the bins k of the n_fft // 2 + 1 with lo <= k fs / n_fft < hi, in exact
    integer arithmetic for integer edges.  None is the full band, Nyquist bin included (which no finite ``hi <= fs / 2`` reaches)."""
    nb = n_fft // 2 + 1
    if band_hz is None:
        return 0, nb
    lo, hi = band_hz
    if not 0 <= lo < hi:
        raise ValueError(f"lsd: band_hz = ({lo}, {hi}) needs 0 <= lo < hi")

    def first_at_or_above(hz) -> int:   # min k with k * fs >= hz * n_fft
        if int(hz) == hz:
            return -(-int(hz) * n_fft // fs)
        return math.ceil(hz * n_fft / fs)

    k_lo, k_hi = min(first_at_or_above(lo), nb), min(first_at_or_above(hi), nb)
    if k_lo >= k_hi:
        raise ValueError(f"lsd: band_hz = ({lo}, {hi}) holds no bin of a {n_fft}-point transform at {fs} Hz")
    return k_lo, k_hi


def _is_band(b) -> bool:
    return b is None or (len(b) == 2 and not isinstance(b[0], (tuple, list)) and b[0] is not None and not isinstance(b[1], (tuple, list)))


def lsd(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None, n_fft: int = 2048, hop: int = 512,
        band_hz=None) -> torch.Tensor:
    """Log-spectral distance per signal: with P(s) = clamp(|stft(s, n_fft, hop, hann, center, reflect)|^2, min=1e-8), the mean over the
    signal's own 1 + len // hop frames of sqrt(mean over the band's bins of (log10 P(preds) - log10 P(target))^2).  ``band_hz``: None
    (all n_fft // 2 + 1 bins), ``(lo, hi)`` in Hz, or a list of up to four of either, which returns ``(nbands, ...)``."""
    fs, n_fft, hop = int(fs), int(n_fft), int(hop)
    if fs <= 0:
        raise ValueError(f"lsd: fs must be positive, got {fs}")
    if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"lsd: n_fft must be a power of two in [256, 4096], got {n_fft}")
    if not 1 <= hop <= n_fft:
        raise ValueError(f"lsd: hop must lie in [1, n_fft = {n_fft}], got {hop}")
    many = not _is_band(band_hz)
    bands = list(band_hz) if many else [band_hz]
    if not 1 <= len(bands) <= LSD_MAX_BANDS:
        raise ValueError(f"lsd: {len(bands)} bands, one call takes 1 to {LSD_MAX_BANDS}")
    bins = [lsd_band_bins(b, fs, n_fft) for b in bands]
    if preds.dim() >= 1 and preds.shape[-1] <= n_fft // 2:
        raise ValueError(f"lsd: signals of {preds.shape[-1]} samples cannot be reflect-padded by n_fft // 2 = {n_fft // 2}")
    p2, g2, lead, lens = _rows(preds, target, "lsd", lengths, least=n_fft // 2 + 1)
    rows, t = p2.shape
    lib = load()
    import ctypes

    lo = (ctypes.c_int * len(bins))(*[b[0] for b in bins])
    hi = (ctypes.c_int * len(bins))(*[b[1] for b in bins])
    ws_bytes = lib.eben_lsd_workspace(rows, t, n_fft, hop, len(bins))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p2.device)
    out = torch.empty((len(bins), rows), dtype=torch.float32, device=p2.device)
    check(lib.eben_lsd(ptr(p2), ptr(g2), rows, t, _lens_ptr(lens), n_fft, hop, lo, hi, len(bins), ws.data_ptr(), ws_bytes, ptr(out), stream()), "lsd")
    return out.reshape((len(bins),) + lead) if many else out[0].reshape(lead)


#: the frame-based measures of ``speech_measures`` and their bits in ``eben_speech_measures`` (include/eben_hip.h EBEN_MEASURE_*)
SPEECH_MEASURES = {"seg_snr": 1, "fw_seg_snr": 2, "llr": 4, "cd": 8}
MEASURES_TILE_FRAMES = 16   # frames of a row per workgroup of the frame kernels (csrc/speech_measures.hip kTileFrames)


def measures_geometry(fs) -> Tuple[int, int, int, int]:
    """``(W, S, P, n_fft)`` of the frame-based measures at ``fs``: 30 ms frames, a quarter of that between them, the LPC order and the
    transform of ``fw_seg_snr``.  ``ValueError`` unless ``fs`` is 16000 or 8000."""
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or int(fs) not in (16000, 8000):
        raise ValueError(f"speech measures: fs must be 16000 or 8000, got {fs!r}")
    w = int(math.floor(0.030 * int(fs) + 0.5))
    return w, w // 4, 16 if int(fs) == 16000 else 10, 1 << math.ceil(math.log2(2 * w))


def measures_window(fs: int) -> np.ndarray:
    """The analysis window in float64: w[n] = 0.5 (1 - cos(2 pi (n + 1) / (W + 1))), n = 0 .. W - 1."""
    w = measures_geometry(fs)[0]
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, w + 1) / (w + 1)))


_windows: Dict[Tuple[int, torch.device], torch.Tensor] = {}


def _measures_window(fs: int, dev: torch.device) -> torch.Tensor:
    """The window on ``dev``, uploaded once per (fs, device) and kept for the life of the module, like ``_stoi_table``'s tables.  The
    upload is a blocking copy from pageable host memory (the one host wait of a (fs, device)'s first call): it has finished when
    ``.to`` returns, so launches on any stream may read the tensor without an event."""
    key = (fs, dev)
    if key not in _windows:
        _windows[key] = torch.from_numpy(measures_window(fs)).to(dev)
    return _windows[key]


def speech_measures(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None,
                    which: Sequence[str] = ("seg_snr", "fw_seg_snr", "llr", "cd")) -> Dict[str, torch.Tensor]:
    """The frame-based objective measures of Hu & Loizou (2008), the non-WSS, non-PESQ part of the ``pysepm`` set, per signal (preds =
    processed, target = clean): ``{"seg_snr": segmental SNR in dB, "fw_seg_snr": frequency-weighted segmental SNR in dB, "llr": LPC
    log-likelihood ratio, "cd": LPC cepstral distance}``, the keys of ``which`` in its order.  (..., T) -> (...) each; with ``lengths``, of
    ``[..., :lengths[r]]`` per row, each value the bits of the call on that row alone.

    Frames of W = 30 ms every S = W / 4 under ``measures_window``, (N - W) // S of them (one fewer than fit, as in the published code);
    ``fs`` is 16000 or 8000; a row needs W + S samples (a shorter one in a device ``lengths`` is NaN).  ``llr`` and ``cd`` are the means of
    the smallest 95 % of the frame values, ``fw_seg_snr``, ``llr`` and ``cd`` leave out frames in which either signal is all zero (NaN
    when none is left).  The definitions are written out at ``eben_speech_measures`` in ``include/eben_hip.h``; pysepm is not installed
    here, so they are restated from the published code (parity unpinned).  One launch sequence for whatever is asked
    (``eben_speech_measures``): the spectral kernel runs only for ``fw_seg_snr``, the LPC work only for ``llr`` or ``cd``; LPC, segmental
    sums and all means in float64, the transform in float32."""
    names = list(which)
    if not names:
        raise ValueError("speech_measures: no measure requested")
    for name in names:
        if name not in SPEECH_MEASURES:
            raise ValueError(f"speech_measures: unknown measure {name!r}; known: {', '.join(SPEECH_MEASURES)}")
    if len(set(names)) != len(names):
        raise ValueError(f"speech_measures: a measure is named twice in {names}")
    w, s, _, _ = measures_geometry(fs)
    fs = int(fs)
    if preds.dim() >= 1 and preds.shape == target.shape and preds.shape[-1] < w + s:
        raise ValueError(f"speech_measures: signals of {preds.shape[-1]} samples hold no frame at {fs} Hz ({w + s} at least)")
    p2, g2, lead, lens = _rows(preds, target, "speech_measures", lengths, least=w + s)
    rows, t = p2.shape
    mask = sum(SPEECH_MEASURES[name] for name in names)
    lib = load()
    ws = torch.empty(lib.eben_speech_measures_workspace(rows, t, fs, mask), dtype=torch.uint8, device=p2.device)
    out = torch.empty((len(names), rows), dtype=torch.float32, device=p2.device)
    check(lib.eben_speech_measures(ptr(p2), ptr(g2), rows, t, _lens_ptr(lens), fs, mask, _measures_window(fs, p2.device).data_ptr(),
                                   ws.data_ptr(), ptr(out), stream()), "speech_measures")
    planes = sorted(names, key=SPEECH_MEASURES.get)   # the planes come in bit order
    return {name: out[planes.index(name)].reshape(lead) for name in names}


def seg_snr(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None) -> torch.Tensor:
    """Segmental SNR in dB per signal (``speech_measures``): the mean of the frames' SNR, each clipped to [-10, 35] dB."""
    return speech_measures(preds, target, fs, lengths, ("seg_snr",))["seg_snr"]


def fw_seg_snr(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None) -> torch.Tensor:
    """Frequency-weighted segmental SNR in dB per signal (``speech_measures``): 25 critical bands, weights (clean band magnitude)^0.2."""
    return speech_measures(preds, target, fs, lengths, ("fw_seg_snr",))["fw_seg_snr"]


def llr(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None) -> torch.Tensor:
    """LPC log-likelihood ratio per signal (``speech_measures``): frame values capped at 2, the mean of the smallest 95 %."""
    return speech_measures(preds, target, fs, lengths, ("llr",))["llr"]


def cepstral_distance(preds: torch.Tensor, target: torch.Tensor, fs: int, lengths: Lengths = None) -> torch.Tensor:
    """LPC cepstral distance per signal (``speech_measures``): frame values capped at 10, the mean of the smallest 95 %."""
    return speech_measures(preds, target, fs, lengths, ("cd",))["cd"]


def _loudness_fs(fs, what: str) -> int:
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or int(fs) <= 0 or int(fs) % 10:
        raise ValueError(f"{what}: fs must be a positive multiple of 10 (the 100 ms hop is a whole number of samples), got {fs!r}")
    return int(fs)


def k_weighting_coefficients(fs) -> Tuple[np.ndarray, np.ndarray]:
    """The two second-order sections of the K-weighting of ITU-R BS.1770-4 at ``fs``, in float64 on the host: ``(shelf, highpass)``, each
    ``[b0, b1, b2, a1, a2]`` with ``a0 = 1`` (the formulas stand at ``eben_loudness`` in ``include/eben_hip.h``; at 48 kHz they give the
    recommendation's printed table).  ``ValueError`` unless ``fs`` is a positive multiple of 10."""
    fs = _loudness_fs(fs, "k_weighting_coefficients")
    f0, gain_db, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / fs)
    vh = 10.0 ** (gain_db / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = np.array([(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0,
                      2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0], dtype=np.float64)
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    highpass = np.array([1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0], dtype=np.float64)
    return shelf, highpass


def loudness_gain(x: torch.Tensor, fs: int, lengths: Lengths = None, target: float = -23.0,
                  peak: float = -1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(loudness, peak, gain)`` per signal, (..., T) -> (...) float32 each: the integrated loudness of ITU-R BS.1770-4 in LUFS (one
    channel: K-weighting, 400 ms blocks every 100 ms, the -70 LUFS and the -10 LU gate; ``-inf`` when no block is left), the sample peak
    ``max |x|``, and the factor that brings the signal to ``target`` LUFS without its peak passing ``peak`` dBFS: ``10^((target - L) / 20)``,
    lowered to ``10^(peak / 20) / max|x|`` where that binds, 1 for a signal whose loudness is not finite.  With ``lengths``, of
    ``[..., :lengths[r]]`` per row (0 is a legal length), each value the bits of the call on that row alone.  One launch sequence
    (``eben_loudness``, ``csrc/loudness.hip``): filter state and sums float64, the weighted signal never stored.  Restated from the
    recommendation (parity with pyloudnorm / libebur128 unpinned)."""
    what = "loudness_gain"
    fs = _loudness_fs(fs, what)
    target, peak = float(target), float(peak)
    if not (math.isfinite(target) and math.isfinite(peak)):
        raise ValueError(f"{what}: target and peak must be finite, got {target} LUFS and {peak} dBFS")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"{what}: expected a (..., time) signal, got shape {tuple(x.shape)}")
    lead, t = tuple(x.shape[:-1]), x.shape[-1]
    rows = math.prod(lead)
    if not 1 <= rows <= 65535:
        raise ValueError(f"{what}: {rows} signals in one call (1 ... 65535)")
    host = _host_lengths(lengths, rows, t, what, least=0) if lengths is not None else None   # refused before anything touches a device
    if not x.is_cuda:
        raise EbenError(f"{what} runs only on an MI355X HIP device (got a tensor on '{x.device}'); there is no CPU path")
    x2 = x.detach().to(torch.float32).contiguous().reshape(rows, t)
    lens = None
    if lengths is not None:
        lens = host.to(x2.device, non_blocking=True) if host is not None else _device_lengths(lengths, rows, lead, x2.device, what)
    lib = load()
    nbytes = lib.eben_loudness_workspace(rows, t, fs)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
    out = torch.empty((3, rows), dtype=torch.float32, device=x2.device)
    check(lib.eben_loudness(ptr(x2), rows, t, _lens_ptr(lens), fs, target, peak, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                            ws.data_ptr(), nbytes, stream()), what)
    return out[0].reshape(lead), out[1].reshape(lead), out[2].reshape(lead)


def integrated_loudness(x: torch.Tensor, fs: int, lengths: Lengths = None) -> torch.Tensor:
    """Integrated loudness in LUFS per signal (``loudness_gain``'s first value): (..., T) -> (...)."""
    return loudness_gain(x, fs, lengths)[0]


class _MeanMetric(torch.nn.Module):
    """torchmetrics-style mean of a per-signal metric: state is a device-side sum and count (not buffers)."""

    def __init__(self):
        super().__init__()
        self._sum: Optional[torch.Tensor] = None
        self._count: Optional[torch.Tensor] = None

    def _values(self, preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None) -> torch.Tensor:
        raise NotImplementedError

    def _accumulate(self, values: torch.Tensor) -> None:
        if self._sum is None or self._sum.device != values.device:
            self._sum = torch.zeros((), dtype=torch.float64, device=values.device)
            self._count = torch.zeros((), dtype=torch.int64, device=values.device)
        self._sum += values.sum(dtype=torch.float64)
        self._count += values.numel()

    def update(self, preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None) -> None:
        self._accumulate(self._values(preds, target, lengths))

    def compute(self) -> torch.Tensor:
        if self._sum is None:
            raise RuntimeError(f"{type(self).__name__}.compute() called before any update()")
        return (self._sum / self._count).to(torch.float32)

    def reset(self) -> None:
        self._sum = self._count = None

    def forward(self, preds: torch.Tensor, target: torch.Tensor, lengths: Lengths = None) -> torch.Tensor:
        """Batch mean of this call; also accumulated into the running state."""
        values = self._values(preds, target, lengths)
        self._accumulate(values)
        return values.mean()


class ScaleInvariantSignalDistortionRatio(_MeanMetric):
    def __init__(self, zero_mean: bool = False):
        super().__init__()
        self.zero_mean = bool(zero_mean)

    def _values(self, preds, target, lengths=None):
        return si_sdr(preds, target, lengths, zero_mean=self.zero_mean)


class ScaleInvariantSignalNoiseRatio(_MeanMetric):
    def _values(self, preds, target, lengths=None):
        return si_snr(preds, target, lengths)


class SignalNoiseRatio(_MeanMetric):
    def __init__(self, zero_mean: bool = False):
        super().__init__()
        self.zero_mean = bool(zero_mean)

    def _values(self, preds, target, lengths=None):
        return snr(preds, target, lengths, zero_mean=self.zero_mean)


class SignalDistortionRatio(_MeanMetric):
    """Mean BSS-eval SDR (``sdr``), torchmetrics' class of the same name without its conjugate-gradient option."""

    def __init__(self, filter_length: int = 512, zero_mean: bool = False, load_diag: Optional[float] = None):
        super().__init__()
        self.filter_length = sdr_filter_length(filter_length, "SignalDistortionRatio: filter_length")
        self.zero_mean, self.load_diag = bool(zero_mean), load_diag

    def _values(self, preds, target, lengths=None):
        return sdr(preds, target, lengths, self.filter_length, self.zero_mean, self.load_diag)


class _SpeechMeasure(_MeanMetric):
    """Mean of one of ``speech_measures``' values at ``fs`` (16000 or 8000)."""

    measure = ""

    def __init__(self, fs: int):
        super().__init__()
        measures_geometry(fs)   # another rate is refused here
        self.fs = int(fs)

    def _values(self, preds, target, lengths=None):
        return speech_measures(preds, target, self.fs, lengths, (self.measure,))[self.measure]


class SegmentalSignalNoiseRatio(_SpeechMeasure):
    measure = "seg_snr"


class FrequencyWeightedSegmentalSNR(_SpeechMeasure):
    measure = "fw_seg_snr"


class LogLikelihoodRatio(_SpeechMeasure):
    measure = "llr"


class CepstralDistance(_SpeechMeasure):
    measure = "cd"


class IntegratedLoudness(_MeanMetric):
    """Mean integrated loudness in LUFS (``integrated_loudness``) of the signals seen; a level has no reference, so ``update`` and
    ``forward`` take one signal.  Signals without a finite loudness (silence, nothing over the gates) are left out of sum and count,
    without a host wait."""

    def __init__(self, fs: int):
        super().__init__()
        self.fs = _loudness_fs(fs, "IntegratedLoudness")

    def _values(self, x, lengths=None):   # noqa: D102 -- one signal, not a pair
        return integrated_loudness(x, self.fs, lengths)

    def _accumulate(self, values: torch.Tensor) -> None:
        if self._sum is None or self._sum.device != values.device:
            self._sum = torch.zeros((), dtype=torch.float64, device=values.device)
            self._count = torch.zeros((), dtype=torch.int64, device=values.device)
        finite = torch.isfinite(values)
        self._sum += torch.where(finite, values, torch.zeros_like(values)).sum(dtype=torch.float64)
        self._count += finite.sum()

    def update(self, x: torch.Tensor, lengths: Lengths = None) -> None:
        self._accumulate(self._values(x, lengths))

    def forward(self, x: torch.Tensor, lengths: Lengths = None) -> torch.Tensor:
        """Mean over this call's signals with a finite loudness (NaN when there is none); also accumulated into the running state."""
        values = self._values(x, lengths)
        self._accumulate(values)
        finite = torch.isfinite(values)
        return (torch.where(finite, values, torch.zeros_like(values)).sum(dtype=torch.float64) / finite.sum()).to(torch.float32)


class ShortTimeObjectiveIntelligibility(_MeanMetric):
    def __init__(self, fs: int, extended: bool = False):
        super().__init__()
        self.fs = int(fs)
        self.extended = bool(extended)

    def _values(self, preds, target, lengths=None):
        return stoi(preds, target, self.fs, lengths, extended=self.extended)


class LogSpectralDistance(_MeanMetric):
    """Mean LSD over one band (``band_hz`` None or ``(lo, hi)`` in Hz)."""

    def __init__(self, fs: int, n_fft: int = 2048, hop: int = 512, band_hz=None):
        super().__init__()
        if not _is_band(band_hz):
            raise ValueError("LogSpectralDistance averages one band: band_hz must be None or (lo, hi)")
        self.fs, self.n_fft, self.hop, self.band_hz = int(fs), int(n_fft), int(hop), band_hz
        lsd_band_bins(band_hz, self.fs, self.n_fft)   # a band without a bin is refused here

    def _values(self, preds, target, lengths=None):
        return lsd(preds, target, self.fs, lengths, self.n_fft, self.hop, self.band_hz)
