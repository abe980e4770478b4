"""Waveform augmentation on the device.

Counterpart of ``vibravox/torch_modules/dsp/data_augmentation.py:8-71`` (``WaveformDataAugmentation``, applied by the BWE
collator to the padded batch, bwe.py:286) for batches that already live in HBM: the same constructor, the same sequence
of ``torch.rand(1)`` / ``torch.randint`` draws on the CPU generator (so a seed selects the same augmentation), the work
itself as HIP kernels:

  * time masking (``dsp/time_masking_waveform.py:18-36``): one in-place zero-fill launch per waveform;
  * speed perturbation (``T.SpeedPerturbation`` = ``torchaudio.functional.speed`` -> ``resample``): windowed-sinc polyphase
    interpolation, ``eben_resample``; the kernel table follows torchaudio's ``_get_sinc_resample_kernel`` (hann window,
    lowpass width 6, rolloff 0.99) -- torchaudio is not installed here, so this part is a restatement (parity unpinned);
  * pitch shift (``T.PitchShift`` = ``torchaudio.functional.pitch_shift``): STFT (n_fft 512, hop 128, periodic hann) as
    framing + one GEMM, ``eben_phase_vocoder`` (time stretch by 2^(-steps/12)), inverse DFT as one GEMM + overlap-add +
    window-envelope normalisation, then ``eben_resample`` back to the original duration, cropped / padded to the input
    length.  Restated like the resampling (parity unpinned).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import CLIP_MAX_BANDS, EbenClipBand, EbenMaskClip, EbenOlaClip, EbenResampleClip, EbenVocoderClip, check, load, ptr, stream


KAISER_BETA = 14.769656459379492   # torchaudio's default beta of "sinc_interp_kaiser"


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, device=None,
                         resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None):
    """(kernels (new, 2*width+orig) float32, width, orig, new) -- torchaudio.functional._get_sinc_resample_kernel.

    The phase/tap grid t is built in float64 and clamped to +-lowpass_filter_width; the sinc, the window and the
    ``base / orig`` scale are float64 and the product is cast to float32 once.  Windows:

      * ``"sinc_interp_hann"`` (default): cos(pi t / (2 width))^2.
      * ``"sinc_interp_kaiser"``: i0(beta sqrt(1 - (t/width)^2)) / i0(beta), beta defaulting to 14.769656459379492.  As
        torchaudio does, beta becomes a 0-dim tensor built from a Python float at the default dtype (float32, so beta is
        rounded to float32 first); its product with the float64 grid is float64, so the numerator i0 runs in float64, while
        the denominator i0(beta) is evaluated on the float32 scalar in float32 and promoted to float64 by the division.

    torchaudio is not installed here: both windows are restatements, not pinned against it.  One known difference:
    torchaudio forms the phase offsets ``arange(0, -new, -1) / new`` at the default dtype (float32) before adding the
    float64 tap grid; here they are float64 (exact for new = 1, within ~1e-7 of torchaudio's table otherwise).
    """
    if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
        raise ValueError(f"Invalid resampling method: {resampling_method}")
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    else:
        beta_t = torch.tensor(float(KAISER_BETA if beta is None else beta), dtype=torch.float32)
        window = torch.i0(beta_t * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(beta_t)
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return k.to(torch.float32).contiguous().to(device), width, orig, new


_kernel_cache = {}


def resample(x: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """torchaudio.functional.resample(x, orig_freq, new_freq) on the device; x (..., time) float32."""
    key = (int(orig_freq), int(new_freq), x.device)
    if key not in _kernel_cache:
        _kernel_cache[key] = sinc_resample_kernel(orig_freq, new_freq, device=x.device)
    k, width, orig, new = _kernel_cache[key]
    if orig == new:
        return x.clone()
    lead, t = x.shape[:-1], x.shape[-1]
    rows = max(1, math.prod(lead))
    x2 = x.contiguous().reshape(rows, t)
    t_out = int(math.ceil(new * t / orig))
    out = torch.empty((rows, t_out), dtype=torch.float32, device=x.device)
    check(load().eben_resample(ptr(x2), ptr(k), ptr(out), rows, t, t_out, orig, new, width, stream()), "resample")
    return out.reshape(*lead, t_out)


def speed(x: torch.Tensor, sample_rate: int, factor: float) -> torch.Tensor:
    """torchaudio.functional.speed: play `factor` times faster = resample from int(factor * rate) to rate."""
    return resample(x, int(factor * sample_rate), int(sample_rate))


_ps_cache = {}


def _pitch_plan(n_fft: int, device):
    key = (n_fft, device)
    if key not in _ps_cache:
        bins = n_fft // 2 + 1
        w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
        n = torch.arange(n_fft, dtype=torch.float64)
        k = torch.arange(bins, dtype=torch.float64)
        ang = 2 * math.pi * k[:, None] * n[None, :] / n_fft
        fwd = torch.cat((torch.cos(ang) * w, -torch.sin(ang) * w), dim=0)                        # (2*bins, n_fft): windowed rDFT
        c = torch.full((bins,), 2.0, dtype=torch.float64)
        c[0] = c[-1] = 1.0
        inv = torch.cat((torch.cos(ang) * c[:, None], -torch.sin(ang) * c[:, None]), dim=0).t() * (w / n_fft)[:, None]   # (n_fft, 2*bins)
        _ps_cache[key] = dict(
            bins=bins, window=w,
            fwd=fwd.to(torch.float32).unsqueeze(-1).contiguous().to(device), inv=inv.to(torch.float32).unsqueeze(-1).contiguous().to(device),
            spec_f=ops.ConvSpec(c_in=n_fft, c_out=2 * bins, ksize=1), spec_i=ops.ConvSpec(c_in=2 * bins, c_out=n_fft, ksize=1),
            cache_f=ops.PackedWeights(), cache_i=ops.PackedWeights(), env={})
    return _ps_cache[key]


def pitch_shift(x: torch.Tensor, sample_rate: int, n_steps: int, bins_per_octave: int = 12, n_fft: int = 512) -> torch.Tensor:
    """torchaudio.functional.pitch_shift(x, sample_rate, n_steps) (defaults: n_fft 512, win 512, hop 128, hann) on the device."""
    import ctypes

    lib = load()
    hop = n_fft // 4
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    lead, t = x.shape[:-1], x.shape[-1]
    rows = max(1, math.prod(lead))
    dev = x.device
    pl = _pitch_plan(n_fft, dev)
    bins = pl["bins"]
    sig = x.contiguous().reshape(rows, t)
    st = stream()
    # STFT (center=True, reflect): frames of all rows as one (n_fft, rows*F) matrix, one GEMM
    nf = t // hop + 1
    fr = torch.empty((1, n_fft, rows * nf), dtype=torch.float32, device=dev)
    check(lib.eben_stft_frames(ptr(sig), ptr(fr), rows, t, n_fft, hop, n_fft // 2, nf, st), "stft_frames")
    d = ops.conv_desc(pl["spec_f"], 1, rows * nf)
    pw = ops.pack_weights(pl["spec_f"], d, pl["fwd"], None, pl["cache_f"], False)
    spec = torch.empty((1, 2 * bins, rows * nf), dtype=torch.float32, device=dev)
    check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(fr), ptr(pw.wp_fwd), None, None, ptr(spec), st), "stft_gemm")
    # time stretch
    nf_out = int(math.ceil(nf / rate))
    if (nf_out - 1) * rate >= nf:   # torch.arange(0, nf, rate) excludes nf itself
        nf_out -= 1
    stretched = torch.empty((1, 2 * bins, rows * nf_out), dtype=torch.float32, device=dev)
    check(lib.eben_phase_vocoder(ptr(spec), ptr(stretched), rows, bins, nf, nf_out, rate, float(hop), st), "phase_vocoder")
    # inverse STFT: one GEMM to windowed frames, overlap-add, window-envelope normalisation
    d = ops.conv_desc(pl["spec_i"], 1, rows * nf_out)
    pw = ops.pack_weights(pl["spec_i"], d, pl["inv"], None, pl["cache_i"], False)
    frames = torch.empty((1, n_fft, rows * nf_out), dtype=torch.float32, device=dev)
    check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(stretched), ptr(pw.wp_fwd), None, None, ptr(frames), st), "istft_gemm")
    len_stretch = int(round(t / rate))
    full = n_fft + hop * (nf_out - 1)
    valid = min(len_stretch, full - n_fft // 2)
    y = torch.zeros((rows, len_stretch), dtype=torch.float32, device=dev)
    ola = torch.empty((rows, valid), dtype=torch.float32, device=dev)
    check(lib.eben_overlap_add_ex(ptr(frames), ptr(ola), rows, valid, n_fft, nf_out, hop, n_fft // 2, 0, 0, nf_out, rows * nf_out, st),
          "overlap_add")
    ek = (nf_out, valid)
    if ek not in pl["env"]:
        w2 = pl["window"] ** 2
        env = torch.zeros(full, dtype=torch.float64)
        for f in range(nf_out):
            env[f * hop:f * hop + n_fft] += w2
        pl["env"][ek] = (1.0 / env[n_fft // 2:n_fft // 2 + valid]).to(torch.float32).to(dev)
    y[:, :valid] = ola * pl["env"][ek]
    out = resample(y, int(sample_rate / rate), int(sample_rate))
    if out.shape[-1] >= t:
        out = out[:, :t]
    else:
        out = torch.nn.functional.pad(out, (0, t - out.shape[-1]))
    return out.contiguous().reshape(*lead, t)


def time_masking_(x: torch.Tensor, masking_percentage: float) -> torch.Tensor:
    """TimeMaskingBlockWaveform.forward (time_masking_waveform.py:28-36): in place, one torch.randint draw."""
    t = x.shape[-1]
    masked = int(t * masking_percentage / 100)
    first = torch.randint(0, t - masked, (1,)).item()
    if not x.is_contiguous():
        raise ValueError("time masking works in place on a contiguous (..., time) tensor")
    check(load().eben_time_mask(ptr(x), x.numel() // t, t, first, masked, stream()), "time_mask")
    return x


# ---------------------------------------------------------------------------------------------
# Per-clip mode (``WaveformDataAugmentation(per_clip=True)``): every clip of the batch makes its own draws and the batch keeps
# its length.  Row b of the result is
#     time_masking( pitch_shift( fit_T( speed(row_b, rate, factor_b) ), rate, steps_b ), pct_b at its drawn position )
# with each stage skipped where the clip's plan says so, each stage the function above applied to that row alone, and fit_T =
# the first T samples, zero-filled on the right.  The kernels (csrc/augment_clips.hip) take their parameters per row.
# ---------------------------------------------------------------------------------------------
class BandTable(NamedTuple):
    """The taps of ``sinc_resample_kernel``'s table that can be non-zero: ``band[p, j] = kernels[p, first[p] + j]``, j < W."""
    band: torch.Tensor    # (new, W) float32
    first: torch.Tensor   # (new,) int32
    W: int
    width: int
    orig: int
    new: int


def _sinc_taps(phase: torch.Tensor, j: torch.Tensor, orig: int, base: float, width: int, lowpass_filter_width: int):
    """``sinc_resample_kernel``'s float64 expression (hann window) at phases ``phase`` (n, 1) and tap indices ``j`` (n, m); also whether
    each tap lies strictly inside the clamp, i.e. can be non-zero."""
    idx = (j - width).to(torch.float64) / orig
    t = (phase + idx) * base
    inside = t.abs() < lowpass_filter_width
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return k.to(torch.float32), inside


def band_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, chunk: int = 4096) -> BandTable:
    """``sinc_resample_kernel(orig_freq, new_freq)`` ("sinc_interp_hann") without its zeros, built directly on the host.

    Where ``|t * base| >= lowpass_filter_width`` the table's argument is clamped, the window is cos(pi/2)^2 ~ 4e-33 and the
    float32 product is exactly 0, so a phase has at most ``2*width + 1`` taps that can be non-zero, and they are contiguous.
    The same float64 expression is evaluated only there: pass 1 finds each phase's span, W is the widest, pass 2 evaluates
    ``[first, first + W)`` with ``first`` moved left where the span would pass the table's last tap (the extra taps are clamped
    ones, exactly 0).  A 16 kHz pitch ratio (new = 16000, orig ~ 17000) takes 16000 x 19 values here instead of 271 M."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    taps = 2 * width + orig
    half = lowpass_filter_width * orig / base                        # the clamp's half width in taps
    cand = torch.arange(2 * math.ceil(half) + 5, dtype=torch.int64)[None, :]
    phases = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new
    firsts, counts = [], []
    for p0 in range(0, new, chunk):
        ph = phases[p0:p0 + chunk]
        lo = torch.floor(width - ph[:, 0] * orig - half).to(torch.int64) - 2      # the span starts near width + orig*p/new - half
        j = lo[:, None] + cand
        _, inside = _sinc_taps(ph, j, orig, base, width, lowpass_filter_width)
        inside &= (j >= 0) & (j < taps)
        assert not bool(inside[:, 0].any()) and not bool((inside[:, -1] & (j[:, -1] < taps - 1)).any()), "band search window too narrow"
        n = inside.sum(dim=1)
        f = lo + inside.to(torch.int64).argmax(dim=1)
        assert bool((n > 0).all()) and bool((torch.gather(inside.cumsum(1), 1, (f - lo + n - 1)[:, None])[:, 0] == n).all()), "band is not contiguous"
        firsts.append(f)
        counts.append(n)
    first, count = torch.cat(firsts), torch.cat(counts)
    W = int(count.max())
    first = first.clamp(0, taps - W)
    band = torch.empty((new, W), dtype=torch.float32)
    jw = torch.arange(W, dtype=torch.int64)[None, :]
    for p0 in range(0, new, chunk):
        band[p0:p0 + chunk], _ = _sinc_taps(phases[p0:p0 + chunk], first[p0:p0 + chunk, None] + jw, orig, base, width, lowpass_filter_width)
    return BandTable(band.contiguous(), first.to(torch.int32).contiguous(), W, width, orig, new)


_IDENTITY_BAND = BandTable(torch.ones((1, 1), dtype=torch.float32), torch.zeros(1, dtype=torch.int32), 1, 0, 1, 1)   # resample()'s orig == new: a copy
_band_cache = {}


def _device_band(orig_freq: int, new_freq: int, device) -> BandTable:
    key = (int(orig_freq), int(new_freq), device)
    if key not in _band_cache:
        b = _IDENTITY_BAND if int(orig_freq) == int(new_freq) else band_resample_kernel(orig_freq, new_freq)
        _band_cache[key] = b._replace(band=b.band.to(device), first=b.first.to(device))
    return _band_cache[key]


def resample_clips(src: torch.Tensor, rows: Sequence[Tuple[int, int, int, int, int]], out: torch.Tensor) -> torch.Tensor:
    """For each ``(src_offset, t_in, orig_freq, new_freq, dst_row)``: ``out[dst_row] = fit_T(resample(src[src_offset : src_offset + t_in], orig_freq,
    new_freq))``, rows of any ratios in one launch (``eben_resample_clips``).  ``src``: float32 device tensor, read flat; ``out``: (R, T), not ``src``."""
    lib = load()
    t = out.shape[-1]
    rows = list(rows)
    ratios = sorted({(o, n) for _, _, o, n, _ in rows})
    for r0 in range(0, len(ratios), CLIP_MAX_BANDS):   # more ratios than one call carries: one call per 16 of them
        part = ratios[r0:r0 + CLIP_MAX_BANDS]
        tabs = [_device_band(o, n, out.device) for o, n in part]
        bands = (EbenClipBand * len(part))(*[EbenClipBand(b.band.data_ptr(), b.first.data_ptr(), b.orig, b.new, b.width, b.W) for b in tabs])
        index = {r: i for i, r in enumerate(part)}
        mine = [EbenResampleClip(off, t_in, index[(o, n)], dst, 0) for off, t_in, o, n, dst in rows if (o, n) in index]
        table = (EbenResampleClip * len(mine))(*mine)
        check(lib.eben_resample_clips(ptr(src), src.numel(), ptr(out), out.numel() // t, t, bands, len(part), table, len(mine), stream()), "resample_clips")
    return out


def time_mask_clips_(x: torch.Tensor, masks: Sequence[Tuple[int, int, int]]) -> torch.Tensor:
    """``x[row, first : first + count] = 0`` for each ``(row, first, count)``, in place, one launch (``eben_time_mask_clips``); x (R, T)."""
    t = x.shape[-1]
    table = (EbenMaskClip * len(masks))(*[EbenMaskClip(r, f, c) for r, f, c in masks])
    check(load().eben_time_mask_clips(ptr(x), x.numel() // t, t, table, len(masks), stream()), "time_mask_clips")
    return x


def pitch_shift_clips(x: torch.Tensor, rows: Sequence[int], steps: Sequence[int], sample_rate: int, out: torch.Tensor, bins_per_octave: int = 12,
                      n_fft: int = 512) -> torch.Tensor:
    """``out[r] = pitch_shift(x[r], sample_rate, s)`` for each r of ``rows`` with its own s of ``steps``; x, out (R, T), ``out`` may be ``x``
    (the rows are gathered before anything is written).

    STFT framing and the two DFT GEMMs are pitch_shift's, on the gathered rows (dense at T) and on the stretched spectra of all rows as
    concatenated columns; the phase vocoder, the overlap-add with its envelope and the resampling take their parameters per row."""
    import ctypes

    lib = load()
    hop = n_fft // 4
    t, dev, st = x.shape[-1], x.device, stream()
    pl = _pitch_plan(n_fft, dev)
    bins = pl["bins"]
    if "w2" not in pl:
        pl["w2"] = (pl["window"] ** 2).to(dev)   # float64, the values pitch_shift's envelope table sums
    n = len(rows)
    sig = x[torch.as_tensor(list(rows), device=dev)].contiguous()
    nf = t // hop + 1
    fr = torch.empty((1, n_fft, n * nf), dtype=torch.float32, device=dev)
    check(lib.eben_stft_frames(ptr(sig), ptr(fr), n, t, n_fft, hop, n_fft // 2, nf, st), "stft_frames")
    d = ops.conv_desc(pl["spec_f"], 1, n * nf)
    pw = ops.pack_weights(pl["spec_f"], d, pl["fwd"], None, pl["cache_f"], False)
    spec = torch.empty((1, 2 * bins, n * nf), dtype=torch.float32, device=dev)
    check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(fr), ptr(pw.wp_fwd), None, None, ptr(spec), st), "stft_gemm")
    # per row: the stretch's geometry exactly as pitch_shift computes it; only this side is ragged
    voc, ola, res = [], [], []
    cols = floats = 0
    for i, s in enumerate(steps):
        rate = 2.0 ** (-float(s) / bins_per_octave)
        nf_out = int(math.ceil(nf / rate))
        if (nf_out - 1) * rate >= nf:
            nf_out -= 1
        len_stretch = int(round(t / rate))
        valid = min(len_stretch, n_fft + hop * (nf_out - 1) - n_fft // 2)
        voc.append(EbenVocoderClip(rate, nf_out, cols))
        ola.append(EbenOlaClip(floats, cols, nf_out, len_stretch, valid))
        res.append((floats, len_stretch, int(sample_rate / rate), int(sample_rate), rows[i]))
        cols += nf_out
        floats += -(-len_stretch // 4) * 4   # rows of the ragged buffer start on 16-byte lines
    stretched = torch.empty((1, 2 * bins, cols), dtype=torch.float32, device=dev)
    check(lib.eben_phase_vocoder_clips(ptr(spec), ptr(stretched), bins, nf, cols, (EbenVocoderClip * n)(*voc), n, float(hop), st), "phase_vocoder_clips")
    d = ops.conv_desc(pl["spec_i"], 1, cols)
    pw = ops.pack_weights(pl["spec_i"], d, pl["inv"], None, pl["cache_i"], False)
    frames = torch.empty((1, n_fft, cols), dtype=torch.float32, device=dev)
    check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(stretched), ptr(pw.wp_fwd), None, None, ptr(frames), st), "istft_gemm")
    y = torch.empty(floats, dtype=torch.float32, device=dev)
    check(lib.eben_overlap_add_clips(ptr(frames), cols, pl["w2"].data_ptr(), ptr(y), floats, n_fft, hop, n_fft // 2, (EbenOlaClip * n)(*ola), n, st),
          "overlap_add_clips")
    return resample_clips(y, res, out)


class ClipPlan(NamedTuple):
    """What one clip drew.  A stage that was not drawn is None; ``masked`` samples are zeroed from ``first_1`` in waveform 1 and from
    ``first_2`` in waveform 2 (None without a second waveform)."""
    clip: int
    factor: Optional[float] = None
    steps: Optional[int] = None
    pct: Optional[float] = None
    masked: int = 0
    first_1: Optional[int] = None
    first_2: Optional[int] = None


def plan_per_clip(module: "WaveformDataAugmentation", B: int, T: int, two_waveforms: bool) -> List[ClipPlan]:
    """The draws of the per-clip mode, on the CPU generator: for clip 0 .. B-1 in order, the draws one call of the batch-level ``forward``
    makes (with both waveforms of a clip sharing factor, steps and percentage, each with its own mask position).  Returns the clips that
    drew at least one stage, in order; needs no GPU."""
    n = 2 if two_waveforms else 1
    plan = []
    for b in range(B):
        if not torch.rand(1) < module.apply_data_augmentation:
            continue
        factor = steps = pct = first_1 = first_2 = None
        masked = 0
        if torch.rand(1) < module.p_speed_perturbation:
            factor = module.speed_perturbation_factors[torch.randint(len(module.speed_perturbation_factors), size=(1,)).item()]
            for _ in range(n):
                torch.randint(1, ())   # T.SpeedPerturbation.forward's own draw, once per waveform (see forward)
        if torch.rand(1) < module.p_pitch_shift:
            steps = module.pitch_shift_steps[torch.randint(len(module.pitch_shift_steps), size=(1,)).item()]
        if torch.rand(1) < module.p_time_masking:
            pct = module.time_masking_percentage[torch.randint(len(module.time_masking_percentage), size=(1,)).item()]
            masked = int(T * pct / 100)
            first_1 = torch.randint(0, T - masked, (1,)).item()
            if two_waveforms:
                first_2 = torch.randint(0, T - masked, (1,)).item()
        if factor is not None or steps is not None or pct is not None:
            plan.append(ClipPlan(b, factor, steps, pct, masked, first_1, first_2))
    return plan


def apply_clip_plan(plan: Sequence[ClipPlan], sample_rate: int, waveform_1: torch.Tensor, waveform_2: Optional[torch.Tensor] = None):
    """The planned stages on (B, 1, T) or (B, T) float32 device tensors; returns new tensors of the same shapes."""
    shape = waveform_1.shape
    T = shape[-1]
    B = waveform_1.numel() // T
    waves = [waveform_1] if waveform_2 is None else [waveform_1, waveform_2]
    assert all(w.shape == shape for w in waves) and (len(shape) == 2 or (len(shape) == 3 and shape[1] == 1)), "per-clip augmentation takes (B, 1, T) or (B, T)"
    # a working copy with rows b (waveform 1) and B + b (waveform 2): every stage is one pass over both, written in place
    x = torch.cat([w.reshape(B, T) for w in waves], dim=0) if len(waves) > 1 else waveform_1.reshape(B, T).clone()
    offs = [k * B for k in range(len(waves))]
    sp = [(p.clip + o, p.factor) for p in plan if p.factor is not None for o in offs]
    if sp:
        src = x[torch.as_tensor([r for r, _ in sp], device=x.device)].contiguous()   # the rows that drew a speed, gathered: the kernel reads them, writes x
        resample_clips(src, [(i * T, T, int(f * sample_rate), int(sample_rate), r) for i, (r, f) in enumerate(sp)], x)
    ps = [(p.clip + o, p.steps) for p in plan if p.steps is not None for o in offs]
    if ps:
        pitch_shift_clips(x, [r for r, _ in ps], [s for _, s in ps], sample_rate, x)
    tm = [(p.clip + o, f, p.masked) for p in plan if p.pct is not None for o, f in zip(offs, (p.first_1, p.first_2))]
    if tm:
        time_mask_clips_(x, tm)
    out = [x[o:o + B].reshape(shape) for o in offs]
    return out[0], (out[1] if waveform_2 is not None else None)


class WaveformDataAugmentation(torch.nn.Module):
    def __init__(self, sample_rate, p_data_augmentation=0, p_speed_perturbation=0.3, p_pitch_shift=0.3, p_time_masking=0.3,
                 speed_perturbation_factors=(0.7, 0.8, 0.85, 0.9, 0.95, 1.05, 1.1, 1.15, 1.2, 1.3),
                 pitch_shift_steps=(-4, -3, -2, -1, 1, 2, 3, 4, 5, 6), time_masking_percentage=(1, 2, 3, 4, 5, 6, 7, 8), per_clip: bool = False):
        super().__init__()
        self.sample_rate = sample_rate
        self.per_clip = bool(per_clip)   # True: every clip makes its own draws and the batch keeps its length (plan_per_clip)
        self.last_plan: List[ClipPlan] = []
        assert 0 <= p_data_augmentation <= 1, "p_data_augmentation must be in [0, 1]"
        assert 0 <= p_speed_perturbation <= 1, "p_speed_perturbation must be in [0, 1]"
        assert 0 <= p_pitch_shift <= 1, "p_pitch_shift must be in [0, 1]"
        assert 0 <= p_time_masking <= 1, "p_time_masking must be in [0, 1]"
        self.apply_data_augmentation = p_data_augmentation
        self.p_speed_perturbation = p_speed_perturbation
        self.p_pitch_shift = p_pitch_shift
        self.p_time_masking = p_time_masking
        self.speed_perturbation_factors = speed_perturbation_factors
        self.pitch_shift_steps = pitch_shift_steps
        self.time_masking_percentage = time_masking_percentage

    def forward(self, waveform_1: torch.Tensor, waveform_2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        if self.per_clip:
            t = waveform_1.shape[-1]
            self.last_plan = plan_per_clip(self, waveform_1.numel() // t, t, waveform_2 is not None)
            if not self.last_plan:
                return waveform_1, waveform_2
            return apply_clip_plan(self.last_plan, self.sample_rate, waveform_1, waveform_2)
        if torch.rand(1) < self.apply_data_augmentation:
            if torch.rand(1) < self.p_speed_perturbation:
                f = self.speed_perturbation_factors[torch.randint(len(self.speed_perturbation_factors), size=(1,)).item()]
                # torchaudio's T.SpeedPerturbation.forward picks its speeder with torch.randint(len(factors), ()) on EVERY call --
                # one draw per waveform even with the single factor the reference constructs it with (data_augmentation.py:56-60)
                torch.randint(1, ())
                waveform_1 = speed(waveform_1, self.sample_rate, f)
                if waveform_2 is not None:
                    torch.randint(1, ())
                    waveform_2 = speed(waveform_2, self.sample_rate, f)
            if torch.rand(1) < self.p_pitch_shift:
                steps = self.pitch_shift_steps[torch.randint(len(self.pitch_shift_steps), size=(1,)).item()]
                waveform_1 = pitch_shift(waveform_1, self.sample_rate, steps)
                if waveform_2 is not None:
                    waveform_2 = pitch_shift(waveform_2, self.sample_rate, steps)
            if torch.rand(1) < self.p_time_masking:
                pct = self.time_masking_percentage[torch.randint(len(self.time_masking_percentage), size=(1,)).item()]
                waveform_1 = time_masking_(waveform_1, pct)
                if waveform_2 is not None:
                    waveform_2 = time_masking_(waveform_2, pct)
        return waveform_1, waveform_2
