"""Enhancing a corpus: utterances of any lengths through a trained EBEN generator in ragged batches.

What the reference does clip by clip (``scripts/eben_enhanced_vibravox.py``: ``cut_to_valid_length``, one batch-1 forward each) runs
here as a few batched forwards: the clips are sorted by length, dealt into batches of at most ``max_batch_samples`` buffer samples and
each batch goes through ``EBENGenerator.forward_ragged`` -- every clip's result is the one its own forward gives.

``evaluate_clips`` scores such a corpus against its references the same way (the reference's ``trainer.test`` does it with batches of
one): per batch one ragged forward and the SI-SDR / STOI kernels with a length per row, straight from the padded buffers.

Recordings at another rate than the model's (the reference's script resamples 48 kHz to 16 kHz in front of every forward) enter
through ``input_rate=``: one ``rate.resample_ragged`` launch per batch writes the generator's padded buffer, and ``enhance_stream``
resamples with carried state.

``enhance_to_pcm`` is ``enhance_clips`` whose results leave the device as the bytes of WAVE files (the reference's script stores every
enhanced recording): one ``eben_pcm_encode_ragged`` launch per batch on the rows of the output buffer, one copy per group to pinned
memory; ``export.enhance_corpus`` runs it from a directory to a directory.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional, Sequence

import torch

from . import ragged

#: the rate ``base_se.py`` evaluates SI-SDR and STOI at
EVAL_RATE = 16000

#: what ``evaluate_clips`` can score, all at ``EVAL_RATE``: the two ``base_se.py`` logs (the default) and the evaluation set of a
#: bandwidth-extension model -- "lsd" over the whole band, "lsd_hf" over [lsd_hf_cutoff_hz, EVAL_RATE / 2] (the band being reconstructed)
EVAL_METRICS = ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
DEFAULT_EVAL_METRICS = ("si_sdr", "stoi")
#: scored after a short distortion filter: "sdr" is the BSS-eval SDR (``metrics.sdr``) with ``sdr_filter_length`` taps
EVAL_METRICS_FILTERED = ("sdr",)
#: the frame-based measures of ``metrics.speech_measures`` (segmental SNR, frequency-weighted segmental SNR, LPC log-likelihood ratio,
#: LPC cepstral distance): one call per batch for those that are named
EVAL_METRICS_FRAMED = ("seg_snr", "fw_seg_snr", "llr", "cd")
#: level: "lufs_diff" is the integrated loudness (ITU-R BS.1770-4, ``metrics.integrated_loudness``) of the enhanced clip minus its
#: reference's, in LU -- one measuring call per signal per batch; NaN when neither has a finite loudness, +-inf when one has none
EVAL_METRICS_LEVEL = ("lufs_diff",)
LSD_N_FFT, LSD_HOP = 2048, 512

#: buffer samples (rows x padded length) per batch: 262 s at 16 kHz.  The widest activations (32 channels at 1/4 of the audio rate,
#: 64 at 1/8) take 32 bytes per audio sample each, 128 MiB a tensor at this budget
MAX_BATCH_SAMPLES = 1 << 22


#: samples per push of ``enhance_stream``: about a second at 16 kHz, a whole number of latent frames for every bank
STREAM_CHUNK = 16384


def _rated(input_rate, model_rate) -> bool:
    """Whether clips at ``input_rate`` need resampling to reach the model: not without an ``input_rate``, not at the model's own."""
    if input_rate is None:
        return False
    if int(input_rate) <= 0 or int(model_rate) <= 0:
        raise ValueError(f"input_rate and model_rate must be positive, got {input_rate} and {model_rate}")
    return int(input_rate) != int(model_rate)


@torch.no_grad()
def enhance_stream(generator, clip: torch.Tensor, chunk_samples: int = STREAM_CHUNK, input_rate: Optional[int] = None, model_rate: int = 16000,
                   output_rate: Optional[int] = None, format: Optional[str] = None):
    """One long ``clip`` (rows, 1, T) through a ``streaming.StreamingEnhancer`` in pushes of ``chunk_samples``: the activations alive at
    any time are those of one chunk plus the stream state, not those of the whole recording.  Returns what
    ``generator(generator.cut_to_valid_length(clip))`` returns, (enhanced (rows, 1, T'), bands (rows, m, L)).  Nothing here waits for
    the device.  With ``input_rate`` the clip is at that rate and enters in pushes of ``chunk_samples`` model-rate samples' worth
    (``StreamingEnhancer.input_chunk_samples``); the result is that of ``augment.resample(clip, input_rate, model_rate)``, at the
    model's rate.

    ``output_rate`` / ``format`` (one of ``corpus.FORMATS``): the enhanced samples leave every push through the enhancer's way out
    (``StreamingEnhancer(output_rate=, output_format=)``) and the call returns their concatenation alone: uint8 (rows, bytes) with
    ``format``, else float32 (rows, 1, T'') at ``output_rate``."""
    from . import streaming

    if format is not None or (output_rate is not None and int(output_rate) != int(model_rate)):
        if clip.dim() != 3 or clip.shape[1] != 1 or clip.dtype is not torch.float32:
            raise ValueError(f"enhance_stream: expected a float32 (rows, 1, T) tensor, got {clip.dtype} {tuple(clip.shape)}")
        rated = _rated(input_rate, model_rate)
        total = clip.shape[2]
        ragged.plan(generator, [resampled_length(total, input_rate, model_rate) if rated else total])
        enhancer = streaming.StreamingEnhancer(generator, chunk_samples, streams=clip.shape[0], input_rate=input_rate if rated else None,
                                               model_rate=model_rate, output_rate=output_rate, output_format=format)
        chunk, parts = enhancer.input_chunk_samples, []
        for pos in range(0, total - chunk + 1, chunk):
            parts.append(enhancer.push(clip[:, :, pos : pos + chunk]))
        parts.append(enhancer.finish(clip[:, :, len(parts) * chunk :]))
        return torch.cat(parts, dim=-1)

    if clip.dim() != 3 or clip.shape[1] != 1 or clip.dtype is not torch.float32:
        raise ValueError(f"enhance_stream: expected a float32 (rows, 1, T) tensor, got {clip.dtype} {tuple(clip.shape)}")
    rows, _, total = clip.shape
    m = generator.pqmf.decimation
    rated = _rated(input_rate, model_rate)
    at_model = resampled_length(total, input_rate, model_rate) if rated else total
    ragged.plan(generator, [at_model])   # refuses a clip below the shortest one before anything runs
    cut = ragged.cut_length(generator, at_model)
    enhancer = streaming.StreamingEnhancer(generator, chunk_samples, streams=rows, return_bands=True, input_rate=input_rate if rated else None,
                                           model_rate=model_rate)
    chunk = enhancer.input_chunk_samples
    enhanced = torch.empty((rows, 1, cut), dtype=torch.float32, device=clip.device)
    bands = torch.empty((rows, m, (cut + generator.pqmf.kernel_size) // m), dtype=torch.float32, device=clip.device)
    pos = done_e = done_b = 0
    while True:
        last = total - pos < chunk
        e, b = enhancer.finish(clip[:, :, pos:]) if last else enhancer.push(clip[:, :, pos : pos + chunk])
        enhanced[:, :, done_e : done_e + e.shape[2]].copy_(e)
        bands[:, :, done_b : done_b + b.shape[2]].copy_(b)
        done_e, done_b, pos = done_e + e.shape[2], done_b + b.shape[2], pos + chunk
        if last:
            break
    if (done_e, done_b) != (enhanced.shape[2], bands.shape[2]):
        raise RuntimeError(f"enhance_stream: the stream returned {done_e} samples and {done_b} band samples of {enhanced.shape[2]} and {bands.shape[2]}")
    return enhanced, bands


def _resampled_rows(clips, idx, l_buf: int, input_rate: int, model_rate: int) -> torch.Tensor:
    """The clips ``idx``, at ``input_rate``, as rows at ``model_rate``: packed raw into one padded buffer and resampled by ONE
    ``rate.resample_ragged`` launch into a (rows, 1, >= l_buf) buffer -- row r starts with ``augment.resample`` of its clip alone and is
    zero behind it.  The buffer is ``l_buf`` wide unless the longest clip resamples to more (rows of equal cut lengths: no margin)."""
    from . import rate

    raw_lengths = [clips[i].shape[-1] for i in idx]
    device = clips[idx[0]].device
    raw = torch.empty((len(idx), 1, max(raw_lengths)), dtype=torch.float32, device=device)   # what lies behind a row is never read
    for r, i in enumerate(idx):
        raw[r, 0, : raw_lengths[r]].copy_(clips[i].reshape(-1))
    width = max(l_buf, resampled_length(raw.shape[2], input_rate, model_rate))
    out = torch.empty((len(idx), 1, width), dtype=torch.float32, device=device)
    rate.resample_ragged(raw, raw_lengths, input_rate, model_rate, out=out)
    return out


@torch.no_grad()
def enhance_clips(generator, clips: Sequence[torch.Tensor], *, max_batch_samples: int = MAX_BATCH_SAMPLES, return_bands: bool = False,
                  input_rate: Optional[int] = None, model_rate: int = 16000):
    """``clips``: 1-D, (1, T) or (1, 1, T) float32 tensors on the generator's device.  Returns the enhanced clips in input order, each
    ``cut_to_valid_length`` long and of its clip's rank; with ``return_bands`` also the list of their (m, L) enhanced bands.  Nothing
    here waits for the device: packing and unpacking are copies on the current stream.

    ``input_rate``: the clips are at that rate (the reference's script resamples 48 kHz recordings in front of the model); they are
    packed raw, the batches are composed on their lengths at ``model_rate``, and one ``rate.resample_ragged`` launch per batch writes
    the generator's input buffer.  The results are at the model's rate: those of ``enhance_clips`` on ``augment.resample(clip,
    input_rate, model_rate)``, bit for bit."""
    clips, rated, lengths = _clips_and_lengths(clips, input_rate, model_rate)
    batches, back = ragged.compose_batches(generator, lengths, max_batch_samples)
    enhanced: List[torch.Tensor] = []
    bands: List[torch.Tensor] = []
    for idx, plan, enh, bnd in _batch_forwards(generator, clips, lengths, batches, rated, input_rate, model_rate):
        for r, i in enumerate(idx):
            enhanced.append(enh[r, 0, : plan.cut[r]].reshape(clips[i].shape[:-1] + (plan.cut[r],)).clone())
            if return_bands:
                bands.append(bnd[r, :, : plan.row_lengths[1][r]].clone())
    enhanced = [enhanced[p] for p in back]
    return (enhanced, [bands[p] for p in back]) if return_bands else enhanced


def _clips_and_lengths(clips, input_rate, model_rate):
    """``(clips as a list, whether they need resampling, their lengths at the model's rate)``; refuses anything that is no mono clip."""
    clips = list(clips)
    for i, c in enumerate(clips):
        if c.dim() not in (1, 2, 3) or c.numel() != c.shape[-1] or c.dtype is not torch.float32:
            raise ValueError(f"clip {i}: expected a float32 tensor of shape (T,), (1, T) or (1, 1, T), got {c.dtype} {tuple(c.shape)}")
    rated = _rated(input_rate, model_rate)
    return clips, rated, [resampled_length(c.shape[-1], input_rate, model_rate) if rated else c.shape[-1] for c in clips]


def _batch_forwards(generator, clips, lengths, batches, rated: bool, input_rate, model_rate):
    """What ``enhance_clips`` and ``enhance_to_pcm`` share: per batch of ``ragged.compose_batches`` the clips packed (or resampled) into
    the padded buffer and one ``forward_ragged``.  Yields ``(idx, plan, enhanced (rows, 1, l_buf), bands)``; row r belongs to clip
    ``idx[r]`` and holds ``plan.cut[r]`` samples.  Runs in the caller's grad mode (``forward_ragged`` wants ``torch.no_grad()``)."""
    for idx in batches:
        plan = ragged.plan(generator, [lengths[i] for i in idx])
        if rated:
            buf = _resampled_rows(clips, idx, plan.l_buf, input_rate, model_rate)
        else:
            buf = torch.zeros((len(idx), 1, plan.l_buf), dtype=torch.float32, device=clips[idx[0]].device)
            for r, i in enumerate(idx):
                buf[r, 0, : plan.cut[r]].copy_(clips[i].reshape(-1)[: plan.cut[r]])
        enh, bnd = generator.forward_ragged(buf, [lengths[i] for i in idx])
        yield idx, plan, enh, bnd


def _encode_group(generator, clips, lengths, counts, group, fmt: int, rated: bool, input_rate, model_rate: int, out_rate: int, max_batch_samples: int,
                  dev_image: torch.Tensor, host_half: torch.Tensor, loudness: Optional[float] = None, peak: float = -1.0):
    """Queues one group of ``enhance_to_pcm``: its clips' batches through the generator, per batch one encode launch from the output
    buffer's rows into the device image (behind one ``rate.resample_ragged`` launch when the files are at another rate), then one
    asynchronous copy of image and clipped counts into ``host_half``.  Returns ``(order, event)``: the group's clips in the order of
    their counts, and the event behind the copy.  Nothing waits.

    With ``loudness`` every batch's rows are measured where they lie, at ``out_rate``, by one ``metrics.loudness_gain`` call in front of
    the encode launch, which reads the gains from the device; the rows' loudness and gain follow the counts in the image's tail
    (float32, ``n`` each) and travel in the same copy."""
    import numpy as np

    from . import corpus as C
    from . import metrics as M
    from . import rate

    lo, hi = group.lo, group.hi
    n = hi - lo
    sub_clips, sub_lengths = clips[lo:hi], lengths[lo:hi]
    counts_at = group.nbytes
    total = counts_at + (4 if loudness is None else 12) * n
    image = dev_image[:counts_at]
    clipped = dev_image[counts_at:counts_at + 4 * n].view(torch.int32)
    if loudness is not None:
        measured = dev_image[counts_at + 4 * n:counts_at + 8 * n].view(torch.float32)
        applied = dev_image[counts_at + 8 * n:total].view(torch.float32)
    order: List[int] = []
    with torch.no_grad(), torch.cuda.device(dev_image.device):
        batches, _ = ragged.compose_batches(generator, sub_lengths, max_batch_samples)
        for idx, plan, enh, _ in _batch_forwards(generator, sub_clips, sub_lengths, batches, rated, input_rate, model_rate):
            src = enh if out_rate == model_rate else rate.resample_ragged(enh, list(plan.cut), model_rate, out_rate)[0]
            src = src.contiguous()
            pitch = src.shape[-1]
            table = np.zeros(len(idx), dtype=C.ENC_ROW_DTYPE)
            for r, i in enumerate(idx):   # the batches are not in clip order: every row carries its own place in the image
                table[r] = (r * pitch, group.starts[i] + C.HEADER_BYTES, counts[lo + i], fmt)
            at = slice(len(order), len(order) + len(idx))
            gains = None
            if loudness is not None:
                level, _, gains = M.loudness_gain(src.reshape(len(idx), pitch), out_rate, [counts[lo + i] for i in idx], loudness, peak)
                measured[at].copy_(level)
                applied[at].copy_(gains)
            C.rows_to_pcm(src, table, image, clipped[at], gains)
            order.extend(idx)
        host_half[:total].copy_(dev_image[:total], non_blocking=True)
        event = torch.cuda.Event()
        event.record()
    return order, event


def enhance_to_pcm(generator, clips: Sequence[torch.Tensor], *, format: str = "PCM16", input_rate: Optional[int] = None,
                   output_rate: Optional[int] = None, model_rate: int = 16000, max_batch_samples: int = MAX_BATCH_SAMPLES,
                   max_stage_bytes: int = 1 << 30, loudness: Optional[float] = None, peak: float = -1.0):
    """``enhance_clips`` whose results leave the device as the bytes of WAVE files: a generator that yields, group by group,
    ``(indices, image, spans, clipped)``.  ``indices``: the clips of the group, a run of consecutive input positions; ``image``: a pinned
    uint8 host tensor; ``spans[k]``: the ``(start, stop)`` of clip ``indices[k]``'s complete mono file in it (``corpus.wav_header`` and
    the data, ``image[start:stop]`` is what goes to disk); ``clipped[k]``: how many of its samples left the format's range (or were NaN).
    The image is one of two pinned halves: it is valid until the generator is advanced again.

    A file holds what ``enhance_clips`` returns for its clip (``cut_to_valid_length`` long, at ``model_rate``), or, with ``output_rate``
    other than ``model_rate``, ``augment.resample`` of it -- converted as ``eben_pcm_encode_ragged`` states: ``rint(x * 2^(b-1))`` clamped
    for the PCM formats, the bits for FLOAT32, no dither.  Clips, ``input_rate`` and the forwards are ``enhance_clips``'s; each group is
    dealt into ragged batches of its own.  Behind ``forward_ragged`` nothing is unpacked: one encode launch per batch reads the rows of
    the output buffer where they lie (one ``rate.resample_ragged`` launch in front of it when the rate changes) and writes at the clips'
    places of the group's image (``corpus.plan_image``: groups of at most ``max_stage_bytes``, halved when there are several, plus 4
    bytes a file for the counts); one asynchronous copy per group brings image and counts to the host, and the next group's launches are
    queued before the previous copy's event is waited for -- the only wait.  The host writes the headers once the copy has arrived.

    ``loudness`` (LUFS, e.g. -23.0): every file is brought to that integrated loudness (ITU-R BS.1770-4, ``metrics.loudness_gain``) with its
    sample peak held at or below ``peak`` dBFS.  Per batch one measuring call on the rows that are about to be encoded -- behind
    ``rate.resample_ragged`` when there is an ``output_rate``, and at that rate -- whose gains the encode launch reads on the device
    (``eben_pcm_encode_ragged_gain``): no scaled copy, no host wait.  The generator then yields a fifth element, ``levels``:
    ``levels[k] = (measured LUFS, gain as a factor)`` of clip ``indices[k]``, brought over in the counts' copy; a clip without a finite
    loudness (silence, or shorter than 0.4 s) keeps its level, gain 1.  Without ``loudness`` nothing changes: four elements, the same bytes."""
    import numpy as np

    from . import corpus as C

    clips, rated, lengths = _clips_and_lengths(clips, input_rate, model_rate)
    if format not in C.FORMATS:
        raise ValueError(f"enhance_to_pcm: format must be one of {', '.join(C.FORMATS)}, got {format!r}")
    model_rate = int(model_rate)
    out_rate = model_rate if output_rate is None else int(output_rate)
    if out_rate <= 0 or model_rate <= 0:
        raise ValueError(f"enhance_to_pcm: output_rate and model_rate must be positive, got {output_rate} and {model_rate}")
    if loudness is not None:
        loudness, peak = float(loudness), float(peak)
        if not (math.isfinite(loudness) and math.isfinite(peak)):
            raise ValueError(f"enhance_to_pcm: loudness and peak must be finite, got {loudness} LUFS and {peak} dBFS")
        if out_rate % 10:
            raise ValueError(f"enhance_to_pcm: loudness is measured over 100 ms hops, which {out_rate} Hz does not divide into whole samples")
    if not clips:
        return
    ragged.plan(generator, lengths)   # refuses a clip that is too short, by index, before anything runs
    counts = [ragged.cut_length(generator, t) for t in lengths]
    if out_rate != model_rate:
        counts = [resampled_length(t, model_rate, out_rate) for t in counts]
    for i, t in enumerate(counts):
        C.wav_header(out_rate, t, format)   # a file too large for a RIFF header is refused before anything runs
    groups = C.plan_image(counts, format, max_stage_bytes)
    if len(groups) > 1:
        groups = C.plan_image(counts, format, max_stage_bytes // 2)
    n_halves = 2 if len(groups) > 1 else 1
    half = max(g.nbytes + C._up((4 if loudness is None else 12) * (g.hi - g.lo)) for g in groups)
    device = clips[0].device
    with torch.cuda.device(device):
        dev_image = torch.empty(half, dtype=torch.uint8, device=device)   # one: a group's launches follow the previous copy in stream order
        host = torch.empty(n_halves * half, dtype=torch.uint8, pin_memory=True)
    fmt = C.FORMATS.index(format)

    def arrived(group, h, order, event):
        event.synchronize()   # the copy that filled this half has finished (a copy's event, never a kernel's)
        n = group.hi - group.lo
        image = host[h * half:h * half + group.nbytes]
        view = image.numpy()
        spans = []
        for k, start in enumerate(group.starts):
            t = counts[group.lo + k]
            view[start:start + C.HEADER_BYTES] = np.frombuffer(C.wav_header(out_rate, t, format), dtype=np.uint8)
            spans.append((start, start + C.HEADER_BYTES + t * C.BYTES_PER_SAMPLE[format]))
        got = host[h * half + group.nbytes:h * half + group.nbytes + 4 * n].numpy().view("<i4")
        clipped = [0] * n
        for pos, i in enumerate(order):
            clipped[i] = int(got[pos])
        if loudness is None:
            return list(range(group.lo, group.hi)), image, spans, clipped
        tail = host[h * half + group.nbytes + 4 * n:h * half + group.nbytes + 12 * n].numpy().view("<f4")
        levels = [(0.0, 1.0)] * n
        for pos, i in enumerate(order):
            levels[i] = (float(tail[pos]), float(tail[n + pos]))
        return list(range(group.lo, group.hi)), image, spans, clipped, levels

    pending = None
    for g, group in enumerate(groups):
        h = g % n_halves
        order, event = _encode_group(generator, clips, lengths, counts, group, fmt, rated, input_rate, model_rate, out_rate, max_batch_samples,
                                     dev_image, host[h * half:(h + 1) * half], loudness, peak)
        if pending is not None:
            yield arrived(*pending)
        pending = (group, h, order, event)
    yield arrived(*pending)


def resampled_length(length: int, orig_freq: int, new_freq: int) -> int:
    """Samples ``augment.resample`` returns for a signal of ``length``: ceil(new * length / orig) over the reduced ratio, in integers."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    return -(-new * int(length) // orig)


def _zero_behind(x: torch.Tensor, lengths: Sequence[int]) -> None:
    """``x`` (rows, l_buf): exact zeros behind ``lengths[r]`` in every row, in place (one launch)."""
    from ._lib import check, load, ptr, stream

    rows, l_buf = x.shape
    lens = torch.tensor(list(lengths), dtype=torch.int32).to(x.device, non_blocking=True)
    check(load().eben_edge_zero(ptr(x), lens.data_ptr(), rows, 1, l_buf, stream()), "edge_zero")


def _check_clip(c, what: str) -> None:
    if not torch.is_tensor(c) or c.dim() not in (1, 2, 3) or c.numel() != c.shape[-1] or c.dtype is not torch.float32:
        got = f"{c.dtype} {tuple(c.shape)}" if torch.is_tensor(c) else type(c).__name__
        raise ValueError(f"{what}: expected a float32 tensor of shape (T,), (1, T) or (1, 1, T), got {got}")


@dataclasses.dataclass(frozen=True)
class LossTerms:
    """The losses ``evaluate_clips`` takes per clip, as ``EBENLightningModule.compute_atomic_losses`` takes them per batch: the
    module's ``discriminator`` and its four loss functions, any of which may be None (its term is then left out, as there)."""
    discriminator: object = None
    freq_loss: object = None          # MultiResolutionSTFTLoss: "generator/reconstructive_loss_freq"
    time_loss: object = None          # any callable (enhanced, reference) -> scalar, row by row: "generator/reconstructive_loss_temp"
    feature_loss: object = None       # FeatureLossForDiscriminatorMelganMultiScales: "generator/feature_matching_loss"
    adversarial_loss: object = None   # HingeLossForDiscriminatorMelganMultiScales: "generator/adv_loss_gen", "discriminator/real_loss", "/fake_loss"

    def __post_init__(self):
        from .torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
        from .torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
        from .torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
        from .torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

        for name, kind in (("discriminator", DiscriminatorEBENMultiScales), ("freq_loss", MultiResolutionSTFTLoss),
                           ("feature_loss", FeatureLossForDiscriminatorMelganMultiScales),
                           ("adversarial_loss", HingeLossForDiscriminatorMelganMultiScales)):
            value = getattr(self, name)
            if value is not None and not isinstance(value, kind):
                raise ValueError(f"LossTerms: {name} must be this package's {kind.__name__} (or None), got {type(value).__name__}: per-clip values "
                                 "exist for these classes only")
        if self.time_loss is not None and not callable(self.time_loss):
            raise ValueError(f"LossTerms: time_loss must be callable, got {type(self.time_loss).__name__}")
        if (self.feature_loss is not None or self.adversarial_loss is not None) and self.discriminator is None:
            raise ValueError("LossTerms: feature_loss and adversarial_loss need the discriminator")

    def keys(self) -> List[str]:
        """The result keys, in the order ``compute_atomic_losses`` yields the terms: the generator's, then the discriminator's."""
        out = [f"generator/{name}" for name, fn in (("reconstructive_loss_freq", self.freq_loss), ("reconstructive_loss_temp", self.time_loss),
                                                    ("feature_matching_loss", self.feature_loss), ("adv_loss_gen", self.adversarial_loss))
               if fn is not None]
        return out + (["discriminator/real_loss", "discriminator/fake_loss"] if self.adversarial_loss is not None else [])


def _batch_losses(terms: LossTerms, generator, plan, enh: torch.Tensor, bnd: torch.Tensor, ref: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The terms of one ragged batch, (rows,) each: ``enh`` (rows, 1, l_buf) and ``bnd`` as ``forward_ragged`` returned them, ``ref`` the
    references packed alike.  The enhanced and the reference branch go through the discriminator stacked as 2 x rows."""
    from . import ops

    rows, cut = len(plan.cut), list(plan.cut)
    out: Dict[str, torch.Tensor] = {}
    stft = fm = hinge = None
    if terms.freq_loss is not None:
        stft = terms.freq_loss.ragged_sums(enh, ref, cut)
    if terms.feature_loss is not None or terms.adversarial_loss is not None:
        disc = terms.discriminator
        ref_bands = generator.pqmf.forward(ref, "analysis")   # zero behind a row is the bank's own zero padding
        band_lengths = list(plan.row_lengths[1])
        dplan = ragged.disc_plan(disc, cut * 2, band_lengths * 2, plan.l_buf, bnd.shape[2])
        emb, lens = disc.forward_ragged(torch.cat((bnd, ref_bands), dim=0), torch.cat((enh, ref), dim=0), dplan)
        if terms.feature_loss is not None:
            pairs = [(scale[lv][:rows], scale[lv][rows:], ln[lv][:rows]) for scale, ln in zip(emb, lens) for lv in range(1, len(scale) - 1)]
            fm = (ops.fm_sums_rows(pairs, rows), 1.0 / (len(emb) * len(emb[-1][1:-1])))   # feature_loss.py's own count
        if terms.adversarial_loss is not None:
            hinge = ops.hinge_rows([(x, target, ln[-1][:rows]) for scale, ln in zip(emb, lens)
                                    for x, target in ((scale[-1][:rows], 1.0), (scale[-1][rows:], 1.0), (scale[-1][:rows], -1.0))], rows)
    if stft is not None or fm is not None or hinge is not None:
        values = ops.clip_losses(rows, enh.device, stft=stft, fm=fm, hinge=hinge)
        for k, (key, have) in enumerate((("generator/reconstructive_loss_freq", stft), ("generator/feature_matching_loss", fm),
                                         ("generator/adv_loss_gen", hinge), ("discriminator/real_loss", hinge), ("discriminator/fake_loss", hinge))):
            if have is not None:
                out[key] = values[k]
    if terms.time_loss is not None:
        out["generator/reconstructive_loss_temp"] = torch.stack(
            [terms.time_loss(enh[r : r + 1, :, :t], ref[r : r + 1, :, :t]).reshape(()).to(torch.float32) for r, t in enumerate(cut)])
    return out


@torch.no_grad()
def evaluate_clips(generator, corrupted: Sequence[torch.Tensor], reference: Sequence[torch.Tensor], *, sample_rate: int = EVAL_RATE,
                   max_batch_samples: int = MAX_BATCH_SAMPLES, return_enhanced: bool = False,
                   metrics: Sequence[str] = DEFAULT_EVAL_METRICS, lsd_hf_cutoff_hz: Optional[float] = None,
                   loss_terms: Optional[LossTerms] = None, input_rate: Optional[int] = None,
                   sdr_filter_length: int = 512) -> Dict[str, object]:
    """Per-clip SI-SDR and STOI of the enhanced ``corrupted[i]`` against ``reference[i]``, at 16 kHz as ``base_se.py`` logs them:
    ``{"si_sdr": (N,) float32, "stoi": (N,) float32}`` on the device, in input order; with ``return_enhanced`` also ``"enhanced"``, the
    list ``enhance_clips`` returns.  ``metrics`` selects among ``EVAL_METRICS``, one key each, all on the same 16 kHz buffers and lengths;
    ``"lsd_hf"`` is the LSD over ``[lsd_hf_cutoff_hz, 8000]`` Hz (Nyquist bin excluded) and needs that cutoff -- it depends on the sensor.
    ``"stoi"`` and ``"estoi"`` together share one resampling / silence-removal / band-envelope run.  ``"sdr"`` (``EVAL_METRICS_FILTERED``)
    is the BSS-eval SDR, which allows the enhanced clip a distortion filter of ``sdr_filter_length`` taps (1 to 512): one ``metrics.sdr``
    call per batch on the same buffers and lengths.  ``EVAL_METRICS_FRAMED`` (``"seg_snr"``, ``"fw_seg_snr"``, ``"llr"``, ``"cd"``) are the
    frame-based measures of ``metrics.speech_measures``: one call per batch for those named; a clip needs 600 samples at 16 kHz after the cut.
    ``"lufs_diff"`` (``EVAL_METRICS_LEVEL``) is the enhanced clip's integrated loudness minus its reference's, in LU.
    Clips as for ``enhance_clips``; a pair has one length, and both are scored on their first
    ``cut_to_valid_length`` samples (a reference may carry anything behind them).  Batches as in ``enhance_clips``: per batch one
    ``forward_ragged`` and the metric kernels with ``lengths = plan.cut`` on the padded buffers -- nothing is unpacked unless
    ``return_enhanced`` asks for it, and nothing here waits for the device.

    With ``loss_terms`` the same batch loop also yields the atomic losses ``test_step`` logs, per clip: keys ``"generator/<name>"`` and
    ``"discriminator/<name>"`` (``LossTerms.keys()``: the terms ``compute_atomic_losses`` would produce for that configuration), each
    (N,) float32 on the device in input order, each value what the clip's own batch of one gives.  They are taken at the model's rate
    on the cut clips.  The batches are then planned with the margin the discriminators and the STFT need behind a row
    (``ragged.loss_margin``); a clip too short for the discriminator's or the STFT's own call is refused by index before anything runs.

    ``input_rate``: both clips of every pair are at that rate, and ``sample_rate`` stays the model's.  Per batch two
    ``rate.resample_ragged`` launches bring them to ``sample_rate`` in the padded buffers; every value is the one this call gives on
    the pairs resampled beforehand with ``augment.resample``."""
    from . import metrics as M

    names = list(metrics)
    for name in names:
        if name not in EVAL_METRICS + EVAL_METRICS_FILTERED + EVAL_METRICS_FRAMED + EVAL_METRICS_LEVEL:
            known = EVAL_METRICS + EVAL_METRICS_FILTERED + EVAL_METRICS_FRAMED + EVAL_METRICS_LEVEL
            raise ValueError(f"evaluate_clips: unknown metric {name!r}; known: {', '.join(known)}")
    if len(set(names)) != len(names):
        raise ValueError(f"evaluate_clips: a metric is named twice in {names}")
    if not names:
        raise ValueError("evaluate_clips: no metric requested")
    if "lsd_hf" in names and lsd_hf_cutoff_hz is None:
        raise ValueError("evaluate_clips: 'lsd_hf' needs lsd_hf_cutoff_hz, the lower edge of the band being reconstructed (there is no default: "
                         "it depends on the sensor)")
    sdr_taps = M.sdr_filter_length(sdr_filter_length, "evaluate_clips: sdr_filter_length") if "sdr" in names else None
    lsd_bands = [None] * ("lsd" in names) + [(lsd_hf_cutoff_hz, EVAL_RATE // 2)] * ("lsd_hf" in names)
    for band in lsd_bands:
        M.lsd_band_bins(band, EVAL_RATE, LSD_N_FFT)   # a cutoff that leaves no bin is refused before anything runs
    corrupted, reference = list(corrupted), list(reference)
    if len(corrupted) != len(reference):
        raise ValueError(f"evaluate_clips: {len(corrupted)} corrupted clips and {len(reference)} references")
    for i, (c, g) in enumerate(zip(corrupted, reference)):
        _check_clip(c, f"corrupted clip {i}")
        _check_clip(g, f"reference clip {i}")
        if c.shape[-1] != g.shape[-1]:
            raise ValueError(f"pair {i}: the corrupted clip has {c.shape[-1]} samples, its reference {g.shape[-1]}")
    sample_rate = int(sample_rate)
    if sample_rate <= 0:
        raise ValueError(f"evaluate_clips: sample_rate must be positive, got {sample_rate}")
    rated = _rated(input_rate, sample_rate)
    lengths = [resampled_length(c.shape[-1], input_rate, sample_rate) if rated else c.shape[-1] for c in corrupted]   # at the model's rate
    min_margin = 0
    if loss_terms is not None:
        if not isinstance(loss_terms, LossTerms):
            raise ValueError(f"evaluate_clips: loss_terms must be a LossTerms, got {type(loss_terms).__name__}")
        uses_disc = loss_terms.feature_loss is not None or loss_terms.adversarial_loss is not None
        # the slack the discriminators' deepest layers and the STFT's reflect padding read behind a row
        min_margin = ragged.loss_margin(loss_terms.discriminator if uses_disc else None, generator.pqmf.decimation, loss_terms.freq_loss)
    batches, back = ragged.compose_batches(generator, lengths, max_batch_samples, min_margin)   # refuses a clip that is too short, by index
    if loss_terms is not None:   # and the clips the discriminator's or the STFT's own batch-1 call would refuse, before anything runs
        cuts = [ragged.cut_length(generator, t) for t in lengths]
        if uses_disc:
            n, m = generator.pqmf.kernel_size, generator.pqmf.decimation
            ragged.disc_plan(loss_terms.discriminator, cuts, [(t + n - 2) // m + 1 for t in cuts])
        if loss_terms.freq_loss is not None:
            pad = ragged.loss_margin(None, 1, loss_terms.freq_loss)
            for i, t in enumerate(cuts):
                if t < pad + 1:
                    raise ValueError(f"clip {i} ({t} samples after cut_to_valid_length) is too short: the STFT reflect-pads {pad} samples")
    if lsd_bands:
        for i, t in enumerate(lengths):
            t16 = resampled_length(ragged.cut_length(generator, t), sample_rate, EVAL_RATE)   # the cut length itself at 16 kHz
            if t16 <= LSD_N_FFT // 2:
                raise ValueError(f"clip {i}: {t16} samples at {EVAL_RATE} Hz cannot be reflect-padded for the LSD ({LSD_N_FFT // 2 + 1} at least)")
    framed = [name for name in names if name in EVAL_METRICS_FRAMED]
    if framed:
        w, hop = M.measures_geometry(EVAL_RATE)[:2]
        for i, t in enumerate(lengths):
            t16 = resampled_length(ragged.cut_length(generator, t), sample_rate, EVAL_RATE)
            if t16 < w + hop:
                raise ValueError(f"clip {i}: {t16} samples at {EVAL_RATE} Hz hold no frame of the frame-based measures ({w + hop} at least)")
    values: Dict[str, List[torch.Tensor]] = {name: [] for name in names}
    enhanced: List[torch.Tensor] = []
    losses: Dict[str, List[torch.Tensor]] = {key: [] for key in (loss_terms.keys() if loss_terms is not None else ())}
    for idx in batches:
        plan = ragged.plan(generator, [lengths[i] for i in idx], min_margin)
        dev = corrupted[idx[0]].device
        if rated:
            buf = _resampled_rows(corrupted, idx, plan.l_buf, input_rate, sample_rate)[:, :, : plan.l_buf].contiguous()
            ref = _resampled_rows(reference, idx, plan.l_buf, input_rate, sample_rate)[:, 0, : plan.l_buf].contiguous()
            _zero_behind(ref, plan.cut)   # a reference ends at its cut length, like its row of the forward
        else:
            buf = torch.zeros((len(idx), 1, plan.l_buf), dtype=torch.float32, device=dev)
            ref = torch.zeros((len(idx), plan.l_buf), dtype=torch.float32, device=dev)
            for r, i in enumerate(idx):
                buf[r, 0, : plan.cut[r]].copy_(corrupted[i].reshape(-1)[: plan.cut[r]])
                ref[r, : plan.cut[r]].copy_(reference[i].reshape(-1)[: plan.cut[r]])
        if loss_terms is None:
            enh, _ = generator.forward_ragged(buf, [lengths[i] for i in idx])   # zero behind every row, like ref
        else:   # the same forward on this batch's wider plan (forward_ragged would plan the batch with the generator's own margin)
            from . import gen_engine

            enh, bnd = gen_engine.engine_of(generator).forward_ragged(buf, plan)
            # the losses at the model's rate on the cut clips, as test_step takes them; resampling is for the metrics
            for key, row in _batch_losses(loss_terms, generator, plan, enh, bnd, ref.reshape(len(idx), 1, plan.l_buf)).items():
                losses[key].append(row)
        if return_enhanced:
            for r, i in enumerate(idx):
                enhanced.append(enh[r, 0, : plan.cut[r]].reshape(corrupted[i].shape[:-1] + (plan.cut[r],)).clone())
        enh, rows = enh.reshape(len(idx), plan.l_buf), plan.cut
        if sample_rate != EVAL_RATE:
            from .augment import resample

            # the resampler's taps reach a few samples past a row's end: they find the zeros the row alone is padded with
            enh, ref = resample(enh, sample_rate, EVAL_RATE), resample(ref, sample_rate, EVAL_RATE)
            rows = [resampled_length(t, sample_rate, EVAL_RATE) for t in rows]
        lens = torch.tensor(rows, dtype=torch.int32).to(dev, non_blocking=True)   # 1 <= each <= the buffer's length by construction
        if "si_sdr" in values:
            values["si_sdr"].append(M.si_sdr(enh, ref, lens))
        if "stoi" in values and "estoi" in values:
            classic, extended = M.stoi_and_estoi(enh, ref, EVAL_RATE, lens)
            values["stoi"].append(classic)
            values["estoi"].append(extended)
        elif "stoi" in values:
            values["stoi"].append(M.stoi(enh, ref, EVAL_RATE, lens))
        elif "estoi" in values:
            values["estoi"].append(M.stoi(enh, ref, EVAL_RATE, lens, extended=True))
        if "si_snr" in values:
            values["si_snr"].append(M.si_snr(enh, ref, lens))
        if "snr" in values:
            values["snr"].append(M.snr(enh, ref, lens))
        if lsd_bands:
            both = M.lsd(enh, ref, EVAL_RATE, lens, LSD_N_FFT, LSD_HOP, lsd_bands)
            for name, row in zip([n for n in ("lsd", "lsd_hf") if n in values], both):
                values[name].append(row)
        if "sdr" in values:
            values["sdr"].append(M.sdr(enh, ref, lens, filter_length=sdr_taps))
        if framed:
            for name, row in M.speech_measures(enh, ref, EVAL_RATE, lens, framed).items():
                values[name].append(row)
        if "lufs_diff" in values:
            values["lufs_diff"].append(M.integrated_loudness(enh, EVAL_RATE, lens) - M.integrated_loudness(ref, EVAL_RATE, lens))
    order = torch.tensor(back, dtype=torch.int64).to(values[names[0]][0].device, non_blocking=True)
    out: Dict[str, object] = {name: torch.cat(values[name]).index_select(0, order) for name in names}
    for key, rows_of in losses.items():
        out[key] = torch.cat(rows_of).index_select(0, order)
    if return_enhanced:
        out["enhanced"] = [enhanced[p] for p in back]
    return out
