"""Enhancing a corpus: utterances of any lengths through a trained EBEN generator in ragged batches.

What the reference does clip by clip (``scripts/eben_enhanced_vibravox.py``: ``cut_to_valid_length``, one batch-1 forward each) runs
here as a few batched forwards: the clips are sorted by length, dealt into batches of at most ``max_batch_samples`` buffer samples and
each batch goes through ``EBENGenerator.forward_ragged`` -- every clip's result is the one its own forward gives.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from . import ragged

#: buffer samples (rows x padded length) per batch: 262 s at 16 kHz.  The widest activations (32 channels at 1/4 of the audio rate,
#: 64 at 1/8) take 32 bytes per audio sample each, 128 MiB a tensor at this budget
MAX_BATCH_SAMPLES = 1 << 22


#: samples per push of ``enhance_stream``: about a second at 16 kHz, a whole number of latent frames for every bank
STREAM_CHUNK = 16384


@torch.no_grad()
def enhance_stream(generator, clip: torch.Tensor, chunk_samples: int = STREAM_CHUNK):
    """One long ``clip`` (rows, 1, T) through a ``streaming.StreamingEnhancer`` in pushes of ``chunk_samples``: the activations alive at
    any time are those of one chunk plus the stream state, not those of the whole recording.  Returns what
    ``generator(generator.cut_to_valid_length(clip))`` returns, (enhanced (rows, 1, T'), bands (rows, m, L)).  Nothing here waits for
    the device."""
    from . import streaming

    if clip.dim() != 3 or clip.shape[1] != 1 or clip.dtype is not torch.float32:
        raise ValueError(f"enhance_stream: expected a float32 (rows, 1, T) tensor, got {clip.dtype} {tuple(clip.shape)}")
    rows, _, total = clip.shape
    m = generator.pqmf.decimation
    ragged.plan(generator, [total])   # refuses a clip below the shortest one before anything runs
    cut = ragged.cut_length(generator, total)
    enhancer = streaming.StreamingEnhancer(generator, chunk_samples, streams=rows, return_bands=True)
    chunk = enhancer.chunk_samples
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


@torch.no_grad()
def enhance_clips(generator, clips: Sequence[torch.Tensor], *, max_batch_samples: int = MAX_BATCH_SAMPLES, return_bands: bool = False):
    """``clips``: 1-D, (1, T) or (1, 1, T) float32 tensors on the generator's device.  Returns the enhanced clips in input order, each
    ``cut_to_valid_length`` long and of its clip's rank; with ``return_bands`` also the list of their (m, L) enhanced bands.  Nothing
    here waits for the device: packing and unpacking are copies on the current stream."""
    clips = list(clips)
    for i, c in enumerate(clips):
        if c.dim() not in (1, 2, 3) or c.numel() != c.shape[-1] or c.dtype is not torch.float32:
            raise ValueError(f"clip {i}: expected a float32 tensor of shape (T,), (1, T) or (1, 1, T), got {c.dtype} {tuple(c.shape)}")
    lengths = [c.shape[-1] for c in clips]
    batches, back = ragged.compose_batches(generator, lengths, max_batch_samples)
    enhanced: List[torch.Tensor] = []
    bands: List[torch.Tensor] = []
    for idx in batches:
        plan = ragged.plan(generator, [lengths[i] for i in idx])
        buf = torch.zeros((len(idx), 1, plan.l_buf), dtype=torch.float32, device=clips[idx[0]].device)
        for r, i in enumerate(idx):
            buf[r, 0, : plan.cut[r]].copy_(clips[i].reshape(-1)[: plan.cut[r]])
        enh, bnd = generator.forward_ragged(buf, [lengths[i] for i in idx])
        for r, i in enumerate(idx):
            enhanced.append(enh[r, 0, : plan.cut[r]].reshape(clips[i].shape[:-1] + (plan.cut[r],)).clone())
            if return_bands:
                bands.append(bnd[r, :, : plan.row_lengths[1][r]].clone())
    enhanced = [enhanced[p] for p in back]
    return (enhanced, [bands[p] for p in back]) if return_bands else enhanced
