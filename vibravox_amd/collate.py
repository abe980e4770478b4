"""Batch assembly on the device (BASELINE config 4): the BWE and the noisy-BWE collators.

Counterparts of ``BWELightningDataModule.data_collator`` (vibravox/lightning_datamodules/bwe.py:232-293) and
``NoisyBWELightningDataModule.data_collator`` (vibravox/lightning_datamodules/noisybwe.py:219-291)
for clips that already live in HBM: the random noise slice (``mix_speech_and_noise_without_rescaling``,
vibravox/utils.py:195-254, or the SNR-controlled ``mix_speech_and_noise_with_rescaling``, utils.py:118-193), the
addition and the crop / pad to a constant length (``set_audio_duration`` / ``pad_audio``, utils.py:7-81) are ONE gather
kernel (``eben_noisy_collate`` / ``eben_noisy_collate_scaled``) instead of a per-item Python loop on
the host.  The random draws are taken from the CPU generator with the reference's calls, in the reference's
order (all mixing draws first, then the crop offsets, then the augmentation's), so the same ``torch.manual_seed`` selects
the same samples as the reference collator.  The default augmentation of noisybwe.yaml:17 is the identity.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import EbenClip, EbenCollateItem, EbenError, check, load, ptr, stream


def _crop_plan(lengths: List[int], samples_or_none, deterministic: bool) -> Tuple[int, List[int]]:
    """(output length T, shift per item): the crop / pad of ``set_audio_duration`` (utils.py:50-81), one draw per item that is cropped
    at random, in item order."""
    if samples_or_none is None:                                          # collate_strategy == "pad"
        return max(lengths), [0] * len(lengths)
    t = int(samples_or_none)
    shifts = []
    for ls in lengths:
        if ls >= t:
            shifts.append((ls - t) // 2 if deterministic else int(torch.randint(low=0, high=ls - t + 1, size=(1,))))   # utils.py:71-73
        else:
            shifts.append(-(t - ls // 2))                                # pad_audio's left run, utils.py:23 (sic)
    return t, shifts


def plan_noisy_bwe(lengths: List[int], noise_lengths: List[int], samples_or_none, deterministic: bool) -> Tuple[int, List[Tuple[int, int, int]]]:
    """Host-side part of the collator: (output length T, [(length, noise_start, shift)] per item), drawing the
    random numbers exactly as the reference does."""
    starts = []
    for ls, ln in zip(lengths, noise_lengths):
        if ln < ls:
            raise ValueError(f"noise_sample length ({ln}) must be >= speech_sample length ({ls})")
        starts.append(int(torch.randint(0, ln - ls, (1,))))            # utils.py:245
    t, shifts = _crop_plan(lengths, samples_or_none, deterministic)
    return t, [(ls, st, sh) for ls, st, sh in zip(lengths, starts, shifts)]


def plan_bwe(lengths: List[int], samples_or_none, deterministic: bool) -> Tuple[int, List[Tuple[int, int]]]:
    """Host-side part of the BWE collator (bwe.py:256-281): (output length T, [(length, shift)] per item).  T is the longest clip
    under ``"pad"`` (``samples_or_none`` None), else ``samples``; ONE ``torch.randint`` per cropped item serves both clips
    (``set_audio_duration``, utils.py:69-79), in item order."""
    t, shifts = _crop_plan(lengths, samples_or_none, deterministic)
    return t, list(zip(lengths, shifts))


def plan_snr_mix(lengths: List[int], noise_lengths: List[int], snr_range: Sequence[float]) -> Tuple[List[int], torch.Tensor]:
    """The draws of ``mix_speech_and_noise_with_rescaling`` (utils.py:160-183): per item ``torch.randint(0, ln - ls, (1,))`` then
    ``torch.empty(1).uniform_(lo, hi)``.  Returns (noise starts, snr_linear (n,) float32 on the host); ``10 ** (snr / 10.0)`` is
    formed here with torch in float32 -- the reference's value exactly, no device ``pow`` to drift from it."""
    starts, snrs = [], []
    for ls, ln in zip(lengths, noise_lengths):
        if ln < ls:
            raise ValueError(f"noise_sample length ({ln}) must be >= speech_sample length ({ls})")
        starts.append(int(torch.randint(0, ln - ls, (1,))))            # utils.py:178
        snr = torch.empty(1).uniform_(snr_range[0], snr_range[1])        # utils.py:182
        snrs.append(10 ** (snr / 10.0))                                  # utils.py:183
    return starts, torch.cat(snrs) if snrs else torch.empty(0)


def samples_of(collate_strategy: str, sample_rate: int) -> Optional[int]:
    """None for ``"pad"``, else the sample count of ``"constant_length-XXX-ms"`` (bwe.py:266-267)."""
    return None if collate_strategy == "pad" else int(sample_rate * int(collate_strategy.split("-")[1]) / 1000)


def clip_powers(clips: List[torch.Tensor]) -> torch.Tensor:
    """Mean square of each 1-D float32 device clip as a (n,) float32 device tensor (``torch.mean(x ** 2)``, utils.py:163-164, with the
    sum kept in float64): ``eben_clip_powers``, no host read."""
    lib = load()
    n = len(clips)
    table = (EbenClip * n)()
    for i, c in enumerate(clips):
        if c.shape[0] < 1:
            raise ValueError("the power of an empty clip is undefined")
        table[i] = EbenClip(ptr(c), c.shape[0])
    dev = clips[0].device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    nbytes = lib.eben_clip_powers_workspace(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    check(lib.eben_clip_powers(table, n, ptr(out), ws.data_ptr(), nbytes, stream()), "clip_powers")
    return out


def _check_1d(speech: List[torch.Tensor], noise: Optional[List[torch.Tensor]] = None) -> None:
    for tns in speech:
        if tns.dim() != 1:
            raise ValueError(f"Each speech sample must be a 1D tensor, but got shape {tuple(tns.shape)}")
    for tns in noise or ():
        if tns.dim() != 1:
            raise ValueError(f"Each noise sample must be a 1D tensor, but got shape {tuple(tns.shape)}")


def _scaled_collate(body, air, noise, plan, t, snr_linear, want_noise: bool):
    """eben_clip_powers on speech and WHOLE noise clips (utils.py:163-164), then eben_noisy_collate_scaled."""
    lib = load()
    n = len(body)
    dev = body[0].device
    powers = clip_powers(list(body) + list(noise))
    snr_dev = snr_linear.to(dev, non_blocking=False)
    table = (EbenCollateItem * n)()
    for i, (ls, st, sh) in enumerate(plan):
        table[i] = EbenCollateItem(ptr(body[i]), ptr(air[i]) if air is not None else None, ptr(noise[i]), ls, st, sh)
    bc = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
    ab = torch.empty((n, 1, t), dtype=torch.float32, device=dev) if air is not None else None
    ns = torch.empty((n, 1, t), dtype=torch.float32, device=dev) if want_noise else None
    check(lib.eben_noisy_collate_scaled(table, n, t, ptr(powers[:n]), ptr(powers[n:]), ptr(snr_dev), ptr(bc), ptr(ab), ptr(ns), stream()),
          "noisy_collate_scaled")
    return bc, ab, ns


def mix_speech_and_noise_with_rescaling(speech_batch: List[torch.Tensor], noise_batch: List[torch.Tensor],
                                        snr_range: Sequence[float] = (-3.0, 5.0)) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """``vibravox.utils.mix_speech_and_noise_with_rescaling`` (utils.py:118-193) for lists of 1-D float32 DEVICE tensors: returns
    (corrupted speech list, scaled noise list), each item as long as its speech clip.  Same checks, same draws on the CPU generator
    (per item ``randint`` then ``uniform_``); ``noise_power`` is the mean square of the whole noise clip, not of the slice."""
    if not isinstance(speech_batch, list) or not all(isinstance(t, torch.Tensor) for t in speech_batch):
        raise TypeError("speech_batch must be a list of torch.Tensor")
    if not isinstance(noise_batch, list) or not all(isinstance(t, torch.Tensor) for t in noise_batch):
        raise TypeError("noise_batch must be a list of torch.Tensor")
    if len(speech_batch) != len(noise_batch):
        raise ValueError("speech_batch and noise_batch must have the same length")
    if not speech_batch:
        return [], []
    _check_1d(speech_batch, noise_batch)
    lengths = [x.shape[0] for x in speech_batch]
    starts, snr_linear = plan_snr_mix(lengths, [x.shape[0] for x in noise_batch], snr_range)
    t = max(lengths)
    bc, _, ns = _scaled_collate(speech_batch, None, noise_batch, [(ls, st, 0) for ls, st in zip(lengths, starts)], t, snr_linear, True)
    return [bc[i, 0, :ls] for i, ls in enumerate(lengths)], [ns[i, 0, :ls] for i, ls in enumerate(lengths)]


def _augment(data_augmentation, deterministic: bool, bc: torch.Tensor, ab: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bwe.py:284-288 / noisybwe.py:284-286: after every collate draw, only when ``deterministic is False``."""
    if deterministic is False and data_augmentation is not None:
        with torch.no_grad():
            bc, ab = data_augmentation(bc, ab)
    return bc, ab


def bwe_collate(batch: List[Dict[str, torch.Tensor]], sample_rate: int, collate_strategy: str = "pad", deterministic: bool = False,
                data_augmentation=None) -> Dict[str, torch.Tensor]:
    """``batch``: dicts of 1-D float32 DEVICE tensors ``audio_body_conducted`` and ``audio_airborne``.  Returns the (B, 1, T) tensors
    of the reference's default collator (bwe.py:232-293): ``eben_noisy_collate`` without a noise clip, then the augmentation."""
    lib = load()
    body = [item["audio_body_conducted"] for item in batch]
    air = [item["audio_airborne"] for item in batch]
    _check_1d(body)
    for a, b in zip(air, body):
        if a.shape != b.shape:                                           # set_audio_duration's assert, utils.py:67
            raise EbenError("audio_airborne and audio_body_conducted must have the same length")
    n = len(batch)
    t, plan = plan_bwe([x.shape[0] for x in body], samples_of(collate_strategy, sample_rate), deterministic)
    table = (EbenCollateItem * n)()
    for i, (ls, sh) in enumerate(plan):
        table[i] = EbenCollateItem(ptr(body[i]), ptr(air[i]), None, ls, 0, sh)
    dev = body[0].device
    bc = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
    ab = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
    check(lib.eben_noisy_collate(table, n, t, ptr(bc), ptr(ab), stream()), "bwe_collate")
    bc, ab = _augment(data_augmentation, deterministic, bc, ab)
    return {"audio_body_conducted": bc, "audio_airborne": ab}


def noisy_bwe_collate(batch: List[Dict[str, torch.Tensor]], sample_rate: int, collate_strategy: str = "pad",
                      deterministic: bool = False, snr_range: Optional[Sequence[float]] = None, data_augmentation=None) -> Dict[str, torch.Tensor]:
    """``batch``: dicts of 1-D float32 DEVICE tensors ``audio_body_conducted`` [, ``audio_airborne``,
    ``audio_body_conducted_speechless_noisy``].  Returns the (B, 1, T) tensors of the reference collator.

    ``snr_range`` None (default): the noise is mixed in at its recorded level, as the reference collator does
    (``mix_speech_and_noise_without_rescaling``).  ``snr_range=(lo, hi)``: the reference's SNR-controlled mixer
    (``mix_speech_and_noise_with_rescaling``) takes its place -- per item ``[randint, uniform_]``, then the crop draws."""
    lib = load()
    body = [item["audio_body_conducted"] for item in batch]
    _check_1d(body)
    dev = body[0].device
    n = len(batch)
    table = (EbenCollateItem * n)()
    if "audio_airborne" not in batch[0]:
        t = max(x.shape[0] for x in body)
        for i, x in enumerate(body):
            table[i] = EbenCollateItem(ptr(x), None, None, x.shape[0], 0, 0)
        out = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
        check(lib.eben_noisy_collate(table, n, t, ptr(out), None, stream()), "noisy_collate")
        return {"audio_body_conducted": out}
    air = [item["audio_airborne"] for item in batch]
    noise = [item["audio_body_conducted_speechless_noisy"] for item in batch]
    for a, b in zip(air, body):
        if a.shape != b.shape:
            raise EbenError("audio_airborne and audio_body_conducted must have the same length")
    samples = samples_of(collate_strategy, sample_rate)
    lengths = [x.shape[0] for x in body]
    if snr_range is None:
        t, plan = plan_noisy_bwe(lengths, [x.shape[0] for x in noise], samples, deterministic)
        for i, (ls, st, sh) in enumerate(plan):
            table[i] = EbenCollateItem(ptr(body[i]), ptr(air[i]), ptr(noise[i]), ls, st, sh)
        bc = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
        ab = torch.empty((n, 1, t), dtype=torch.float32, device=dev)
        check(lib.eben_noisy_collate(table, n, t, ptr(bc), ptr(ab), stream()), "noisy_collate")
    else:
        _check_1d([], noise)
        starts, snr_linear = plan_snr_mix(lengths, [x.shape[0] for x in noise], snr_range)
        t, shifts = _crop_plan(lengths, samples, deterministic)
        bc, ab, _ = _scaled_collate(body, air, noise, list(zip(lengths, starts, shifts)), t, snr_linear, False)
    bc, ab = _augment(data_augmentation, deterministic, bc, ab)
    return {"audio_body_conducted": bc, "audio_airborne": ab}
