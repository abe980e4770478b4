"""CPU: the host side of the per-clip augmentation (``WaveformDataAugmentation(per_clip=True)``) -- the band tables against
``sinc_resample_kernel``'s full tables bit for bit, ``plan_per_clip``'s draws against the batch-level ``forward``'s, and the
refusals of the four C entries of ``csrc/augment_clips.hip`` (no launch is reached, so no GPU is needed)."""
import ctypes
import math
import os

import pytest
import torch

from vibravox_amd import augment
from vibravox_amd._lib import EbenClipBand, EbenMaskClip, EbenOlaClip, EbenResampleClip, EbenVocoderClip

FACTORS = (0.7, 0.8, 0.85, 0.9, 0.95, 1.05, 1.1, 1.15, 1.2, 1.3)
STEPS = (-4, -3, -2, -1, 1, 2, 3, 4, 5, 6)


def bits(t):
    return t.contiguous().view(torch.int32)


def check_band(orig_freq, new_freq):
    full, width, orig, new = augment.sinc_resample_kernel(orig_freq, new_freq)
    b = augment.band_resample_kernel(orig_freq, new_freq)
    assert (b.width, b.orig, b.new) == (width, orig, new) and b.band.shape == (new, b.W) and b.first.shape == (new,)
    assert b.band.dtype == torch.float32 and b.first.dtype == torch.int32
    assert b.W <= 2 * width + 1
    assert int(b.first.min()) >= 0 and int(b.first.max()) + b.W <= full.shape[1]
    idx = b.first.long()[:, None] + torch.arange(b.W)[None, :]
    assert torch.equal(bits(torch.gather(full, 1, idx)), bits(b.band))          # bit for bit inside [first, first + W)
    outside = torch.ones_like(full, dtype=torch.bool).scatter_(1, idx, False)
    assert bool((full[outside] == 0.0).all())                                    # and the full table is exactly 0 outside
    assert bool((b.band != 0).any(dim=1).all())
    return b


@pytest.mark.parametrize("factor", FACTORS)
def test_band_equals_the_full_speed_table(factor):
    b = check_band(int(factor * 16000), 16000)
    assert b.W < 2 * b.width + b.orig


@pytest.mark.parametrize("steps", STEPS)
def test_band_equals_the_full_pitch_table_at_2_khz(steps):
    """At sample_rate 2000 the reduced pitch ratios (4 -> 2519 : 2000, -3 -> 1681 : 2000, ...) give full tables of a few million floats."""
    b = check_band(int(2000 / 2.0 ** (-steps / 12)), 2000)
    assert b.new >= 500 and b.orig > 500


def test_band_equals_the_16_khz_pitch_table_of_steps_minus_3_in_slices():
    """6727 : 8000, the smallest 16 kHz pitch ratio: every phase, 400 at a time, each slice of the full table evaluated with
    ``sinc_resample_kernel``'s own expression on that slice (a 400 x 6741 float64 temporary instead of 8000 x 6741)."""
    orig_freq = int(16000 / 2.0 ** (3 / 12))
    g = math.gcd(orig_freq, 16000)
    assert (orig_freq // g, 16000 // g) == (6727, 8000)
    b = augment.band_resample_kernel(orig_freq, 16000)
    orig, new, lpw = b.orig, b.new, 6
    base = min(orig, new) * 0.99
    width = math.ceil(lpw * orig / base)
    assert (b.width, b.W <= 2 * width + 1, b.band.shape) == (width, True, (new, b.W))
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    phases = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new
    for p0 in range(0, new, 400):
        t = phases[p0:p0 + 400] + idx                                            # augment.sinc_resample_kernel, lines for these phases
        t = (t * base).clamp_(-lpw, lpw)
        window = torch.cos(t * math.pi / lpw / 2) ** 2
        t = t * math.pi
        full = (torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)).to(torch.float32)
        cols = b.first[p0:p0 + 400].long()[:, None] + torch.arange(b.W)[None, :]
        assert torch.equal(bits(torch.gather(full, 1, cols)), bits(b.band[p0:p0 + 400])), p0
        assert bool((full[torch.ones_like(full, dtype=torch.bool).scatter_(1, cols, False)] == 0.0).all()), p0


def test_identity_ratio_is_a_copy():
    b = augment._device_band(16000, 16000, torch.device("cpu"))
    assert (b.orig, b.new, b.width, b.W) == (1, 1, 0, 1) and b.band.tolist() == [[1.0]] and b.first.tolist() == [0]


# ---- the draws ------------------------------------------------------------------------------------------------------------------------
def module(**kw):
    return augment.WaveformDataAugmentation(16000, per_clip=True, **kw)


@pytest.mark.parametrize("two", [False, True])
def test_plan_advances_the_generator_as_one_forward_per_clip_does(monkeypatch, two):
    B, T = 5, 1000
    mod = module(p_data_augmentation=1, p_speed_perturbation=1, p_pitch_shift=1, p_time_masking=1)
    torch.manual_seed(11)
    plan = augment.plan_per_clip(mod, B, T, two)
    state = torch.get_rng_state()
    assert [p.clip for p in plan] == list(range(B))
    for p in plan:
        assert p.factor in mod.speed_perturbation_factors and p.steps in mod.pitch_shift_steps and p.pct in mod.time_masking_percentage
        assert p.masked == int(T * p.pct / 100) and 0 <= p.first_1 < T - p.masked
        assert (p.first_2 is None) != two and (not two or 0 <= p.first_2 < T - p.masked)

    # the batch-level forward on a one-clip CPU stand-in: the transforms keep the length, the mask makes its draw without the kernel
    monkeypatch.setattr(augment, "speed", lambda w, sr, f: w)
    monkeypatch.setattr(augment, "pitch_shift", lambda w, sr, s: w)

    def masking(x, pct):
        t = x.shape[-1]
        drawn.append(torch.randint(0, t - int(t * pct / 100), (1,)).item())
        return x

    monkeypatch.setattr(augment, "time_masking_", masking)
    batch = augment.WaveformDataAugmentation(16000, p_data_augmentation=1, p_speed_perturbation=1, p_pitch_shift=1, p_time_masking=1)
    x = torch.zeros(1, 1, T)
    torch.manual_seed(11)
    for p in plan:
        drawn = []
        batch(x, x.clone() if two else None)
        assert drawn == ([p.first_1, p.first_2] if two else [p.first_1])
    assert torch.equal(torch.get_rng_state(), state)


def test_plan_is_empty_after_one_draw_per_clip_when_augmentation_is_off():
    mod = module(p_data_augmentation=0, p_speed_perturbation=1, p_pitch_shift=1, p_time_masking=1)
    torch.manual_seed(3)
    assert augment.plan_per_clip(mod, 7, 500, True) == []
    state = torch.get_rng_state()
    torch.manual_seed(3)
    for _ in range(7):
        torch.rand(1)
    assert torch.equal(torch.get_rng_state(), state)


def test_plan_differs_across_the_clips_of_a_batch():
    mod = module(p_data_augmentation=0.9, p_speed_perturbation=0.7, p_pitch_shift=0.7, p_time_masking=0.7)
    torch.manual_seed(0)
    plan = augment.plan_per_clip(mod, 32, 4000, True)
    for field in ("factor", "steps", "pct"):
        assert len({getattr(p, field) for p in plan if getattr(p, field) is not None}) >= 3, field
    assert 0 < len(plan) < 32 or any(p.factor is None for p in plan)      # not all clips drew everything
    assert len({(p.factor, p.steps, p.pct) for p in plan}) > 8


def test_forward_on_cpu_keeps_the_batch_and_records_the_plan():
    mod = module(p_data_augmentation=0)
    x = torch.randn(3, 1, 100)
    a, b = mod(x, None)
    assert a is x and b is None and mod.last_plan == []
    assert augment.WaveformDataAugmentation(16000).per_clip is False


def test_per_clip_config_instantiates():
    import yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "lightning_datamodule", "data_augmentation", "per_clip.yaml")))
    assert cfg["_target_"] == "vibravox_amd.augment.WaveformDataAugmentation" and cfg["per_clip"] is True
    kw = {k: (tuple(v["_args_"][0]) if isinstance(v, dict) else v) for k, v in cfg.items() if k not in ("_target_", "sample_rate")}
    mod = augment.WaveformDataAugmentation(16000, **kw)
    assert mod.per_clip and 0 < mod.apply_data_augmentation <= 1


# ---- argument errors, no GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


X, OUT, BAND, FIRST, W2 = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000   # never dereferenced: every call below is refused (or has nothing to do)
V = ctypes.c_void_p
EINVAL = -1


def test_time_mask_clips_argument_errors_without_gpu(lib):
    def call(x=X, rows=4, t=100, clips=((1, 10, 20),), count=None, null_table=False):
        table = None if null_table else (EbenMaskClip * max(1, len(clips)))(*[EbenMaskClip(*c) for c in clips])
        return lib.eben_time_mask_clips(V(x), rows, t, table, len(clips) if count is None else count, None)

    msg = lib.eben_last_error
    assert call(clips=((0, 0, 0), (3, 100, 0))) == 0                                     # nothing to zero: checked, no launch
    assert call(x=0) == EINVAL and b"null" in msg() and call(null_table=True) == EINVAL and b"null" in msg()
    assert call(rows=0) == EINVAL and b"0 rows" in msg() and call(t=0) == EINVAL and call(count=0) == EINVAL and b"0 masks" in msg()
    assert call(x=X + 2) == EINVAL and b"misaligned" in msg()
    assert call(clips=((4, 0, 1),)) == EINVAL and b"row 4 of 4" in msg() and call(clips=((-1, 0, 1),)) == EINVAL
    assert call(clips=((0, 0, 101),)) == EINVAL and b"of 100 samples" in msg()           # count > T
    assert call(clips=((0, 81, 20),)) == EINVAL and call(clips=((0, -1, 2),)) == EINVAL and call(clips=((0, 0, -1),)) == EINVAL
    assert call(clips=((0, 0, 0), (1, 2 ** 31 - 1, 2 ** 31 - 1))) == EINVAL and b"mask 1" in msg()


def test_resample_clips_argument_errors_without_gpu(lib):
    good_band, good_row = (BAND, FIRST, 7, 10, 7, 13), dict(src_offset=0, t_in=100, band=0, dst_row=1)

    def call(x=X, x_floats=400, out=OUT, out_rows=4, t=100, bands=(good_band,), nbands=None, rows=None, count=None, null=None, **change):
        rows = [dict(good_row, **change)] if rows is None else rows
        bt = None if null == "bands" else (EbenClipBand * max(1, len(bands)))(*[EbenClipBand(*b) for b in bands])
        rt = None if null == "rows" else (EbenResampleClip * max(1, len(rows)))(*[EbenResampleClip(reserved=0, **r) for r in rows])
        return lib.eben_resample_clips(V(x), x_floats, V(out), out_rows, t, bt, len(bands) if nbands is None else nbands, rt,
                                       len(rows) if count is None else count, None)

    msg = lib.eben_last_error
    for k in ("x", "out"):
        assert call(**{k: 0}) == EINVAL and b"null" in msg(), k
        assert call(**{k: 0x700002}) == EINVAL and b"misaligned" in msg(), k
    assert call(null="bands") == EINVAL and call(null="rows") == EINVAL and b"null" in msg()
    assert call(count=0) == EINVAL and b"0 rows" in msg() and call(out_rows=0) == EINVAL and call(t=0) == EINVAL and call(x_floats=0) == EINVAL
    assert call(nbands=0) == EINVAL and call(bands=(good_band,) * 17) == EINVAL and b"1..16" in msg()
    assert call(out=X + 4 * 399) == EINVAL and b"overlaps" in msg() and call(x=OUT + 4 * 399) == EINVAL and b"overlaps" in msg()
    assert call(bands=((0, FIRST, 7, 10, 7, 13),)) == EINVAL and b"null table of ratio 0" in msg() and call(bands=((BAND, 0, 7, 10, 7, 13),)) == EINVAL
    for bad in ((BAND, FIRST, 0, 10, 7, 13), (BAND, FIRST, 7, 0, 7, 13), (BAND, FIRST, 7, 10, -1, 13), (BAND, FIRST, 7, 10, 7, 0), (BAND, FIRST, 7, 10, 7, 22)):
        assert call(bands=(bad,)) == EINVAL and b"ratio 0 is" in msg(), bad
    assert call(band=1) == EINVAL and b"ratio 1 of 1" in msg() and call(band=-1) == EINVAL
    assert call(t_in=0) == EINVAL and call(t_in=401) == EINVAL and b"of 400" in msg()     # count > what x holds
    assert call(src_offset=301) == EINVAL and call(src_offset=-1) == EINVAL
    assert call(dst_row=4) == EINVAL and b"row 4 of 4" in msg() and call(dst_row=-1) == EINVAL
    assert call(rows=[good_row, dict(good_row, src_offset=100)]) == EINVAL and b"two rows write row 1" in msg()


def test_phase_vocoder_clips_argument_errors_without_gpu(lib):
    def call(spec=X, out=OUT, bins=257, frames=8, out_cols=20, rows=((1.25, 7, 0), (0.8, 10, 7)), count=None, null_table=False):
        table = None if null_table else (EbenVocoderClip * max(1, len(rows)))(*[EbenVocoderClip(*r) for r in rows])
        return lib.eben_phase_vocoder_clips(V(spec), V(out), bins, frames, out_cols, table, len(rows) if count is None else count, 128.0, None)

    msg = lib.eben_last_error
    assert call(spec=0) == EINVAL and call(out=0) == EINVAL and call(null_table=True) == EINVAL and b"null" in msg()
    assert call(count=0) == EINVAL and b"0 rows" in msg() and call(bins=1) == EINVAL and call(frames=0) == EINVAL and call(out_cols=0) == EINVAL
    assert call(rows=((0.0, 7, 0),)) == EINVAL and b"rate 0" in msg() and call(rows=((float("nan"), 7, 0),)) == EINVAL and call(rows=((1.0, 0, 0),)) == EINVAL
    assert call(rows=((1.25, 7, 0), (0.8, 10, 6))) == EINVAL and b"ascending, disjoint" in msg()      # overlaps the row before
    assert call(rows=((1.25, 7, 0), (0.8, 10, 11))) == EINVAL and b"of 20" in msg()                   # past the output
    assert call(rows=((1.25, 7, -1),)) == EINVAL


def test_overlap_add_clips_argument_errors_without_gpu(lib):
    # 7 frames of 512 at hop 128 cover 1280 samples, 1024 after the 256 of padding
    good = dict(dst_offset=0, col=0, frames_out=7, len_stretch=1100, valid=1024)

    def call(buf=X, cols=20, w2=W2, out=OUT, out_floats=4000, win=512, hop=128, pad=256, rows=None, count=None, null_table=False, **change):
        rows = [dict(good, **change)] if rows is None else rows
        table = None if null_table else (EbenOlaClip * max(1, len(rows)))(*[EbenOlaClip(**r) for r in rows])
        return lib.eben_overlap_add_clips(V(buf), cols, V(w2), V(out), out_floats, win, hop, pad, table, len(rows) if count is None else count, None)

    msg = lib.eben_last_error
    for k in ("buf", "w2", "out"):
        assert call(**{k: 0}) == EINVAL and b"null" in msg(), k
    assert call(null_table=True) == EINVAL and b"null" in msg()
    assert call(w2=W2 + 4) == EINVAL and b"misaligned" in msg() and call(out=OUT + 1) == EINVAL
    assert call(count=0) == EINVAL and b"0 rows" in msg() and call(cols=0) == EINVAL and call(out_floats=0) == EINVAL
    assert call(win=0) == EINVAL and call(hop=0) == EINVAL and call(hop=513) == EINVAL and call(pad=-1) == EINVAL
    assert call(frames_out=0) == EINVAL and call(frames_out=21) == EINVAL and b"of 20" in msg() and call(col=14) == EINVAL and call(col=-1) == EINVAL
    assert call(len_stretch=0) == EINVAL and call(len_stretch=4001) == EINVAL and b"of 4000" in msg() and call(dst_offset=2901) == EINVAL
    assert call(valid=1025) == EINVAL and b"1025 valid samples" in msg()                  # past what the frames cover
    assert call(valid=1101, frames_out=9) == EINVAL and call(valid=-1) == EINVAL          # past the row itself
    second = dict(good, dst_offset=1100, col=7)
    assert call(rows=[good, dict(second, col=6)]) == EINVAL and b"reads columns" in msg()
    assert call(rows=[good, dict(second, dst_offset=1099)]) == EINVAL and b"writes 1100 samples" in msg()
