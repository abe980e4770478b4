"""GPU: the per-clip augmentation kernels (``csrc/augment_clips.hip``) and ``WaveformDataAugmentation(per_clip=True)``.

Every comparison is ``torch.equal`` against the batch-level function of ``vibravox_amd/augment.py`` applied to that row alone: the
per-row kernels repeat its arithmetic operation for operation (the band table only leaves out taps that are exactly 0).  The two DFT
GEMMs of the pitch shift run on all rows' columns at once.  Their kernel is tap2 in every case, with the same channel chunking, but its
row-tile template argument FM (``eben_conv1d_variant_f32``, slot 1) grows with the column count to fill the grid: 1 for one row's
columns, 2 and then 4 for the concatenation of many rows.  A column's dot products run over the same channels in the same order under
each FM, so its bits do not depend on where it stands or on how many columns stand beside it; the small cases below all run under FM 1,
``test_pitch_rows_keep_their_bits_when_the_gemm_plan_changes`` measures the equality under FM 2 and FM 4."""
import math

import pytest
import torch

from formula import formula_tensor
from vibravox_amd import augment, collate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def fit(y, t):
    """The first t samples, zero-filled on the right."""
    return y[..., :t] if y.shape[-1] >= t else torch.nn.functional.pad(y, (0, t - y.shape[-1]))


@pytest.mark.parametrize("t", [1000, 1537, 4096, 8])
def test_resampler_rows_equal_speed_of_each_row(hip, t):
    """Six ratios in one launch; 1537 puts rows off the 16-byte lines, 8 is shorter than one band (13 taps)."""
    factors = (0.7, 1.3, 0.95, 1.05, 0.8, 1.2)
    x = formula_tensor(f"clips/rs/{t}", (6, t)).to(DEV)
    out = torch.full((6, t), float("nan"), device=DEV)
    augment.resample_clips(x, [(b * t, t, int(f * 16000), 16000, b) for b, f in enumerate(factors)], out)
    for b, f in enumerate(factors):
        want = augment.speed(x[b:b + 1], 16000, f)
        assert torch.equal(out[b:b + 1], fit(want, t)), (t, f)
    assert augment.speed(x[:1], 16000, 0.7).shape[-1] > t                                 # 0.7 is cropped
    tail = math.ceil(10 * t / 13)                                                        # 1.3 is padded: 13 : 10
    assert augment.speed(x[1:2], 16000, 1.3).shape[-1] == tail < t
    assert bool((out[1, tail:] == 0).all()) and (t == 8 or bool((out[1, tail - 8:tail] != 0).all()))


def test_resampler_reads_ragged_rows_and_writes_chosen_rows(hip):
    """Source rows of different lengths at odd offsets of a flat buffer, destination rows out of order, a row left alone."""
    t, lens, factors, dst = 1001, (1301, 640, 1001), (1.15, 0.85, 1.0), (3, 0, 2)
    flat = formula_tensor("clips/ragged", (1 + sum(lens) + 2,)).to(DEV)
    offs = [1, 1 + lens[0] + 1, 1 + lens[0] + 1 + lens[1] + 1]
    out = torch.full((4, t), 7.0, device=DEV)
    augment.resample_clips(flat, [(o, n, int(f * 16000), 16000, d) for o, n, f, d in zip(offs, lens, factors, dst)], out)
    for o, n, f, d in zip(offs, lens, factors, dst):
        assert torch.equal(out[d:d + 1], fit(augment.speed(flat[None, o:o + n], 16000, f), t)), f
    assert bool((out[1] == 7.0).all())


def test_time_mask_rows(hip):
    t = 1537
    x = formula_tensor("clips/tm", (7, t))
    masks = [(0, 0, 0), (1, 0, 61), (2, 1476, 61), (3, 309, 46), (5, 2, 1), (6, 0, t), (4, t, 0)]
    want = x.clone()
    for r, f, c in masks:
        want[r, f:f + c] = 0
    got = augment.time_mask_clips_(x.to(DEV), masks)
    assert torch.equal(got.cpu(), want) and bool((want[0] == x[0]).all()) and bool((want[4] == x[4]).all())


@pytest.mark.parametrize("t", [1000, 1537])
def test_pitch_rows_equal_pitch_shift_of_each_row(hip, t):
    """Bit equality; at these sizes both DFT GEMMs run under FM 1 for one row and for the concatenation (see the module docstring)."""
    steps, rows = (-4, -1, 1, 6, 3), (5, 0, 2, 6, 3)
    x = formula_tensor(f"clips/ps/{t}", (7, t)).to(DEV)
    out = torch.full((7, t), 7.0, device=DEV)
    augment.pitch_shift_clips(x, rows, steps, 2000, out)
    for r, s in zip(rows, steps):
        assert torch.equal(out[r:r + 1], augment.pitch_shift(x[r:r + 1], 2000, s)), (t, s)
    assert bool((out[1] == 7.0).all()) and bool((out[4] == 7.0).all())


def gemm_fm(hip, c_in, c_out, cols):
    """The tap2 kernel's FM for the (c_out, c_in) x (c_in, cols) DFT GEMM (eben_conv1d_variant_f32: family, FM, ...)."""
    import ctypes

    from vibravox_amd import ops

    d = ops.conv_desc(ops.ConvSpec(c_in=c_in, c_out=c_out, ksize=1), 1, cols)
    out = (ctypes.c_int * 8)()
    assert hip.eben_conv1d_variant_f32(ctypes.byref(d), 0, 0, out, 8) == 0 and out[0] == 2
    return out[1]


@pytest.mark.parametrize("rows,fm", [(16, 2), (32, 4)])
def test_pitch_rows_keep_their_bits_when_the_gemm_plan_changes(hip, rows, fm):
    """At the benchmark's row length a row alone has 313 STFT frames and both GEMMs run tap2_kernel<FM = 1>; 16 / 32 rows together have
    5008 / 10016 columns (5328 / 10703 stretched) and run FM = 2 / 4.  One row of every step, and the last row, against the row alone."""
    t, steps = 40000, (-4, -1, 1, 6, 3)
    nf = t // 128 + 1
    per_row = [steps[r % 5] for r in range(rows)]
    stretched = []
    for s in per_row:
        rate = 2.0 ** (-s / 12)
        n = math.ceil(nf / rate)
        stretched.append(n - 1 if (n - 1) * rate >= nf else n)
    assert gemm_fm(hip, 512, 514, nf) == 1 and all(gemm_fm(hip, 514, 512, n) == 1 for n in stretched)
    assert gemm_fm(hip, 512, 514, rows * nf) == fm and gemm_fm(hip, 514, 512, sum(stretched)) == fm
    x = formula_tensor(f"clips/ps/fm/{rows}", (rows, t)).to(DEV)
    out = torch.empty_like(x)
    augment.pitch_shift_clips(x, list(range(rows)), per_row, 2000, out)
    for r in (0, 1, 2, 3, 4, rows - 1):
        assert torch.equal(out[r:r + 1], augment.pitch_shift(x[r:r + 1], 2000, per_row[r])), (rows, r)


def test_module_rows_follow_the_chain_of_merged_functions(hip):
    B, T, sr = 5, 1537, 2000
    mod = augment.WaveformDataAugmentation(sr, per_clip=True, p_data_augmentation=0.6, p_speed_perturbation=0.6, p_pitch_shift=0.6, p_time_masking=0.6)
    a, b = formula_tensor("clips/mod/a", (B, 1, T)).to(DEV), formula_tensor("clips/mod/b", (B, 1, T)).to(DEV)
    torch.manual_seed(2)
    oa, ob = mod(a.clone(), b.clone())
    plan = {p.clip: p for p in mod.last_plan}
    assert any(p.factor is not None and p.steps is not None for p in plan.values())       # speed and pitch together
    assert len(plan) < B                                                                  # one clip untouched
    assert any(p.factor is None and p.steps is None and p.pct is not None for p in plan.values())   # one with only a mask
    assert oa.shape == a.shape and ob.shape == b.shape
    for c in range(B):
        for w, (src, got) in enumerate(((a, oa), (b, ob))):
            want = src[c].clone()                                                         # (1, T)
            p = plan.get(c)
            if p is not None:
                if p.factor is not None:
                    want = fit(augment.speed(want, sr, p.factor), T)
                if p.steps is not None:
                    want = augment.pitch_shift(want, sr, p.steps)
                if p.pct is not None:
                    first = (p.first_1, p.first_2)[w]
                    assert p.masked == int(T * p.pct / 100)
                    want[:, first:first + p.masked] = 0
                    assert bool((got[c, 0, first:first + p.masked] == 0).all())
            assert torch.equal(got[c], want), (c, w, p)
    masked = [p for p in plan.values() if p.pct is not None]
    assert any(p.first_1 != p.first_2 for p in masked)                                    # each waveform at its own position
    flat_a, _ = mod(a.reshape(B, T).clone(), None)                                        # (B, T), one waveform
    assert flat_a.shape == (B, T)


def test_collator_keeps_the_batch_length_per_clip(hip):
    sr, strategy, samples = 2000, "constant_length-500-ms", 1000
    lengths = (700, 1000, 1300, 2100)
    batch = [{"audio_body_conducted": formula_tensor(f"clips/col/bc/{i}", (n,)).to(DEV), "audio_airborne": formula_tensor(f"clips/col/ab/{i}", (n,)).to(DEV)}
             for i, n in enumerate(lengths)]
    kw = dict(p_data_augmentation=1, p_speed_perturbation=1, p_pitch_shift=0, p_time_masking=1)
    per_clip = augment.WaveformDataAugmentation(sr, per_clip=True, **dict(kw, p_pitch_shift=0.5))
    for seed in range(5):
        torch.manual_seed(seed)
        got = collate.bwe_collate(batch, sr, strategy, False, per_clip)
        assert got["audio_body_conducted"].shape == got["audio_airborne"].shape == (len(lengths), 1, samples), seed
        assert len({p.factor for p in per_clip.last_plan}) > 1 and bool(torch.isfinite(got["audio_body_conducted"]).all())
    torch.manual_seed(0)
    got = collate.bwe_collate(batch, sr, strategy, False, augment.WaveformDataAugmentation(sr, **kw))
    assert got["audio_body_conducted"].shape[-1] != samples                               # the batch mode's speed draw changes T
