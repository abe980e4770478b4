"""Data front end on the GPU: eben_clip_powers, the SNR-controlled collate, bwe_collate and the time-parallel biquad
(lowpass_biquad / remove_hf) against the float64 oracle of tests/frontend_oracle.py and the vectors recorded from the reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import frontend_oracle as F  # noqa: E402
from make_collate_golden import items  # noqa: E402  (only the input definitions; the reference is not imported)

pytestmark = pytest.mark.gpu

STRATEGIES = [("pad", False), ("constant_length-50-ms", False), ("constant_length-50-ms", True), ("constant_length-100-ms", False)]
SNR = (-3.0, 5.0)


def _dev(batch):
    return [{k: v.cuda() for k, v in it.items()} for it in batch]


def _ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


# ---- eben_clip_powers -----------------------------------------------------------------------------------------------------------
def _powers_case(clips):
    from vibravox_amd.collate import clip_powers

    dev = [c.cuda() for c in clips]
    got = clip_powers(dev)
    again = clip_powers(dev)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                                           # fixed summation order: the same bits
    want = np.array([np.mean(c.numpy().astype(np.float64) ** 2) for c in clips])
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print("clip_powers worst error in ulp:", float((err / _ulp(want)).max()))
    assert np.all(err <= _ulp(want)), (err / _ulp(want)).max()               # within 1 float32 ulp of the float64 mean
    return got


def test_clip_powers_lengths_and_zero_clip(hip):
    g = torch.Generator().manual_seed(0)
    lengths = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 100003, 600001]     # the last: more segments than partial sums per clip
    clips = [torch.randn(n, generator=g) * (0.01 + 0.1 * i) for i, n in enumerate(lengths)]
    clips.append(torch.zeros(777))
    got = _powers_case(clips)
    assert float(got[-1]) == 0.0


def test_clip_powers_sixty_clips_and_unaligned_views(hip):
    """60 clips cross the by-value table chunk (48); views that start 1, 2, 3 floats into a buffer leave the 16-byte grid."""
    g = torch.Generator().manual_seed(1)
    clips = [torch.rand(int(n), generator=g) - 0.5 for n in torch.randint(1, 3000, (60,), generator=g)]
    _powers_case(clips)
    from vibravox_amd.collate import clip_powers

    base = (torch.rand(9000, generator=g) - 0.5)
    dbase = base.cuda()
    views = [(o, n) for o in (1, 2, 3) for n in (1, 2, 5, 8191)]
    got = clip_powers([dbase[o:o + n] for o, n in views]).cpu().numpy().astype(np.float64)
    want = np.array([np.mean(base[o:o + n].numpy().astype(np.float64) ** 2) for o, n in views])
    assert np.all(np.abs(got - want) <= _ulp(want))


# ---- SNR-controlled collate -------------------------------------------------------------------------------------------------
def _check_mixed(got_bc, want_bc, want_ns, what):
    err = np.abs(got_bc.astype(np.float64) - want_bc.astype(np.float64))
    bound = F.mix_bound(want_ns, want_bc)
    print(what, "worst error / bound:", float((err / np.maximum(bound, 1e-300)).max()), "exact:", float((err == 0).mean()))
    assert np.all(err <= bound), (what, err.max())


@pytest.mark.parametrize("strategy,deterministic", STRATEGIES)
def test_snr_collate_matches_oracle(hip, strategy, deterministic):
    from vibravox_amd.collate import clip_powers, noisy_bwe_collate, plan_snr_mix

    batch = items()
    dev_batch = _dev(batch)
    torch.manual_seed(11)
    want = F.noisy_bwe_collate_snr(batch, 16000, strategy, deterministic, SNR)
    torch.manual_seed(11)
    got = noisy_bwe_collate(dev_batch, 16000, strategy, deterministic, snr_range=SNR)
    assert set(got) == {"audio_body_conducted", "audio_airborne"}
    assert got["audio_body_conducted"].shape == want["audio_body_conducted"].shape
    assert torch.equal(got["audio_airborne"].cpu(), want["audio_airborne"])
    _check_mixed(got["audio_body_conducted"].cpu().numpy(), want["audio_body_conducted"].numpy(), want["noise_scaled"].numpy(), strategy)
    # gains: the reference's float32 chain on the device's powers and the plan's snr_linear, within 1 ulp of the oracle's
    torch.manual_seed(11)
    _, snr_linear = plan_snr_mix([b["audio_body_conducted"].shape[0] for b in batch],
                                 [b["audio_body_conducted_speechless_noisy"].shape[0] for b in batch], SNR)
    p = clip_powers([b["audio_body_conducted"] for b in dev_batch] + [b["audio_body_conducted_speechless_noisy"] for b in dev_batch]).cpu()
    gains = torch.sqrt(p[:len(batch)] / (p[len(batch):] * snr_linear)).numpy()
    assert np.all(np.abs(gains.astype(np.float64) - want["gains"].numpy()) <= _ulp(want["gains"].numpy()))


def test_device_mixer_against_the_reference_fixture(hip):
    from vibravox_amd.collate import mix_speech_and_noise_with_rescaling

    fgold = np.load(os.path.join(HERE, "golden", "frontend_golden.npz"))
    batch = _dev(items())
    for k, rng in enumerate([(-3.0, 5.0), (0.0, 0.0)]):
        torch.manual_seed(0)
        noisy, scaled = mix_speech_and_noise_with_rescaling([b["audio_body_conducted"] for b in batch],
                                                            [b["audio_body_conducted_speechless_noisy"] for b in batch], rng)
        assert len(noisy) == len(scaled) == len(batch)
        for i, b in enumerate(batch):
            ref_ns, ref_bc = fgold[f"mixr/seed0/r{k}/scaled{i}"], fgold[f"mixr/seed0/r{k}/noisy{i}"]
            assert noisy[i].shape == scaled[i].shape == b["audio_body_conducted"].shape
            _check_mixed(scaled[i].cpu().numpy(), ref_ns, ref_ns, f"scaled{i}")      # the scaled-noise output
            _check_mixed(noisy[i].cpu().numpy(), ref_bc, ref_ns, f"noisy{i}")
            # the gain, read back from the largest scaled sample: within 2 ulp (2^-22) of the reference's, plus that sample's own rounding
            st = int(fgold[f"mixr/seed0/r{k}/start"][i])
            sl = b["audio_body_conducted_speechless_noisy"][st: st + ref_ns.shape[0]].cpu().numpy().astype(np.float64)
            j = int(np.abs(sl).argmax())
            g_ref = float(fgold[f"mixr/seed0/r{k}/gain"][i])
            assert abs(float(scaled[i][j]) / sl[j] - g_ref) <= (2.0 ** -22 + 2.0 ** -24) * g_ref


def test_snr_collate_sixty_items_and_all_zero_speech(hip):
    """60 items: two launches, the power arrays offset with the table.  An all-zero speech clip has gain 0: zeros out."""
    from vibravox_amd.collate import mix_speech_and_noise_with_rescaling, noisy_bwe_collate

    g = torch.Generator().manual_seed(5)
    batch = []
    for i, n in enumerate(torch.randint(50, 900, (60,), generator=g)):
        n = int(n)
        batch.append({"audio_body_conducted": torch.zeros(n) if i == 7 else torch.rand(n, generator=g) - 0.5,
                      "audio_airborne": torch.rand(n, generator=g) - 0.5,
                      "audio_body_conducted_speechless_noisy": (torch.rand(n + 1 + 13 * i, generator=g) - 0.5) * 0.2})
    torch.manual_seed(2)
    want = F.noisy_bwe_collate_snr(batch, 16000, "constant_length-25-ms", False, SNR)
    torch.manual_seed(2)
    got = noisy_bwe_collate(_dev(batch), 16000, "constant_length-25-ms", False, snr_range=SNR)
    assert torch.equal(got["audio_airborne"].cpu(), want["audio_airborne"])
    _check_mixed(got["audio_body_conducted"].cpu().numpy(), want["audio_body_conducted"].numpy(), want["noise_scaled"].numpy(), "60 items")
    assert float(want["gains"][7]) == 0.0 and not got["audio_body_conducted"][7].any()
    noisy, scaled = mix_speech_and_noise_with_rescaling([torch.zeros(300).cuda()], [torch.rand(400, generator=g).cuda()])
    assert not noisy[0].any() and not scaled[0].any() and noisy[0].shape == (300,)


# ---- bwe_collate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,deterministic", STRATEGIES)
def test_bwe_collate_matches_oracle_bit_exact(hip, strategy, deterministic):
    """800- and 1600-sample targets against clips of 250 .. 1250 samples: crops, and pad_audio's quirk on the shorter clips."""
    from vibravox_amd.collate import bwe_collate

    batch = items()
    torch.manual_seed(11)
    want = F.bwe_collate(batch, 16000, strategy, deterministic)
    after_want = torch.rand(1)
    torch.manual_seed(11)
    got = bwe_collate(_dev(batch), 16000, strategy, deterministic)
    assert torch.equal(torch.rand(1), after_want)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape
        assert torch.equal(got[k].cpu(), want[k]), k


def test_bwe_collate_sixty_items(hip):
    from vibravox_amd.collate import bwe_collate

    g = torch.Generator().manual_seed(5)
    batch = [{"audio_body_conducted": torch.randn(int(n), generator=g), "audio_airborne": torch.randn(int(n), generator=g)}
             for n in torch.randint(50, 900, (60,), generator=g)]
    for strategy in ("pad", "constant_length-25-ms"):
        torch.manual_seed(3)
        want = F.bwe_collate(batch, 16000, strategy, False)
        torch.manual_seed(3)
        got = bwe_collate(_dev(batch), 16000, strategy, False)
        for k in want:
            assert torch.equal(got[k].cpu(), want[k]), (strategy, k)


def test_bwe_collate_applies_the_augmentation_after_the_collate_draws(hip):
    from oracle import augment_oracle as A
    from vibravox_amd.augment import WaveformDataAugmentation
    from vibravox_amd.collate import bwe_collate

    kw = dict(p_data_augmentation=1, p_speed_perturbation=0, p_pitch_shift=0, p_time_masking=1)
    batch = items()
    torch.manual_seed(21)
    want = F.bwe_collate(batch, 16000, "constant_length-50-ms", False, A.WaveformDataAugmentation(16000, **kw))
    after_want = torch.rand(1)
    torch.manual_seed(21)
    got = bwe_collate(_dev(batch), 16000, "constant_length-50-ms", False, WaveformDataAugmentation(16000, **kw))
    assert torch.equal(torch.rand(1), after_want)
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k
    assert (want["audio_body_conducted"] == 0).all(dim=0).any()              # a masked run is there to be compared
    # deterministic: no augmentation, no draw of its
    torch.manual_seed(21)
    want = F.bwe_collate(batch, 16000, "constant_length-50-ms", True)
    got = bwe_collate(_dev(batch), 16000, "constant_length-50-ms", True, WaveformDataAugmentation(16000, **kw))
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k


# ---- eben_biquad / lowpass_biquad / remove_hf -------------------------------------------------------------------------------
FILTERS = [(16000, 4000), (16000, 200), (48000, 50)]


def _signal(rows, t, amplitude, seed):
    """a slow sine (passes every filter here) plus white noise, peak `amplitude`"""
    r = np.random.RandomState(seed)
    n = np.arange(t)[None, :]
    x = 0.6 * np.sin(2 * np.pi * n * (0.0007 + 0.0002 * np.arange(rows)[:, None]) + r.rand(rows, 1) * 6) + 0.4 * (2 * r.rand(rows, t) - 1)
    return (amplitude * x).astype(np.float32)


def _cases():
    """(t, padding_length): with L the chunk length read from the code, rows and padded rows of 2, L-1, L, L+1, 3L+5 and 40 001 samples
    (and the same around the per-thread run), the short rows at padding 1 and t-1, 3000 at t = 3001 and 4000."""
    from vibravox_amd.filters import CHUNK as L, SUBCHUNK as S

    cases = [(t, p) for t in (2, S - 1, S, S + 1, 3 * S + 5) for p in sorted({1, t - 1})]
    cases += [(3001, 3000), (4000, 3000)]
    cases += [(L - 3, 1), (L - 2, 1), (L - 1, 1)]                            # padded rows of L-1, L, L+1 samples: the second pass's rows too
    cases += [(t, 3000) for t in (L - 1, L, L + 1, 3 * L + 5, 40001)]
    return cases


def _check_rows(got, want, what, factor=8.0):
    """|got - oracle| <= 8 * 2^-24 * max|oracle row|: kernel and oracle agree to ~1e-11 before each pass's float32 rounding; a
    rounding-boundary flip of one ulp after the first pass reaches the output with gain <= sum|h| < 2, the second rounding adds one."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=-1)
    tol = factor * 2.0 ** -24 * np.abs(want).max(axis=-1)
    assert np.all(err <= tol), (what, float((err / np.maximum(tol, 1e-300)).max()))
    return float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("sr,fc", FILTERS)
@pytest.mark.parametrize("rows", [1, 3, 70])
def test_remove_hf_matches_float64_oracle(hip, rows, sr, fc):
    from vibravox_amd.filters import remove_hf

    worst = 0.0
    for t, pad in _cases():
        x = _signal(rows, t, 0.5, seed=t + pad)
        want = F.remove_hf(x, sr, fc, pad)
        got = remove_hf(torch.from_numpy(x).cuda(), sr, fc, pad).cpu().numpy()
        worst = max(worst, _check_rows(got, want, (rows, sr, fc, t, pad)))
    print(f"remove_hf rows={rows} sr={sr} fc={fc}: worst error / tolerance = {worst:.3f}")


def test_remove_hf_clamp_between_the_passes_and_leading_dimensions(hip):
    from vibravox_amd.filters import remove_hf

    x = _signal(6, 9000, 1.5, seed=1)
    want, mid = F.remove_hf(x, 16000, 4000, 3000, return_intermediate=True)
    assert mid.max() == 1.0 and mid.min() == -1.0                            # the clamp acts on the intermediate ...
    unclamped = F._lfilter_f32(np.pad(x.astype(np.float64), ((0, 0), (3000, 3000)), mode="reflect"), F._coef(16000, 4000, None), clamp=False)
    assert np.abs(unclamped).max() > 1.05                                    # ... and it is needed
    xd = torch.from_numpy(x).cuda()
    got = remove_hf(xd.reshape(2, 3, 9000), 16000, 4000)                     # (..., time): leading dimensions kept, default padding
    assert got.shape == (2, 3, 9000) and got.is_contiguous()
    _check_rows(got.reshape(6, 9000).cpu().numpy(), want, "amplitude 1.5")
    x = _signal(3, 9000, 0.3, seed=2)
    want, mid = F.remove_hf(x, 16000, 4000, 3000, return_intermediate=True)
    assert np.abs(mid).max() < 1.0                                           # the clamp never acts
    _check_rows(remove_hf(torch.from_numpy(x).cuda(), 16000, 4000).cpu().numpy(), want, "amplitude 0.3")
    # 1-D input
    assert remove_hf(xd[0], 16000, 4000).shape == (9000,)


def test_remove_hf_copies_a_non_contiguous_input_and_is_reproducible(hip):
    from vibravox_amd.filters import remove_hf

    x = _signal(4, 20001, 0.5, seed=3)
    xd = torch.from_numpy(x).cuda()
    want = F.remove_hf(x[:, ::2], 16000, 200, 3000)
    view = xd[:, ::2]
    assert not view.is_contiguous()
    got = remove_hf(view, 16000, 200)                                        # handled by one copy
    _check_rows(got.cpu().numpy(), want, "strided view")
    assert torch.equal(xd, torch.from_numpy(x).cuda())                       # the input is left alone
    a, b = remove_hf(xd, 48000, 50), remove_hf(xd, 48000, 50)
    assert torch.equal(a, b)                                                 # two runs agree bit for bit


@pytest.mark.parametrize("sr,fc", FILTERS)
def test_lowpass_biquad_forward_pass_alone(hip, sr, fc):
    """reversed = 0, pad = 0, clamp on.  One rounding: a flip moves an element by one of its own ulps, <= 2^-23 max|row|."""
    from vibravox_amd.filters import CHUNK, lowpass_biquad

    for rows, t in ((1, 1), (3, CHUNK + 1), (2, 40001)):
        x = _signal(rows, t, 1.2, seed=t)
        want = F.lowpass_biquad(x, sr, fc)
        got = lowpass_biquad(torch.from_numpy(x).cuda(), sr, fc).cpu().numpy()
        _check_rows(got, want, (sr, fc, rows, t), factor=2.0)
    assert np.abs(want).max() <= 1.0


def test_biquad_reversed_with_padding_and_without_clamp(hip):
    """The C entry point's own flags: a reversed pass over a reflect-padded row, stored in the input's orientation, no clamp."""
    from scipy.signal import lfilter

    from vibravox_amd.filters import _biquad, lowpass_biquad_coefficients

    coef = lowpass_biquad_coefficients(16000, 200)
    x = _signal(3, 9001, 1.5, seed=4)
    xp = np.pad(x.astype(np.float64), ((0, 0), (700, 700)), mode="reflect")
    want = lfilter(coef[:3], [1.0, coef[3], coef[4]], xp[:, ::-1], axis=-1)[:, ::-1]
    assert np.abs(want).max() > 1.0
    got = _biquad(torch.from_numpy(x).cuda(), 700, coef, True, False).cpu().numpy()
    _check_rows(got, want.astype(np.float32), "reversed, padded, unclamped", factor=2.0)


def test_filter_errors_on_the_device(hip):
    from vibravox_amd._lib import EbenError
    from vibravox_amd.filters import remove_hf

    x = torch.zeros(2, 100, device="cuda")
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        remove_hf(x, 16000, 4000, padding_length=100)
    with pytest.raises(ValueError, match="padding_length"):
        remove_hf(x, 16000, 4000, padding_length=0)
    with pytest.raises(EbenError, match="float32"):
        remove_hf(x.double(), 16000, 4000, padding_length=10)
    coef = (ctypes.c_double * 5)(1, 0, 0, 0, 0)
    y = torch.empty(2, 300, device="cuda")
    assert hip.eben_biquad(x.data_ptr(), y.data_ptr(), 2, 100, 100, coef, 0, 0, None, 0, None) != 0    # refused before any launch
