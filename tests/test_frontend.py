"""Data front end, CPU side: the float64 oracle (tests/frontend_oracle.py) against vectors recorded from the reference's own
functions, the host-side planners against the oracle (same seed -> same samples, same generator state afterwards), error
behaviour, the biquad coefficients, an independent pin of the oracle's remove_hf, and the C ABI's new names."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import frontend_oracle as F  # noqa: E402
from make_collate_golden import LENGTHS, items  # noqa: E402  (only the input definitions; the reference is not imported)
from make_frontend_golden import SNR_RANGES  # noqa: E402

STRATEGIES = [("pad", False), ("constant_length-50-ms", False), ("constant_length-50-ms", True), ("constant_length-100-ms", False)]
NEW_NAMES = ("eben_clip_powers", "eben_clip_powers_workspace", "eben_noisy_collate_scaled", "eben_biquad", "eben_biquad_workspace")


@pytest.fixture(scope="module")
def fgold():
    return np.load(os.path.join(HERE, "golden", "frontend_golden.npz"))


def test_oracle_matches_reference_functions(fgold):
    batch = items()
    speech = [b["audio_body_conducted"] for b in batch]
    noise = [b["audio_body_conducted_speechless_noisy"] for b in batch]
    assert float(fgold["check:gain_rel"]) <= 2.0 ** -22          # the reference itself stays inside the cap used below
    for seed in (0, 1):
        for k, rng in enumerate(SNR_RANGES):
            torch.manual_seed(seed)
            noisy, scaled, gains = F.mix_speech_and_noise_with_rescaling(speech, noise, rng)
            ref_g = fgold[f"mixr/seed{seed}/r{k}/gain"].astype(np.float64)
            got_g = torch.cat(gains).numpy().astype(np.float64)
            assert np.all(np.abs(got_g - ref_g) <= 2.0 ** -22 * ref_g), (seed, k, got_g, ref_g)
            for i, n in enumerate(noise):
                st = int(fgold[f"mixr/seed{seed}/r{k}/start"][i])
                sl = n[st: st + speech[i].shape[0]].numpy()
                for name, got in (("scaled", scaled[i]), ("noisy", noisy[i])):
                    want = fgold[f"mixr/seed{seed}/r{k}/{name}{i}"]
                    err = np.abs(got.numpy().astype(np.float64) - want)
                    assert np.all(err <= F.mix_bound(ref_g[i] * sl.astype(np.float64), want)), (seed, k, name, i, err.max())
        for det in (False, True):
            torch.manual_seed(seed)
            for i, b in enumerate(batch):
                a, ab = F.C.set_audio_duration(audio=b["audio_body_conducted"], desired_samples=800, audio_bis=b["audio_airborne"], deterministic=det)
                np.testing.assert_array_equal(a.numpy(), fgold[f"bwe/seed{seed}/det{int(det)}/bc{i}"])
                np.testing.assert_array_equal(ab.numpy(), fgold[f"bwe/seed{seed}/det{int(det)}/air{i}"])


def _apply(batch, t, plan, gains=None):
    """numpy statement of what eben_noisy_collate (gains None, no noise) / eben_noisy_collate_scaled compute from a plan."""
    bc = np.zeros((len(batch), 1, t), np.float32)
    ab = np.zeros((len(batch), 1, t), np.float32)
    for i, (item, (ls, st, sh)) in enumerate(zip(batch, plan)):
        sp, ai, no = (item[k].numpy() for k in ("audio_body_conducted", "audio_airborne", "audio_body_conducted_speechless_noisy"))
        u = np.arange(t) + sh
        ok = (u >= 0) & (u < ls)
        v = sp[u[ok]]
        if gains is not None:
            v = v + no[st + u[ok]] * np.float32(gains[i])
        bc[i, 0, ok] = v
        ab[i, 0, ok] = ai[u[ok]]
    return bc, ab


@pytest.mark.parametrize("strategy,deterministic", STRATEGIES)
def test_plan_bwe_selects_the_oracle_samples(strategy, deterministic):
    from vibravox_amd.collate import plan_bwe, samples_of

    batch = items()
    torch.manual_seed(3)
    want = F.bwe_collate(batch, 16000, strategy, deterministic)
    after_want = torch.rand(1)
    torch.manual_seed(3)
    samples = samples_of(strategy, 16000)
    t, plan = plan_bwe([ls for ls, _, _ in LENGTHS], samples, deterministic)
    after_got = torch.rand(1)
    bc, ab = _apply(batch, t, [(ls, 0, sh) for ls, sh in plan])
    np.testing.assert_array_equal(bc, want["audio_body_conducted"].numpy())
    np.testing.assert_array_equal(ab, want["audio_airborne"].numpy())
    assert t == (max(ls for ls, _, _ in LENGTHS) if strategy == "pad" else samples)
    assert torch.equal(after_got, after_want)                   # the CPU generator ends in the same state


@pytest.mark.parametrize("strategy,deterministic", STRATEGIES)
def test_snr_plan_selects_the_oracle_samples(strategy, deterministic):
    from vibravox_amd.collate import _crop_plan, plan_snr_mix, samples_of

    batch = items()
    torch.manual_seed(4)
    want = F.noisy_bwe_collate_snr(batch, 16000, strategy, deterministic, (-3.0, 5.0))
    after_want = torch.rand(1)
    torch.manual_seed(4)
    lengths = [ls for ls, _, _ in LENGTHS]
    starts, snr_linear = plan_snr_mix(lengths, [ln for _, _, ln in LENGTHS], (-3.0, 5.0))
    t, shifts = _crop_plan(lengths, samples_of(strategy, 16000), deterministic)
    after_got = torch.rand(1)
    assert snr_linear.dtype is torch.float32 and snr_linear.shape == (len(batch),)
    # the oracle's gain chain on the plan's snr_linear: equal gains means equal snr_linear bits (and equal powers)
    gains = [float(torch.sqrt(F.power(b["audio_body_conducted"]) / (F.power(b["audio_body_conducted_speechless_noisy"]) * s)))
             for b, s in zip(batch, snr_linear)]
    np.testing.assert_array_equal(np.float32(gains), want["gains"].numpy())
    bc, ab = _apply(batch, t, list(zip(lengths, starts, shifts)), gains)
    np.testing.assert_array_equal(bc, want["audio_body_conducted"].numpy())
    np.testing.assert_array_equal(ab, want["audio_airborne"].numpy())
    assert torch.equal(after_got, after_want)


def test_default_keywords_leave_the_noisy_plan_untouched():
    """snr_range=None / data_augmentation=None: the draws of plan_noisy_bwe are those of oracle.collate_oracle, as before."""
    import inspect

    from vibravox_amd.collate import noisy_bwe_collate, plan_noisy_bwe

    sig = inspect.signature(noisy_bwe_collate)
    assert sig.parameters["snr_range"].default is None and sig.parameters["data_augmentation"].default is None
    assert list(sig.parameters)[:4] == ["batch", "sample_rate", "collate_strategy", "deterministic"]
    batch = items()
    for strategy, det in STRATEGIES:
        torch.manual_seed(9)
        want = F.C.noisy_bwe_collate(batch, 16000, strategy, det)
        after_want = torch.rand(1)
        torch.manual_seed(9)
        samples = None if strategy == "pad" else int(16000 * int(strategy.split("-")[1]) / 1000)
        t, plan = plan_noisy_bwe([ls for ls, _, _ in LENGTHS], [ln for _, _, ln in LENGTHS], samples, det)
        assert torch.equal(torch.rand(1), after_want)
        bc, ab = _apply(batch, t, plan, [1.0] * len(batch))
        np.testing.assert_array_equal(bc, want["audio_body_conducted"].numpy())
        np.testing.assert_array_equal(ab, want["audio_airborne"].numpy())


def test_error_behaviour():
    from vibravox_amd._lib import EbenError
    from vibravox_amd.collate import bwe_collate, mix_speech_and_noise_with_rescaling, plan_snr_mix
    from vibravox_amd.filters import remove_hf

    with pytest.raises(ValueError):
        plan_snr_mix([100], [99], (-3.0, 5.0))                 # utils.py:174-175
    with pytest.raises(RuntimeError):
        plan_snr_mix([100], [100], (-3.0, 5.0))                # torch.randint(0, 0): the reference fails the same way
    with pytest.raises(ValueError):
        F.mix_speech_and_noise_with_rescaling([torch.zeros(100)], [torch.zeros(99)])
    with pytest.raises(RuntimeError):
        F.mix_speech_and_noise_with_rescaling([torch.ones(100)], [torch.ones(100)])
    # the reference's checks come before any device work, so they can be met without a GPU
    with pytest.raises(TypeError):
        mix_speech_and_noise_with_rescaling((torch.zeros(4),), [torch.zeros(8)])
    with pytest.raises(TypeError):
        mix_speech_and_noise_with_rescaling([torch.zeros(4)], [np.zeros(8)])
    with pytest.raises(ValueError):
        mix_speech_and_noise_with_rescaling([torch.zeros(4)], [torch.zeros(8), torch.zeros(8)])
    with pytest.raises(ValueError, match="1D"):
        mix_speech_and_noise_with_rescaling([torch.zeros(2, 4)], [torch.zeros(8)])
    with pytest.raises(ValueError, match="1D"):
        mix_speech_and_noise_with_rescaling([torch.zeros(4)], [torch.zeros(1, 8)])
    with pytest.raises(ValueError, match="1D"):
        bwe_collate([{"audio_body_conducted": torch.zeros(1, 4), "audio_airborne": torch.zeros(1, 4)}], 16000)
    with pytest.raises(EbenError, match="same length"):        # set_audio_duration's assert, utils.py:67
        bwe_collate([{"audio_body_conducted": torch.zeros(5), "audio_airborne": torch.zeros(4)}], 16000)
    with pytest.raises(EbenError, match="no CPU path"):
        remove_hf(torch.zeros(1, 100), 16000, 4000, padding_length=10)
    with pytest.raises(ValueError, match="padding_length"):
        remove_hf(torch.zeros(1, 100), 16000, 4000, padding_length=0)


@pytest.mark.parametrize("sr,fc,each", [(16000, 4000, False), (16000, 200, False), (48000, 50, False), (16000, 3000, True), (44100, 8000, True)])
def test_lowpass_coefficients_against_the_closed_form(sr, fc, each):
    """2^-22 relative to the closed form in float64.  Relative to the coefficient set's scale, max|c| (between 1 and 2, a1's size):
    the function restates torchaudio's float32 steps, and those cancel -- 1 - cos(w0) at a low cut-off keeps 2^-24 absolute on a
    number of size w0^2 / 2, and at fc = sr / 4 the float32 w0 misses pi/2 by 4e-8, which is then all of a1 -- so no implementation
    of that recipe can hold 2^-22 of each coefficient's own size.  Where nothing cancels (`each`) every coefficient holds it."""
    from vibravox_amd.filters import lowpass_biquad_coefficients

    got = lowpass_biquad_coefficients(sr, fc)
    want = F.lowpass_coefficients_f64(sr, fc)
    assert len(got) == 5 and all(isinstance(c, float) for c in got)
    scale = max(abs(w) for w in want)
    for name, g, w in zip(("b0", "b1", "b2", "a1", "a2"), got, want):
        assert np.float32(g) == g, (name, g)                      # float32 values, as torchaudio hands them to lfilter
        assert abs(g - w) <= 2.0 ** -22 * (abs(w) if each else scale), (name, g, w)


@pytest.mark.parametrize("f0", [500.0, 1000.0, 2000.0])
def test_oracle_remove_hf_is_the_squared_magnitude_response_with_zero_delay(f0):
    """Independent pin of the oracle's remove_hf (no torchaudio here): a sine below, at and above the cut-off comes out, away from
    the edges, as |H(f0)|^2 times the input, sample for sample -- forward-backward filtering squares the magnitude and cancels the
    phase.  H from scipy.signal.freqz of the coefficients.  1e-6 absolute at amplitude 0.5: the poles (|z| = 0.76 at 16 kHz / 1 kHz)
    have forgotten the reflected edges to 1e-30 after 1000 samples, and the float32 intermediate adds 2^-25 * 0.5 * sum|h| < 3e-8."""
    from scipy.signal import freqz

    sr, fc, n = 16000, 1000, 8000
    coef = F.lowpass_coefficients_f64(sr, fc)
    x = (0.5 * np.sin(2 * np.pi * f0 * np.arange(n) / sr + 0.3)).astype(np.float32)
    y = F.remove_hf(x[None, :], sr, fc, padding_length=3000, coef=coef)[0]
    _, h = freqz(coef[:3], [1.0, coef[3], coef[4]], worN=[f0], fs=sr)
    want = np.abs(h[0]) ** 2 * x.astype(np.float64)
    assert y.shape == x.shape and y.dtype == np.float32
    assert np.abs(y[1000:-1000] - want[1000:-1000]).max() <= 1e-6
    if f0 == fc:
        assert abs(np.abs(h[0]) ** 2 - 0.5) < 1e-3               # Q = 0.707: -3 dB per pass at the cut-off, -6 dB for the pair


def test_header_signatures_and_library_agree_on_the_new_names():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "eben_hip.h")).read()
    declared = set(re.findall(r"EBEN_API\s+[\w\s\*]+?\b(eben_\w+)\s*\(", header))
    for name in NEW_NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct EbenClip" in header and _lib.EbenClip._fields_[0][0] == "data"
    import ctypes

    assert ctypes.sizeof(_lib.EbenClip) == 16 and ctypes.sizeof(_lib.EbenCollateItem) == 48   # layouts the by-value tables rely on
    assert lib.eben_version() == _lib.ABI_VERSION == 6 == int(re.search(r"#define EBEN_ABI_VERSION (\d+)", header).group(1))
    # workspace queries answer without a GPU; the chunk length of vibravox_amd.filters is the library's
    from vibravox_amd.filters import CHUNK

    assert lib.eben_biquad_workspace(3, CHUNK) == 0
    assert lib.eben_biquad_workspace(3, CHUNK + 1) == 3 * 2 * 32
    assert lib.eben_biquad_workspace(1, 2 * CHUNK + 1) == 3 * 32
    assert lib.eben_clip_powers_workspace(60) >= 60 * 8
    # argument checks come before any launch
    coef = (ctypes.c_double * 5)(1, 0, 0, 0, 0)
    assert lib.eben_biquad(1, 2, 1, 10, 10, coef, 0, 0, None, 0, None) != 0 and b"reflection" in lib.eben_last_error()
    assert lib.eben_clip_powers(None, 0, None, None, 0, None) != 0
