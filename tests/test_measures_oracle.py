"""CPU: the float64 oracle of the frame-based speech measures (``tests/measures_oracle.py``) against itself -- its two LPC routes and
its float32 spectral variant on the rows of the GPU tests, the clamps those rows must stay away from, a few properties -- and the host
side of the feature: exports, the refusals of ``eben_speech_measures``, ``metrics.speech_measures`` and ``inference.evaluate_clips``
before anything touches a device.

``ORACLE_SPREAD`` and ``FW_F32_SPREAD`` are measured, not fixed in advance (``-s`` prints them).  Observed here over the 54 rows:
ORACLE_SPREAD 7.9e-11 for ``llr`` and 2.9e-10 for ``cd`` (0 for the two SNRs, which have no LPC), FW_F32_SPREAD 4.8e-6 dB; no frame of a
compared row at a ``seg_snr``, ``llr`` or ``cd`` clamp, at most 20 % of a row's (frame, band) values at a ``fw_seg_snr`` clamp."""
import ctypes

import numpy as np
import pytest
import torch

from tests import measures_oracle as O
from tests import ragged_oracle as R
from vibravox_amd import inference
from vibravox_amd import metrics as m
from vibravox_amd._lib import SIGNATURES, EbenError, load


@pytest.fixture(scope="module")
def lib():
    return load()


def test_geometry_window_and_tile_are_mirrored():
    assert O.geometry(16000) == (480, 120, 16, 1024) == m.measures_geometry(16000)
    assert O.geometry(8000) == (240, 60, 10, 512) == m.measures_geometry(8000)
    assert O.TILE_FRAMES == m.MEASURES_TILE_FRAMES
    for fs in O.RATES:
        assert np.array_equal(O.window(fs), m.measures_window(fs)) and m.measures_window(fs).dtype == np.float64
        w, s, _, _ = O.geometry(fs)
        assert [O.frame_count(n, fs) for n in (w - 1, w, w + s - 1, w + s, w + 2 * s - 1, w + 2 * s)] == [0, 0, 0, 1, 1, 2]
        assert [O.frame_count(n, fs) for n in O.row_lengths(fs)][:8] == [1, 1, 2, 10, 11, 16, 17, 17]
        nonzero = (O.band_filters(fs) > 0).sum(axis=1)
        assert nonzero.min() == 7 and nonzero.max() == 29, nonzero
    for fs in (44100, 0, 16000.5, True, "16000"):
        with pytest.raises(ValueError, match="16000 or 8000"):
            m.measures_geometry(fs)


def test_the_two_lpc_routes_and_the_float32_spectrum_agree_on_the_gpu_tests_rows():
    spread, f32 = O.oracle_spread(), O.fw_f32_spread()
    print(f"ORACLE_SPREAD = { {k: f'{v:.3e}' for k, v in spread.items()} }, FW_F32_SPREAD = {f32:.3e} dB")
    assert all(np.isfinite(v) for v in spread.values()) and np.isfinite(f32)   # recorded, not held to a number: the bars are built from them
    assert spread["seg_snr"] == 0.0 == spread["fw_seg_snr"]                     # no LPC in them
    worst_fw = 0.0
    for fs in O.RATES:
        for route in ("direct", "toeplitz"):
            for (kind, n), row in zip(O.inputs(fs)[2], O.table(fs, route)):
                assert all(np.isfinite(row[name]) for name in O.NAMES), (fs, kind, n, row)
                seg, fw, llr, cd = row["_clamped"]
                # the clamps cannot hide an error: no frame sits at one, and few band values do
                assert seg == 0.0 and llr == 0.0 and cd == 0.0 and fw <= 0.30, (fs, kind, n, row["_clamped"])
                worst_fw = max(worst_fw, fw)
    print(f"largest share of (frame, band) values at a fw_seg_snr clamp: {worst_fw:.3f}")


def test_oracle_properties():
    fs = 16000
    targets, preds, labels = O.inputs(fs)
    i = labels.index(("bwe", O.row_lengths(fs)[4]))
    t, p = targets[i], preds[i]
    base = O.measures(p, t, fs)
    same = O.measures(t, t, fs)
    assert (same["seg_snr"], same["fw_seg_snr"], same["llr"], same["cd"]) == (35.0, 35.0, 0.0, 0.0)
    gain = O.measures(0.37 * p, t, fs)   # the LPC envelope does not see a gain
    assert abs(gain["llr"] - base["llr"]) <= 1e-9 and abs(gain["cd"] - base["cd"]) <= 1e-9 and gain["seg_snr"] != base["seg_snr"]
    # a row's value is that of its own samples: zeros behind it that make no further frame change nothing, zeros that make frames do --
    # which is why a padded batch needs its lengths
    w, s, _, _ = O.geometry(fs)
    pad = lambda x, n: np.concatenate([x, np.zeros(n)])
    assert O.frame_count(len(t) + s - 1, fs) == O.frame_count(len(t), fs) == 11
    within = O.measures(pad(p, s - 1), pad(t, s - 1), fs)
    assert all(within[k] == base[k] for k in O.NAMES)
    beyond = O.measures(pad(p, 999), pad(t, 999), fs)
    assert O.frame_count(len(t) + 999, fs) == 19 and all(beyond[k] != base[k] for k in O.NAMES)
    # an empty frame (either signal all zero in it) counts for seg_snr alone.  By hand: every frame as a row of its own (W + S samples
    # are one frame), then the means over the frames that count
    hole_p = p.copy()
    hole_p[2 * s : 2 * s + w] = 0.0          # frame 2 of preds is silent
    holed = O.measures(hole_p, t, fs)
    per = [O.measures(hole_p[f * s : f * s + w + s], t[f * s : f * s + w + s], fs) for f in range(11)]
    assert all(np.isnan(per[2][k]) for k in ("fw_seg_snr", "llr", "cd")) and abs(per[2]["seg_snr"]) <= 1e-9   # 10 log10(cc / (cc + eps) + eps)
    rest = [row for f, row in enumerate(per) if f != 2]
    assert all(np.isfinite(row[k]) for row in rest for k in O.NAMES)
    assert abs(holed["seg_snr"] - np.mean([row["seg_snr"] for row in per])) <= 1e-12          # all 11 frames
    assert abs(holed["fw_seg_snr"] - np.mean([row["fw_seg_snr"] for row in rest])) <= 1e-12   # the 10 non-empty ones
    for k in ("llr", "cd"):   # (95 * 10 + 50) // 100 = 10: nothing trimmed among the 10
        assert abs(holed[k] - np.mean([row[k] for row in rest])) <= 1e-12, k
    whole = [O.measures(p[f * s : f * s + w + s], t[f * s : f * s + w + s], fs) for f in range(11)]
    for k in ("llr", "cd"):   # without the hole the largest of the 11 frame values is trimmed: (95 * 11 + 50) // 100 = 10
        assert abs(base[k] - np.mean(sorted(row[k] for row in whole)[:10])) <= 1e-12, k
    silent = O.measures(np.zeros_like(t), t, fs)
    assert abs(silent["seg_snr"]) <= 1e-9 and all(np.isnan(silent[k]) for k in ("fw_seg_snr", "llr", "cd"))
    short = O.measures(p[: w + s - 1], t[: w + s - 1], fs)
    assert all(np.isnan(short[k]) for k in O.NAMES)
    # the trimmed mean: 0.95 F' rounded half up of the smallest values
    assert O.trimmed_mean([3.0]) == 3.0 and O.trimmed_mean([1.0] * 10) == 1.0 and np.isnan(O.trimmed_mean([]))
    assert O.trimmed_mean(list(range(11, 0, -1))) == np.mean(np.arange(1, 11)) and O.trimmed_mean([5.0, 1.0]) == 3.0


def test_library_exports_the_entries(lib):
    for name in ("eben_speech_measures_workspace", "eben_speech_measures"):
        assert name in SIGNATURES and getattr(lib, name) is not None
    ws = lib.eben_speech_measures_workspace
    assert ws(0, 32000, 16000, 15) == ws(65536, 32000, 16000, 15) == ws(3, 0, 16000, 15) == ws(3, 2 ** 31 - 1, 16000, 15) == 0
    assert ws(3, 32000, 44100, 15) == ws(3, 32000, 16000, 0) == ws(3, 32000, 16000, 16) == 0
    # a double per row, possible frame and measure behind the tables
    for fs in O.RATES:
        w, s, _, _ = O.geometry(fs)
        grown = ws(4, w + 200 * s, fs, 15) - ws(4, w + 100 * s, fs, 15)
        assert abs(grown - 8 * 4 * 4 * 100) < 256 and ws(1, w + s, fs, 1) > 0


def test_raw_entry_refuses_bad_arguments_before_any_launch(lib):
    """The pointers are host memory: nothing may be launched on them -- every call returns in the checks."""
    x = (ctypes.c_float * 4096)()
    win = (ctypes.c_double * 480)()
    out = (ctypes.c_float * 16)()
    ws = (ctypes.c_char * 65536)()
    args = lambda **kw: [kw.get(k, d) for k, d in (("preds", x), ("target", x), ("rows", 4), ("t_max", 1000), ("lengths", None), ("fs", 16000),
                                                   ("measures", 15), ("window", win), ("ws", ws), ("out", out), ("stream", None))]
    for key in ("preds", "target", "window", "ws", "out"):
        assert lib.eben_speech_measures(*args(**{key: None})) == -1 and b"null" in lib.eben_last_error(), key
    for kw in (dict(rows=0), dict(rows=65536), dict(t_max=0), dict(t_max=2 ** 31 - 1)):
        assert lib.eben_speech_measures(*args(**kw)) == -1 and b"outside" in lib.eben_last_error(), kw
    for fs in (0, 44100, 48000):
        assert lib.eben_speech_measures(*args(fs=fs)) == -1 and b"fs" in lib.eben_last_error(), fs
    for mask in (0, 16, 31, -1):
        assert lib.eben_speech_measures(*args(measures=mask)) == -1 and b"measures" in lib.eben_last_error(), mask


def test_metrics_speech_measures_checks_its_arguments_on_cpu_tensors():
    p, g = torch.randn(3, 2000), torch.randn(3, 2000)
    assert tuple(m.SPEECH_MEASURES) == ("seg_snr", "fw_seg_snr", "llr", "cd")
    with pytest.raises(ValueError, match="16000 or 8000"):
        m.speech_measures(p, g, 44100)
    with pytest.raises(ValueError, match="unknown measure 'wss'"):
        m.speech_measures(p, g, 16000, which=("llr", "wss"))
    with pytest.raises(ValueError, match="twice"):
        m.speech_measures(p, g, 16000, which=("llr", "llr"))
    with pytest.raises(ValueError, match="no measure"):
        m.speech_measures(p, g, 16000, which=())
    with pytest.raises(ValueError, match="same shape"):
        m.speech_measures(p, g[:, :1999], 16000)
    with pytest.raises(ValueError, match="no frame"):
        m.speech_measures(p[:, :599], g[:, :599], 16000)
    with pytest.raises(ValueError, match=r"row 1 has length 599, outside \[600, 2000\]"):
        m.speech_measures(p, g, 16000, lengths=[2000, 599, 600])
    with pytest.raises(ValueError, match=r"row 2 has length 299, outside \[300, 2000\]"):
        m.speech_measures(p, g, 8000, lengths=[2000, 300, 299])
    with pytest.raises(ValueError, match="3 rows"):
        m.speech_measures(p, g, 16000, lengths=[2000, 2000])
    for fn in (m.seg_snr, m.fw_seg_snr, m.llr, m.cepstral_distance):
        with pytest.raises(ValueError, match="16000 or 8000"):
            fn(p, g, 22050)
        with pytest.raises(EbenError):      # valid arguments: refused for being on the CPU, there is no CPU path
            fn(p, g, 16000, [2000, 600, 1234])
    with pytest.raises(EbenError):
        m.speech_measures(p, g, 8000, which=("cd", "seg_snr"))
    for cls, name in ((m.SegmentalSignalNoiseRatio, "seg_snr"), (m.FrequencyWeightedSegmentalSNR, "fw_seg_snr"), (m.LogLikelihoodRatio, "llr"),
                      (m.CepstralDistance, "cd")):
        with pytest.raises(ValueError, match="16000 or 8000"):
            cls(48000)
        metric = cls(8000)
        assert isinstance(metric, m._MeanMetric) and list(metric.state_dict().keys()) == [] and (metric.fs, metric.measure) == (8000, name)
        with pytest.raises(RuntimeError):
            metric.compute()
        with pytest.raises(EbenError):
            metric(p, g)


def test_evaluate_clips_knows_the_framed_measures_and_leaves_the_pinned_tuples_alone():
    gen = R.formula_generator(1, 32)[0]
    clip = lambda t: torch.zeros(1, 1, t)      # CPU clips: anything that reaches a kernel raises EbenError
    ok = [clip(2000), clip(1500)]
    assert inference.EVAL_METRICS_FRAMED == ("seg_snr", "fw_seg_snr", "llr", "cd")
    assert inference.EVAL_METRICS_FILTERED == ("sdr",)
    assert inference.EVAL_METRICS == ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
    assert inference.DEFAULT_EVAL_METRICS == ("si_sdr", "stoi")
    with pytest.raises(ValueError, match="unknown metric 'wss'") as err:
        inference.evaluate_clips(gen, ok, ok, metrics=("llr", "wss"))
    assert "known: si_sdr, stoi, estoi, si_snr, snr, lsd, lsd_hf, sdr, seg_snr, fw_seg_snr, llr, cd" in str(err.value)
    with pytest.raises(ValueError, match="twice"):
        inference.evaluate_clips(gen, ok, ok, metrics=("cd", "cd"))
    # a clip with fewer than W + S samples at 16 kHz after the cut is refused by index before anything runs (the generator's own shortest
    # clip is longer than that at 16 kHz: a model at 32 kHz reaches it)
    pair = [clip(4000), clip(1100)]
    with pytest.raises(ValueError, match="clip 1: 496 samples at 16000 Hz hold no frame"):
        inference.evaluate_clips(gen, pair, pair, sample_rate=32000, metrics=("si_sdr", "seg_snr"))
    with pytest.raises((EbenError, RuntimeError, AssertionError)) as reached:   # without a framed measure it is not
        inference.evaluate_clips(gen, pair, pair, sample_rate=32000, metrics=("si_sdr",))
    assert not isinstance(reached.value, ValueError)
    for name in inference.EVAL_METRICS_FRAMED:   # the names are accepted: the call gets as far as the device work, which CPU clips cannot do
        with pytest.raises((EbenError, RuntimeError, AssertionError)) as reached:
            inference.evaluate_clips(gen, ok, ok, metrics=(name,))
        assert not isinstance(reached.value, ValueError)
