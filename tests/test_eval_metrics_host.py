"""CPU: the host side of the evaluation metrics (ESTOI, zero-mean SI-SDR / SI-SNR, SNR, LSD) -- constructors and exports, the refusals
of the raw entries and of ``inference.evaluate_clips`` (all before any device work), the ``band_hz`` -> bin-range arithmetic, and the
float64 oracle of ``tests/eval_metrics_oracle.py`` against plain-loop restatements of itself."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import eval_metrics_oracle as E
from tests import metrics_oracle as M
from tests import ragged_oracle as R
from vibravox_amd import inference
from vibravox_amd._lib import SIGNATURES, EbenError, load

NEW_ENTRIES = ("eben_signal_ratio", "eben_estoi_workspace", "eben_estoi", "eben_lsd_workspace", "eben_lsd")


@pytest.fixture(scope="module")
def lib():
    return load()


@pytest.fixture(scope="module")
def gen():
    return R.formula_generator(1, 32)[0]


def test_the_refused_options_construct_and_hold_no_state():
    from vibravox_amd import metrics as m

    made = [m.ScaleInvariantSignalDistortionRatio(zero_mean=True), m.ShortTimeObjectiveIntelligibility(16000, extended=True),
            m.SignalNoiseRatio(), m.SignalNoiseRatio(zero_mean=True), m.ScaleInvariantSignalNoiseRatio(),
            m.LogSpectralDistance(16000), m.LogSpectralDistance(16000, 512, 128, (4000, 8000))]
    assert made[0].zero_mean is True and made[1].extended is True and made[1].fs == 16000
    for metric in made:
        assert isinstance(metric, m._MeanMetric) and list(metric.state_dict().keys()) == []
        with pytest.raises(RuntimeError):
            metric.compute()
    with pytest.raises(ValueError):
        m.LogSpectralDistance(16000, band_hz=[None, (4000, 8000)])
    with pytest.raises(ValueError):
        m.LogSpectralDistance(16000, band_hz=(7999.9, 8000))    # no bin in it


def test_library_exports_the_new_entries(lib):
    for name in NEW_ENTRIES:
        assert name in SIGNATURES and getattr(lib, name) is not None


def test_workspaces(lib):
    for fs in (16000, 10000, 48000):
        assert lib.eben_estoi_workspace(0, 100, fs) == lib.eben_estoi_workspace(3, 0, fs) == lib.eben_estoi_workspace(3, 100, 0) == 0
        for rows, t in ((1, 1), (1, 257), (5, 4100), (8, 40003)):
            assert lib.eben_estoi_workspace(rows, t, fs) >= lib.eben_stoi_workspace(rows, t, fs) + 8 * rows
    assert lib.eben_lsd_workspace(0, 100, 2048, 512, 1) == lib.eben_lsd_workspace(3, 100, 2048, 0, 1) == 0
    assert lib.eben_lsd_workspace(3, 5000, 2048, 512, 2) >= 8 * 2 * 3 * (1 + 5000 // 512)


def test_raw_entries_refuse_bad_arguments_before_any_launch(lib):
    """The pointers are host memory: nothing may be launched on them (no GPU here anyway) -- every call returns in the checks."""
    x = (ctypes.c_float * 64)()
    out = (ctypes.c_float * 8)()
    ws = (ctypes.c_char * 65536)()
    msg = lambda: lib.eben_last_error()
    for kw in ((None, x, 4, 16, None, 0, 0, out), (x, None, 4, 16, None, 0, 0, out), (x, x, 4, 16, None, 0, 0, None), (x, x, 0, 16, None, 0, 0, out),
               (x, x, 4, 0, None, 0, 0, out), (x, x, 4, 16, None, 2, 0, out), (x, x, 4, 16, None, -1, 0, out), (x, x, 4, 16, None, 1, 2, out)):
        assert lib.eben_signal_ratio(*kw, None) == -1, kw
    table = (ctypes.c_float * 9)()
    args = lambda **kw: [kw.get(k, d) for k, d in (("clean", x), ("processed", x), ("rows", 4), ("t_max", 16), ("lengths", None), ("fs", 16000),
                                                   ("table", table), ("taps", 9), ("ws", ws), ("ws_bytes", 65536), ("out", out),
                                                   ("out_classic", None), ("stream", None))]
    for key in ("clean", "processed", "ws", "out"):
        assert lib.eben_estoi(*args(**{key: None})) == -1 and b"null" in msg(), key
    for kw in (dict(rows=0), dict(rows=65536), dict(t_max=0), dict(fs=0), dict(table=None), dict(taps=8)):
        assert lib.eben_estoi(*args(**kw)) == -1, kw
    assert lib.eben_estoi(*args(ws_bytes=lib.eben_estoi_workspace(4, 16, 16000) - 1)) != 0 and b"workspace" in msg()
    lo, hi = (ctypes.c_int * 4)(0, 128, 0, 0), (ctypes.c_int * 4)(257, 256, 257, 257)
    largs = lambda **kw: [kw.get(k, d) for k, d in (("preds", x), ("target", x), ("rows", 1), ("t_max", 64), ("lengths", None), ("n_fft", 512),
                                                    ("hop", 128), ("lo", lo), ("hi", hi), ("nbands", 2), ("ws", ws), ("ws_bytes", 65536), ("out", out),
                                                    ("stream", None))]
    for key in ("preds", "target", "lo", "hi", "ws", "out"):
        assert lib.eben_lsd(*largs(**{key: None})) == -1 and b"null" in msg(), key
    for kw in (dict(rows=0), dict(rows=65536), dict(t_max=0), dict(n_fft=128), dict(n_fft=8192), dict(n_fft=768), dict(hop=0), dict(hop=513),
               dict(nbands=0), dict(nbands=5), dict(hi=(ctypes.c_int * 4)(258, 256, 0, 0)), dict(lo=(ctypes.c_int * 4)(-1, 128, 0, 0)),
               dict(lo=(ctypes.c_int * 4)(0, 256, 0, 0))):
        assert lib.eben_lsd(*largs(**kw)) == -1, kw
    assert lib.eben_lsd(*largs(ws_bytes=lib.eben_lsd_workspace(1, 64, 512, 128, 2) - 1)) == -2 and b"workspace" in msg()


def test_cpu_tensors_and_bad_lengths_are_refused_by_the_new_calls():
    from vibravox_amd import metrics as m

    p, g = torch.randn(3, 2000), torch.randn(3, 2000)
    calls = (lambda **kw: m.si_sdr(p, g, zero_mean=True, **kw), lambda **kw: m.si_snr(p, g, **kw), lambda **kw: m.snr(p, g, **kw),
             lambda **kw: m.stoi(p, g, 16000, extended=True, **kw), lambda **kw: m.stoi_and_estoi(p, g, 16000, **kw),
             lambda **kw: m.lsd(p, g, 16000, n_fft=512, hop=128, **kw))
    for call in calls:
        with pytest.raises(EbenError):
            call()
        with pytest.raises(ValueError, match="row 1 "):
            call(lengths=[2000, 0, 5])
        with pytest.raises(ValueError, match="3 rows"):
            call(lengths=[2000, 2000])
    with pytest.raises(ValueError, match=r"row 2 has length 256, outside \[257, 2000\]"):    # cannot be reflect-padded
        m.lsd(p, g, 16000, lengths=[2000, 257, 256], n_fft=512, hop=128)
    with pytest.raises(ValueError, match="reflect"):
        m.lsd(p[:, :1024], g[:, :1024], 16000)
    for kw in (dict(n_fft=1000), dict(n_fft=128), dict(n_fft=8192), dict(hop=0), dict(hop=4096), dict(band_hz=[None] * 5), dict(band_hz=[]),
               dict(band_hz=(4000, 3000)), dict(band_hz=(-1, 3000)), dict(band_hz=(8001, 9000))):
        with pytest.raises(ValueError):
            m.lsd(p, g, 16000, **kw)
    with pytest.raises(ValueError):
        m.lsd(p, g, 0)


def test_evaluate_clips_refuses_metric_names_before_touching_a_device(gen):
    clip = lambda t: torch.zeros(1, 1, t)      # CPU clips: anything that reached a kernel would raise EbenError instead
    ok = [clip(2000), clip(1500)]
    with pytest.raises(ValueError, match="unknown metric 'pesq'"):
        inference.evaluate_clips(gen, ok, ok, metrics=("si_sdr", "pesq"))
    with pytest.raises(ValueError, match="lsd_hf_cutoff_hz"):
        inference.evaluate_clips(gen, ok, ok, metrics=("si_sdr", "lsd_hf"))
    with pytest.raises(ValueError, match="no bin"):
        inference.evaluate_clips(gen, ok, ok, metrics=("lsd_hf",), lsd_hf_cutoff_hz=7999.0)
    with pytest.raises(ValueError):
        inference.evaluate_clips(gen, ok, ok, metrics=())
    with pytest.raises(ValueError, match="twice"):
        inference.evaluate_clips(gen, ok, ok, metrics=("snr", "snr"))
    # an LSD needs more than 1024 samples at 16 kHz: the clip is named (16 kHz, and 48 kHz clips three times as long)
    with pytest.raises(ValueError, match="clip 1"):
        inference.evaluate_clips(gen, [clip(2000), clip(1000)], [clip(2000), clip(1000)], metrics=("lsd",))
    with pytest.raises(ValueError, match="clip 0"):
        inference.evaluate_clips(gen, [clip(3000), clip(6000)], [clip(3000), clip(6000)], sample_rate=48000, metrics=("si_sdr", "lsd_hf"),
                                 lsd_hf_cutoff_hz=4000)
    assert inference.EVAL_METRICS == ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
    assert inference.DEFAULT_EVAL_METRICS == ("si_sdr", "stoi")


def test_band_hz_to_bin_range():
    from vibravox_amd.metrics import lsd_band_bins

    assert lsd_band_bins(None, 16000, 2048) == (0, 1025)            # the full band: Nyquist bin included
    assert lsd_band_bins((0, 8000), 16000, 2048) == (0, 1024)       # hi = fs / 2 is exclusive: bin 1024 sits AT 8000 Hz
    assert lsd_band_bins((4000, 8000), 16000, 2048) == (512, 1024)
    assert lsd_band_bins((4000, 8000), 16000, 512) == (128, 256)
    assert lsd_band_bins((4000, 1e9), 16000, 512) == (128, 257)     # only a hi beyond fs / 2 reaches the Nyquist bin
    assert lsd_band_bins((4000.0, 8000.0), 16000, 2048) == (512, 1024)
    assert lsd_band_bins((3999.9, 4000.1), 16000, 2048) == (512, 513)
    with pytest.raises(ValueError, match="no bin"):
        lsd_band_bins((4000.1, 4007.8), 16000, 2048)                # between bin 512 (4000 Hz) and bin 513 (4007.8125 Hz)
    for fs, n_fft in ((16000, 2048), (44100, 1024), (48000, 4096), (22050, 256)):
        for lo, hi in ((0, 100), (1000, 3000), (3000, fs // 2), (fs // 4, fs // 2), (777, 7777)):
            k = np.arange(n_fft // 2 + 1)
            inside = np.nonzero((lo * n_fft <= k * fs) & (k * fs < hi * n_fft))[0]     # lo <= k fs / n_fft < hi, in integers
            assert lsd_band_bins((lo, hi), fs, n_fft) == (int(inside[0]), int(inside[-1]) + 1), (fs, n_fft, lo, hi)


def test_estoi_oracle_against_a_triple_loop_on_one_segment():
    rng = np.random.RandomState(3)
    x, y = rng.rand(M.NUMBAND, M.N) + 0.1, rng.rand(M.NUMBAND, M.N) + 0.1

    def loops(a):
        a = [[float(v) for v in row] for row in a]
        for b in range(M.NUMBAND):                      # every band's 30 frames: centre, unit norm
            mean = sum(a[b]) / M.N
            a[b] = [v - mean for v in a[b]]
            norm = math.sqrt(sum(v * v for v in a[b]))
            a[b] = [v / norm for v in a[b]]
        for n in range(M.N):                            # every frame's 15 bands
            mean = sum(a[b][n] for b in range(M.NUMBAND)) / M.NUMBAND
            for b in range(M.NUMBAND):
                a[b][n] -= mean
            norm = math.sqrt(sum(a[b][n] ** 2 for b in range(M.NUMBAND)))
            for b in range(M.NUMBAND):
                a[b][n] /= norm
        return a

    xn, yn = loops(x), loops(y)
    d = sum(xn[b][n] * yn[b][n] for b in range(M.NUMBAND) for n in range(M.N)) / M.N
    assert abs(E.estoi_from_envelopes(x, y) - d) <= 1e-14
    assert np.abs(E.row_col_normalize(x[None])[0] - np.array(xn)).max() <= 1e-14
    assert abs(E.estoi_from_envelopes(x, x) - 1.0) <= 1e-14                # a segment against itself
    assert E.estoi_from_envelopes(x[:, :29], y[:, :29]) == 1e-5           # fewer than 30 frames
    # the two stated conventions: no dither, and a constant band (centred norm exactly 0) contributes 0 instead of 0 / 0
    flat = x.copy()
    flat[4] = 0.25
    got = E.row_col_normalize(flat[None])[0]
    assert np.isfinite(got).all() and E.CONVENTIONS["dither"] is False and E.CONVENTIONS["zero_norm_value"] == 0.0
    # two segments: the mean over J of the per-segment values
    x2, y2 = rng.rand(M.NUMBAND, M.N + 1) + 0.1, rng.rand(M.NUMBAND, M.N + 1) + 0.1
    both = 0.5 * (E.estoi_from_envelopes(x2[:, :-1], y2[:, :-1]) + E.estoi_from_envelopes(x2[:, 1:], y2[:, 1:]))
    assert abs(E.estoi_from_envelopes(x2, y2) - both) <= 1e-14


def test_ratio_oracles():
    rng = np.random.RandomState(5)
    t = rng.randn(3, 4001)
    p = t + 0.1 * rng.randn(3, 4001)
    # zero-mean SI-SDR does not see a constant added to preds; the plain one does
    assert np.abs(E.si_sdr(p + 0.5, t, zero_mean=True) - E.si_sdr(p, t, zero_mean=True)).max() <= 1e-9
    assert (np.abs(E.si_sdr(p + 0.5, t) - E.si_sdr(p, t)) > 1.0).all()
    assert np.array_equal(E.si_sdr(p, t), M.si_sdr(p, t)) and np.array_equal(E.si_snr(p, t), E.si_sdr(p, t, zero_mean=True))
    assert np.abs(E.snr(p + 0.5, t, zero_mean=True) - E.snr(p, t, zero_mean=True)).max() <= 1e-9
    # SNR of target + noise at a known ratio; a single sample under zero_mean is eps / eps
    assert np.abs(E.snr(p, t) - 10 * np.log10((t ** 2).sum(-1) / ((t - p) ** 2).sum(-1))).max() <= 1e-6
    assert float(E.snr(np.array([0.3]), np.array([0.7]), zero_mean=True)) == 0.0 == float(E.si_sdr(np.array([0.3]), np.array([0.7]), zero_mean=True))


def test_lsd_oracle():
    x = M.speech_like("lsdh", 1, 5000, 16000)[0]
    assert E.lsd(x, x) == 0.0 and E.lsd(np.zeros(2048), np.zeros(2048)) == 0.0
    # a gain g shifts every log power above the floor by 2 log10 g
    loud = x + 0.01 * np.sin(np.arange(5000) * 1.3)
    lp = E.log_power(loud, 512, 128)
    assert lp.shape == (257, 1 + 5000 // 128)
    live = (lp > -7).all(0).numpy()
    d = (E.log_power(0.5 * loud, 512, 128) - lp).abs().numpy()[:, live]
    assert live.any() and np.abs(d - 2 * math.log10(2)).max() <= 1e-9
    with pytest.raises(RuntimeError):
        E.lsd(x[:1024], x[:1024])     # torch refuses to reflect-pad 1024 samples by 1024
    assert np.isfinite(E.lsd(x[:1025], 0.5 * x[:1025]))
