"""CPU: the float64 oracle of the BSS-eval SDR (``tests/sdr_oracle.py``) against itself -- its two routes on the inputs of the GPU
tests, the closed form at one tap -- and the host side of the feature: exports, the refusals of ``eben_sdr``, ``metrics.sdr`` and
``inference.evaluate_clips`` before anything touches a device.

``ORACLE_SPREAD`` is measured, not fixed in advance: the largest disagreement in dB of the fft / dense-solve route and the direct-sum /
Levinson route over every compared row.  Observed here: 1.8e-12 dB (``-s`` prints it)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ragged_oracle as R
from tests import sdr_oracle as O
from vibravox_amd import inference
from vibravox_amd import metrics as m
from vibravox_amd._lib import SIGNATURES, EbenError, load

S = m.SDR_SEGMENT


@pytest.fixture(scope="module")
def lib():
    return load()


def test_the_two_routes_agree_on_the_gpu_tests_inputs():
    ORACLE_SPREAD = O.oracle_spread(S)
    print(f"ORACLE_SPREAD = {ORACLE_SPREAD:.3e} dB")
    assert np.isfinite(ORACLE_SPREAD)      # recorded, not held to a number: the GPU tests' bar is built from it
    for kind in O.KINDS:
        for L in O.FILTER_LENGTHS:
            lengths = O.row_lengths(L, S)
            assert lengths[0] == 1 and 300 in lengths and 2 * S + 5 in lengths and len(set(lengths)) == len(lengths)
            for zero_mean, load_diag in O.SETTINGS:
                fft, direct = O.case(kind, L, S, zero_mean, load_diag)
                keep = O.compared(fft)
                assert np.array_equal(keep, O.compared(direct))
                # every row but the single sample lies inside the compared range; one sample is always proportional to its target
                # (coh = 1: +inf, or NaN once its mean is taken off) unless load_diag regularises it
                assert keep[1:].all(), (kind, L, zero_mean, load_diag, fft)
                assert keep[0] == (load_diag is not None), (kind, L, zero_mean, load_diag, fft[0])
                if zero_mean:
                    assert np.isnan(fft[0]) and np.isnan(direct[0])


def test_one_tap_is_si_sdr_without_eps():
    for kind in O.KINDS:
        for zero_mean in (False, True):
            targets, preds = O.case_inputs(kind, 1, S, zero_mean)
            for t, p in list(zip(targets, preds))[1:]:
                want = O.si_sdr_no_eps(p, t, zero_mean)
                for route in ("fft", "direct"):
                    assert abs(O.sdr(p, t, 1, zero_mean, None, route) - want) <= 1e-9, (kind, zero_mean, len(t), route)


def test_oracle_properties():
    targets, preds = O.inputs("speech", 64, S)
    t, p = targets[1], preds[1]
    base = O.sdr(p, t, 64)
    # zero padding behind a row changes nothing; a longer filter can only explain more; a scale on either signal changes nothing
    assert abs(O.sdr(np.concatenate([p, np.zeros(500)]), np.concatenate([t, np.zeros(500)]), 64) - base) <= 1e-9
    assert O.sdr(p, t, 512) >= base >= O.sdr(p, t, 1)
    assert abs(O.sdr(3.0 * p, 0.25 * t, 64) - base) <= 1e-9
    assert np.isnan(O.sdr(p, np.zeros_like(t), 64)) and np.isnan(O.sdr(p, np.zeros_like(t), 64, route="direct"))
    v = O.sdr(t, t, 64)
    assert not (np.isfinite(v) and v < 100.0)
    assert O.sdr(p, t, 64, load_diag=1e-3) < base


def test_library_exports_the_entries_and_the_segment_is_mirrored(lib):
    for name in ("eben_sdr_workspace", "eben_sdr"):
        assert name in SIGNATURES and getattr(lib, name) is not None
    assert lib.eben_sdr_workspace(0, 100, 512) == lib.eben_sdr_workspace(3, 0, 512) == lib.eben_sdr_workspace(3, 100, 0) == 0
    assert lib.eben_sdr_workspace(3, 100, 513) == 0
    # 2 L doubles per row and segment: one more sample than a whole number of segments adds one segment per row
    for rows, L in ((1, 512), (5, 7)):
        grown = lib.eben_sdr_workspace(rows, 2 * S + 1, L) - lib.eben_sdr_workspace(rows, 2 * S, L)
        assert abs(grown - 16 * L * rows) < 256     # (sizes are rounded to 256 bytes)
        assert lib.eben_sdr_workspace(rows, S + 1, L) == lib.eben_sdr_workspace(rows, 2 * S, L)
    assert lib.eben_sdr_workspace(256, 192000, 512) < 256 * 512 * 512 * 8 // 8      # an eighth of the dense route's matrices


def test_raw_entry_refuses_bad_arguments_before_any_launch(lib):
    """The pointers are host memory: nothing may be launched on them -- every call returns in the checks."""
    x = (ctypes.c_float * 64)()
    out = (ctypes.c_float * 8)()
    ws = (ctypes.c_char * 65536)()
    args = lambda **kw: [kw.get(k, d) for k, d in (("preds", x), ("target", x), ("rows", 4), ("t_max", 16), ("lengths", None), ("L", 8),
                                                   ("zero_mean", 0), ("load_diag", 0.0), ("ws", ws), ("out", out), ("stream", None))]
    for key in ("preds", "target", "ws", "out"):
        assert lib.eben_sdr(*args(**{key: None})) == -1 and b"null" in lib.eben_last_error(), key
    for kw in (dict(rows=0), dict(rows=65536), dict(t_max=0), dict(t_max=2 ** 31 - 1), dict(zero_mean=2), dict(load_diag=float("nan"))):
        assert lib.eben_sdr(*args(**kw)) == -1, kw
    for L in (0, -1, 513):
        assert lib.eben_sdr(*args(L=L)) == -1 and b"filter_length" in lib.eben_last_error(), L


def test_metrics_sdr_checks_its_arguments_on_cpu_tensors():
    p, g = torch.randn(3, 2000), torch.randn(3, 2000)
    with pytest.raises(NotImplementedError, match="use_cg_iter"):
        m.sdr(p, g, use_cg_iter=10)
    for L in (0, 513, -4, 2.5, True):
        with pytest.raises(ValueError, match="filter_length"):
            m.sdr(p, g, filter_length=L)
        with pytest.raises(ValueError, match="filter_length"):
            m.SignalDistortionRatio(filter_length=L)
    with pytest.raises(ValueError, match="load_diag"):
        m.sdr(p, g, load_diag=float("nan"))
    with pytest.raises(ValueError, match="same shape"):
        m.sdr(p, g[:, :1999])
    with pytest.raises(ValueError, match="row 1 "):
        m.sdr(p, g, lengths=[2000, 0, 5])
    with pytest.raises(ValueError, match="3 rows"):
        m.sdr(p, g, lengths=[2000, 2000])
    with pytest.raises(EbenError):      # valid arguments: refused for being on the CPU, there is no CPU path
        m.sdr(p, g, filter_length=16, zero_mean=True, load_diag=1e-3)
    metric = m.SignalDistortionRatio(filter_length=64, zero_mean=True, load_diag=1e-3)
    assert isinstance(metric, m._MeanMetric) and list(metric.state_dict().keys()) == []
    assert (metric.filter_length, metric.zero_mean, metric.load_diag) == (64, True, 1e-3)
    assert (m.SignalDistortionRatio().filter_length, m.SignalDistortionRatio().zero_mean, m.SignalDistortionRatio().load_diag) == (512, False, None)
    with pytest.raises(RuntimeError):
        metric.compute()
    with pytest.raises(EbenError):
        metric(p, g)


def test_evaluate_clips_knows_sdr_and_leaves_the_pinned_tuples_alone():
    gen = R.formula_generator(1, 32)[0]
    clip = lambda t: torch.zeros(1, 1, t)      # CPU clips: anything that reaches a kernel raises EbenError
    ok = [clip(2000), clip(1500)]
    assert inference.EVAL_METRICS_FILTERED == ("sdr",)
    assert inference.EVAL_METRICS == ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
    assert inference.DEFAULT_EVAL_METRICS == ("si_sdr", "stoi")
    with pytest.raises(ValueError, match="unknown metric 'pesq'") as err:
        inference.evaluate_clips(gen, ok, ok, metrics=("sdr", "pesq"))
    assert "known: si_sdr, stoi, estoi, si_snr, snr, lsd, lsd_hf, sdr" in str(err.value)
    with pytest.raises(ValueError, match="twice"):
        inference.evaluate_clips(gen, ok, ok, metrics=("sdr", "sdr"))
    for L in (0, 513, 1.5):
        with pytest.raises(ValueError, match="sdr_filter_length"):
            inference.evaluate_clips(gen, ok, ok, metrics=("sdr",), sdr_filter_length=L)
    # the name is accepted: the call gets as far as the device work, which CPU clips cannot do
    with pytest.raises((EbenError, RuntimeError, AssertionError)) as reached:
        inference.evaluate_clips(gen, ok, ok, metrics=("sdr",), sdr_filter_length=16)
    assert not isinstance(reached.value, ValueError)
