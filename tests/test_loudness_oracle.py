"""CPU: the float64 oracle of the integrated loudness (``tests/loudness_oracle.py``) against the recommendation and against itself, the
conditions its rows must meet for the GPU tests, and the host side of the feature: coefficients, exports, the refusals of
``eben_loudness`` / ``eben_pcm_encode_ragged_gain``, ``metrics.loudness_gain``, ``inference.enhance_to_pcm`` and ``evaluate_clips`` before
anything touches a device.

Measured, not fixed in advance (``-s`` prints them).  Observed here: ORACLE_SPREAD 9.6e-13 LU (cascade against one fourth-order filter,
over the 36 rows); the 48 kHz coefficients differ from the recommendation's printed table by 8.9e-16; 5 s of a 997 Hz sine at amplitude
1.0 measure -3.01027 LKFS at 48 kHz (-3.00751 at 44.1 kHz, -2.97004 at 16 kHz: the bilinear warp of the definition, not an error); the
3 s rows have 27 blocks of which 19 are kept (2 or 3 under the absolute gate, 5 or 6 under the relative), every block 1.7 LU or more
from the absolute gate and 6.5 LU or more from the relative gate."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import loudness_oracle as O
from tests import ragged_oracle as R
from vibravox_amd import inference
from vibravox_amd import metrics as m
from vibravox_amd._lib import SIGNATURES, EbenError, load


@pytest.fixture(scope="module")
def lib():
    return load()


def test_the_48_khz_coefficients_are_the_printed_table():
    (sb, sa), (hb, ha) = O.coefficients(48000)
    diff = max(np.abs(np.r_[sb, sa[1:]] - np.array(O.TABLE_48K_SHELF)).max(), np.abs(ha[1:] - np.array(O.TABLE_48K_HIGHPASS)).max())
    print(f"largest |formula - printed table| at 48 kHz = {diff:.3e}")
    assert diff <= 5e-15                       # the table has 14 decimals: half a unit of its last place
    assert list(hb) == [1.0, -2.0, 1.0] and sa[0] == ha[0] == 1.0


def test_the_calibration_sine_measures_what_the_recommendation_states():
    values = {}
    for fs in O.RATES:
        t = np.arange(5 * fs) / fs
        values[fs] = O.loudness(np.sin(2.0 * np.pi * 997.0 * t).astype(np.float32), fs)
    print("997 Hz sine, amplitude 1.0, 5 s: " + ", ".join(f"{fs} Hz {v:.5f} LKFS" for fs, v in values.items()))
    assert abs(values[48000] - (-3.01)) <= 0.005
    assert all(abs(v - (-3.01)) <= 0.05 for v in values.values())   # the other rates: the definition's bilinear warp, a few hundredths


def test_the_two_routes_agree_and_the_rows_stay_clear_of_both_gates():
    spread = O.oracle_spread()
    print(f"ORACLE_SPREAD = {spread:.3e} LU")
    assert math.isfinite(spread) and spread < 1e-9    # recorded; the GPU bar is built from it (ulp32 of -18 LUFS is 1.9e-6)
    for fs in O.RATES:
        h = fs // 10
        lengths = O.row_lengths(fs)
        assert [O.block_count(n, fs) for n in lengths[:4]] == [0, 1, 1, 2]
        assert [O.block_count(n, fs) for n in lengths[4:7]] == [0, 0, 0] and lengths[4:7] == [4095, 4096, 4097]
        assert lengths[8] % O.CHUNK == 0 and O.block_count(lengths[7], fs) >= 1
        assert h % 16 == 0 if fs != 44100 else h % 16 != 0       # 44.1 kHz: hops that are no multiple of a thread's samples
        for x, (level, pk) in zip(O.inputs(fs), O.table(fs)):
            assert x.dtype == np.float32 and pk == float(np.abs(x).max())
            z = O.blocks(x, fs)
            _, l, rel, kept = O.gated(z)
            assert math.isfinite(level) == (len(z) > 0)
            if len(z):
                # a flipped block cannot hide behind a tolerance: no block within 0.5 LU of either gate
                assert np.abs(l - O.ABSOLUTE_GATE).min() >= 0.5 and np.abs(l[l > O.ABSOLUTE_GATE] - rel).min() >= 0.5, (fs, len(x))
        z = O.blocks(O.inputs(fs)[-1], fs)
        _, l, rel, kept = O.gated(z)
        under_abs, under_rel = int((l <= O.ABSOLUTE_GATE).sum()), int(((l > O.ABSOLUTE_GATE) & (l <= rel)).sum())
        margins = (np.abs(l - O.ABSOLUTE_GATE).min(), np.abs(l[l > O.ABSOLUTE_GATE] - rel).min())
        print(f"[{fs} Hz, 3 s] {len(z)} blocks, {int(kept.sum())} kept ({under_abs} under the absolute gate, {under_rel} under the relative); "
              f"nearest block {margins[0]:.2f} LU from the absolute gate, {margins[1]:.2f} LU from the relative")
        assert len(z) == 27 and under_abs >= 2 and under_rel >= 2 and kept.sum() == 27 - under_abs - under_rel   # both gates drop blocks


def test_oracle_properties():
    fs = 16000
    x = O.inputs(fs)[-1]
    base = O.loudness(x, fs)
    assert abs(O.loudness(2.0 * x.astype(np.float64), fs) - (base + 20.0 * math.log10(2.0))) <= 1e-9    # a gain moves L by its dB
    assert O.loudness(np.zeros(3 * fs), fs) == -math.inf and O.loudness(x[: 4 * (fs // 10) - 1], fs) == -math.inf
    assert O.loudness(1e-5 * x.astype(np.float64), fs) == -math.inf                                    # everything under the absolute gate
    tail = np.concatenate([x, np.zeros(fs // 10 - 1)])                                                 # zeros that make no further block
    assert O.loudness(tail, fs) == base
    assert O.gain(-math.inf, 0.5) == 1.0 and O.gain(-20.0, 0.0) == 1.0
    assert abs(O.gain(-20.0, 0.1) - 10.0 ** (-3.0 / 20.0)) <= 1e-15
    assert abs(O.gain(-40.0, 0.5) - 10.0 ** (-1.0 / 20.0) / 0.5) <= 1e-15                              # the ceiling binds
    assert abs(O.gain(-40.0, 0.5, ceiling_db=-6.0) - 10.0 ** (-6.0 / 20.0) / 0.5) <= 1e-15


def test_k_weighting_coefficients_on_the_host(lib):
    for fs in O.RATES + (8000, 22050, 96000):
        shelf, highpass = m.k_weighting_coefficients(fs)
        (sb, sa), (hb, ha) = O.coefficients(fs)
        assert shelf.dtype == highpass.dtype == np.float64 and shelf.shape == highpass.shape == (5,)
        want = np.r_[sb, sa[1:], hb, ha[1:]]
        assert np.abs(np.r_[shelf, highpass] - want).max() <= 4 * np.finfo(np.float64).eps * 3.0       # the same formulas: a few ulp of libm
        coef = (ctypes.c_double * 10)()
        assert lib.eben_k_weighting(fs, coef) == 0
        assert np.abs(np.array(coef[:]) - want).max() <= 4 * np.finfo(np.float64).eps * 3.0            # what the kernels run with
    for fs in (0, -16000, 44101, 16000.0, True, "48000", None):
        with pytest.raises(ValueError, match="multiple of 10"):
            m.k_weighting_coefficients(fs)
    coef = (ctypes.c_double * 10)()
    assert lib.eben_k_weighting(44101, coef) == -1 and b"multiple of 10" in lib.eben_last_error()
    assert lib.eben_k_weighting(48000, None) == -1


def test_library_exports_the_entries(lib):
    for name in ("eben_k_weighting", "eben_loudness_workspace", "eben_loudness", "eben_pcm_encode_ragged_gain"):
        assert name in SIGNATURES and getattr(lib, name) is not None
    ws = lib.eben_loudness_workspace
    assert ws(0, 48000, 48000) == ws(65536, 48000, 48000) == ws(3, 0, 48000) == ws(3, 2 ** 31 - 1, 48000) == 0
    assert ws(3, 48000, 0) == ws(3, 48000, 44101) == ws(3, 48000, -10) == 0
    assert ws(1, 1, 10) > 0 and ws(1, 1, 48000) > 0
    # no weighted signal in it: a few numbers per 4096-sample chunk and per hop, far below the row's own 4 bytes a sample
    for fs in O.RATES:
        assert ws(4, 60 * fs, fs) < 4 * 60 * fs * 4 // 16
    assert ws(1, 3600 * 48000, 48000) < 8 * 2 ** 20    # an hour at 48 kHz: 42 k chunks, 36 k hops


def test_raw_entries_refuse_bad_arguments_before_any_launch(lib):
    """The pointers are host memory: nothing may be launched on them -- every call returns in the checks."""
    x = (ctypes.c_float * 8192)()
    lens = (ctypes.c_int32 * 4)()
    out = (ctypes.c_float * 16)()
    need = lib.eben_loudness_workspace(4, 2000, 16000)
    ws = (ctypes.c_char * (need + 16))()
    base = ctypes.addressof(ws)
    base += -base % 8
    inf, nan = float("inf"), float("nan")
    keys = (("x", x), ("rows", 4), ("t_max", 2000), ("lengths", lens), ("fs", 16000), ("target", -23.0), ("peak_db", -1.0), ("loudness", out),
            ("peak", out), ("gain", out), ("ws", base), ("ws_bytes", need), ("stream", None))
    args = lambda **kw: [kw.get(k, d) for k, d in keys]
    call = lambda **kw: (lib.eben_loudness(*args(**kw)), lib.eben_last_error())
    for key in ("x", "loudness", "peak", "ws"):
        rc, msg = call(**{key: None})
        assert rc == -1 and b"null" in msg, key
    odd = lambda a: ctypes.addressof(a) + 2
    for key, value in (("x", odd(x)), ("lengths", odd(lens)), ("loudness", odd(out)), ("peak", odd(out)), ("gain", odd(out)), ("ws", base + 4)):
        rc, msg = call(**{key: value})
        assert rc == -1 and b"misaligned" in msg, key
    for kw in (dict(rows=0), dict(rows=-1), dict(rows=65536)):
        rc, msg = call(**kw)
        assert rc == -1 and b"rows" in msg, kw
    for kw in (dict(t_max=0), dict(t_max=-5), dict(t_max=2 ** 31 - 1)):
        rc, msg = call(**kw)
        assert rc == -1 and b"t_max" in msg, kw
    for fs in (0, -16000, 44101, 15):
        rc, msg = call(fs=fs)
        assert rc == -1 and b"multiple of 10" in msg, fs
    for kw in (dict(target=nan), dict(target=inf), dict(peak_db=-inf), dict(peak_db=nan)):
        rc, msg = call(**kw)
        assert rc == -1 and b"finite" in msg, kw
    rc, msg = call(ws_bytes=need - 1)
    assert rc == -1 and b"workspace" in msg
    rc, msg = call(ws_bytes=0)
    assert rc == -1 and b"workspace" in msg

    # the gain encoder: what eben_pcm_encode_ragged refuses, and a null or misaligned table of gains
    from vibravox_amd import corpus

    rows = np.zeros(2, dtype=corpus.ENC_ROW_DTYPE)
    rows[0], rows[1] = (0, 0, 100, 0), (100, 208, 100, 0)
    image = (ctypes.c_char * 1024)()
    at = ctypes.addressof(image)
    at += -at % 16
    clipped = (ctypes.c_int32 * 2)()
    gains = (ctypes.c_float * 2)(1.0, 1.0)
    enc = lambda g, r=2, nbytes=512: lib.eben_pcm_encode_ragged_gain(ctypes.addressof(x), 8192, rows.ctypes.data, rows.ctypes.data, at, nbytes,
                                                                    ctypes.addressof(clipped), g, r, None)
    assert enc(None) == -1 and b"gains" in lib.eben_last_error()
    assert enc(ctypes.addressof(gains) + 2) == -1 and b"gains" in lib.eben_last_error()
    assert enc(ctypes.addressof(gains), r=0) == -1 and b"pcm_encode_ragged_gain" in lib.eben_last_error()
    assert enc(ctypes.addressof(gains), nbytes=300) == -1 and b"row 1 writes" in lib.eben_last_error()


def test_loudness_gain_checks_its_arguments_on_cpu_tensors():
    x = torch.randn(3, 20000)
    for fs in (0, 44101, 16000.0, True):
        with pytest.raises(ValueError, match="multiple of 10"):
            m.loudness_gain(x, fs)
        with pytest.raises(ValueError, match="multiple of 10"):
            m.integrated_loudness(x, fs)
    for kw in (dict(target=float("nan")), dict(peak=float("inf"))):
        with pytest.raises(ValueError, match="finite"):
            m.loudness_gain(x, 16000, **kw)
    with pytest.raises(ValueError, match=r"row 1 has length 20001, outside \[0, 20000\]"):
        m.loudness_gain(x, 16000, lengths=[20000, 20001, 0])
    with pytest.raises(ValueError, match=r"row 2 has length -1"):
        m.integrated_loudness(x, 16000, lengths=[20000, 0, -1])
    with pytest.raises(ValueError, match="3 rows"):
        m.loudness_gain(x, 16000, lengths=[5, 5])
    with pytest.raises(ValueError, match="time"):
        m.loudness_gain(torch.zeros(()), 16000)
    with pytest.raises(EbenError):                       # valid arguments, 0 a legal length: refused for being on the CPU
        m.loudness_gain(x, 16000, lengths=[20000, 0, 6399])
    with pytest.raises(EbenError):
        m.integrated_loudness(x, 48000)
    with pytest.raises(ValueError, match="multiple of 10"):
        m.IntegratedLoudness(22055)
    metric = m.IntegratedLoudness(48000)
    assert isinstance(metric, m._MeanMetric) and list(metric.state_dict().keys()) == [] and metric.fs == 48000
    with pytest.raises(RuntimeError):
        metric.compute()
    with pytest.raises(EbenError):
        metric(x)
    with pytest.raises(EbenError):
        metric.update(x, [20000, 10, 0])


def test_rows_to_pcm_and_enhance_to_pcm_check_the_loudness_arguments_first():
    gen = R.formula_generator(1, 32)[0]
    clips = [torch.zeros(1, 1, 8000), torch.zeros(1, 1, 9000)]   # CPU clips: anything that reaches a kernel raises EbenError
    for kw in (dict(loudness=float("nan")), dict(loudness=-23.0, peak=float("inf"))):
        with pytest.raises(ValueError, match="finite"):
            next(inference.enhance_to_pcm(gen, clips, **kw))
    with pytest.raises(ValueError, match="100 ms hops"):
        next(inference.enhance_to_pcm(gen, clips, loudness=-23.0, output_rate=11025))
    assert list(inference.enhance_to_pcm(gen, [], loudness=-23.0)) == []
    from vibravox_amd import export

    with pytest.raises(ValueError, match="finite"):
        export.enhance_corpus({"s": gen}, "/nonexistent", "/nonexistent/out", "speech_clean", "test", loudness=float("inf"))


def test_evaluate_clips_knows_lufs_diff_and_leaves_the_pinned_tuples_alone():
    gen = R.formula_generator(1, 32)[0]
    clip = lambda t: torch.zeros(1, 1, t)
    ok = [clip(2000), clip(1500)]
    assert inference.EVAL_METRICS_LEVEL == ("lufs_diff",)
    assert inference.EVAL_METRICS_FRAMED == ("seg_snr", "fw_seg_snr", "llr", "cd")
    assert inference.EVAL_METRICS_FILTERED == ("sdr",)
    assert inference.EVAL_METRICS == ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
    assert inference.DEFAULT_EVAL_METRICS == ("si_sdr", "stoi")
    with pytest.raises(ValueError, match="unknown metric 'lkfs'") as err:
        inference.evaluate_clips(gen, ok, ok, metrics=("lufs_diff", "lkfs"))
    assert str(err.value).endswith("known: si_sdr, stoi, estoi, si_snr, snr, lsd, lsd_hf, sdr, seg_snr, fw_seg_snr, llr, cd, lufs_diff")
    with pytest.raises(ValueError, match="twice"):
        inference.evaluate_clips(gen, ok, ok, metrics=("lufs_diff", "lufs_diff"))
    with pytest.raises((EbenError, RuntimeError, AssertionError)) as reached:   # the name is accepted: the call gets as far as the device work
        inference.evaluate_clips(gen, ok, ok, metrics=("lufs_diff",))
    assert not isinstance(reached.value, ValueError)
