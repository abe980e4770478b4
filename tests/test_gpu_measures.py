"""GPU: the frame-based speech measures (``eben_speech_measures`` through ``vibravox_amd.metrics.speech_measures``),
``inference.evaluate_clips(metrics=(..., "seg_snr", "fw_seg_snr", "llr", "cd"))`` and the metric classes on top of it.

Bar against the float64 oracle of every row ALONE (``tests/measures_oracle.py``): ``ulp32(oracle) + 100 * ORACLE_SPREAD[measure]`` for
``seg_snr``, ``llr`` and ``cd`` -- one float32 ulp because the output is the float32 rounding of a float64 value, and a hundred times the
oracle's own two-route disagreement for a third summation order -- and ``ulp32(oracle) + 4 * FW_F32_SPREAD`` for ``fw_seg_snr``, whose
transform is float32 in another butterfly order than the oracle's float32 variant.  Both spreads are measured on these rows
(``tests/test_measures_oracle.py`` prints them: 7.9e-11 / 2.9e-10 for llr / cd, 4.8e-6 dB).  The rows stay away from the clamps (asserted
on the oracle there), so a clamp cannot hide an error; the clamps have rows of their own here.

Bit equality (compared as int32, so NaN equals NaN): every row of a padded batch with NaN behind every row's end has the bits of the dense
call on that row alone, also reversed and in a wider buffer; ``which`` subsets give the bits of the full call.

The trimmed mean has one route for every frame count (a radix select, no sort): there is no resident / spilled pair to test apart; the
rows of two seconds (262 frames, more than a workgroup has threads) and the rows of identical signals (every value tied) cover its loops
and its ties.

[MI355X] observed maxima against the oracle over the 27 rows of each rate (``test_rows_of_different_lengths_against_the_oracle`` prints
them with -s), in float32 ulp of the oracle value: ``seg_snr`` 0.500 (4.8e-7 dB), ``llr`` 0.493 (2.1e-8), ``cd`` 0.499 (2.3e-7) -- the
float32 rounding of the result and nothing else -- and ``fw_seg_snr`` 2.50 at 16 kHz (4.8e-6 dB, a row of two frames, bar 2.1e-5) and 1.11
at 8 kHz (2.1e-6 dB).  Ragged against every row alone, reversed, widened, subsets, dense: 0 bit differences."""
import functools

import numpy as np
import pytest
import torch

from tests import measures_oracle as O
from tests import ragged_oracle as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SLACK = 37                      # t_max is larger than the longest row


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # NaN == NaN


def padded(rows_of, t, order):
    """The rows (1-D arrays, each its own length) in a (rows, t) device buffer, NaN behind every row's end."""
    body = np.full((len(order), t), np.nan, np.float32)
    for r, i in enumerate(order):
        body[r, : len(rows_of[i])] = rows_of[i]
    return torch.from_numpy(body).to(DEV)


def run_ragged(targets, preds, fs, which=O.NAMES, extra=0, reverse=False, lengths=None):
    """The rows (reversed, in a buffer ``extra`` wider) through ``metrics.speech_measures``; (len(which), rows) float32 on the device in the
    rows' own order.  ``lengths``: a device table that replaces the rows' own lengths."""
    from vibravox_amd.metrics import speech_measures

    order = list(range(len(targets)))[::-1] if reverse else list(range(len(targets)))
    t = max(len(x) for x in targets) + SLACK + extra
    g, p = padded(targets, t, order), padded(preds, t, order)
    keep_g, keep_p = g.clone(), p.clone()
    lens = [len(targets[i]) for i in order] if lengths is None else lengths
    got = speech_measures(p, g, fs, lens, which)
    assert list(got) == list(which)
    for v in got.values():
        assert v.shape == (len(order),) and v.dtype is torch.float32 and v.is_cuda
    assert same_bits(g, keep_g) and same_bits(p, keep_p)       # the inputs are untouched
    back = torch.tensor(np.argsort(order), device=DEV)
    return torch.stack([got[name].index_select(0, back) for name in which])


def alone(targets, preds, fs, which=O.NAMES):
    """The dense call on every row alone: a (1, n) buffer of its own, no lengths."""
    from vibravox_amd.metrics import speech_measures

    cols = []
    for t, p in zip(targets, preds):
        got = speech_measures(_dev(p[None]), _dev(t[None]), fs, None, which)
        cols.append(torch.stack([got[name].reshape(()) for name in which]))
    return torch.stack(cols, dim=1)


@functools.lru_cache(maxsize=None)
def batch(fs):
    targets, preds, labels = O.inputs(fs)
    return targets, preds, labels, run_ragged(targets, preds, fs), alone(targets, preds, fs)


@pytest.mark.parametrize("fs", O.RATES)
def test_rows_of_different_lengths_against_the_oracle(hip, fs):
    targets, preds, labels, got, _ = batch(fs)
    want = O.table(fs)
    got = got.cpu().numpy().astype(np.float64)
    for k, name in enumerate(O.NAMES):
        oracle = np.array([row[name] for row in want])
        err = np.abs(got[k] - oracle)
        bar = O.bar(name, oracle)
        worst = int(np.argmax(err / bar))
        print(f"[{fs} Hz {name}] largest |device - oracle| = {err.max():.3e} ({(err / O.ulp32(oracle)).max():.3f} float32 ulp of the oracle value); "
              f"closest to its bar: row {labels[worst]} {err[worst]:.3e} of {bar[worst]:.3e}")
        assert np.isfinite(got[k]).all() and (err <= bar).all(), (name, labels[worst], err[worst], bar[worst])


@pytest.mark.parametrize("fs", O.RATES)
def test_every_row_has_the_bits_of_the_call_on_it_alone(hip, fs):
    targets, preds, _, got, each = batch(fs)
    assert same_bits(got, each), (got, each)
    # wherever the row stands and however wide the buffer is
    assert same_bits(run_ragged(targets, preds, fs, reverse=True), each)
    assert same_bits(run_ragged(targets, preds, fs, extra=1000), each)


@pytest.mark.parametrize("fs", O.RATES)
def test_dense_call_and_subsets_have_the_bits_of_the_full_ragged_call(hip, fs):
    from vibravox_amd import metrics as m

    targets, preds, labels, got, _ = batch(fs)
    n = O.row_lengths(fs)[6]
    rows = [i for i, (_, length) in enumerate(labels) if length == n]       # one row per kind, equal lengths
    g, p = torch.stack([_dev(targets[i]) for i in rows]), torch.stack([_dev(preds[i]) for i in rows])
    dense = m.speech_measures(p, g, fs)
    full = m.speech_measures(p, g, fs, [n] * len(rows))
    on_device = m.speech_measures(p, g, fs, torch.tensor([n] * len(rows), dtype=torch.int32, device=DEV))
    for k, name in enumerate(O.NAMES):
        assert same_bits(dense[name], got[k][rows]) and same_bits(full[name], dense[name]) and same_bits(on_device[name], dense[name]), name
    # leading dimensions are kept
    shaped = m.speech_measures(p.reshape(3, 1, n), g.reshape(3, 1, n), fs, which=("cd",))["cd"]
    assert shaped.shape == (3, 1) and same_bits(shaped.reshape(3), dense["cd"])
    # subsets, in any order: the same bits (the spectral kernel and the LPC work are skipped when nobody asks)
    for which in (("seg_snr",), ("fw_seg_snr",), ("llr",), ("cd",), ("cd", "llr"), ("fw_seg_snr", "seg_snr"), ("cd", "seg_snr"), ("llr", "fw_seg_snr")):
        part = run_ragged(targets, preds, fs, which)
        for k, name in enumerate(which):
            assert same_bits(part[k], got[O.NAMES.index(name)]), (which, name)
    for fn, name in ((m.seg_snr, "seg_snr"), (m.fw_seg_snr, "fw_seg_snr"), (m.llr, "llr"), (m.cepstral_distance, "cd")):
        assert same_bits(fn(p, g, fs), dense[name]), name


def test_the_clamps_are_reached(hip):
    fs = 16000
    n = O.row_lengths(fs)[6]
    t = O.speech(4242, n, fs)
    noise = O._f32(0.3 * np.random.RandomState(99).randn(n))
    targets, preds = [t, t], [t, noise]
    want = [O.measures(p, g, fs) for p, g in zip(preds, targets)]
    got = run_ragged(targets, preds, fs).cpu().numpy().astype(np.float64)
    # identical signals: both SNRs at their upper clamp, both LPC distances 0 (every frame value tied)
    assert (want[0]["seg_snr"], want[0]["fw_seg_snr"], want[0]["llr"], want[0]["cd"]) == (35.0, 35.0, 0.0, 0.0)
    assert got[:, 0].tolist() == [35.0, 35.0, 0.0, 0.0], got[:, 0]
    # white noise against speech: every frame at the llr and cd clamps
    assert want[1]["_clamped"][2] == 1.0 == want[1]["_clamped"][3] and (want[1]["llr"], want[1]["cd"]) == (2.0, 10.0)
    assert got[2, 1] == 2.0 and got[3, 1] == 10.0, got[:, 1]
    for k, name in enumerate(O.NAMES[:2]):
        assert abs(got[k, 1] - want[1][name]) <= O.bar(name, want[1][name]), (name, got[k, 1], want[1][name])


@pytest.mark.parametrize("fs", O.RATES)
def test_empty_frames_and_rows_without_a_value_leave_their_neighbours_alone(hip, fs):
    w, s, _, _ = O.geometry(fs)
    n = O.row_lengths(fs)[6]
    t = O.speech(4242, n, fs)
    p = O.degrade("mix", t, O.speech(4243, n, fs), 1)
    holed = p.copy()
    holed[3 * s : 3 * s + w + s] = 0.0                 # frames 3 and 4 of preds are silent: empty
    targets = [t, t, t, t, t, np.zeros(n)]
    preds = [p, holed, np.zeros(n), p, p, p]           # row 2: every frame empty; row 5: a silent target
    t_max = n + SLACK
    lens = torch.tensor([n, n, n, w + s - 1, t_max + 1, n], dtype=torch.int32, device=DEV)
    got = run_ragged(targets, preds, fs, lengths=lens)
    each = alone(targets[:2], preds[:2], fs)
    assert same_bits(got[:, :2], each)
    host = got.cpu().numpy().astype(np.float64)
    want = O.measures(holed, t, fs)
    whole = O.measures(p, t, fs)
    assert all(np.isfinite(want[name]) and want[name] != whole[name] for name in O.NAMES) and want["_clamped"][2] < 1.0
    for k, name in enumerate(O.NAMES):
        assert abs(host[k, 1] - want[name]) <= O.bar(name, want[name]), (name, host[k, 1], want[name])
    # every frame empty: seg_snr is finite (the oracle's value), the others NaN
    silent = O.measures(np.zeros(n), t, fs)
    assert np.isnan(host[1:, 2]).all() and abs(host[0, 2] - silent["seg_snr"]) <= O.bar("seg_snr", silent["seg_snr"]), host[:, 2]
    assert np.isnan(host[1:, 5]).all() and np.isfinite(host[0, 5]), host[:, 5]
    # device lengths without a frame or outside the buffer: NaN everywhere
    assert np.isnan(host[:, 3]).all() and np.isnan(host[:, 4]).all(), host[:, 3:5]


# ---- evaluate_clips and the classes -------------------------------------------------------------------------------------------------
EVAL_LENGTHS = (4000, 2500, 1111)
EVAL_NAMES = ("si_sdr", "seg_snr", "fw_seg_snr", "llr", "cd")


@functools.lru_cache(maxsize=None)
def corpus():
    gen = R.formula_generator(1, 32)[0].to(DEV)
    ref = [O.speech(900 + i, t, 16000) for i, t in enumerate(EVAL_LENGTHS)]
    cor = [O.degrade("bwe", x, O.speech(950 + i, len(x), 16000), i) for i, x in enumerate(ref)]
    return gen, [_dev(x).reshape(1, 1, -1) for x in cor], [_dev(x).reshape(1, 1, -1) for x in ref]


def test_evaluate_clips_has_the_values_of_speech_measures_on_every_enhanced_clip(hip, monkeypatch):
    from vibravox_amd import metrics as m
    from vibravox_amd import ragged
    from vibravox_amd.inference import evaluate_clips

    gen, cor, ref = corpus()
    seen = []
    real = m.check
    monkeypatch.setattr(m, "check", lambda rc, what="": (seen.append(what), real(rc, what))[1])
    out = evaluate_clips(gen, cor, ref, metrics=EVAL_NAMES, return_enhanced=True)
    assert seen == ["si_sdr_ragged", "speech_measures"]          # one call per ragged batch for the four
    assert list(out) == list(EVAL_NAMES) + ["enhanced"]
    for i, t in enumerate(EVAL_LENGTHS):
        n = ragged.cut_length(gen, t)
        own = m.speech_measures(out["enhanced"][i].reshape(1, n), ref[i].reshape(1, -1)[:, :n].contiguous(), 16000)
        for name in EVAL_NAMES[1:]:
            assert out[name].shape == (len(EVAL_LENGTHS),) and out[name].dtype is torch.float32 and torch.isfinite(out[name]).all()
            assert same_bits(out[name][i : i + 1], own[name]), (name, i, out[name][i], own[name])
    # naming them changes no other value; the defaults launch none of it
    del seen[:]
    plain = evaluate_clips(gen, cor, ref, metrics=("si_sdr",))
    assert seen == ["si_sdr_ragged"] and same_bits(plain["si_sdr"], out["si_sdr"])
    part = evaluate_clips(gen, cor, ref, metrics=("cd", "seg_snr"), max_batch_samples=6000)
    assert list(part) == ["cd", "seg_snr"] and same_bits(part["cd"], out["cd"]) and same_bits(part["seg_snr"], out["seg_snr"])


def test_metric_classes_average_and_accumulate(hip):
    from vibravox_amd import metrics as m

    fs = 8000
    targets, preds, labels, got, _ = batch(fs)
    n = O.row_lengths(fs)[4]
    rows = [i for i, (_, length) in enumerate(labels) if length == n]
    g, p = torch.stack([_dev(targets[i]) for i in rows]), torch.stack([_dev(preds[i]) for i in rows])
    for k, cls in enumerate((m.SegmentalSignalNoiseRatio, m.FrequencyWeightedSegmentalSNR, m.LogLikelihoodRatio, m.CepstralDistance)):
        metric = cls(fs)
        values = got[k][rows].double()
        first = metric(p[:2], g[:2])
        assert abs(float(first) - float(values[:2].mean())) <= 1e-5
        metric.update(p[2:], g[2:], lengths=[n])
        assert abs(float(metric.compute()) - float(values.mean())) <= 1e-5
        assert list(metric.state_dict().keys()) == []
        metric.reset()
        with pytest.raises(RuntimeError):
            metric.compute()
