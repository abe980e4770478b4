"""GPU: the evaluation metrics beyond SI-SDR and classic STOI -- ESTOI, zero-mean SI-SDR / SI-SNR, SNR and the log-spectral distance
(``eben_estoi`` / ``eben_signal_ratio`` / ``eben_lsd`` through ``vibravox_amd.metrics``), ``inference.evaluate_clips(metrics=...)`` and
the Lightning surface on top of them.

Every kernel case hands over views 4 bytes off the 16-byte grid inside a sentinel-fenced allocation with NaN behind every row's end and
asserts three things: the ragged call has the bits of every row alone (compared as int32, so NaN equals NaN), reversing the row order
and widening the buffer by 1000 changes no bit, and the fences and inputs are untouched.

Bars against the float64 oracle of every row ALONE (tests/eval_metrics_oracle.py): ESTOI ``STOI_TOL`` (the envelopes are classic STOI's
and the tail is fp64), the ratios ``SDR_TOL``, LSD four times what float32 ``torch.stft`` loses on the same float32 inputs, per row and
band -- not a number fixed in advance: the test computes it.

[MI355X] observed maxima against the oracle (each test prints its own with -s): ESTOI 7.7e-8 at 16 kHz and 1.4e-8 at 10 kHz; the ratios
1.5e-6 dB; LSD 8.9e-8 at n_fft 2048 and 1.0e-7 at 512 on live rows where float32 torch.stft loses 4.4e-7 .. 4.7e-6 and 1.9e-7 .. 2.1e-6
(the device's distance is the float32 rounding of its result); evaluate_clips against every pair alone: 0 bit differences, also from
48 kHz."""
import functools

import numpy as np
import pytest
import torch

from tests import eval_metrics_oracle as E
from tests import metrics_oracle as M
from tests import ragged_oracle as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
STOI_TOL = 1e-6     # |device - oracle| per row (tests/test_gpu_metrics.py)
SDR_TOL = 1e-4      # dB, up to 60 dB
FENCE = 64
SENTINEL = 12345.0

SDR_T, SDR_LENGTHS, SDR_SNRS = 40003, (40003, 31968, 16001, 7777, 257, 1), (-5, 0, 10, 30, 60, 5)
STOI16_T, STOI16_LENGTHS = 40003, (40003, 31968, 16001, 12000, 9000, 7777, 500, 300)
STOI10_T, STOI10_LENGTHS = 4100, (4100, 4000, 999, 257, 256)
# LSD: the issue's lengths, then a pair of all-zero rows and a zero preds row against a live reference (3000 / 700 samples)
LSD2048 = dict(n_fft=2048, hop=512, lengths=(1025, 2048, 2049, 5000, 20000), lowpassed=3, extra=3000)
LSD512 = dict(n_fft=512, hop=128, lengths=(257, 512, 1000, 4099), lowpassed=2, extra=700)
LSD_BANDS = [None, (4000, 8000)]
EVAL_LENGTHS = (16001, 12000, 9000, 7777)
EVAL_NAMES = ("si_sdr", "stoi", "estoi", "si_snr", "snr", "lsd", "lsd_hf")
HF_CUTOFF = 4000


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _noisy(x, snr_db, seed):
    """tests/test_gpu_metrics.py::_noisy: white noise at ``snr_db`` below the signal's own power."""
    n = np.random.RandomState(seed).randn(*x.shape)
    snr = np.broadcast_to(np.asarray(snr_db, np.float64), x.shape[:-1])[..., None]
    scale = np.sqrt((x ** 2).mean(-1, keepdims=True) / (n ** 2).mean(-1, keepdims=True)) * 10 ** (-snr / 20)
    return x + n * scale


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # NaN == NaN


def fenced(rows_of, t, order=None):
    """The rows (1-D float64 arrays, each its own length) in a (rows, t) view 4 bytes off the 16-byte grid inside a fenced allocation,
    NaN behind every row's end.  Returns (host image, device allocation, view)."""
    order = list(range(len(rows_of))) if order is None else order
    body = np.full((len(order), t), np.nan, np.float32)
    for r, i in enumerate(order):
        body[r, : len(rows_of[i])] = rows_of[i]
    n = body.size
    flat = torch.full((FENCE + 1 + n + FENCE,), SENTINEL, dtype=torch.float32)
    flat[FENCE + 1 : FENCE + 1 + n] = torch.from_numpy(body).reshape(-1)
    dev = flat.to(DEV)
    view = dev[FENCE + 1 : FENCE + 1 + n].view(len(order), t)
    assert view.data_ptr() % 16 == 4
    return flat, dev, view


def untouched(flat, dev):
    got = dev.cpu()
    return same_bits(got, flat) and float(got[:FENCE].min()) == SENTINEL == float(got[-FENCE:].max()) and float(got[FENCE]) == SENTINEL


# ---- the metrics under test: name -> (device call(preds, target, lengths) -> (rows,) or (bands, rows), oracle(preds row, target row)) ----
def _metric(name):
    from vibravox_amd import metrics as m

    if name.startswith("lsd"):
        cfg = LSD2048 if name == "lsd2048" else LSD512
        bins = [m.lsd_band_bins(b, 16000, cfg["n_fft"]) for b in LSD_BANDS]
        return (lambda p, c, lengths=None: m.lsd(p, c, 16000, lengths, cfg["n_fft"], cfg["hop"], LSD_BANDS),
                lambda p, c: [E.lsd(p, c, cfg["n_fft"], cfg["hop"], b) for b in bins])
    return {
        "estoi16": (lambda p, c, lengths=None: m.stoi(p, c, 16000, lengths, extended=True), lambda p, c: float(E.estoi(p[None], c[None], 16000)[0])),
        "estoi10": (lambda p, c, lengths=None: m.stoi(p, c, 10000, lengths, extended=True), lambda p, c: float(E.estoi(p[None], c[None], 10000)[0])),
        "si_sdr_zm": (lambda p, c, lengths=None: m.si_sdr(p, c, lengths, zero_mean=True), lambda p, c: float(E.si_sdr(p, c, True))),
        "si_snr": (lambda p, c, lengths=None: m.si_snr(p, c, lengths), lambda p, c: float(E.si_snr(p, c))),
        "snr": (lambda p, c, lengths=None: m.snr(p, c, lengths), lambda p, c: float(E.snr(p, c))),
        "snr_zm": (lambda p, c, lengths=None: m.snr(p, c, lengths, zero_mean=True), lambda p, c: float(E.snr(p, c, True))),
        "si_sdr": (lambda p, c, lengths=None: m.si_sdr(p, c, lengths), lambda p, c: float(E.si_sdr(p, c))),
    }[name]


@functools.lru_cache(maxsize=None)
def signals(kind):
    """(clean rows, processed rows, buffer width): float32 values as float64, each row its own length."""
    if kind == "ratio":
        # the rows of tests/test_gpu_ragged_metrics.py's SI-SDR case, with 0.5 added to preds only: zero-mean and plain values lie many dB apart
        clean = [_f32(M.speech_like(f"rsdr{n}", 3, n, 16000)[2]) for n in SDR_LENGTHS]
        proc = [_f32(_noisy(c[None], snr, 21 + r)[0] + 0.5) for r, (c, snr) in enumerate(zip(clean, SDR_SNRS))]
        return clean, proc, SDR_T
    if kind == "stoi16":
        clean = [_f32(M.speech_like(f"rag{n}", 1, n, 16000)[0]) for n in STOI16_LENGTHS]
        return clean, [_f32(_noisy(c[None], 3.0, n + 1)[0]) for c, n in zip(clean, STOI16_LENGTHS)], STOI16_T
    if kind == "stoi10":
        clean = [_f32(np.random.RandomState(n).randn(n)) for n in STOI10_LENGTHS]
        return clean, [_f32(_noisy(c[None], 3.0, n + 1)[0]) for c, n in zip(clean, STOI10_LENGTHS)], STOI10_T
    cfg = LSD2048 if kind == "lsd2048" else LSD512
    clean, proc = [], []
    for r, n in enumerate(cfg["lengths"]):
        ref = M.speech_like(f"lsd{n}", 1, n, 16000)[0]
        deg = 0.8 * ref + 0.05 * M.speech_like("other", 1, n, 16000, seed=3)[0]
        if r == cfg["lowpassed"]:    # a 16-tap mean: the high bins fall by decades
            deg = np.convolve(ref, np.ones(16) / 16, mode="same")
        clean.append(_f32(ref))
        proc.append(_f32(deg))
    n = cfg["extra"]
    live = _f32(M.speech_like("live", 1, n, 16000)[0])
    clean += [np.zeros(n), live]
    proc += [np.zeros(n), np.zeros(n)]
    return clean, proc, max(cfg["lengths"])


SIGNALS_OF = dict(estoi16="stoi16", estoi10="stoi10", si_sdr_zm="ratio", si_snr="ratio", snr="ratio", snr_zm="ratio", si_sdr="ratio",
                  lsd2048="lsd2048", lsd512="lsd512")


@functools.lru_cache(maxsize=None)
def case(name):
    """(oracle, alone): the float64 oracle of every row alone and the dense device value of every row alone, (rows,) or (bands, rows)."""
    clean, proc, _ = signals(SIGNALS_OF[name])
    call, oracle = _metric(name)
    want = np.array([oracle(p, c) for p, c in zip(proc, clean)], np.float64).T
    alone = np.stack([call(_dev(p[None]), _dev(c[None])).cpu().numpy().reshape(want.shape[:-1]) for p, c in zip(proc, clean)], axis=-1)
    return want, alone.astype(np.float32)


def run_ragged(name, extra=0, reverse=False):
    """The case's rows (reversed, in a buffer `extra` wider) in fenced buffers through the public entry point; checks fences and inputs;
    values in the case's own row order."""
    clean, proc, t = signals(SIGNALS_OF[name])
    order = list(range(len(clean)))[::-1] if reverse else list(range(len(clean)))
    lengths = [len(clean[i]) for i in order]
    c_flat, c_dev, c = fenced(clean, t + extra, order)
    p_flat, p_dev, p = fenced(proc, t + extra, order)
    got = _metric(name)[0](p, c, lengths).cpu().numpy()
    assert got.shape[-1] == len(order) and got.dtype == np.float32
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    back = np.empty_like(got)
    back[..., order] = got
    return back


def check_case(name, tol):
    """The three assertions of every case, and the bar against the oracle (`tol`: a number, or an array per value)."""
    want, alone = case(name)
    got = run_ragged(name)
    err = np.abs(got.astype(np.float64) - want)
    print(f"[{name}] |ragged - oracle| = {np.array2string(err, formatter=dict(float_kind=lambda v: f'{v:.2e}'))} (bar {np.array2string(np.asarray(tol, np.float64), formatter=dict(float_kind=lambda v: f'{v:.2e}'))}); "
          f"oracle {np.array2string(want, precision=5)}")
    assert np.array_equal(_bits(got), _bits(alone)), (got, alone)
    assert np.array_equal(_bits(run_ragged(name, reverse=True)), _bits(alone))
    assert np.array_equal(_bits(run_ragged(name, extra=1000)), _bits(alone))
    assert (err <= tol).all(), (err, want)
    return want, got


# ---- ESTOI ------------------------------------------------------------------------------------------------------------------------
def test_estoi_16k_rows_of_different_lengths(hip):
    from vibravox_amd.metrics import stoi, stoi_and_estoi

    want, got = check_case("estoi16", STOI_TOL)
    clean, proc, t = signals("stoi16")
    frames = [E.envelopes(c, p, 16000)[0].shape[1] for c, p in zip(clean[:5], proc[:5])]
    assert [f - 29 for f in frames] == [68, 49, 33, 20, 5]                      # segments of the five scored rows
    assert (want[5:] == 1e-5).all() and (got[5:] == np.float32(1e-5)).all()      # the three short rows
    _, _, c = fenced(clean, t)
    _, _, p = fenced(proc, t)
    lengths = list(STOI16_LENGTHS)
    classic = stoi(p, c, 16000, lengths)
    assert (np.abs(classic.cpu().numpy()[:5] - got[:5]) > 0.1).all(), (classic, got)   # the flag cannot be ignored
    both = stoi_and_estoi(p, c, 16000, lengths)      # one front end, two tails: the bits of the two calls
    assert same_bits(both[0], classic) and np.array_equal(_bits(both[1].cpu().numpy()), _bits(got))


def test_estoi_10k_rows_of_different_lengths(hip):
    """Stationary noise keeps every frame: 4100 samples leave exactly 30 STFT frames, ONE segment (J = 1); every shorter row 1e-5."""
    want, got = check_case("estoi10", STOI_TOL)
    assert want[0] != 1e-5 and (want[1:] == 1e-5).all() and (got[1:] == np.float32(1e-5)).all()
    clean, proc, _ = signals("stoi10")
    assert E.envelopes(clean[0], proc[0], 10000)[0].shape[1] == 30


def test_estoi_device_lengths_out_of_range_give_nan(hip):
    from vibravox_amd.metrics import stoi, stoi_and_estoi

    clean, proc, _ = signals("stoi16")
    _, alone = case("estoi16")
    row, t = STOI16_LENGTHS.index(9000), 9500
    c_flat, c_dev, c = fenced([clean[0][:t], clean[row], clean[0][:t]], t)
    p_flat, p_dev, p = fenced([proc[0][:t], proc[row], proc[0][:t]], t)
    lens = torch.tensor([0, 9000, t + 1], dtype=torch.int32, device=DEV)
    got = stoi(p, c, 16000, lens, extended=True).cpu().numpy()
    pair = stoi_and_estoi(p, c, 16000, lens)
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    assert np.isnan(got[[0, 2]]).all() and np.array_equal(_bits(got[1:2]), _bits(alone[row : row + 1])), got
    assert np.array_equal(_bits(pair[1].cpu().numpy()), _bits(got)) and np.isnan(pair[0].cpu().numpy()[[0, 2]]).all()


# ---- signal ratios ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["si_sdr_zm", "si_snr", "snr", "snr_zm"])
def test_signal_ratios_rows_of_different_lengths(hip, name):
    want, got = check_case(name, SDR_TOL)
    if name != "snr":
        assert got[5] == 0.0 and want[5] == 0.0      # one sample minus its own mean: eps / eps


def test_zero_mean_and_plain_ratios_lie_apart_and_plain_si_sdr_keeps_its_kernel(hip):
    from vibravox_amd._lib import check, stream

    plain, _ = check_case("si_sdr", SDR_TOL)         # zero_mean=False: the parent's entries; each row the bits of the dense call on it alone
    assert (np.abs(plain - case("si_sdr_zm")[0])[:5] > 1.0).all() and (np.abs(case("snr")[0] - case("snr_zm")[0])[:5] > 1.0).all()
    assert np.array_equal(_bits(case("si_snr")[1]), _bits(case("si_sdr_zm")[1]))
    # the raw entry: without a table every row is t_max long; (SI_SDR, zero_mean = 0) is eben_si_sdr itself; out-of-range lengths give NaN
    clean, proc, _ = signals("ratio")
    t = 7777
    c_flat, c_dev, c = fenced([x[:t] for x in clean[:4]], t)
    p_flat, p_dev, p = fenced([x[:t] for x in proc[:4]], t)
    out = torch.full((4, 4), 7.0, dtype=torch.float32, device=DEV)
    check(hip.eben_signal_ratio(p.data_ptr(), c.data_ptr(), 4, t, None, 0, 0, out[0].data_ptr(), stream()), "signal_ratio")
    check(hip.eben_si_sdr(p.data_ptr(), c.data_ptr(), 4, t, out[1].data_ptr(), stream()), "si_sdr")
    lens = torch.tensor([0, t, t + 1, -3], dtype=torch.int32, device=DEV)
    check(hip.eben_signal_ratio(p.data_ptr(), c.data_ptr(), 4, t, lens.data_ptr(), 1, 1, out[2].data_ptr(), stream()), "signal_ratio")
    check(hip.eben_signal_ratio(p.data_ptr(), c.data_ptr(), 4, t, None, 1, 1, out[3].data_ptr(), stream()), "signal_ratio")
    got = out.cpu().numpy()
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and np.isfinite(got[0]).all()
    assert np.isnan(got[2, [0, 2, 3]]).all() and np.array_equal(_bits(got[2, 1:2]), _bits(got[3, 1:2])) and np.isfinite(got[3]).all()
    want = float(E.snr(proc[1][:t], clean[1][:t], True))
    assert abs(float(got[2, 1]) - want) <= SDR_TOL


# ---- LSD --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lsd_float32_distance(name):
    """|LSD through float32 torch.stft - the float64 oracle| on the same float32 inputs, per band and row."""
    from vibravox_amd.metrics import lsd_band_bins

    cfg = LSD2048 if name == "lsd2048" else LSD512
    clean, proc, _ = signals(name)
    bins = [lsd_band_bins(b, 16000, cfg["n_fft"]) for b in LSD_BANDS]
    f32 = np.array([[E.lsd(p, c, cfg["n_fft"], cfg["hop"], b, dtype=torch.float32) for b in bins] for p, c in zip(proc, clean)]).T
    return np.abs(f32 - case(name)[0])


@pytest.mark.parametrize("name", ["lsd2048", "lsd512"])
def test_lsd_rows_of_different_lengths(hip, name):
    cfg = LSD2048 if name == "lsd2048" else LSD512
    dist32 = lsd_float32_distance(name)
    print(f"[{name}] |float32 torch.stft - oracle| = {np.array2string(dist32, precision=2)}")
    want, got = check_case(name, 4.0 * dist32)
    rows = len(cfg["lengths"])
    assert (want[:, :rows] > 1e-3).all() and want[0, cfg["lowpassed"]] > 1.0              # live rows; the low-passed one lies decades apart
    assert (got[:, rows] == 0.0).all() and (want[:, rows] == 0.0).all()                     # all-zero pair: exactly 0
    assert np.isfinite(got[:, rows + 1]).all() and (got[:, rows + 1] > 1.0).all()           # zero preds against a live reference


def test_lsd_device_lengths_out_of_range_give_nan(hip):
    from vibravox_amd.metrics import LogSpectralDistance, lsd

    clean, proc, _ = signals("lsd512")
    _, alone = case("lsd512")
    row, t = LSD512["lengths"].index(1000), 1000
    filler_c, filler_p = clean[3][:t], proc[3][:t]
    c_flat, c_dev, c = fenced([filler_c, filler_c, filler_c, clean[row], clean[0]], t)
    p_flat, p_dev, p = fenced([filler_p, filler_p, filler_p, proc[row], proc[0]], t)
    lens = torch.tensor([0, t + 1, 512 // 2, 1000, 257], dtype=torch.int32, device=DEV)
    got = lsd(p, c, 16000, lens, 512, 128, LSD_BANDS).cpu().numpy()
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    assert got.shape == (2, 5) and np.isnan(got[:, :3]).all(), got
    assert np.array_equal(_bits(got[:, 3]), _bits(alone[:, row])) and np.array_equal(_bits(got[:, 4]), _bits(alone[:, 0])), (got, alone)
    # one band per call: the bits of that band in the two-band launch; the class averages it
    hf = lsd(p[3:], c[3:], 16000, [1000, 257], 512, 128, (4000, 8000))
    assert hf.shape == (2,) and np.array_equal(_bits(hf.cpu().numpy()), _bits(got[1, 3:]))
    metric = LogSpectralDistance(16000, 512, 128, (4000, 8000))
    assert abs(float(metric(p[3:], c[3:], lengths=[1000, 257])) - float(got[1, 3:].astype(np.float64).mean())) <= 1e-6
    assert list(metric.state_dict().keys()) == []


# ---- evaluate_clips ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(fs=16000):
    lengths = tuple(t * (fs // 16000) for t in EVAL_LENGTHS)
    gen = R.formula_generator(1, 32)[0].to(DEV)
    ref = [_f32(M.speech_like(f"ev{t}", 1, t, fs)[0]) for t in lengths]
    cor = [_f32(_noisy(x[None], 5.0 if fs == 16000 else 10.0, t + 3)[0]) for x, t in zip(ref, lengths)]
    return gen, [_dev(x).reshape(1, 1, -1) for x in cor], [_dev(x).reshape(1, 1, -1) for x in ref], lengths


def check_every_pair_alone(out, gen, ref_dev, lengths, fs):
    """All seven values of every clip: the bits of the dense metric on (returned enhanced clip, cut reference) alone, at 16 kHz."""
    from vibravox_amd import metrics as m
    from vibravox_amd import ragged
    from vibravox_amd.augment import resample

    assert set(out) == set(EVAL_NAMES) | {"enhanced"}
    diffs = 0
    for i, (e, g, t) in enumerate(zip(out["enhanced"], ref_dev, lengths)):
        n = ragged.cut_length(gen, t)
        assert e.shape == (1, 1, n)
        e16, g16 = e.reshape(1, n), g.reshape(1, -1)[:, :n].contiguous()
        if fs != 16000:
            e16, g16 = resample(e16, fs, 16000), resample(g16, fs, 16000)
        alone = dict(si_sdr=m.si_sdr(e16, g16), stoi=m.stoi(e16, g16, 16000), estoi=m.stoi(e16, g16, 16000, extended=True),
                     si_snr=m.si_snr(e16, g16), snr=m.snr(e16, g16), lsd=m.lsd(e16, g16, 16000),
                     lsd_hf=m.lsd(e16, g16, 16000, band_hz=(HF_CUTOFF, 8000)))
        for name in EVAL_NAMES:
            assert out[name].shape == (len(lengths),) and out[name].dtype is torch.float32 and out[name].is_cuda
            assert torch.isfinite(out[name][i])
            diffs += int(not same_bits(out[name][i : i + 1], alone[name].reshape(1)))
            assert same_bits(out[name][i : i + 1], alone[name].reshape(1)), (name, i, out[name][i], alone[name])
    print(f"[evaluate_clips at {fs} Hz] bit differences against every pair alone: {diffs}; " +
          ", ".join(f"{k} {np.array2string(out[k].cpu().numpy(), precision=4)}" for k in EVAL_NAMES))


@pytest.mark.parametrize("fs", [16000, 48000])
def test_evaluate_clips_all_metrics_against_every_pair_alone(hip, fs):
    from vibravox_amd.inference import evaluate_clips

    gen, cor, ref_dev, lengths = corpus(fs)
    out = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, return_enhanced=True, metrics=EVAL_NAMES, lsd_hf_cutoff_hz=HF_CUTOFF)
    check_every_pair_alone(out, gen, ref_dev, lengths, fs)
    assert (out["estoi"] != 1e-5).any() and not same_bits(out["stoi"], out["estoi"])
    # two batches, another order of names: the same bits; a subset returns its own keys only
    small = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, max_batch_samples=40000 * (fs // 16000), metrics=EVAL_NAMES[::-1],
                           lsd_hf_cutoff_hz=HF_CUTOFF)
    assert list(small) == list(EVAL_NAMES[::-1]) and all(same_bits(small[k], out[k]) for k in EVAL_NAMES)
    only = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, metrics=("estoi", "lsd_hf"), lsd_hf_cutoff_hz=HF_CUTOFF)
    assert list(only) == ["estoi", "lsd_hf"] and same_bits(only["estoi"], out["estoi"]) and same_bits(only["lsd_hf"], out["lsd_hf"])
    # the default call: the parent's keys, and the bits of the explicit two names and of the full set's
    default = evaluate_clips(gen, cor, ref_dev, sample_rate=fs)
    explicit = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, metrics=("si_sdr", "stoi"))
    assert list(default) == ["si_sdr", "stoi"] == list(explicit)
    for k in ("si_sdr", "stoi"):
        assert same_bits(default[k], explicit[k]) and same_bits(default[k], out[k])


def test_evaluate_clips_default_launches_what_it_launched(hip, monkeypatch):
    """The default call makes the library calls of the parent: per batch the generator's, one eben_si_sdr_ragged and one eben_stoi_ragged
    -- none of the new entries."""
    from vibravox_amd import metrics as m
    from vibravox_amd.inference import evaluate_clips

    gen, cor, ref_dev, _ = corpus()
    seen = []
    real = m.check
    monkeypatch.setattr(m, "check", lambda rc, what="": (seen.append(what), real(rc, what))[1])
    evaluate_clips(gen, cor, ref_dev)
    assert seen == ["si_sdr_ragged", "stoi_ragged"]
    del seen[:]
    evaluate_clips(gen, cor, ref_dev, metrics=EVAL_NAMES, lsd_hf_cutoff_hz=HF_CUTOFF)
    assert seen == ["si_sdr_ragged", "stoi_and_estoi", "si_snr", "snr", "lsd"]      # STOI and ESTOI share a front end, the two LSD bands a launch


def _module():
    from functools import partial

    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales

    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    opt = partial(FusedAdam, lr=3e-4)
    return EBENLightningModule(sample_rate=16000, generator=EBENGenerator(m=4, n=32, p=2).to(dev),
                               discriminator=DiscriminatorEBENMultiScales(q=4, min_channels=24).to(dev), generator_optimizer=opt,
                               discriminator_optimizer=opt, feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales(),
                               adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales())


def test_module_evaluate_clips_logs_the_extra_corpus_means(hip):
    mod = _module()
    mod.dataloader_names = ["speech_clean", "speech_noisy"]
    _, cor, ref_dev, _ = corpus()
    out = mod.evaluate_clips(cor, ref_dev, dataloader_idx=1, metrics=("si_sdr", "stoi", "estoi", "lsd", "lsd_hf"), lsd_hf_cutoff_hz=HF_CUTOFF)
    suffix = "/speech_noisy"
    assert set(mod.logged) == {f"test/{k}{suffix}" for k in ("torchmetrics_si_sdr", "torchmetrics_stoi", "estoi", "lsd", "lsd_hf")}
    assert set(mod.metrics.keys()) == {"torchmetrics_si_sdr", "torchmetrics_stoi"}           # the reference's collection, unchanged
    # float32 means of four values: one float32 rounding between the two ways to sum
    for key, name in (("torchmetrics_stoi", "stoi"), ("estoi", "estoi"), ("lsd", "lsd"), ("lsd_hf", "lsd_hf")):
        assert abs(float(mod.logged[f"test/{key}{suffix}"]) - float(out[name].double().mean())) <= 1e-5, key
    with pytest.raises(ValueError, match="lsd_hf_cutoff_hz"):
        mod.evaluate_clips(cor, ref_dev, metrics=("lsd_hf",))
