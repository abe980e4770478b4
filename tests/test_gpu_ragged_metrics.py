"""GPU: SI-SDR and STOI over rows of different lengths (``eben_si_sdr_ragged`` / ``eben_stoi_ragged`` through ``vibravox_amd.metrics``
and through their raw entries), ``inference.evaluate_clips`` and the Lightning surface on top of them.

Bars, the project's own (tests/test_gpu_metrics.py): ``STOI_TOL`` and ``SDR_TOL`` against the float64 oracle of every row ALONE, and bit
equality (compared as int32, so NaN equals NaN) with the dense call on the row alone -- a ragged row runs the dense kernels' loops with
its own length, in the same order, so this is a condition and not a measurement.

The kernel tests hand over views 4 bytes off the 16-byte grid inside a sentinel-fenced allocation, with NaN behind every row's length in
both signals: a row's value can only come out right if nothing behind its length is read, and fences and inputs are compared afterwards.

[MI355X] observed maxima against the oracle (each test prints its own with -s): SI-SDR 9.4e-7 dB, STOI 5.8e-8 at 16 kHz and 2.9e-8 at
10 kHz; evaluate_clips 2.1e-7 dB and 4.7e-8 (1.8e-7 dB and 3.5e-8 from 48 kHz); evaluate_clips against the batch-1 loop: 0 and 0."""
import functools

import numpy as np
import pytest
import torch

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
EVAL_LENGTHS = (16001, 12000, 9000, 7777, 1000)


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


# ---- the cases: rows (each alone, float32 values as float64), the oracle of every row alone, the dense device value of every row alone ----
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "sdr":
        # row 2 of speech_like starts inside a syllable: the 257 samples of the 60 dB row carry enough energy (sum t^2 >> the metric's
        # eps = 1.2e-7 times 10^6) for the oracle to reach 59 dB
        clean = [_f32(M.speech_like(f"rsdr{n}", 3, n, 16000)[2]) for n in SDR_LENGTHS]
        proc = [_f32(_noisy(c[None], snr, 21 + r)[0]) for r, (c, snr) in enumerate(zip(clean, SDR_SNRS))]
        fs = None
    elif name == "stoi16":
        clean = [_f32(M.speech_like(f"rag{n}", 1, n, 16000)[0]) for n in STOI16_LENGTHS]
        proc = [_f32(_noisy(c[None], 3.0, n + 1)[0]) for c, n in zip(clean, STOI16_LENGTHS)]
        fs = 16000
    else:
        clean = [_f32(np.random.RandomState(n).randn(n)) for n in STOI10_LENGTHS]
        proc = [_f32(_noisy(c[None], 3.0, n + 1)[0]) for c, n in zip(clean, STOI10_LENGTHS)]
        fs = 10000
    from vibravox_amd.metrics import si_sdr, stoi

    if fs is None:
        oracle = np.array([float(M.si_sdr(p, c)) for p, c in zip(proc, clean)])
        alone = np.array([float(si_sdr(_dev(p[None]), _dev(c[None])).cpu()) for p, c in zip(proc, clean)], np.float32)
    else:
        oracle = np.array([float(M.stoi(p[None], c[None], fs)[0]) for p, c in zip(proc, clean)])
        alone = np.array([float(stoi(_dev(p[None]), _dev(c[None]), fs).cpu()) for p, c in zip(proc, clean)], np.float32)
    return clean, proc, fs, oracle, alone


def run_ragged(name, t, order=None):
    """The case's rows in `order` in fenced (rows, t) buffers through the public entry point; checks fences and inputs; values in the
    case's own row order."""
    from vibravox_amd.metrics import si_sdr, stoi

    clean, proc, fs, _, _ = case(name)
    order = list(range(len(clean))) if order is None else order
    lengths = [len(clean[i]) for i in order]
    c_flat, c_dev, c = fenced(clean, t, order)
    p_flat, p_dev, p = fenced(proc, t, order)
    got = (si_sdr(p, c, lengths=lengths) if fs is None else stoi(p, c, fs, lengths=lengths)).cpu().numpy()
    assert got.shape == (len(order),) and got.dtype == np.float32
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    back = np.empty_like(got)
    back[order] = got
    return back


def check_case(name, t, tol):
    _, _, _, oracle, alone = case(name)
    got = run_ragged(name, t)
    err = np.abs(got.astype(np.float64) - oracle)
    print(f"[{name}] max|ragged - oracle| = {err.max():.2e} (bar {tol:g}); oracle {np.array2string(oracle, precision=5)}")
    assert np.array_equal(_bits(got), _bits(alone)), (got, alone)
    assert err.max() <= tol, (err, oracle)
    return oracle


def test_si_sdr_rows_of_different_lengths(hip):
    oracle = check_case("sdr", SDR_T, SDR_TOL)
    assert oracle[4] > 59


def test_stoi_16k_rows_of_different_lengths(hip):
    oracle = check_case("stoi16", STOI16_T, STOI_TOL)
    assert (oracle != 1e-5).sum() >= 4 and oracle[6] == 1e-5 and oracle[7] == 1e-5


def test_stoi_10k_rows_of_different_lengths(hip):
    """Stationary noise keeps every frame: 4100 samples (no slack) leave exactly 30 STFT frames, one segment; 4000 leave 29; 257 one
    frame and 256 none."""
    oracle = check_case("stoi10", STOI10_T, STOI_TOL)
    assert oracle[0] != 1e-5 and all(oracle[1:] == 1e-5)


@pytest.mark.parametrize("name,t", [("stoi16", STOI16_T), ("stoi10", STOI10_T), ("sdr", SDR_T)])
def test_batch_composition_changes_no_bit(hip, name, t):
    alone = case(name)[4]
    rows = len(alone)
    assert np.array_equal(_bits(run_ragged(name, t, list(range(rows))[::-1])), _bits(alone))
    assert np.array_equal(_bits(run_ragged(name, t + 1000)), _bits(alone))


def test_device_lengths_out_of_range_give_nan(hip):
    from vibravox_amd._lib import check, stream
    from vibravox_amd.metrics import si_sdr, stoi, stoi_resample_table

    clean, proc, _, _, alone = case("stoi16")
    row, t = STOI16_LENGTHS.index(9000), 9500
    c_rows = [clean[0][:t], clean[row], clean[0][:t]]
    p_rows = [proc[0][:t], proc[row], proc[0][:t]]
    c_flat, c_dev, c = fenced(c_rows, t)
    p_flat, p_dev, p = fenced(p_rows, t)
    lens = torch.tensor([0, 9000, t + 1], dtype=torch.int32, device=DEV)
    table = torch.from_numpy(stoi_resample_table(16000)[0]).to(torch.float32).to(DEV)
    out = torch.full((2, 3), 7.0, dtype=torch.float32, device=DEV)
    check(hip.eben_si_sdr_ragged(p.data_ptr(), c.data_ptr(), 3, t, lens.data_ptr(), out[0].data_ptr(), stream()), "si_sdr_ragged")
    ws_bytes = hip.eben_stoi_ragged_workspace(3, t, 16000)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    check(hip.eben_stoi_ragged(c.data_ptr(), p.data_ptr(), 3, t, lens.data_ptr(), 16000, table.data_ptr(), table.numel(), ws.data_ptr(),
                               ws_bytes, out[1].data_ptr(), stream()), "stoi_ragged")
    got = out.cpu().numpy()
    assert untouched(c_flat, c_dev) and untouched(p_flat, p_dev)
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 2]).all(), got
    sdr_alone = si_sdr(_dev(proc[row][None]), _dev(clean[row][None])).cpu().numpy()
    assert np.array_equal(_bits(got[0, 1:2]), _bits(sdr_alone)) and np.array_equal(_bits(got[1, 1:2]), _bits(alone[row : row + 1])), got
    assert got[1, 1] != np.float32(1e-5)
    # the same table through the public calls: used as it is; another dtype or shape is refused
    assert np.array_equal(_bits(si_sdr(p, c, lengths=lens).cpu().numpy()), _bits(got[0]))
    assert np.array_equal(_bits(stoi(p, c, 16000, lengths=lens).cpu().numpy()), _bits(got[1]))
    for bad in (lens.to(torch.int64), lens[:2], lens.reshape(3, 1)):
        with pytest.raises(ValueError):
            si_sdr(p, c, lengths=bad)
        with pytest.raises(ValueError):
            stoi(p, c, 16000, lengths=bad)


def test_metric_classes_take_lengths(hip):
    from vibravox_amd.metrics import ScaleInvariantSignalDistortionRatio, ShortTimeObjectiveIntelligibility

    clean, proc, _, _, _ = case("stoi16")
    lengths = list(STOI16_LENGTHS)
    _, _, c = fenced(clean, STOI16_T)
    _, _, p = fenced(proc, STOI16_T)
    for metric, oracle in ((ScaleInvariantSignalDistortionRatio(), lambda a, b: float(M.si_sdr(a, b))),
                           (ShortTimeObjectiveIntelligibility(16000), lambda a, b: float(M.stoi(a[None], b[None], 16000)[0]))):
        want = np.array([oracle(a, b) for a, b in zip(proc, clean)])
        first = metric(p[:3], c[:3], lengths=lengths[:3])
        metric.update(p[3:], c[3:], lengths=torch.tensor(lengths[3:]))
        assert first.is_cuda and first.dim() == 0
        np.testing.assert_allclose(float(first), want[:3].mean(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(float(metric.compute()), want.mean(), rtol=0, atol=1e-4)
        assert list(metric.state_dict().keys()) == []


# ---- evaluate_clips ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(fs=16000, lengths=EVAL_LENGTHS):
    gen = R.formula_generator(1, 32)[0].to(DEV)
    ref = [_f32(M.speech_like(f"ev{t}", 1, t, fs)[0]) for t in lengths]
    cor = [_f32(_noisy(x[None], 5.0 if fs == 16000 else 10.0, t + 3)[0]) for x, t in zip(ref, lengths)]
    return gen, [_dev(x).reshape(1, 1, -1) for x in cor], [_dev(x).reshape(1, 1, -1) for x in ref], ref


def check_against_alone(out, ref, cut, to16k=None):
    """Every clip's values against the oracle and the dense device metrics on (returned enhanced clip, cut reference), each alone."""
    from vibravox_amd.metrics import si_sdr, stoi

    sdr, sti = out["si_sdr"].cpu().numpy(), out["stoi"].cpu().numpy()
    worst = [0.0, 0.0]
    for i, (e, g, n) in enumerate(zip(out["enhanced"], ref, cut)):
        assert e.shape == (1, 1, n)
        e16, g16 = e.reshape(1, n), _dev(g[:n]).reshape(1, n)
        if to16k is not None:
            e16, g16 = to16k(e16), to16k(g16)
        e64, g64 = e16.double().cpu().numpy(), g16.double().cpu().numpy()
        worst[0] = max(worst[0], abs(float(sdr[i]) - float(M.si_sdr(e64, g64)[0])))
        worst[1] = max(worst[1], abs(float(sti[i]) - float(M.stoi(e64, g64, 16000)[0])))
        if to16k is None:   # at 16 kHz: the bits of the dense metrics on the pair alone
            assert np.array_equal(_bits(sdr[i : i + 1]), _bits(si_sdr(e16, g16).cpu().numpy())), i
            assert np.array_equal(_bits(sti[i : i + 1]), _bits(stoi(e16, g16, 16000).cpu().numpy())), i
    print(f"[evaluate_clips] max|si_sdr - oracle| = {worst[0]:.2e} dB (bar {SDR_TOL:g}), max|stoi - oracle| = {worst[1]:.2e} (bar {STOI_TOL:g}); "
          f"stoi {np.array2string(sti, precision=5)}")
    assert worst[0] <= SDR_TOL and worst[1] <= STOI_TOL, worst


def test_evaluate_clips_against_every_pair_alone(hip):
    from vibravox_amd import ragged
    from vibravox_amd.inference import MAX_BATCH_SAMPLES, evaluate_clips
    from vibravox_amd.metrics import si_sdr, stoi

    gen, cor, ref_dev, ref = corpus()
    cut = [ragged.cut_length(gen, t) for t in EVAL_LENGTHS]
    small = 40000
    assert len(ragged.compose_batches(gen, EVAL_LENGTHS, MAX_BATCH_SAMPLES)[0]) == 1
    assert len(ragged.compose_batches(gen, EVAL_LENGTHS, small)[0]) >= 2
    one = evaluate_clips(gen, cor, ref_dev, return_enhanced=True)
    assert set(one) == {"si_sdr", "stoi", "enhanced"} and one["si_sdr"].shape == one["stoi"].shape == (5,)
    assert one["si_sdr"].is_cuda and one["si_sdr"].dtype is torch.float32
    check_against_alone(one, ref, cut)     # per clip, in input order: the batches are sorted by length, the inputs are not
    two = evaluate_clips(gen, cor, ref_dev, max_batch_samples=small, return_enhanced=True)
    check_against_alone(two, ref, cut)
    assert set(evaluate_clips(gen, cor, ref_dev)) == {"si_sdr", "stoi"}
    # what a reference carries behind cut_to_valid_length is never read
    junk = [g.clone() for g in ref_dev]
    for g, n in zip(junk, cut):
        g[..., n:] = float("nan")
    assert sum(n < t for n, t in zip(cut, EVAL_LENGTHS)) == 4     # 12000 samples are a valid length as they are
    again = evaluate_clips(gen, cor, junk)
    assert same_bits(again["si_sdr"], one["si_sdr"]) and same_bits(again["stoi"], one["stoi"])
    # reported, not a bar: the batch-1 loop (tests/test_gpu_ragged.py states how far a ragged row may sit from its batch-1 row)
    with torch.no_grad():
        loop = [(gen(gen.cut_to_valid_length(c))[0], gen.cut_to_valid_length(g)) for c, g in zip(cor, ref_dev)]
    d_sdr = max(abs(float(si_sdr(e, g)) - float(one["si_sdr"][i])) for i, (e, g) in enumerate(loop))
    d_stoi = max(abs(float(stoi(e, g, 16000)) - float(one["stoi"][i])) for i, (e, g) in enumerate(loop))
    print(f"[evaluate_clips] max|value - batch-1 loop's| = {d_sdr:.2e} dB si_sdr, {d_stoi:.2e} stoi")


def test_evaluate_clips_resamples_other_rates_to_16k(hip):
    from vibravox_amd import ragged
    from vibravox_amd.augment import resample
    from vibravox_amd.inference import evaluate_clips

    lengths = (48001, 30000)
    gen, cor, ref_dev, ref = corpus(48000, lengths)
    out = evaluate_clips(gen, cor, ref_dev, sample_rate=48000, return_enhanced=True)

    def to16k(x):
        return resample(x, 48000, 16000)

    check_against_alone(out, ref, [ragged.cut_length(gen, t) for t in lengths], to16k)


# ---- the Lightning surface --------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("names", [None, ["speech_clean", "speech_noisy"]])
def test_module_evaluate_clips_logs_the_corpus_means(hip, names):
    mod = _module()
    mod.dataloader_names = names
    _, cor, ref_dev, _ = corpus()
    dl = 1 if names else 0
    out = mod.evaluate_clips(cor, ref_dev, dataloader_idx=dl, max_batch_samples=40000)
    suffix = f"/{names[dl]}" if names else ""
    assert set(mod.logged) == {f"test/torchmetrics_si_sdr{suffix}", f"test/torchmetrics_stoi{suffix}"}
    assert set(out) == {"si_sdr", "stoi"} and out["stoi"].shape == (5,)
    # float32 means of five values below 100 in magnitude: one float32 rounding (ulp 7.6e-6 at 64..128) between the two ways to sum
    for key, values in (("torchmetrics_si_sdr", out["si_sdr"]), ("torchmetrics_stoi", out["stoi"])):
        mean = float(values.double().mean())
        assert abs(float(mod.logged[f"test/{key}{suffix}"]) - mean) <= 1e-5
        assert abs(float(mod.metrics[key].compute()) - mean) <= 1e-5
    mod.evaluate_clips(cor[:2], ref_dev[:2], stage="validation", dataloader_idx=dl)   # the running state goes on: 7 clips now
    want = (float(out["stoi"].double().sum()) + float(out["stoi"][:2].double().sum())) / 7
    assert f"validation/torchmetrics_stoi{suffix}" in mod.logged and abs(float(mod.metrics["torchmetrics_stoi"].compute()) - want) <= 1e-5


@pytest.mark.parametrize("rate", [16000, 48000])
def test_eval_hook_with_lengths_scores_the_rows_alone(hip, rate):
    from vibravox_amd.augment import resample
    from vibravox_amd.lightning_modules.base_se import BaseSELightningModule

    lengths = (16001, 9000, 12000) if rate == 16000 else (48001, 30000)
    ref = [_f32(M.speech_like(f"hook{t}", 1, t, rate)[0]) for t in lengths]
    enh = [_f32(_noisy(x[None], 10.0, t + 5)[0]) for x, t in zip(ref, lengths)]
    t_max = max(lengths)
    r_flat, r_dev, r = fenced(ref, t_max)
    e_flat, e_dev, e = fenced(enh, t_max)
    mod = BaseSELightningModule(sample_rate=rate)
    mod.common_eval_logging("test", {"enhanced": e.unsqueeze(1), "reference": r.unsqueeze(1), "lengths": list(lengths)}, 0, 0)
    assert untouched(r_flat, r_dev) and untouched(e_flat, e_dev)     # at 48 kHz the slack is zeroed on a copy
    to16k = (lambda x: x) if rate == 16000 else (lambda x: resample(x, rate, 16000))
    pairs = [(to16k(_dev(a[None])).double().cpu().numpy(), to16k(_dev(b[None])).double().cpu().numpy()) for a, b in zip(enh, ref)]
    sdr = np.mean([float(M.si_sdr(a, b)[0]) for a, b in pairs])
    sti = np.array([float(M.stoi(a, b, 16000)[0]) for a, b in pairs])
    assert (sti != 1e-5).all()
    assert abs(float(mod.logged["test/torchmetrics_si_sdr"]) - sdr) <= SDR_TOL
    assert abs(float(mod.logged["test/torchmetrics_stoi"]) - sti.mean()) <= STOI_TOL
    assert abs(float(mod.metrics["torchmetrics_stoi"].compute()) - sti.mean()) <= STOI_TOL
