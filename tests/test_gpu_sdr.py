"""GPU: the BSS-eval signal-to-distortion ratio (``eben_sdr`` through ``vibravox_amd.metrics.sdr``), ``inference.evaluate_clips(metrics=(...,
"sdr"))`` and the Lightning surface on top of it.

Every kernel case hands over views 4 bytes off the 16-byte grid inside a sentinel-fenced allocation with NaN behind every row's end and
asserts: the ragged call has the bits of every row alone (compared as int32, so NaN equals NaN), reversing the row order and widening the
buffer by 1000 changes no bit, and the fences and inputs are untouched.

Bar against the float64 oracle of every row ALONE (``tests/sdr_oracle.py``): ``ulp32(oracle) + 100 * ORACLE_SPREAD`` -- one float32 ulp
because the output is the float32 rounding of an fp64 value, and a hundred times the oracle's own two-route disagreement (measured here on
these inputs, 1.8e-12 dB) for a third summation order (segments, waves) and the Levinson recursion.  It holds for every row whose oracle
value lies in [-30, 60] dB, and every listed row must: none may be left out -- except the row of ONE sample without ``load_diag``.  A single
sample is proportional to its target whatever it holds, so coh = 1 for any implementation (+inf from both oracle routes; NaN with
``zero_mean``, which leaves a silent target); that row is held to the statement for proportional signals instead (nothing finite below
100 dB, respectively NaN), and with ``load_diag = 1e-3`` it is an ordinary 30.0 dB row under the bar.

[MI355X] observed maxima against the oracle (each test prints its own with -s): at most 0.500 float32 ulp of the oracle value (9.5e-7 dB below 32 dB) over all
30 (kind, L, setting) cases, i.e. the float32 rounding of the result and nothing else; L = 1 against the closed form 9.3e-7 dB; the 30 dB
single-sample row with load_diag 6.3e-13 dB; ragged against every row alone, reversed and widened: 0 bit differences; evaluate_clips
against every pair alone: 0 bit differences, also from 48 kHz."""
import functools

import numpy as np
import pytest
import torch

from tests import metrics_oracle as M
from tests import ragged_oracle as R
from tests import sdr_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FENCE = 64
SENTINEL = 12345.0
SLACK = 37                      # t_max is larger than the longest row
EVAL_LENGTHS = (16001, 12000, 9000, 7777)
EVAL_NAMES = ("si_sdr", "stoi", "sdr")


def _segment():
    from vibravox_amd import metrics as m

    return m.SDR_SEGMENT


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _noisy(x, snr_db, seed):
    n = np.random.RandomState(seed).randn(*x.shape)
    scale = np.sqrt((x ** 2).mean(-1, keepdims=True) / (n ** 2).mean(-1, keepdims=True)) * 10 ** (-snr_db / 20)
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


def run_ragged(targets, preds, L, zero_mean, load_diag, extra=0, reverse=False, lengths=None):
    """The rows (reversed, in a buffer ``extra`` wider) in fenced buffers through ``metrics.sdr``; checks fences and inputs; values in the
    rows' own order.  ``lengths``: a device table that replaces the rows' own lengths."""
    from vibravox_amd.metrics import sdr

    order = list(range(len(targets)))[::-1] if reverse else list(range(len(targets)))
    t = max(len(x) for x in targets) + SLACK + extra
    g_flat, g_dev, g = fenced(targets, t, order)
    p_flat, p_dev, p = fenced(preds, t, order)
    lens = [len(targets[i]) for i in order] if lengths is None else lengths
    got = sdr(p, g, lens, filter_length=L, zero_mean=zero_mean, load_diag=load_diag)
    assert got.shape == (len(order),) and got.dtype is torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert untouched(g_flat, g_dev) and untouched(p_flat, p_dev)
    back = np.empty_like(got)
    back[order] = got
    return back


def alone(targets, preds, L, zero_mean, load_diag):
    """The dense call on every row alone: a (1, n) buffer of its own, no lengths."""
    from vibravox_amd.metrics import sdr

    return np.array([float(sdr(_dev(p[None]), _dev(t[None]), None, L, zero_mean, load_diag).cpu()[0]) for t, p in zip(targets, preds)], np.float32)


def bar(oracle):
    return O.ulp32(oracle) + 100.0 * O.oracle_spread(_segment())


@pytest.mark.parametrize("L", O.FILTER_LENGTHS)
@pytest.mark.parametrize("kind", O.KINDS)
def test_sdr_rows_of_different_lengths(hip, kind, L):
    S = _segment()
    lengths = O.row_lengths(L, S)
    worst = 0.0
    for zero_mean, load_diag in O.SETTINGS:
        targets, preds = O.case_inputs(kind, L, S, zero_mean)
        assert [len(t) for t in targets] == lengths
        want = O.case(kind, L, S, zero_mean, load_diag)[0]
        got = run_ragged(targets, preds, L, zero_mean, load_diag)
        # the bits of every row alone, whatever else is in the batch, wherever the row stands and however wide the buffer is
        each = alone(targets, preds, L, zero_mean, load_diag)
        assert np.array_equal(_bits(got), _bits(each)), (zero_mean, load_diag, got, each)
        assert np.array_equal(_bits(run_ragged(targets, preds, L, zero_mean, load_diag, reverse=True)), _bits(each))
        assert np.array_equal(_bits(run_ragged(targets, preds, L, zero_mean, load_diag, extra=1000)), _bits(each))
        # the bar, on every row: none is left out but the single sample without load_diag (module docstring)
        keep = O.compared(want)
        assert keep[1:].all() and keep[0] == (load_diag is not None), (zero_mean, load_diag, want)
        with np.errstate(invalid="ignore"):     # inf - inf on the single sample
            err = np.abs(got.astype(np.float64) - want)
        print(f"[{kind} L={L} zero_mean={zero_mean} load_diag={load_diag}] oracle {np.array2string(want, precision=3)}; |device - oracle| = "
              f"{np.array2string(err, formatter=dict(float_kind=lambda v: f'{v:.2e}'))} (bar {np.array2string(bar(want), formatter=dict(float_kind=lambda v: f'{v:.2e}'))})")
        assert (err[keep] <= bar(want)[keep]).all(), (zero_mean, load_diag, err, bar(want))
        worst = max(worst, float((err[keep] / O.ulp32(want)[keep]).max()))
        if load_diag is None:
            if zero_mean:
                assert np.isnan(got[0]) and np.isnan(want[0])
            else:
                assert not (np.isfinite(got[0]) and got[0] < 100.0), got[0]
    print(f"[{kind} L={L}] largest |device - oracle| over the compared rows: {worst:.3f} float32 ulp of the oracle value")


@pytest.mark.parametrize("kind", O.KINDS)
def test_one_tap_is_si_sdr_without_eps(hip, kind):
    """L = 1 against the closed-form float64 SI-SDR without eps: coh = rho^2 -- a check that leans on nobody's memory of torchmetrics."""
    S = _segment()
    for zero_mean in (False, True):
        targets, preds = O.case_inputs(kind, 1, S, zero_mean)
        want = np.array([O.si_sdr_no_eps(p, t, zero_mean) for t, p in list(zip(targets, preds))[1:]])
        got = run_ragged(targets, preds, 1, zero_mean, None)[1:]
        err = np.abs(got.astype(np.float64) - want)
        print(f"[{kind} zero_mean={zero_mean}] closed form {np.array2string(want, precision=3)}; |device - closed form| = "
              f"{np.array2string(err, formatter=dict(float_kind=lambda v: f'{v:.2e}'))}")
        assert O.compared(want).all() and (err <= bar(want)).all(), (err, want)


def test_rows_that_have_no_value_leave_their_neighbours_alone(hip):
    """Device lengths 0, -1 and t_max + 1, and a silent target: NaN.  preds == target: nothing finite below 100 dB.  The live rows between
    them keep the bits they have alone."""
    S, L = _segment(), 64
    targets, preds = O.inputs("speech", L, S)
    live = [1, 4, 6]                                  # 300, S + 1 and S + L samples
    each = alone([targets[i] for i in live], [preds[i] for i in live], L, False, None)
    n = len(targets[4])
    filler_t, filler_p = targets[4], preds[4]
    rows_t = [filler_t, targets[1], filler_t, targets[4], filler_t, np.zeros(n), targets[6], filler_t]
    rows_p = [filler_p, preds[1], filler_p, preds[4], filler_p, filler_p, preds[6], filler_t]
    t_max = max(len(x) for x in rows_t) + SLACK
    lens = torch.tensor([0, 300, -1, n, t_max + 1, n, len(targets[6]), n], dtype=torch.int32, device=DEV)
    got = run_ragged(rows_t, rows_p, L, False, None, lengths=lens)
    assert np.isnan(got[[0, 2, 4]]).all(), got
    assert np.isnan(got[5]), got                      # silent target: 0 / 0, there is no eps
    assert not (np.isfinite(got[7]) and got[7] < 100.0), got
    assert np.array_equal(_bits(got[[1, 3, 6]]), _bits(each)), (got, each)
    # zero padding behind a row changes nothing: the row alone in a buffer of zeros, scored over the whole buffer
    from vibravox_amd.metrics import SignalDistortionRatio, sdr

    padded = lambda x: _dev(np.concatenate([x, np.zeros(777)])[None])
    whole = sdr(padded(preds[4]), padded(targets[4]), None, L)
    assert abs(float(whole[0]) - float(each[1])) <= float(O.ulp32(each[1]))
    # the class: the mean of the rows' values, no state_dict entries
    metric = SignalDistortionRatio(filter_length=L)
    rows = torch.stack([_dev(np.concatenate([x, np.zeros(len(targets[6]) - len(x))])) for x in (targets[1], targets[4], targets[6])])
    rows_hat = torch.stack([_dev(np.concatenate([x, np.zeros(len(targets[6]) - len(x))])) for x in (preds[1], preds[4], preds[6])])
    mean = metric(rows_hat, rows, lengths=[300, n, len(targets[6])])
    assert abs(float(mean) - float(each.astype(np.float64).mean())) <= 1e-5 and abs(float(metric.compute()) - float(mean)) <= 1e-5
    assert list(metric.state_dict().keys()) == []


# ---- evaluate_clips ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(fs=16000):
    lengths = tuple(t * (fs // 16000) for t in EVAL_LENGTHS)
    gen = R.formula_generator(1, 32)[0].to(DEV)
    ref = [_f32(M.speech_like(f"ev{t}", 1, t, fs)[0]) for t in lengths]
    cor = [_f32(_noisy(x[None], 5.0 if fs == 16000 else 10.0, t + 3)[0]) for x, t in zip(ref, lengths)]
    return gen, [_dev(x).reshape(1, 1, -1) for x in cor], [_dev(x).reshape(1, 1, -1) for x in ref], lengths


@pytest.mark.parametrize("fs", [16000, 48000])
def test_evaluate_clips_sdr_has_the_bits_of_every_pair_alone(hip, fs):
    from vibravox_amd import metrics as m
    from vibravox_amd import ragged
    from vibravox_amd.augment import resample
    from vibravox_amd.inference import evaluate_clips

    gen, cor, ref_dev, lengths = corpus(fs)
    out = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, metrics=EVAL_NAMES, return_enhanced=True)
    assert list(out) == list(EVAL_NAMES) + ["enhanced"]
    assert out["sdr"].shape == (len(lengths),) and out["sdr"].dtype is torch.float32 and out["sdr"].is_cuda and torch.isfinite(out["sdr"]).all()
    for i in range(len(lengths)):
        pair = evaluate_clips(gen, [cor[i]], [ref_dev[i]], sample_rate=fs, metrics=EVAL_NAMES)
        for name in EVAL_NAMES:
            assert same_bits(out[name][i : i + 1], pair[name]), (name, i, out[name][i], pair[name])
        # and of metrics.sdr on the returned enhanced clip against the cut reference, at 16 kHz
        n = ragged.cut_length(gen, lengths[i])
        e16, g16 = out["enhanced"][i].reshape(1, n), ref_dev[i].reshape(1, -1)[:, :n].contiguous()
        if fs != 16000:
            e16, g16 = resample(e16, fs, 16000), resample(g16, fs, 16000)
        assert same_bits(out["sdr"][i : i + 1], m.sdr(e16, g16).reshape(1)), i
    # the other metrics: the bits of the call that does not name "sdr"; two batches and another order of names: the same bits
    without = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, metrics=("si_sdr", "stoi"))
    assert list(without) == ["si_sdr", "stoi"] and all(same_bits(without[k], out[k]) for k in without)
    small = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, max_batch_samples=40000 * (fs // 16000), metrics=EVAL_NAMES[::-1])
    assert list(small) == list(EVAL_NAMES[::-1]) and all(same_bits(small[k], out[k]) for k in EVAL_NAMES)
    # a filter of 512 taps explains more than one of 16, and at least as much as plain scaling: SDR >= SI-SDR without eps
    short = evaluate_clips(gen, cor, ref_dev, sample_rate=fs, metrics=("sdr",), sdr_filter_length=16)["sdr"]
    print(f"[evaluate_clips at {fs} Hz] sdr {np.array2string(out['sdr'].cpu().numpy(), precision=4)}, 16 taps "
          f"{np.array2string(short.cpu().numpy(), precision=4)}, si_sdr {np.array2string(out['si_sdr'].cpu().numpy(), precision=4)}")
    assert (out["sdr"] >= short).all() and (short > out["si_sdr"] - 1e-3).all() and not same_bits(short, out["sdr"])


def test_evaluate_clips_launches_sdr_only_when_it_is_named(hip, monkeypatch):
    from vibravox_amd import metrics as m
    from vibravox_amd.inference import evaluate_clips

    gen, cor, ref_dev, _ = corpus()
    seen = []
    real = m.check
    monkeypatch.setattr(m, "check", lambda rc, what="": (seen.append(what), real(rc, what))[1])
    evaluate_clips(gen, cor, ref_dev)
    assert seen == ["si_sdr_ragged", "stoi_ragged"]
    del seen[:]
    evaluate_clips(gen, cor, ref_dev, metrics=EVAL_NAMES)
    assert seen == ["si_sdr_ragged", "stoi_ragged", "sdr"]      # one metrics.sdr call per ragged batch


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


def test_module_evaluate_clips_logs_the_corpus_mean_of_sdr(hip):
    mod = _module()
    _, cor, ref_dev, _ = corpus()
    out = mod.evaluate_clips(cor, ref_dev, metrics=EVAL_NAMES)
    assert set(mod.logged) == {"test/torchmetrics_si_sdr", "test/torchmetrics_stoi", "test/sdr"}
    assert set(mod.metrics.keys()) == {"torchmetrics_si_sdr", "torchmetrics_stoi"}           # the reference's collection, unchanged
    assert torch.isfinite(out["sdr"]).all()
    assert abs(float(mod.logged["test/sdr"]) - float(out["sdr"].double().mean())) <= 1e-5
