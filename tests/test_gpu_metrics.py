"""GPU: the SI-SDR / STOI kernels (vibravox_amd/metrics.py -> csrc/metrics.hip) against the float64 restatement in
tests/metrics_oracle.py, and the validation / test hooks of BaseSELightningModule."""
import numpy as np
import pytest
import torch

from tests import metrics_oracle as M

pytestmark = pytest.mark.gpu

STOI_TOL = 1e-6     # |device - oracle| per row; observed <= 5.5e-8 on the MI355X
SDR_TOL = 1e-4      # dB, up to 60 dB; observed <= 1.8e-6


def _noisy(x, snr_db, seed):
    n = np.random.RandomState(seed).randn(*x.shape)
    snr = np.broadcast_to(np.asarray(snr_db, np.float64), x.shape[:-1])[..., None]
    scale = np.sqrt((x ** 2).mean(-1, keepdims=True) / (n ** 2).mean(-1, keepdims=True)) * 10 ** (-snr / 20)
    return x + n * scale


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def batch():
    """The BASELINE validation shape: 32 speech-like clips of 31968 samples at 16 kHz, and a processed version of each at
    SNRs from -5 to 60 dB."""
    clean = M.speech_like("val", 32, 31968, 16000).astype(np.float32).astype(np.float64)
    snrs = np.array([-5, 0, 5, 10, 20, 30, 45, 60] * 4, np.float64)
    processed = _noisy(clean, snrs, 11).astype(np.float32).astype(np.float64)
    return clean, processed


def test_rows_keep_different_frame_counts(batch):
    clean, _ = batch
    counts = {len(M.kept_frames(M.resample(c, 16000))) for c in clean}
    assert len(counts) >= 8, counts


@pytest.mark.parametrize("fs", [16000, 10000])
def test_stoi_batch_against_oracle(hip, batch, fs):
    from vibravox_amd.metrics import stoi

    clean, processed = batch
    got = stoi(_dev(processed), _dev(clean), fs).cpu().numpy()
    want = M.stoi(processed, clean, fs)
    err = np.abs(got - want)
    print(f"[stoi fs={fs}] max|d - oracle| = {err.max():.2e}, d in [{want.min():.3f}, {want.max():.3f}]")
    assert got.shape == (32,)
    assert err.max() <= STOI_TOL, (err.max(), int(err.argmax()))


@pytest.mark.parametrize("fs,t", [(16000, 16001), (16000, 7777), (16000, 40003), (10000, 4100), (10000, 4000), (10000, 999)])
def test_stoi_single_clips_at_odd_lengths(hip, fs, t):
    """10 kHz stationary noise keeps every frame: 4100 samples leave exactly 30 STFT frames (one segment), 4000 leave 29
    (-> 1e-5), 999 leaves 5."""
    from vibravox_amd.metrics import stoi

    if fs == 10000:
        clean = np.random.RandomState(t).randn(1, t).astype(np.float32).astype(np.float64)
    else:
        clean = M.speech_like(f"odd{t}", 1, t, fs).astype(np.float32).astype(np.float64)
    processed = _noisy(clean, 3.0, t + 1).astype(np.float32).astype(np.float64)
    got = stoi(_dev(processed), _dev(clean), fs).cpu().numpy()
    want = M.stoi(processed, clean, fs)
    if fs == 10000 and t == 4000:
        assert want[0] == 1e-5
    if fs == 10000 and t == 4100:
        assert want[0] != 1e-5
    np.testing.assert_allclose(got, want, rtol=0, atol=STOI_TOL)


def test_stoi_shape_and_identity(hip, batch):
    from vibravox_amd.metrics import stoi

    clean = _dev(batch[0][:6]).reshape(2, 3, -1)
    d = stoi(clean, clean, 16000)
    assert d.shape == (2, 3) and d.is_cuda
    np.testing.assert_allclose(d.cpu().numpy(), 1.0, atol=1e-5)


def test_si_sdr_against_oracle_up_to_60_db(hip, batch):
    from vibravox_amd.metrics import si_sdr

    clean, processed = batch
    got = si_sdr(_dev(processed), _dev(clean)).cpu().numpy()
    want = M.si_sdr(processed, clean)
    err = np.abs(got - want)
    print(f"[si_sdr] max|dB - oracle| = {err.max():.2e} over [{want.min():.1f}, {want.max():.1f}] dB")
    assert want.max() > 59
    assert err.max() <= SDR_TOL, err.max()
    odd = M.speech_like("sdr", 3, 12345, 16000).astype(np.float32).astype(np.float64)
    got = si_sdr(_dev(0.3 * odd[::-1]), _dev(odd)).cpu().numpy()
    np.testing.assert_allclose(got, M.si_sdr(0.3 * odd[::-1], odd), rtol=0, atol=SDR_TOL)


def test_metric_classes_accumulate_like_torchmetrics(hip, batch):
    from vibravox_amd.metrics import ScaleInvariantSignalDistortionRatio, ShortTimeObjectiveIntelligibility

    clean, processed = batch
    for metric, oracle in ((ScaleInvariantSignalDistortionRatio(), M.si_sdr),
                           (ShortTimeObjectiveIntelligibility(16000), lambda p, t: M.stoi(p, t, 16000))):
        a = metric(_dev(processed[:20]), _dev(clean[:20]))
        metric.update(_dev(processed[20:]), _dev(clean[20:]))
        assert a.is_cuda and a.dim() == 0
        want = oracle(processed, clean)
        np.testing.assert_allclose(float(a), want[:20].mean(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(float(metric.compute()), want.mean(), rtol=0, atol=1e-4)
        metric.reset()
        with pytest.raises(RuntimeError):
            metric.compute()
        assert list(metric.state_dict().keys()) == []


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
def test_validation_hook_logs_si_sdr_and_stoi(hip, names):
    mod = _module()
    mod.dataloader_names = names
    air = M.speech_like("air", 4, 24000, 16000)
    bc = _noisy(air, 5.0, 5)
    batch = {"audio_body_conducted": _dev(bc).unsqueeze(1), "audio_airborne": _dev(air).unsqueeze(1)}
    dl = 1 if names else 0
    outputs = mod.validation_step(batch, 0, dl)
    step_keys = set(mod.logged)
    suffix = f"/{names[dl]}" if names else ""
    assert step_keys and all(k.startswith(("validation/generator/", "validation/discriminator/")) for k in step_keys)
    assert all(k.endswith(suffix) for k in step_keys)
    mod.on_validation_batch_end(outputs, batch, 0, dl)
    new = set(mod.logged) - step_keys
    assert new == {f"validation/torchmetrics_si_sdr{suffix}", f"validation/torchmetrics_stoi{suffix}"}
    enh = outputs["enhanced"].double().cpu().numpy()[:, 0]
    ref = outputs["reference"].double().cpu().numpy()[:, 0]
    assert abs(float(mod.logged[f"validation/torchmetrics_si_sdr{suffix}"]) - M.si_sdr(enh, ref).mean()) <= SDR_TOL
    assert abs(float(mod.logged[f"validation/torchmetrics_stoi{suffix}"]) - M.stoi(enh, ref, 16000).mean()) <= STOI_TOL
    mod.on_test_batch_end(mod.test_step(batch, 0, dl), batch, 0, dl)
    assert f"test/torchmetrics_stoi{suffix}" in mod.logged


def test_batch_without_reference_logs_no_metric(hip):
    mod = _module()
    air = M.speech_like("noref", 2, 16000, 16000)
    batch = {"audio_body_conducted": _dev(air).unsqueeze(1)}
    outputs = mod.validation_step(batch, 0)
    mod.on_validation_batch_end(outputs, batch, 0)
    assert not any("torchmetrics" in k for k in mod.logged)


def test_other_sample_rates_are_resampled_to_16k(hip):
    from vibravox_amd.augment import resample
    from vibravox_amd.lightning_modules.base_se import BaseSELightningModule

    mod = BaseSELightningModule(sample_rate=48000)
    ref = _dev(M.speech_like("48k", 2, 48000, 48000)).unsqueeze(1)
    enh = _dev(_noisy(ref.double().cpu().numpy(), 10.0, 9))
    mod.common_eval_logging("test", {"enhanced": enh, "reference": ref}, 0, 0)
    e16, r16 = (resample(x, 48000, 16000).double().cpu().numpy()[:, 0] for x in (enh, ref))
    assert abs(float(mod.logged["test/torchmetrics_stoi"]) - M.stoi(e16, r16, 16000).mean()) <= STOI_TOL
    assert abs(float(mod.logged["test/torchmetrics_si_sdr"]) - M.si_sdr(e16, r16).mean()) <= SDR_TOL
