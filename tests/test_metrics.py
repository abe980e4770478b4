"""CPU (no GPU): the float64 SI-SDR / STOI restatement (tests/metrics_oracle.py) has the properties STOI and SI-SDR have
whatever pystoi's exact conventions are; the metrics ABI is declared, bound and exported; the public API has no CPU path;
the evaluation metrics add no state_dict keys."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noisy(x, snr_db, seed):
    n = np.random.RandomState(seed).randn(*x.shape)
    scale = np.sqrt((x ** 2).mean(-1, keepdims=True) / (n ** 2).mean(-1, keepdims=True)) * 10 ** (-snr_db / 20)
    return x + n * scale


@pytest.fixture(scope="module")
def speech():
    return M.speech_like("cpu", 3, 24000, 16000)


def test_stoi_of_a_signal_with_itself_is_one(speech):
    np.testing.assert_allclose(M.stoi(speech, speech, 16000), 1.0, atol=1e-9)


def test_stoi_falls_monotonically_with_noise(speech):
    d = np.array([M.stoi(_noisy(speech, snr, 7), speech, 16000) for snr in (20, 10, 0, -5)])
    assert np.all(np.diff(d, axis=0) < 0), d


def test_stoi_is_invariant_to_scaling_the_processed_signal(speech):
    y = _noisy(speech, 5, 3)
    np.testing.assert_allclose(M.stoi(3.7 * y, speech, 16000), M.stoi(y, speech, 16000), atol=1e-9)


def test_fewer_than_thirty_frames_gives_1e_5():
    # stationary noise at 10 kHz keeps every frame: 4000 samples -> 30 frames -> 29 STFT frames after overlap-add
    x = np.random.RandomState(0).randn(4000)
    assert len(M.kept_frames(x)) == 30
    assert M.stoi_clip(x, x + 0.1, 10000) == 1e-5
    x = np.random.RandomState(0).randn(4100)   # 31 frames -> 30 STFT frames: one segment
    assert len(M.kept_frames(x)) == 31
    assert M.stoi_clip(x, x, 10000) == pytest.approx(1.0)


def test_kept_frame_overlap_add_equals_an_explicit_loop():
    f = np.random.RandomState(1).randn(9, M.N_FRAME)
    np.testing.assert_array_equal(M.overlap_add(f), M.overlap_add_loop(f))
    assert len(M.overlap_add(f)) == (9 + 1) * (M.N_FRAME // 2)


def test_third_octave_matrix():
    obm, edges = M.thirdoct()
    assert obm.shape == (15, 257)
    assert edges[:, 0].tolist() == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert edges[:, 1].tolist() == [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]
    for b, (lo, hi) in enumerate(edges):
        assert obm[b].sum() == hi - lo and obm[b, lo:hi].all()


def test_polyphase_sum_equals_resample_poly():
    x = M.speech_like("rs", 1, 3001, 16000)[0]
    a, b = M.resample(x, 16000), M.resample_direct(x, 16000)
    assert len(a) == len(b) == math.ceil(3001 * 5 / 8)
    np.testing.assert_allclose(a, b, atol=1e-12)


def test_si_sdr_of_scaled_target_plus_orthogonal_noise():
    rs = np.random.RandomState(2)
    t = rs.randn(4, 5000)
    n = rs.randn(4, 5000)
    n -= (n * t).sum(-1, keepdims=True) / (t * t).sum(-1, keepdims=True) * t   # orthogonal to t
    a = np.array([0.5, 1.0, 2.0, 10.0])[:, None]
    want = 10 * np.log10(a[:, 0] ** 2 * (t * t).sum(-1) / (n * n).sum(-1))
    np.testing.assert_allclose(M.si_sdr(a * t + n, t), want, atol=1e-6)


def test_product_resample_table_matches_the_oracle():
    from vibravox_amd.metrics import stoi_resample_table

    h, up, down = stoi_resample_table(16000)
    hr, p, q = M.resample_filter(16000)
    assert (up, down) == (p, q) == (5, 8)
    assert len(h) == 2 * 290 + 1
    np.testing.assert_allclose(h, p * hr, rtol=0, atol=1e-15)


def test_metrics_abi_is_declared_bound_and_exported():
    from vibravox_amd import _lib

    header = open(os.path.join(ROOT, "include", "eben_hip.h")).read()
    for name in ("eben_si_sdr", "eben_stoi_workspace", "eben_stoi"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.eben_stoi_workspace(32, 31968, 16000) > 0
        assert lib.eben_stoi_workspace(0, 31968, 16000) == 0


def test_metrics_have_no_cpu_path():
    from vibravox_amd import metrics
    from vibravox_amd._lib import EbenError

    x = torch.zeros(2, 4000)
    with pytest.raises(EbenError):
        metrics.si_sdr(x, x)
    with pytest.raises(EbenError):
        metrics.stoi(x, x, 16000)
    with pytest.raises(ValueError):
        metrics.si_sdr(x, x[:1])


def test_eval_metrics_add_no_state_dict_keys():
    from functools import partial

    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    gen, disc = EBENGenerator(m=4, n=32, p=2), DiscriminatorEBENMultiScales(q=4, min_channels=24)
    opt = partial(FusedAdam, lr=3e-4)
    mod = EBENLightningModule(sample_rate=16000, generator=gen, discriminator=disc, generator_optimizer=opt, discriminator_optimizer=opt)
    want = [f"generator.{k}" for k in gen.state_dict()] + [f"discriminator.{k}" for k in disc.state_dict()]
    assert sorted(mod.state_dict().keys()) == sorted(want)
    assert set(mod.metrics.keys()) == {"torchmetrics_si_sdr", "torchmetrics_stoi"}
