"""CPU (no GPU): the options of MultiResolutionSTFTLoss beyond multi_stft.yaml -- which constructor arguments are built and which
raise, the Slaney mel filterbank restated from librosa and the banded forms of it the kernels read, the windows the folded STFT forms
may take, the Hydra override of the reference's commented ``scale: "mel"`` / ``n_bins: 128`` lines, and the float64 restatement of
the terms (tests/stft_terms_oracle.py) against the project's oracle of the default configuration."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from vibravox_amd.torch_modules.losses.mrstft_loss import (  # noqa: E402
    WINDOWS, MultiResolutionSTFTLoss, hz_to_mel, mel_bands, mel_filterbank, mel_to_hz, window_foldable)

REF = dict(fft_sizes=(512, 1024, 2048), hop_sizes=(50, 120, 240), win_lengths=(240, 600, 1200), sample_rate=16000, perceptual_weighting=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# constructor
# ---------------------------------------------------------------------------------------------------------------------------------
ACCEPT = [
    dict(scale="mel", n_bins=128),
    dict(scale="mel", n_bins=40, w_lin_mag=1.0),
    dict(w_sc=1.0, w_log_mag=0.0, w_lin_mag=1.0),
    dict(w_sc=0.0, w_log_mag=1.0, w_lin_mag=0.0),
    dict(w_sc=0.5, w_log_mag=2.0, w_lin_mag=1.0, mag_distance="L2"),
    dict(mag_distance="L1", reduction="mean", output="loss", device=None, eps=1e-8),
    dict(device="cuda"),
] + [dict(window=w) for w in WINDOWS]

REJECT = [
    (dict(scale="chroma", n_bins=12), NotImplementedError),
    (dict(w_phs=1.0), NotImplementedError),
    (dict(scale_invariance=True), NotImplementedError),
    (dict(reduction="sum"), NotImplementedError),
    (dict(reduction="none"), NotImplementedError),
    (dict(output="full"), NotImplementedError),
    (dict(window="gaussian_window"), NotImplementedError),
    (dict(w_sc=0.0, w_log_mag=0.0, w_lin_mag=0.0), NotImplementedError),
    (dict(mag_distance="L3"), ValueError),
    (dict(scale="mel", n_bins=None), ValueError),
    (dict(scale="mel", n_bins=600), ValueError),          # n_bins > n_fft 512
    (dict(scale="mel", n_bins=128, sample_rate=None, perceptual_weighting=False), ValueError),
    (dict(no_such_argument=1), TypeError),
]


@pytest.mark.parametrize("kw", ACCEPT, ids=[repr(k) for k in ACCEPT])
def test_constructor_accepts(kw):
    loss = MultiResolutionSTFTLoss(**{**REF, **kw})
    assert loss.state_dict() == {}, "every table stays out of the state_dict"


@pytest.mark.parametrize("kw,exc", REJECT, ids=[repr(k) for k, _ in REJECT])
def test_constructor_rejects(kw, exc):
    with pytest.raises(exc):
        MultiResolutionSTFTLoss(**{**REF, **kw})


def test_default_configuration_is_recognised():
    """The configurations that stay on the default kernels (stft._YamlTerms), whatever spelling of the defaults they use."""
    assert MultiResolutionSTFTLoss(**REF).default_terms
    assert MultiResolutionSTFTLoss(**REF, window="hann_window", w_sc=1, w_log_mag=1, w_lin_mag=0, w_phs=0, mag_distance="L1",
                                   reduction="mean", output="loss", scale=None).default_terms
    for kw in ACCEPT[:5] + [dict(window="hamming_window")]:
        assert not MultiResolutionSTFTLoss(**{**REF, **kw}).default_terms, kw


# ---------------------------------------------------------------------------------------------------------------------------------
# mel scale and filterbank
# ---------------------------------------------------------------------------------------------------------------------------------
def test_slaney_scale_break_and_round_trip():
    assert hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12)
    assert hz_to_mel(200.0 / 3) == pytest.approx(1.0, abs=1e-12)               # linear part: 200/3 Hz per mel
    assert hz_to_mel(6400.0) - hz_to_mel(1000.0) == pytest.approx(27.0, abs=1e-9)   # log part: 27 mel per factor 6.4
    lo = hz_to_mel(1000.0 - 1e-6)
    assert abs(lo - 15.0) < 1e-7                                                  # continuous at the break
    f = np.concatenate((np.linspace(0, 8000, 1001), [999.9999, 1000.0, 1000.0001, 22050.0]))
    np.testing.assert_allclose(mel_to_hz(hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)
    m = np.linspace(0, 60, 601)
    np.testing.assert_allclose(hz_to_mel(mel_to_hz(m)), m, rtol=1e-12, atol=1e-12)


MELS = [(16000, 512, 128), (16000, 1024, 128), (16000, 2048, 128), (16000, 2048, 40), (22050, 1024, 80), (16000, 511, 64)]


@pytest.mark.parametrize("sr,n_fft,n_mels", MELS)
def test_mel_filterbank_structure(sr, n_fft, n_mels):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fb = mel_filterbank(sr, n_fft, n_mels)
    assert fb.dtype == np.float32 and fb.shape == (n_mels, n_fft // 2 + 1)
    assert (fb >= 0).all()
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    edges = mel_to_hz(np.linspace(0, hz_to_mel(sr / 2), n_mels + 2))
    inside = np.zeros(fb.shape[1], np.int64)
    for m in range(n_mels):
        nz = np.flatnonzero(fb[m])
        assert nz.size, m
        assert (np.diff(nz) == 1).all(), f"filter {m}'s support is not one contiguous range"
        # the support is the open interval between the outer edges; the triangle rises up to its centre frequency and falls after
        # it, so its peak is one of the two bins around the centre, and no bin exceeds the peak value 2 / (f[m+2] - f[m]) it takes there
        assert freqs[nz[0]] > edges[m] and freqs[nz[-1]] < edges[m + 2]
        left, right = nz[freqs[nz] <= edges[m + 1]], nz[freqs[nz] >= edges[m + 1]]
        assert (np.diff(fb[m, left]) >= 0).all() and (np.diff(fb[m, right]) <= 0).all(), m
        peak = nz[np.argmax(fb[m, nz])]
        assert peak in set(left[-1:]) | set(right[:1]), (m, peak)
        assert fb[m].max() <= np.float32(2.0 / (edges[m + 2] - edges[m])) * (1 + 2.0 ** -22), m
        inside[nz] += 1
        # Slaney norm: area sum_k F[m, k] * (sr / n_fft) ~= 1 once the triangle spans many bins
        if nz.size >= 16:
            assert abs(fb[m].astype(np.float64).sum() * sr / n_fft - 1.0) < 0.05, (m, nz.size)
    assert inside.max() <= 2, "a bin lies in more than two filters"


def test_mel_filterbank_values_restated():
    """A few entries recomputed by hand from the definition (2 / (f[m+2] - f[m]) x triangle), float64, to float32's rounding."""
    sr, n_fft, n_mels = 16000, 1024, 128
    fb = mel_filterbank(sr, n_fft, n_mels)
    edges = mel_to_hz(np.linspace(0.0, hz_to_mel(8000.0), n_mels + 2))
    for m, k in ((0, 1), (10, 7), (64, 90), (127, 500)):
        f = k * sr / n_fft
        tri = max(0.0, min((f - edges[m]) / (edges[m + 1] - edges[m]), (edges[m + 2] - f) / (edges[m + 2] - edges[m + 1])))
        want = tri * 2.0 / (edges[m + 2] - edges[m])
        assert fb[m, k] == pytest.approx(want, rel=3e-7, abs=1e-12), (m, k)


def test_empty_filter_warns_as_librosa():
    with pytest.warns(UserWarning, match="Empty filters"):
        mel_filterbank(8000, 64, 40)


@pytest.mark.parametrize("sr,n_fft,n_mels", MELS)
def test_banded_tables_reproduce_the_dense_product_and_its_adjoint(sr, n_fft, n_mels):
    """mel_bands' forward gather (filter ranges) and adjoint gather (each bin's <= 2 filters) against fb @ M and fb^T @ G."""
    fb = mel_filterbank(sr, n_fft, n_mels)
    lo, off, w, bin_m, bin_w = (t.numpy() for t in mel_bands(fb))
    bins = fb.shape[1]
    g = np.random.default_rng(n_fft + n_mels)
    mag = g.standard_normal((bins, 7))
    grad = g.standard_normal((n_mels, 7))
    fwd = np.stack([w[off[m]:off[m + 1]].astype(np.float64) @ mag[lo[m]:lo[m] + off[m + 1] - off[m]] for m in range(n_mels)])
    np.testing.assert_allclose(fwd, fb.astype(np.float64) @ mag, rtol=0, atol=1e-12)
    pairs = bin_m.reshape(bins, 2)
    adj = np.zeros((bins, 7))
    for k in range(bins):
        for q in range(2):
            if pairs[k, q] >= 0:
                adj[k] += float(bin_w[2 * k + q]) * grad[pairs[k, q]]
    np.testing.assert_allclose(adj, fb.astype(np.float64).T @ grad, rtol=0, atol=1e-12)
    assert (lo >= 0).all() and (lo + np.diff(off) <= bins).all() and pairs.max() < n_mels


def test_module_mel_tables():
    loss = MultiResolutionSTFTLoss(**REF, scale="mel", n_bins=128)
    for i, n_fft in enumerate(REF["fft_sizes"]):
        assert torch.equal(loss.get_buffer(f"fb_{i}"), torch.from_numpy(mel_filterbank(16000, n_fft, 128)))
    (p0, *_) = loss._build_plans()
    assert p0.mel[0] == 128 and p0.mel[1].dtype == torch.int32 and p0.mel[3].dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# windows and the folded forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,foldable", [("hann_window", True), ("blackman_window", True), ("bartlett_window", True),
                                             ("hamming_window", False), ("kaiser_window", False)])
def test_math_for_takes_dense_for_windows_the_fold_cannot_take(window, foldable):
    loss = MultiResolutionSTFTLoss(**REF, window=window)
    for p in loss._build_plans():
        assert p.foldable == foldable == window_foldable(window, p.win)
        for mode in ("folded", "bf16x3", "folded_x3", "folded_x6"):
            assert p.math_for(mode) == (mode if foldable else "dense")
        assert p.math_for("dense") == "dense"


def test_window_basis_matches_torch_window():
    from vibravox_amd.torch_modules.losses.mrstft_loss import windowed_dft_basis
    for window in WINDOWS:
        basis = windowed_dft_basis(16, 10, window)[:, 0].double()
        w = getattr(torch, window)(10, dtype=torch.float64)
        assert torch.allclose(basis[0], w.float().double(), rtol=1e-7, atol=0), window   # bin 0's cosine row is the window itself


def test_folded_modes_reproduce_torch_stft_for_foldable_windows():
    """Where a window is foldable, the folded contraction (the right half of the basis against the even / odd parts of a frame)
    equals the dense one to float64 rounding: what the folded path on the device relies on."""
    n_fft, hop, win = 512, 50, 240
    x = torch.randn(2, 3000, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    for window in WINDOWS:
        loss = MultiResolutionSTFTLoss(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,), window=window)
        (p,) = loss._build_plans()
        if p.math_for("folded") != "folded":
            continue
        frames = p.frames(3000)
        q = torch.arange(frames).unsqueeze(0) * hop + torch.arange(win).unsqueeze(1) - p.pad
        q = torch.where(q < 0, -q, q)
        q = torch.where(q >= 3000, 2 * 2999 - q, q)
        fr = x[:, q]                                                    # (rows, win, frames)
        basis = p.basis_f[:, :, 0].double()
        h, bins = win // 2, p.bins
        m = torch.arange(1, h)
        e = torch.cat((fr[:, h:h + 1], fr[:, h + m] + fr[:, h - m]), 1)
        o = torch.cat((torch.zeros_like(fr[:, :1]), fr[:, h + m] - fr[:, h - m]), 1)
        folded = torch.cat((basis[:bins, h:] @ e, basis[bins:, h:] @ o), 1)
        dense = basis @ fr
        assert float((folded - dense).abs().max()) <= 1e-5 * float(dense.abs().max()), window


# ---------------------------------------------------------------------------------------------------------------------------------
# Hydra override and the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_run_py_mel_override_composes_and_instantiates():
    import run

    cfg = run.compose(["+lightning_module.reconstructive_loss_freq_fn.scale=mel", "+lightning_module.reconstructive_loss_freq_fn.n_bins=128"])
    node = cfg["lightning_module"]["reconstructive_loss_freq_fn"]
    assert node == {"_target_": "vibravox_amd.torch_modules.losses.mrstft_loss.MultiResolutionSTFTLoss", "fft_sizes": [512, 1024, 2048],
                    "hop_sizes": [50, 120, 240], "win_lengths": [240, 600, 1200], "sample_rate": 16000, "perceptual_weighting": True,
                    "scale": "mel", "n_bins": 128}
    loss = run.instantiate(node)
    assert loss.scale == "mel" and loss.n_bins == 128 and not loss.default_terms
    assert run.instantiate(run.compose([])["lightning_module"]["reconstructive_loss_freq_fn"]).default_terms


def test_restatement_of_the_default_matches_the_project_oracle():
    from oracle import eben_oracle as O
    from stft_terms_oracle import mrstft_terms_loss

    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 1, 4000, generator=g, dtype=torch.float64), torch.randn(2, 1, 4000, generator=g, dtype=torch.float64)
    fir = O.a_weighting_fir(16000).double()
    geo = dict(fft_sizes=REF["fft_sizes"], hop_sizes=REF["hop_sizes"], win_lengths=REF["win_lengths"])
    a = mrstft_terms_loss(x, y, **geo, fir=fir)
    b = O.mrstft_loss(x, y, **geo, perceptual_weighting=True, fir=fir)
    assert math.isclose(float(a), float(b), rel_tol=1e-12)
    # the terms by weight: linear in the weights, L2 differs from L1
    kw = dict(**geo, fir=fir, scale="mel", n_bins=64)
    parts = [float(mrstft_terms_loss(x, y, **kw, w_sc=ws, w_log_mag=wl, w_lin_mag=wn)) for ws, wl, wn in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    mixed = float(mrstft_terms_loss(x, y, **kw, w_sc=0.5, w_log_mag=2.0, w_lin_mag=1.0))
    assert math.isclose(mixed, 0.5 * parts[0] + 2.0 * parts[1] + parts[2], rel_tol=1e-12)
    assert float(mrstft_terms_loss(x, y, **kw, mag_distance="L2")) != float(mrstft_terms_loss(x, y, **kw))
