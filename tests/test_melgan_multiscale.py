"""CPU (no GPU): MelganMultiScalesDiscriminator's host side -- the Kaiser-windowed sinc tables against an independent float64
closed form, the unchanged Hann default, the C ABI of the multi-rate kernels, the state_dict contract, same-seed
construction and the Hydra option."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 14.769656459379492


def kaiser_closed_form(orig_freq, new_freq, width_lp=6, rolloff=0.99, beta=BETA):
    """torchaudio's _get_sinc_resample_kernel with the Kaiser window, written out in numpy float64 (beta rounded to float32
    as torchaudio's default-dtype tensor does)."""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = math.ceil(width_lp * orig / base)
    j = np.arange(-width, width + orig, dtype=np.float64)
    p = np.arange(new, dtype=np.float64)
    t = np.clip((-p[:, None] / new + j[None, :] / orig) * base, -width_lp, width_lp)
    b = float(np.float32(beta))
    window = np.i0(b * np.sqrt(1.0 - (t / width_lp) ** 2)) / np.i0(b)
    x = t * np.pi
    sinc = np.where(x == 0, 1.0, np.sin(x) / np.where(x == 0, 1.0, x))
    return sinc * window * (base / orig), width, orig, new


@pytest.mark.parametrize("rates", [(16000, 8000), (16000, 4000), (24000, 3000), (22050, 5512)])
def test_kaiser_tables_match_float64_closed_form(rates):
    from vibravox_amd.augment import sinc_resample_kernel

    k, width, orig, new = sinc_resample_kernel(*rates, resampling_method="sinc_interp_kaiser")
    ref, rw, ro, rn = kaiser_closed_form(*rates)
    assert (width, orig, new) == (rw, ro, rn)
    assert k.dtype is torch.float32 and tuple(k.shape) == ref.shape == (new, 2 * width + orig)
    assert float(np.abs(k.numpy().astype(np.float64) - ref).max()) <= 1e-7


def test_kaiser_shapes_of_the_discriminator_scales():
    from vibravox_amd.augment import sinc_resample_kernel

    assert sinc_resample_kernel(16000, 8000, resampling_method="sinc_interp_kaiser")[1:] == (13, 2, 1)
    assert sinc_resample_kernel(16000, 4000, resampling_method="sinc_interp_kaiser")[1:] == (25, 4, 1)
    k, width, orig, new = sinc_resample_kernel(22050, 22050 // 4, resampling_method="sinc_interp_kaiser")
    assert (width, orig, new) == (25, 11025, 2756) and tuple(k.shape) == (2756, 11075)
    with pytest.raises(ValueError):
        sinc_resample_kernel(2, 1, resampling_method="sinc_interp_linear")


def test_hann_default_is_unchanged():
    from vibravox_amd.augment import sinc_resample_kernel

    z = np.load(os.path.join(ROOT, "tests", "golden", "resample_kernels.npz"))
    keys = [k for k in z.files if re.fullmatch(r"\d+_\d+", k)]
    assert len(keys) >= 5
    for key in keys:
        a, b = (int(v) for v in key.split("_"))
        want = z[key]
        for k in (sinc_resample_kernel(a, b)[0], sinc_resample_kernel(a, b, resampling_method="sinc_interp_hann")[0]):
            assert k.dtype is torch.float32 and k.shape == want.shape
            np.testing.assert_array_equal(k.numpy(), want)


NEW_ABI = ("eben_multirate_down", "eben_multirate_down_adjoint", "eben_resample_adjoint")


def test_multirate_abi_is_declared_bound_and_exported():
    from vibravox_amd import _lib

    header = open(os.path.join(ROOT, "include", "eben_hip.h")).read()
    declared = set(re.findall(r"EBEN_API\s+[\w\s\*]+?\b(eben_\w+)\s*\(", header))
    assert int(re.search(r"#define EBEN_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 6
    lib = _lib.load()
    assert lib.eben_version() == 6
    for name in NEW_ABI:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_multirate_abi_rejects_bad_plans_without_gpu():
    import ctypes

    from vibravox_amd import _lib

    lib = _lib.load()
    w = (ctypes.c_int * 6)(13, 25, 49, 97, 194, 400)
    outs = (ctypes.c_void_p * 6)(*([1] * 6))
    assert lib.eben_multirate_down(1, 1, w, outs, 2, 100, 1, None) < 0      # nothing to downsample
    assert lib.eben_multirate_down(1, 1, w, outs, 2, 100, 7, None) < 0      # beyond the fused path's 6 scales
    assert lib.eben_multirate_down(None, 1, w, outs, 2, 100, 3, None) < 0
    assert lib.eben_resample_adjoint(1, 1, 1, 2, 10, 6, 2, 1, 13, 0, None) < 0   # t_out beyond ceil(new * t_in / orig)


def _melgan_keys_shapes(disc):
    return {k: tuple(v.shape) for k, v in disc.state_dict().items()}


def test_state_dict_is_three_melgan_discriminators():
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import DiscriminatorMelGAN, MelganMultiScalesDiscriminator

    ms = MelganMultiScalesDiscriminator(16000)
    one = _melgan_keys_shapes(DiscriminatorMelGAN(0.2))
    want = {f"discriminators.{s}.{k}": v for s in range(3) for k, v in one.items()}
    assert _melgan_keys_shapes(ms) == want
    assert not any("downsamplers" in k for k in ms.state_dict())
    assert len(ms.discriminators) == len(ms.downsamplers) == 3
    assert [(d.orig_freq, d.new_freq) for d in ms.downsamplers] == [(16000, 16000), (16000, 8000), (16000, 4000)]
    assert sum(p.numel() for p in ms.parameters()) > 1e3


def test_same_seed_gives_sequentially_built_discriminators():
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import DiscriminatorMelGAN, MelganMultiScalesDiscriminator

    torch.manual_seed(3)
    ms = MelganMultiScalesDiscriminator(16000, scales=3, alpha_leaky_relu=0.2)
    torch.manual_seed(3)
    seq = [DiscriminatorMelGAN(0.2) for _ in range(3)]
    for s, d in enumerate(seq):
        for k, v in d.state_dict().items():
            assert torch.equal(ms.state_dict()[f"discriminators.{s}.{k}"], v), (s, k)


def test_cpu_tensors_raise():
    from vibravox_amd import ops
    from vibravox_amd._lib import EbenError

    x = torch.zeros(1, 1, 64)
    with pytest.raises(EbenError):
        ops.multirate_downsample(x, 16000, 3)
    with pytest.raises(EbenError):
        ops.kaiser_resample(x, 22050, 5512)


def test_hydra_option_composes_and_instantiates():
    import run

    cfg = run.compose(["lightning_module/dnn_module@lightning_module.discriminator=melgan_multi_scales_from_scratch"])
    node = cfg["lightning_module"]["discriminator"]
    assert node == {"_target_": "vibravox_amd.torch_modules.dnn.melgan_discriminator.MelganMultiScalesDiscriminator",
                    "sample_rate": 16000, "scales": 3, "alpha_leaky_relu": 0.2}
    disc = run.instantiate(node)
    assert type(disc).__name__ == "MelganMultiScalesDiscriminator" and disc.sample_rate == 16000 and len(disc.discriminators) == 3
    assert run.compose([])["lightning_module"]["discriminator"]["_target_"].endswith("DiscriminatorEBENMultiScales")
