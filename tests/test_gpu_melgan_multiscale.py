"""GPU: MelganMultiScalesDiscriminator and its Kaiser-sinc multi-rate downsampling (csrc/multirate.hip, eben_resample) against
float64 restatements.

Resampling tolerance: every output is an fp32 sum of `taps` products of fp32 operands (the table is the same fp32 table in both
computations, so only the accumulation rounds), hence |got - ref| <= gamma_taps * sum_j |k_j| |x_j| with
gamma_n = n u / (1 - n u), u = 2^-24 -- checked element-wise against the float64 sum of absolute products.  The adjoint is the
same bound with the number of products per input sample.  Module embeddings use the existing MelGAN tests' 5e-5 relative bar;
gradients the relative-L2 bar of test_gpu_models (2 x the reference's fp32-vs-fp64 floor + 1e-3).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import eben_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U = 2.0 ** -24


def table(orig_freq, new_freq):
    from vibravox_amd.augment import sinc_resample_kernel

    return sinc_resample_kernel(orig_freq, new_freq, resampling_method="sinc_interp_kaiser")


def ref_resample(x64, k, width, orig, new):
    """torchaudio _apply_sinc_resample_kernel in float64: F.pad + conv1d(stride orig) + interleave + crop."""
    lead, t = x64.shape[:-1], x64.shape[-1]
    w = x64.reshape(-1, t)
    y = F.conv1d(F.pad(w, (width, width + orig))[:, None], k.double()[:, None, :], stride=orig)
    y = y.transpose(1, 2).reshape(w.shape[0], -1)[..., : int(math.ceil(new * t / orig))]
    return y.reshape(*lead, -1)


def gamma(n):
    return n * U / (1 - n * U)


def check_bound(got, ref, bound, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    excess = float(((got - ref).abs() - bound).max()) if got.numel() else -1.0
    assert excess <= 1e-30, (what, excess, float((got - ref).abs().max()))


def lengths_for(orig, width):
    return sorted({n for n in (1, 2, 3, width, width + 1, 2 * orig * width - 1, 2 * orig * width + 1) if n >= 1})


FUSED = [(16000, s) for s in (1, 2, 3, 4)] + [(24000, s) for s in (1, 2, 3, 4)]


@pytest.mark.parametrize("sr,scales", FUSED + [(22050, 3)])
def test_forward_against_float64(hip, sr, scales):
    from vibravox_amd import ops

    g = torch.Generator().manual_seed(sr + scales)
    _, w_last, o_last, _ = table(sr, sr // 2 ** (scales - 1)) if scales > 1 else (None, 0, 1, 1)
    shapes = [(4, 1, 15679), (32, 1, 31968)] + [(2, 1, n) for n in lengths_for(o_last, w_last)]
    for shape in shapes:
        x = torch.randn(shape, generator=g)
        outs = ops.multirate_downsample(x.to(DEV), sr, scales)
        assert len(outs) == scales
        assert torch.equal(outs[0].cpu(), x)
        for s in range(1, scales):
            k, width, orig, new = table(sr, sr // 2 ** s)
            ref = ref_resample(x.double(), k, width, orig, new)
            bound = gamma(2 * width + orig) * ref_resample(x.double().abs(), k.abs(), width, orig, new)
            check_bound(outs[s], ref, bound, (shape, s))


def test_identity_scale_is_the_input(hip):
    from vibravox_amd import ops

    x = torch.randn(2, 1, 3000, device=DEV)
    outs = ops.multirate_downsample(x, 16000, 3)
    assert outs[0].data_ptr() == x.data_ptr() and outs[0].shape == x.shape
    assert ops.kaiser_resample(x, 16000, 16000) is x
    assert ops.multirate_downsample(x, 22050, 3)[0] is x


def _adjoint(x_shape, sr, scales, gs):
    """d_audio of ops.multirate_downsample for output gradients gs (gs[0] is the identity scale's)."""
    from vibravox_amd import ops

    x = torch.zeros(x_shape, device=DEV, requires_grad=True)
    outs = ops.multirate_downsample(x, sr, scales)
    (dx,) = torch.autograd.grad(outs, x, grad_outputs=gs)
    return dx


@pytest.mark.parametrize("sr,scales,t", [(16000, 3, 15679), (24000, 4, 4097), (16000, 2, 27), (22050, 3, 15679), (22050, 3, 11076)])
def test_adjoint_identities(hip, sr, scales, t):
    from vibravox_amd import ops

    g = torch.Generator().manual_seed(t)
    x = torch.randn(3, 1, t, generator=g)
    outs = [o.detach().cpu() for o in ops.multirate_downsample(x.to(DEV), sr, scales)]
    ys = [torch.randn(o.shape, generator=g) for o in outs]
    zeros = [torch.zeros_like(y, device=DEV) for y in ys]
    separate = []
    for s in range(1, scales):
        k, width, orig, new = table(sr, sr // 2 ** s)
        gs = list(zeros)
        gs[s] = ys[s].to(DEV)
        dx = _adjoint(x.shape, sr, scales, gs).cpu()
        # <A x, y> = <x, A^T y> in float64
        lhs, rhs = float((outs[s].double() * ys[s].double()).sum()), float((x.double() * dx.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * float(outs[s].double().norm() * ys[s].double().norm()), (s, lhs, rhs)   # Cauchy-Schwarz scale
        # the adjoint against float64 autograd through the restatement (= the transposed conv)
        x64 = x.double().requires_grad_(True)
        (ref,) = torch.autograd.grad(ref_resample(x64, k, width, orig, new), x64, ys[s].double())
        xa = x.double().abs().requires_grad_(True)
        (absum,) = torch.autograd.grad(ref_resample(xa, k.abs(), width, orig, new), xa, ys[s].double().abs())
        per_sample = -(-(2 * width + orig) // orig) * new
        check_bound(dx, ref, gamma(per_sample) * absum, ("adjoint", s))
        separate.append(ops.resample_adjoint(ys[s].to(DEV), sr, sr // 2 ** s, t))
    # fused d_audio = g_0 + sum of the separate adjoints, and it is reproducible bit for bit
    gs = [y.to(DEV) for y in ys]
    d1, d2 = _adjoint(x.shape, sr, scales, gs), _adjoint(x.shape, sr, scales, gs)
    assert torch.equal(d1, d2)
    want = gs[0].clone()
    for d in separate:
        want = want + d
    assert float((d1 - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_general_adjoint_accumulates(hip):
    from vibravox_amd import ops

    g = torch.randn(5, 1, 3920, device=DEV)
    base = torch.randn(5, 1, 15679, device=DEV)
    acc = base.clone()
    ops.resample_adjoint(g, 22050, 5512, 15679, accumulate_into=acc)
    fresh = ops.resample_adjoint(g, 22050, 5512, 15679)
    assert float((acc - (base + fresh)).abs().max()) <= 1e-6 * float(acc.abs().max())


def _module_and_state(sr, scales, seed=0):
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import MelganMultiScalesDiscriminator

    torch.manual_seed(seed)
    disc = MelganMultiScalesDiscriminator(sr, scales=scales)
    sd = {k: v.detach().clone().double() for k, v in disc.state_dict().items()}
    return disc.to(DEV), sd


def _oracle_embeddings(sd, audio64, sr, scales):
    out = []
    for s in range(scales):
        if s == 0:
            sig = audio64
        else:
            k, width, orig, new = table(sr, sr // 2 ** s)
            sig = ref_resample(audio64, k, width, orig, new)
        out.append(O.melgan_disc_forward(sd, f"discriminators.{s}", sig))
    return out


def rel_max(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


@pytest.mark.parametrize("sr,scales,t", [(16000, 3, 15679), (22050, 3, 6007)])
def test_module_embeddings_and_gradients_against_float64(hip, golden, sr, scales, t):
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales

    disc, sd = _module_and_state(sr, scales)
    g = torch.Generator().manual_seed(7)
    audio, audio_b = 0.5 * torch.randn(2, 1, t, generator=g), 0.5 * torch.randn(2, 1, t, generator=g)
    ad = audio.to(DEV).requires_grad_(True)
    e_a = disc(ad)
    with torch.no_grad():
        e_b = disc(audio_b.to(DEV))
    assert [len(e) for e in e_a] == [8] * scales
    osd = {k: v.requires_grad_(True) for k, v in sd.items()}
    oa = audio.double().requires_grad_(True)
    o_a = _oracle_embeddings(osd, oa, sr, scales)
    with torch.no_grad():
        o_b = _oracle_embeddings(osd, audio_b.double(), sr, scales)
    for s in range(scales):
        for i, (x, r) in enumerate(zip(e_a[s], o_a[s])):
            assert rel_max(x, r) <= 5e-5, (s, i, rel_max(x, r))
    fm, hinge = FeatureLossForDiscriminatorMelganMultiScales(), HingeLossForDiscriminatorMelganMultiScales()
    (fm(e_a, e_b) + 0.5 * hinge(embeddings=e_a, target=1) + 0.25 * hinge(embeddings=e_a, target=-1)).backward()
    (O.feature_loss(o_a, o_b) + 0.5 * O.hinge_loss(o_a, 1) + 0.25 * O.hinge_loss(o_a, -1)).backward()
    floor = float(golden["check:disc_grad_fp64_floor"])
    worst = rel_l2(ad.grad, oa.grad)
    for k, prm in disc.named_parameters():
        worst = max(worst, rel_l2(prm.grad, osd[k].grad))
    assert worst <= 2 * floor + 1e-3, (worst, floor)


def test_reference_test_bodies(hip):
    """melgan_discriminator_test.py, feature_loss_test.py and hinge_loss_test.py of the reference, on the real class."""
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import MelganMultiScalesDiscriminator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales

    torch.manual_seed(0)
    sample = torch.randn(4, 1, 15679).to(DEV)
    disc = MelganMultiScalesDiscriminator(sample_rate=16000).to(DEV)
    scales_embeddings = disc(sample)
    assert isinstance(scales_embeddings, list)
    assert len(scales_embeddings) == len(disc.discriminators)
    assert all(isinstance(x[-1], torch.Tensor) for x in scales_embeddings)
    assert sum(p.numel() for p in disc.parameters()) > 1e3
    loss = FeatureLossForDiscriminatorMelganMultiScales()(disc(sample), disc(sample))
    assert loss.shape == torch.Size([])
    hinge = HingeLossForDiscriminatorMelganMultiScales()
    for target in (-1, 1):
        assert hinge(disc(sample), target=target).shape == torch.Size([])
    versions = disc.get_downsampled_versions(sample)
    assert [tuple(v.shape) for v in versions] == [(4, 1, 15679), (4, 1, 7840), (4, 1, 3920)]


def test_one_scale_is_a_plain_melgan_discriminator(hip):
    from vibravox_amd.torch_modules.dnn.melgan_discriminator import DiscriminatorMelGAN, MelganMultiScalesDiscriminator

    torch.manual_seed(5)
    ms = MelganMultiScalesDiscriminator(16000, scales=1).to(DEV)
    torch.manual_seed(5)
    one = DiscriminatorMelGAN(0.2).to(DEV)
    x = torch.randn(2, 1, 4001, device=DEV)
    a, b = ms(x), one(x)
    assert len(a) == 1 and len(a[0]) == len(b)
    for u, v in zip(a[0], b):
        assert torch.equal(u, v)
