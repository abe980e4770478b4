"""``EBENLightningModule``'s two autograd train steps -- the step without the redundant discriminator passes
(``exploit_step_redundancy``) and the literal as-executed order -- against each other on CPU stand-ins: a six-layer toy generator
with the attributes the step uses (``pqmf.forward(x, mode)``, ``cut_to_valid_length``, ``last_conv``), a two-chain toy discriminator
that returns lists of embeddings, plain-torch feature-matching and hinge losses, ``torch.optim.Adam``, clips of 2 x 1 x 130.

Both steps compute the same mathematics in a different order of passes, so per step they must log the same names (none of
``train/discriminator/*`` where the ``torch.rand(1)`` draw skips the update), the same values and the same lambdas, and leave the same
parameters up to the order of the fp32 sums.
"""
import copy
from functools import partial

import pytest
import torch

from vibravox_amd.lightning_modules.eben import EBENLightningModule

STEPS = 3
#: max-abs difference of any parameter between the two paths after STEPS steps.  Measured over the nine cases below: 1.49e-8 (the
#: paths accumulate the same gradients in a different order; Adam turns a last-bit difference of a gradient into a last-bit
#: difference of the update).  The bound is that figure times 4, which allows for convolution sums that depend on the thread count.
PARAM_BOUND = 4 * 1.49e-8


class _ToyPQMF(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.register_buffer("analysis", torch.randn(4, 1, 5, generator=g) * 0.3)
        self.register_buffer("synthesis", torch.randn(1, 4, 5, generator=g) * 0.3)

    def forward(self, x, mode):
        return torch.nn.functional.conv1d(x, self.analysis if mode == "analysis" else self.synthesis, padding=2)


class _ToyGenerator(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.pqmf = _ToyPQMF()
        self.body = torch.nn.ModuleList([torch.nn.Conv1d(1 if i == 0 else 8, 8, 3, padding=1) for i in range(5)])
        self.last_conv = torch.nn.Conv1d(8, 4, 3, padding=1, bias=False)

    def cut_to_valid_length(self, x):
        return x[..., :x.shape[-1] - x.shape[-1] % 4]

    def forward(self, x):
        for conv in self.body:
            x = torch.nn.functional.leaky_relu(conv(x), 0.2)
        bands = torch.tanh(self.last_conv(x))
        return self.pqmf.forward(bands, "synthesis"), bands


class _ToyDiscriminator(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.chains = torch.nn.ModuleList([
            torch.nn.ModuleList([torch.nn.Conv1d(c, 6, 5, padding=2), torch.nn.Conv1d(6, 6, 5, stride=2, padding=2), torch.nn.Conv1d(6, 1, 3, padding=1)])
            for c in (4, 1)])

    def forward(self, bands, audio):
        out = []
        for chain, x in zip(self.chains, (bands, audio)):
            embeddings = []
            for i, conv in enumerate(chain):
                x = conv(x) if i == len(chain) - 1 else torch.nn.functional.leaky_relu(conv(x), 0.2)
                embeddings.append(x)
            out.append(embeddings)
        return out


class _FeatureLoss(torch.nn.Module):
    def forward(self, enhanced, reference):
        pairs = [(a, b.detach()) for ea, eb in zip(enhanced, reference) for a, b in zip(ea[:-1], eb[:-1])]
        return sum((a - b).abs().mean() / b.abs().mean() for a, b in pairs) / len(pairs)


class _HingeLoss(torch.nn.Module):
    def forward(self, embeddings, target):
        return sum(torch.relu(1 - target * chain[-1]).mean() for chain in embeddings) / len(embeddings)


def _module(balancing, ratio, redundancy):
    torch.manual_seed(5)
    gen, disc = _ToyGenerator(), _ToyDiscriminator()
    opt = partial(torch.optim.Adam, lr=3e-4, betas=(0.5, 0.9))
    mod = EBENLightningModule(
        sample_rate=16000, generator=gen, discriminator=disc, generator_optimizer=opt, discriminator_optimizer=opt,
        reconstructive_loss_freq_fn=None, reconstructive_loss_time_fn=torch.nn.L1Loss(), feature_matching_loss_fn=_FeatureLoss(),
        adversarial_loss_fn=_HingeLoss(), dynamic_loss_balancing=balancing, beta_ema=0.9, update_discriminator_ratio=ratio)
    mod.exploit_step_redundancy = redundancy
    return mod


def _run(mod, batches):
    torch.manual_seed(87)   # the torch.rand(1) draws of the discriminator phase: 0.5 passes at steps 0 and 2 and skips step 1
    steps = []
    for bc, air in batches:
        mod.logged.clear()
        out = mod.training_step({"audio_body_conducted": bc, "audio_airborne": air})
        assert out["enhanced"].shape == out["reference"].shape == out["corrupted"].shape == (2, 1, 128)
        lambdas = None if mod.last_lambdas is None else [float(t) for t in mod.last_lambdas]
        steps.append(({k: float(v) for k, v in mod.logged.items()}, lambdas))
    return steps


@pytest.mark.parametrize("ratio", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("balancing", [None, "simple", "ema"])
def test_fused_and_literal_paths_agree(balancing, ratio):
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(2, 1, 130, generator=g), torch.randn(2, 1, 130, generator=g)) for _ in range(STEPS)]
    fused, literal = _module(balancing, ratio, True), _module(balancing, ratio, False)
    for a, b in zip(fused.parameters(), literal.parameters()):
        assert torch.equal(a, b)
    got, want = _run(fused, batches), _run(literal, copy.deepcopy(batches))
    updates = []
    for i, ((logs_f, lam_f), (logs_l, lam_l)) in enumerate(zip(got, want)):
        assert logs_f.keys() == logs_l.keys(), (i, sorted(logs_f), sorted(logs_l))
        assert {"train/generator/reconstructive_loss_temp", "train/generator/feature_matching_loss", "train/generator/adv_loss_gen",
                "train/generator/backprop_loss"} <= logs_f.keys()
        discriminator_keys = {k for k in logs_f if k.startswith("train/discriminator/")}
        assert discriminator_keys in (set(), {f"train/discriminator/{k}" for k in ("real_loss", "fake_loss", "backprop_loss")})
        updates.append(bool(discriminator_keys))
        for k in logs_f:
            assert logs_f[k] == pytest.approx(logs_l[k], rel=1e-6), (i, k)
        assert (lam_f is None) == (lam_l is None) == (balancing is None)
        if lam_f is not None:
            assert lam_f == pytest.approx(lam_l, rel=1e-6), i
    assert updates == {1.0: [True, True, True], 0.5: [True, False, True], 0.0: [False, False, False]}[ratio]
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(fused.parameters(), literal.parameters()))
    print(f"balancing {balancing} ratio {ratio}: parameters differ by {worst:.3e} max-abs")
    assert worst <= PARAM_BOUND, worst
