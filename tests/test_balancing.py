"""Dynamic loss balancing (``vibravox/lightning_modules/eben.py:222-240``) as ``EBENLightningModule`` exposes it: ``balance_losses``
over the module's ``dynamic_loss_balancing`` / ``beta_ema`` as they are at the call, the state readable and assignable as
``atomic_norms_old``, the last call's figures as ``last_norms`` / ``last_lambdas``.  CPU: the one-element torch arithmetic.

The goldens were recorded from the reference module itself (tests/golden/make_golden.py, make_variants_golden.py): its norms, cast to
fp32 and fed through the torch route step after step, must give its lambdas EXACTLY -- the formula is a handful of fp32 operations in
a fixed order, and the recorded lambdas are those operations' results.
"""
import os

import numpy as np
import pytest
import torch

from make_variants_golden import VARIANTS
from tests.test_step_paths import _module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCED = {name: (cfg.get("balancing", "ema"), steps) for name, (cfg, steps) in VARIANTS.items() if cfg.get("balancing", "ema") is not None}


def _reference_lambdas(old):
    return [torch.clamp(1 / (o + 1e-4), min=0.0, max=1e4) for o in old]


def _replay(mod, fixture, prefixes):
    for prefix in prefixes:
        norms = list(torch.from_numpy(fixture[f"{prefix}/balancing/norms"]).to(torch.float32))
        losses = [torch.ones(()) for _ in norms]
        lambdas, backprop, seed = mod.balance_losses(norms, losses)
        want = torch.from_numpy(fixture[f"{prefix}/balancing/lambdas"]).to(torch.float32)
        assert torch.equal(torch.stack(mod.last_lambdas), want), (prefix, torch.stack(mod.last_lambdas), want)
        assert torch.equal(torch.stack(lambdas), want) and seed is None
        assert torch.equal(torch.stack(mod.last_norms), torch.stack(norms))
        assert torch.equal(backprop, sum(w * 1.0 for w in want))


def test_the_variant_fixture_has_thirteen_balanced_steps():
    assert sum(steps for _, steps in BALANCED.values()) == 13


@pytest.mark.parametrize("name", list(BALANCED))
def test_golden_norms_give_the_golden_lambdas_in_every_balanced_variant(name):
    mode, steps = BALANCED[name]
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "eben_variants_golden.npz"))
    _replay(_module(mode, 1.0, True), fixture, [f"var/{name}/step{i}" for i in range(steps)])


def test_golden_norms_give_the_golden_lambdas_in_the_default_configuration(golden):
    _replay(_module("ema", 1.0, True), golden, ["step0", "step1"])


def test_assigned_state_and_changed_mode_take_effect_at_the_next_call():
    beta = 0.9
    mod = _module("ema", 1.0, True)
    assert mod.atomic_norms_old is None and mod.last_lambdas is None and mod.last_norms is None
    losses = [torch.tensor(0.5), torch.tensor(2.0), torch.tensor(-3.0)]
    n0 = [torch.tensor(v) for v in (0.25, 3.0, 40.0)]
    lam0, _, _ = mod.balance_losses(n0, losses)
    # first call: the state is the norms, and the EMA is applied to it anyway
    state = [beta * n + (1 - beta) * n for n in n0]
    assert torch.equal(torch.stack(mod.atomic_norms_old), torch.stack(state))
    assert torch.equal(torch.stack(lam0), torch.stack(_reference_lambdas(state)))
    # the one door: what is assigned is what the next call continues from
    assigned = [torch.tensor(v) for v in (7.0, 0.125, 1e-5)]
    mod.atomic_norms_old = [t.clone() for t in assigned]
    n1 = [torch.tensor(v) for v in (0.5, 2.0, 3e-5)]
    lam1, backprop, _ = mod.balance_losses(n1, losses)
    state = [beta * o + (1 - beta) * n for o, n in zip(assigned, n1)]
    want = _reference_lambdas(state)
    assert torch.equal(torch.stack(lam1), torch.stack(want)) and torch.equal(torch.stack(mod.last_lambdas), torch.stack(want))
    assert torch.equal(torch.stack(mod.atomic_norms_old), torch.stack(state))
    assert torch.equal(backprop, sum(loss * lam for loss, lam in zip(losses, want)))
    assert float(want[2]) < 1e4 and float(_reference_lambdas([torch.tensor(0.0)])[0]) == 1e4   # both sides of the clamp exist
    assert torch.equal(torch.stack(lam0), torch.stack(_reference_lambdas([beta * n + (1 - beta) * n for n in n0])))   # earlier lambdas keep their values
    # beta_ema is read at the call
    mod.beta_ema = 0.5
    lam2, _, _ = mod.balance_losses(n0, losses)
    state = [0.5 * o + (1 - 0.5) * n for o, n in zip(state, n0)]
    assert torch.equal(torch.stack(lam2), torch.stack(_reference_lambdas(state)))
    # "simple": the current norms alone
    mod.dynamic_loss_balancing = "simple"
    lam3, _, _ = mod.balance_losses(n1, losses)
    assert torch.equal(torch.stack(lam3), torch.stack(_reference_lambdas(n1)))
    assert torch.equal(torch.stack(mod.atomic_norms_old), torch.stack(n1))
    # None: the plain sum, unit lambdas, nothing recorded
    mod.dynamic_loss_balancing = None
    seeds = [torch.full((2, 3), float(i + 1)) for i in range(3)]
    lam4, backprop, seed = mod.balance_losses(None, losses, seeds)
    assert lam4 == [1.0, 1.0, 1.0] and torch.equal(backprop, sum(losses)) and torch.equal(seed, torch.full((2, 3), 6.0))
    assert torch.equal(torch.stack(mod.last_lambdas), torch.stack(lam3)) and torch.equal(torch.stack(mod.atomic_norms_old), torch.stack(n1))
    # and back: "ema" continues from the state "simple" left
    mod.dynamic_loss_balancing = "ema"
    lam5, _, seed = mod.balance_losses(n0, losses, seeds)
    state = [0.5 * o + (1 - 0.5) * n for o, n in zip(n1, n0)]
    assert torch.equal(torch.stack(lam5), torch.stack(_reference_lambdas(state)))
    want_seed = None
    for s, lam in zip(seeds, lam5):
        want_seed = s * lam if want_seed is None else want_seed + s * lam
    assert torch.equal(seed, want_seed)
