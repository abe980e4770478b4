"""GPU: the drop-in modules and the full GAN train step (all through libeben_hip.so) against the
CPU oracle and the golden fixtures frozen from the reference.

Gradient comparisons use the relative L2 norm per tensor: the graph is discontinuous (LeakyReLU
masks, sign(a-b) of the L1 feature loss) and fp32 rounding noise flips isolated elements -- the
reference's own fp32 and fp64 gradients differ by `check:disc_grad_fp64_floor` (~1e-2) in that
metric on the discriminator, which is the bar used here.
"""
from functools import partial

import numpy as np
import pytest
import torch

from formula import formula_audio, formula_state_dict, iter_embeddings, summarize
from oracle import eben_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def max_abs(got, ref):
    return float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max())


def contract(golden, tag):
    return {k: tuple(int(x) for x in s.split(",")) for k, s in zip(golden[f"contract/{tag}/keys"], golden[f"contract/{tag}/shapes"])}


def build_generator(golden, p):
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    gen = EBENGenerator(m=4, n=32, p=p)
    shapes = contract(golden, "G")
    shapes["first_conv.weight"] = (32, p, 3)
    assert list(gen.state_dict().keys()) == list(contract(golden, "G").keys())
    sd = formula_state_dict(shapes, f"G{p}")
    missing, unexpected = gen.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pqmf.") for k in missing)
    np.testing.assert_array_equal(gen.pqmf.analysis_weights.numpy(), golden["pqmf/analysis_4_32"])
    osd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    return gen.to(DEV), osd


def build_discriminator(golden):
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales

    disc = DiscriminatorEBENMultiScales(q=4, min_channels=24)
    shapes = contract(golden, "D")
    assert {k: tuple(v.shape) for k, v in disc.state_dict().items()} == shapes
    sd = formula_state_dict(shapes, "D")
    disc.load_state_dict(sd, strict=True)
    return disc.to(DEV), {k: v.clone() for k, v in sd.items()}


def check_summary(golden, prefix, t, rtol=5e-5, atol=5e-6):
    s = summarize(t.detach().cpu())
    assert tuple(golden[f"{prefix}:shape"]) == tuple(s["shape"])
    np.testing.assert_allclose(s["probe"], golden[f"{prefix}:probe"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(s["l2"], golden[f"{prefix}:l2"], rtol=rtol)


@pytest.mark.parametrize("p", [2, 1])
def test_generator_matches_oracle_and_reference_golden(hip, golden, p):
    gen, osd = build_generator(golden, p)
    x = O.cut_to_valid_length(formula_audio("g_in", 2, 8192))
    enh, bands = gen(x.to(DEV))
    assert enh.shape == x.shape  # the reference's own test (tests/torch_modules/eben_generator_test.py:2-8)
    check_summary(golden, f"gen{p}/enhanced", enh)
    check_summary(golden, f"gen{p}/bands", bands)
    osd = {k: v.requires_grad_(not k.startswith("pqmf.")) for k, v in osd.items()}
    o_enh, o_bands = O.generator_forward(osd, x, p)
    assert max_abs(enh, o_enh) < 2e-5 and max_abs(bands, o_bands) < 2e-5
    mse = float(((enh.detach().cpu().double() - o_enh.detach().double()) ** 2).mean())
    assert mse < 1e-10  # north_star bar is 1e-5; fp32 floor ~5e-15
    wgt = formula_audio("g_seed", 2, enh.shape[2], amp=1.0)
    ((enh * wgt.to(DEV)).sum() + (bands ** 2).sum()).backward()
    ((o_enh * wgt).sum() + (o_bands ** 2).sum()).backward()
    worst = 0.0
    for k, prm in gen.named_parameters():
        if prm.grad is None:
            continue
        worst = max(worst, rel_l2(prm.grad, osd[k].grad))
        np.testing.assert_allclose(prm.grad.double().norm().item(), golden[f"gen{p}/grad_l2/{k}"], rtol=2e-3)
    assert worst < 2e-3, worst


# test_generator_forward_in_the_shipped_bf16x3_arithmetic: the x3 forward's measured distance from the float64 oracle ([MI355X], see the
# docstring); the test holds 4 x these
X3_MEASURED = {"enhanced": (2.631e-07, 1.954e-15), "bands": (1.137e-07, 4.829e-16)}   # output -> (max_abs, mse)


def test_generator_forward_in_the_shipped_bf16x3_arithmetic(hip, golden):
    """The generator forward as the bf16-mixed train step runs it -- inside gen_engine.forward_math("bf16x3"): hi + lo bf16 operands,
    three piece products in every conv and ResidualUnit -- against the oracle in float64, next to the default six-product forward.
    [MI355X] batch 2 x 8160, max |got - oracle| / mean squared error:
      default (bf16x6)  enhanced 4.458e-08 / 3.839e-17   bands 2.650e-08 / 5.220e-18
      bf16x3            enhanced 2.631e-07 / 1.954e-15   bands 1.137e-07 / 4.829e-16   (6 x / 51 x and 4 x / 93 x the default's)
    The bar on the x3 forward is 4 x its measured distance (input-dependent rounding over 30-odd chained layers): ~1e-6, four orders
    of magnitude under the 2e-2 .. 5e-2 of the whole-step tests that were its only check; and mse < 1e-8, the figure VERDICT.md quotes for
    the bf16 plan's generator output against the north-star bar of 1e-5."""
    from vibravox_amd import gen_engine, ops

    gen, osd = build_generator(golden, 2)
    x = O.cut_to_valid_length(formula_audio("g_in", 2, 8192))
    with torch.no_grad():
        o_enh, o_bands = O.generator_forward({k: v.double() for k, v in osd.items()}, x.double(), 2)
        assert o_enh.dtype == torch.float64 and o_bands.dtype == torch.float64
        before = (gen_engine.conv_forward_math(), gen_engine.ru_forward_math())
        assert before == (ops.MATH_BF16X6, ops.MATH_BF16X6)
        enh6, bands6 = gen(x.to(DEV))
        with gen_engine.forward_math("bf16x3"):
            assert gen_engine.conv_forward_math() == ops.MATH_BF16X3 and gen_engine.ru_forward_math() == ops.MATH_BF16X3
            enh3, bands3 = gen(x.to(DEV))
            torch.cuda.synchronize()
        assert (gen_engine.conv_forward_math(), gen_engine.ru_forward_math()) == before

    def figures(got, ref):
        return max_abs(got, ref), float(((got.detach().cpu().double() - ref) ** 2).mean())

    got = {"x6": {"enhanced": figures(enh6, o_enh), "bands": figures(bands6, o_bands)},
           "x3": {"enhanced": figures(enh3, o_enh), "bands": figures(bands3, o_bands)}}
    for m, outs in got.items():
        for k, (ma, mse) in outs.items():
            print(f"[gen {m}] {k}: max_abs {ma:.3e} mse {mse:.3e}")
    assert not torch.equal(enh3, enh6)   # the block did change the arithmetic
    for k, (ma, mse) in got["x3"].items():
        assert ma < 4 * X3_MEASURED[k][0] and mse < 4 * X3_MEASURED[k][1], (k, ma, mse)
        assert mse < 1e-8, (k, mse)
        assert got["x6"][k][0] < 2e-5 and got["x6"][k][1] < 1e-10, (k, got["x6"][k])   # the default forward's own bars


def test_generator_config1_forward(hip, golden):
    """BASELINE config 1: generator-only forward, batch 4 x 16000 -> 15840."""
    gen, _ = build_generator(golden, 2)
    x = gen.cut_to_valid_length(formula_audio("cfg1", 4, 16000))
    assert x.shape[2] == 15840
    with torch.no_grad():
        enh, bands = gen(x.to(DEV))
    check_summary(golden, "cfg1/enhanced", enh)
    check_summary(golden, "cfg1/bands", bands)


def test_discriminator_losses_grads(hip, golden):
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales

    disc, osd = build_discriminator(golden)
    bands = formula_audio("d_bands", 8, 2016, amp=0.5).reshape(2, 4, 2016)
    audio = formula_audio("d_audio", 2, 4 * 2016 - 32)
    bands_b = formula_audio("d_bands_b", 8, 2016, amp=0.5).reshape(2, 4, 2016)
    audio_b = formula_audio("d_audio_b", 2, 4 * 2016 - 32)
    bd, ad = bands.to(DEV).requires_grad_(True), audio.to(DEV).requires_grad_(True)
    e_a = disc(bands=bd, audio=ad)
    with torch.no_grad():
        e_b = disc(bands=bands_b.to(DEV), audio=audio_b.to(DEV))
    assert [len(s) for s in e_a] == [9, 9, 9, 8]
    for name, t in iter_embeddings(e_a):
        check_summary(golden, f"disc/{name}", t)
    fm, hinge = FeatureLossForDiscriminatorMelganMultiScales(), HingeLossForDiscriminatorMelganMultiScales()
    l_fm, l_hp, l_hm = fm(e_a, e_b), hinge(embeddings=e_a, target=1), hinge(embeddings=e_a, target=-1)
    np.testing.assert_allclose(l_fm.item(), golden["loss/fm"], rtol=2e-5)
    np.testing.assert_allclose(l_hp.item(), golden["loss/hinge_p1"], rtol=1e-5)
    np.testing.assert_allclose(l_hm.item(), golden["loss/hinge_m1"], rtol=1e-5)
    (l_fm + 0.5 * l_hp + 0.25 * l_hm).backward()
    # oracle on the same inputs
    osd = {k: v.requires_grad_(True) for k, v in osd.items()}
    ob, oa = bands.clone().requires_grad_(True), audio.clone().requires_grad_(True)
    o_a = O.discriminator_forward(osd, ob, oa, 4)
    with torch.no_grad():
        o_b = O.discriminator_forward(osd, bands_b, audio_b, 4)
    (O.feature_loss(o_a, o_b) + 0.5 * O.hinge_loss(o_a, 1) + 0.25 * O.hinge_loss(o_a, -1)).backward()
    floor = float(golden["check:disc_grad_fp64_floor"])
    worst = max(rel_l2(bd.grad, ob.grad), rel_l2(ad.grad, oa.grad))
    for k, prm in disc.named_parameters():
        worst = max(worst, rel_l2(prm.grad, osd[k].grad))
        np.testing.assert_allclose(prm.grad.double().norm().item(), golden[f"disc/grad_l2/{k}"], rtol=2e-2)
    assert worst <= 2 * floor + 1e-3, (worst, floor)
    np.testing.assert_allclose(bd.grad.double().norm().item(), golden["disc/grad_bands:l2"], rtol=2e-3)
    np.testing.assert_allclose(ad.grad.double().norm().item(), golden["disc/grad_audio:l2"], rtol=2e-3)


def make_module(golden, use_mrstft, fused_adam=True):
    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    gen, g_sd = build_generator(golden, 2)
    disc, d_sd = build_discriminator(golden)
    opt = partial(FusedAdam if fused_adam else torch.optim.Adam, lr=3e-4, betas=(0.5, 0.9))
    mr = MultiResolutionSTFTLoss(fft_sizes=(512, 1024, 2048), hop_sizes=(50, 120, 240), win_lengths=(240, 600, 1200),
                                 sample_rate=16000, perceptual_weighting=True).to(DEV) if use_mrstft else None
    mod = EBENLightningModule(sample_rate=16000, generator=gen, discriminator=disc, generator_optimizer=opt,
                              discriminator_optimizer=opt, reconstructive_loss_freq_fn=mr,
                              feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales(),
                              adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales(),
                              dynamic_loss_balancing="ema", beta_ema=0.9, update_discriminator_ratio=1)
    return mod, g_sd, d_sd


@pytest.mark.parametrize("fused_adam,literal,engine,disc_math", [(True, False, True, "f32"), (False, False, True, "f32"), (True, False, False, "f32"),
                                                                (True, True, False, "f32"), (True, False, True, "bf16x6")])
def test_two_train_steps_against_reference_replay_golden(hip, golden, fused_adam, literal, engine, disc_math):
    """eben.py:82-130 replayed over the REFERENCE modules (golden) vs this build's LightningModule:
    the literal as-executed order, the order with the redundant discriminator passes removed (autograd),
    and the batched discriminator engine (one forward, one stacked backward) -- the engine also in the "bf16x6" plan
    (discriminator forward / input gradients with three bf16 pieces per operand on the bf16 matrix pipe: fp32-grade
    products, so the SAME tolerances apply)."""
    mod, g_sd, d_sd = make_module(golden, use_mrstft=False, fused_adam=fused_adam)
    mod.exploit_step_redundancy = not literal
    mod.use_disc_engine = engine
    mod.disc_math = disc_math
    for i in range(2):
        batch = {"audio_body_conducted": formula_audio(f"step{i}/bc", 2, 8200).to(DEV),
                 "audio_airborne": formula_audio(f"step{i}/air", 2, 8200).to(DEV)}
        out = mod.training_step(batch)
        assert set(out) == {"corrupted", "enhanced", "reference"}
        check_summary(golden, f"step{i}/enhanced", out["enhanced"], rtol=2e-4, atol=2e-5)
        for k in ("train/generator/feature_matching_loss", "train/generator/adv_loss_gen", "train/generator/backprop_loss",
                  "train/discriminator/real_loss", "train/discriminator/fake_loss", "train/discriminator/backprop_loss"):
            # the lambda-weighted sums inherit the balancing norms' tolerance (lambda = 1 / norm; the norms are gradients through the
            # sign() of the feature-matching loss: any other fp32 rounding of the same arithmetic moves them by ~1e-3 on these clips)
            rtol = 4e-3 if (disc_math != "f32" and "backprop" in k) else 5e-4
            np.testing.assert_allclose(mod.logged[k].item(), golden[f"step{i}/{k}"], rtol=rtol)
        # [MI355X] the split plan's norms sit 2.5e-3 from the reference's on these two formula clips (enhanced ~ reference: the
        # feature-matching gradient is a sum of sign(a - b) terms over nearly equal embeddings), the fp32 MFMA kernels' 1-2e-3
        ntol = 2e-3 if disc_math == "f32" else 4e-3
        np.testing.assert_allclose(torch.stack(mod.last_norms).cpu().numpy(), golden[f"step{i}/balancing/norms"], rtol=ntol)
        np.testing.assert_allclose(torch.stack(mod.last_lambdas).cpu().numpy(), golden[f"step{i}/balancing/lambdas"], rtol=ntol)
    for k, v in mod.generator.state_dict().items():
        if not k.startswith("pqmf."):
            np.testing.assert_allclose(v.double().norm().item(), golden[f"post/G/{k}"][1], rtol=2e-4)
    # Adam's first steps move a weight by ~lr * sign(g): where the fake and real hinge gradients cancel, the sign is decided by
    # the last bits -- [MI355X] the split plan leaves one discriminator tensor 2.7e-4 from the reference's norm (fp32 kernels: < 2e-4)
    dtol = 2e-4 if disc_math == "f32" else 5e-4
    for k, v in mod.discriminator.state_dict().items():
        np.testing.assert_allclose(v.double().norm().item(), golden[f"post/D/{k}"][1], rtol=dtol)


_MSTEP_ORACLE = []


def mstep_oracle(g_sd, d_sd):
    """Two consecutive default-configuration steps of the CPU oracle on the formula clips mstep0 / mstep1 from the golden weights:
    six tests compare against this one trajectory, computed once per session (~10 s of CPU each time otherwise)."""
    if not _MSTEP_ORACLE:
        trainer = O.OracleTrainer(g_sd, d_sd, p=2, q=4, use_mrstft=True)
        for i in range(2):
            bc, air = formula_audio(f"mstep{i}/bc", 2, 8200), formula_audio(f"mstep{i}/air", 2, 8200)
            _MSTEP_ORACLE.append((bc, air, trainer.step(bc, air)))
    return _MSTEP_ORACLE


@pytest.mark.parametrize("literal,engine,split", [(False, True, False), (False, False, False), (True, False, False), (False, True, True)])
def test_train_step_with_mrstft_against_oracle(hip, golden, literal, engine, split):
    """Full default configuration (MRSTFT + FM + hinge, EMA balancing).  The MRSTFT term is a
    restatement of third-party auraloss (parity unpinned); everything else is pinned.  ``split``: the fp32-grade split-bf16 forms
    of the discriminator (plan "bf16x6") and of the windowed-DFT contractions ("folded_x6") at the same tolerances."""
    mod, g_sd, d_sd = make_module(golden, use_mrstft=True)
    mod.exploit_step_redundancy = not literal
    mod.use_disc_engine = engine
    if split:
        mod.disc_math, mod.stft_math = "bf16x6", "folded_x6"
    for i, (bc, air, logs) in enumerate(mstep_oracle(g_sd, d_sd)):
        mod.training_step({"audio_body_conducted": bc.to(DEV), "audio_airborne": air.to(DEV)})
        for k in ("train/generator/reconstructive_loss_freq", "train/generator/feature_matching_loss", "train/generator/adv_loss_gen",
                  "train/generator/backprop_loss", "train/discriminator/real_loss", "train/discriminator/fake_loss"):
            np.testing.assert_allclose(mod.logged[k].item(), logs[k].item(), rtol=1e-3, err_msg=k)
        np.testing.assert_allclose(torch.stack(mod.last_norms).cpu().numpy(), logs["balancing/norms"].numpy(), rtol=5e-3)


@pytest.mark.parametrize("batch,length", [(1, 16000), (1, 4321), (3, 1000)])
def test_generator_inference_variable_length(hip, golden, batch, length):
    """the evaluation path (eben.py:132-165: cut_to_valid_length, generator forward under
    no_grad, any clip length, batch 1) against the oracle on the same weights."""
    gen, osd = build_generator(golden, 2)
    x = formula_audio(f"infer/{batch}/{length}", batch, length)
    with torch.no_grad():
        cut = gen.cut_to_valid_length(x.to(DEV))
        enh, bands = gen(cut)
    o_cut = O.cut_to_valid_length(x)
    assert cut.shape == o_cut.shape and enh.shape == cut.shape
    o_enh, o_bands = O.generator_forward(osd, o_cut, 2)
    assert max_abs(enh, o_enh) < 2e-5 and max_abs(bands, o_bands) < 2e-5
    assert float(((enh.cpu().double() - o_enh.detach().double()) ** 2).mean()) < 1e-10   # north-star bar: MSE < 1e-5


def test_eval_step_logs_reference_losses(hip, golden):
    """eben.py:132-165: validation / test step -- outputs and the logged atomic losses of both networks
    equal the oracle's on the same weights; no gradient state is touched."""
    mod, g_sd, d_sd = make_module(golden, use_mrstft=False)
    bc, air = formula_audio("eval/bc", 2, 8200), formula_audio("eval/air", 2, 8200)
    out = mod.validation_step({"audio_body_conducted": bc.to(DEV), "audio_airborne": air.to(DEV)}, 0)
    assert set(out) == {"corrupted", "enhanced", "reference"} and not out["enhanced"].requires_grad
    assert all(p.grad is None for p in mod.parameters())
    x = O.cut_to_valid_length(bc)
    ref = O.cut_to_valid_length(air)
    o_enh, o_bands = O.generator_forward(g_sd, x, 2)
    assert max_abs(out["enhanced"], o_enh) < 2e-5
    o_ref_bands = O.pqmf_analysis(ref, g_sd["pqmf.analysis_weights"], bands=4)
    e_emb = O.discriminator_forward(d_sd, o_bands, o_enh, 4)
    r_emb = O.discriminator_forward(d_sd, o_ref_bands, ref, 4)
    want = {"validation/generator/feature_matching_loss": O.feature_loss(e_emb, r_emb),
            "validation/generator/adv_loss_gen": O.hinge_loss(e_emb, 1),
            "validation/discriminator/real_loss": O.hinge_loss(r_emb, 1),
            "validation/discriminator/fake_loss": O.hinge_loss(e_emb, -1)}
    for k, v in want.items():
        np.testing.assert_allclose(mod.logged[k].item(), float(v), rtol=5e-4, err_msg=k)
    only_bc = mod.test_step({"audio_body_conducted": bc.to(DEV)}, 0)
    assert set(only_bc) == {"corrupted", "enhanced"}


def test_full_size_step_properties(hip, golden):
    """BASELINE config 2 shape (batch 32 x 32000 -> 31968): size-independent properties only."""
    mod, _, _ = make_module(golden, use_mrstft=True)
    g = torch.Generator().manual_seed(1234)
    batch = {"audio_body_conducted": (0.1 * torch.randn(32, 1, 32000, generator=g)).to(DEV),
             "audio_airborne": (0.1 * torch.randn(32, 1, 32000, generator=g)).to(DEV)}
    before = {k: v.clone() for k, v in mod.discriminator.state_dict().items()}
    out = mod.training_step(batch)
    torch.cuda.synchronize()
    assert out["enhanced"].shape == (32, 1, 31968) and torch.isfinite(out["enhanced"]).all()
    assert out["enhanced"].abs().max() <= 4.0 * 1.05  # tanh-bounded bands through a gain-4 synthesis bank
    for k, v in mod.logged.items():
        assert torch.isfinite(v).all(), k
    lam = torch.stack(mod.last_lambdas)
    assert (lam > 0).all() and (lam <= 1e4).all()
    moved = {k: float((v - before[k]).abs().max()) for k, v in mod.discriminator.state_dict().items()}
    assert max(moved.values()) <= 3e-4 * 1.01  # first Adam step moves every element by <= lr
    # the logit biases see d(real)/db = -1/4 and d(fake)/db = +1/4 while every hinge term is active
    # (near-zero logits at init): exactly zero gradient, so they may stay put; everything else moves
    still = [k for k, m in moved.items() if m == 0.0]
    assert all(k.endswith(".bias") for k in still) and len(still) <= 4, still


# ---- the bf16 step (disc_math = "bf16", BASELINE config 2) against the fp32 step ---------------------------------
# What bf16 MFMA operands cost, measured on MI355X and bounded here (tools/bf16_where.py, tools/bf16_trajectory.py):
#   * the generator never sees the discriminator's arithmetic in its forward: its output is IDENTICAL;
#   * each hinge branch's discriminator gradient (fake_loss alone, real_loss alone) moves by 1e-3 relative L2;
#   * their SUM -- the gradient Adam gets -- is what survives a cancellation of R = (|G_fake| + |G_real|) / |G_fake + G_real|
#     = 240 (config 2, noise inputs, default init) ... 700 (two formula clips): an absolute error of 1e-3 of a branch is
#     R * 1e-3 of the sum.  The error does not come from the gradient contractions (bf16 dX / dW: 7e-3 / 2.4e-2 of the sum at
#     R = 232) but from the FORWARD: bf16 products move pre-activations by ~1e-3, a fraction of them changes sign, and every
#     flipped LeakyReLU mask changes one path of the backward by a factor 5.  The same mechanism separates the reference's own
#     fp32 and fp64 gradients by 8.5e-3 (golden check:disc_grad_fp64_floor); the error goes with sqrt(eps), so neither hi + lo
#     activation operands (EBEN_MATH_BF16X2: measured, no gain) nor anything short of ~2^-18 products would bring it to 1e-2.
#   * the PQMF-band discriminators (9 % of the discriminator's FLOPs) carry most of it (0.25-0.75 per tensor against MelGAN's
#     0.03-0.07): the "bf16" plan therefore runs THEIR forward in exact fp32 (+1.6 ms on a 21.3 ms step) and everything else
#     on bf16 operands -- 3.4e-2 of the summed gradient at config 2, against 0.18 for bf16 everywhere ("bf16_plain").
BF16_STEP_TOLERANCES = {
    # one step from the same state, bf16 step vs fp32 step at BASELINE config 2 (32 x 32000 noise clips, default init)
    "loss": 2e-3,                    # every logged loss but the two below, relative
    "feature_matching_loss": 2e-2,   # a sum of L1 distances between nearly equal embeddings
    "backprop_loss": 2e-2,           # lambda-weighted: inherits the balancing norms
    "balancing_norms": 3e-2,         # |d loss / d last_conv.weight| per loss, relative
    "generator_grad": 2e-2,          # whole-vector relative L2 (bf16 critic + bf16 generator backward)
    "discriminator_grad": 5e-2,      # whole-vector relative L2 of the summed gradient (R = 240)
    "discriminator_branch_grad": 3e-3,   # fake_loss alone / real_loss alone
    "discriminator_grad_vs_branches": 5e-4,   # |dG| / (|G_fake| + |G_real|): the bound that does not depend on R
}


def _one_step(make, disc_math, gen_bwd="f32", seed_weights=None, stft_math="folded"):
    from vibravox_amd.disc_engine import DiscriminatorEngine
    from vibravox_amd.lightning_modules.eben import DISC_MATH_PLANS

    mod, batch = make()
    mod.disc_math, mod.gen_backward_math, mod.stft_math = disc_math, gen_bwd, stft_math
    if seed_weights is not None:
        mod._disc_engine = DiscriminatorEngine(mod.discriminator, DISC_MATH_PLANS[disc_math])
        mod._disc_engine.seed_weights = seed_weights
    out = mod.training_step(batch)
    torch.cuda.synchronize()
    moments = []
    for opt in mod.optimizers():   # Adam's first moment after one step = (1 - beta1) * grad
        moments.append(torch.cat([opt.state[p]["exp_avg"].double().flatten().cpu() for grp in opt.param_groups for p in grp["params"]
                                  if "exp_avg" in opt.state.get(p, {})]))
    return out["enhanced"].clone(), {k: float(v) for k, v in mod.logged.items()}, torch.stack(mod.last_norms).cpu(), moments


def _rel(a, b):
    return float((a - b).norm() / a.norm())


@pytest.mark.parametrize("plan", ["bf16", "bf16_bl"])
def test_bf16_step_against_fp32_step_at_config2(hip, plan):
    """BASELINE config 2 (batch 32 x 32000 samples, default initialisation, noise clips -- bench.py's workload): the bf16 step
    against the fp32 step, every quantity of BF16_STEP_TOLERANCES -- with the engine's tensors at rest in fp32 ("bf16") and in the
    bf16 bundle layout ("bf16_bl", what bench.py times)."""
    import bench

    def make():
        return bench.build_module(DEV, 1234), bench.synthetic_batch(32, 32000, 1234, DEV)

    tol = BF16_STEP_TOLERANCES
    # the bf16 step exactly as bench.py runs it: bf16 plan, bf16 generator backward, MRSTFT contractions on hi + lo bf16 operands
    f32, bf = _one_step(make, "f32"), _one_step(make, plan, "bf16", stft_math="folded_x3")
    # the generator's forward: fp32-grade six-product arithmetic in the fp32 plans, hi + lo operands (three products, 2^-17 each) in the
    # bf16 step -- orders of magnitude inside north_star's 1e-5
    assert float(((f32[0].double() - bf[0].double()) ** 2).mean()) < 1e-8
    for k, v in f32[1].items():
        t = tol["feature_matching_loss"] if "feature_matching" in k else tol["backprop_loss"] if "backprop" in k else tol["loss"]
        assert abs(bf[1][k] - v) <= t * abs(v), (k, v, bf[1][k])
    assert float(((f32[2] - bf[2]).abs() / f32[2].abs()).max()) < tol["balancing_norms"]
    g_rel, d_rel = _rel(f32[3][0], bf[3][0]), _rel(f32[3][1], bf[3][1])
    branches = {}
    for name, w in (("fake", (1.0, 1.0, 0.0)), ("real", (1.0, 0.0, 1.0))):
        a, b = _one_step(make, "f32", seed_weights=w), _one_step(make, plan, seed_weights=w)
        branches[name] = (float(a[3][1].norm()), _rel(a[3][1], b[3][1]))
    vs_branches = float((f32[3][1] - bf[3][1]).norm()) / (branches["fake"][0] + branches["real"][0])
    cancel = (branches["fake"][0] + branches["real"][0]) / float(f32[3][1].norm())
    print(f"{plan} step at config 2: generator grad {g_rel:.3e}, discriminator grad {d_rel:.3e} (R = {cancel:.0f}), branches "
          f"fake {branches['fake'][1]:.3e} real {branches['real'][1]:.3e}, |dG| / (|G_fake| + |G_real|) {vs_branches:.3e}")
    assert g_rel < tol["generator_grad"] and d_rel < tol["discriminator_grad"]
    assert max(branches["fake"][1], branches["real"][1]) < tol["discriminator_branch_grad"]
    assert vs_branches < tol["discriminator_grad_vs_branches"]
    assert cancel > 50   # the regime the bound is stated for: the two hinge branches cancel
    # every contraction on single bf16 operands: the mode this build does NOT headline
    plain = _one_step(make, "bf16_plain", "bf16")
    assert _rel(f32[3][1], plain[3][1]) > 2 * d_rel


@pytest.mark.parametrize("plan", ["bf16", "bf16_bl"])
def test_bf16_step_against_reference_replay_golden(hip, golden, plan):
    """The two-step replay of eben.py:82-130 over the reference modules (golden fixtures, two formula clips of 8200 samples)
    with the bf16 step.  Committed tolerances: logged values as below; the discriminator's update is bounded per hinge branch
    and against the branch magnitudes (R = 670 here: the summed gradient itself moves by ~0.3, see BF16_STEP_TOLERANCES)."""
    table = {"train/generator/feature_matching_loss": 2e-2, "train/generator/adv_loss_gen": 2e-3, "train/generator/backprop_loss": 5e-2,
             "train/discriminator/real_loss": 2e-3, "train/discriminator/fake_loss": 2e-3, "train/discriminator/backprop_loss": 2e-3}
    mod, g_sd, d_sd = make_module(golden, use_mrstft=False)
    mod.disc_math, mod.gen_backward_math = plan, "bf16"
    for i in range(2):
        batch = {"audio_body_conducted": formula_audio(f"step{i}/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio(f"step{i}/air", 2, 8200).to(DEV)}
        out = mod.training_step(batch)
        check_summary(golden, f"step{i}/enhanced", out["enhanced"], rtol=2e-3 if i else 2e-4, atol=2e-4 if i else 2e-5)
        for k, rtol in table.items():
            np.testing.assert_allclose(mod.logged[k].item(), golden[f"step{i}/{k}"], rtol=rtol * (1 if i == 0 else 5), err_msg=f"step {i} {k}")
        np.testing.assert_allclose(torch.stack(mod.last_norms).cpu().numpy(), golden[f"step{i}/balancing/norms"], rtol=5e-2)
        np.testing.assert_allclose(torch.stack(mod.last_lambdas).cpu().numpy(), golden[f"step{i}/balancing/lambdas"], rtol=5e-2)

    def make():
        m, _, _ = make_module(golden, use_mrstft=False)
        return m, {"audio_body_conducted": formula_audio("step0/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio("step0/air", 2, 8200).to(DEV)}

    f32, bf = _one_step(make, "f32"), _one_step(make, plan, "bf16")
    norms = {}
    for name, w in (("fake", (1.0, 1.0, 0.0)), ("real", (1.0, 0.0, 1.0))):
        a, b = _one_step(make, "f32", seed_weights=w), _one_step(make, plan, seed_weights=w)
        norms[name] = float(a[3][1].norm())
        assert _rel(a[3][1], b[3][1]) < BF16_STEP_TOLERANCES["discriminator_branch_grad"], name
    assert float((f32[3][1] - bf[3][1]).norm()) / (norms["fake"] + norms["real"]) < 1e-3
    assert _rel(f32[3][0], bf[3][0]) < 2e-2


@pytest.mark.parametrize("plan", ["bf16", "bf16_bl"])
def test_bf16_training_statistics_against_fp32(hip, plan):
    """Do the two arithmetic modes train the same way?  40 steps from the same state on the same sequence of noise batches
    (4 x 16000), once in fp32, once in fp32 with every input sample perturbed by at most ONE fp32 ulp, once in bf16.
    This GAN's training is chaotic at this scale: the one-ulp run leaves the fp32 run by > 10 % of the discriminator losses
    within 40 steps -- a step-by-step comparison means something only for the first steps, after that only statistics do:
      * steps 0-2: the bf16 run's discriminator losses stay within 1e-2 of the fp32 run's (measured 0, 6e-5, 5e-3);
      * the mean over the 40 steps of the discriminator loss (real + fake): the bf16 run within 4 % of the fp32 run (measured
        1.953 / 1.979 / 1.990 and, one build later, 1.992 / 1.982 / 2.027 for fp32 / one-ulp / bf16); the feature-matching mean, a
        much noisier statistic, within 40 % (0.178 / 0.172 / 0.165, then 0.181 / 0.167 / 0.138)."""
    import bench

    def run(mode, perturb):
        mod = bench.build_module(DEV, 1234)
        mod.disc_math = mode
        mod.gen_backward_math = "f32" if mode == "f32" else "bf16"
        torch.manual_seed(7)
        rows = []
        for i in range(40):
            batch = bench.synthetic_batch(4, 16000, 1000 + i, DEV)
            if perturb:
                g = torch.Generator().manual_seed(5000 + i)
                batch = {k: v * (1 + 2.0 ** -23 * (2 * torch.rand(v.shape, generator=g).to(DEV) - 1)) for k, v in batch.items()}
            mod.training_step(batch)
            rows.append([float(mod.logged[f"train/{k}"]) for k in ("discriminator/real_loss", "discriminator/fake_loss", "generator/feature_matching_loss")])
        return np.array(rows)

    f32, ulp, bf = run("f32", False), run("f32", True), run(plan, False)
    dev = lambda a: np.abs(a[:, :2] - f32[:, :2]).max(axis=1) / np.abs(f32[:, :2]).min(axis=1)
    assert dev(ulp).max() > 0.1, "the chaos yardstick: one ulp on the inputs is amplified to > 10 % within 40 steps"
    assert dev(bf)[:3].max() < 1e-2
    d_mean = lambda a: float((a[:, 0] + a[:, 1]).mean())
    fm_mean = lambda a: float(a[:, 2].mean())
    print(f"mean D loss over 40 steps: fp32 {d_mean(f32):.4f}, fp32 + 1 ulp {d_mean(ulp):.4f}, bf16 {d_mean(bf):.4f}; "
          f"mean FM: {fm_mean(f32):.4f} / {fm_mean(ulp):.4f} / {fm_mean(bf):.4f}")
    # one 40-step trajectory per mode: the means carry the trajectory's own scatter (the one-ulp run's feature-matching mean sits 3-8 %
    # from the fp32 run's, the bf16 run's 7-24 %, from build to build -- any change of summation order re-rolls all three)
    # (the 40-step mean moves with the ORDER of the fp32 sums inside the bf16 kernels: 1.94 .. 2.02 against fp32's 1.93 across five kernel
    # builds of the same arithmetic -- the chaos yardstick above amplifies one ulp to > 10 % of a step's loss)
    assert abs(d_mean(bf) - d_mean(f32)) < max(0.06 * d_mean(f32), 2 * abs(d_mean(ulp) - d_mean(f32)))
    assert abs(fm_mean(bf) - fm_mean(f32)) < 0.4 * fm_mean(f32)


def test_variable_clip_lengths_keep_the_pack_caches_bounded(hip, golden):
    """``collate_strategy: "pad"`` / a short last batch give the step a new (batch, length) every time: the engine's packed
    weight images must not pile up (one fwd + two dX images per layer and shape, re-packed after every optimiser step)."""
    from vibravox_amd.disc_engine import _Layer

    mod, _, _ = make_module(golden, use_mrstft=False)
    seen = []
    for i, (b, t) in enumerate([(2, 4100), (2, 8200), (1, 6000), (2, 5000), (2, 7000), (2, 4100)]):
        mod.training_step({"audio_body_conducted": formula_audio(f"var{i}/bc", b, t).to(DEV), "audio_airborne": formula_audio(f"var{i}/air", b, t).to(DEV)})
        layers = [lay for ch in mod._disc_engine.chains for lay in ch.layers]
        assert max(len(lay.packs) for lay in layers) <= _Layer.MAX_PACKS
        seen.append(float(mod.logged["train/discriminator/real_loss"]))
    torch.cuda.synchronize()
    assert all(np.isfinite(seen)) and max(len(lay.packs) for lay in layers) <= 3   # after prepack: only the last step's shapes


def test_train_step_is_bitwise_reproducible(hip, golden):
    """Every kernel on the path reduces in a fixed order (no float atomics), so two runs from the same
    state must agree bit for bit -- parameters and Adam moments; a difference is a race between the
    streams the step runs on (main, weight-gradient side stream, the discriminator chains)."""
    def run():
        mod, _, _ = make_module(golden, use_mrstft=True)
        g = torch.Generator().manual_seed(99)
        batch = {"audio_body_conducted": (0.1 * torch.randn(8, 1, 16000, generator=g)).to(DEV),
                 "audio_airborne": (0.1 * torch.randn(8, 1, 16000, generator=g)).to(DEV)}
        for _ in range(2):
            mod.training_step(batch)
        torch.cuda.synchronize()
        out = {f"G.{k}": v.clone() for k, v in mod.generator.state_dict().items()}
        out.update({f"D.{k}": v.clone() for k, v in mod.discriminator.state_dict().items()})
        for oi, opt in enumerate(mod.optimizers()):
            for pi, prm in enumerate(p for grp in opt.param_groups for p in grp["params"]):
                if "exp_avg" in opt.state.get(prm, {}):   # the frozen PQMF banks never get a moment
                    out[f"adam{oi}.m.{pi}"] = opt.state[prm]["exp_avg"].clone()
        return out

    a, b = run(), run()
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


def test_bucketed_grad_sync_path_on_gpu_matches_plain_step(hip, golden):
    """The data-parallel plumbing of bench.py (gradients as views of flat buckets, all-reduce issued
    from post-accumulate hooks on a side stream, 1/N folded into Adam) on a single-rank RCCL group:
    must reproduce the plain single-GPU step."""
    import os

    import torch.distributed as dist

    from vibravox_amd.ddp import BucketedZeroGrad, GradSync

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        plain, _, _ = make_module(golden, use_mrstft=False)
        synced, _, _ = make_module(golden, use_mrstft=False)
        g_opt, d_opt = synced.optimizers()
        gs = GradSync(synced.generator.parameters(), bucket_bytes=1 << 20)
        ds = GradSync(synced.discriminator.parameters(), bucket_bytes=8 << 20)
        g_w, d_w = BucketedZeroGrad(g_opt, gs), BucketedZeroGrad(d_opt, ds)
        synced._optimizers = [g_w, d_w]
        synced.grad_sync = {id(g_w): gs, id(d_w): ds}
        for i in range(2):
            batch = {"audio_body_conducted": formula_audio(f"step{i}/bc", 2, 8200).to(DEV),
                     "audio_airborne": formula_audio(f"step{i}/air", 2, 8200).to(DEV)}
            plain.training_step(batch)
            synced.training_step(batch)
        torch.cuda.synchronize()
        assert gs.launched >= 2 * len(gs.buckets) and ds.launched >= 2 * len(ds.buckets)
        for (k, a), (_, b) in zip(plain.generator.state_dict().items(), synced.generator.state_dict().items()):
            assert torch.allclose(a, b, rtol=0, atol=1e-6), k
        for (k, a), (_, b) in zip(plain.discriminator.state_dict().items(), synced.discriminator.state_dict().items()):
            assert torch.allclose(a, b, rtol=0, atol=1e-6), k
        del plain, synced, gs, ds

        # the benchmarked plan (bf16 bundle layout, MRSTFT, every launch sequence replayed as a graph -- on by default next to a process
        # group): the rank of a data-parallel job as bench.py builds it, against the plain step of the same plan, long enough for the
        # sequences to be captured; the gradients land in the bucket views the graphs were captured on
        from vibravox_amd import ops

        def run(with_group):
            mod, _, _ = make_module(golden, use_mrstft=True)
            mod.set_precision("bf16-mixed")
            syncs = None
            if with_group:
                g_opt, d_opt = mod.optimizers()
                syncs = (GradSync(mod.generator.parameters()), GradSync(mod.discriminator.parameters()))
                g_w, d_w = BucketedZeroGrad(g_opt, syncs[0]), BucketedZeroGrad(d_opt, syncs[1])
                mod._optimizers = [g_w, d_w]
                mod.grad_sync = {id(g_w): syncs[0], id(d_w): syncs[1]}
            for i in range(6):
                mod.training_step({"audio_body_conducted": formula_audio(f"ddp/{i}/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio(f"ddp/{i}/air", 2, 8200).to(DEV)})
            torch.cuda.synchronize()
            out = {f"G.{k}": v.clone() for k, v in mod.generator.state_dict().items()}
            out.update({f"D.{k}": v.clone() for k, v in mod.discriminator.state_dict().items()})
            return out, ops.graphs_captured(), syncs

        assert ops.DDP_GRAPHS
        a, _, _ = run(False)
        b, n_graphs, syncs = run(True)
        assert n_graphs >= 22, n_graphs
        assert all(sy.launched >= 6 * len(sy.buckets) for sy in syncs)
        worst = max(float((a[k] - b[k]).abs().max()) for k in a)
        assert worst <= 1e-6, worst
    finally:
        dist.destroy_process_group()


def test_noisy_bwe_chain_collate_augment_step_against_oracle(hip, golden):
    """BASELINE config 4 end to end at oracle size: ragged resident clips -> device collator (noise slice + mix + crop / pad,
    noisybwe.py:219-291) -> WaveformDataAugmentation (time masking, data_augmentation.py:38-71) -> EBEN training_step, against the same
    chain made of the CPU oracles (collate_oracle + augment_oracle + OracleTrainer) under the same torch seed: the assembled batch
    bit for bit, the step's logged losses / balancing norms at the train-step tolerances, for two consecutive steps."""
    from oracle import augment_oracle as A
    from oracle import collate_oracle as C
    from vibravox_amd.augment import WaveformDataAugmentation
    from vibravox_amd.collate import noisy_bwe_collate

    mod, g_sd, d_sd = make_module(golden, use_mrstft=True)
    trainer = O.OracleTrainer(g_sd, d_sd, p=2, q=4, use_mrstft=True)
    kw = dict(p_data_augmentation=1.0, p_speed_perturbation=0.0, p_pitch_shift=0.0, p_time_masking=1.0, time_masking_percentage=(1, 2, 3))
    dev_aug, ora_aug = WaveformDataAugmentation(16000, **kw), A.WaveformDataAugmentation(16000, **kw)
    lengths = [(7000, 9100), (9500, 9600), (8192, 12000), (10100, 10101)]   # speech / noise samples: shorter and longer than the 512 ms target
    strategy = "constant_length-512-ms"                                      # 8192 samples
    for step in range(2):
        items = []
        for i, (ls, ln) in enumerate(lengths):
            items.append({"audio_body_conducted": formula_audio(f"nbwe/{step}/{i}/bc", 1, ls).reshape(-1),
                          "audio_airborne": formula_audio(f"nbwe/{step}/{i}/air", 1, ls).reshape(-1),
                          "audio_body_conducted_speechless_noisy": 0.3 * formula_audio(f"nbwe/{step}/{i}/noise", 1, ln).reshape(-1)})
        torch.manual_seed(100 + step)
        ref = C.noisy_bwe_collate([dict(it) for it in items], 16000, strategy, False)
        rbc, rair = ora_aug(ref["audio_body_conducted"].clone(), ref["audio_airborne"].clone())
        state = float(torch.rand(1))
        torch.manual_seed(100 + step)
        got = noisy_bwe_collate([{k: v.to(DEV) for k, v in it.items()} for it in items], 16000, strategy, False)
        gbc, gair = dev_aug(got["audio_body_conducted"], got["audio_airborne"])
        assert float(torch.rand(1)) == state                                 # same draws consumed
        assert gbc.shape == (4, 1, 8192) and torch.equal(gbc.cpu(), rbc) and torch.equal(gair.cpu(), rair)
        assert float((gbc == 0).float().mean()) > 0.009                      # the time mask is in
        mod.training_step({"audio_body_conducted": gbc, "audio_airborne": gair})
        logs = trainer.step(rbc, rair)
        for k in ("train/generator/reconstructive_loss_freq", "train/generator/feature_matching_loss", "train/generator/adv_loss_gen",
                  "train/generator/backprop_loss", "train/discriminator/real_loss", "train/discriminator/fake_loss"):
            np.testing.assert_allclose(mod.logged[k].item(), logs[k].item(), rtol=1e-3, err_msg=k)
        np.testing.assert_allclose(torch.stack(mod.last_norms).cpu().numpy(), logs["balancing/norms"].numpy(), rtol=5e-3)


def test_noisy_bwe_chain_at_config4_size(hip, golden):
    """The same chain at BASELINE config 4's size (batch 32, constant_length-2500-ms = 40000 samples, bench.py --workload noisybwe):
    size-independent properties -- the collated clips are sums / crops of their sources, the mask zeroes the drawn share, the step's
    outputs and losses are finite and every parameter moved by at most one Adam step."""
    import bench
    from vibravox_amd.augment import WaveformDataAugmentation
    from vibravox_amd.collate import noisy_bwe_collate

    mod, _, _ = make_module(golden, use_mrstft=True)
    pool = bench.noisy_bwe_source(DEV, n_items=32, seed=99)
    aug = WaveformDataAugmentation(16000, p_data_augmentation=1.0, p_speed_perturbation=0.0, p_pitch_shift=0.0, p_time_masking=1.0)
    torch.manual_seed(5)
    batch = noisy_bwe_collate(pool, 16000, "constant_length-2500-ms")
    assert batch["audio_body_conducted"].shape == (32, 1, 40000)
    bc, air = aug(batch["audio_body_conducted"], batch["audio_airborne"])
    energy = float(bc.pow(2).mean())
    assert 0.008 < energy < 0.014     # speech (sigma 0.1) + noise (sigma 0.05): 0.0125 where the clip covers the window, 0 in the padding / mask
    params = [p for p in mod.generator.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    out = mod.training_step({"audio_body_conducted": bc, "audio_airborne": air})
    torch.cuda.synchronize()
    cut = 40000 - (40000 + 32) % 256
    assert out["enhanced"].shape == (32, 1, cut) and torch.isfinite(out["enhanced"]).all()
    for k, v in mod.logged.items():
        assert np.isfinite(float(v)), k
    steps = [float((p.detach() - b).abs().max()) for p, b in zip(params, before)]
    assert max(steps) <= 3e-4 * 1.001 + 1e-7 and sum(st > 0.0 for st in steps) >= len(steps) - 2, sorted(steps)[:4]


def _adam_moments(optimizers):
    """Adam's first moment after ONE step from zero state = (1 - beta1) * gradient: the step's gradients, read back per network."""
    out = []
    for opt in optimizers:
        out.append(torch.cat([opt.state[p]["exp_avg"].detach().double().flatten().cpu() for grp in opt.param_groups for p in grp["params"]
                              if "exp_avg" in opt.state.get(p, {})]))
    return out


def test_full_size_step_against_oracle(hip, golden):
    """BASELINE config 2 at its FULL size (batch 32 x 32000 -> 31968 noise clips, default initialisation: bench.py's workload): one
    train step of eben.py:82-130 through the CPU oracle (pinned to the reference by the golden fixtures; ~5-20 s on the host) against
    the HIP step in three arithmetic plans -- "f32" (exact fp32 products), "bf16x6" (fp32-grade split products) at the fp32 tolerances,
    and the plan bench.py times ("bf16" discriminator plan + bf16 generator backward + "folded_x3" MRSTFT) at BF16_STEP_TOLERANCES.
    Gradients are compared through Adam's first moment after the step (whole-vector relative L2 per network)."""
    import bench

    floor = float(golden["check:disc_grad_fp64_floor"])
    probe = bench.build_module(DEV, 1234)
    g_sd = {k: v.detach().cpu().clone() for k, v in probe.generator.state_dict().items()}
    d_sd = {k: v.detach().cpu().clone() for k, v in probe.discriminator.state_dict().items()}
    del probe
    data = bench.synthetic_batch(32, 32000, 1234, "cpu")
    trainer = O.OracleTrainer(g_sd, d_sd, p=2, q=4, use_mrstft=True)
    logs = trainer.step(data["audio_body_conducted"], data["audio_airborne"])
    want = _adam_moments([trainer.g_opt, trainer.d_opt])
    keys = ("train/generator/reconstructive_loss_freq", "train/generator/feature_matching_loss", "train/generator/adv_loss_gen",
            "train/generator/backprop_loss", "train/discriminator/real_loss", "train/discriminator/fake_loss")
    tol = BF16_STEP_TOLERANCES
    report = {}
    for plan, gen_bwd, stft in (("f32", "f32", "folded"), ("bf16x6", "f32", "folded_x6"), ("bf16", "bf16", "folded_x3"), ("bf16_bl", "bf16", "folded_x3")):
        mod = bench.build_module(DEV, 1234)
        mod.disc_math, mod.gen_backward_math, mod.stft_math = plan, gen_bwd, stft
        out = mod.training_step({k: v.to(DEV) for k, v in data.items()})
        torch.cuda.synchronize()
        enh = out["enhanced"].cpu().double()
        mse = float(((enh - logs["enhanced"].double()) ** 2).mean())
        # north-star bar: 1e-5; fp32-grade forwards 1e-10, the bf16 plans' three-product ResidualUnits 1e-8
        assert enh.shape == (32, 1, 31968) and mse < (1e-8 if plan in ("bf16", "bf16_bl") else 1e-10), (plan, mse)
        got = _adam_moments(mod.optimizers())
        g_rel, d_rel = _rel(want[0], got[0]), _rel(want[1], got[1])
        norms = (torch.stack(mod.last_norms).cpu().double() - logs["balancing/norms"].double()).abs() / logs["balancing/norms"].double().abs()
        worst = {k: abs(float(mod.logged[k]) - float(logs[k])) / abs(float(logs[k])) for k in keys}
        report[plan] = (mse, g_rel, d_rel, float(norms.max()), max(worst.values()))
        if plan in ("bf16", "bf16_bl"):
            for k, w in worst.items():
                t = tol["feature_matching_loss"] if "feature_matching" in k else tol["backprop_loss"] if "backprop" in k else tol["loss"]
                assert w <= t, (plan, k, w)
            assert float(norms.max()) < tol["balancing_norms"]
            assert g_rel < tol["generator_grad"] and d_rel < tol["discriminator_grad"], (g_rel, d_rel)
        else:
            assert max(worst.values()) <= 1e-3, (plan, worst)
            assert float(norms.max()) < 5e-3, (plan, norms)
            # the generator's gradient passes through the discriminators' sign() / LeakyReLU discontinuities too: the reference's own
            # fp32-vs-fp64 floor is the yardstick for both networks
            assert g_rel <= 2 * floor + 1e-3 and d_rel <= 2 * floor + 1e-3, (plan, g_rel, d_rel, floor)
        del mod
    print("full-size step vs oracle (enhanced MSE, generator grad, discriminator grad, balancing norms, worst logged loss): "
          + "; ".join(f"{k}: " + " ".join(f"{x:.2e}" for x in v) for k, v in report.items()))


@pytest.mark.parametrize("plan", ["bf16", "bf16_bl"])
def test_benchmarked_plan_two_steps_with_mrstft_against_oracle(hip, golden, plan):
    """What bench.py times -- discriminator plan "bf16", bf16 generator backward, MRSTFT contractions "folded_x3" -- for two
    consecutive steps on the formula clips against the CPU oracle (the reference-pinned restatement): logged values at the bf16
    tolerances of `test_bf16_step_against_reference_replay_golden`, the generator output at the fp32 bound on the first step."""
    table = {"train/generator/reconstructive_loss_freq": 2e-3, "train/generator/feature_matching_loss": 2e-2, "train/generator/adv_loss_gen": 2e-3,
             "train/generator/backprop_loss": 5e-2, "train/discriminator/real_loss": 2e-3, "train/discriminator/fake_loss": 2e-3}
    mod, g_sd, d_sd = make_module(golden, use_mrstft=True)
    mod.disc_math, mod.gen_backward_math, mod.stft_math = plan, "bf16", "folded_x3"
    for i, (bc, air, logs) in enumerate(mstep_oracle(g_sd, d_sd)):
        out = mod.training_step({"audio_body_conducted": bc.to(DEV), "audio_airborne": air.to(DEV)})
        if i == 0:
            assert max_abs(out["enhanced"], logs["enhanced"]) < 2e-5
        for k, rtol in table.items():
            np.testing.assert_allclose(mod.logged[k].item(), logs[k].item(), rtol=rtol * (1 if i == 0 else 5), err_msg=f"step {i} {k}")
        np.testing.assert_allclose(torch.stack(mod.last_norms).cpu().numpy(), logs["balancing/norms"].numpy(), rtol=5e-2)


def test_prepack_graphs_of_both_networks_survive_a_forward_at_another_shape(hip, golden):
    """train x4 (the prepack sequences, one per network, settle and are captured into HIP graphs) -> validation forward at another batch /
    length (the shared image caches miss and reallocate) -> train x2: bit-identical to the same sequence with the graphs disabled.  A
    replay that kept writing the buffers it captured would leave the generator's convolutions on pre-update weights from here on."""
    from vibravox_amd import ops

    def run(graphs):
        prev = ops.ReplayedPrepack.enabled
        ops.ReplayedPrepack.enabled = graphs
        try:
            mod, _, _ = make_module(golden, use_mrstft=False)
            captured = []
            for i in range(6):
                if i == 4:
                    mod.validation_step({"audio_body_conducted": formula_audio("pp/val/bc", 3, 5000).to(DEV),
                                         "audio_airborne": formula_audio("pp/val/air", 3, 5000).to(DEV)}, 0)
                batch = {"audio_body_conducted": formula_audio(f"pp/{i}/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio(f"pp/{i}/air", 2, 8200).to(DEV)}
                mod.training_step(batch)
                if i == 3:
                    captured = [g.graph is not None for g in (mod._prepack_graph, mod._disc_engine._prepack_graph)]   # one per network
            torch.cuda.synchronize()
            out = {f"G.{k}": v.clone() for k, v in mod.generator.state_dict().items()}
            out.update({f"D.{k}": v.clone() for k, v in mod.discriminator.state_dict().items()})
            out["enhanced"] = mod.generator(mod.generator.cut_to_valid_length(formula_audio("pp/probe", 2, 8200).to(DEV)))[0].detach().clone()
            return out, captured
        finally:
            ops.ReplayedPrepack.enabled = prev

    (a, cap_a), (b, cap_b) = run(True), run(False)
    assert len(cap_a) == 2 and all(cap_a) and not any(cap_b), (cap_a, cap_b)   # both sequences were graph replays before the validation forward
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


def test_generator_graphs_match_eager_launches(hip, golden):
    """The generator's training forward, input-gradient chain and weight-gradient launches replayed as HIP graphs (gen_engine.py:
    forward_train / backward_train) against the same launches issued one by one: train x5 (the three sequences settle and are
    captured) -> validation forward at another shape (image caches reallocate: the signatures change, eager rounds, new captures)
    -> train x5, a new batch tensor every step: bit-identical parameters and outputs."""
    from vibravox_amd import gen_engine, ops

    def run(graphs):
        prev = gen_engine.USE_GRAPHS
        gen_engine.USE_GRAPHS = graphs
        try:
            mod, _, _ = make_module(golden, use_mrstft=True)
            mod.gen_backward_math = "bf16"
            captured = []
            for i in range(10):
                if i == 5:
                    mod.validation_step({"audio_body_conducted": formula_audio("gg/val/bc", 3, 5000).to(DEV),
                                         "audio_airborne": formula_audio("gg/val/air", 3, 5000).to(DEV)}, 0)
                batch = {"audio_body_conducted": formula_audio(f"gg/{i}/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio(f"gg/{i}/air", 2, 8200).to(DEV)}
                mod.training_step(batch)
                if i in (4, 9):
                    e = mod.generator._engine
                    captured.append(sum(g.graph is not None for g in [e._fwd_graph] + e._dx_graphs + e._dw_graphs))
            torch.cuda.synchronize()
            out = {f"G.{k}": v.clone() for k, v in mod.generator.state_dict().items()}
            out.update({f"D.{k}": v.clone() for k, v in mod.discriminator.state_dict().items()})
            out["enhanced"] = mod.generator(mod.generator.cut_to_valid_length(formula_audio("gg/probe", 2, 8200).to(DEV)))[0].detach().clone()
            return out, captured
        finally:
            gen_engine.USE_GRAPHS = prev

    (a, cap_a), (b, cap_b) = run(True), run(False)
    groups = len([t for t in gen_engine.BWD_GROUPS.split(",") if t.strip()])   # backward segment groups (default: one segment each, 7)
    assert cap_a == [1 + 2 * groups] * 2 and cap_b == [0, 0], (cap_a, cap_b)   # forward + groups x (input gradients, weight gradients)
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


def test_two_generator_forwards_before_one_backward_with_graphs(hip, golden):
    """Plain PyTorch semantics next to the replayed generator forward (gen_engine.forward_train): y1 = G(x1); y2 = G(x2);
    loss(y1, y2).backward().  A replay rewrites the previous replay's saved activations in place, so the second forward must not replay
    while the first is undifferentiated -- gradients bit-identical to the same sequence with graphs off; and a backward through a forward
    whose buffers a LATER replay has rewritten (retain_graph, new forward, second backward) raises instead of returning wrong gradients."""
    from vibravox_amd import gen_engine

    def run(graphs):
        prev = gen_engine.USE_GRAPHS
        gen_engine.USE_GRAPHS = graphs
        try:
            mod, _, _ = make_module(golden, use_mrstft=False)
            mod.gen_backward_math = "f32"
            for i in range(5):   # the training forward settles and is captured
                mod.training_step({"audio_body_conducted": formula_audio(f"tf/{i}/bc", 2, 8200).to(DEV), "audio_airborne": formula_audio(f"tf/{i}/air", 2, 8200).to(DEV)})
            gen = mod.generator
            assert (gen._engine._fwd_graph.graph is not None) == graphs
            for p in gen.parameters():
                p.grad = None
            x1 = gen.cut_to_valid_length(formula_audio("tf/x1", 2, 8200).to(DEV))
            x2 = gen.cut_to_valid_length(formula_audio("tf/x2", 2, 8200).to(DEV))
            w1, w2 = formula_audio("tf/w1", 2, x1.shape[-1]).to(DEV), formula_audio("tf/w2", 2, x1.shape[-1]).to(DEV)
            y1 = gen(x1)[0]
            y2 = gen(x2)[0]
            ((y1 * w1).sum() + (y2 * w2).sum()).backward()
            torch.cuda.synchronize()
            out = {k: p.grad.clone() for k, p in gen.named_parameters() if p.grad is not None}
            out["y1"], out["y2"] = y1.detach().clone(), y2.detach().clone()
            return out, gen
        finally:
            gen_engine.USE_GRAPHS = prev

    (a, gen), (b, _) = run(True), run(False)
    assert len(a) > 80 and [k for k in a if not torch.equal(a[k], b[k])] == []
    prev = gen_engine.USE_GRAPHS
    gen_engine.USE_GRAPHS = True
    try:
        x = gen.cut_to_valid_length(formula_audio("tf/x3", 2, 8200).to(DEV))
        y = gen(x)[0]
        y.sum().backward(retain_graph=True)
        gen(x)[0].sum().backward()              # a newer replay rewrites the buffers y's graph still points at
        with pytest.raises(RuntimeError, match="rewritten by a later replayed forward"):
            y.sum().backward()
    finally:
        gen_engine.USE_GRAPHS = prev


def test_replayed_sequences_follow_changing_batch_shapes(hip, golden):
    """Train steps at alternating batch shapes (2 x 8200, 3 x 6100, each twice in a row so that the sequences of BOTH shapes are captured,
    then interleaved) in the benchmarked plan: every replayed sequence -- discriminator chains, generator forward / backward, prepack --
    against the same steps with all launch sequences issued eagerly: bit-identical parameters."""
    from vibravox_amd import gen_engine, ops

    shapes = [(2, 8200), (2, 8200), (2, 8200), (3, 6100), (3, 6100), (3, 6100), (2, 8200), (3, 6100), (2, 8200), (2, 8200)]

    def run(graphs):
        prev = (ops.ReplayedChain.enabled, ops.ReplayedPrepack.enabled, gen_engine.USE_GRAPHS)
        ops.ReplayedChain.enabled = ops.ReplayedPrepack.enabled = gen_engine.USE_GRAPHS = graphs
        try:
            mod, _, _ = make_module(golden, use_mrstft=True)
            mod.disc_math, mod.gen_backward_math, mod.stft_math = "bf16_bl", "bf16", "folded_x3"
            for i, (b, t) in enumerate(shapes):
                mod.training_step({"audio_body_conducted": formula_audio(f"sh/{i}/bc", b, t).to(DEV), "audio_airborne": formula_audio(f"sh/{i}/air", b, t).to(DEV)})
            torch.cuda.synchronize()
            out = {f"G.{k}": v.clone() for k, v in mod.generator.state_dict().items()}
            out.update({f"D.{k}": v.clone() for k, v in mod.discriminator.state_dict().items()})
            return out
        finally:
            ops.ReplayedChain.enabled, ops.ReplayedPrepack.enabled, gen_engine.USE_GRAPHS = prev

    a, b = run(True), run(False)
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


def test_fused_adam_follows_a_restored_state(hip):
    """optimizer.load_state_dict() after a step replaces the moment tensors: the kernel's cached table must follow (and a deep copy
    of the optimiser must step at all)."""
    import copy

    from vibravox_amd.optim import FusedAdam

    torch.manual_seed(0)
    w = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (1000, 17, 4096)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in w]
    ours, theirs = FusedAdam(w, lr=3e-4, betas=(0.5, 0.9)), torch.optim.Adam(ref, lr=3e-4, betas=(0.5, 0.9))
    def step(k):
        for p, q in zip(w, ref):
            g = torch.randn(p.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(100 + k))
            p.grad, q.grad = g.clone(), g.clone()
        ours.step(); theirs.step()
    step(0); step(1)
    saved_o, saved_t = copy.deepcopy(ours.state_dict()), copy.deepcopy(theirs.state_dict())
    step(2)
    ours.load_state_dict(saved_o); theirs.load_state_dict(saved_t)   # back to the state after two steps: new moment tensors
    step(3)
    for p, q in zip(w, ref):
        assert torch.allclose(p, q, rtol=0, atol=2e-6)
    for p, q in zip(w, ref):
        assert torch.allclose(ours.state[p]["exp_avg"], theirs.state[q]["exp_avg"], rtol=1e-5, atol=1e-6)   # a stale table would be off by O(1)
    clone = copy.deepcopy(ours)
    for p in clone.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    clone.step()



def test_bundle_layout_step_against_the_fp32_at_rest_bf16_step(hip):
    """Plan "bf16_bl" (embeddings / stacked gradients at rest as bf16 bundles: disc_engine_bl.py) against plan "bf16" (fp32 tensors at
    rest, rounded when staged) at BASELINE config 2: the MFMA operands are the same roundings of the same values, so one step from the
    same state gives the same losses and gradients up to summation order, the 16-bit (hi + lo) feature-matching / logits operands and
    the bf16 roundings those flip -- [MI355X] losses 4e-6, balancing norms 3e-5, generator gradient 1.3e-4, discriminator gradient
    4e-3 (R = 240), i.e. a tenth of what separates either plan from the fp32 step (BF16_STEP_TOLERANCES)."""
    import bench

    def make():
        return bench.build_module(DEV, 1234), bench.synthetic_batch(32, 32000, 1234, DEV)

    a = _one_step(make, "bf16", "bf16", stft_math="folded_x3")
    b = _one_step(make, "bf16_bl", "bf16", stft_math="folded_x3")
    assert torch.equal(a[0], b[0])
    worst = max(abs(b[1][k] - v) / abs(v) for k, v in a[1].items())
    norms = float(((a[2] - b[2]).abs() / a[2].abs()).max())
    g_rel, d_rel = _rel(a[3][0], b[3][0]), _rel(a[3][1], b[3][1])
    print(f"bundle layout vs fp32 at rest: worst logged value {worst:.2e}, balancing norms {norms:.2e}, generator grad {g_rel:.2e}, discriminator grad {d_rel:.2e}")
    assert worst < 5e-5 and norms < 3e-4
    assert g_rel < 1e-3 and d_rel < 1.5e-2
