"""GPU: the fit loop end to end on a WAVE tree -- batch 2, ``constant_length-500-ms``, 6 train, 3 validation and 3 test clips; the
shape ``tests/test_gpu_corpus.py::test_two_training_steps_and_a_test_split_from_files`` trains at.

Run A is ``fit`` over 2 epochs of 3 steps; A' is the same run again; run B is stopped behind step 3 (``every_n_train_steps=3``) and
continued by a freshly built module with another initialisation from ``checkpoints/last.ckpt``.  Bit equality of A and B rests on
the training kernels summing in a fixed order (no floating-point atomics under csrc/), which is why A and A' are compared first: the
resume comparison allows every tensor 4 times the largest difference A and A' show for it -- zero, when they agree bit for bit.

Figures measured on the MI355X for A against A' (largest difference over all tensors and logged values): 32-true 0, bf16-mixed 0.
"""
import csv
import functools
import os
import shutil
from functools import partial

import numpy as np
import pytest
import torch

from tests import corpus_fixtures as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENSOR = "throat_microphone"
TRAIN = [("a", "PCM16", 9000, 16000, 1), ("b", "PCM16", 36000, 48000, 1), ("c", "PCM24", 8500, 16000, 1), ("d", "FLOAT32", 8001, 16000, 2),
         ("e", "PCM32", 20000, 16000, 1), ("f", "PCM16", 9000, 16000, 1)]          # at 16 kHz every clip is longer than 500 ms = 8000 samples
EVAL = [("p", "PCM16", 36000, 48000, 1), ("q", "PCM24", 20000, 16000, 1), ("r", "FLOAT32", 9000, 16000, 2)]   # 0.75 s, 1.25 s, 0.56 s
PRECISIONS = ["32-true", "bf16-mixed"]


def write_split(root, split, specs, seed):
    for s_i, sensor in enumerate(["headset_microphone", SENSOR]):
        for k, (stem, fmt, frames, rate, channels) in enumerate(specs):
            x = W.samples(fmt, frames, channels, seed + 100 * s_i + k)
            x = (x * np.float32(0.1)).astype(np.float32) if fmt == "FLOAT32" else x // 10   # a tenth of full scale, as recordings are
            W.write_wav(os.path.join(root, "speech_clean", split, sensor, stem + ".wav"), x, fmt, rate)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("fit_corpus")
    write_split(root, "train", TRAIN, 0)
    write_split(root, "validation", EVAL, 1000)
    write_split(root, "test", EVAL, 2000)
    return root


def build(seed):
    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    torch.manual_seed(seed)
    opt = partial(FusedAdam, lr=3e-4, betas=(0.5, 0.9))
    return EBENLightningModule(
        sample_rate=16000, generator=EBENGenerator(m=4, n=32, p=2).to(DEV), discriminator=DiscriminatorEBENMultiScales(q=4, min_channels=24).to(DEV),
        generator_optimizer=opt, discriminator_optimizer=opt,
        reconstructive_loss_freq_fn=MultiResolutionSTFTLoss(fft_sizes=(512, 1024, 2048), hop_sizes=(50, 120, 240), win_lengths=(240, 600, 1200),
                                                            sample_rate=16000, perceptual_weighting=True).to(DEV),
        feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales(), adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales(),
        dynamic_loss_balancing="ema")


class StopAt:
    def __init__(self, step):
        self.step = step

    def on_train_batch_end(self, trainer, module):
        if trainer.global_step == self.step:
            trainer.should_stop = True


def full_state(mod):
    """Every state_dict tensor, both moments and the step of every trained parameter, and the balancer's norms, on the host."""
    out = {f"state_dict/{k}": v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    for i, opt in enumerate(mod.configure_optimizers()):
        for idx, st in opt.state_dict()["state"].items():
            out.update({f"optimizer{i}/{idx}/{k}": torch.as_tensor(v).detach().cpu().clone() for k, v in st.items()})
    out.update({f"balancer/{k}": t.detach().cpu().clone() for k, t in enumerate(mod.balancer.old)})
    return out


def fit(tree, work, precision, *, seed=3, every=None, stop=None, ckpt_path=None):
    from vibravox_amd import fit as F
    from vibravox_amd.lightning_datamodules import LocalBWEDataModule

    mod = build(seed)
    dm = LocalBWEDataModule(16000, root=tree, sensor=SENSOR, collate_strategy="constant_length-500-ms", batch_size=2, shuffle=True, device=DEV)
    policy = F.ModelCheckpoint(monitor="validation/torchmetrics_stoi", mode="max", save_top_k=2, save_last=True, dirpath=str(work / "checkpoints"),
                               filename="epoch_{epoch:03d}", every_n_train_steps=every)
    log = F.CSVLogger(str(work / "csv"))
    trainer = F.Trainer(max_epochs=2, log_every_n_steps=1, precision=precision, callbacks=[policy] + ([StopAt(stop)] if stop else []), logger=log)
    torch.manual_seed(11)   # the run's draws: the collator's crops and the discriminator-update draw of every step
    trainer.fit(mod, dm, ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    return dict(module=mod, dm=dm, trainer=trainer, rows=list(log.rows), state=full_state(mod), work=work)


@functools.lru_cache(maxsize=None)
def run_a(tree, base, precision):
    return fit(tree, base / f"a-{precision}", precision)


def worst(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return tmp_path_factory.mktemp("fit_runs")


@pytest.fixture(scope="module")
def repeat_bounds():
    """precision -> {tensor or logged name: largest |A - A'|}, filled by the determinism test (the resume test runs behind it)."""
    return {}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_uninterrupted_runs_agree_and_leave_the_policys_files(hip, tree, base, repeat_bounds, precision):
    a = run_a(tree, base, precision)
    again = fit(tree, base / f"again-{precision}", precision)
    assert a["trainer"].global_step == 6 and a["trainer"].current_epoch == 2
    assert [(r["epoch"], r["step"]) for r in a["rows"]] == [(0, 1), (0, 2), (0, 3), (0, 3), (1, 4), (1, 5), (1, 6), (1, 6)]
    assert a["state"].keys() == again["state"].keys()
    bounds = {k: worst(a["state"][k], again["state"][k]) for k in a["state"]}
    for ra, rb in zip(a["rows"], again["rows"]):
        assert ra.keys() == rb.keys()
        for k in ra:
            bounds[f"logged/{k}"] = max(bounds.get(f"logged/{k}", 0.0), abs(ra[k] - rb[k]))
    repeat_bounds[precision] = bounds
    print(f"{precision}: A against A': largest difference {max(bounds.values()):.3e} ({max(bounds, key=bounds.get)})")
    # the files of save_top_k=2 + save_last over two epochs, and no others
    ck = a["work"] / "checkpoints"
    assert sorted(os.listdir(ck)) == ["epoch_000.ckpt", "epoch_001.ckpt", "last.ckpt"]
    for name in os.listdir(ck):
        loaded = torch.load(ck / name, map_location="cpu", weights_only=True)
        assert loaded["epoch"] == (0 if name == "epoch_000.ckpt" else 1) and list(loaded["state_dict"]) == list(a["module"].state_dict())
    last = torch.load(ck / "last.ckpt", map_location="cpu", weights_only=True)
    for k, v in last["state_dict"].items():
        assert torch.equal(v, a["state"][f"state_dict/{k}"]), k
    assert last["global_step"] == 12 and last["vibravox_amd"]["train_step"] == 6 and last["vibravox_amd"]["precision"] == precision
    with open(a["work"] / "csv" / "metrics.csv", newline="") as f:
        table = list(csv.DictReader(f))
    stoi = [(row["epoch"], row["step"]) for row in table if row["validation/torchmetrics_stoi"] != ""]
    assert stoi == [("0", "3"), ("1", "6")] and all(np.isfinite(float(row["validation/torchmetrics_stoi"])) for row in table
                                                    if row["validation/torchmetrics_stoi"] != "")
    assert max(bounds.values()) == 0.0, {k: v for k, v in bounds.items() if v}     # the finding, were it otherwise: see the module docstring


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_resumed_run_ends_where_the_uninterrupted_one_ends(hip, tree, base, repeat_bounds, precision):
    from vibravox_amd import checkpoint as C

    a = run_a(tree, base, precision)
    work = base / f"b-{precision}"
    first = fit(tree, work, precision, every=3, stop=3)
    assert first["trainer"].global_step == 3 and first["rows"] == a["rows"][:3]
    assert os.listdir(work / "checkpoints") == ["last.ckpt"]          # stopped before the epoch's validation: no ranked file yet
    saved = C.load_file(str(work / "checkpoints" / "last.ckpt"))["vibravox_amd"]
    assert (saved["train_step"], saved["loader_epoch"], saved["batches_served"]) == (3, 0, 3)
    second = fit(tree, work, precision, seed=99, every=3, ckpt_path=str(work / "checkpoints" / "last.ckpt"))
    assert second["trainer"].global_step == 6 and second["trainer"].current_epoch == 2
    bounds = repeat_bounds.get(precision, {})
    assert second["state"].keys() == a["state"].keys()
    for k, want in a["state"].items():
        got = second["state"][k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        allowed = 4 * bounds.get(k, 0.0)
        if allowed == 0.0:
            assert torch.equal(got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8)), k
        else:
            assert worst(got, want) <= allowed, (k, worst(got, want), allowed)
    assert [(r["epoch"], r["step"]) for r in second["rows"]] == [(r["epoch"], r["step"]) for r in a["rows"][3:]]
    for got, want in zip(second["rows"], a["rows"][3:]):                # the validation of epoch 0 and everything of steps 4 to 6
        assert got.keys() == want.keys()
        for k in want:
            assert abs(got[k] - want[k]) <= 4 * bounds.get(f"logged/{k}", 0.0), (k, got[k], want[k])
    assert sorted(os.listdir(work / "checkpoints")) == ["epoch_000.ckpt", "epoch_001.ckpt", "last.ckpt"]


def scramble(mod):
    from vibravox_amd import ops

    with torch.no_grad():
        for p in mod.parameters():
            if p.requires_grad:
                p.mul_(0.5).add_(0.01)
    ops.bump_weights_epoch([p for p in mod.parameters() if p.requires_grad])   # as an optimizer that wrote them would


def test_the_test_stage_and_the_exported_generator_follow_last_ckpt(hip, tree, base, tmp_path):
    from vibravox_amd import checkpoint as C
    from vibravox_amd import inference
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    a = run_a(tree, base, "bf16-mixed")
    mod, dm, trainer = a["module"], a["dm"], a["trainer"]
    C.restore(mod, a["work"] / "checkpoints" / "last.ckpt")   # run A's final state (the first test of this file compares the two), whatever ran since
    dm.setup("test")
    corrupted, reference = dm.test_clips()
    mod.eval()
    mod.logged.clear()
    mod.evaluate_clips(corrupted, reference, losses=True)
    want = {k: float(v) for k, v in mod.logged.items() if k.startswith("test/")}
    enhanced = [e.clone() for e in inference.enhance_clips(mod.generator, corrupted)]
    assert {"test/torchmetrics_si_sdr", "test/torchmetrics_stoi", "test/generator/feature_matching_loss", "test/discriminator/real_loss"} <= set(want)
    scramble(mod)          # what Trainer.test restores over: other weights, and the packed images built from them
    assert not torch.equal(inference.enhance_clips(mod.generator, corrupted)[0], enhanced[0])
    got = trainer.test(mod, dm, ckpt_path="last")
    assert got == want
    assert trainer.logger.rows[-1] == dict(want, epoch=2, step=6)
    out = C.export_generator(a["work"] / "checkpoints" / "last.ckpt", tmp_path / "pretrained")
    gen = EBENGenerator.from_pretrained(out).to(DEV).eval()
    again = inference.enhance_clips(gen, corrupted)
    assert len(again) == len(enhanced) == 3 and all(torch.equal(x, y) for x, y in zip(again, enhanced))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_trained_module_taken_back_to_an_earlier_checkpoint_repeats_the_run(hip, tree, base, tmp_path, precision):
    """``fit(ckpt_path=epoch_000.ckpt)`` on run A's own module, which has trained past that point: its moments, its graphs and the packed
    and bf16 images derived from its newer weights exist.  A restore that left those images as they are would continue from stale ones."""
    from vibravox_amd import fit as F

    a = run_a(tree, base, precision)
    policy = F.ModelCheckpoint(monitor="validation/torchmetrics_stoi", mode="max", save_top_k=2, save_last=True, dirpath=str(tmp_path / "checkpoints"),
                               filename="epoch_{epoch:03d}")
    log = F.CSVLogger(str(tmp_path / "csv"))
    trainer = F.Trainer(max_epochs=2, log_every_n_steps=1, precision=precision, callbacks=[policy], logger=log)
    torch.manual_seed(5)   # replaced by the checkpoint's
    trainer.fit(a["module"], a["dm"], ckpt_path=str(a["work"] / "checkpoints" / "epoch_000.ckpt"))
    assert trainer.global_step == 6 and log.rows == a["rows"][4:]            # steps 4 to 6 and the second validation
    got = full_state(a["module"])
    assert got.keys() == a["state"].keys()
    for k, want in a["state"].items():
        assert torch.equal(got[k].reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8)), k
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["epoch_001.ckpt", "last.ckpt"]


class Poison:
    """Sets one weight to NaN behind a step, in front of the checkpoint callback."""

    def on_train_batch_end(self, trainer, module):
        with torch.no_grad():
            module.generator.last_conv.weight[1, 2, 0] = float("nan")


def test_a_non_finite_parameter_is_refused_and_the_files_stay(hip, tree, base, tmp_path):
    from vibravox_amd import fit as F

    a = run_a(tree, base, "bf16-mixed")
    ck = tmp_path / "checkpoints"
    shutil.copytree(a["work"] / "checkpoints", ck)
    before = {n: (ck / n).read_bytes() for n in sorted(os.listdir(ck))}
    policy = F.ModelCheckpoint(monitor="validation/torchmetrics_stoi", mode="max", save_top_k=2, save_last=True, dirpath=str(ck),
                               filename="epoch_{epoch:03d}", every_n_train_steps=1)
    trainer = F.Trainer(max_epochs=2, limit_train_batches=1, precision="bf16-mixed", callbacks=[Poison(), policy, StopAt(4)])
    with pytest.raises(F.NonFiniteError, match=r"state_dict\.generator\.last_conv\.weight holds 1 non-finite value"):
        trainer.fit(a["module"], a["dm"], ckpt_path=str(ck / "epoch_000.ckpt"))     # one step of epoch 1, then the refused save
    assert trainer.global_step == 4
    assert {n: (ck / n).read_bytes() for n in sorted(os.listdir(ck))} == before
