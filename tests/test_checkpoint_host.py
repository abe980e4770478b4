"""No GPU: the image plan, the checkpoint file and its restore on the CPU path, the checkpoint policy's bookkeeping, the CSV logger,
``run.compose`` with the new groups, and a fit that is interrupted and resumed on CPU stand-ins (the toy networks of
``tests/test_step_paths.py``) -- which must end where the uninterrupted fit ends, bit for bit."""
import csv
import os
from functools import partial

import pytest
import torch

from tests import test_step_paths as S
from vibravox_amd import checkpoint as C
from vibravox_amd import fit as F
from vibravox_amd.lightning_datamodules.local_bwe import ResidentLoader
from vibravox_amd.lightning_modules.eben import EBENLightningModule


# ---- plan_image -------------------------------------------------------------------------------------------------------------------------
def test_plan_image_offsets_order_and_size():
    named = [("w", torch.zeros(3, 5)), ("none", torch.zeros(0, 7)), ("b", torch.zeros(1, dtype=torch.uint8)), ("i", torch.zeros(2, dtype=torch.int64)),
             ("h", torch.zeros(9, dtype=torch.bfloat16)), ("s", torch.tensor(1.0))]
    plan = C.plan_image(named)
    assert plan.names == ["w", "none", "b", "i", "h", "s"]
    assert [(e.offset, e.nbytes) for e in plan.entries] == [(0, 60), (64, 0), (64, 1), (80, 16), (96, 18), (128, 4)]
    assert [e.shape for e in plan.entries] == [(3, 5), (0, 7), (1,), (2,), (9,), ()] and plan.entries[4].dtype is torch.bfloat16
    assert plan.total == 144 and plan.counters_bytes == 32 and plan.image_bytes == 176
    assert C.plan_image(dict(named)) == plan and C.plan_image([]).total == 0
    tensors = [torch.randn(3, 5), torch.zeros(0, 7), torch.tensor([7], dtype=torch.uint8), torch.tensor([1, -2]),
               torch.randn(9).to(torch.bfloat16), torch.tensor(float("nan"))]
    image = C.assemble_host(plan, tensors, torch.full((plan.image_bytes + 8,), 0xA5, dtype=torch.uint8))
    for e, t in zip(plan.entries, tensors):
        assert torch.equal(plan.view(image, e).reshape(-1).view(torch.uint8), t.contiguous().reshape(-1).view(torch.uint8)), e.name
    assert image[60:64].tolist() == [0] * 4 and image[65:80].tolist() == [0] * 15 and image[132:144].tolist() == [0] * 12   # zeroed padding
    assert plan.counters(image).tolist() == [0, 0, 0, 0, 0, 1] and image[plan.image_bytes:].tolist() == [0xA5] * 8


def test_the_abi_plans_and_refuses_without_a_device():
    """``eben_pack_plan`` is host arithmetic, and a malformed table is refused before the first HIP call: both run here."""
    import ctypes

    from vibravox_amd import _lib
    from vibravox_amd._lib import EbenPackEntry

    lib, b = _lib.load(), _lib.pack_block_bytes()
    assert b == 16384 and ctypes.sizeof(EbenPackEntry) == 32
    sizes = [0, 4, b, b + 4, 3 * b + 20]
    table, at = (EbenPackEntry * len(sizes))(), 0
    for k, n in enumerate(sizes):
        table[k] = EbenPackEntry(4096, at, n, 1, 0)
        at = (at + n + 15) // 16 * 16
    blocks = ctypes.c_int64(-1)
    assert lib.eben_pack_plan(table, len(sizes), ctypes.byref(blocks), None) == 0 and blocks.value == 0 + 1 + 1 + 2 + 4
    for field, value in (("image_offset", table[2].image_offset + 4), ("nbytes", b + 32), ("nbytes", b - 2), ("tensor", None), ("kind", 2),
                         ("nbytes", -4), ("image_offset", 1 << 40)):
        bad = (EbenPackEntry * len(sizes))(*table)
        setattr(bad[2], field, value)
        assert lib.eben_pack_tensors(bad, len(sizes), 4096, at, 8192, None) == -1, (field, value)
        assert lib.eben_unpack_tensors(bad, len(sizes), 4096, at, None) == -1, (field, value)
        assert b"entr" in lib.eben_last_error()
    assert lib.eben_pack_tensors(table, len(sizes), 4096 + 8, at, 8192, None) == -1        # the image off the 16-byte grid
    assert lib.eben_pack_tensors(table, len(sizes), 4096, at, None, None) == -1            # float32 entries without counters


# ---- CPU stand-ins ----------------------------------------------------------------------------------------------------------------------
def stub(seed, ratio=0.5):
    torch.manual_seed(seed)
    gen, disc = S._ToyGenerator(), S._ToyDiscriminator()
    opt = partial(torch.optim.Adam, lr=3e-4, betas=(0.5, 0.9))
    return EBENLightningModule(
        sample_rate=16000, generator=gen, discriminator=disc, generator_optimizer=opt, discriminator_optimizer=opt,
        reconstructive_loss_freq_fn=None, reconstructive_loss_time_fn=torch.nn.L1Loss(), feature_matching_loss_fn=S._FeatureLoss(),
        adversarial_loss_fn=S._HingeLoss(), dynamic_loss_balancing="ema", beta_ema=0.9, update_discriminator_ratio=ratio)


class StubData:
    """Six clips of 160 samples; a batch is a random 130-sample crop of two of them, drawn from the global CPU generator like the
    collators' crops.  ``built`` counts the batches that were assembled."""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.clips = [(torch.randn(1, 160, generator=g), torch.randn(1, 160, generator=g)) for _ in range(6)]
        self.built = 0

    def make(self, indices):
        self.built += 1
        at = [int(torch.randint(0, 31, (1,))) for _ in indices]
        return {"audio_body_conducted": torch.stack([self.clips[i][0][:, a:a + 130] for i, a in zip(indices, at)]),
                "audio_airborne": torch.stack([self.clips[i][1][:, a:a + 130] for i, a in zip(indices, at)])}

    def train_dataloader(self):
        return ResidentLoader(6, 2, self.make, shuffle=True, seed=5)


def full_state(mod):
    """Every tensor, step and balancer value of a module, by name."""
    out = {f"sd/{k}": v.clone() for k, v in mod.state_dict().items()}
    for i, opt in enumerate(mod.configure_optimizers()):
        for idx, st in opt.state_dict()["state"].items():
            out.update({f"opt{i}/{idx}/{k}": torch.as_tensor(v).clone() for k, v in st.items()})
    out.update({f"balancer/{k}": torch.as_tensor(t).clone() for k, t in enumerate(mod.balancer.old or [])})
    return out


def assert_same_state(a, b):
    sa, sb = full_state(a), full_state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k].reshape(-1).view(torch.uint8), sb[k].reshape(-1).view(torch.uint8)), k


def train(mod, steps, seed=87):
    torch.manual_seed(seed)
    data = StubData()
    for _ in range(steps):
        mod.training_step(data.make([0, 1]))


# ---- file round trip --------------------------------------------------------------------------------------------------------------------
def test_cpu_round_trip_through_the_file(tmp_path):
    a = stub(1)
    train(a, 3)
    taken = C.Snapshot().take(C.TrainState.of(a, {"epoch": 2, "train_step": 3, "loader_epoch": 2, "batches_served": 1}))
    assert taken.nonfinite() == []
    path = str(tmp_path / "x" / "a.ckpt")
    C.write_file(taken.checkpoint({"ModelCheckpoint": {"best_model_path": "p"}}), path)
    assert os.listdir(tmp_path / "x") == ["a.ckpt"]                                           # the .tmp name is gone
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "optimizer_states", "lr_schedulers", "loops", "callbacks",
            "vibravox_amd"} == set(ckpt)
    assert ckpt["epoch"] == 2 and ckpt["lr_schedulers"] == [] and ckpt["vibravox_amd"]["train_step"] == 3
    # optimizer.step() calls over both optimizers: 3 of the generator's and one per discriminator update (ratio 0.5)
    optimizer_steps = sum(int(max(float(st["step"]) for st in opt.state_dict()["state"].values())) for opt in a.configure_optimizers())
    assert ckpt["global_step"] == optimizer_steps and 3 <= optimizer_steps <= 6 and list(ckpt["state_dict"]) == list(a.state_dict())
    storages = {t.untyped_storage().data_ptr() for t in ckpt["state_dict"].values()}
    storages |= {st[k].untyped_storage().data_ptr() for o in ckpt["optimizer_states"] for st in o["state"].values() for k in ("exp_avg", "exp_avg_sq")}
    assert len(storages) == 1                                                                 # one image, written once
    for o, opt in zip(ckpt["optimizer_states"], a.configure_optimizers()):                    # torch's own layout: a fresh Adam loads it
        want = opt.state_dict()
        assert o["param_groups"] == want["param_groups"] and o["state"].keys() == want["state"].keys()
    b = stub(2)
    with pytest.raises(AssertionError):
        assert_same_state(a, b)
    torch.manual_seed(1234)
    report = C.restore(b, path)
    assert report == {"skipped": [], "epoch": 2, "global_step": optimizer_steps, "train_step": 3, "loader_epoch": 2, "batches_served": 1,
                      "callbacks": {"ModelCheckpoint": {"best_model_path": "p"}}, "native": True}
    assert_same_state(a, b)
    assert torch.equal(torch.get_rng_state(), taken.state.rng_cpu)
    torch.set_rng_state(taken.state.rng_cpu)
    want = torch.rand(1)
    C.restore(b, ckpt)
    assert torch.equal(torch.rand(1), want)
    # and the continuation is the uninterrupted one
    torch.set_rng_state(taken.state.rng_cpu)
    data = StubData()
    batch = data.make([2, 3])
    torch.set_rng_state(taken.state.rng_cpu)
    a.training_step(batch)
    torch.set_rng_state(taken.state.rng_cpu)
    b.training_step({k: v.clone() for k, v in batch.items()})
    assert_same_state(a, b)


def test_snapshot_before_the_first_step_and_restore_creates_moments(tmp_path):
    fresh = stub(1)
    taken = C.Snapshot().take(C.TrainState.of(fresh))
    assert taken.state.balancer is None and taken.state.moments == [{}, {}]
    trained = stub(1)
    train(trained, 2)
    C.write_file(C.Snapshot().take(C.TrainState.of(trained)).checkpoint(), str(tmp_path / "t.ckpt"))
    C.restore(fresh, str(tmp_path / "t.ckpt"))          # a fresh optimizer: the moments are created as its first step creates them
    assert_same_state(trained, fresh)
    C.restore(trained, taken.checkpoint())              # and back: no balancer state, moments kept where the checkpoint has none
    assert trained.balancer.old is None


def test_foreign_checkpoints(tmp_path):
    a = stub(1)
    train(a, 2)
    ckpt = C.Snapshot().take(C.TrainState.of(a)).checkpoint()
    foreign = {"state_dict": dict(ckpt["state_dict"]), "optimizer_states": ckpt["optimizer_states"], "epoch": 4, "global_step": 9}
    foreign["state_dict"]["metrics.torchmetrics_stoi.total"] = torch.zeros(1)
    foreign["state_dict"]["reconstructive_loss_freq_fn.window"] = torch.zeros(4)
    b = stub(2)
    b.balancer.old = [torch.tensor(1.0)]
    torch.manual_seed(77)
    before = torch.get_rng_state()
    report = C.restore(b, foreign)
    assert report["skipped"] == ["metrics.torchmetrics_stoi.total", "reconstructive_loss_freq_fn.window"] and not report["native"]
    assert (report["epoch"], report["global_step"], report["train_step"], report["loader_epoch"], report["batches_served"]) == (4, 9, 0, 4, 0)
    assert b.balancer.old is None and torch.equal(torch.get_rng_state(), before)      # a fresh balancer, the RNG left alone
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    missing = dict(foreign, state_dict={k: v for k, v in foreign["state_dict"].items() if k != "generator.last_conv.weight"})
    with pytest.raises(KeyError, match="generator.last_conv.weight"):
        C.restore(stub(2), missing)
    extra = dict(foreign, state_dict=dict(foreign["state_dict"], **{"discriminator.more.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="discriminator.more.weight"):
        C.restore(stub(2), extra)
    weights = dict(foreign)
    del weights["optimizer_states"]
    c = stub(3)
    C.restore(c, weights)                                                               # weights only: the optimizers stay fresh
    assert all(not opt.state_dict()["state"] for opt in c.configure_optimizers())


def test_export_generator_loads_with_from_pretrained(tmp_path):
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(7)
            self.generator = EBENGenerator(m=4, n=32, p=2)
            self.head = torch.nn.Linear(2, 2)

        def configure_optimizers(self):
            return []

    holder = Holder()
    path = str(tmp_path / "g.ckpt")
    C.write_file(C.Snapshot().take(C.TrainState.of(holder)).checkpoint(), path)
    out = C.export_generator(path, tmp_path / "pretrained")
    assert sorted(os.listdir(out)) == ["config.json", "model.safetensors"]
    back = EBENGenerator.from_pretrained(out)
    want, got = holder.generator.state_dict(), back.state_dict()
    assert list(want) == list(got) and back.p == 2
    for k in want:
        assert torch.equal(want[k], got[k]), k
    C.write_file({"state_dict": {"generator.x": torch.zeros(1)}}, str(tmp_path / "foreign.ckpt"))
    with pytest.raises(ValueError, match="m, n, p"):
        C.export_generator(tmp_path / "foreign.ckpt", tmp_path / "nothing")


# ---- ModelCheckpoint --------------------------------------------------------------------------------------------------------------------
class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.generator = torch.nn.Linear(3, 2)

    def configure_optimizers(self):
        return []


class Clock:
    """What ``ModelCheckpoint.save`` reads of a trainer."""

    def __init__(self):
        self.current_epoch = self.global_step = 0

    def counters(self):
        return {"epoch": self.current_epoch, "train_step": self.global_step}


def files_after_each(tmp_path, scores, **policy):
    cb = F.ModelCheckpoint(monitor="validation/torchmetrics_stoi", dirpath=str(tmp_path / "ck"), filename="epoch_{epoch:03d}", **policy)
    clock, module, seen = Clock(), Tiny(), []
    for epoch, score in enumerate(scores):
        clock.current_epoch, clock.global_step = epoch, 3 * (epoch + 1)
        cb.save(clock, module, {"validation/torchmetrics_stoi": score})
        cb.drain()
        seen.append(sorted(os.listdir(tmp_path / "ck")) if os.path.isdir(tmp_path / "ck") else [])
    return cb, seen


def names(*epochs, last=True):
    return sorted([f"epoch_{e:03d}.ckpt" for e in epochs] + (["last.ckpt"] if last else []))


SCORES = [0.5, 0.7, 0.7, 0.6, 0.9, 0.1]   # a tie at epochs 1 and 2


@pytest.mark.parametrize("mode,k,kept", [
    ("max", 0, [(), (), (), (), (), ()]),
    ("max", 1, [(0,), (1,), (1,), (1,), (4,), (4,)]),                       # the tie does not replace the file it ties with
    ("max", 2, [(0,), (0, 1), (1, 2), (1, 2), (2, 4), (2, 4)]),             # 0.6 does not beat the worst kept (0.7); of the tied, the older leaves
    ("max", -1, [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5)]),
    ("min", 1, [(0,), (0,), (0,), (0,), (0,), (5,)]),
    ("min", 2, [(0,), (0, 1), (0, 1), (0, 3), (0, 3), (0, 5)]),             # the tie (0.7 against the worst kept 0.7) is not saved
])
def test_the_policy_decides_which_files_exist(tmp_path, mode, k, kept):
    cb, seen = files_after_each(tmp_path, SCORES, mode=mode, save_top_k=k, save_last=True)
    assert seen == [names(*epochs) for epochs in kept]
    for name in seen[-1]:
        assert "state_dict" in torch.load(tmp_path / "ck" / name, map_location="cpu", weights_only=True)
    last = torch.load(tmp_path / "ck" / "last.ckpt", map_location="cpu", weights_only=True)
    assert last["epoch"] == 5 and last["vibravox_amd"]["train_step"] == 18       # the newest state, also when its own file was not kept
    if k:
        best = {"max": 4, "min": 5}[mode]
        assert cb.best_model_path == str(tmp_path / "ck" / f"epoch_{best:03d}.ckpt") and cb.best_model_score == SCORES[best]
        assert last["callbacks"]["ModelCheckpoint"]["best_model_path"] == cb.best_model_path


def test_policy_without_last_without_monitor_and_name_versions(tmp_path):
    _, seen = files_after_each(tmp_path / "a", SCORES[:3], mode="max", save_top_k=1, save_last=False)
    assert seen == [names(0, last=False), names(1, last=False), names(1, last=False)]
    cb = F.ModelCheckpoint(monitor=None, save_top_k=1, save_last=True, dirpath=str(tmp_path / "b"), filename="epoch_{epoch:03d}-{step}")
    clock, module = Clock(), Tiny()
    for clock.global_step in (3, 6):
        cb.save(clock, module, {})
        cb.drain()
    assert sorted(os.listdir(tmp_path / "b")) == ["epoch_000-6.ckpt", "last.ckpt"]      # no monitor: the newest replaces the one before
    cb = F.ModelCheckpoint(monitor="m", mode="max", save_top_k=-1, dirpath=str(tmp_path / "c"), filename="e{epoch}_{m:.2f}")
    for score in (0.25, 0.25):
        cb.save(clock, module, {"m": score})
    cb.save(clock, module, {"other": 1.0})                                              # no value for the monitor, no last: nothing to write
    cb.drain()
    assert sorted(os.listdir(tmp_path / "c")) == ["e0_0.25-v1.ckpt", "e0_0.25.ckpt"]    # a taken name gets a version
    with pytest.raises(ValueError):
        F.ModelCheckpoint(monitor=None, save_top_k=2)
    with pytest.raises(ValueError):
        F.ModelCheckpoint(mode="best")


def test_last_is_a_link_where_the_filesystem_allows_it_else_a_copy(tmp_path, monkeypatch):
    src = tmp_path / "a.ckpt"
    torch.save({"x": torch.arange(3)}, src)
    how = F.ModelCheckpoint.link_or_copy(str(src), str(tmp_path / "last.ckpt"))
    assert how in ("link", "copy") and (how == "copy" or os.path.samefile(src, tmp_path / "last.ckpt"))

    def refuse(*a, **k):
        raise OSError("no hard links here")
    monkeypatch.setattr(os, "link", refuse)
    assert F.ModelCheckpoint.link_or_copy(str(src), str(tmp_path / "last2.ckpt"), {"x": torch.arange(3)}) == "copy"
    assert not os.path.samefile(src, tmp_path / "last2.ckpt")
    assert torch.equal(torch.load(tmp_path / "last2.ckpt", weights_only=True)["x"], torch.arange(3))
    assert F.ModelCheckpoint.link_or_copy(str(src), str(tmp_path / "last.ckpt")) == "copy"          # over an existing link, from the file
    assert (tmp_path / "last.ckpt").read_bytes() == src.read_bytes() and sorted(os.listdir(tmp_path)) == ["a.ckpt", "last.ckpt", "last2.ckpt"]
    _, seen = files_after_each(tmp_path / "run", [0.1, 0.2], mode="max", save_top_k=1, save_last=True)
    assert seen == [names(0), names(1)]


def test_a_non_finite_state_is_refused_and_the_files_stay(tmp_path):
    cb = F.ModelCheckpoint(monitor=None, save_top_k=1, save_last=True, dirpath=str(tmp_path), filename="e{epoch}")
    clock, module = Clock(), Tiny()
    cb.save(clock, module, {})
    cb.drain()
    before = {n: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path)}
    assert sorted(before) == ["e0.ckpt", "last.ckpt"]
    with torch.no_grad():
        module.generator.bias[1] = float("nan")
    clock.current_epoch = 1
    taken = cb.save(clock, module, {})
    assert taken is not None and taken.nonfinite() == [("state_dict.generator.bias", 1)]     # the snapshot is still the caller's
    with pytest.raises(F.NonFiniteError, match="state_dict.generator.bias"):
        cb.drain()
    assert {n: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path)} == before


# ---- CSVLogger --------------------------------------------------------------------------------------------------------------------------
def test_csv_logger_rows(tmp_path):
    log = F.CSVLogger(str(tmp_path / "csv"))
    log.log_metrics({"train/generator/adv_loss_gen": torch.tensor(0.1), "train/generator/backprop_loss": 2.5}, step=1, epoch=0)
    log.log_metrics({"validation/torchmetrics_stoi": 1 / 3}, step=3, epoch=0)
    log.log_metrics({"train/generator/backprop_loss": 1e-30}, step=4, epoch=1)
    log.save()
    with open(tmp_path / "csv" / "metrics.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["epoch", "step", "train/generator/adv_loss_gen", "train/generator/backprop_loss", "validation/torchmetrics_stoi"]
    assert rows[1:] == [["0", "1", repr(float(torch.tensor(0.1))), "2.5", ""], ["0", "3", "", "", repr(1 / 3)], ["1", "4", "", "1e-30", ""]]
    assert float(rows[2][4]) == 1 / 3 and os.listdir(tmp_path / "csv") == ["metrics.csv"]


# ---- run.compose ------------------------------------------------------------------------------------------------------------------------
def test_compose_adds_the_callbacks_and_logging_groups():
    import run

    plain = run.compose([])
    assert set(plain) == {"sample_rate", "description", "lightning_datamodule", "lightning_module", "trainer"}
    assert plain["trainer"] == {"accelerator": "gpu", "devices": 1, "max_steps": 10, "log_every_n_steps": 1, "precision": "32-true"}
    assert not run.fit_requested(plain) and not run.fit_requested(run.compose(["++trainer.max_steps=20"]))
    cfg = run.compose(["+callbacks=bwe_checkpoint", "+logging=csv", "trainer.max_epochs=2"])
    assert {k: v for k, v in cfg.items() if k not in ("callbacks", "logging", "trainer")} == {k: v for k, v in plain.items() if k != "trainer"}
    assert cfg["trainer"] == dict(plain["trainer"], max_epochs=2) and run.fit_requested(cfg)
    assert cfg["callbacks"] == {"checkpoint": {
        "_target_": "vibravox_amd.fit.ModelCheckpoint", "monitor": "validation/torchmetrics_stoi", "mode": "max", "save_top_k": 2, "save_last": True,
        "verbose": False, "dirpath": "checkpoints/", "filename": "epoch_{epoch:03d}", "auto_insert_metric_name": False, "save_weights_only": False}}
    assert cfg["logging"] == {"log_every_n_steps": 100, "logger": {"_target_": "vibravox_amd.fit.CSVLogger", "save_dir": "csv/"}}
    cb = run.instantiate(cfg["callbacks"])["checkpoint"]
    assert isinstance(cb, F.ModelCheckpoint) and (cb.monitor, cb.mode, cb.save_top_k, cb.save_last) == ("validation/torchmetrics_stoi", "max", 2, True)
    assert isinstance(run.instantiate(cfg["logging"]["logger"]), F.CSVLogger)
    for extra in (["+ckpt_path=checkpoints/last.ckpt"], ["trainer.limit_train_batches=5"], ["trainer.check_val_every_n_epoch=2"]):
        assert run.fit_requested(run.compose(extra))
    assert run.compose(["+ckpt_path=checkpoints/last.ckpt"])["ckpt_path"] == "checkpoints/last.ckpt"
    with pytest.raises(KeyError):
        run.compose(["trainer.no_such_key=1"])


# ---- interrupted and resumed fit ----------------------------------------------------------------------------------------------------------
class Record:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step, epoch):
        self.rows.append((epoch, step, dict(metrics)))


class StopAt:
    def __init__(self, step):
        self.step = step

    def on_train_batch_end(self, trainer, module):
        if trainer.global_step == self.step:
            trainer.should_stop = True


class StubDataModule:
    def __init__(self):
        self.data = StubData()

    def train_dataloader(self):
        return self.data.train_dataloader()


def test_a_resumed_fit_ends_where_the_uninterrupted_one_ends(tmp_path):
    whole, log_whole = stub(1), Record()
    torch.manual_seed(87)
    F.Trainer(max_epochs=2, log_every_n_steps=1, logger=log_whole).fit(whole, StubDataModule())
    rng_at_the_end = torch.get_rng_state()
    assert [(e, s) for e, s, _ in log_whole.rows] == [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5), (1, 6)]
    assert len({tuple(sorted(m)) for _, _, m in log_whole.rows}) == 2     # steps with and without the discriminator update (ratio 0.5)

    first, log_first = stub(1), Record()
    policy = dict(monitor="validation/torchmetrics_stoi", mode="max", save_top_k=2, save_last=True, dirpath=str(tmp_path / "ck"),
                  filename="epoch_{epoch:03d}", every_n_train_steps=3)
    torch.manual_seed(87)
    F.Trainer(max_epochs=2, log_every_n_steps=1, logger=log_first, callbacks=[F.ModelCheckpoint(**policy), StopAt(3)]).fit(first, StubDataModule())
    assert log_first.rows == log_whole.rows[:3]
    assert os.listdir(tmp_path / "ck") == ["last.ckpt"]                   # no validation data: monitoring is off, only save_last applies
    saved = C.load_file(str(tmp_path / "ck" / "last.ckpt"))["vibravox_amd"]
    assert (saved["train_step"], saved["loader_epoch"], saved["batches_served"]) == (3, 0, 3)

    second, log_second, dm = stub(2), Record(), StubDataModule()
    torch.manual_seed(4321)                                                # the restored RNG state replaces this one
    trainer = F.Trainer(max_epochs=2, log_every_n_steps=1, logger=log_second, callbacks=[F.ModelCheckpoint(**policy)])
    trainer.fit(second, dm, ckpt_path=str(tmp_path / "ck" / "last.ckpt"))
    assert dm.data.built == 3 and trainer.global_step == 6 and trainer.current_epoch == 2      # the served batches were not built again
    assert log_second.rows == log_whole.rows[3:]                          # every logged value of steps 4 to 6, as floats: bit for bit
    assert_same_state(whole, second)
    assert torch.equal(torch.get_rng_state(), rng_at_the_end)
    last = C.load_file(str(tmp_path / "ck" / "last.ckpt"))
    assert (last["epoch"], last["vibravox_amd"]["train_step"], last["vibravox_amd"]["loader_epoch"], last["vibravox_amd"]["batches_served"]) == (1, 6, 2, 0)


def test_a_fit_resumed_inside_an_epoch_skips_without_building(tmp_path):
    whole, log_whole = stub(1), Record()
    torch.manual_seed(87)
    F.Trainer(max_epochs=2, log_every_n_steps=1, logger=log_whole).fit(whole, StubDataModule())
    policy = dict(monitor=None, save_top_k=1, save_last=True, dirpath=str(tmp_path), filename="s{step}", every_n_train_steps=2)
    first = stub(1)   # (seeds the global generator for its initialisation: before the run's own seed)
    torch.manual_seed(87)
    F.Trainer(max_epochs=2, callbacks=[F.ModelCheckpoint(**policy), StopAt(4)]).fit(first, StubDataModule())
    assert sorted(os.listdir(tmp_path)) == ["last.ckpt", "s4.ckpt"]
    second, log_second, dm = stub(2), Record(), StubDataModule()
    F.Trainer(max_epochs=2, log_every_n_steps=1, logger=log_second).fit(second, dm, ckpt_path=str(tmp_path / "s4.ckpt"))
    assert dm.data.built == 2 and log_second.rows == log_whole.rows[4:]
    assert_same_state(whole, second)
