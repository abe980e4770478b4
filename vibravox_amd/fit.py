"""The fit loop around ``EBENLightningModule``: epochs, validation, checkpoints, exact resume, test.

What the reference gets from Lightning's ``Trainer.fit`` / ``Trainer.test``, ``ModelCheckpoint`` and ``CSVLogger`` for the keys its
configs use (``configs/callbacks/bwe_checkpoint.yaml``, ``configs/logging/csv.yaml``, ``configs/trainer``), on this project's own
pieces: the train step, the resident datamodules, ``evaluate_clips`` and ``checkpoint.Snapshot``.  Nothing here needs a GPU: with a
module on the CPU the same loop runs on ``checkpoint.assemble_host``.

Data-parallel runs: with ``WORLD_SIZE`` > 1 only rank 0 takes snapshots and writes files.  No multi-rank run of this loop was possible
where it was written: that rule is untested on hardware.
"""
from __future__ import annotations

import concurrent.futures
import csv
import itertools
import os
import re
from typing import Dict, List, Optional

import torch

from . import checkpoint as C


class NonFiniteError(RuntimeError):
    """A snapshot holds an infinity or a NaN: the checkpoint is not written."""


def _rank() -> int:
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank()
    return int(os.environ.get("RANK", 0))


# ---- checkpoint policy --------------------------------------------------------------------------------------------------------------------
class ModelCheckpoint:
    """Lightning's ``ModelCheckpoint`` for the reference's keys.  Which files exist after a save is host bookkeeping (``decide``); the
    snapshot, the write, the ``last.ckpt`` link and the deletions run on one writer thread, in order, while the device trains on.

    ``filename`` is formatted as Lightning does with ``auto_insert_metric_name=False``: ``{epoch:03d}``, ``{step}`` and
    ``{<logged name>:fmt}`` are replaced by their values; a name that is taken gets ``-v1``, ``-v2``, ...  ``monitor`` is looked up in the
    validation's logged values, also under ``<monitor>/<first dataloader name>`` when the module suffixes them.  A save that finds no
    value for ``monitor`` -- a step-triggered one before the first validation, a datamodule without validation data -- keeps
    ``last.ckpt`` only."""

    def __init__(self, monitor: Optional[str] = None, mode: str = "min", save_top_k: int = 1, save_last: Optional[bool] = None,
                 dirpath: str = "checkpoints/", filename: Optional[str] = None, every_n_train_steps: Optional[int] = None,
                 save_weights_only: bool = False, verbose: bool = False, auto_insert_metric_name: bool = False):
        if mode not in ("min", "max"):
            raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
        if save_top_k < -1:
            raise ValueError(f"save_top_k must be -1 (all), 0 (none) or a count, got {save_top_k}")
        if monitor is None and save_top_k not in (-1, 0, 1):
            raise ValueError(f"save_top_k={save_top_k} needs a monitor")
        if auto_insert_metric_name:
            raise NotImplementedError("auto_insert_metric_name=True is not offered (the reference sets False)")
        self.monitor, self.mode, self.save_top_k, self.save_last = monitor, mode, int(save_top_k), bool(save_last)
        self.dirpath, self.filename = dirpath, filename or "epoch_{epoch:03d}-step_{step}"
        self.every_n_train_steps, self.save_weights_only, self.verbose = every_n_train_steps, save_weights_only, verbose
        self.best_k_models: Dict[str, float] = {}   # path -> score, in the order they were saved
        self.best_model_path, self.best_model_score, self.last_model_path = "", None, ""
        self.snapshot = C.Snapshot()
        self._pool: Optional[concurrent.futures.ThreadPoolExecutor] = None
        self._jobs: List[concurrent.futures.Future] = []
        self._failed = False

    # -- bookkeeping (host only, no file touched) ----------------------------------------------------------------------------------------
    def format_name(self, metrics: Dict[str, float], epoch: int, step: int) -> str:
        values = dict(metrics, epoch=epoch, step=step)

        def sub(m):
            value = values.get(m.group(1), 0)
            return format(value, m.group(2)[1:]) if m.group(2) else str(value)
        name = re.sub(r"\{([^{}:]+)(:[^{}]*)?\}", sub, self.filename)
        base, version = os.path.join(self.dirpath, name), 0
        path = base + ".ckpt"
        while path in self.best_k_models or os.path.exists(path):
            version += 1
            path = f"{base}-v{version}.ckpt"
        return path

    def score_of(self, metrics: Dict[str, float]) -> Optional[float]:
        if self.monitor is None:
            return None
        key = self.monitor if self.monitor in metrics else next((k for k in metrics if k.startswith(self.monitor + "/")), None)
        if key is None:
            return None
        s = float(metrics[key])
        return s if s == s else (float("-inf") if self.mode == "max" else float("inf"))   # a NaN is the worst score there is

    def decide(self, path: str, score: Optional[float]):
        """Records a save of ``path`` with ``score`` and returns ``(write, delete)``: whether the file is written and the files that leave.
        A score enters the top ``save_top_k`` only when it beats the worst one kept (a tie does not); the one that leaves is the worst,
        the oldest among equals."""
        k = self.save_top_k
        if k == 0:
            return False, []
        if self.monitor is None:   # no ranking: every save is kept (-1) or replaces the one before (1)
            delete = list(self.best_k_models) if k == 1 else []
            if k == 1:
                self.best_k_models.clear()
            self.best_k_models[path] = float("nan")
            self.best_model_path = path
            return True, delete
        if score is None:
            return False, []
        better = (lambda a, b: a > b) if self.mode == "max" else (lambda a, b: a < b)
        worst = (min if self.mode == "max" else max)
        if k != -1 and len(self.best_k_models) >= k:
            kth = worst(self.best_k_models, key=self.best_k_models.get)
            if not better(score, self.best_k_models[kth]):
                return False, []
        self.best_k_models[path] = score
        delete = []
        if k != -1 and len(self.best_k_models) > k:
            kth = worst(self.best_k_models, key=self.best_k_models.get)
            del self.best_k_models[kth]
            delete.append(kth)
        best = (max if self.mode == "max" else min)(self.best_k_models, key=self.best_k_models.get)
        self.best_model_path, self.best_model_score = best, self.best_k_models[best]
        return True, delete

    def state_dict(self) -> dict:
        return {"monitor": self.monitor, "best_model_score": self.best_model_score, "best_model_path": self.best_model_path,
                "best_k_models": dict(self.best_k_models), "last_model_path": self.last_model_path, "dirpath": self.dirpath}

    def load_state_dict(self, state: dict) -> None:
        if os.path.abspath(state.get("dirpath", self.dirpath)) != os.path.abspath(self.dirpath):
            return   # another directory: its files are not this run's to rank or delete
        self.best_k_models = {p: float(s) for p, s in state.get("best_k_models", {}).items() if os.path.exists(p)}
        self.best_model_path, self.best_model_score = state.get("best_model_path", ""), state.get("best_model_score")
        self.last_model_path = state.get("last_model_path", "")

    # -- files ---------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def link_or_copy(src: str, dst: str, ckpt: Optional[dict] = None) -> str:
        """``dst`` becomes a hard link to ``src`` where the filesystem allows it ("link"), else a second write ("copy")."""
        tmp = dst + ".tmp"
        if os.path.exists(tmp):
            os.remove(tmp)
        try:
            os.link(src, tmp)
            how = "link"
        except OSError:
            if ckpt is not None:
                torch.save(ckpt, tmp)
            else:
                import shutil
                shutil.copyfile(src, tmp)
            how = "copy"
        os.replace(tmp, dst)
        return how

    def _write(self, taken: C.Taken, path: Optional[str], last: Optional[str], delete: List[str], callbacks: dict) -> None:
        if self._failed:
            return   # a save before this one was refused: nothing is written or deleted behind it
        try:
            bad = taken.nonfinite()
            if bad:
                name, count = bad[0]
                raise NonFiniteError(f"checkpoint refused: {name} holds {count} non-finite value{'s' if count != 1 else ''}"
                                     f"{f' (and {len(bad) - 1} more tensors do)' if len(bad) > 1 else ''}; the files on disk stay as they were")
            ckpt = taken.checkpoint(callbacks, self.save_weights_only)
            if path is not None:
                C.write_file(ckpt, path)
            if last is not None:
                if path is not None:
                    self.link_or_copy(path, last, ckpt)
                else:
                    C.write_file(ckpt, last)
            for p in delete:
                if os.path.exists(p):
                    os.remove(p)
        except BaseException:
            self._failed = True
            raise

    def save(self, trainer: "Trainer", module, metrics: Dict[str, float]) -> Optional[C.Taken]:
        """One save under the policy; returns the snapshot (also when nothing will be written from it is decided later, on the writer
        thread), or None when the policy asks for no file at all."""
        if _rank() != 0:
            return None
        path = self.format_name(metrics, trainer.current_epoch, trainer.global_step)
        write, delete = self.decide(path, self.score_of(metrics))
        last = os.path.join(self.dirpath, "last.ckpt") if self.save_last else None
        if not write and last is None:
            return None
        if last is not None:
            self.last_model_path = last
        self.check()   # a refusal of an earlier save surfaces here at the latest
        taken = self.snapshot.take(C.TrainState.of(module, trainer.counters()))
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="checkpoint-writer")
        callbacks = {"ModelCheckpoint": self.state_dict()}
        job = self._pool.submit(self._write, taken, path if write else None, last, delete, callbacks)
        self.snapshot.reading(taken, job)
        self._jobs.append(job)
        return taken

    def check(self) -> None:
        """Raises what a finished write raised."""
        pending = []
        for job in self._jobs:
            if job.done():
                job.result()
            else:
                pending.append(job)
        self._jobs = pending

    def drain(self) -> None:
        """Waits for every write; raises the first error among them."""
        jobs, self._jobs = self._jobs, []
        try:
            for job in jobs:
                job.result()
        finally:
            concurrent.futures.wait(jobs)
            self._failed = False

    # -- the loop's hooks ----------------------------------------------------------------------------------------------------------------
    def on_train_batch_end(self, trainer: "Trainer", module) -> None:
        n = self.every_n_train_steps
        if n and trainer.global_step % n == 0:
            self.save(trainer, module, {})

    def on_validation_end(self, trainer: "Trainer", module) -> None:
        self.save(trainer, module, trainer.callback_metrics)

    def on_train_epoch_end(self, trainer: "Trainer", module) -> None:
        if not trainer.validated_this_epoch:
            self.save(trainer, module, {})

    def on_fit_end(self, trainer: "Trainer", module) -> None:
        self.drain()


# ---- logging ----------------------------------------------------------------------------------------------------------------------------
class CSVLogger:
    """``save_dir/metrics.csv``: one row per logging event, ``epoch`` and ``step`` first, then every name ever logged in sorted order (a
    name an event did not log stays empty).  Values are written with ``repr``: they read back as the floats they were."""

    def __init__(self, save_dir: str = "csv/"):
        self.save_dir = save_dir
        self.rows: List[Dict[str, float]] = []

    @property
    def path(self) -> str:
        return os.path.join(self.save_dir, "metrics.csv")

    def log_metrics(self, metrics: Dict[str, float], step: int, epoch: int) -> None:
        self.rows.append(dict({k: float(v) for k, v in metrics.items()}, epoch=int(epoch), step=int(step)))

    def save(self) -> None:
        if _rank() != 0:
            return
        names = ["epoch", "step"] + sorted({k for row in self.rows for k in row} - {"epoch", "step"})
        os.makedirs(self.save_dir, exist_ok=True)
        tmp = self.path + ".tmp"
        with open(tmp, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(names)
            for row in self.rows:
                w.writerow([repr(row[k]) if k in row else "" for k in names])
        os.replace(tmp, self.path)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def _limit(n: int, limit) -> int:
    """Lightning's ``limit_*_batches``: None all, an int that many, a float that fraction."""
    if limit is None:
        return n
    if isinstance(limit, float):
        return min(n, int(n * limit))
    return min(n, int(limit))


class Trainer:
    """``fit`` / ``test`` for the subset of Lightning's ``Trainer`` arguments the reference's configs use.  Callbacks are objects with any
    of ``on_train_batch_end``, ``on_validation_end``, ``on_train_epoch_end``, ``on_fit_end`` ``(trainer, module)``; setting
    ``trainer.should_stop`` in one ends the fit behind the current step, before anything else of its epoch.  ``logger``: an object with
    ``log_metrics(metrics, step, epoch)`` and optionally ``save()``."""

    def __init__(self, max_epochs: Optional[int] = None, max_steps: int = -1, check_val_every_n_epoch: int = 1, limit_train_batches=None,
                 limit_val_batches=None, log_every_n_steps: int = 50, precision=None, callbacks=None, logger=None, freeze_gc: bool = False):
        self.max_epochs, self.max_steps = max_epochs, -1 if max_steps is None else int(max_steps)
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.limit_train_batches, self.limit_val_batches = limit_train_batches, limit_val_batches
        self.log_every_n_steps, self.precision = max(1, int(log_every_n_steps)), precision
        self.callbacks = list(callbacks.values()) if isinstance(callbacks, dict) else list(callbacks or [])
        self.logger, self.freeze_gc = logger, freeze_gc
        self.current_epoch = 0        # the epoch in progress (the one just finished, in the hooks behind it)
        self.global_step = 0          # training steps taken
        self.batches_served = 0       # of the epoch in progress
        self.should_stop = False
        self.validated_this_epoch = False
        self.callback_metrics: Dict[str, float] = {}
        self.datamodule = None
        self._epoch_done = False

    @property
    def checkpoint_callback(self) -> Optional[ModelCheckpoint]:
        return next((c for c in self.callbacks if isinstance(c, ModelCheckpoint)), None)

    def counters(self) -> Dict[str, int]:
        """Where a continuation picks up: behind a finished epoch at batch 0 of the next one."""
        done = self._epoch_done
        return {"epoch": self.current_epoch, "train_step": self.global_step, "loader_epoch": self.current_epoch + (1 if done else 0),
                "batches_served": 0 if done else self.batches_served}

    def _call(self, hook: str, module) -> None:
        for c in self.callbacks:
            fn = getattr(c, hook, None)
            if fn is not None:
                fn(self, module)

    def _log(self, metrics: Dict[str, float]) -> None:
        if self.logger is not None and metrics:
            self.logger.log_metrics(metrics, self.global_step, self.current_epoch)

    @staticmethod
    def _logged(module, prefix: str) -> Dict[str, float]:
        return {k: float(v) for k, v in module.logged.items() if k.startswith(prefix)}

    # -- validation ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def validate(self, module, datamodule) -> Dict[str, float]:
        """The validation split's logged values.  Whole splits through ``evaluate_clips`` where the datamodule has ``val_clips`` (both
        roots with ``root_secondary``), else ``validation_step`` + ``common_eval_logging`` over ``val_dataloader()`` with every value
        averaged over its batches; {} when the datamodule has neither.  Runs under ``eval()`` and ``no_grad``."""
        has_clips, has_loader = hasattr(datamodule, "val_clips"), hasattr(datamodule, "val_dataloader")
        if not has_clips and not has_loader:
            return {}
        was_training = module.training
        module.eval()
        kept = dict(module.logged)
        module.logged.clear()
        for metric in getattr(module, "metrics", {}).values():
            if hasattr(metric, "reset"):
                metric.reset()
        try:
            if has_clips:
                whichs = ["principal", "secondary"] if getattr(datamodule, "root_secondary", None) is not None else ["principal"]
                module.dataloader_names = whichs if len(whichs) > 1 else None   # on_fit_start: the keys of a dict of loaders
                for idx, which in enumerate(whichs):
                    corrupted, reference = datamodule.val_clips(which)
                    n = _limit(len(corrupted), self.limit_val_batches)
                    module.evaluate_clips(corrupted[:n], reference[:n], stage="validation", dataloader_idx=idx)
                out = self._logged(module, "validation/")
            else:
                loaders = datamodule.val_dataloader()
                module.dataloader_names = list(loaders) if isinstance(loaders, dict) else None
                sums: Dict[str, List[float]] = {}
                for idx, loader in enumerate(loaders.values() if isinstance(loaders, dict) else [loaders]):
                    n = _limit(len(loader), self.limit_val_batches) if hasattr(loader, "__len__") else self.limit_val_batches
                    for i, batch in enumerate(itertools.islice(loader, n)):
                        module.logged.clear()
                        outputs = module.validation_step(batch, i, idx)
                        module.on_validation_batch_end(outputs, batch, i, idx)
                        for k, v in self._logged(module, "validation/").items():
                            sums.setdefault(k, []).append(v)
                out = {k: sum(v) / len(v) for k, v in sums.items()}
        finally:
            module.logged.clear()
            module.logged.update(kept)
            module.train(was_training)
        return out

    # -- fit -----------------------------------------------------------------------------------------------------------------------------
    def _epoch_batches(self, loader, epoch: int, skip: int):
        """(number of batches of the epoch, iterator over those behind the first ``skip``).  A loader with ``plan`` / ``make_batch``
        (``ResidentLoader``) skips without building; an endless generator counts ``limit_train_batches`` as an epoch."""
        if hasattr(loader, "__next__"):
            if self.limit_train_batches is None:
                raise ValueError("an endless train loader needs trainer.limit_train_batches: the length of an epoch")
            n = int(self.limit_train_batches)
            return n, itertools.islice(loader, max(0, n - skip))
        if hasattr(loader, "plan") and hasattr(loader, "make_batch"):
            plan = loader.plan(epoch)
            n = _limit(len(plan), self.limit_train_batches)
            loader.epoch = epoch + 1   # what iter() would have left
            return n, (loader.make_batch(indices) for indices in plan[skip:n])
        n = _limit(len(loader), self.limit_train_batches)
        return n, itertools.islice(iter(loader), skip, n)

    def fit(self, module, datamodule, ckpt_path: Optional[str] = None) -> None:
        self.datamodule, module.trainer = datamodule, self
        if self.precision is not None and hasattr(module, "set_precision"):
            module.set_precision(self.precision)
        if hasattr(datamodule, "setup"):
            datamodule.setup("fit")
        self.should_stop = False
        skip = 0
        if ckpt_path is not None:
            report = C.restore(module, ckpt_path)
            self.current_epoch, self.global_step, skip = report["loader_epoch"], report["train_step"], report["batches_served"]
            state = report["callbacks"].get("ModelCheckpoint")
            if state and self.checkpoint_callback is not None:
                self.checkpoint_callback.load_state_dict(state)
        loader = datamodule.train_dataloader()
        module.train()
        try:
            while not self._finished():
                self._epoch_done, self.validated_this_epoch = False, False
                n, batches = self._epoch_batches(loader, self.current_epoch, skip)
                self.batches_served, skip = min(skip, n), 0
                for batch in batches:
                    if self.freeze_gc and self.global_step == 3:   # set-up and warm-up objects are long-lived: keep the cyclic GC off them
                        import gc
                        gc.collect()
                        gc.freeze()
                    module.logged.clear()
                    module.training_step(batch, self.batches_served)
                    self.global_step += 1
                    self.batches_served += 1
                    if self.global_step % self.log_every_n_steps == 0:
                        self._log(self._logged(module, "train/"))
                    self._call("on_train_batch_end", module)
                    if self.should_stop or (self.max_steps > 0 and self.global_step >= self.max_steps):
                        break
                if self.should_stop or self.batches_served < n:
                    break   # stopped inside the epoch: nothing of its end runs
                if n == 0:
                    raise RuntimeError("the train loader has no batch: fewer items than ranks, or than one batch with drop_last")
                self._epoch_done = True
                if (self.current_epoch + 1) % max(1, int(self.check_val_every_n_epoch)) == 0:
                    metrics = self.validate(module, datamodule)
                    if metrics:
                        self.callback_metrics, self.validated_this_epoch = metrics, True
                        self._log(metrics)
                        self._call("on_validation_end", module)
                self._call("on_train_epoch_end", module)
                if self.logger is not None and hasattr(self.logger, "save"):
                    self.logger.save()
                self.current_epoch += 1
                self._epoch_done = False
                self.batches_served = 0
        finally:
            try:
                self._call("on_fit_end", module)
            finally:
                if self.logger is not None and hasattr(self.logger, "save"):
                    self.logger.save()

    def _finished(self) -> bool:
        return (self.should_stop or (self.max_epochs is not None and self.max_epochs >= 0 and self.current_epoch >= self.max_epochs)
                or (self.max_steps > 0 and self.global_step >= self.max_steps)
                or (self.max_epochs is None and self.max_steps <= 0 and self.current_epoch >= 1000))   # Lightning's default of 1000 epochs

    # -- test ----------------------------------------------------------------------------------------------------------------------------
    def _resolve(self, ckpt_path: Optional[str]) -> Optional[str]:
        if ckpt_path in ("last", "best"):
            cb = self.checkpoint_callback
            if cb is None:
                raise ValueError(f"ckpt_path={ckpt_path!r} needs a ModelCheckpoint among the callbacks")
            path = cb.last_model_path or os.path.join(cb.dirpath, "last.ckpt") if ckpt_path == "last" else cb.best_model_path
            if not path or not os.path.exists(path):
                raise FileNotFoundError(f"ckpt_path={ckpt_path!r}: no such checkpoint ({path or 'none was saved'})")
            return path
        return ckpt_path

    @torch.no_grad()
    def test(self, module, datamodule, ckpt_path: Optional[str] = "last") -> Dict[str, float]:
        """Restores the named checkpoint (None: the module as it is) and scores the test split: ``evaluate_clips(*dm.test_clips(),
        losses=True)``, the content of the reference's ``test_step`` over the split; then ``on_test_end``.  Returns the logged values."""
        self.datamodule, module.trainer = datamodule, self
        cb = self.checkpoint_callback
        if cb is not None:
            cb.drain()
        path = self._resolve(ckpt_path)
        if path is not None:
            C.restore(module, path)
        if hasattr(datamodule, "setup"):
            datamodule.setup("test")
        was_training = module.training
        module.eval()
        module.logged.clear()
        whichs = ["principal", "secondary"] if getattr(datamodule, "root_secondary", None) is not None else ["principal"]
        module.dataloader_names = whichs if len(whichs) > 1 else None
        for idx, which in enumerate(whichs):
            module.evaluate_clips(*datamodule.test_clips(which), stage="test", dataloader_idx=idx, losses=True)
        out = self._logged(module, "test/")
        module.train(was_training)
        self._log(out)
        if self.logger is not None and hasattr(self.logger, "save"):
            self.logger.save()
        module.on_test_end()
        return out
