"""Constructor / logging contract of ``vibravox/lightning_modules/base_se.py:16-196`` that the EBEN
train step relies on, plus the speech-quality half of the reference's evaluation hooks:
``on_validation_batch_end`` / ``on_test_batch_end`` -> ``common_eval_logging`` log
``{stage}/torchmetrics_si_sdr[/dataloader]`` and ``{stage}/torchmetrics_stoi[/dataloader]`` for every batch with a
reference, computed at 16 kHz on the device (``vibravox_amd.metrics``: HIP kernels, no host round trip).  Still out of
scope: the model-based scores ``noresqa_mos`` and ``torchsquim_stoi`` (they need downloaded
weights, so batches without a reference log nothing here) and the audio logging.

Lightning is optional: when ``lightning`` is importable the class is a real ``LightningModule``
(so ``run.py lightning_module=eben`` drives it through ``Trainer.fit``); otherwise a small
stand-in implements the five methods ``training_step`` calls (``optimizers``, ``toggle_optimizer``,
``untoggle_optimizer``, ``manual_backward``, ``log``) with Lightning's semantics.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from ..metrics import ScaleInvariantSignalDistortionRatio, ShortTimeObjectiveIntelligibility

try:  # pragma: no cover - not installed in the build image
    from lightning import LightningModule as _Base

    HAVE_LIGHTNING = True
except Exception:
    HAVE_LIGHTNING = False

    class _Base(torch.nn.Module):  # type: ignore
        """Lightning-free stand-in for the subset of LightningModule used by the EBEN step."""

        def __init__(self):
            super().__init__()
            self.automatic_optimization = True
            self.logged: Dict[str, torch.Tensor] = {}
            self._optimizers = None
            self._toggled: Dict[int, List[bool]] = {}
            self.grad_sync = {}  # optimizer id -> vibravox_amd.ddp.GradSync (data-parallel runs)
            self._sync_pending: List[str] = []

        def optimizers(self, use_pl_optimizer: bool = True):
            if self._optimizers is None:
                self._optimizers = self.configure_optimizers()
            return self._optimizers

        def toggle_optimizer(self, optimizer):
            """requires_grad=False on every parameter not owned by `optimizer` (lightning semantics)."""
            owned = {id(p) for grp in optimizer.param_groups for p in grp["params"]}
            state = []
            for p in self.parameters():
                state.append((p, p.requires_grad))
                if id(p) not in owned:
                    p.requires_grad_(False)
            self._toggled[id(optimizer)] = state

        def untoggle_optimizer(self, optimizer):
            for p, req in self._toggled.pop(id(optimizer), []):
                p.requires_grad_(req)

        def manual_backward(self, loss, *args, **kwargs):
            loss.backward(*args, **kwargs)

        def log(self, name, value, sync_dist: bool = False, **kwargs):
            """``sync_dist=True`` (every train-step value, eben.py:103-124): Lightning reduces each value to the rank mean
            with a collective of its own -- 7 per step; here the names are queued and ``flush_logged`` reduces them
            together."""
            self.logged[name] = value.detach() if torch.is_tensor(value) else torch.as_tensor(value)
            if sync_dist and torch.distributed.is_available() and torch.distributed.is_initialized() \
                    and torch.distributed.get_world_size() > 1 and name not in self._sync_pending:
                self._sync_pending.append(name)

        def flush_logged(self) -> None:
            """ONE packed all-reduce(mean) for every value logged with ``sync_dist`` since the last flush (called at the end
            of ``training_step``: off the critical path, after the last gradient exchange has been issued)."""
            if self._sync_pending:
                from ..ddp import all_reduce_scalars

                names, self._sync_pending = self._sync_pending, []
                for n, v in zip(names, all_reduce_scalars([self.logged[n] for n in names])):
                    self.logged[n] = v


class BaseSELightningModule(_Base):
    def __init__(self, sample_rate: int, description: str = None):
        super().__init__()
        self.sample_rate = sample_rate
        self.description = description
        self.dataloader_names = None
        # base_se.py:38-45 (the two metrics that need no pretrained network); no parameters or buffers, so no state_dict keys
        self.metrics = torch.nn.ModuleDict(dict(torchmetrics_si_sdr=ScaleInvariantSignalDistortionRatio(),
                                                torchmetrics_stoi=ShortTimeObjectiveIntelligibility(fs=16000)))

    def _to_16k(self, x: torch.Tensor) -> torch.Tensor:
        """torchaudio ``Resample(sample_rate, 16000)`` of the reference (identity at 16 kHz)."""
        if int(self.sample_rate) == 16000:
            return x
        from ..augment import resample

        return resample(x.contiguous(), int(self.sample_rate), 16000)

    def _ragged_to_16k(self, enhanced: torch.Tensor, reference: torch.Tensor, lengths):
        """A padded batch whose row r is ``[..., :lengths[r]]`` (one length per row of the flattened leading dimensions), at 16 kHz:
        each row's resampling is the one the row alone gets.  The resampler's taps reach past a row's end, where the row alone is
        zero-padded, so what lies behind each row is zeroed first, on a copy.  At 16 kHz nothing is touched or read behind a row."""
        if int(self.sample_rate) == 16000:
            return enhanced, reference, lengths
        import math

        from .. import metrics
        from .._lib import check, load, ptr, stream

        if enhanced.shape != reference.shape or enhanced.dim() < 1:
            raise ValueError(f"common_eval_logging: enhanced {tuple(enhanced.shape)} and reference {tuple(reference.shape)} must have one shape")
        t = enhanced.shape[-1]
        lead = tuple(enhanced.shape[:-1])
        rows = math.prod(lead)
        host = metrics._host_lengths(lengths, rows, t, "common_eval_logging")
        lens = (host.to(enhanced.device, non_blocking=True) if host is not None
                else metrics._device_lengths(lengths, rows, lead, enhanced.device, "common_eval_logging"))
        out = []
        for x in (enhanced, reference):
            x = x.detach().to(torch.float32).reshape(rows, 1, t).clone(memory_format=torch.contiguous_format)
            check(load().eben_edge_zero(ptr(x), lens.data_ptr(), rows, 1, t, stream()), "edge_zero")
            out.append(self._to_16k(x.reshape(lead + (t,))))
        g = math.gcd(int(self.sample_rate), 16000)
        orig, new = int(self.sample_rate) // g, 16000 // g
        lens16 = ((lens.to(torch.int64) * new + (orig - 1)) // orig).to(torch.int32)   # augment.resample's length of the row alone
        lens16 = torch.where((lens >= 1) & (lens <= t), lens16, torch.zeros_like(lens16))   # an out-of-range row stays out of range: NaN
        return out[0], out[1], lens16

    def common_eval_logging(self, stage: str, outputs, batch_idx: int, dataloader_idx: int = 0) -> None:
        """base_se.py:67-130: with a reference, SI-SDR and STOI of the enhanced speech at 16 kHz, batch means logged as
        ``{stage}/torchmetrics_si_sdr{suffix}`` and ``{stage}/torchmetrics_stoi{suffix}`` (the metric objects also accumulate,
        as torchmetrics' forward does).  Without a reference the reference logs only model-based scores, which are out of
        scope: nothing is logged.  ``outputs["lengths"]`` (optional, as ``metrics.si_sdr`` takes it) makes the batch a padded one:
        row r is scored on its first ``lengths[r]`` samples alone."""
        if "reference" not in outputs:
            return
        names = getattr(self, "dataloader_names", None)
        suffix = f"/{names[dataloader_idx]}" if names is not None else ""
        lengths = outputs.get("lengths")
        if lengths is None:
            enhanced, reference = self._to_16k(outputs["enhanced"]), self._to_16k(outputs["reference"])
        else:
            enhanced, reference, lengths = self._ragged_to_16k(outputs["enhanced"], outputs["reference"], lengths)
        for key, metric in self.metrics.items():
            self.log(f"{stage}/{key}{suffix}", metric(enhanced, reference, lengths=lengths), sync_dist=True, prog_bar=True,
                     add_dataloader_idx=False)

    def on_validation_batch_end(self, outputs, batch, batch_idx: int, dataloader_idx: int = 0) -> None:
        self.common_eval_logging("validation", outputs, batch_idx, dataloader_idx)

    def on_test_batch_end(self, outputs, batch, batch_idx: int, dataloader_idx: int = 0) -> None:
        self.common_eval_logging("test", outputs, batch_idx, dataloader_idx)
