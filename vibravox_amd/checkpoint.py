"""The training state as one byte image: snapshots that do not stop the step, checkpoint files, restores in place.

A run's state is several hundred tensors -- the modules' parameters and buffers and two Adam moments per trained parameter.
``Snapshot.take`` gathers them on the device into one image with one launch per 48 tensors (``eben_pack_tensors``, csrc/snapshot.hip),
queues one copy of the image to pinned memory behind it and returns; a writer thread waits for the copy's event and ``torch.save``s a
dict whose tensors are views into that pinned image, while the device goes on training.  ``restore`` goes the other way
(``eben_unpack_tensors``) into the parameter and moment storages that exist, so replayed graphs and cached pointer tables stay valid.
For CPU tensors the image is assembled with torch copies (``assemble_host``): the loop's host path, and the oracle of the kernels.

The file is a ``torch.save`` of a dict in Lightning 2.x's checkpoint layout (``lightning_layout``) with one key of its own,
``vibravox_amd``; it loads with ``torch.load(path, map_location="cpu", weights_only=True)``.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Mapping, Optional, Tuple, Union

import torch

ALIGN = 16   # every tensor of an image starts on this grid (EbenPackEntry.image_offset)
TRAINED = ("generator.", "discriminator.")   # the state_dict keys a restore loads strictly


def _up(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


# ---- the image's layout (host only) -----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ImageEntry:
    name: str
    dtype: torch.dtype
    shape: Tuple[int, ...]
    offset: int
    nbytes: int


@dataclass(frozen=True)
class ImagePlan:
    entries: Tuple[ImageEntry, ...]
    total: int   # bytes of the tensors with their padding: a multiple of 16

    @property
    def names(self) -> List[str]:
        return [e.name for e in self.entries]

    @property
    def counters_bytes(self) -> int:
        """The non-finite counters, one uint32 an entry, ride behind the tensors so that one copy brings both to the host."""
        return _up(4 * len(self.entries))

    @property
    def image_bytes(self) -> int:
        return self.total + self.counters_bytes

    def view(self, image: torch.Tensor, entry: ImageEntry) -> torch.Tensor:
        """The entry's tensor as a view into a uint8 image."""
        return image[entry.offset:entry.offset + entry.nbytes].view(entry.dtype).reshape(entry.shape)

    def counters(self, image: torch.Tensor) -> torch.Tensor:
        return image[self.total:self.total + 4 * len(self.entries)].view(torch.int32)


def plan_image(named_tensors: Union[Mapping[str, torch.Tensor], Iterable[Tuple[str, torch.Tensor]]]) -> ImagePlan:
    """Where each tensor goes: the given order, every offset the next multiple of 16 behind the tensor before it.  Reads shapes and
    dtypes only."""
    items = named_tensors.items() if isinstance(named_tensors, Mapping) else named_tensors
    entries, at = [], 0
    for name, t in items:
        nbytes = t.numel() * t.element_size()
        entries.append(ImageEntry(name, t.dtype, tuple(t.shape), at, nbytes))
        at = _up(at + nbytes)
    return ImagePlan(tuple(entries), at)


def assemble_host(plan: ImagePlan, tensors: List[torch.Tensor], image: torch.Tensor) -> torch.Tensor:
    """What ``eben_pack_tensors`` leaves in a device image, with torch copies into a CPU one: the tensors' bytes, zeros in the padding,
    and behind them the count of infinities and NaNs of every float32 tensor (0 for the others)."""
    image[:plan.image_bytes].zero_()
    counts = plan.counters(image)
    for k, (e, t) in enumerate(zip(plan.entries, tensors)):
        if e.nbytes:
            image[e.offset:e.offset + e.nbytes].copy_(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu())
            if e.dtype is torch.float32:
                counts[k] = int((~torch.isfinite(plan.view(image, e))).sum())
    return image


# ---- what a bit-exact continuation needs ------------------------------------------------------------------------------------------------
def _optimizers(module) -> list:
    return list(module.configure_optimizers())


@dataclass
class TrainState:
    """References to everything a continuation needs -- nothing is copied here.  ``tensors`` (name -> tensor, in the image's order: the
    module's ``state_dict``, then the generator optimizer's moments, then the discriminator optimizer's, then the balancer's norms) is
    what a snapshot packs; the rest is small host state."""
    tensors: "OrderedDict[str, torch.Tensor]"
    state_keys: List[str]                        # the state_dict's keys
    moments: List[Dict[int, Tuple[str, str]]]    # per optimizer: parameter index -> the names of exp_avg and exp_avg_sq in `tensors`
    steps: List[Dict[int, float]]                # per optimizer: parameter index -> step
    param_groups: List[list]                     # per optimizer: torch's state_dict()["param_groups"]
    balancer: Optional[List[str]]                # names of the balancer's norms in `tensors`; None before the first balanced step
    rng_cpu: torch.Tensor
    rng_cuda: Optional[torch.Tensor]
    counters: Dict[str, int] = field(default_factory=dict)   # epoch, train_step, loader_epoch, batches_served
    extra: Dict[str, object] = field(default_factory=dict)   # precision plan, generator {m, n, p}

    @classmethod
    def of(cls, module, counters: Optional[Dict[str, int]] = None) -> "TrainState":
        sd = module.state_dict()
        tensors: "OrderedDict[str, torch.Tensor]" = OrderedDict((f"state_dict.{k}", v) for k, v in sd.items())
        moments, steps, groups = [], [], []
        for i, opt in enumerate(_optimizers(module)):
            osd = opt.state_dict()   # torch's layout: parameter indices, the live state tensors
            m, s = {}, {}
            for idx in sorted(osd["state"]):
                st = osd["state"][idx]
                names = (f"optimizer.{i}.{idx}.exp_avg", f"optimizer.{i}.{idx}.exp_avg_sq")
                tensors[names[0]], tensors[names[1]] = st["exp_avg"], st["exp_avg_sq"]
                m[idx], s[idx] = names, float(st["step"])
            moments.append(m)
            steps.append(s)
            groups.append(osd["param_groups"])
        balancer = None
        old = getattr(getattr(module, "balancer", None), "old", None)
        if old is not None:
            balancer = [f"balancer.old.{k}" for k in range(len(old))]
            for name, t in zip(balancer, old):
                tensors[name] = torch.as_tensor(t)
        extra: Dict[str, object] = {"precision": getattr(module, "precision", None)}
        gen = getattr(module, "generator", None)
        pqmf = getattr(gen, "pqmf", None)
        if hasattr(gen, "p") and hasattr(pqmf, "_decimation"):
            extra["generator"] = {"m": int(pqmf._decimation), "n": int(pqmf._kernel_size), "p": int(gen.p)}
        on_cuda = any(t.is_cuda for t in tensors.values())
        return cls(tensors, list(sd), moments, steps, groups, balancer, torch.get_rng_state(),
                   torch.cuda.get_rng_state(next(t.device for t in tensors.values() if t.is_cuda)) if on_cuda else None,
                   dict(counters or {}), extra)


# ---- snapshots --------------------------------------------------------------------------------------------------------------------------
class Taken:
    """One snapshot: the host image it is arriving in and the state that is not a tensor.  ``wait()`` blocks until the image is complete."""

    def __init__(self, plan: ImagePlan, image: torch.Tensor, event, state: TrainState, slot: int):
        self.plan, self.image, self.event, self.state, self.slot = plan, image, event, state, slot

    def wait(self) -> "Taken":
        if self.event is not None:
            self.event.synchronize()
        return self

    def nonfinite(self) -> List[Tuple[str, int]]:
        """(name, count) of every tensor that holds an infinity or a NaN, in the image's order."""
        counts = self.plan.counters(self.wait().image).tolist()
        return [(e.name, c) for e, c in zip(self.plan.entries, counts) if c]

    def tensor(self, name: str) -> torch.Tensor:
        return self.plan.view(self.image, next(e for e in self.plan.entries if e.name == name))

    def checkpoint(self, callbacks: Optional[dict] = None, weights_only: bool = False) -> dict:
        return lightning_layout(self.wait(), callbacks, weights_only)


class Snapshot:
    """One device image, two host images (pinned for a device state) so that one can be written to disk while the next is filled, and
    an event per host image.  ``take`` is the pack launches on the current stream and one ``copy_(non_blocking=True)`` on a copy stream
    behind them; it returns without waiting for the device."""

    def __init__(self):
        self.plan: Optional[ImagePlan] = None
        self.device_image = None
        self.host = [None, None]
        self.events = [None, None]
        self.in_use = [None, None]   # per host image: a concurrent.futures.Future of whoever still reads it
        self.turn = 0
        self._table = None
        self._copy_stream = self._packed = self._copied = None

    def _fit(self, plan: ImagePlan, device: torch.device) -> None:
        same = self.plan is not None and self.plan.entries == plan.entries and (self.device_image is None) == (device.type != "cuda")
        if same:
            return
        for f in self.in_use:
            if f is not None:
                f.result()
        self.plan, self._table, self.in_use = plan, None, [None, None]
        if device.type == "cuda":
            self.device_image = torch.zeros(plan.image_bytes, dtype=torch.uint8, device=device)   # zeros: the bytes behind the last counter
            self.host = [torch.empty(plan.image_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.events = [torch.cuda.Event() for _ in range(2)]
            self._copy_stream, self._packed, self._copied = torch.cuda.Stream(device), torch.cuda.Event(), None
        else:
            self.device_image = None
            self.host = [torch.empty(plan.image_bytes, dtype=torch.uint8) for _ in range(2)]
            self.events = [None, None]

    def take(self, state: TrainState) -> Taken:
        tensors = list(state.tensors.values())
        plan = plan_image(state.tensors)
        devices = {t.device for t in tensors}
        if len(devices) != 1:
            raise ValueError(f"a snapshot takes tensors of one device, got {sorted(map(str, devices))}")
        device = devices.pop()
        self._fit(plan, device)
        slot, self.turn = self.turn, self.turn ^ 1
        if self.in_use[slot] is not None:   # the file written from this image two snapshots ago
            self.in_use[slot].result()
            self.in_use[slot] = None
        if device.type != "cuda":
            return Taken(plan, assemble_host(plan, tensors, self.host[slot]), None, state, slot)
        from ._lib import check, load, stream

        table, keep = pack_table(plan, tensors, self._table)
        self._table = table
        image = self.device_image
        if self._copied is not None:
            torch.cuda.current_stream(device).wait_event(self._copied)
        check(load().eben_pack_tensors(table, len(plan.entries), image.data_ptr(), plan.total, image.data_ptr() + plan.total, stream()), "pack_tensors")
        del keep   # contiguous copies of strided tensors: the caching allocator hands their memory on in stream order
        # The copy to the host rides a stream of its own behind the pack launches: over PCIe it takes about as long as a train step, and
        # on the current stream the next step would queue behind it.  The next pack waits for it (above) before it overwrites the image.
        self._packed.record()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(self._packed)
            self.host[slot].copy_(image, non_blocking=True)
            self.events[slot].record()
        self._copied = self.events[slot]
        return Taken(plan, self.host[slot], self.events[slot], state, slot)

    def reading(self, taken: Taken, future) -> None:
        """``future`` completes when the reader of the snapshot's host image (a writer thread) is done with it."""
        self.in_use[taken.slot] = future


def pack_table(plan: ImagePlan, tensors: List[torch.Tensor], table=None):
    """The ``EbenPackEntry`` table of device ``tensors`` laid out by ``plan`` (``table``: one of the same plan to refresh), and the
    contiguous copies it points at where a tensor was strided."""
    from ._lib import EbenPackEntry

    n = len(plan.entries)
    fresh = table is None
    if fresh:
        table = (EbenPackEntry * n)()
    keep = []
    for k, (e, t) in enumerate(zip(plan.entries, tensors)):
        if not t.is_cuda:
            raise ValueError(f"{e.name}: a device image takes device tensors, got one on {t.device}")
        if not t.is_contiguous():
            t = t.contiguous()
            keep.append(t)
        if fresh:
            table[k] = EbenPackEntry(t.data_ptr() or 16, e.offset, e.nbytes, int(e.dtype is torch.float32), 0)
        else:
            table[k].tensor = t.data_ptr() or 16   # an empty tensor has no storage: any non-null pointer, never read
    return table, keep


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
LIGHTNING_VERSION = "2.2.0"


def lightning_layout(taken: Taken, callbacks: Optional[dict] = None, weights_only: bool = False) -> dict:
    """The checkpoint dict.  Lightning is not installed where this was written: the keys below restate its 2.x layout from memory and
    are pinned by no test against Lightning itself -- this function is the one place that knows them.  ``global_step`` counts
    ``optimizer.step()`` calls over both optimizers, as Lightning does under manual optimisation; the plain count of training steps is
    ``vibravox_amd/train_step``.  Every tensor is a view into the snapshot's one host image."""
    st, plan = taken.state, taken.plan
    views = {e.name: plan.view(taken.image, e) for e in plan.entries}
    c = st.counters
    optimizer_steps = int(sum(max(s.values()) for s in st.steps if s))
    out = {
        "epoch": int(c.get("epoch", 0)),
        "global_step": optimizer_steps,
        "pytorch-lightning_version": LIGHTNING_VERSION,
        "state_dict": OrderedDict((k, views[f"state_dict.{k}"]) for k in st.state_keys),
        "lr_schedulers": [],
        "loops": {"fit_loop": {"epoch_progress": {"current": {"completed": int(c.get("epoch", 0))}},
                               "epoch_loop.batch_progress": {"current": {"completed": int(c.get("batches_served", 0))}}}},
        "callbacks": dict(callbacks or {}),
        "vibravox_amd": {
            "train_step": int(c.get("train_step", 0)),
            "loader_epoch": int(c.get("loader_epoch", 0)),
            "batches_served": int(c.get("batches_served", 0)),
            "balancer_old": None if st.balancer is None else [views[n] for n in st.balancer],
            "rng_cpu": st.rng_cpu,
            "rng_cuda": st.rng_cuda,
            "precision": st.extra.get("precision"),
            "generator": st.extra.get("generator"),
        },
    }
    if not weights_only:
        out["optimizer_states"] = [
            {"state": {idx: {"step": torch.tensor(steps[idx]), "exp_avg": views[a], "exp_avg_sq": views[b]} for idx, (a, b) in moments.items()},
             "param_groups": groups}
            for moments, steps, groups in zip(st.moments, st.steps, st.param_groups)]
    return out


def write_file(ckpt: dict, path: str) -> None:
    """``torch.save`` to ``path``.tmp, then ``os.replace``: a reader never sees a file that is not complete."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def load_file(path: str) -> dict:
    return torch.load(path, map_location="cpu", weights_only=True)


# ---- restore ----------------------------------------------------------------------------------------------------------------------------
def _new_adam_state(p: torch.Tensor) -> dict:
    """An Adam state as ``FusedAdam.step`` (and ``torch.optim.Adam``) creates it at a parameter's first step."""
    return {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
            "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}


def _scatter(pairs: List[Tuple[str, torch.Tensor, torch.Tensor]]) -> None:
    """``dst`` <- ``src`` (CPU) for every (name, dst, src): one host image, one copy to the device and ``eben_unpack_tensors`` into the
    storages that exist where ``dst`` is on the device, plain copies where it is not."""
    device = [(n, d, s) for n, d, s in pairs if d.is_cuda]
    for n, d, s in pairs:
        if d.shape != s.shape or d.dtype != s.dtype:
            raise ValueError(f"{n}: the checkpoint holds {tuple(s.shape)} {s.dtype}, the module {tuple(d.shape)} {d.dtype}")
        if not d.is_cuda:
            d.copy_(s)
    if not device:
        return
    from ._lib import EbenPackEntry, check, load, stream

    plan = plan_image([(n, s) for n, _, s in device])
    host = assemble_host(plan, [s for _, _, s in device], torch.empty(plan.image_bytes, dtype=torch.uint8).pin_memory())
    dev = device[0][1].device
    image = host.to(dev, non_blocking=True)
    table = (EbenPackEntry * len(device))()
    strided = []
    for k, (e, (n, d, _)) in enumerate(zip(plan.entries, device)):
        target = d if d.is_contiguous() else torch.empty_like(d, memory_format=torch.contiguous_format)
        if target is not d:
            strided.append((d, target))
        table[k] = EbenPackEntry(target.data_ptr() or 16, e.offset, e.nbytes, int(e.dtype is torch.float32), 0)
    check(load().eben_unpack_tensors(table, len(device), image.data_ptr(), plan.total, stream()), "unpack_tensors")
    for d, target in strided:
        d.copy_(target)
    torch.cuda.current_stream(dev).synchronize()   # the pinned image is freed on return


@torch.no_grad()
def restore(module, path_or_dict: Union[str, os.PathLike, dict]) -> dict:
    """Loads a checkpoint into ``module`` in place: parameters, buffers, Adam moments and steps, balancer state, RNG states.  Moments of
    a fresh optimizer are created first, as its first step would.  ``generator.*`` / ``discriminator.*`` keys are loaded strictly; any
    other ``state_dict`` key the module does not have is skipped and reported; without a ``vibravox_amd`` key (a checkpoint of the
    reference's) the balancer starts fresh and the RNG states stay as they are.  Returns the report: ``skipped``, ``epoch``,
    ``global_step``, ``train_step``, ``loader_epoch``, ``batches_served``, ``callbacks``, ``native`` (whether ``vibravox_amd`` was
    there)."""
    from . import ops

    ckpt = path_or_dict if isinstance(path_or_dict, dict) else load_file(os.fspath(path_or_dict))
    saved, live = ckpt["state_dict"], module.state_dict()
    missing = [k for k in live if k.startswith(TRAINED) and k not in saved]
    unexpected = [k for k in saved if k.startswith(TRAINED) and k not in live]
    if missing or unexpected:
        raise KeyError(f"the checkpoint does not fit the module: missing {missing}, unexpected {unexpected}")
    pairs = [(k, live[k], saved[k]) for k in live if k in saved]
    skipped = [k for k in saved if k not in live]
    optimizers = _optimizers(module)
    steps = []
    for i, (opt, osd) in enumerate(zip(optimizers, ckpt.get("optimizer_states") or [])):
        params = [p for g in opt.param_groups for p in g["params"]]
        for g, saved_group in zip(opt.param_groups, osd["param_groups"]):
            for key, value in saved_group.items():
                if key != "params" and key in g:
                    g[key] = value
        for idx, st in osd["state"].items():
            p = params[int(idx)]
            if not opt.state[p]:
                opt.state[p].update(_new_adam_state(p))
            mine = opt.state[p]
            pairs += [(f"optimizer.{i}.{idx}.{key}", mine[key], st[key]) for key in ("exp_avg", "exp_avg_sq")]
            steps.append((mine["step"], st["step"]))
    _scatter(pairs)
    for mine, theirs in steps:
        mine.fill_(float(theirs))
    ops.bump_weights_epoch([d for _, d, _ in pairs])   # packed weight images and bf16 bundles follow the restored parameters
    own = ckpt.get("vibravox_amd")
    balancer = getattr(module, "balancer", None)
    if balancer is not None:
        device = next((d.device for _, d, _ in pairs), torch.device("cpu"))
        old = None if own is None else own.get("balancer_old")
        balancer.old = None if old is None else [t.clone().to(device) for t in old]
        balancer.last_norms = balancer.last_lambdas = None
    if own is not None:
        torch.set_rng_state(own["rng_cpu"])
        if own.get("rng_cuda") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(own["rng_cuda"])
    own = own or {}
    return {"skipped": skipped, "epoch": int(ckpt.get("epoch", 0)), "global_step": int(ckpt.get("global_step", 0)),
            "train_step": int(own.get("train_step", 0)), "loader_epoch": int(own.get("loader_epoch", ckpt.get("epoch", 0))),
            "batches_served": int(own.get("batches_served", 0)), "callbacks": ckpt.get("callbacks") or {}, "native": bool(own)}


# ---- generator export -------------------------------------------------------------------------------------------------------------------
def export_generator(ckpt_path: Union[str, os.PathLike], out_dir: Union[str, os.PathLike]) -> str:
    """The ``generator.*`` tensors and ``{m, n, p}`` of a checkpoint as a ``save_pretrained`` directory (``config.json``,
    ``model.safetensors``): what ``EBENGenerator.from_pretrained`` and ``python -m vibravox_amd.export --generator`` load.  Host only."""
    from safetensors.torch import save_file

    ckpt = load_file(os.fspath(ckpt_path))
    config = (ckpt.get("vibravox_amd") or {}).get("generator")
    if not config:
        raise ValueError(f"{ckpt_path}: no generator {{m, n, p}} under 'vibravox_amd' (a checkpoint of another program: build the "
                         f"EBENGenerator and load its state_dict instead)")
    prefix = "generator."
    tensors = {k[len(prefix):]: v.contiguous().clone() for k, v in ckpt["state_dict"].items() if k.startswith(prefix)}
    if not tensors:
        raise ValueError(f"{ckpt_path}: no generator.* tensor in the state_dict")
    out_dir = os.fspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump({k: int(config[k]) for k in ("m", "n", "p")}, f, indent=2)
    save_file(tensors, os.path.join(out_dir, "model.safetensors"), metadata={"format": "pt"})
    return out_dir
