"""torch.autograd plumbing over the C ABI of libeben_hip.so.

PyTorch is used for device memory (caching allocator), streams and the autograd graph; every
arithmetic op of the EBEN hot path below is a hand-written HIP kernel (``vibravox_amd/csrc``).
Nothing here runs on CPU tensors: ``_lib.ptr`` raises for them.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os
import warnings
import weakref
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import EbenConv1dDesc, EbenPackJob, EbenRuPackJob, EbenWnBwdItem, EbenWnScaleItem, check, load, ptr, stream

# Optimisers that write parameters behind autograd's back (FusedAdam) bump the epoch of exactly
# the storages they touched, so that only those layers' packed-weight caches are rebuilt.
_storage_epoch: Dict[int, int] = {}


def bump_weights_epoch(params=None) -> None:
    if params is None:
        for k in list(_storage_epoch):
            _storage_epoch[k] += 1
        _storage_epoch[-1] = _storage_epoch.get(-1, 0) + 1
        return
    for p in params:
        k = p.data_ptr()
        _storage_epoch[k] = _storage_epoch.get(k, 0) + 1


_param_lists: "weakref.WeakKeyDictionary" = None


def parameters_of(module) -> list:
    """``list(module.parameters())`` without walking the module tree each step (four walks of ~190 tensors were 0.7 ms of a step's host
    time): the list is kept per module until ``bump_weights_epoch()`` (no arguments) says the parameters were replaced -- the same call
    that invalidates the engines' packed-weight caches.  ``requires_grad`` is NOT cached: callers filter on it."""
    global _param_lists
    if _param_lists is None:
        import weakref
        _param_lists = weakref.WeakKeyDictionary()
    epoch = _storage_epoch.get(-1, 0)
    hit = _param_lists.get(module)
    if hit is None or hit[0] != epoch:
        hit = _param_lists[module] = (epoch, list(module.parameters()))
    return hit[1]


def conv_params(m):
    """(v, g) of a weight-normalised HipConv1d, (weight, None) of a plain one -- the Parameter objects, kept on the module until
    ``bump_weights_epoch()`` announces replaced parameters (the engines ask ~300 times a step)."""
    epoch = _storage_epoch.get(-1, 0)
    hit = m.__dict__.get("_vg")
    if hit is None or hit[0] != epoch:
        if m.weight_norm:
            prm = m.parametrizations["weight"]
            vg = (prm.original1, prm.original0)
        else:
            vg = (m.weight, None)
        hit = m.__dict__["_vg"] = (epoch, vg)
    return hit[1]


MATH_F32, MATH_BF16, MATH_BF16X2, MATH_BF16X3, MATH_BF16X6 = 0, 1, 2, 3, 4   # EBEN_MATH_* of include/eben_hip.h
ROUTE_NOW, ROUTE_SIDE, ROUTE_COLLECT = "now", "side", "collect"


class BackwardMode(NamedTuple):
    """What a backward pass has been asked to do: ``_mode``, replaced for the length of a ``_scope``."""
    # The skips: a Function's ``needs_input_grad`` is fixed at forward time, so without them the weight-gradient GEMMs would run inside
    # torch.autograd.grad(loss, bands), and the input gradients inside the balancing norms' torch.autograd.grad(bands, last_conv.weight),
    # although their results are discarded.
    skip_input_grads: bool = False
    skip_weight_grads: bool = False
    # Arithmetic of the BACKWARD contractions (input and weight gradients) of `conv_layer`; the forward is always exact fp32.  Read when
    # the forward runs (the backward image of the weights is packed then).
    math: int = MATH_F32
    # A layer's weight gradient is launched now and returned to the caller (autograd), deferred to the side stream
    # (``weight_grads_on_side_stream``), or launched now with its slab-sum job appended to ``jobs`` (``collect_wn_jobs``); what that
    # means for one layer's parameters is ``_wg_route``'s to say.
    route: str = ROUTE_NOW
    sink: object = None            # ``ddp.GradSync``: results are written into its gradient-bucket views where it has them
    jobs: Optional[list] = None    # ROUTE_COLLECT


_mode = BackwardMode()


class _scope:
    """Context manager: ``fields`` of the backward mode replaced inside, the record found on entry (``prev``) back on exit."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        global _mode
        self.prev, _mode = _mode, _mode._replace(**self.fields)
        return self

    def __exit__(self, *exc):
        global _mode
        _mode = self.prev


def input_grads_disabled():
    return _scope(skip_input_grads=True)


def weight_grads_disabled():
    return _scope(skip_weight_grads=True)


def backward_math(math: int):
    """with ops.backward_math(ops.MATH_BF16): forwards run inside record bf16 backward contractions."""
    return _scope(math=math)


def collect_wn_jobs(jobs: list, sink=None):
    """Inside this context ``weight_grads`` / ``weight_grads_ru`` launch the weight-gradient kernels only, on the current stream (the
    caller has made the stream the work belongs on current), and append the slab-sum + weight-norm job of each layer to ``jobs``: the
    caller runs them as ONE ``wn_bwd_multi(jobs)`` (gen_engine's graph-captured weight-gradient body).  sink: results go straight into
    its gradient buffers (``grad_buffer(param)``)."""
    return _scope(route=ROUTE_COLLECT, sink=sink, jobs=jobs)


def accumulate_grad(p, t, hooks: bool = False) -> None:
    """``t`` becomes ``p.grad`` or is added to it, as autograd would; hooks: and the post-accumulate hooks fire (``ddp.GradSync``)."""
    if p.grad is None:
        p.grad = t
    else:
        p.grad.add_(t)
    if hooks:
        for hook in list((getattr(p, "_post_accumulate_grad_hooks", None) or {}).values()):
            hook(p)


def _no_grad_hooks(p) -> bool:
    return p is None or (not getattr(p, "_post_accumulate_grad_hooks", None) and not p._backward_hooks)


# Weight-gradient work on a side HIP stream.  A layer's backward is a serial chain of launches: input gradient (needed by the next
# layer) and, independent of it, the weight-gradient GEMM + slab reduction + weight-norm chain rule.  Inside
# `weight_grads_on_side_stream()` the second group is issued on a side stream, so the input-gradient chain of the whole network is not
# held up by it.  The caller must `join()` before anything on the main stream reads the parameter gradients (the optimiser step).  The
# deferred gradients never pass through autograd -- backward() returns None for them (it may clone what it is given, and the deferred
# kernels would then fill a tensor nobody reads) -- so without a sink only layers whose parameters hold no `.grad` and carry no
# accumulation hook are deferred (`_wg_route`): `join()` assigns `p.grad` itself once the side stream is done.
class _Pending:
    """What ``join()`` still owes."""

    __slots__ = ("keep", "wn_jobs", "assign", "sunk")

    def __init__(self):
        # keep: every tensor a side-stream kernel reads, referenced until the join -- autograd sums gradients IN PLACE into a buffer it
        # holds the only reference to (a residual add hands the same tensor to both branches), which would rewrite the gradient on the
        # main stream under the kernel reading it.  wn_jobs: the slab sums + weight-norm chain rule of ALL deferred layers, one
        # multi-tensor call at the join.  assign: (parameter, gradient) for ``.grad``.  sunk: parameters to report to the sink.
        self.keep, self.wn_jobs, self.assign, self.sunk = [], [], [], []

    def defer(self, keep, jobs) -> None:
        """A weight-gradient launch on the side stream: what it reads, and the jobs that finish it."""
        self.keep.append(keep)
        self.wn_jobs.extend(jobs)

    def hand_over(self, pairs, sink=None, early: bool = False, keep=None) -> None:
        """(parameter, gradient) pairs of work queued on the side stream, which reads ``keep``: a view of ``sink``'s buckets is reported
        to it (early: now, from the current stream, else at the join), anything else is assigned at the join."""
        if keep is not None:
            self.keep.append(keep)
        if sink is None:
            self.assign.extend(pairs)
        elif early:
            sink.mark_ready([p for p, _ in pairs])
        else:
            self.sunk.extend(p for p, _ in pairs)

    def settle(self, sink) -> None:
        st = _sides.stream
        if st is not None:
            for k in SIDE_STREAMS[1:]:
                st.wait_stream(aux_stream(k, st.device))
            if self.wn_jobs:
                with torch.cuda.stream(st):
                    wn_bwd_multi(self.wn_jobs)   # two launches
                self.wn_jobs = []
            torch.cuda.current_stream(st.device).wait_stream(st)
        assign, self.assign = self.assign, []
        for p, t in assign:   # complete on this stream from here on
            accumulate_grad(p, t)
        if self.sunk:
            sunk, self.sunk = self.sunk, []
            sink.mark_ready(sunk)
        self.keep.clear()   # the current stream has waited for the side stream: what its kernels read may be reused from here on

    def drop(self) -> None:
        # a backward that raised half-way leaves jobs pointing at tensors nobody will hand over: wait for what was launched, then
        # drop everything instead of letting the next join() write through stale pointers
        st = _sides.stream
        if st is not None:
            for k in SIDE_STREAMS:
                torch.cuda.current_stream(st.device).wait_stream(aux_stream(k, st.device))
        self.__init__()


_pending = _Pending()
hand_over = _pending.hand_over   # for the engines: what their own side-stream launches produced


class weight_grads_on_side_stream(_scope):
    """sink: an object with ``grad_buffer(param) -> tensor | None`` and ``mark_ready(params)`` (``ddp.GradSync``): the
    weight gradients are then written straight into the sink's buffers (data-parallel gradient buckets) and reported at
    ``join()``, instead of being handed to autograd -- which would accumulate them into ``p.grad`` on the main stream
    the moment the layer's backward returns, i.e. force the weight-gradient work back onto the critical path."""

    def __init__(self, sink=None):
        super().__init__(route=ROUTE_SIDE, sink=sink, jobs=None)
        self.sink = sink

    def __exit__(self, exc_type, *exc):
        super().__exit__(exc_type, *exc)
        if exc_type is not None:
            _pending.drop()

    def join(self):
        _pending.settle(self.sink)


# The HIP runtime multiplexes a process's streams onto a fixed number of hardware queues, and streams that share a queue execute in
# submission order with each other (how many queues, and why: _env.py).  So a train step uses the main stream plus exactly THREE
# auxiliary streams, created together on first use, in this order:
#   0: MelGAN discriminator chain   1: the three PQMF-band discriminator chains (in series)   2: generator weight gradients and weight
#   pre-packing (the "side" stream below)
# A data-parallel rank adds one communication stream of its own (ddp.GradSync).
_aux = {"device": None, "streams": None}
#: HIP priorities of the three auxiliary streams (0 = default, -1 = high; torch's range on this device is (0, -1)).  The stream that
#: carries the generator's weight gradients, the weight pre-packing and (spread backward) one PQMF-band chain gets the high one: the
#: step ends on that work and every other queue's kernels can absorb a delay.  [MI355X, same box] ms/step: "0,0,0" 15.27 / 15.07,
#: "0,0,-1" 15.12 / 14.92 / 14.94, "-1,0,0" 15.42, "0,-1,0" 15.69, "-1,0,-1" 15.19, "0,-1,-1" 15.13, "-1,-1,-1" 15.27; the MelGAN
#: layer-4 forward launch inside the step 0.438 -> 0.36 ms.  Round 5 (9.3 ms step, persistent tile kernels that hold a CU for their whole
#: launch): the high priority no longer pays -- "0,0,-1" 9.282 / 9.287 / 9.269, "0,0,0" 9.199 / 9.223 / 9.229, "-1,0,0" 9.305 / 9.291 /
#: 9.322 (same box, 100 steps each) -- all default
AUX_PRIORITY = tuple(int(t) for t in os.environ.get("EBEN_AUX_PRIORITY", "0,0,0").split(","))


def aux_stream(i: int, device=None) -> "torch.cuda.Stream":
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    if _aux["streams"] is None or _aux["device"] != device:
        _aux["device"], _aux["streams"] = device, [torch.cuda.Stream(device=device, priority=AUX_PRIORITY[i]) for i in range(3)]
    return _aux["streams"][i]


#: auxiliary streams the deferred weight-gradient jobs are dealt over (round robin).  One stream is the measured best [MI355X]:
#: "2" 15.35 / 15.39 ms/step, "2,1" 15.62, "2,1,0" 15.54, "2,0" 16.76 -- the other queues still carry the discriminators'
#: weight gradients, and a generator job dealt behind them waits for work it does not depend on
SIDE_STREAMS = tuple(int(t) for t in os.environ.get("EBEN_SIDE_STREAMS", "2").split(",") if t.strip() != "")


class _Sides:
    __slots__ = ("stream", "rr")   # the side stream once it has been used (the joins wait for it); whom the last job was dealt to


_sides = _Sides()
_sides.stream, _sides.rr = None, -1


def _side_stream(device, deal: bool = False) -> "torch.cuda.Stream":
    """The side stream (weight pre-packing; joins); ``deal``: the next one of SIDE_STREAMS, for a weight-gradient job."""
    st = _sides.stream = aux_stream(SIDE_STREAMS[0], device)
    if not deal or len(SIDE_STREAMS) == 1:
        return st
    _sides.rr = (_sides.rr + 1) % len(SIDE_STREAMS)
    return aux_stream(SIDE_STREAMS[_sides.rr], device)


class WnJob(NamedTuple):
    """One slab-sum / weight-norm job: the arguments of ``eben_wn_bwd`` for one layer (built by ``wn_job``)."""
    slabs: torch.Tensor
    nslab: int
    slab_stride: int
    rows: int
    cols: int
    row_stride: int
    g: Optional[torch.Tensor]
    v: torch.Tensor
    norm: Optional[torch.Tensor]
    dg: object       # outputs: tensors or raw device pointers
    dv: object
    dbias: object
    col_perm_k: int = 0


def wn_job(slabs, nslab: int, row_stride: int, v, g, norm, outs, *, col_perm_k: int = 0) -> WnJob:
    """The job that sums ``nslab`` split-K slabs of ``v``'s shape (rows of ``row_stride`` floats) and applies the weight-norm chain rule
    into ``outs`` = (dv, dg, dbias).  The logits layer (one output channel) is the one-row case, its two branches two jobs over views
    of one slab buffer; without ``g`` the sums are written as they are.  col_perm_k: the slabs' columns are in the bundle-major order
    of ``eben_bl_conv1d_bwd_dw``."""
    dv, dg, dbias = outs
    rows = v.shape[0]
    has_g = g is not None
    return WnJob(slabs, nslab, rows * row_stride, rows, v.numel() // rows, row_stride, g.detach() if has_g else None, v.detach(),
                 norm if has_g else None, dg, dv, dbias, col_perm_k)


def wn_bwd_multi(jobs) -> None:
    """jobs: one ``WnJob`` per layer (or a plain sequence of its fields in order, the form this call took before the record), on the
    current stream, as one multi-tensor call."""
    if not jobs:
        return
    items = (EbenWnBwdItem * len(jobs))()
    p = lambda t: t if t is None or isinstance(t, int) else ptr(t)   # outputs may arrive as raw device pointers
    for it, job in zip(items, jobs):
        if not isinstance(job, WnJob):
            job = WnJob(*job)
        it.col_perm_k = job.col_perm_k
        it.slabs, it.g, it.v, it.norm = ptr(job.slabs), ptr(job.g), ptr(job.v), ptr(job.norm)
        it.dg, it.dv, it.dbias = p(job.dg), p(job.dv), p(job.dbias)
        it.slab_stride, it.nslab, it.rows, it.cols, it.row_stride = job.slab_stride, job.nslab, job.rows, job.cols, job.row_stride
    check(load().eben_wn_bwd_multi(items, len(jobs), stream()), "wn_bwd_multi")


def wn_scale_multi(jobs) -> None:
    """jobs: (g, v, rows, cols, scale, norm) per layer, one multi-tensor call on the current stream."""
    if not jobs:
        return
    items = (EbenWnScaleItem * len(jobs))()
    for it, (g, v, rows, cols, scale, norm) in zip(items, jobs):
        it.g, it.v, it.scale, it.norm, it.rows, it.cols = ptr(g), ptr(v), ptr(scale), ptr(norm), rows, cols
    check(load().eben_wn_scale_multi(items, len(jobs), stream()), "wn_scale_multi")


class KernelTimer:
    """HIP-event timing of one layer's forward ("fwd") or input-gradient ("dx") launch on the stream it is launched on (bench.py)."""

    def __init__(self, spec: "ConvSpec", which: str = "fwd"):
        self.spec, self.which, self.enabled, self.events, self.batch = spec, which, False, [], None

    def start(self):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def stop(self, e0, batch: int) -> None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.events.append((e0, e1))
        self.batch = batch

    def mean_ms(self) -> Optional[float]:
        if not self.events:
            return None
        return sum(a.elapsed_time(b) for a, b in self.events) / len(self.events)


_timers: List[KernelTimer] = []


def set_kernel_timers(timers: Sequence[KernelTimer]) -> None:
    _timers[:] = list(timers)


def set_kernel_timer(t: Optional[KernelTimer]) -> None:
    set_kernel_timers([] if t is None else [t])


def kernel_timer_for(spec: "ConvSpec", which: str) -> Optional[KernelTimer]:
    for t in _timers:
        if t.enabled and t.which == which and t.spec == spec:
            return t
    return None


def _empty(n_bytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(max(1, (n_bytes + 3) // 4), dtype=torch.float32, device=like.device)


def _iptr(t: torch.Tensor) -> int:
    """Device pointer of a contiguous int32 table (``ptr`` takes float32 only)."""
    if not t.is_cuda or t.dtype is not torch.int32 or not t.is_contiguous():
        raise _lib.EbenError(f"expected a contiguous int32 tensor on a HIP device, got {t.dtype} on '{t.device}'")
    return t.data_ptr()


# --------------------------------------------------------------------------------------------
# conv layers
# --------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvSpec:
    """Static description of one Conv1d / ConvTranspose1d layer (+ fused activations)."""

    c_in: int
    c_out: int
    ksize: int
    stride: int = 1
    dilation: int = 1
    groups: int = 1
    pad_l: int = 0
    pad_r: int = 0
    reflect: bool = False
    transposed: bool = False
    output_padding: int = 0
    in_slope: float = 1.0
    out_slope: float = 1.0

    def out_len(self, l_in: int) -> int:
        if self.transposed:
            return (l_in - 1) * self.stride - 2 * self.pad_l + self.dilation * (self.ksize - 1) + self.output_padding + 1
        return (l_in + self.pad_l + self.pad_r - self.dilation * (self.ksize - 1) - 1) // self.stride + 1

    def weight_shape(self) -> Tuple[int, int, int]:
        if self.transposed:
            return (self.c_in, self.c_out // self.groups, self.ksize)
        return (self.c_out, self.c_in // self.groups, self.ksize)


_desc_cache: Dict[Tuple[ConvSpec, int, int], EbenConv1dDesc] = {}


# EBEN_CONV_ROUTE_* of include/eben_hip.h: the answers of eben_conv1d_kernel_generation and out[0] of eben_conv1d_variant
CONV_ROUTE_NONE, CONV_ROUTE_TAP1, CONV_ROUTE_TAP2, CONV_ROUTE_THIN, CONV_ROUTE_TAP3, CONV_ROUTE_GC, CONV_ROUTE_TAP4 = 0, 1, 2, 3, 4, 5, 6
CONV_ROUTES_WITH_FM_EPILOGUE = (CONV_ROUTE_THIN, CONV_ROUTE_TAP3)   # the input gradients eben_conv1d_bwd_dx_fm accepts


def conv_desc(spec: ConvSpec, batch: int, l_in: int, math: int = MATH_F32) -> EbenConv1dDesc:
    key = (spec, batch, l_in, math)
    d = _desc_cache.get(key)
    if d is None:
        if len(_desc_cache) >= 4096:   # variable clip lengths ("pad" collation): do not grow without bound
            _desc_cache.clear()
        d = EbenConv1dDesc(
            batch, spec.c_in, spec.c_out, l_in, spec.out_len(l_in), spec.ksize, spec.stride, spec.dilation, spec.groups,
            spec.pad_l, spec.pad_r, 1 if spec.reflect else 0, 1 if spec.transposed else 0, spec.in_slope, spec.out_slope, math,
        )
        _desc_cache[key] = d
    return d


def weights_key(params, *extra) -> tuple:
    """When a weight image is current: address, ``_version`` and storage epoch of every tensor in ``params`` (None allowed), the global
    epoch, and whatever else the caller's image depends on (``extra``).  The one staleness test of every image cache."""
    e = _storage_epoch
    return tuple(None if t is None else (t.data_ptr(), t._version, e.get(t.data_ptr(), 0)) for t in params) + (e.get(-1, 0),) + extra


def _addrs(image) -> tuple:
    return (image.data_ptr(),) if isinstance(image, torch.Tensor) else tuple(t.data_ptr() for t in image if isinstance(t, torch.Tensor))


class PackedWeights:
    """Image cache of one layer or fused residual unit: its parameter tensors, their weight-norm scale and norm, and MFMA-layout
    images of the weights (scale folded in) by slot, each with the ``weights_key`` of the parameters it was built from.  What a slot
    is, how its image is built and which slots are kept belongs to the owner (``pack_weights``: the latest descriptor;
    ``disc_engine._Layer``: up to MAX_PACKS shapes and directions; ``gen_engine``: a fused unit's forward image and one backward image
    per arithmetic).  ``prepack`` rebuilds the images of many caches after an optimiser step."""

    __slots__ = ("params", "scale", "norm", "scale_key", "images", "used", "prune", "reuse")

    def __init__(self, prune: bool = False):
        self.params = ()          # (v, g) of a layer (g None without weight norm); (v, g) of each conv of a fused unit
        self.scale = self.norm = self.scale_key = None
        self.images = {}          # slot -> (weights_key at build time, image)
        self.used = set()         # slots read since the last prepack (only tracked where ``prune``)
        self.prune = prune        # prepack drops the slots not used since the last one (else it rebuilds every slot held)
        self.reuse = False        # inside prepack: rebuild into the buffers already held (a graph replay writes the ones it captured)

    def current(self, slot, key) -> bool:
        hit = self.images.get(slot)
        return hit is not None and hit[0] == key

    def buffer(self, old: Optional[torch.Tensor], numel: int, like: torch.Tensor) -> torch.Tensor:
        """A float buffer of ``numel`` elements: ``old`` itself while rebuilding in place and it has that size (the step that read the
        old contents is complete), else a fresh one."""
        if self.reuse and old is not None and old.numel() == numel and old.device == like.device:
            return old
        return torch.empty(numel, dtype=torch.float32, device=like.device)

    def wn_jobs(self) -> list:
        """``wn_scale_multi`` jobs of every weight-normalised (v, g) pair of ``params``, into the buffers held: (scale, norm) of one
        pair, or one [scale, norm] block per pair (a fused unit)."""
        pairs = [(v.detach(), g.detach()) for v, g in zip(self.params[0::2], self.params[1::2]) if g is not None]
        if not pairs:
            self.scale = self.norm = None
            return []
        rows = pairs[0][0].shape[0]
        if len(pairs) == 1:
            self.scale = self.buffer(self.scale, rows, pairs[0][0])
            self.norm = self.buffer(self.norm, rows, pairs[0][0])
            bufs = [(self.scale, self.norm)]
        else:
            self.scale = self.buffer(self.scale, 2 * len(pairs) * rows, pairs[0][0]).view(2 * len(pairs), rows)
            bufs = [(self.scale[2 * i], self.scale[2 * i + 1]) for i in range(len(pairs))]
        return [(g, v, v.shape[0], v.numel() // v.shape[0], s, n) for (v, g), (s, n) in zip(pairs, bufs)]

    def ensure_scale(self) -> tuple:
        """The weight-norm scale and norm of the current parameters (what the images fold in), launched when stale.  Returns the
        parameters' ``weights_key``."""
        key = weights_key(self.params)
        if self.scale_key == key:
            return key
        jobs = self.wn_jobs()
        if len(jobs) == 1:
            g, v, rows, cols, scale, norm = jobs[0]
            check(load().eben_wn_scale(ptr(g), ptr(v), rows, cols, ptr(scale), ptr(norm), stream()), "wn_scale")
        else:
            wn_scale_multi(jobs)
        self.scale_key = key
        return key

    def state(self, slots=None) -> tuple:
        """What a launch sequence reading this cache depends on besides values: the parameter storage, where the scale / norm and the
        images of ``slots`` (default: every slot held) are, and whether each is current."""
        key = weights_key(self.params)
        addr = lambda t: 0 if t is None else t.data_ptr()
        return (tuple(addr(t) for t in self.params), addr(self.scale), addr(self.norm), self.scale_key == key,
                tuple((s, _addrs(self.images[s][1]), self.images[s][0] == key) for s in (self.images if slots is None else slots)))


class ConvImages(NamedTuple):
    """What ``pack_weights`` returns: the images of one descriptor (wp_bwd None when not asked for) and the scale / norm they fold in."""

    wp_fwd: torch.Tensor
    wp_bwd: Optional[torch.Tensor]
    scale: Optional[torch.Tensor]
    norm: Optional[torch.Tensor]
    d: EbenConv1dDesc
    d_bwd: EbenConv1dDesc


_pack_batch: List[Optional[dict]] = [None]


def conv1d_pack(d: EbenConv1dDesc, v, scale, wp_fwd, wp_bwd) -> None:
    """``eben_conv1d_pack`` on the current stream -- or, inside ``pack_batch()``, one job of the ``eben_conv1d_pack_multi`` call
    issued when the context closes (the prepack sequences: ~150 images per step in ~15 launches)."""
    if _pack_batch[0] is not None:
        _pack_batch[0]["conv"].append((d, v, scale, wp_fwd, wp_bwd))
        return
    check(load().eben_conv1d_pack(ctypes.byref(d), ptr(v), ptr(scale), ptr(wp_fwd), ptr(wp_bwd), stream()), "conv1d_pack")


def ru_pack(c: int, math: int, which: int, vd, sd, vp, sp, img) -> None:
    """``eben_ru_pack_ex`` (image of a fused residual unit) on the current stream -- or, inside ``pack_batch()`` and for the split
    arithmetics, one job of the ``eben_ru_pack_multi`` call issued when the context closes."""
    if _pack_batch[0] is not None and math != MATH_F32:
        _pack_batch[0]["ru"].append((c, math, which, vd, sd, vp, sp, img))
        return
    check(load().eben_ru_pack_ex(c, math, which, ptr(vd), ptr(sd), ptr(vp), ptr(sp), ptr(img), stream()), "ru_pack")


@contextlib.contextmanager
def pack_batch():
    """Collects the ``conv1d_pack`` / ``ru_pack`` calls made inside and issues them as one ``eben_conv1d_pack_multi`` and one
    ``eben_ru_pack_multi`` on the current stream at exit (everything the jobs read -- the weight-norm scales -- must have been
    launched on that stream before)."""
    if _pack_batch[0] is not None:   # nested: the outer context flushes
        yield
        return
    _pack_batch[0] = {"conv": [], "ru": []}
    try:
        yield
        jobs = _pack_batch[0]
    finally:
        _pack_batch[0] = None
    if jobs["conv"]:
        table = (EbenPackJob * len(jobs["conv"]))()
        for it, (d, v, scale, wp_fwd, wp_bwd) in zip(table, jobs["conv"]):
            it.desc, it.v, it.scale, it.wp_fwd, it.wp_bwd = d, ptr(v), ptr(scale), ptr(wp_fwd), ptr(wp_bwd)
        check(load().eben_conv1d_pack_multi(table, len(table), stream()), "conv1d_pack_multi")
    if jobs["ru"]:
        table = (EbenRuPackJob * len(jobs["ru"]))()
        for it, (c, math, which, vd, sd, vp, sp, img) in zip(table, jobs["ru"]):
            it.channels, it.math, it.which = c, math, which
            it.v_dil, it.scale_dil, it.v_pw, it.scale_pw, it.wimg = ptr(vd), ptr(sd), ptr(vp), ptr(sp), ptr(img)
        check(load().eben_ru_pack_multi(table, len(table), stream()), "ru_pack_multi")


def pack_weights(spec: ConvSpec, d: EbenConv1dDesc, v: torch.Tensor, g: Optional[torch.Tensor],
                 cache: Optional[PackedWeights], need_bwd: bool, d_bwd: Optional[EbenConv1dDesc] = None) -> ConvImages:
    """Images of one conv layer for the forward launch of ``d`` and the backward launches of ``d_bwd`` (when it differs: bf16
    backward math), from ``cache`` while the parameters and the descriptor's shape and arithmetic are unchanged.  A cache keeps the
    latest descriptor's images and always holds the backward one (it serves every later pass); the weight-norm scale is rebuilt with
    them (inside ``prepack``, which has rebuilt it already, into the buffers held)."""
    lib = load()
    d_bwd = d if d_bwd is None else d_bwd
    pw = cache if cache is not None else PackedWeights()
    if _prepacked is not None and torch.cuda.current_stream() != _sides.stream:
        join_prepack()   # images built ahead of time on the side stream: first consumer waits for them
    need_bwd = need_bwd or cache is not None  # a module-level cache serves every later pass
    pw.params = (v, g)
    slot = (d.batch, d.l_in, d.math, d_bwd.math)
    key = weights_key(pw.params)
    hit = pw.images.get(slot)
    if hit is not None and hit[0] == key and (hit[1].wp_bwd is not None or not need_bwd):
        return hit[1]
    if not pw.reuse:
        pw.scale_key = None
        pw.ensure_scale()
    old = (None, None) if hit is None else hit[1]
    wp_fwd = pw.buffer(old[0], lib.eben_conv1d_packed_floats(ctypes.byref(d), 0), v)
    wp_bwd = pw.buffer(old[1], lib.eben_conv1d_packed_floats(ctypes.byref(d_bwd), 1), v) if need_bwd else None
    if d_bwd is d or not need_bwd:
        conv1d_pack(d, v, pw.scale, wp_fwd, wp_bwd)
    else:
        conv1d_pack(d, v, pw.scale, wp_fwd, None)
        conv1d_pack(d_bwd, v, pw.scale, None, wp_bwd)
    img = ConvImages(wp_fwd, wp_bwd, pw.scale, pw.norm, d, d_bwd)
    pw.images = {slot: (key, img)}
    return img


def conv_images(modules) -> list:
    """``prepack`` entries of the HipConv1d layers among ``modules`` that hold images: each rebuilds its latest descriptor."""
    def entry(pw):
        def rebuild(slot):
            img = pw.images[slot][1]
            pack_weights(None, img.d, *pw.params, pw, True, img.d_bwd)
        return pw, rebuild

    return [entry(m._packed) for m in modules if m._packed.images]


_replayed = weakref.WeakSet()   # every ReplayedPrepack / ReplayedChain alive: graphs_pending() asks them


def graphs_pending() -> int:
    """Launch sequences that are in use but still run eagerly on their way to a capture (a step that captures takes tens of ms: a
    measurement waits until this is 0)."""
    if capture_gate.settled and capture_gate.active():
        return 0   # multi-rank: the gate has closed for good, whatever still runs eagerly stays eager
    if eager_multi_rank():
        return 0
    return sum(1 for r in list(_replayed) if type(r).enabled and r.sig is not None and r.graph is None)


def eager_multi_rank() -> bool:
    """True when a multi-rank run asked for eager launches (``EBEN_DDP_GRAPHS=0``, see ``DDP_GRAPHS``)."""
    if DDP_GRAPHS:
        return False
    d = torch.distributed
    return d.is_available() and d.is_initialized() and d.get_world_size() > 1


#: Multi-rank runs replay the collective-free launch sequences as graphs like a single-GPU run does (every graph holds the launches of ONE
#: stream between two joins; the all-reduces are issued outside them, from ``GradSync.mark_ready`` / ``finish``).  WHEN a sequence is
#: captured is agreed by all ranks (``CaptureGate``: a vote at the end of each of the first steps; captures only in steps every rank
#: opened, each behind a drain of the communication streams, with ``capture_error_mode="thread_local"`` so that the process group's
#: watchdog thread may go on querying its events).  Without the graphs a rank enqueues ~11 ms of host work per ~9 ms step.
#: ``EBEN_DDP_GRAPHS=0`` is the escape hatch (eager launches).  No N > 1 run on hardware has happened yet: the
#: protocol is covered by the world-size-2 gloo test of tests/test_ddp_gloo.py with a recorder in place of the HIP capture.
DDP_GRAPHS = os.environ.get("EBEN_DDP_GRAPHS", "1") != "0"


class CaptureGate:
    """Multi-rank agreement on WHEN launch sequences are captured into HIP graphs (one process per GPU, ``WORLD_SIZE > 1``).

    A capture is a host-side event of tens of milliseconds with a device-wide synchronisation at both ends.  On one rank its timing is
    nobody else's business; with several ranks exchanging gradient buckets it has to be the SAME step on every rank -- else one rank
    sits in a capture while the others wait for it inside a collective, step after step, and which step that is depends on each rank's
    allocator history (a signature contains addresses).  The gate makes the decision a function of the step index agreed by all ranks:

      * a ``ReplayedChain`` / ``ReplayedPrepack`` that reaches its capture threshold is HELD (it goes on running eagerly) and the rank
        votes "ready"; a sequence still counting eager rounds makes the rank vote "busy"; a rank with neither votes "idle";
      * ``step_end()`` -- called by the train step after its last collective was issued -- all-reduces the three flags (one tiny
        blocking collective per step, only until the gate has settled) and opens the gate for the NEXT step iff at least one rank is
        ready and every rank is ready or idle: all ranks see the same sums, so all open in the same step;
      * in an open step exactly the sequences held before it are captured, each after ``drain()``: no capture starts while a gradient
        bucket's collective is in flight (the communication streams registered by ``ddp.GradSync`` are synchronised first);
      * after three consecutive votes with nothing ready or busy anywhere the gate SETTLES: no more votes, no more captures (a
        signature that turns up later -- a validation shape -- runs eagerly for good).

    Single-rank runs (and ``EBEN_DDP_GRAPHS=0``, which keeps multi-rank runs eager altogether) never consult it."""

    QUIET_VOTES = 3

    def __init__(self):
        self._drains = []
        self.reset()

    def reset(self) -> None:
        self.open, self.settled = False, False
        self.ready = self.busy = self.quiet = self.step = 0
        #: (step index, what) of every capture under the gate and every vote result: identical on all ranks (tests/test_ddp_gloo.py)
        self.history = []

    @staticmethod
    def active() -> bool:
        d = torch.distributed
        return DDP_GRAPHS and d.is_available() and d.is_initialized() and d.get_world_size() > 1

    def register_drain(self, fn) -> None:
        """fn(): returns once none of the caller's collectives is in flight (``ddp.GradSync``: synchronise the communication stream)."""
        if fn not in self._drains:
            self._drains.append(fn)

    def drain(self) -> None:
        for fn in self._drains:
            fn()

    def counting(self) -> None:
        """A sequence ran one of its eager rounds below the capture threshold."""
        if not self.settled:
            self.busy += 1

    def may_capture(self, seq, what: str = "") -> bool:
        """Called by a sequence AT its capture threshold: True = capture now (gate open and the sequence was held before this step)."""
        if self.settled:
            return False
        if self.open and getattr(seq, "_held_since", None) is not None and seq._held_since < self.step:
            self.drain()
            self.history.append((self.step, "capture " + what))
            seq._held_since = None
            return True
        if getattr(seq, "_held_since", None) is None:
            seq._held_since = self.step
        self.ready += 1
        return False

    def step_end(self, group=None) -> None:
        if self.settled or not self.active():
            return
        d = torch.distributed
        world = d.get_world_size(group)
        ready, busy = int(self.ready > 0), int(self.busy > 0)
        dev = torch.device("cuda", torch.cuda.current_device()) if d.get_backend(group) == "nccl" else torch.device("cpu")
        vote = torch.tensor([ready, int(not ready and not busy), busy], dtype=torch.int32, device=dev)
        d.all_reduce(vote, op=d.ReduceOp.SUM, group=group)
        r, idle, b = (int(v) for v in vote.tolist())
        self.open = r >= 1 and r + idle == world
        self.quiet = self.quiet + 1 if (r == 0 and b == 0) else 0
        self.history.append((self.step, f"vote ready {r} idle {idle} busy {b} -> {'open' if self.open else 'closed'}"))
        if self.quiet >= self.QUIET_VOTES:
            self.settled, self.open = True, False
            self.history.append((self.step, "settled"))
        self.ready = self.busy = 0
        self.step += 1


capture_gate = CaptureGate()


def graphs_captured() -> int:
    """Launch sequences currently replayed as graphs."""
    return sum(1 for r in list(_replayed) if r.graph is not None)


@contextlib.contextmanager
def _no_gc():
    """Keeps Python's cyclic garbage collector off while a HIP graph is being captured.  torch.cuda.graph collects once on entry,
    but a collection that triggers mid-capture destroys whatever unreachable objects it finds there -- graphs, streams, events and
    tensors of earlier modules -- and releasing those inside a capture aborts the process."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


# Does ``seq`` capture in this round?  Single rank: once it is at its threshold.  Multi-rank, the gate hears of every eager round: below
# the threshold the rank is busy, at it the sequence asks (and is held until every rank may capture).
def _capture_due(seq, what: str, at_threshold: bool) -> bool:
    if not capture_gate.active():
        return at_threshold
    if not at_threshold:
        capture_gate.counting()
        return False
    return capture_gate.may_capture(seq, what)


def _try_capture(cls, what: str, fn, stream_):
    """``cls._capture(fn, stream_)``, or None where it raised (the caller runs ``fn`` itself)."""
    try:
        return cls._capture(fn, stream_)
    except Exception as exc:   # capture is an optimisation: fall back to eager launches for good
        warnings.warn(f"{what} graph capture failed ({exc!r}): staying with eager launches")
        cls.enabled = False
        return None


class ReplayedPrepack:
    """Graph replay of a prepack sequence.  Rebuilding the packed weight images after an optimiser step is ~150 tiny launches per
    step (one or two per layer and direction) whose cost is entirely host-side: ~3 ms of Python / launch time per step during which
    the GPU has nothing else queued -- on a 19 ms step.  The sequence is static (same kernels, same parameter storage, same image
    buffers every step), so after two eager rounds it is captured into a HIP graph and replayed: one launch call.  ``sig`` names
    everything the launches depend on besides the weights' values (layers, shapes, parameter storage AND the addresses of the image /
    scale buffers the launches write: a forward at another shape between two train steps -- validation -- reallocates them, and a
    replay would go on filling the orphaned ones); a new signature falls back to eager rounds and a new capture.  The prepack bodies
    rebuild INTO the buffers the caches hold (``PackedWeights.reuse``), so the signature settles after one eager round.  Tensors
    allocated by the body while capturing live in the graph's pool for as long as the graph."""

    enabled = os.environ.get("EBEN_PREPACK_GRAPH", "1") != "0"

    def __init__(self):
        self.graph, self.sig, self.rounds = None, None, 0
        _replayed.add(self)

    @staticmethod
    def _capture(body, stream_):
        """``body()`` recorded into a HIP graph on ``stream_`` (tests substitute a recorder)."""
        graph = torch.cuda.CUDAGraph()
        with _no_gc(), torch.cuda.graph(graph, stream=stream_, capture_error_mode="thread_local"):
            body()
        return graph

    def run(self, sig, body, stream_) -> bool:
        """Runs (or replays) ``body`` on ``stream_`` (a torch side stream, current on entry); True when it was a replay, in which
        case the caller refreshes its own cache keys (the body's bookkeeping did not run)."""
        if not self.enabled or eager_multi_rank():
            body()
            return False
        if sig != self.sig:
            self.graph, self.sig, self.rounds = None, sig, 0
        self.rounds += 1
        if self.graph is not None:
            self.graph.replay()
            return True
        graph = _try_capture(ReplayedPrepack, "prepack", body, stream_) if _capture_due(self, "prepack", self.rounds >= 3) else None
        if graph is None:
            body()
            return False
        self.graph = graph
        graph.replay()
        return False   # the body ran (under capture): its bookkeeping is current


class ReplayedChain:
    """Graph replay of one LINEAR launch sequence with device-side results (a sub-discriminator's forward body, stacked input
    gradients or weight gradients on its stream).  ``run(sig, fn, stream)`` returns what ``fn()`` returned -- tensors allocated by the
    body, which from the capture on live in the graph's pool and are REWRITTEN IN PLACE by every replay: valid until the next call.
    ``sig`` names everything the launches read besides values -- shapes, every input / weight-image / parameter address, arithmetic
    plan -- a new signature falls back to eager calls and, the second time in a row it is seen, a new capture.  Bodies chained
    through their results settle one after the other (the consumer's signature contains the producer's output addresses, which only
    stop changing once the producer replays).  One graph per chain and phase: no cross-stream edge inside a graph (the HIP runtime
    would serve parallel branches from extra hardware queues, see ``aux_stream``); events between chains stay outside."""

    enabled = os.environ.get("EBEN_CHAIN_GRAPHS", "1") != "0"
    #: graphs kept per chain, least recently used first out.  A run whose signature alternates -- variable clip lengths, a validation
    #: shape between train steps, ``update_discriminator_ratio < 1`` toggling ``want_param_grads`` -- replays each variant from its own
    #: graph instead of paying a capture (device-wide synchronisation, tens of ms) at every other change.  Each graph keeps its pool
    #: (the tensors its body allocates) for as long as it is cached: with KEEP variants alive a chain pins up to KEEP times its
    #: activation memory (~22 chains per step; config 2: ~1.5 GB per variant in total) -- lower it for runs over many clip lengths.
    KEEP = int(os.environ.get("EBEN_CHAIN_GRAPHS_KEEP", "4"))
    _generation = [0]

    def __init__(self):
        self.graph, self.sig, self.rounds, self.out = None, None, 0, None
        self.captures = 0   # names the generation of the tensors in ``out`` (unique per capture, restored on a cache hit)
        self._cache = {}    # signature -> (graph, out, generation), insertion order = recency
        self._seen = {}     # signature -> eager rounds so far (signatures that strictly alternate still reach their second round)
        _replayed.add(self)

    @staticmethod
    def _capture(fn, stream_):
        """(graph, what ``fn()`` returned while it was recorded) -- tests substitute a recorder.  stream_ None: torch's own capture
        stream (a sequence that normally runs on the default stream, which cannot capture); the replays are launched on whatever stream
        is current then."""
        graph = torch.cuda.CUDAGraph()
        with _no_gc(), torch.cuda.graph(graph, stream=stream_, capture_error_mode="thread_local"):
            out = fn()
        return graph, out

    def run(self, sig, fn, stream_):
        if not self.enabled or eager_multi_rank() or _timers_enabled():
            return fn()
        hit = self._cache.pop(sig, None)
        if hit is not None:
            self._cache[sig] = hit   # most recent
            self.graph, self.out, self.captures = hit
            self.sig = sig
            self.graph.replay()
            return self.out
        if sig != self.sig:
            self.graph, self.sig, self.out = None, sig, None
        self.rounds = self._seen.get(sig, 0) + 1
        self._seen[sig] = self.rounds
        while len(self._seen) > 4 * max(1, self.KEEP):   # bounded: forget the oldest signatures' counts
            self._seen.pop(next(iter(self._seen)))
        if not _capture_due(self, "chain", self.rounds >= 2):
            if self.rounds >= 2:
                self._seen[sig] = self.rounds = 1   # held at the threshold: the next sighting asks again
            return fn()
        captured = _try_capture(ReplayedChain, "chain", fn, stream_)
        if captured is None:
            return fn()
        graph, out = captured
        ReplayedChain._generation[0] += 1
        self.graph, self.out, self.captures = graph, out, ReplayedChain._generation[0]
        self._cache[sig] = (graph, out, self.captures)
        self._seen.pop(sig, None)
        while len(self._cache) > max(1, self.KEEP):
            self._cache.pop(next(iter(self._cache)))
        graph.replay()   # the capture recorded the launches without running them
        return out


def _timers_enabled() -> bool:
    return any(t.enabled for t in _timers)


def prepack(entries, graph: ReplayedPrepack, join: bool = True):
    """Rebuilds the packed weight images of one network on the side stream, right after its optimiser step: the ~2 tiny launches per
    layer leave the next forward's critical path and run underneath whatever the main stream does next.  entries: (cache,
    rebuild(slot)) per layer or fused unit (``conv_images``, ``GeneratorEngine.image_caches``, ``DiscriminatorEngine.image_caches``).
    One ``wn_scale_multi`` for every stale scale, then every slot the cache keeps (``PackedWeights.prune``) rebuilt into the buffers it
    occupies (conv images as one ``eben_conv1d_pack_multi``, fused-unit images as one ``eben_ru_pack_multi``), replayed by ``graph``
    once the sequence has settled.  Returns the event recorded behind it; ``join``: ``join_prepack`` waits for it (else the caller's
    streams do)."""
    global _prepacked
    entries = [(c, rebuild) for c, rebuild in entries if c.images or c.scale is not None]
    if not entries:
        return None
    dev = entries[0][0].params[0].device
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)   # the step that used the old images (and the optimiser that changed the weights) is complete

    def kept(c):
        return [s for s in c.images if s in c.used or not c.prune]

    def body():
        jobs = []
        for c, _ in entries:   # weight-norm scales of every layer: one multi-tensor launch
            key = weights_key(c.params)
            if c.scale_key != key:
                c.reuse = True
                jobs += c.wn_jobs()
                c.reuse = False
                c.scale_key = key
        wn_scale_multi(jobs)
        with pack_batch():
            for c, rebuild in entries:
                keep = kept(c)
                for slot in [s for s in c.images if s not in keep]:
                    del c.images[slot]   # a shape of an earlier step: rebuilt on demand if it comes back
                c.reuse = True
                try:
                    key = weights_key(c.params)
                    for slot in keep:
                        if not c.current(slot, key):
                            rebuild(slot)
                finally:
                    c.reuse = False
                c.used = set()   # re-packing is not a use: the next step decides what survives the next prepack

    # everything the launch sequence depends on besides the weights' values (ReplayedPrepack): the caches, the slots rebuilt, the
    # parameter storage, the buffers the launches write, and WHICH scales and images are stale (one skipped while capturing would never
    # be rebuilt by the replays)
    sig = tuple((id(c), c.state(kept(c)), len(kept(c)) == len(c.images)) for c, _ in entries) + (_storage_epoch.get(-1, 0),)
    with torch.cuda.stream(side), torch.no_grad():
        if graph.run(sig, body, side):
            for c, _ in entries:   # replayed: the images and scales are current, the cache keys are not
                key = weights_key(c.params)
                c.scale_key = key
                c.images = {slot: (key, img) for slot, (_, img) in c.images.items()}
                c.used = set()
        ev = torch.cuda.Event()
        ev.record()
    if join:
        _prepacked = ev
    return ev


_prepacked: Optional["torch.cuda.Event"] = None   # behind the latest ``prepack(join=True)`` until a consumer has waited for it


def join_prepack() -> None:
    """The current stream waits for the images `prepack` built (an event: later side-stream work is not waited for)."""
    global _prepacked
    if _prepacked is not None:
        ev, _prepacked = _prepacked, None
        torch.cuda.current_stream().wait_event(ev)


#: transposed convs with a fused output activation: mask the gradient by one element-wise launch so that the bf16 weight-gradient
#: kernel applies (see weight_grads)
PREMASK_TRANSPOSED_DW = os.environ.get("EBEN_PREMASK_DW", "1") != "0"


def dw_workspace(d: EbenConv1dDesc) -> tuple:
    """(bytes, slabs, row stride) of ``eben_conv1d_bwd_dw``'s workspace for this descriptor: asked once, kept on the descriptor."""
    ws = getattr(d, "_dw_ws", None)
    if ws is None:
        nslab, row_stride = ctypes.c_int(0), ctypes.c_int(0)
        ws = d._dw_ws = (load().eben_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(row_stride)), nslab.value, row_stride.value)
    return ws


def weight_grads(d: EbenConv1dDesc, dy: torch.Tensor, y: Optional[torch.Tensor], x: torch.Tensor, v: torch.Tensor,
                 g: Optional[torch.Tensor], bias: Optional[torch.Tensor], norm: Optional[torch.Tensor]):
    """Weight (+ bias) gradient of one conv layer: ``eben_conv1d_bwd_dw`` into split-K slabs, then the slab sum and the
    weight-norm chain rule.  dy: gradient at the layer output (``y``: the saved output when a fused output activation has to
    be differentiated, else None); x: the layer input; v / g / bias: the PARAMETERS (g, bias may be None); norm: ||v|| rows.
    Returns (dv, dg, dbias) -- or Nones for gradients that were deferred: inside ``weight_grads_on_side_stream()`` the work is
    issued on the side stream, and the results are either written straight into the sink's buckets (reported at ``join()``)
    or assigned to ``.grad`` by ``join()`` (never handed to autograd: it may clone what it is given, and the deferred
    kernels would then fill a tensor nobody reads)."""
    lib = load()
    use_side, outs, sunk = _wg_route(v, g, bias)
    premask = None
    if PREMASK_TRANSPOSED_DW and d.transposed and d.out_slope != 1.0 and y is not None and d.math in (MATH_BF16, MATH_BF16X2):
        # ConvTranspose1d with a fused output activation: the bf16 weight-gradient kernel takes no mask on that operand (the layer
        # would fall to the exact-fp32 kernel, 3-4x the time for the decoder's transposed convs) -- the masked gradient is formed by
        # one element-wise launch on the stream the weight gradient runs on, and the layer handed over as one without activation
        plain = getattr(d, "_dw_plain", None)
        if plain is None:
            plain = d._dw_plain = type(d).from_buffer_copy(d)
            plain.out_slope = 1.0
        premask, slope, d = (dy, y), d.out_slope, plain
    ws_bytes, nslab, row_stride = dw_workspace(d)
    # Every buffer is allocated on the CURRENT stream's pool; on the deferred path the kernels are launched on the side stream through
    # its raw handle (no torch stream switch) and everything they touch stays referenced until join(), after which the current
    # stream -- which waits for the side stream there -- may reuse it.
    slabs = _empty(ws_bytes, x)
    job = wn_job(slabs, nslab, row_stride, v, g, norm, outs)
    st = _wg_stream(use_side, x.device)
    if premask is not None:
        gm = torch.empty_like(dy)
        check(lib.eben_lrelu_bwd(ptr(dy), ptr(y), ptr(gm), dy.numel(), slope, st), "lrelu_bwd")
        dy, y = gm, None
    check(lib.eben_conv1d_bwd_dw(ctypes.byref(d), ptr(dy), ptr(y), ptr(x), 1 if bias is not None else 0, ptr(slabs), ws_bytes, st), "conv1d_bwd_dw")
    return _wg_finish(use_side, (dy, x, y, norm, slabs) + (premask or ()), [(job, (v, g, bias), sunk)])[0]


def grad_outputs(v, g, bias, sink=None, whole_layer: bool = False):
    """Where a layer's three weight gradients are written: ((dv, dg, dbias), sunk).  With a data-parallel ``sink`` (``ddp.GradSync``)
    p.grad is a view of a gradient bucket and the results go there directly, a parameter the sink holds no buffer for gets a fresh
    tensor; ``whole_layer``: the sink is used only when it has a buffer for every parameter of the layer.  sunk: every output is a
    view of the sink."""
    params = (v, g, bias)
    outs = [None if sink is None or p is None else sink.grad_buffer(p) for p in params]
    sunk = sink is not None and all(o is not None for p, o in zip(params, outs) if p is not None)
    if whole_layer and not sunk:
        outs = [None, None, None]
    dv, dg, dbias = outs
    if dv is None:
        dv = torch.empty_like(v)
    if dg is None and g is not None:
        dg = torch.empty_like(g)
    if dbias is None and bias is not None:
        dbias = torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    return (dv, dg, dbias), sunk


def add_logits_branches(params, gf, gr, sink=None):
    """Logits layer: the fake and the real branch are separate weight gradients, then added (into the sink's buffers, where it has
    them) -- the reference's structure (two autograd graphs accumulating into one .grad).  While every hinge term is active the
    two bias gradients are -c*N and +c*N summed in the SAME order, i.e. they cancel exactly and Adam leaves the bias alone; one sum
    over both branches leaves a rounding residue that Adam (m / sqrt(v)) turns into a full-size step."""
    outs, _ = grad_outputs(*params, sink)
    return tuple(None if a is None else torch.add(a, b, out=o) for a, b, o in zip(gf, gr, outs))


def _wg_route(v, g, bias):
    """Where a layer's weight gradients go: (issue on the side stream?, the outputs, are they bucket views of a data-parallel sink?)."""
    # The one place that turns (backward mode, parameter state) into a route.  A side scope defers a layer that may bypass autograd;
    # one that may not (data-parallel: every ``.grad`` is a bucket view) is deferred all the same where the sink takes all its results.
    side = _mode.route == ROUTE_SIDE
    use_side = side and isinstance(v, torch.nn.Parameter) and bypasses_autograd((v, g, bias), None)
    sink = None if use_side else _mode.sink
    outs, sunk = grad_outputs(v, g, bias, sink, whole_layer=True)
    if sink is not None:
        use_side = sunk and side   # collecting: the caller has made the producing stream current
    return use_side, outs, sunk


def bypasses_autograd(params, sink) -> bool:
    """May the gradients of ``params`` (None allowed) reach them behind autograd's back: each has a bucket view in ``sink``; without
    one, none holds a gradient that autograd would add to, or a hook that it would fire."""
    if sink is not None:
        return all(p is None or sink.grad_buffer(p) is not None for p in params)
    return all(p is None or (p.grad is None and _no_grad_hooks(p)) for p in params)


def _wg_stream(use_side: bool, device) -> int:
    """The raw handle of the stream a weight-gradient kernel is launched on: the current one, or the side stream behind it."""
    if not use_side:
        return stream()
    side = _side_stream(device, deal=True)
    side.wait_stream(torch.cuda.current_stream(device))   # dy (and everything saved by the forward) is complete on the main stream
    return side.cuda_stream


def _wg_finish(use_side: bool, keep: tuple, layers) -> list:
    """What follows the weight-gradient launch of ``layers`` = [(job, (v, g, bias), sunk)]: deferred (the slab sums and the weight-norm
    chain rule of ALL layers are one multi-tensor launch at join(), which also assigns or reports the results; ``keep`` is what the
    launch reads), collected by ``collect_wn_jobs``, or run here.  Returns (dv, dg, dbias) per layer, Nones where deferred."""
    jobs = [job for job, _, _ in layers]
    if use_side:
        _pending.defer(keep, jobs)
        for job, params, sunk in layers:
            pairs = [(p, t) for p, t in zip(params, (job.dv, job.dg, job.dbias)) if p is not None and t is not None]
            _pending.hand_over(pairs, _mode.sink if sunk else None)
        return [(None, None, None)] * len(layers)
    if _mode.route == ROUTE_COLLECT:
        _mode.jobs.extend(jobs)
    else:
        wn_bwd_multi(jobs)
    return [(job.dv, job.dg, job.dbias) for job in jobs]


def _weight_grads_unit(launch, what: str, c: int, nslab: int, device, keep: tuple, pw_params, dil_params):
    """Both weight gradients of a fused ResidualUnit of ``c`` channels by one launch ``launch(slabs_p, slabs_d, stream)`` that reads
    ``keep``: ``*_params`` = (v, g, norm) of the pointwise / dilated conv (weight-normalised, no bias).  Routed like ``weight_grads``
    (side stream / gradient buckets / immediate); returns False when the two layers would be routed differently, else a pair of
    (dv, dg, None) results -- Nones where deferred."""
    (vp, gp, np_), (vd, gd, nd) = pw_params, dil_params
    (use_side, outs_p, sunk_p), (side_d, outs_d, sunk_d) = _wg_route(vp, gp, None), _wg_route(vd, gd, None)
    if use_side != side_d or sunk_p != sunk_d:
        return False
    slabs_p = torch.empty(nslab * c * c, dtype=torch.float32, device=device)
    slabs_d = torch.empty(nslab * c * 3 * c, dtype=torch.float32, device=device)
    job_p = wn_job(slabs_p, nslab, c, vp, gp, np_, outs_p)
    job_d = wn_job(slabs_d, nslab, 3 * c, vd, gd, nd, outs_d)
    check(launch(ptr(slabs_p), ptr(slabs_d), _wg_stream(use_side, device)), what)
    return tuple(_wg_finish(use_side, keep + (np_, nd, slabs_p, slabs_d), [(job_p, (vp, gp, None), sunk_p), (job_d, (vd, gd, None), sunk_d)]))


def weight_grads_ru(math: int, dilation: int, gy: torch.Tensor, u: torch.Tensor, out_slope: float, h: torch.Tensor, gh: torch.Tensor,
                    x: torch.Tensor, in_slope: float, pw_params, dil_params):
    """Both weight gradients of a fused ResidualUnit in one launch (``eben_ru_dw``: the reduction runs along time, no packing
    pass); see ``_weight_grads_unit`` (False: the caller takes the per-layer path)."""
    lib = load()
    b, c, l = gy.shape
    launch = lambda sp, sd, st: lib.eben_ru_dw(math, b, c, l, dilation, ptr(gy), ptr(u), float(out_slope), ptr(h), ptr(gh), ptr(x), float(in_slope), sp, sd, st)
    return _weight_grads_unit(launch, "ru_dw", c, lib.eben_ru_dw_slabs(b, c, l), gy.device, (gy, u, h, gh, x), pw_params, dil_params)


def weight_grads_ru_bl(dilation: int, gzb: torch.Tensor, hb: torch.Tensor, ghb: torch.Tensor, xb: torch.Tensor, pw_params, dil_params):
    """``weight_grads_ru`` on the four bf16 bundle planes of a unit (``eben_rubl_dw``, csrc/ru_bl.hip): g_z and g_h as written by
    ``eben_rubl_bwd``, h and xin as saved by ``eben_rubl_fwd`` -- planes of shape (batch, C / 8, L, 8)."""
    lib = load()
    b, cb, l, _ = gzb.shape
    c = 8 * cb
    launch = lambda sp, sd, st: lib.eben_rubl_dw(b, c, l, dilation, gzb.data_ptr(), hb.data_ptr(), ghb.data_ptr(), xb.data_ptr(), sp, sd, st)
    return _weight_grads_unit(launch, "rubl_dw", c, lib.eben_rubl_dw_slabs(b, c, l), gzb.device, (gzb, hb, ghb, xb), pw_params, dil_params)


class _ConvLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, v, g, bias, spec: ConvSpec, cache):
        lib = load()
        x = x.contiguous()
        b, c, l_in = x.shape
        if c != spec.c_in:
            raise _lib.EbenError(f"conv expects {spec.c_in} input channels, got {c}")
        d = conv_desc(spec, b, l_in)
        d_bwd = conv_desc(spec, b, l_in, _mode.math) if _mode.math != MATH_F32 else d
        need_dx = ctx.needs_input_grad[0]
        pw = pack_weights(spec, d, v.detach(), None if g is None else g.detach(), cache, need_dx, d_bwd)
        y = torch.empty((b, spec.c_out, d.l_out), dtype=torch.float32, device=x.device)
        tm = kernel_timer_for(spec, "fwd")
        e0 = tm.start() if tm is not None else None
        check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(x), ptr(pw.wp_fwd), ptr(bias), None, ptr(y), stream()), "conv1d_fwd")
        if tm is not None:
            tm.stop(e0, b)
        ctx.spec, ctx.d = spec, d_bwd   # the descriptor the backward launches use
        ctx.wp_bwd, ctx.norm = pw.wp_bwd, pw.norm
        ctx.has_g, ctx.has_bias = g is not None, bias is not None
        # identities only: the gradient sink looks its bucket views up by parameter, join() assigns .grad to them
        ctx.bias_param = bias
        ctx.v_param = v if isinstance(v, torch.nn.Parameter) else None
        ctx.g_param = g if isinstance(g, torch.nn.Parameter) else None
        ctx.save_for_backward(x, v, g, y if spec.out_slope != 1.0 else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = load()
        x, v, g, y = ctx.saved_tensors
        spec, d = ctx.spec, ctx.d
        dy = dy.contiguous()
        st = stream()
        dx = dv = dg = dbias = None
        if ctx.needs_input_grad[0] and not _mode.skip_input_grads:
            ws_bytes = lib.eben_conv1d_bwd_dx_workspace(ctypes.byref(d))
            ws = _empty(ws_bytes, x) if ws_bytes else None
            dx = torch.empty_like(x)
            check(lib.eben_conv1d_bwd_dx(ctypes.byref(d), ptr(dy), ptr(y), ptr(ctx.wp_bwd), ptr(x), ptr(dx), 0, ptr(ws), ws_bytes, st),
                  "conv1d_bwd_dx")
        want_w = ctx.needs_input_grad[1] or (ctx.has_g and ctx.needs_input_grad[2]) or (ctx.has_bias and ctx.needs_input_grad[3])
        if want_w and not _mode.skip_weight_grads:
            dv, dg, dbias = weight_grads(d, dy, y, x, ctx.v_param if ctx.v_param is not None else v,
                                         (ctx.g_param if ctx.g_param is not None else g) if ctx.has_g else None,
                                         ctx.bias_param if ctx.has_bias else None, ctx.norm)
        return dx, dv, dg, dbias, None, None


def conv_layer(x: torch.Tensor, v: torch.Tensor, g: Optional[torch.Tensor], bias: Optional[torch.Tensor], spec: ConvSpec,
               cache: Optional[PackedWeights] = None) -> torch.Tensor:
    """lrelu_out(conv(lrelu_in(x); weight_norm(g, v)) + bias) with full autograd support."""
    return _ConvLayerFn.apply(x, v, g, bias, spec, cache)


# --------------------------------------------------------------------------------------------
# elementwise
# --------------------------------------------------------------------------------------------
class _LeakyReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope: float):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(load().eben_lrelu_fwd(ptr(x), ptr(y), x.numel(), slope, stream()), "lrelu_fwd")
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(load().eben_lrelu_bwd(ptr(dy), ptr(y), ptr(dx), dy.numel(), ctx.slope, stream()), "lrelu_bwd")
        return dx, None


def leaky_relu(x: torch.Tensor, slope: float) -> torch.Tensor:
    return _LeakyReluFn.apply(x, slope)


class _AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape:
            raise _lib.EbenError(f"add: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        out = torch.empty_like(a)
        check(load().eben_add(ptr(a), ptr(b), ptr(out), a.numel(), stream()), "add")
        return out

    @staticmethod
    def backward(ctx, dout):
        return dout, dout


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _AddFn.apply(a, b)


class _TanhLiftFn(torch.autograd.Function):
    """tanh(x + cat(lift, 0)) -- eben_generator.py:203-208; ``lift`` receives a gradient (the first channels of x's) only where it
    asks for one: the generator's input is data in training, and the first bands of an input that does require a gradient carry it."""

    @staticmethod
    def forward(ctx, x, lift):
        x, lift = x.contiguous(), lift.contiguous()
        b, c, l = x.shape
        out = torch.empty_like(x)
        check(load().eben_tanh_lift_fwd(ptr(x), ptr(lift), ptr(out), b, c, lift.shape[1], l, stream()), "tanh_lift_fwd")
        ctx.save_for_backward(out)
        ctx.lift_channels = lift.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(out)
        check(load().eben_tanh_bwd(ptr(dout), ptr(out), ptr(dx), out.numel(), stream()), "tanh_bwd")
        return dx, (dx[:, : ctx.lift_channels].clone() if ctx.needs_input_grad[1] else None)


def tanh_lift(x: torch.Tensor, lift: torch.Tensor) -> torch.Tensor:
    return _TanhLiftFn.apply(x, lift)


class _ReflectPadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad_l: int, pad_r: int):
        x = x.contiguous()
        b, c, l = x.shape
        y = torch.empty((b, c, l + pad_l + pad_r), dtype=torch.float32, device=x.device)
        check(load().eben_reflect_pad_fwd(ptr(x), ptr(y), b * c, l, pad_l, pad_r, stream()), "reflect_pad_fwd")
        ctx.geom = (b, c, l, pad_l, pad_r)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, c, l, pad_l, pad_r = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty((b, c, l), dtype=torch.float32, device=dy.device)
        check(load().eben_reflect_pad_bwd(ptr(dy), ptr(dx), b * c, l, pad_l, pad_r, stream()), "reflect_pad_bwd")
        return dx, None, None


def reflect_pad(x: torch.Tensor, pad_l: int, pad_r: int) -> torch.Tensor:
    return _ReflectPadFn.apply(x, pad_l, pad_r)


# --------------------------------------------------------------------------------------------
# FIR banks (PQMF, A-weighting)
# --------------------------------------------------------------------------------------------
def _fir_decimate(x, w, ly, bands, ntaps, stride, off0):
    b, _, lx = x.shape
    y = torch.empty((b, bands, ly), dtype=torch.float32, device=x.device)
    check(load().eben_fir_decimate(ptr(x), ptr(w), ptr(y), b, lx, ly, bands, ntaps, stride, off0, stream()), "fir_decimate")
    return y


def _fir_interp_sum(y, w, lx, bands, ntaps, stride, off0):
    b, _, ly = y.shape
    x = torch.empty((b, 1, lx), dtype=torch.float32, device=y.device)
    check(load().eben_fir_interp_sum(ptr(y), ptr(w), ptr(x), b, lx, ly, bands, ntaps, stride, off0, stream()), "fir_interp_sum")
    return x


class _FirDecimateFn(torch.autograd.Function):
    """y[b,k,t] = sum_j w[k,j] x[b,0,t*stride+off0+j]  (pqmf.py:194-202 with off0 = -(N-1))."""

    @staticmethod
    def forward(ctx, x, w, ly: int, stride: int, off0: int):
        x, w = x.contiguous(), w.contiguous()
        bands, ntaps = w.shape[0], w.shape[-1]
        ctx.geom = (x.shape[2], bands, ntaps, stride, off0)
        ctx.save_for_backward(w)
        return _fir_decimate(x, w, ly, bands, ntaps, stride, off0)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        lx, bands, ntaps, stride, off0 = ctx.geom
        dx = _fir_interp_sum(dy.contiguous(), w, lx, bands, ntaps, stride, off0) if ctx.needs_input_grad[0] else None
        return dx, None, None, None, None


class _FirInterpSumFn(torch.autograd.Function):
    """x[b,0,u] = sum_k sum_{t*stride+off0+j=u} w[k,j] y[b,k,t]  (pqmf.py:204-213 + band sum)."""

    @staticmethod
    def forward(ctx, y, w, lx: int, stride: int, off0: int):
        y, w = y.contiguous(), w.contiguous()
        bands, ntaps = w.shape[0], w.shape[-1]
        ctx.geom = (y.shape[2], bands, ntaps, stride, off0)
        ctx.save_for_backward(w)
        return _fir_interp_sum(y, w, lx, bands, ntaps, stride, off0)

    @staticmethod
    def backward(ctx, dx):
        (w,) = ctx.saved_tensors
        ly, bands, ntaps, stride, off0 = ctx.geom
        dy = _fir_decimate(dx.contiguous(), w, ly, bands, ntaps, stride, off0) if ctx.needs_input_grad[0] else None
        return dy, None, None, None, None


def fir_decimate(x, w, ly, stride, off0):
    return _FirDecimateFn.apply(x, w, ly, stride, off0)


def fir_interp_sum(y, w, lx, stride, off0):
    return _FirInterpSumFn.apply(y, w, lx, stride, off0)


# --------------------------------------------------------------------------------------------
# multi-rate downsampling (MelganMultiScalesDiscriminator: torchaudio Resample, "sinc_interp_kaiser")
# --------------------------------------------------------------------------------------------
_multirate_cache: Dict[tuple, object] = {}


def _kaiser_table(orig_freq: int, new_freq: int, device):
    """(kernels, width, orig, new) of Resample(orig_freq, new_freq, "sinc_interp_kaiser"), cached per (rates, device)."""
    key = ("kaiser", int(orig_freq), int(new_freq), device)
    if key not in _multirate_cache:
        from .augment import sinc_resample_kernel

        _multirate_cache[key] = sinc_resample_kernel(orig_freq, new_freq, device=device, resampling_method="sinc_interp_kaiser")
    return _multirate_cache[key]


def _fused_plan(sample_rate: int, scales: int, device):
    """Packed tables and widths of the fused path, or None when some scale does not reduce to new = 1 (orig = 2^s)."""
    key = ("fused", int(sample_rate), int(scales), device)
    if key not in _multirate_cache:
        plan = None
        if 2 <= scales <= 6 and all(_kaiser_table(sample_rate, sample_rate // 2 ** s, "cpu")[2:] == (2 ** s, 1) for s in range(1, scales)):
            tabs = [_kaiser_table(sample_rate, sample_rate // 2 ** s, "cpu") for s in range(1, scales)]
            packed = torch.cat([k.reshape(-1) for k, *_ in tabs]).to(device)
            plan = (packed, (ctypes.c_int * (scales - 1))(*[w for _, w, _, _ in tabs]))
        _multirate_cache[key] = plan
    return _multirate_cache[key]


class _MultirateFusedFn(torch.autograd.Function):
    """(x, A_1 x, ..., A_{S-1} x) for scales that all reduce to orig = 2^s, new = 1: one forward, one adjoint launch.
    The identity scale is returned as-is (autograd hands it back as a view of x) so that its gradient joins the adjoint."""

    @staticmethod
    def forward(ctx, x, plan, scales: int):
        packed, widths = plan
        lead, t = x.shape[:-1], x.shape[-1]
        rows = max(1, x.numel() // max(t, 1))
        x2 = x.contiguous()
        outs = [torch.empty((*lead, -(-t // 2 ** s)), dtype=torch.float32, device=x.device) for s in range(1, scales)]
        check(load().eben_multirate_down(ptr(x2), ptr(packed), widths, _ptr_array(outs), rows, t, scales, stream()), "multirate_down")
        ctx.geom = (plan, scales, rows, t, x.shape)
        return (x, *outs)

    @staticmethod
    def backward(ctx, g0, *gs):
        plan, scales, rows, t, shape = ctx.geom
        packed, widths = plan
        g0 = g0.contiguous()
        gs = [g.contiguous() for g in gs]
        dx = torch.empty(shape, dtype=torch.float32, device=g0.device)
        check(load().eben_multirate_down_adjoint(ptr(g0), _ptr_array(gs), ptr(packed), widths, ptr(dx), rows, t, scales, stream()),
              "multirate_down_adjoint")
        return dx, None, None


def _resample_fwd(x2, k, rows, t, t_out, orig, new, width):
    out = torch.empty((rows, t_out), dtype=torch.float32, device=x2.device)
    check(load().eben_resample(ptr(x2), ptr(k), ptr(out), rows, t, t_out, orig, new, width, stream()), "resample")
    return out


class _ResampleFn(torch.autograd.Function):
    """torchaudio _apply_sinc_resample_kernel for any reduced ratio orig : new: forward eben_resample, backward its adjoint."""

    @staticmethod
    def forward(ctx, x, table):
        k, width, orig, new = table
        lead, t = x.shape[:-1], x.shape[-1]
        rows = max(1, x.numel() // max(t, 1))
        t_out = -(-new * t // orig)
        ctx.geom = (table, rows, t, t_out, x.shape)
        return _resample_fwd(x.contiguous().reshape(rows, t), k, rows, t, t_out, orig, new, width).reshape(*lead, t_out)

    @staticmethod
    def backward(ctx, g):
        (k, width, orig, new), rows, t, t_out, shape = ctx.geom
        g = g.contiguous()
        dx = torch.empty(shape, dtype=torch.float32, device=g.device)
        check(load().eben_resample_adjoint(ptr(g), ptr(k), ptr(dx), rows, t, t_out, orig, new, width, 0, stream()), "resample_adjoint")
        return dx, None


def resample_adjoint(g: torch.Tensor, orig_freq: int, new_freq: int, t_in: int, accumulate_into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A^T g of kaiser_resample(., orig_freq, new_freq) for inputs of length t_in (dx += A^T g if accumulate_into is given)."""
    k, width, orig, new = _kaiser_table(orig_freq, new_freq, g.device)
    g = g.contiguous()
    rows, t_out = max(1, g.numel() // g.shape[-1]), g.shape[-1]
    dx = accumulate_into if accumulate_into is not None else torch.empty((*g.shape[:-1], t_in), dtype=torch.float32, device=g.device)
    check(load().eben_resample_adjoint(ptr(g), ptr(k), ptr(dx), rows, t_in, t_out, orig, new, width, int(accumulate_into is not None),
                                       stream()), "resample_adjoint")
    return dx


def kaiser_resample(x: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """torchaudio Resample(orig_freq, new_freq, resampling_method="sinc_interp_kaiser")(x), differentiable; x (..., time).
    orig == new returns x itself, as Resample.forward does."""
    if not x.is_cuda:
        ptr(x)   # raises: there is no CPU path
    if int(orig_freq) == int(new_freq):
        return x
    return _ResampleFn.apply(x, _kaiser_table(orig_freq, new_freq, x.device))


def multirate_downsample(x: torch.Tensor, sample_rate: int, scales: int) -> List[torch.Tensor]:
    """[Resample(sample_rate, sample_rate // 2**s, "sinc_interp_kaiser")(x) for s < scales] on the device, differentiable.

    When every ratio reduces to new = 1 (sample_rate divisible by 2^(scales-1)) all scales come from one fused forward launch and
    their gradients, the identity scale's included, go back through one fused adjoint launch; otherwise each scale runs the
    general rational path (eben_resample / eben_resample_adjoint).  Scale 0 is x itself (a view of it on the fused path)."""
    if not x.is_cuda:
        ptr(x)   # raises: there is no CPU path
    if scales < 1:
        raise ValueError(f"scales must be >= 1, got {scales}")
    if scales == 1:
        return [x]
    plan = _fused_plan(sample_rate, scales, x.device) if x.dtype is torch.float32 else None
    if plan is not None:
        return list(_MultirateFusedFn.apply(x, plan, scales))
    return [kaiser_resample(x, sample_rate, sample_rate // 2 ** s) for s in range(scales)]


# --------------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------------
def _ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t)
    return arr


class _FeatureLossFn(torch.autograd.Function):
    """sum_i mean|a_i-b_i| / mean|a_i| * inv_count  (feature_loss.py:37-50)."""

    @staticmethod
    def forward(ctx, inv_count: float, n_pairs: int, *tensors):
        lib = load()
        a = [t.contiguous() for t in tensors[:n_pairs]]
        b = [t.contiguous() for t in tensors[n_pairs:]]
        for ta, tb in zip(a, b):
            if ta.shape != tb.shape:
                raise _lib.EbenError(f"feature loss: shape mismatch {tuple(ta.shape)} vs {tuple(tb.shape)}")
        inter = [None] * (2 * n_pairs)
        inter[0::2], inter[1::2] = a, b
        ptrs = _ptr_array(inter)
        numel = (ctypes.c_int64 * n_pairs)(*[t.numel() for t in a])
        dev = a[0].device
        ws_bytes = lib.eben_fm_sums_workspace(n_pairs)
        ws = _empty(ws_bytes, a[0])
        sums = torch.empty(2 * n_pairs, dtype=torch.float32, device=dev)
        check(lib.eben_fm_sums(ptrs, numel, n_pairs, ptr(ws), ws_bytes, ptr(sums), stream()), "fm_sums")
        ctx.inv_count, ctx.n_pairs = inv_count, n_pairs
        ctx.save_for_backward(sums, *a, *b)
        return (sums[0::2] / sums[1::2]).sum() * inv_count

    @staticmethod
    def backward(ctx, gout):
        lib = load()
        n = ctx.n_pairs
        sums = ctx.saved_tensors[0]
        a, b = ctx.saved_tensors[1 : 1 + n], ctx.saved_tensors[1 + n :]
        inter = [None] * (2 * n)
        inter[0::2], inter[1::2] = a, b
        da = [torch.empty_like(t) for t in a]
        gout = gout.contiguous().reshape(1)
        check(lib.eben_fm_bwd(_ptr_array(inter), _ptr_array(da), (ctypes.c_int64 * n)(*[t.numel() for t in a]), n, ptr(sums),
                              ptr(gout), ctx.inv_count, stream()), "fm_bwd")
        return (None, None, *da, *([None] * n))


def last_conv_grad_norms(seeds: Sequence[torch.Tensor], bands: torch.Tensor, pre: torch.Tensor, conv) -> Optional[List[torch.Tensor]]:
    """||d L_i / d conv.weight|| for the seeds s_i = d L_i / d bands of the balancing losses in one pass over ``pre`` (``eben_last_conv_norms``:
    bands = tanh(conv(pre) + lift), eben.py:222-229 / eben_generator.py:159-166, 203-208); None when ``conv`` is not the layer that kernel is
    built for (then the caller differentiates through autograd).  Returns 0-dim views of one device vector."""
    sp = getattr(conv, "spec", None)
    if (sp is None or getattr(conv, "weight_norm", True) or conv.bias is not None or not (1 <= len(seeds) <= 4)
            or (sp.c_in, sp.c_out, sp.ksize, sp.stride, sp.dilation, sp.groups, sp.pad_l, sp.pad_r) != (32, 4, 3, 1, 1, 1, 1, 1) or not sp.reflect
            or sp.in_slope != 1.0 or sp.out_slope != 1.0 or pre.dtype is not torch.float32 or not pre.is_cuda):
        return None
    b, _, l = pre.shape
    lib = load()
    ts = [t.contiguous() for t in seeds]
    bands_c, pre_c = bands.detach().contiguous(), pre.detach().contiguous()
    nbytes = lib.eben_last_conv_norms_workspace(b)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=pre.device)
    out = torch.empty(len(ts), dtype=torch.float32, device=pre.device)
    check(lib.eben_last_conv_norms(_ptr_array(ts), len(ts), ptr(bands_c), ptr(pre_c), b, sp.c_in, sp.c_out, l, sp.ksize, sp.pad_l, ptr(ws), nbytes, ptr(out),
                                   stream()), "last_conv_norms")
    return [out[i] for i in range(len(ts))]


def weighted_sum(tensors: Sequence[torch.Tensor], weights: torch.Tensor) -> torch.Tensor:
    """sum_i weights[i] * tensors[i] (weights: device vector), torch's order and roundings, one launch (``eben_weighted_sum``)."""
    ts = [t.contiguous() for t in tensors]
    out = torch.empty_like(ts[0])
    check(load().eben_weighted_sum(_ptr_array(ts), ptr(weights), len(ts), out.numel(), ptr(out), stream()), "weighted_sum")
    return out


def feature_loss(emb_a: List[List[torch.Tensor]], emb_b: List[List[torch.Tensor]]) -> torch.Tensor:
    a = [t for scale in emb_a for t in scale[1:-1]]
    b = [t.detach() for scale in emb_b for t in scale[1:-1]]
    inv = 1.0 / (len(emb_a) * len(emb_a[-1][1:-1]))
    return _FeatureLossFn.apply(inv, len(a), *a, *b)


class _HingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target: float):
        x = x.contiguous()
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        check(load().eben_hinge_fwd(ptr(x), x.numel(), float(target), ptr(out), stream()), "hinge_fwd")
        ctx.target = float(target)
        ctx.save_for_backward(x)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        gout = gout.contiguous().reshape(1)
        check(load().eben_hinge_bwd(ptr(x), x.numel(), ctx.target, ptr(gout), 1.0, ptr(dx), stream()), "hinge_bwd")
        return dx, None


def hinge_mean(x: torch.Tensor, target: float) -> torch.Tensor:
    """mean(relu(1 - target*x)) -- hinge_loss.py:41."""
    return _HingeFn.apply(x, target)


#: loss values from their partial sums by one launch each (eben_stft_loss_total, eben_disc_losses) instead of one-element torch kernels
FUSED_LOSS_GLUE = os.environ.get("EBEN_FUSED_LOSS_GLUE", "1") != "0"


# --------------------------------------------------------------------------------------------
# per-row losses over ragged buffers (csrc/ragged_losses.hip): inference only, nothing here waits for the device
# --------------------------------------------------------------------------------------------
FILL_ZERO, FILL_MIRROR = 0, 1   # EBEN_FILL_* of include/eben_hip.h


def edge_fill(x: torch.Tensor, lens: torch.Tensor, mode: int, count: int) -> None:
    """``eben_edge_fill`` on (rows, channels, l_buf) ``x`` in place; ``lens``: (rows,) int32 on the device."""
    rows, channels, l_buf = x.shape
    check(load().eben_edge_fill(ptr(x), _iptr(lens), rows, channels, l_buf, mode, count, stream()), "edge_fill")


def _void_array(addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


def fm_sums_rows(pairs, rows: int) -> torch.Tensor:
    """(npairs, rows, 2) of (sum |a - b|, sum |a|) over each row's valid extent; ``pairs``: (a, b, lens) with a and b (rows, C, l_buf)
    and lens (rows,) int32 on the device.  At most 32 pairs."""
    lib, n = load(), len(pairs)
    addresses = []
    for a, b, lens in pairs:
        if a.shape != b.shape or a.dim() != 3 or a.shape[0] != rows or lens.numel() != rows:
            raise _lib.EbenError(f"fm_sums_rows: pair of {tuple(a.shape)} and {tuple(b.shape)} with {lens.numel()} lengths for {rows} rows")
        addresses += [ptr(a), ptr(b)]
    like = pairs[0][0]
    ws_bytes = lib.eben_fm_sums_rows_workspace(n, rows)
    ws = _empty(ws_bytes, like)
    sums = torch.empty((n, rows, 2), dtype=torch.float32, device=like.device)
    check(lib.eben_fm_sums_rows(_void_array(addresses), (ctypes.c_int * n)(*[a.shape[1] for a, _, _ in pairs]),
                                (ctypes.c_int * n)(*[a.shape[2] for a, _, _ in pairs]), _void_array([_iptr(lens) for _, _, lens in pairs]), n, rows,
                                ptr(ws), ws_bytes, ptr(sums), stream()), "fm_sums_rows")
    return sums


def hinge_rows(terms, rows: int) -> torch.Tensor:
    """(n, rows) of mean max(0, 1 - target x) over each row's valid extent; ``terms``: (x, target, lens) with x (rows, 1, l_buf) logits."""
    lib, n = load(), len(terms)
    for x, _, lens in terms:
        if x.dim() != 3 or x.shape[:2] != (rows, 1) or lens.numel() != rows:
            raise _lib.EbenError(f"hinge_rows: logits of {tuple(x.shape)} with {lens.numel()} lengths for {rows} rows")
    out = torch.empty((n, rows), dtype=torch.float32, device=terms[0][0].device)
    check(lib.eben_hinge_rows(_void_array([ptr(x) for x, _, _ in terms]), (ctypes.c_int * n)(*[x.shape[2] for x, _, _ in terms]),
                              (ctypes.c_float * n)(*[float(t) for _, t, _ in terms]), _void_array([_iptr(lens) for _, _, lens in terms]), n, rows,
                              ptr(out), stream()), "hinge_rows")
    return out


def clip_losses(rows: int, device, stft=None, fm=None, hinge=None) -> torch.Tensor:
    """(5, rows): per row [MRSTFT, feature matching, adv_loss_gen, real_loss, fake_loss] in one launch.  ``stft``: per resolution
    (sums (rows, 3), frames_of_row (rows,) int32, bins); ``fm``: (sums (npairs, rows, 2), inv_count); ``hinge``: (3 * chains, rows) with
    term 3 * chain + k, k = adv_loss_gen / real_loss / fake_loss.  A group left out yields NaN."""
    stft = list(stft or ())
    n = len(stft)
    out = torch.empty((5, rows), dtype=torch.float32, device=device)
    fm_sums, inv = fm if fm is not None else (None, 0.0)
    check(load().eben_clip_losses(_void_array([ptr(s) for s, _, _ in stft]) if n else None, _void_array([_iptr(f) for _, f, _ in stft]) if n else None,
                                  (ctypes.c_int * n)(*[int(b) for _, _, b in stft]) if n else None, n, ptr(fm_sums),
                                  fm_sums.shape[0] if fm_sums is not None else 0, float(inv), ptr(hinge), hinge.shape[0] // 3 if hinge is not None else 0,
                                  rows, ptr(out), stream()), "clip_losses")
    return out
