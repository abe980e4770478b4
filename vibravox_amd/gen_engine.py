"""Forward / backward of the EBEN generator's convolutional core as explicit kernel chains.

``EBENGenerator.forward`` (``vibravox/torch_modules/dnn/eben_generator.py:168-213``) is a chain of 45 small-channel conv
layers; through ``torch.autograd`` every ResidualUnit (:287-316) costs three launches and seven tensor passes forward
(dilated conv, pointwise conv, add) and, backward, two input-gradient launches, a reflect fold, two weight-gradient
launches and the adds autograd inserts where a gradient fans in.  This engine runs the core -- PQMF analysis, first conv,
encoder blocks, latent convs, decoder blocks: everything up to the input of ``last_conv`` -- outside autograd:

  * forward: one fused launch per ResidualUnit (``eben_ru_fwd``: x read once; h = dilated(x) and u = lrelu(pointwise(h)) kept
    for the backward), the shared LeakyReLU of the block inputs (:187-189) folded into that launch's tile staging;
  * backward: the reverse walk of the layer table (``gen_layers.backward_segments``) over the forward's records, one per core layer
    -- per step the input gradient, then the weight gradient.  Per ResidualUnit ``g_h = pointwise^T(g_y * lrelu'(u))`` and ``g_x =
    (g_y + fold(dilated^T(g_h))) * lrelu'(x) + skip`` -- the residual / skip joins ride in the reflect-fold pass
    (``eben_conv1d_bwd_dx_res``), no add kernel runs; the weight gradients are launched beside the input-gradient chain
    (``ops.weight_grads``: side stream, straight into ``.grad`` or the data-parallel buckets);
  * ``last_conv`` (the leaf of the loss balancing, eben.py:223), the tanh recomposition and the PQMF synthesis stay in
    autograd: the step differentiates them three extra times with ``retain_graph`` and they are cheap.

Arithmetic: the forward (training, evaluation and the exported output alike) runs on the bf16 matrix pipe with every fp32 operand
entering as three bf16 pieces (``RU_FWD_MATH`` / ``CONV_FWD_MATH`` = EBEN_MATH_BF16X6: six piece products, dropped terms <= 2^-26 of
a product, fp32 accumulation) -- fp32-grade, held by ``tests/test_gpu_ops.py`` to the fp32 MFMA kernels' own bound against fp64;
``EBEN_RU_FWD_MATH=f32 EBEN_GEN_CONV_FWD_MATH=f32`` selects the ``v_mfma_f32_*_f32`` kernels.  The module tree, parameters and
``state_dict`` are untouched -- this is only how ``EBENGenerator.forward`` executes.

The core's parameter gradients are produced by the engine as a side effect of ``backward`` (written to ``.grad`` / the data-parallel
buckets, never returned to autograd): ``torch.autograd.grad(loss, core parameters)`` returns nothing useful for them -- differentiate
with ``backward()`` and read ``.grad``, as the train step does (only ``last_conv``, outside the core, is reached through
``torch.autograd.grad``: eben.py:223-227).
"""
from __future__ import annotations

import ctypes
import dataclasses
import contextlib
import functools
import os
import weakref
from typing import Dict, List, Optional

import torch

from . import ops
from ._lib import check, load, ptr, stream
from .gen_layers import backward_segments, layers

USE_FUSED_RU = os.environ.get("EBEN_RU_FUSED", "1") != "0"
USE_FUSED_RU_BWD = os.environ.get("EBEN_RU_FUSED_BWD", "1") != "0"
USE_FUSED_RU_DW = os.environ.get("EBEN_RU_FUSED_DW", "1") != "0"
#: bf16 generator backward: the units' saved tensors at rest as bf16 bundles + sign bytes, written by the forward, and the bundle-layout
#: backward / weight-gradient launches (csrc/ru_bl.hip) -- 32 bytes per element and unit instead of 52-56
USE_RU_BL = os.environ.get("EBEN_RU_BL", "1") != "0"
#: data-parallel runs: report the generator's gradients to the bucket exchange at the join of its weight gradients instead of group by group
#: from the side stream (see DiscriminatorEngineBL.defer_mark_ready: a collective issued early waits on the communication stream and stalls
#: its hardware queue's other streams; [MI355X, single-rank RCCL] 9.18 -> 9.06 ms per step).  EBEN_G_DEFER_READY=0: the early form.
DEFER_MARK_READY = os.environ.get("EBEN_G_DEFER_READY", "1") != "0"
USE_GRAPHS = os.environ.get("EBEN_GEN_GRAPHS", "1") != "0"   # training forward / backward sequences replayed as HIP graphs
#: backward segments (3 decoder blocks, latent convs, 3 encoder blocks) per replayed graph.  A group's weight gradients start on the side
#: stream when its whole input-gradient graph has been issued, and what the main stream waits for in front of the generator's Adam is the
#: LAST group's weight gradients: one segment per graph keeps that tail at one encoder block ([MI355X, same box, 2 x alternated] "2,2,3"
#: 8.839 / 8.842, "2,2,2,1" 8.865 / 8.845, "3,3,1" 9.008 / 8.982, one per graph 8.795 / 8.809 ms per step; rounds 3-5 were bound by the host's
#: enqueue time -- a replay costs it ~70 us -- and ran "2,2,3")
BWD_GROUPS = os.environ.get("EBEN_GEN_BWD_GROUPS", "1,1,1,1,1,1,1")
# arithmetic of the fused ResidualUnit launches (include/eben_hip.h, eben_ru_*_ex): the forward and the fp32 backward run on the bf16
# matrix pipe with three bf16 pieces per operand (EBEN_MATH_BF16X6: every mantissa bit of the fp32 operands, fp32 accumulate --
# fp32 arithmetic at 6/16 of the fp32 MFMA's cost); "f32" selects the v_mfma_f32_32x32x2_f32 kernels (bisecting aid).
_RU_MATH = {"f32": ops.MATH_F32, "bf16x6": ops.MATH_BF16X6, "bf16x3": ops.MATH_BF16X3, "bf16": ops.MATH_BF16}
RU_FWD_MATH = _RU_MATH[os.environ.get("EBEN_RU_FWD_MATH", "bf16x6")]
# the arithmetic of the ResidualUnit forwards right now: EBENLightningModule's engine train step of the bf16-mixed plan runs inside
# ``forward_math("bf16x3")`` (hi + lo operands, three piece products; the weight images are cached per arithmetic and the prepack behind
# the optimiser step -- inside the same block -- rebuilds the ones of the step that just ran); everything outside a train step --
# validation, prediction, from_pretrained inference -- runs RU_FWD_MATH
_ru_fwd_math = [RU_FWD_MATH]


def ru_forward_math() -> int:
    return _ru_fwd_math[0]


def set_ru_forward_math(name=None) -> None:
    """``None`` restores the default (``EBEN_RU_FWD_MATH``, fp32-grade six-product arithmetic)."""
    _ru_fwd_math[0] = RU_FWD_MATH if name is None else _RU_MATH[name]
RU_BWD_F32_MATH = _RU_MATH[os.environ.get("EBEN_RU_BWD_F32_MATH", "bf16x6")]
# forward of the other conv layers of the core (first / strided / latent / transposed convs): the same fp32-grade split form
CONV_FWD_MATH = _RU_MATH[os.environ.get("EBEN_GEN_CONV_FWD_MATH", "bf16x6")]
_conv_fwd_math = [CONV_FWD_MATH]   # like _ru_fwd_math: the strided / transposed / latent convs of the generator


def conv_forward_math() -> int:
    return _conv_fwd_math[0]


def set_forward_math(name=None) -> None:
    """Arithmetic of the generator's forward from now on: ``"bf16x3"`` (hi + lo operands: the bf16-mixed plan) or ``None`` = the defaults
    (``EBEN_RU_FWD_MATH`` / ``EBEN_GEN_CONV_FWD_MATH``: fp32-grade six-product arithmetic)."""
    set_ru_forward_math(name)
    _conv_fwd_math[0] = CONV_FWD_MATH if name is None else _RU_MATH[name]


@contextlib.contextmanager
def forward_math(name=None):
    """``set_forward_math(name)`` for the duration of a ``with`` block, the previous arithmetic restored on exit (also on an exception):
    the train step of the bf16-mixed plan runs inside one, so that a validation / prediction forward of the same process computes in the
    default fp32-grade arithmetic whether or not a train step ran before it."""
    saved = (_ru_fwd_math[0], _conv_fwd_math[0])
    set_forward_math(name)
    try:
        yield
    finally:
        _ru_fwd_math[0], _conv_fwd_math[0] = saved


#: strided convs from this stride up run as space-to-depth + stride-1 tap-conv where the tap-conv does not cover them directly (0: never)
S2D_MIN_STRIDE = int(os.environ.get("EBEN_GEN_S2D_MIN_STRIDE", "8"))


def _params(m):
    return ops.conv_params(m)


class _ConvRec:
    """What the backward of one conv launch needs (``layer``: its table entry; None for the two convs inside a ``_UnitRec``)."""

    __slots__ = ("m", "spec", "d", "x", "y", "wp_bwd", "norm", "scale", "layer")

    def __init__(self, m, spec, d, x, y, wp_bwd, norm, scale=None, layer=None):
        self.m, self.spec, self.d, self.x, self.y, self.wp_bwd, self.norm, self.scale, self.layer = m, spec, d, x, y, wp_bwd, norm, scale, layer


class _UnitRec:
    """What the backward of one ResidualUnit needs: the records of its two convs and, by ``route``, "bl": the backward image ``img`` and
    the bf16 bundles ``xb`` / ``hb`` + sign bytes ``um`` (csrc/ru_bl.hip); "fused": ``img`` in arithmetic ``math``, x / h / u in the conv
    records; "layers": nothing more -- gradients conv by conv."""

    __slots__ = ("layer", "route", "dil", "pwc", "img", "math", "xb", "hb", "um")

    def __init__(self, layer, route, dil, pwc, img=None, math=None, xb=None, hb=None, um=None):
        self.layer, self.route, self.dil, self.pwc, self.img, self.math, self.xb, self.hb, self.um = layer, route, dil, pwc, img, math, xb, hb, um


class GeneratorEngine:
    def __init__(self, gen):
        self.gen = gen
        self._spec_cache: Dict[tuple, ops.ConvSpec] = {}
        self._ru_images: Dict[int, ops.PackedWeights] = {}   # id(ResidualUnit) -> its image cache
        self._s2d_images: Dict[int, tuple] = {}  # id(conv) -> (key, image of the space-to-depth form, permuted weights)
        # the training forward and, per backward segment, the input-gradient and the weight-gradient launches as replayed HIP graphs (ops.ReplayedChain)
        self._fwd_graph = ops.ReplayedChain()
        self._dx_graphs: List[ops.ReplayedChain] = []   # per backward segment (decoder block / latent / encoder block)
        self._dw_graphs: List[ops.ReplayedChain] = []
        self._static: Dict[tuple, torch.Tensor] = {}   # (name, shape) -> buffer the graphs read their per-step input from
        self._dwq: Optional[list] = None               # while the input-gradient chain runs in queue mode: its weight-gradient jobs
        self._serial, self._graph_serial, self._fwd_replayed, self._outstanding = 0, None, False, None   # forward_train's guard
        # the layer table (gen_layers.py): the core entries in launch order (= their slot in the records), every entry by its path, units, convs
        self._core = [la for la in layers(gen) if la.core]
        self._bwd = tuple(tuple((st, self._core.index(st.layer)) for st in seg) for seg in backward_segments(gen))   # (step, its record's slot)
        self._by_path = {la.path: la for la in layers(gen)}
        self._core_units = [la.module for la in self._core if la.kind == "unit"]
        self._core_convs = [m for la in self._core for m in ((la.module.dilated_conv, la.module.pointwise_conv) if la.kind == "unit" else (la.module,))]

    # ---- helpers ------------------------------------------------------------------------------------
    def _spec(self, m, in_slope=None, out_slope=None) -> ops.ConvSpec:
        if in_slope is None and out_slope is None:
            return m.spec
        key = (id(m), in_slope, out_slope)
        s = self._spec_cache.get(key)
        if s is None:
            kw = {}
            if in_slope is not None:
                kw["in_slope"] = float(in_slope)
            if out_slope is not None:
                kw["out_slope"] = float(out_slope)
            s = self._spec_cache[key] = dataclasses.replace(m.spec, **kw)
        return s

    def _pack(self, m, spec, batch, l_in, train):
        d = ops.conv_desc(spec, batch, l_in, conv_forward_math())   # layers the split bf16 tap-conv does not cover run their fp32 kernel
        d_bwd = ops.conv_desc(spec, batch, l_in, ops._mode.math)
        v, g = _params(m)
        pw = ops.pack_weights(m.spec, d, v.detach(), None if g is None else g.detach(), m._packed, train, d_bwd)
        return d, d_bwd, pw

    # ---- stride >= 8 as space-to-depth ---------------------------------------------------------------------------------------
    # The split-operand tap-conv stages the input tile of 128 outputs through a per-thread prefetch that a stride-8 layer's 1032
    # positions exceed: EncBlock's last strided conv and the input gradient of DecBlock's first transposed conv fell to the exact-fp32
    # kernel (0.15 ms each, the longest launches of the generator).  With the time axis folded into channels (`eben_space_to_depth`:
    # channel (c, r) = samples S q + r) the same contraction is a stride-1 conv with k / S taps over C S channels, which it covers.
    def _s2d_route(self, m, spec, batch: int, l_q: int, kq: int, math: int, c: int, rows_out: int, in_slope: float, out_slope: float, scale):
        """(descriptor, packed image) of the stride-1 form, or None when the tap-conv does not cover it either."""
        lib = load()
        alt = self._spec_cache.get((id(m), "s2d", in_slope, out_slope))
        if alt is None:
            alt = self._spec_cache[(id(m), "s2d", in_slope, out_slope)] = ops.ConvSpec(
                c_in=c * spec.stride, c_out=rows_out, ksize=kq, in_slope=float(in_slope), out_slope=float(out_slope))
        d = ops.conv_desc(alt, batch, l_q, math)
        if lib.eben_conv1d_kernel_generation(ctypes.byref(d), 0) != ops.CONV_ROUTE_TAP3:
            return None
        v, g = _params(m)
        key = ops.weights_key((v, g), batch, l_q, math)
        hit = self._s2d_images.get(id(m))
        if hit is None or hit[0] != key:
            vv = v.detach().view(rows_out, c, kq, spec.stride).permute(0, 1, 3, 2).reshape(rows_out, c * spec.stride, kq).contiguous()
            wp = torch.empty(lib.eben_conv1d_packed_floats(ctypes.byref(d), 0), dtype=torch.float32, device=v.device)
            ops.conv1d_pack(d, vv, scale, wp, None)
            hit = self._s2d_images[id(m)] = (key, wp, vv)
        return d, hit[1]

    @staticmethod
    def _s2d_wanted(spec, math: int) -> bool:
        return (S2D_MIN_STRIDE > 0 and spec.stride >= S2D_MIN_STRIDE and spec.ksize % spec.stride == 0 and spec.groups == 1
                and spec.dilation == 1 and math != ops.MATH_F32)

    def _conv(self, m, x, train, in_slope=None, recs=None, layer=None):
        """y = conv layer ``m`` on x (its own fused output activation; ``in_slope``: LeakyReLU on load); ``recs``: gets its record."""
        lib = load()
        spec = self._spec(m, in_slope=in_slope)
        b, _, l_in = x.shape
        d, d_bwd, pw = self._pack(m, spec, b, l_in, train)
        y = torch.empty((b, spec.c_out, d.l_out), dtype=torch.float32, device=x.device)
        route = None
        if not spec.transposed and self._s2d_wanted(spec, conv_forward_math()) and lib.eben_conv1d_kernel_generation(ctypes.byref(d), 0) not in (ops.CONV_ROUTE_TAP3, ops.CONV_ROUTE_GC):
            kq = spec.ksize // spec.stride
            l_q = d.l_out + kq - 1
            route = self._s2d_route(m, spec, b, l_q, kq, conv_forward_math(), spec.c_in, spec.c_out, spec.in_slope, spec.out_slope, pw.scale)
        if route is not None:
            xq = torch.empty((b, spec.c_in * spec.stride, l_q), dtype=torch.float32, device=x.device)
            check(lib.eben_space_to_depth(ptr(x), None, 1.0, ptr(xq), b * spec.c_in, l_in, spec.stride, -spec.pad_l, l_q,
                                          1 if spec.reflect else 0, stream()), "space_to_depth")
            check(lib.eben_conv1d_fwd(ctypes.byref(route[0]), ptr(xq), ptr(route[1]), ptr(m.bias), None, ptr(y), stream()), "conv1d_fwd")
        else:
            check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(x), ptr(pw.wp_fwd), ptr(m.bias), None, ptr(y), stream()), "conv1d_fwd")
        if recs is not None:
            recs.append(_ConvRec(m, spec, d_bwd, x, y if spec.out_slope != 1.0 else None, pw.wp_bwd, pw.norm, pw.scale, layer))
        return y

    @staticmethod
    def _ru_bwd_math() -> int:
        """Math of the fused backward launch: plain bf16 operands next to a bf16 generator backward (``ops.backward_math``), else
        the fp32-grade split."""
        return ops.MATH_BF16 if ops._mode.math != ops.MATH_F32 else RU_BWD_F32_MATH

    def _ru_cache(self, ru) -> ops.PackedWeights:
        c = self._ru_images.get(id(ru))
        if c is None:
            c = self._ru_images[id(ru)] = ops.PackedWeights()
        c.params = _params(ru.dilated_conv) + _params(ru.pointwise_conv)
        return c

    def _ru_image(self, ru, which: int = 0) -> torch.Tensor:
        """Weight images of the fused unit (both convs, weight-norm scales folded in): 0 forward, 1 backward (transposed, in the
        math of the current backward).  Slots: ("fwd", forward math) and ("bwd", math) per backward math."""
        c = self._ru_cache(ru)
        slot = ("fwd", ru_forward_math()) if which == 0 else ("bwd", self._ru_bwd_math())
        if not c.current(slot, ops.weights_key(c.params)):
            self._ru_rebuild(ru, c, slot)
        return c.images[slot][1]

    def _ru_rebuild(self, ru, c: ops.PackedWeights, slot) -> None:
        """Builds image ``slot``.  When the forward image is not current (a parameter or the forward math changed), the weight-norm
        scales, the forward image and the backward image of every math this unit has been differentiated in are rebuilt with it (so
        that ``ops.prepack``, which runs outside the step's math context, rebuilds the right ones); inside it (``c.reuse``) the scales
        are current already and the images go into the buffers held."""
        lib = load()
        vd, _, vp, _ = c.params
        vd, vp = vd.detach(), vp.detach()
        ch = vd.shape[0]
        key = ops.weights_key(c.params)
        fwd = ("fwd", ru_forward_math())
        slots = [slot]
        if not c.current(fwd, key):
            if not c.reuse:
                c.scale_key = None
                c.ensure_scale()
            old, c.images = c.images, {}
            bwd = [s for s in old if s[0] == "bwd"]
            slots = [fwd] + bwd + ([slot] if slot != fwd and slot not in bwd else [])
        else:
            old = c.images
        for s in slots:
            hit = old.get(s)
            img = c.buffer(None if hit is None else hit[1], lib.eben_ru_packed_floats_ex(ch, s[1]), vd)
            ops.ru_pack(ch, s[1], 0 if s[0] == "fwd" else 1, vd, c.scale[0], vp, c.scale[2], img)
            c.images[s] = (key, img)

    def image_caches(self) -> list:
        """``ops.prepack`` entries of the fused units that hold images."""
        return [(c, lambda slot, ru=ru, c=c: self._ru_rebuild(ru, c, slot))
                for ru in self._core_units if (c := self._ru_images.get(id(ru))) is not None and c.images]

    def _residual_unit(self, ru, x, in_slope, train, recs, layer=None):
        """y = xin + lrelu(pointwise(dilated(xin))), xin = lrelu(x, in_slope).  Returns y; ``recs`` gets the ``_UnitRec`` of the route."""
        lib = load()
        b, c, l = x.shape
        dil, pwc = ru.dilated_conv, ru.pointwise_conv
        if train:
            # the backward images of the two convs (and their weight-norm norms) come from the per-layer caches
            spec_d = self._spec(dil, in_slope=in_slope if in_slope != 1.0 else None)
            _, dd_bwd, pw_d = self._pack(dil, spec_d, b, l, True)
            _, dp_bwd, pw_p = self._pack(pwc, pwc.spec, b, l, True)
        fwd_math = ru_forward_math()
        fusable = dil.spec.ksize == 3 and dil.spec.reflect and lib.eben_ru_supported(c, dil.spec.dilation, fwd_math) == 1
        if (train and USE_RU_BL and USE_FUSED_RU and USE_FUSED_RU_BWD and USE_FUSED_RU_DW and fusable and fwd_math in (ops.MATH_BF16X6, ops.MATH_BF16X3)
                and self._ru_bwd_math() == ops.MATH_BF16 and lib.eben_rubl_supported(c, dil.spec.dilation) == 1 and self._ru_bl_params_ok(ru, l)):
            # what the bf16 backward reads, written once in the layout its MFMA operands want (csrc/ru_bl.hip)
            img = self._ru_image(ru)
            y = torch.empty_like(x)
            xb = torch.empty((b, c // 8, l, 8), dtype=torch.bfloat16, device=x.device)
            hb = torch.empty_like(xb)
            um = torch.empty((b, c // 8, l), dtype=torch.uint8, device=x.device)
            check(lib.eben_rubl_fwd(fwd_math, b, c, l, dil.spec.dilation, ptr(x), float(in_slope), float(pwc.spec.out_slope), ptr(img), ptr(y),
                                    xb.data_ptr(), hb.data_ptr(), um.data_ptr(), stream()), "rubl_fwd")
            recs.append(_UnitRec(layer, "bl", _ConvRec(dil, spec_d, dd_bwd, x if in_slope != 1.0 else None, None, pw_d.wp_bwd, pw_d.norm),
                                 _ConvRec(pwc, pwc.spec, dp_bwd, None, None, pw_p.wp_bwd, pw_p.norm), self._ru_image(ru, 1), xb=xb, hb=hb, um=um))
            return y
        if USE_FUSED_RU and fusable:
            img = self._ru_image(ru)
            y = torch.empty_like(x)
            h = torch.empty_like(x) if train else None
            u = torch.empty_like(x) if train else None
            check(lib.eben_ru_fwd_ex(fwd_math, b, c, l, dil.spec.dilation, ptr(x), float(in_slope), float(pwc.spec.out_slope), ptr(img), ptr(y),
                                     ptr(h), ptr(u), stream()), "ru_fwd")
        else:   # layer by layer (bisecting aid, EBEN_RU_FUSED=0)
            xin = x
            if in_slope != 1.0:
                xin = torch.empty_like(x)
                check(lib.eben_lrelu_fwd(ptr(x), ptr(xin), x.numel(), float(in_slope), stream()), "lrelu_fwd")
            h = self._conv(dil, xin, train)
            u = self._conv(pwc, h, train)
            y = torch.empty_like(x)
            check(lib.eben_add(ptr(xin), ptr(u), ptr(y), x.numel(), stream()), "add")
        if train:
            bm = self._ru_bwd_math()
            fused = USE_FUSED_RU_BWD and dil.spec.ksize == 3 and dil.spec.reflect and lib.eben_ru_supported(c, dil.spec.dilation, bm) == 1
            dil_rec, pwc_rec = _ConvRec(dil, spec_d, dd_bwd, x, None, pw_d.wp_bwd, pw_d.norm), _ConvRec(pwc, pwc.spec, dp_bwd, h, u, pw_p.wp_bwd, pw_p.norm)
            recs.append(_UnitRec(layer, "fused", dil_rec, pwc_rec, self._ru_image(ru, 1), bm) if fused else _UnitRec(layer, "layers", dil_rec, pwc_rec))
        return y

    # ---- forward -------------------------------------------------------------------------------------
    def _launch(self, layer, x, train, recs):
        """Entry ``layer`` of the table on its input: the unit's fused launch, or the conv's; ``recs``: gets the layer's record."""
        if layer.kind == "unit":
            return self._residual_unit(layer.module, x, layer.in_slope, train, recs, layer)
        return self._conv(layer.module, x, train, in_slope=layer.in_slope if layer.in_slope != 1.0 else None, recs=recs, layer=layer)

    def forward(self, cut_audio: torch.Tensor, train: bool, fill=None):
        """Returns (input of last_conv, first_bands, the records for ``backward`` -- one per core layer, in table order -- or None).
        ``fill(layer path, x)``, inference only: called on the input of every layer with taps along time right before its launch
        (``forward_ragged`` writes the rows' own edges there)."""
        gen = self.gen
        lib = load()
        ops.join_prepack()   # images rebuilt ahead of time on the side stream
        first_bands = gen.pqmf(cut_audio, "analysis", bands=gen.p).detach()
        saved = [] if train else None
        x, skips = first_bands, {}
        for layer in self._core:
            if layer.add is not None:
                s = torch.empty_like(x)
                check(lib.eben_add(ptr(x), ptr(skips[layer.add]), ptr(s), x.numel(), stream()), "add")
                x = s
            if fill is not None:
                fill(layer.path, x)
            x = self._launch(layer, x, train, saved)
            if layer.skip is not None:
                skips[layer.skip] = x
        return x, first_bands, saved

    # ---- ragged batches: rows of different lengths, inference only (vibravox_amd/ragged.py) ---------------------------------------
    @staticmethod
    def _edge_fill(x: torch.Tensor, table: torch.Tensor, f) -> None:
        """Fill ``f`` of the plan on ``x`` in place; ``table``: the plan's row lengths on the device, (resolutions, rows) int32."""
        rows, channels, l_buf = x.shape
        lens = table.data_ptr() + 4 * rows * f.level
        if f.mode == "zero_all":
            check(load().eben_edge_zero(ptr(x), lens, rows, channels, l_buf, stream()), "edge_zero")
        else:
            check(load().eben_edge_fill(ptr(x), lens, rows, channels, l_buf, 1 if f.mode == "mirror" else 0, f.count, stream()), "edge_fill")

    def forward_ragged(self, padded_audio: torch.Tensor, plan):
        """(enhanced (B,1,l_buf), bands (B,m,l_buf of the bands)) of zero-padded rows of ``plan.cut`` samples each, every row equal to its
        own batch-1 forward on [0, its length) and zero behind: ``forward(.., train=False)`` launch for launch, with the plan's edge fill
        in front of each layer.  Equal rows need no fill: the call is the batched forward.  Inference only (no backward exists)."""
        if torch.is_grad_enabled():
            raise RuntimeError("EBEN generator engine: forward_ragged has no backward; call it under torch.no_grad()")
        gen = self.gen
        b, c, l = padded_audio.shape
        if c != 1 or b != len(plan.cut) or l != plan.l_buf:
            raise ValueError(f"forward_ragged: expected a ({len(plan.cut)}, 1, {plan.l_buf}) buffer for this plan, got {tuple(padded_audio.shape)}")
        x = padded_audio.contiguous()
        if not plan.fills:
            pre, first_bands, _ = self.forward(x, False)
            bands = ops.tanh_lift(gen.last_conv(pre), first_bands)
            return gen.pqmf.synthesis_sum(bands), bands
        table = torch.tensor(plan.row_lengths, dtype=torch.int32).to(x.device, non_blocking=True)   # the one upload of the batch
        todo = iter(plan.fills)

        def fill(path, t):
            f = next(todo)
            if f.layer != path or t.shape[2] != plan.buffer_lengths[f.level]:
                raise RuntimeError(f"ragged plan out of step with the forward: {f} in front of {path} on {tuple(t.shape)}")
            self._edge_fill(t, table, f)

        if x is padded_audio:
            x = x.clone()   # the caller's buffer stays as it is
        fill("pqmf.analysis", x)
        pre, first_bands, _ = self.forward(x, False, fill)
        fill("last_conv", pre)
        bands = ops.tanh_lift(gen.last_conv(pre), first_bands)
        fill("pqmf.synthesis", bands)
        enhanced = gen.pqmf.synthesis_sum(bands)
        fill("enhanced", enhanced)
        return enhanced, bands

    # ---- streaming: one push of a stream schedule, inference only (vibravox_amd/streaming.py) -----------------------------------------
    def stream_state(self, plan, streams: int, device) -> "StreamState":
        """The plan's state tensors for ``streams`` rows on ``device``: two buffers per tensor, allocated here once."""
        return StreamState(plan, streams, device)

    def _stream_node(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """Node ``name`` of the stream on its buffer: the launch ``forward(.., train=False)`` makes for that layer."""
        gen = self.gen
        if name == "pqmf.analysis":
            return gen.pqmf(x, "analysis", bands=gen.p)
        if name == "pqmf.synthesis":
            return gen.pqmf.synthesis_sum(x)
        if name == "last_conv":
            return gen.last_conv(x)
        return self._launch(self._by_path[name], x, False, None)

    def _stream_launch(self, state: "StreamState", op, outs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """One ``streaming.Launch`` on every row of ``state``: the node's output."""
        if op.node == "lift":
            y = ops.tanh_lift(outs["last_conv"], state.view("lift.operand"))
        else:
            x = state.view(op.node)
            if x.shape[2] != op.l_in:
                raise RuntimeError(f"stream state out of step with the schedule: {op} on a buffer of {x.shape[2]}")
            y = self._stream_node(op.node, x)
        if y.shape[2] != op.l_out:
            raise RuntimeError(f"stream schedule out of step with the kernels: {op} gave {y.shape[2]} samples")
        return y

    def _stream_ops(self, state: "StreamState", operations, chunk, emit_rows: int, splice) -> Dict[str, torch.Tensor]:
        """The operations of one push on ``state``; returns the tensors emitted (``emit_rows`` rows each), by output name.  Every layer is
        launched as ``forward`` launches it; ``splice(op, kind, key, dst, total, prev, src, add, channels)`` launches a splice."""
        from .streaming import Splice

        ops.join_prepack()
        outs: Dict[str, torch.Tensor] = {}
        emitted: Dict[str, torch.Tensor] = {}

        def operand(name):
            if name is None:
                return None
            if name == "input":
                return chunk
            kind, key = name.split(":", 1)
            return outs[key] if kind == "out" else state.view(key)

        for op in operations:
            if not isinstance(op, Splice):
                outs[op.node] = self._stream_launch(state, op, outs)
                continue
            total = op.n_carry + op.n_new
            kind, key = op.dst.split(":", 1)
            if total == 0:
                state.length[key] = 0
                continue
            prev, src, add = operand(op.prev), operand(op.src), operand(op.add)
            channels = (prev if prev is not None else src).shape[1]
            if kind == "emit":
                dst = emitted[key] = torch.empty((emit_rows, channels, total), dtype=torch.float32, device=state.device)
            else:
                dst = state.twin(key, total)
            splice(op, kind, key, dst, total, prev, src, add, channels)
            if kind == "tape":
                state.flip(key, total)
        return emitted

    def stream_run(self, state: "StreamState", operations, chunk: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Executes one push's operations (``streaming.Schedule.push``) on ``state``; returns the tensors emitted, by output name.
        Every input is spliced by ``eben_stream_splice`` and every layer launched as ``forward`` launches it; nothing waits."""
        if torch.is_grad_enabled():
            raise RuntimeError("EBEN generator engine: stream_run has no backward; call it under torch.no_grad()")
        lib = load()
        rows = state.rows
        pitch = lambda t: 0 if t is None else t.shape[2]

        def splice(op, kind, key, dst, total, prev, src, add, channels):
            check(lib.eben_stream_splice(ptr(dst), total, ptr(prev), pitch(prev), op.prev_off, op.n_carry, ptr(src), pitch(src), op.src_off, op.n_new,
                                         ptr(add), pitch(add), op.add_off, rows * channels, stream()), "stream_splice")

        return self._stream_ops(state, operations, chunk, rows, splice)

    def stream_run_pooled(self, state: "StreamState", steady, chunks: torch.Tensor, mask, n_active: int) -> Dict[str, torch.Tensor]:
        """One steady-state push (``plan.steady``) of the slots whose bit is set in ``mask`` (64-bit words), on the shared ``state`` of a
        ``streaming.StreamPool``.  ``chunks``: the ``n_active`` pushed chunks in slot order, one row each.  Every layer runs over all
        slots as in ``stream_run``; every splice is an ``eben_stream_splice_rows``: the analysis tape reads the compact input, every
        tape that holds state carries its idle slots over to the twin buffer, and the emits come back compact, a row per active slot
        in slot order."""
        if torch.is_grad_enabled():
            raise RuntimeError("EBEN generator engine: stream_run_pooled has no backward; call it under torch.no_grad()")
        if tuple(chunks.shape[:2]) != (n_active, 1) or n_active != sum(bin(w).count("1") for w in mask) or n_active < 1:
            raise ValueError(f"stream_run_pooled: {tuple(chunks.shape)} chunks for {n_active} active slots of mask {mask}")
        lib = load()
        rows = state.rows
        words = (ctypes.c_uint64 * 4)(*mask)
        pitch = lambda t: 0 if t is None else t.shape[2]

        def splice(op, kind, key, dst, total, prev, src, add, channels):
            idle = None
            if kind == "tape" and key != "lift.operand":   # the lift's operand is rewritten whole from another tape every push: it holds no state
                idle = state.view(key)
                if idle.shape[2] != total:
                    raise RuntimeError(f"pool state out of step with the steady list: {op} on a buffer of {idle.shape[2]}")
            check(lib.eben_stream_splice_rows(ptr(dst), total, ptr(prev), pitch(prev), op.prev_off, op.n_carry, ptr(src), pitch(src), op.src_off,
                                              op.n_new, ptr(add), pitch(add), op.add_off, ptr(idle), pitch(idle), rows * channels, channels, words,
                                              1 if op.src == "input" else 0, 1 if kind == "emit" else 0, stream()), "stream_splice_rows")

        return self._stream_ops(state, steady, chunks, n_active, splice)

    def stream_move(self, pool: "StreamState", slot: int, private: "StreamState", names, into_pool: bool) -> None:
        """A session's steady-state buffers (tensors ``names`` of the plan) between the batch-1 state ``private`` and row ``slot`` of the
        shared state ``pool``: a (channels, length) block is contiguous on both sides, so it is one ``eben_copy_segments`` launch per
        64 tensors.  Out of the pool, ``private`` is set to the steady lengths first."""
        from ._lib import EbenCopySegment

        if not 0 <= slot < pool.rows or private.rows != 1:
            raise ValueError(f"stream_move: slot {slot} of {pool.rows}, a private state of {private.rows} rows")
        lib = load()
        lengths = pool.steady_lengths
        if not into_pool:
            private.reset()
            for name in names:
                private.length[name] = lengths[name]
        table = []
        for name in names:   # addresses by arithmetic: building ~40 pairs of tensor views costs more host time than the launch
            n = lengths[name]
            if private.length[name] != n or pool.length[name] != n:
                raise RuntimeError(f"stream_move: {name} holds {private.length[name]} and {pool.length[name]} samples, its steady length is {n}")
            mine, row = private.address(name, 0), pool.address(name, slot)
            table.append(EbenCopySegment(row, mine, pool.channels[name] * n) if into_pool else EbenCopySegment(mine, row, pool.channels[name] * n))
        for i in range(0, len(table), 64):
            part = table[i : i + 64]
            check(lib.eben_copy_segments((EbenCopySegment * len(part))(*part), len(part), stream()), "copy_segments")

    # ---- backward ------------------------------------------------------------------------------------
    def _dx(self, rec: _ConvRec, dy, res_pre=None, res_post=None):
        lib = load()
        d = rec.d
        spec = rec.spec
        if (spec.transposed and res_pre is None and res_post is None and spec.in_slope == 1.0 and spec.output_padding == 0
                and self._s2d_wanted(spec, d.math) and lib.eben_conv1d_kernel_generation(ctypes.byref(d), 1) != ops.CONV_ROUTE_TAP3):
            # input gradient of ConvTranspose1d = stride-S conv of the (masked) output gradient with the same (in, out, k) weights
            b, c_dy, l_dy = dy.shape
            kq = spec.ksize // spec.stride
            l_q = rec.x.shape[2] + kq - 1
            route = self._s2d_route(rec.m, spec, b, l_q, kq, d.math, c_dy, spec.c_in, 1.0, 1.0, rec.scale)
            if route is not None:
                gq = torch.empty((b, c_dy * spec.stride, l_q), dtype=torch.float32, device=dy.device)
                check(lib.eben_space_to_depth(ptr(dy), ptr(rec.y) if spec.out_slope != 1.0 else None, spec.out_slope, ptr(gq), b * c_dy, l_dy,
                                              spec.stride, -spec.pad_l, l_q, 0, stream()), "space_to_depth")
                dx = torch.empty_like(rec.x)
                check(lib.eben_conv1d_fwd(ctypes.byref(route[0]), ptr(gq), ptr(route[1]), None, None, ptr(dx), stream()), "conv1d_fwd")
                return dx
        ws_bytes = getattr(d, "_dx_ws", None)
        if ws_bytes is None:
            ws_bytes = d._dx_ws = lib.eben_conv1d_bwd_dx_workspace(ctypes.byref(d))
        ws = ops._empty(ws_bytes, dy) if ws_bytes else None
        dx = torch.empty_like(rec.x)
        xmask = rec.x if rec.spec.in_slope != 1.0 else None
        check(lib.eben_conv1d_bwd_dx_res(ctypes.byref(d), ptr(dy), ptr(rec.y), ptr(rec.wp_bwd), ptr(xmask), ptr(res_pre), ptr(res_post), ptr(dx),
                                         ptr(ws), ws_bytes, stream()), "conv1d_bwd_dx_res")
        return dx

    def _emit_dw(self, grads, *operands) -> None:
        """One record's weight gradients, ``grads(*operands, trainable_only=..) -> [(parameter, gradient)]``: not wanted, queued for
        ``_dw_body`` while ``backward_train``'s input-gradient chain runs, or accumulated now.  The queue runs only where ``_deferrable()``
        found every core parameter trainable and routed alike: there ``grads`` launches without looking (``trainable_only=False``) and a
        bundle-layout unit it cannot serve is that check's bug, an assertion; launch by launch it is the user's pattern, an error."""
        if ops._mode.skip_weight_grads:
            return
        job = functools.partial(grads, *operands)
        if self._dwq is not None:
            self._dwq.append(job)
        else:
            for p, t in job(trainable_only=True):   # not deferred (no side-stream context): accumulate like autograd would
                if p is not None and t is not None and p.requires_grad:
                    ops.accumulate_grad(p, t, hooks=True)

    def _conv_dw(self, rec: _ConvRec, dy, trainable_only: bool) -> list:
        return self._conv_grads(rec, dy) if not trainable_only or _params(rec.m)[0].requires_grad else []

    def _unit_dw_bl(self, dil: _ConvRec, pwc: _ConvRec, gzb, hb, ghb, xb, trainable_only: bool) -> list:
        res = self._unit_grads_bl(dil, pwc, gzb, hb, ghb, xb)
        if res is False:
            assert trainable_only   # launch by launch
            raise RuntimeError("bundle-layout ResidualUnit: the two convs' weight gradients are routed differently (one of them holds a gradient "
                               "or a hook the other does not); set EBEN_RU_BL=0 for this pattern")
        return res

    @staticmethod
    def _conv_grads(rec: _ConvRec, dy) -> list:
        """One conv's weight gradients as (parameter, gradient) pairs; none for what was deferred."""
        v, g = _params(rec.m)
        grads = ops.weight_grads(rec.d, dy, rec.y, rec.x, v, g, rec.m.bias, rec.norm)
        return [(p, t) for p, t in zip((v, g, rec.m.bias), grads) if p is not None and t is not None]

    @staticmethod
    def _unit_pairs(dil: _ConvRec, pwc: _ConvRec, res) -> list:
        """(parameter, gradient) pairs of ``ops.weight_grads_ru`` / ``weight_grads_ru_bl``'s result for the unit's two convs."""
        return list(zip(_params(pwc.m), res[0][:2])) + list(zip(_params(dil.m), res[1][:2]))

    def _unit_grads(self, dil: _ConvRec, pwc: _ConvRec, gy, gh, bm: int, trainable_only: bool) -> list:
        """Weight gradients of both convs of a fused unit as (parameter, gradient) pairs: one ``eben_ru_dw`` launch (reduction along
        time, operands straight from the activation tensors) where both are weight-normalised bias-free parameters, else layer by
        layer.  ``trainable_only``: nothing is launched for a conv that does not require a gradient."""
        (vd, gd), (vp, gp) = _params(dil.m), _params(pwc.m)
        wanted = lambda *ps: not trainable_only or all(p.requires_grad for p in ps)
        if (USE_FUSED_RU_DW and gd is not None and gp is not None and dil.m.bias is None and pwc.m.bias is None and wanted(vd, vp, gd, gp)
                and bm in (ops.MATH_BF16, ops.MATH_BF16X6)):
            res = ops.weight_grads_ru(bm, dil.spec.dilation, gy, pwc.y, float(pwc.spec.out_slope), pwc.x, gh, dil.x, float(dil.spec.in_slope),
                                      (vp, gp, pwc.norm), (vd, gd, dil.norm))
            if res is not False:
                return self._unit_pairs(dil, pwc, res)
        return [pair for rec, dy in ((pwc, gy), (dil, gh)) if wanted(_params(rec.m)[0]) for pair in self._conv_grads(rec, dy)]

    def _unit_grads_bl(self, dil: _ConvRec, pwc: _ConvRec, gzb, hb, ghb, xb):
        """``_unit_grads`` of a bundle-layout unit (``eben_rubl_dw``); False where its two convs are routed differently."""
        (vd, gd), (vp, gp) = _params(dil.m), _params(pwc.m)
        res = ops.weight_grads_ru_bl(dil.spec.dilation, gzb, hb, ghb, xb, (vp, gp, pwc.norm), (vd, gd, dil.norm))
        return False if res is False else self._unit_pairs(dil, pwc, res)

    @staticmethod
    def _ru_bl_params_ok(ru, length: int) -> bool:
        """The bundle-layout weight-gradient launch serves weight-normalised, bias-free, trainable convs (every unit of the reference) whose
        gradients take the SAME route (both or neither hold a gradient / carry a hook: the unit's two weight gradients are one launch) on
        rows longer than the dilation (the kernels' reflect window); anything else keeps the fp32-at-rest path, which can fall back conv
        by conv -- the bundle path saves only bf16 planes and cannot."""
        keys = []
        for m in (ru.dilated_conv, ru.pointwise_conv):
            v, g = _params(m)
            if g is None or m.bias is not None or not (v.requires_grad and g.requires_grad):
                return False
            keys.append((v.grad is None and g.grad is None, ops._no_grad_hooks(v) and ops._no_grad_hooks(g)))
        return keys[0] == keys[1] and ru.dilated_conv.spec.dilation < length

    def _ru_backward(self, rec: _UnitRec, gy, res_post=None):
        dil, pwc, ins = rec.dil, rec.pwc, rec.dil.spec.in_slope
        b, c, l = gy.shape
        if rec.route == "bl":
            gx = torch.empty_like(gy)
            gzb, ghb = torch.empty_like(rec.xb), torch.empty_like(rec.xb)
            check(load().eben_rubl_bwd(b, c, l, dil.spec.dilation, ptr(gy), rec.um.data_ptr(), float(pwc.spec.out_slope), ptr(dil.x) if ins != 1.0 else None,
                                       float(ins), ptr(res_post), ptr(rec.img), ptr(gx), gzb.data_ptr(), ghb.data_ptr(), stream()), "rubl_bwd")
            self._emit_dw(self._unit_dw_bl, dil, pwc, gzb, rec.hb, ghb, rec.xb)
            return gx
        if rec.route == "fused":   # one launch: g_h and g_x = (g_y + fold(dilated^T g_h)) * lrelu'(x) + skip gradient
            gx, gh = torch.empty_like(gy), torch.empty_like(gy)
            check(load().eben_ru_bwd_ex(rec.math, b, c, l, dil.spec.dilation, ptr(gy), ptr(pwc.y), float(pwc.spec.out_slope),
                                        ptr(dil.x) if ins != 1.0 else None, float(ins), ptr(res_post), ptr(rec.img), ptr(gx), ptr(gh), stream()), "ru_bwd")
            self._emit_dw(self._unit_grads, dil, pwc, gy, gh, rec.math)
            return gx
        gh = self._dx(pwc, gy)                       # pointwise^T(gy * lrelu'(u))
        self._emit_dw(self._conv_dw, pwc, gy)
        gx = self._dx(dil, gh, res_pre=gy, res_post=res_post)   # (gy + fold(dilated^T gh)) * lrelu'(x) + skip gradient
        self._emit_dw(self._conv_dw, dil, gh)
        return gx

    def _n_segments(self) -> int:
        return len(self._bwd)

    def _bwd_segment(self, saved, k: int, g: torch.Tensor, skip_grads: dict) -> torch.Tensor:
        """Segment k of the backward plan (``gen_layers.backward_segments``) on the forward's records: takes the gradient at the segment's
        output, returns the one at its input.  Per step the input gradient, then the weight gradient.  ``skip_grads``: the gradients of
        the encoder outputs by their index, filed by the step that added one to its input, read by the one that consumed it."""
        for step, slot in self._bwd[k]:
            rec = saved[slot]
            if rec.layer is not step.layer:
                raise RuntimeError(f"EBEN generator engine: the record of {rec.layer.path} stands where the backward expects {step.layer.path}")
            post = None if step.joins is None else skip_grads[step.joins]   # joins behind the layer's activation mask
            if step.layer.kind == "unit":
                g = self._ru_backward(rec, g, res_post=post)
            else:
                dy = g
                if step.dx:                           # False: its input is data, only the weight gradient
                    g = self._dx(rec, dy, res_post=post)
                self._emit_dw(self._conv_dw, rec, dy)
            if step.yields is not None:
                skip_grads[step.yields] = g
        return g

    @torch.no_grad()
    def backward(self, saved, g_pre: torch.Tensor) -> None:
        """Input-gradient chain on the current stream, weight gradients through ``ops.weight_grads`` (inside
        ``ops.weight_grads_on_side_stream()``: beside the chain, joined by the caller)."""
        g = g_pre.contiguous()
        skip_grads: Dict[int, torch.Tensor] = {}
        for k in range(self._n_segments()):
            g = self._bwd_segment(saved, k, g, skip_grads)

    # ---- the training step's three launch sequences as replayed graphs ----------------------------------------------------------
    # ~36 launches forward, ~50 along the input-gradient chain and ~30 weight-gradient launches per step, each a few microseconds of
    # GPU-side dispatch but 15-30 us of Python + ctypes on the host: 1.2 + 2.2 + 0.5 ms of host time per step ([MI355X]
    # tools/host_times.py) on a 12 ms step whose host side took 11.3 ms in all.  Every per-step input is copied into a static
    # buffer, every tensor the bodies allocate lives in the graph's pool (rewritten in place by the next replay: valid until then,
    # which is as long as the step needs it), and the weight images are the ones ops.prepack rebuilds in place.
    @staticmethod
    def _graphs_usable() -> bool:
        return USE_GRAPHS and ops.ReplayedChain.enabled and not ops.eager_multi_rank() and not ops._timers_enabled()

    def _static_buf(self, name: str, like: torch.Tensor) -> torch.Tensor:
        key = (name, tuple(like.shape), like.dtype, like.device)
        buf = self._static.get(key)
        if buf is None:
            if len(self._static) >= 8:   # variable clip lengths: keep the buffers of the recent shapes only
                self._static.pop(next(iter(self._static)))
            buf = self._static[key] = torch.empty_like(like, memory_format=torch.contiguous_format)
        return buf

    def _fwd_sig(self, buf: torch.Tensor) -> tuple:
        """Everything the captured forward depends on besides values: input buffer, arithmetic, and per layer and fused unit the image
        cache's buffers and whether they are current (a stale image makes the eager path rebuild it -- a replay would not)."""
        parts = [buf.data_ptr(), tuple(buf.shape), ops._mode.math, conv_forward_math(), ru_forward_math()]
        parts += [m._packed.state() for m in self._core_convs]
        parts += [None if (c := self._ru_images.get(id(ru))) is None else c.state() for ru in self._core_units]
        return tuple(parts)

    def forward_train(self, x: torch.Tensor):
        """``forward(x, True)``, replayed as a graph once the sequence has settled.

        A replay REWRITES the outputs and saved activations of the previous replay in place.  Plain PyTorch semantics -- two
        grad-enabled forwards, then a backward through both -- therefore need a guard: every call gets a serial number; while the
        latest replayed forward has not been differentiated (and its autograd node is still alive) the next forward runs eagerly on
        fresh tensors, and ``backward_train`` refuses saved state whose serial is no longer the graph's (a second backward with
        ``retain_graph`` after a newer replay) instead of returning gradients of the wrong forward."""
        self._fwd_replayed = False
        self._serial += 1
        if not self._graphs_usable() or self._replay_outstanding():
            return self.forward(x, True)
        ops.join_prepack()   # the wait stays outside the graph
        buf = self._static_buf("x", x)
        buf.copy_(x)
        out = self._fwd_graph.run(self._fwd_sig(buf), lambda: self.forward(buf, True), None)
        self._fwd_replayed = self._fwd_graph.graph is not None
        if self._fwd_replayed:
            self._graph_serial = self._serial   # whose forward the graph's buffers hold
        return out

    def _replay_outstanding(self) -> bool:
        """The graph's buffers hold a forward that an autograd node still alive has not been differentiated through."""
        ref = self._outstanding
        if ref is None:
            return False
        if ref() is None:
            self._outstanding = None
            return False
        return True

    def _note_ctx(self, ctx) -> None:
        ctx.serial = self._serial
        self._outstanding = weakref.ref(ctx) if self._fwd_replayed else None

    def _deferrable(self) -> bool:
        """Weight gradients of the whole core go through ``weight_grads_on_side_stream().join()``'s assignment (no gradient held, no
        hook) or, data-parallel, straight into the sink's bucket views: the test ``ops._wg_route`` applies layer by layer."""
        mode = ops._mode
        if mode.route != ops.ROUTE_SIDE or mode.skip_weight_grads:
            return False
        params = [p for m in self._core_convs for p in _params(m) + (m.bias,) if p is not None]
        return all(p.requires_grad for p in params) and ops.bypasses_autograd(params, mode.sink)

    def _dw_body(self, queue: list, sink=None) -> list:
        """The queued weight-gradient work on the current stream: every layer's kernel, then ONE slab-sum / weight-norm launch.
        Returns [(parameter, gradient)] (with a data-parallel ``sink``: the gradients are its bucket views)."""
        jobs, assign = [], []
        with ops.collect_wn_jobs(jobs, sink):
            for job in queue:
                assign += job(trainable_only=False)   # the queued form: see _emit_dw
        ops.wn_bwd_multi(jobs)
        return assign

    @torch.no_grad()
    def backward_train(self, saved, g_pre: torch.Tensor, serial: Optional[int] = None) -> None:
        """``backward(saved, g_pre)``; behind a replayed forward and inside ``ops.weight_grads_on_side_stream()``: per segment (decoder
        block / latent convs / encoder block) the input-gradient launches as one graph on the current stream and the segment's
        weight-gradient launches as one graph on the side stream behind it -- the weight gradients of segment k run beside the
        input-gradient chain of segment k + 1, as the launch-by-launch schedule has them.  Results are assigned by the context's
        ``join()``.  ([MI355X] as two graphs -- the whole chain, then all weight gradients -- the step went 12.0 -> 12.5 ms: the chain
        alone fills a fraction of the GPU.)"""
        from_graph = self._fwd_graph.out is not None and saved is self._fwd_graph.out[2]
        if from_graph and serial is not None and serial != self._graph_serial:
            raise RuntimeError("EBEN generator engine: this forward's saved activations were rewritten by a later replayed forward (backward "
                               "through an old graph after a new training forward); set EBEN_GEN_GRAPHS=0 for that pattern")
        self._outstanding = None   # differentiated: the next forward may replay over these buffers
        if not (self._graphs_usable() and self._fwd_replayed and from_graph and self._deferrable()):
            return self.backward(saved, g_pre)
        gbuf = self._static_buf("g", g_pre)
        gbuf.copy_(g_pre)
        n = self._n_segments()
        # segments per graph: a replay costs ~70 us of host time, a graph per segment (14 replays) 1.35 ms per step against 0.74 for two
        # graphs; three groups keep the weight gradients beside the chain at 0.5 ms
        sizes = [int(t) for t in BWD_GROUPS.split(",")] if BWD_GROUPS else []
        if sum(sizes) != n:
            sizes = [1] * n
        bounds = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
        while len(self._dx_graphs) < len(sizes):
            self._dx_graphs.append(ops.ReplayedChain())
            self._dw_graphs.append(ops.ReplayedChain())
        dev = gbuf.device
        main = torch.cuda.current_stream(dev)
        side = ops._side_stream(dev)
        g, skip_grads = gbuf, {}
        for k in range(len(sizes)):
            def dx_body(k=k, g=g):
                self._dwq = []
                sk = dict(skip_grads)
                try:
                    out = g
                    for seg in range(bounds[k], bounds[k + 1]):
                        out = self._bwd_segment(saved, seg, out, sk)
                finally:
                    queue, self._dwq = self._dwq, None
                return out, {j: t for j, t in sk.items() if j not in skip_grads}, queue

            # one signature for all segments: they settle, and are captured, in the same step, each on the results of the one before
            g, new_skips, queue = self._dx_graphs[k].run((self._fwd_graph.captures, gbuf.data_ptr(), ops._mode.math), dx_body, None)
            skip_grads.update(new_skips)
            if not queue:
                continue
            side.wait_stream(main)
            sink = ops._mode.sink
            with torch.cuda.stream(side):
                graphed = self._dx_graphs[k].graph is not None
                if graphed:
                    assign = self._dw_graphs[k].run((self._dx_graphs[k].captures, id(sink)), lambda: self._dw_body(queue, sink), side)
                else:
                    assign = self._dw_body(queue, sink)
                # data-parallel: this group's gradients sit in their bucket views once the side stream has run the launches above.  They
                # are reported by join(), from the main stream, once it has waited for the side stream -- or (early) from THIS stream now
                # (GradSync.mark_ready records its event on the current stream), so that a bucket filled by an early group is exchanged
                # underneath the later groups' input-gradient chain instead of behind join().  keep: eager tensors, referenced until join()
                ops.hand_over(assign, sink, early=not DEFER_MARK_READY, keep=None if graphed else queue)


class StreamState:
    """Device state of one ``StreamingEnhancer``: per tensor of the plan two flat buffers of ``capacity`` samples per (row, channel) --
    a splice reads one and writes the other -- and the length the current one holds, as a contiguous (rows, channels, length) view."""

    def __init__(self, plan, streams: int, device):
        self.plan, self.rows = plan, int(streams)
        self.device = torch.empty(0, device=device).device   # with its index, as tensors report it
        self.channels = {t.name: t.channels for t in plan.tensors}
        self.capacity = {t.name: t.capacity for t in plan.tensors}
        self.buffers = {t.name: [torch.empty(self.rows * t.channels * t.capacity, dtype=torch.float32, device=self.device) for _ in range(2)]
                        for t in plan.tensors}
        self.base = {name: [t.data_ptr() for t in pair] for name, pair in self.buffers.items()}
        self.steady_lengths = {t.name: t.length for t in plan.tensors}
        self.reset()

    def reset(self) -> None:
        self.current = {name: 0 for name in self.buffers}
        self.length = {name: 0 for name in self.buffers}

    def _shaped(self, name: str, which: int, length: int) -> torch.Tensor:
        c = self.channels[name]
        return self.buffers[name][which][: self.rows * c * length].view(self.rows, c, length)

    def view(self, name: str) -> torch.Tensor:
        return self._shaped(name, self.current[name], self.length[name])

    def address(self, name: str, row: int) -> int:
        """Device address of row ``row`` of the current view: its (channels, length) block is contiguous."""
        return self.base[name][self.current[name]] + 4 * row * self.channels[name] * self.length[name]

    def twin(self, name: str, length: int) -> torch.Tensor:
        """The buffer a splice writes: the one the current view does not live in."""
        if length > self.capacity[name]:
            raise RuntimeError(f"stream state: {name} needs {length} samples, the plan allots {self.capacity[name]}")
        return self._shaped(name, 1 - self.current[name], length)

    def flip(self, name: str, length: int) -> None:
        self.current[name], self.length[name] = 1 - self.current[name], length


class _CoreFn(torch.autograd.Function):
    """The engine behind autograd: outputs (input of last_conv, first_bands); the parameters are arguments only so that the
    graph knows the output depends on them -- their gradients are produced by the engine, not returned."""

    @staticmethod
    def forward(ctx, x, engine, *params):
        pre, first_bands, saved = engine.forward_train(x)
        ctx.engine, ctx.saved = engine, saved
        engine._note_ctx(ctx)
        # fresh tensor objects: behind a replayed forward `pre` is the SAME object every step, and autograd writes this call's history
        # into what it is handed
        pre, first_bands = pre.detach(), first_bands.detach()
        ctx.mark_non_differentiable(first_bands)
        return pre, first_bands

    @staticmethod
    def backward(ctx, g_pre, _g_fb):
        ctx.engine.backward_train(ctx.saved, g_pre, getattr(ctx, "serial", None))
        return (None, None) + (None,) * (len(ctx.needs_input_grad) - 2)


def engine_of(gen) -> GeneratorEngine:
    engine = getattr(gen, "_engine", None)
    if engine is None:
        engine = GeneratorEngine(gen)
        object.__setattr__(gen, "_engine", engine)   # not a submodule / buffer: invisible to state_dict
    return engine


def core(gen, cut_audio: torch.Tensor):
    """(input of ``gen.last_conv``, first_bands) through the engine; differentiable w.r.t. the generator's parameters."""
    engine = engine_of(gen)
    # the parameters the core owns: NOT last_conv's -- the balancing passes differentiate the losses w.r.t. last_conv.weight alone
    # (eben.py:223-227) and must not reach into the core
    params = [p for m in (gen.first_conv, gen.encoder_blocks, gen.latent_conv, gen.decoder_blocks) for p in ops.parameters_of(m) if p.requires_grad]
    if torch.is_grad_enabled() and params:
        return _CoreFn.apply(cut_audio.contiguous(), engine, *params)
    pre, first_bands, _ = engine.forward(cut_audio.contiguous(), False)
    return pre, first_bands
