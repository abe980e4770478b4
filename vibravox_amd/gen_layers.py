"""The EBEN generator's layers with taps along time, in launch order: the one place that turns the module tree into an order (host
only, no GPU needed).

``GeneratorEngine.forward`` launches the core entries one by one, ``ragged.plan`` derives its edge fills from their ``ConvSpec``s,
``streaming.nodes_of`` makes a stream node of each, and ``GeneratorEngine._stream_node`` finds a node's launch by its path.  The
training backward walks ``backward_segments``: the same entries in reverse, with where a skip's gradient leaves and rejoins the chain.
A change to the generator's shape -- another block, a different residual stack, a slope somewhere else -- is made here, for both.
"""
from __future__ import annotations

import dataclasses
import itertools
from typing import Optional, Tuple


@dataclasses.dataclass(frozen=True)
class Layer:
    path: str                  # module path: "first_conv", "encoder_blocks.1.residuals.2", "decoder_blocks.0.conv_trans", "last_conv", ...
    kind: str                  # "conv" | "unit" | "convT"
    module: object             # the HipConv1d, or the ResidualUnit for kind "unit"
    spec: object               # ConvSpec of the conv with taps along time: a unit is its dilated conv (the pointwise conv reads one
                               # sample, the residual add none)
    in_slope: float            # LeakyReLU applied on load (1.0: none)
    segment: Optional[tuple]   # the backward segment it belongs to (a run of equal values): ("misc",), ("enc", i), ("latent",), ("dec", i)
    add: Optional[int]         # index of the encoder output added to its input
    skip: Optional[int]        # its output is encoder output ``skip``
    core: bool                 # run by the engine; False: last_conv, which stays in autograd


def _build(gen) -> Tuple[Layer, ...]:
    slope, n_enc = gen.nl.negative_slope, len(gen.encoder_blocks)
    out = []

    def conv(path, m, segment, in_slope=1.0, add=None, skip=None, core=True):
        out.append(Layer(path, "convT" if m.spec.transposed else "conv", m, m.spec, in_slope, segment, add, skip, core))

    def units(path, blk, segment, first_slope):
        for k, ru in enumerate(blk.residuals):
            out.append(Layer(f"{path}.residuals.{k}", "unit", ru, ru.dilated_conv.spec, first_slope if k == 0 else 1.0, segment, None, None, True))

    conv("first_conv", gen.first_conv, ("misc",))
    for i, blk in enumerate(gen.encoder_blocks):   # the block's input activation rides on its first unit's load
        units(f"encoder_blocks.{i}", blk, ("enc", i), slope)
        conv(f"encoder_blocks.{i}.conv", blk.conv, ("enc", i), skip=i)
    conv("latent_conv.1", gen.latent_conv[1], ("latent",), in_slope=slope)   # latent_conv[0], the activation, on its load
    conv("latent_conv.3", gen.latent_conv[3], ("latent",))
    for i, blk in enumerate(gen.decoder_blocks):
        conv(f"decoder_blocks.{i}.conv_trans", blk.conv_trans, ("dec", i), add=n_enc - 1 - i)
        units(f"decoder_blocks.{i}", blk, ("dec", i), 1.0)
    conv("last_conv", gen.last_conv, None, core=False)
    return tuple(out)


def layers(gen) -> Tuple[Layer, ...]:
    """The table of ``gen``, built once and kept on it."""
    table = getattr(gen, "_layers", None)
    if table is None:
        table = _build(gen)
        object.__setattr__(gen, "_layers", table)   # not a submodule / buffer: invisible to state_dict
    return table


@dataclasses.dataclass(frozen=True)
class BackwardStep:
    layer: Layer
    dx: bool                   # its input needs a gradient; False: the input is data, only the weight gradient is taken
    joins: Optional[int]       # the gradient of encoder output ``joins`` (the layer in front made it) joins behind its activation mask: res_post
    yields: Optional[int]      # its input gradient is also the gradient of encoder output ``yields``, which it added to its input


def backward_segments(gen) -> Tuple[Tuple[BackwardStep, ...], ...]:
    """The backward of ``gen``'s core, built once and kept on it: the runs of equal ``Layer.segment`` last first, each a tuple of steps in
    launch order (its layers in reverse).  The run of the first layer alone, whose input is data, rides at the end of the last segment."""
    plan = getattr(gen, "_backward_segments", None)
    if plan is None:
        core = [la for la in layers(gen) if la.core]
        steps = [BackwardStep(la, i > 0, core[i - 1].skip if i else None, la.add) for i, la in enumerate(core)]
        plan = [tuple(run) for _, run in itertools.groupby(reversed(steps), key=lambda st: st.layer.segment)]
        if len(plan) > 1 and not any(st.dx for st in plan[-1]):   # nothing to hand on: its weight gradient closes the segment in front
            plan[-2:] = [plan[-2] + plan[-1]]
        plan = tuple(plan)
        object.__setattr__(gen, "_backward_segments", plan)
    return plan
