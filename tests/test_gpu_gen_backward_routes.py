"""GPU: every ResidualUnit route of the generator engine's backward (vibravox_amd/gen_engine.py: ``_residual_unit`` decides the route,
the reverse walk of the layer table runs it) at the smallest generator case of the suite -- ``build_generator(golden, 2)`` on
``formula_audio(.., 2, 8192)`` cut to a valid length: 32 samples at the deepest level, longer than the largest dilation (9), which the
reflect windows need.

Per route: the launches issued one by one against the CPU oracle, and the queued weight gradients behind replayed graphs against
the same launches issued one by one.  The routes are set as module attributes of ``gen_engine``, the backward arithmetic through
``ops.backward_math`` / ``EBENLightningModule.gen_backward_math``.
"""
import contextlib

import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests.test_gpu_models import BF16_STEP_TOLERANCES, DEV, build_generator, make_module, rel_l2

pytestmark = pytest.mark.gpu

#: route -> (gen_engine switches away from their defaults, arithmetic of the backward, the route every unit's record must name)
ROUTES = {
    "fused-f32": ({}, "f32", "fused"),                                     # fused forward, fused backward in six-piece math, fused dW
    "bundle-layout-bf16": ({}, "bf16", "bl"),                              # bf16 bundles + sign bytes at rest
    "fp32-at-rest-bf16": ({"USE_RU_BL": False}, "bf16", "fused"),          # fp32 at rest, fused bf16 backward, fused dW
    "dw-conv-by-conv": ({"USE_FUSED_RU_DW": False}, "f32", "fused"),       # fused forward and backward, weight gradients conv by conv
    "bwd-layer-by-layer": ({"USE_FUSED_RU_BWD": False}, "f32", "layers"),  # fused forward, layer-by-layer backward
    "fwd-layer-by-layer": ({"USE_FUSED_RU": False}, "f32", "fused"),       # layer-by-layer forward; the backward stays fused
}


@contextlib.contextmanager
def switched(switches, graphs):
    from vibravox_amd import gen_engine

    names = list(switches) + ["USE_GRAPHS"]
    prev = {k: getattr(gen_engine, k) for k in names}
    try:
        for k, v in dict(switches, USE_GRAPHS=graphs).items():
            setattr(gen_engine, k, v)
        yield
    finally:
        for k, v in prev.items():
            setattr(gen_engine, k, v)


_ORACLE = []


def oracle_grads(golden):
    """(input, loss weights, the CPU oracle's gradient per parameter) of the loss of test_generator_matches_oracle_and_reference_golden,
    computed once for all routes."""
    if not _ORACLE:
        _, osd = build_generator(golden, 2)
        x = O.cut_to_valid_length(formula_audio("g_in", 2, 8192))
        osd = {k: v.requires_grad_(not k.startswith("pqmf.")) for k, v in osd.items()}
        o_enh, o_bands = O.generator_forward(osd, x, 2)
        wgt = formula_audio("g_seed", 2, o_enh.shape[2], amp=1.0)
        ((o_enh * wgt).sum() + (o_bands ** 2).sum()).backward()
        _ORACLE.append((x, wgt, {k: v.grad.detach() for k, v in osd.items() if v.grad is not None}))
    return _ORACLE[0]


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_launch_by_launch_against_the_oracle(hip, golden, route):
    """Forward and backward launch by launch (no graphs, no queue: every weight gradient accumulated where its input gradient is
    taken) against the CPU oracle.  fp32 backward: test_generator_matches_oracle_and_reference_golden's own bar, 2e-3 relative L2 per
    tensor.  bf16 backward: BF16_STEP_TOLERANCES["generator_grad"] = 2e-2 on the whole gradient vector.

    [MI355X] measured on the hand-unrolled walk this test was written against, worst tensor / whole vector: fused-f32 1.23e-6 / 3.72e-7,
    bundle-layout-bf16 5.79e-3 / 2.01e-3, fp32-at-rest-bf16 5.79e-3 / 2.01e-3, dw-conv-by-conv 1.23e-6 / 3.71e-7, bwd-layer-by-layer
    1.31e-6 / 3.71e-7, fwd-layer-by-layer 1.26e-6 / 3.73e-7; the table walk gives the same figures.  Every unit's record names the
    route the switches ask for."""
    from vibravox_amd import ops

    switches, bwd, unit_route = ROUTES[route]
    x, wgt, ref = oracle_grads(golden)
    with switched(switches, graphs=False):
        gen, _ = build_generator(golden, 2)
        with ops.backward_math({"f32": ops.MATH_F32, "bf16": ops.MATH_BF16}[bwd]):
            enh, bands = gen(x.to(DEV))
            ((enh * wgt.to(DEV)).sum() + (bands ** 2).sum()).backward()
            records = gen._engine.forward(x.to(DEV), True)[2]
    torch.cuda.synchronize()
    assert [r.route for r in records if r.layer.kind == "unit"] == [unit_route] * 18
    grads = {k: p.grad for k, p in gen.named_parameters() if p.grad is not None}
    assert set(grads) == set(ref)
    worst = max(rel_l2(g, ref[k]) for k, g in grads.items())
    whole = rel_l2(torch.cat([grads[k].flatten() for k in grads]), torch.cat([ref[k].flatten() for k in grads]))
    print(f"route {route} ({bwd} backward) against the oracle: worst tensor {worst:.3e}, whole gradient vector {whole:.3e}")
    if bwd == "f32":
        assert worst < 2e-3, worst
    else:
        assert whole < BF16_STEP_TOLERANCES["generator_grad"], whole


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_queued_and_replayed_against_launch_by_launch(hip, golden, route):
    """Five train steps at 2 x 8200 with the route's weight gradients queued per backward group and both sequences replayed as HIP
    graphs, against the same steps launch by launch: bit-identical generator parameters, and forward + groups x (input gradients,
    weight gradients) sequences captured."""
    from vibravox_amd import gen_engine

    switches, bwd, _ = ROUTES[route]

    def run(graphs):
        with switched(switches, graphs):
            mod, _, _ = make_module(golden, use_mrstft=False)
            mod.gen_backward_math = bwd
            for i in range(5):
                mod.training_step({"audio_body_conducted": formula_audio(f"gg/{i}/bc", 2, 8200).to(DEV),
                                   "audio_airborne": formula_audio(f"gg/{i}/air", 2, 8200).to(DEV)})
            torch.cuda.synchronize()
            e = mod.generator._engine
            captured = sum(g.graph is not None for g in [e._fwd_graph] + e._dx_graphs + e._dw_graphs)
            return {k: v.detach().clone() for k, v in mod.generator.named_parameters()}, captured

    (a, cap_a), (b, cap_b) = run(True), run(False)
    groups = len([t for t in gen_engine.BWD_GROUPS.split(",") if t.strip()])
    assert (cap_a, cap_b) == (1 + 2 * groups, 0), (cap_a, cap_b)
    assert a and [k for k in a if not torch.equal(a[k], b[k])] == []
