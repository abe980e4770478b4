"""CPU: the generator's layer table (vibravox_amd/gen_layers.py), which the engine's forward, the ragged plan and the stream nodes
all read, against the module tree and against the ragged plan's fills (every layer of these generators has a reach > 0 -- the table in
DESIGN.md -- so the plan of two unequal clips names every layer, in launch order)."""
import pytest

from vibravox_amd import ragged
from vibravox_amd.gen_layers import backward_segments, layers
from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator, ResidualUnit
from vibravox_amd.torch_modules.utils import HipConv1d


@pytest.fixture(scope="module", params=[(32, 1), (32, 2), (512, 2)], ids=lambda np_: f"n{np_[0]}-p{np_[1]}")
def gen(request):
    n, p = request.param
    return EBENGenerator(4, n, p)


def test_the_table_is_built_once_and_stays_out_of_the_state_dict(gen):
    keys = set(gen.state_dict())
    table = layers(gen)
    assert layers(gen) is table and isinstance(table, tuple)
    assert set(gen.state_dict()) == keys and "_layers" not in dict(gen.named_modules())


def test_paths_are_the_ragged_plans_layers_in_launch_order(gen):
    fills = [f.layer for f in ragged.plan(gen, [3000, 2000]).fills]
    assert fills[0] == "pqmf.analysis" and fills[-2:] == ["pqmf.synthesis", "enhanced"]
    assert [la.path for la in layers(gen)] == fills[1:-2]
    assert len(layers(gen)) == 28


def test_every_path_resolves_to_its_module_and_spec(gen):
    for la in layers(gen):
        assert gen.get_submodule(la.path) is la.module, la.path
        if la.kind == "unit":
            assert isinstance(la.module, ResidualUnit) and la.spec is la.module.dilated_conv.spec
        else:
            assert isinstance(la.module, HipConv1d) and la.spec is la.module.spec
            assert la.kind == ("convT" if la.spec.transposed else "conv")
    assert [la.kind for la in layers(gen)].count("unit") == 18 and [la.kind for la in layers(gen)].count("convT") == 3


def test_the_slopes_ride_on_the_first_unit_of_each_encoder_block_and_the_first_latent_conv(gen):
    sloped = [la.path for la in layers(gen) if la.in_slope != 1.0]
    assert sloped == ["encoder_blocks.0.residuals.0", "encoder_blocks.1.residuals.0", "encoder_blocks.2.residuals.0", "latent_conv.1"]
    assert all(la.in_slope == gen.nl.negative_slope for la in layers(gen) if la.path in sloped)


def test_the_decoder_adds_the_encoder_outputs_in_reverse(gen):
    skips = [(la.path, la.skip) for la in layers(gen) if la.skip is not None]
    adds = [(la.path, la.add) for la in layers(gen) if la.add is not None]
    assert skips == [(f"encoder_blocks.{i}.conv", i) for i in range(3)]
    assert adds == [(f"decoder_blocks.{i}.conv_trans", 2 - i) for i in range(3)]
    assert [a for _, a in adds] == [s for _, s in reversed(skips)]
    assert not any(la.skip is not None and la.add is not None for la in layers(gen))


def test_segments_are_contiguous_and_last_conv_alone_is_outside_the_core(gen):
    table = layers(gen)
    assert [la.core for la in table] == [True] * 27 + [False] and table[-1].path == "last_conv" and table[-1].segment is None
    runs = []
    for la in table[:-1]:
        if not runs or runs[-1] != la.segment:
            runs.append(la.segment)
    assert runs == [("misc",)] + [("enc", i) for i in range(3)] + [("latent",)] + [("dec", i) for i in range(3)]
    # a block's run: the encoder's [unit, unit, unit, conv], the decoder's [conv_trans, unit, unit, unit]; the backward walks it in reverse
    for name, kinds in (("enc", ["unit"] * 3 + ["conv"]), ("dec", ["convT"] + ["unit"] * 3)):
        for i in range(3):
            assert [la.kind for la in table if la.segment == (name, i)] == kinds
            assert all(la.path.startswith(f"{name}oder_blocks.{i}.") for la in table if la.segment == (name, i))
    assert [la.path for la in table if la.segment == ("misc",)] == ["first_conv"]
    assert [la.path for la in table if la.segment == ("latent",)] == ["latent_conv.1", "latent_conv.3"]


# ---- the backward plan: literal expectations, taken from the walk GeneratorEngine._bwd_segment wrote out by hand before it read the plan
def test_the_backward_plan_is_built_once_and_stays_out_of_the_state_dict(gen):
    keys = set(gen.state_dict())
    plan = backward_segments(gen)
    assert backward_segments(gen) is plan and isinstance(plan, tuple) and all(isinstance(seg, tuple) for seg in plan)
    assert set(gen.state_dict()) == keys and "_backward_segments" not in dict(gen.named_modules())
    assert all(step.layer is layers(gen)[[la.path for la in layers(gen)].index(step.layer.path)] for seg in plan for step in seg)


def test_backward_segments_run_decoder_latent_encoder_last_first_each_in_launch_order(gen):
    units = lambda blk: [f"{blk}.residuals.{k}" for k in (2, 1, 0)]
    want = [units(f"decoder_blocks.{i}") + [f"decoder_blocks.{i}.conv_trans"] for i in (2, 1, 0)]
    want += [["latent_conv.3", "latent_conv.1"]]
    want += [[f"encoder_blocks.{i}.conv"] + units(f"encoder_blocks.{i}") for i in (2, 1, 0)]
    want[-1] += ["first_conv"]   # its weight gradient closes encoder block 0's segment
    assert [[step.layer.path for step in seg] for seg in backward_segments(gen)] == want
    assert len(backward_segments(gen)) == 7


def test_every_core_layer_is_one_backward_step_and_first_conv_alone_takes_no_input_gradient(gen):
    steps = [step for seg in backward_segments(gen) for step in seg]
    assert sorted(step.layer.path for step in steps) == sorted(la.path for la in layers(gen) if la.core) and len(steps) == 27
    assert [step.layer.path for step in steps if not step.dx] == ["first_conv"]
    assert steps[-1].layer.path == "first_conv" and steps[-1].joins is None and steps[-1].yields is None


def test_skip_gradients_leave_at_the_transposed_convs_and_join_behind_the_encoder_outputs(gen):
    steps = [step for seg in backward_segments(gen) for step in seg]
    assert {step.layer.path: step.joins for step in steps if step.joins is not None} == {
        "encoder_blocks.1.residuals.0": 0, "encoder_blocks.2.residuals.0": 1, "latent_conv.1": 2}
    assert {step.layer.path: step.yields for step in steps if step.yields is not None} == {
        "decoder_blocks.0.conv_trans": 2, "decoder_blocks.1.conv_trans": 1, "decoder_blocks.2.conv_trans": 0}
    # a gradient is filed before it is read: the step that yields encoder output j runs before the one it joins
    order = {step.layer.path: n for n, step in enumerate(steps)}
    for j in range(3):
        assert order[f"decoder_blocks.{2 - j}.conv_trans"] < min(order[s.layer.path] for s in steps if s.joins == j)
    # every layer a gradient joins carries the activation mask it joins behind
    assert all(step.layer.in_slope != 1.0 for step in steps if step.joins is not None)
