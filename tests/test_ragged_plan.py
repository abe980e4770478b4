"""CPU: the ragged-batch plan (vibravox_amd/ragged.py) -- its fill counts, margin, refusals and batch composer -- and, in float64, the
scheme itself: a plain-torch generator forward that executes the plan on a padded buffer (tests/ragged_oracle.py: NaN behind every row's
end, the fill, large finite junk behind the fill) gives every row what the oracle's forward of that row alone gives.

Bound of the float64 comparison: 1e-12.  Both sides run the same float64 convolutions on the same values; they differ only in where
the row sits inside the tensor handed to the convolution, i.e. in summation order: a few ulp (2.2e-16) of values of order one."""
import ctypes
import os

import numpy as np
import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests import ragged_oracle as R
from vibravox_amd import ragged

LENGTH_SETS = {
    "mixed": [992, 1248, 1300, 2016, 3040, 2784, 2272],        # cut 992 1248 1248 2016 3040 2784 2272: the minimum, two equal rows
    "frames": [4321, 4064, 3808, 3552, 3296, 1000],            # cut 4320 and rows 1, 2, 3 and 4 latent frames (256 samples) short of it
}


@pytest.fixture(scope="module")
def generators():
    return {p: R.formula_generator(p) for p in (1, 2)}


@pytest.fixture(scope="module")
def gen512():
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    return EBENGenerator(m=4, n=512, p=2)


@pytest.mark.parametrize("which", ["mixed", "frames"])
@pytest.mark.parametrize("p", [2, 1])
def test_every_row_of_the_ragged_restatement_equals_its_own_forward(generators, p, which):
    gen, sd = generators[p]
    lengths = LENGTH_SETS[which]
    plan = ragged.plan(gen, lengths)
    assert plan.l_buf == max(plan.cut) + 768
    if which == "mixed":
        assert plan.cut == (992, 1248, 1248, 2016, 3040, 2784, 2272)
    else:
        assert [(max(plan.cut) - t) // 256 for t in plan.cut][:4] == [0, 1, 2, 3] and min(plan.cut) == 992
    clips = [formula_audio(f"ragged/{i}", 1, t).double() for i, t in enumerate(lengths)]
    padded = torch.full((len(clips), 1, plan.l_buf), float("nan"), dtype=torch.float64)
    for r, c in enumerate(clips):
        padded[r, 0, : plan.cut[r]] = c[0, 0, : plan.cut[r]]
    enh, bands = R.generator_forward_ragged(sd, padded, plan, p)
    assert enh.shape == (len(clips), 1, plan.l_buf) and bands.shape == (len(clips), 4, plan.buffer_lengths[1])
    worst = 0.0
    for r, c in enumerate(clips):
        o_enh, o_bands = O.generator_forward(sd, O.cut_to_valid_length(c), p)
        t, l0 = plan.cut[r], plan.row_lengths[1][r]
        assert o_enh.shape[2] == t and o_bands.shape[2] == l0
        err = max(float((enh[r : r + 1, :, :t] - o_enh).abs().max()), float((bands[r : r + 1, :, :l0] - o_bands).abs().max()))
        worst = max(worst, err)
        assert err < 1e-12, (r, err)
        assert float(enh[r, :, t:].abs().max()) == 0.0 and float(bands[r, :, l0:].abs().max()) == 0.0   # all slack zeroed
    print("p", p, "worst |ragged - own forward|", worst)


def test_plan_of_the_default_generator(generators):
    plan = ragged.plan(generators[2][0], [4321, 4064, 3808, 3552, 3296, 1000])
    assert plan.cut == (4320, 4064, 3808, 3552, 3296, 992)
    assert plan.margin == 768 and plan.l_buf == 4320 + 768
    assert plan.buffer_lengths == (5088, 1280, 640, 160, 20)
    assert plan.row_lengths[1] == (1088, 1024, 960, 896, 832, 256) and plan.row_lengths[4] == (17, 16, 15, 14, 13, 4)
    got = [(f.layer, f.mode, f.count, f.level) for f in plan.fills]
    want = [("pqmf.analysis", "zero_all", 29, 0), ("first_conv", "mirror", 1, 1)]
    for i, lv in enumerate((1, 2, 3)):
        want += [(f"encoder_blocks.{i}.residuals.{k}", "mirror", d, lv) for k, d in enumerate((1, 3, 9))]
        want.append((f"encoder_blocks.{i}.conv", "mirror", 1, lv))
    want += [("latent_conv.1", "mirror", 3, 4), ("latent_conv.3", "mirror", 3, 4)]
    for i, lv in enumerate((4, 3, 2)):
        want.append((f"decoder_blocks.{i}.conv_trans", "zero", 1, lv))
        want += [(f"decoder_blocks.{i}.residuals.{k}", "mirror", d, lv - 1) for k, d in enumerate((1, 3, 9))]
    want += [("last_conv", "mirror", 1, 1), ("pqmf.synthesis", "zero_all", 8, 1), ("enhanced", "zero_all", 32, 0)]
    assert got == want
    # every fill fits every row's slack, and a mirror never starts in front of its row
    for f in plan.fills:
        for n in plan.row_lengths[f.level]:
            assert n + f.count <= plan.buffer_lengths[f.level] and (f.mode != "mirror" or f.count <= n - 1)


def test_reach_of_single_layers():
    from vibravox_amd.ops import ConvSpec

    assert ragged.reach(ConvSpec(32, 32, 3, dilation=9, pad_l=9, pad_r=9, reflect=True), 500) == 9
    assert ragged.reach(ConvSpec(128, 256, 16, stride=8, pad_l=7, pad_r=7, reflect=True), 504) == 1
    assert ragged.reach(ConvSpec(256, 64, 7, pad_l=3, pad_r=3, reflect=True), 4) == 3
    assert ragged.reach(ConvSpec(256, 128, 16, stride=8, pad_l=4, transposed=True), 17) == 1
    assert ragged.reach(ConvSpec(64, 32, 4, stride=2, pad_l=1, transposed=True), 100) == 1
    assert ragged.reach(ConvSpec(32, 32, 1), 100) == 0


def test_margin_for_n32_and_n512(generators, gen512):
    for gen, n in ((generators[2][0], 32), (gen512, 512)):
        plan = ragged.plan(gen, [3000, 2000])
        want = -(-max(3 * gen.multiple, n) // gen.multiple) * gen.multiple
        assert plan.margin == want == 768 and plan.l_buf == max(plan.cut) + 768
        assert (plan.l_buf + n) % gen.multiple == 0          # the buffer is itself a valid length
        assert {f.layer: f.count for f in plan.fills}["pqmf.synthesis"] == n // 4
    assert ragged.plan(gen512, [3000, 2000]).cut == (2816, 1792)


def test_equal_cut_lengths_need_no_fill(generators):
    plan = ragged.plan(generators[2][0], [1300, 1248, 1400])
    assert plan.cut == (1248, 1248, 1248) and plan.fills == () and plan.l_buf == 1248 and plan.margin == 0 and not plan.ragged
    assert ragged.plan(generators[2][0], [5000]).fills == ()


def test_a_clip_the_generator_would_refuse_is_named(generators):
    assert ragged.plan(generators[2][0], [2000, 992]).cut == (1760, 992)
    with pytest.raises(ValueError, match="clip 1 "):
        ragged.plan(generators[2][0], [2000, 991])
    with pytest.raises(ValueError, match="clip 2 "):
        ragged.plan(generators[2][0], [2000, 3000, 100])
    with pytest.raises(ValueError, match="clip 0 "):
        ragged.compose_batches(generators[2][0], [991, 3000], 1 << 20)
    with pytest.raises(RuntimeError):   # the reference refuses the same clip: a reflect pad of 3 on 3 latent frames
        torch.nn.functional.pad(torch.zeros(1, 1, 3), (3, 3), mode="reflect")


def test_composer_respects_the_budget_and_round_trips(generators):
    gen = generators[2][0]
    rng = np.random.RandomState(0)
    lengths = [int(t) for t in rng.randint(1000, 40000, size=57)] + [1000, 1000, 1000]
    budget = 100_000
    batches, back = ragged.compose_batches(gen, lengths, budget)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(len(lengths)))
    assert [flat[back[i]] for i in range(len(lengths))] == list(range(len(lengths)))
    cuts = [ragged.cut_length(gen, t) for t in lengths]
    assert [cuts[i] for i in flat] == sorted(cuts)
    assert len(batches) < len(lengths)
    for b in batches:
        plan = ragged.plan(gen, [lengths[i] for i in b])
        assert len(b) * plan.l_buf <= budget or len(b) == 1
    # a clip above the budget is a batch of its own
    batches, _ = ragged.compose_batches(gen, [200_000, 1000, 1000], budget)
    assert batches == [[1, 2], [0]]


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_edge_fill_argument_errors_without_gpu(lib):
    """The host entries refuse bad arguments before any launch (EBEN_EINVAL = -1 and a message)."""
    x, lens = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)   # never dereferenced: every call below is refused
    assert lib.eben_edge_fill(x, lens, 3, 5, 40, 1, 0, None) == -1 and b"count" in lib.eben_last_error()
    assert lib.eben_edge_fill(x, lens, 3, 5, 40, 0, -2, None) == -1
    assert lib.eben_edge_fill(x, lens, 3, 5, 40, 1, 40, None) == -1
    assert lib.eben_edge_fill(x, lens, 3, 5, 40, 2, 1, None) == -1 and b"mode" in lib.eben_last_error()
    assert lib.eben_edge_fill(None, lens, 3, 5, 40, 1, 1, None) == -1 and b"null" in lib.eben_last_error()
    assert lib.eben_edge_fill(x, None, 3, 5, 40, 1, 1, None) == -1
    assert lib.eben_edge_fill(ctypes.c_void_p(0x1002), lens, 3, 5, 40, 1, 1, None) == -1 and b"misaligned" in lib.eben_last_error()
    assert lib.eben_edge_fill(x, lens, 0, 5, 40, 1, 1, None) == -1
    assert lib.eben_edge_fill(x, lens, 3, 5, 0, 1, 1, None) == -1
    assert lib.eben_edge_zero(None, lens, 3, 5, 40, None) == -1
    assert lib.eben_edge_zero(x, None, 3, 5, 40, None) == -1
    assert lib.eben_edge_zero(x, lens, 3, 0, 40, None) == -1
