"""GPU: ragged-batch generator inference -- the edge-fill kernels through their raw entry points against torch indexing, and
``EBENGenerator.forward_ragged`` / ``inference.enhance_clips`` against the float64 oracle of every clip ALONE and against the same build's
batch-1 forward of that clip.

Bars: max|.| < 2e-5 on enhanced and bands and MSE < 1e-10 against the oracle, the bars of
test_gpu_models.py::test_generator_inference_variable_length; and a ragged row may be no further from the oracle than twice its batch-1
row is (where a row sits among the kernels' tiles can move a rounding, nothing more)."""
import functools

import pytest
import torch

from formula import formula_audio, formula_tensor
from oracle import eben_oracle as O
from tests import ragged_oracle as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LENGTHS = (4321, 4064, 3808, 3552, 3296, 1000)    # cut 4320 4064 3808 3552 3296 992: the longest, 1 / 2 / 3 / 4 latent frames short, the minimum
LENGTHS_512 = (2100, 1800, 1536, 1300, 600)       # n = 512: cut 2048 1792 1536 1280 512 (the minimum: four latent frames)
FENCE = 64
SENTINEL = 12345.0


# ---- the fill kernels -------------------------------------------------------------------------------------------------------------
def fenced(rows, channels, l_buf, lens, tag):
    """A (rows, channels, l_buf) view 4 bytes off the 16-byte grid inside a fenced allocation: formula values in front of each row's end,
    NaN behind it."""
    n = rows * channels * l_buf
    flat = torch.full((FENCE + 1 + n + FENCE,), SENTINEL, dtype=torch.float32)
    body = formula_tensor(tag, (rows, channels, l_buf))
    for r, ln in enumerate(lens):
        body[r, :, max(ln, 0):] = float("nan")
    flat[FENCE + 1 : FENCE + 1 + n] = body.reshape(-1)
    dev = flat.to(DEV)
    view = dev[FENCE + 1 : FENCE + 1 + n].view(rows, channels, l_buf)
    assert view.data_ptr() % 16 == 4
    return flat, dev, view


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # NaN == NaN


def expected_fill(flat, rows, channels, l_buf, lens, mode, count):
    want = flat.clone()
    x = want[FENCE + 1 : FENCE + 1 + rows * channels * l_buf].view(rows, channels, l_buf)
    for r, ln in enumerate(lens):
        if ln < 0 or ln >= l_buf:
            continue                                                # no slack
        if mode == "zero_all":
            x[r, :, ln:] = 0.0
        elif ln + count > l_buf or (mode == "mirror" and count > ln - 1):
            continue                                                # the kernel must skip the row
        elif mode == "mirror":
            x[r, :, ln : ln + count] = x[r, :, ln - 1 - count : ln - 1].flip(-1)
        else:
            x[r, :, ln : ln + count] = 0.0
    return want


@pytest.mark.parametrize("channels,l_buf", [(5, 40), (32, 40), (5, 1000), (32, 1000)])
def test_edge_fill_equals_torch_indexing(hip, channels, l_buf):
    from vibravox_amd._lib import check, stream

    rows = 3
    for count in (1, 3, 9, 8):
        tables = [(l_buf, l_buf - 13, l_buf - count + 1),     # no slack / an ordinary row / a fill that would leave the buffer
                  (l_buf - count, count, -1),                 # a fill up to the buffer's last sample / a mirror from in front of the row / nonsense
                  (count + 1, l_buf - 11, l_buf)]             # the shortest row a mirror of `count` fits
        for lens in tables:
            table = torch.tensor(lens, dtype=torch.int32, device=DEV)
            for mode in ("zero", "mirror", "zero_all"):
                flat, dev, view = fenced(rows, channels, l_buf, lens, f"fill/{channels}/{l_buf}")
                if mode == "zero_all":
                    check(hip.eben_edge_zero(view.data_ptr(), table.data_ptr(), rows, channels, l_buf, stream()), "edge_zero")
                else:
                    check(hip.eben_edge_fill(view.data_ptr(), table.data_ptr(), rows, channels, l_buf, 1 if mode == "mirror" else 0, count,
                                             stream()), "edge_fill")
                want = expected_fill(flat, rows, channels, l_buf, lens, mode, count)
                got = dev.cpu()
                assert same_bits(got, want), (mode, count, lens)
                assert float(got[:FENCE].min()) == SENTINEL == float(got[-FENCE:].max()) and float(got[FENCE]) == SENTINEL


# ---- the ragged forward -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(p, n=32):
    """The generator on the device, the clips, and per clip the float64 oracle of that clip alone (computed once)."""
    gen, sd = R.formula_generator(p, n)
    lengths = LENGTHS if n == 32 else LENGTHS_512
    clips = [formula_audio(f"ragged/{n}/{i}", 1, t) for i, t in enumerate(lengths)]
    refs = [O.generator_forward(sd, O.cut_to_valid_length(c.double(), n=n), p) for c in clips]
    return gen.to(DEV), lengths, clips, refs


def pack(clips, length=None, slack=0.0):
    length = length or max(c.shape[2] for c in clips)
    buf = torch.full((len(clips), 1, length), slack, dtype=torch.float32)
    for r, c in enumerate(clips):
        buf[r, 0, : c.shape[2]] = c[0, 0]
    return buf.to(DEV)


def dist(got, ref):
    d = got.detach().double().cpu() - ref
    return float(d.abs().max()), float((d ** 2).mean())


def check_rows(gen, clips, refs, enhanced, bands, tag):
    """Each clip's ragged result against the oracle of the clip alone and against the batch-1 device forward of the clip."""
    for r, (clip, (o_enh, o_bands)) in enumerate(zip(clips, refs)):
        t, l0 = o_enh.shape[2], o_bands.shape[2]
        with torch.no_grad():
            b1_enh, b1_bands = gen(gen.cut_to_valid_length(clip.to(DEV)))
        assert b1_enh.shape[2] == t
        (e_max, e_mse), (b_max, b_mse) = dist(enhanced[r][..., :t].reshape(1, 1, t), o_enh), dist(bands[r][..., :l0].reshape(1, -1, l0), o_bands)
        (e1_max, e1_mse), (b1_max, b1_mse) = dist(b1_enh, o_enh), dist(b1_bands, o_bands)
        print(f"{tag} row {r} ({t} samples): ragged enhanced max {e_max:.2e} mse {e_mse:.2e} bands max {b_max:.2e} | batch-1 enhanced max "
              f"{e1_max:.2e} mse {e1_mse:.2e} bands max {b1_max:.2e}")
        assert e_max < 2e-5 and b_max < 2e-5 and e_mse < 1e-10, (r, e_max, b_max, e_mse)
        assert e_max <= 2 * e1_max and b_max <= 2 * b1_max, (r, e_max, e1_max, b_max, b1_max)
        assert e_mse ** 0.5 <= 2 * e1_mse ** 0.5 and b_mse ** 0.5 <= 2 * b1_mse ** 0.5, (r, e_mse, e1_mse, b_mse, b1_mse)


def slack_is_zero(plan, enhanced, bands):
    for r, (t, l0) in enumerate(zip(plan.cut, plan.row_lengths[1])):
        if not (same_bits(enhanced[r, :, t:], torch.zeros_like(enhanced[r, :, t:])) and same_bits(bands[r, :, l0:], torch.zeros_like(bands[r, :, l0:]))):
            return False
    return True


@pytest.mark.parametrize("p", [2, 1])
def test_ragged_forward_gives_every_row_its_own_forward(hip, p):
    from vibravox_amd import ragged

    gen, lengths, clips, refs = case(p)
    plan = ragged.plan(gen, lengths)
    assert plan.cut == (4320, 4064, 3808, 3552, 3296, 992) and plan.l_buf == 5088
    with torch.no_grad():
        enhanced, bands = gen.forward_ragged(pack(clips), lengths)
    assert enhanced.shape == (6, 1, 5088) and bands.shape == (6, 4, 1280)
    assert slack_is_zero(plan, enhanced, bands)
    check_rows(gen, clips, refs, enhanced, bands, f"p={p}")


def test_equal_cut_lengths_are_the_batched_forward(hip):
    gen, _, _, _ = case(2)
    lengths = (1300, 1248, 1400)
    padded = pack([formula_audio(f"ragged/eq/{i}", 1, t) for i, t in enumerate(lengths)])
    with torch.no_grad():
        enhanced, bands = gen.forward_ragged(padded, lengths)
        want_enh, want_bands = gen(padded[:, :, :1248].contiguous())
    assert enhanced.shape == (3, 1, 1248)
    assert torch.equal(enhanced, want_enh) and torch.equal(bands, want_bands)


def test_what_lies_behind_a_clip_is_never_read(hip):
    from vibravox_amd import ragged

    gen, lengths, clips, _ = case(2)
    plan = ragged.plan(gen, lengths)
    cut = [c[:, :, :t] for c, t in zip(clips, plan.cut)]
    with torch.no_grad():
        clean = gen.forward_ragged(pack(cut, plan.l_buf), lengths)
        poisoned = gen.forward_ragged(pack(cut, plan.l_buf, slack=float("nan")), lengths)
        short = gen.forward_ragged(pack(cut, slack=float("nan")), lengths)   # shorter than l_buf: padded inside
    for got in (poisoned, short):
        assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])
        assert slack_is_zero(plan, *got)


def test_enhance_clips_in_three_batches(hip):
    from vibravox_amd import ragged
    from vibravox_amd.inference import enhance_clips

    gen, lengths, clips, refs = case(2)
    budget = 10200
    batches, _ = ragged.compose_batches(gen, lengths, budget)
    assert [sorted(b) for b in batches] == [[4, 5], [2, 3], [0, 1]]
    shaped = [c.to(DEV).reshape(shape) for c, shape in zip(clips, [(-1,), (1, -1), (1, 1, -1)] * 2)]
    enhanced, bands = enhance_clips(gen, shaped, max_batch_samples=budget, return_bands=True)
    cut = ragged.plan(gen, lengths).cut
    assert [tuple(e.shape) for e in enhanced] == [(cut[0],), (1, cut[1]), (1, 1, cut[2]), (cut[3],), (1, cut[4]), (1, 1, cut[5])]
    assert [tuple(b.shape) for b in bands] == [(4, (t + 32) // 4) for t in cut]
    check_rows(gen, clips, refs, enhanced, bands, "enhance_clips")
    only = enhance_clips(gen, shaped, max_batch_samples=budget)
    assert all(torch.equal(a, b) for a, b in zip(only, enhanced))


def test_ragged_forward_with_a_512_tap_bank(hip):
    from vibravox_amd import ragged

    gen, lengths, clips, refs = case(2, 512)
    plan = ragged.plan(gen, lengths)
    assert plan.cut == (2048, 1792, 1536, 1280, 512) and plan.margin == 768
    with torch.no_grad():
        enhanced, bands = gen.forward_ragged(pack(clips), lengths)
    assert enhanced.shape == (5, 1, 2816) and slack_is_zero(plan, enhanced, bands)
    check_rows(gen, clips, refs, enhanced, bands, "n=512")


def test_ragged_forward_refuses_autograd_and_short_clips(hip):
    gen, lengths, clips, _ = case(2)
    with pytest.raises(RuntimeError, match="no backward"):
        gen.forward_ragged(pack(clips), lengths)
    with torch.no_grad(), pytest.raises(ValueError, match="clip 1 "):
        gen.forward_ragged(pack(clips[:2]), (4321, 991))
