"""CPU: the discriminators' ragged plan (``ragged.disc_plan``) -- row lengths, fills, margins, refusals -- and, in float64, the scheme
itself: the oracle's discriminator / feature-matching / hinge / MRSTFT pieces executing the plan on padded buffers with NaN in every
slack position no fill has written (tests/ragged_losses_oracle.py) give every clip the five values its own batch of one gives.

Bound of the float64 comparison: 1e-12.  Both sides run the same float64 operations on the same values; they differ in where a row
sits inside the tensor handed to a convolution and in the order of a few sums, i.e. by a few ulp (2.2e-16) of values of order one --
the bound of tests/test_ragged_plan.py."""
import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests import ragged_losses_oracle as L
from tests import ragged_oracle as R
from vibravox_amd import ragged

RAW = (4321, 3300, 3040, 2790, 2530)
CUT = (4320, 3296, 3040, 2784, 2528)
TERMS = ("reconstructive_loss_freq", "feature_matching_loss", "adv_loss_gen", "real_loss", "fake_loss")


@pytest.fixture(scope="module")
def nets():
    disc, d_sd = L.seeded_discriminator()
    return {p: R.formula_generator(p) for p in (1, 2)}, disc, d_sd


def conv_len(l, k, s, pad, d):
    return (l + 2 * pad - d * (k - 1) - 1) // s + 1


def own_lengths(chain, l):
    """A row's own lengths through chain 0..2 (dilation chain + 1) / 3 (MelGAN) by the conv length formula."""
    if chain < 3:
        d = chain + 1
        out = [l, conv_len(l + 2, 3, 1, 1, d)]
        for _ in range(5):
            out.append(conv_len(out[-1], 7, 2, 3, d))
        out.append(conv_len(out[-1], 5, 1, 2, d))
        out.append(conv_len(out[-1], 3, 1, 1, 1))
        return out
    out = [l, conv_len(l + 14, 15, 1, 0, 1)]
    for _ in range(4):
        out.append(conv_len(out[-1], 41, 4, 20, 1))
    out.append(conv_len(out[-1], 5, 1, 2, 1))
    out.append(conv_len(out[-1], 3, 1, 1, 1))
    return out


def the_plan(nets, p=2):
    gen, _ = nets[0][p]
    disc = nets[1]
    margin = ragged.loss_margin(disc, gen.pqmf.decimation)
    gplan = ragged.plan(gen, RAW, margin)
    return gplan, ragged.disc_plan(disc, gplan.cut, gplan.row_lengths[1], gplan.l_buf, gplan.buffer_lengths[1])


def test_row_lengths_are_each_rows_own_conv_arithmetic(nets):
    gplan, plan = the_plan(nets)
    assert gplan.cut == CUT and plan.cut == CUT and plan.band_lengths == tuple((t + 32) // 4 for t in CUT)
    for c in range(4):
        table = plan.lengths(c)
        for r in range(len(CUT)):
            assert [level[r] for level in table] == own_lengths(c, plan.band_lengths[r] if c < 3 else CUT[r]), (c, r)
    assert plan.lengths(2)[-1] == (15, 7, 5, 3, 1) and plan.lengths(3)[-1] == (17, 13, 12, 11, 10)


def test_margin_and_every_fill_fits_at_every_level(nets):
    gen, disc = nets[0][2][0], nets[1]
    assert ragged.loss_margin(disc, 4) == 1280   # the stride-4 k41 conv at 1/64 of the audio rate reads 20 frames past a row's end
    gplan, plan = the_plan(nets)
    assert gplan.margin == 1280 and gplan.l_buf == 5600 and plan.audio_l_buf == 5600 and plan.bands_l_buf == gplan.buffer_lengths[1] == 1408
    assert plan.audio_margin == 1280 and plan.bands_margin == 320
    assert ragged.plan(gen, RAW).l_buf == 5088 and ragged.plan(gen, RAW, 0).margin == 768   # every existing call keeps its l_buf
    own = ragged.disc_plan(disc, gplan.cut, gplan.row_lengths[1])                               # the plan's own margins: what it needs
    assert (own.audio_margin, own.bands_margin) == (1280, 64)
    for which in (plan, own):
        for c, chain in enumerate(which.chains):
            assert chain[0].in_buffer == (which.bands_l_buf if c < 3 else which.audio_l_buf)
            for layer in chain:
                for mode, count in layer.fills:
                    assert count >= 1
                    for l in layer.in_lengths:
                        assert l + count <= layer.in_buffer, (layer.path, l, count)
                        assert mode != ragged.MIRROR or count <= l - 1
                assert layer.out_buffer == own_lengths(c, chain[0].in_buffer)[chain.index(layer) + 1]
    with pytest.raises(ValueError, match="does not fit"):
        ragged.disc_plan(disc, gplan.cut, gplan.row_lengths[1], ragged.plan(gen, RAW).l_buf, ragged.plan(gen, RAW).buffer_lengths[1])


def test_first_layers_get_the_double_pad_and_the_mirror(nets):
    _, plan = the_plan(nets)
    for c in range(3):   # ReflectionPad1d(1), then a conv with zero padding 1: x[len] = x[len - 2], x[len + 1] = 0
        assert plan.chains[c][0].fills == ((ragged.ZERO, 2), (ragged.MIRROR, 1))
        assert all(mode == ragged.ZERO for layer in plan.chains[c][1:] for mode, _ in layer.fills)
    assert plan.chains[3][0].fills == ((ragged.MIRROR, 7),)
    assert max(count for layer in plan.chains[3] for _, count in layer.fills) <= 20


def test_short_clips_are_refused_by_index_naming_the_chain(nets):
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales

    gen, disc = nets[0][2][0], nets[1]
    assert ragged.disc_shortest(disc, gen.pqmf) == {"chains": (2, 315, 631, 8), "bands": 631, "audio": 8, "cut": 2528}
    with pytest.raises(ValueError, match=r"clip 2 .*pqmf_discriminators\.2 \(dilation 3\) needs 631"):
        ragged.disc_plan(disc, (4320, 2528, 2272), (1088, 640, 576))
    ragged.disc_plan(disc, (4320, 2528), (1088, 640))
    # the limit is the chains' arithmetic, whatever the widths: 9 -> 29 -> 69 -> 149 -> 309 -> 629 through the five stride-2 k7 convs
    # at dilation 3 (l -> (l - 13) // 2 + 1), + 2 for the first layer
    other = DiscriminatorEBENMultiScales(q=4, min_channels=8)
    assert ragged.disc_shortest(other)["bands"] == 631
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    wide = EBENGenerator(m=4, n=512, p=2)   # (cut + 512) / 4 >= 631 and cut + 512 a multiple of 256
    assert ragged.disc_shortest(other, wide.pqmf)["cut"] == 2048


def test_raw_entries_refuse_bad_arguments_before_any_launch():
    """The pointers are host memory: nothing may be launched on them (no GPU here anyway) -- every call returns in the checks."""
    import ctypes

    from vibravox_amd._lib import load

    lib = load()
    assert lib.eben_version() == 6
    f = (ctypes.c_float * 4096)()
    i32 = (ctypes.c_int32 * 4)(8, 8, 8, 8)
    addr = lambda a, off=0: ctypes.addressof(a) + off
    vp = lambda *xs: (ctypes.c_void_p * len(xs))(*xs)
    ints = lambda *xs: (ctypes.c_int * len(xs))(*xs)
    msg = lambda: lib.eben_last_error()
    assert lib.eben_fm_sums_rows_workspace(0, 4) == 0 == lib.eben_fm_sums_rows_workspace(3, 0) and lib.eben_fm_sums_rows_workspace(3, 4) == 3 * 4 * 32 * 8
    ws_bytes = lib.eben_fm_sums_rows_workspace(1, 4)
    fm = lambda **kw: lib.eben_fm_sums_rows(*[kw.get(k, d) for k, d in (("ptrs", vp(addr(f), addr(f))), ("channels", ints(2)), ("l_bufs", ints(8)),
                                                                         ("lens", vp(addr(i32))), ("npairs", 1), ("rows", 4), ("ws", addr(f)),
                                                                         ("ws_bytes", ws_bytes), ("sums", addr(f)), ("stream", None))])
    for key in ("ptrs", "channels", "l_bufs", "lens", "ws", "sums"):
        assert fm(**{key: None}) == -1 and b"null" in msg(), key
    for kw in (dict(npairs=0), dict(npairs=33), dict(rows=0), dict(rows=65536), dict(channels=ints(0)), dict(l_bufs=ints(0)),
               dict(ptrs=vp(addr(f), None)), dict(ptrs=vp(addr(f, 2), addr(f))), dict(lens=vp(None)), dict(sums=addr(f, 1))):
        assert fm(**kw) == -1, kw
    assert fm(ws_bytes=ws_bytes - 1) != 0 and b"workspace" in msg()
    hinge = lambda **kw: lib.eben_hinge_rows(*[kw.get(k, d) for k, d in (("xs", vp(addr(f))), ("l_bufs", ints(8)), ("targets", (ctypes.c_float * 1)(1.0)),
                                                                       ("lens", vp(addr(i32))), ("n", 1), ("rows", 4), ("out", addr(f)), ("stream", None))])
    for key in ("xs", "l_bufs", "targets", "lens", "out"):
        assert hinge(**{key: None}) == -1 and b"null" in msg(), key
    for kw in (dict(n=0), dict(n=33), dict(rows=0), dict(l_bufs=ints(-1)), dict(xs=vp(None)), dict(lens=vp(addr(i32, 1)))):
        assert hinge(**kw) == -1, kw
    need = lib.eben_stft_loss_sums_rows_workspace(4)
    assert need == 4 * 32 * 3 * 4 and lib.eben_stft_loss_sums_rows_workspace(0) == 0
    sums = lambda **kw: lib.eben_stft_loss_sums_rows(*[kw.get(k, d) for k, d in (("x", addr(f)), ("y", addr(f)), ("rows", 4), ("bins", 3), ("frames", 8),
                                                                               ("of_row", addr(i32)), ("row_stride", 8), ("bin_stride", 64), ("im_off", 192),
                                                                               ("eps", 1e-8), ("ws", addr(f)), ("ws_bytes", need), ("out", addr(f)), ("stream", None))])
    for key in ("x", "y", "of_row", "ws", "out"):
        assert sums(**{key: None}) == -1 and b"null" in msg(), key
    for kw in (dict(rows=0), dict(bins=0), dict(frames=0), dict(bin_stride=7), dict(of_row=addr(i32, 2))):
        assert sums(**kw) == -1, kw
    assert sums(ws_bytes=need - 1) != 0 and b"workspace" in msg()
    clip = lambda **kw: lib.eben_clip_losses(*[kw.get(k, d) for k, d in (("sums", vp(addr(f))), ("frames", vp(addr(i32))), ("bins", ints(3)), ("n_res", 1),
                                                                       ("fm", addr(f)), ("npairs", 1), ("inv", 1.0), ("hinge", addr(f)), ("nchains", 1), ("rows", 4),
                                                                       ("out", addr(f)), ("stream", None))])
    for kw in (dict(out=None), dict(rows=0), dict(n_res=9), dict(sums=None), dict(sums=vp(None)), dict(bins=ints(0)), dict(fm=None), dict(hinge=None),
               dict(npairs=-1)):
        assert clip(**kw) == -1, kw


@pytest.mark.parametrize("p", [2, 1])
def test_float64_run_of_the_plan_equals_every_clips_own_losses(nets, p):
    from vibravox_amd.torch_modules.losses.mrstft_loss import a_weighting_taps

    (gen, g_sd), disc, d_sd = nets[0][p], nets[1], nets[2]
    gplan, plan1 = the_plan(nets, p)
    rows = len(RAW)
    plan = ragged.disc_plan(disc, gplan.cut * 2, gplan.row_lengths[1] * 2, gplan.l_buf, gplan.buffer_lengths[1])
    assert plan.chains[2][0].fills == plan1.chains[2][0].fills
    corrupted = [formula_audio(f"rlosses/bc/{i}", 1, t).double() for i, t in enumerate(RAW)]
    references = [formula_audio(f"rlosses/air/{i}", 1, t).double() for i, t in enumerate(RAW)]
    padded = torch.zeros((rows, 1, gplan.l_buf), dtype=torch.float64)
    ref = torch.zeros((rows, 1, gplan.l_buf), dtype=torch.float64)
    for r in range(rows):
        padded[r, 0, : CUT[r]] = corrupted[r][0, 0, : CUT[r]]
        ref[r, 0, : CUT[r]] = references[r][0, 0, : CUT[r]]
    enh, bands = R.generator_forward_ragged(g_sd, padded, gplan, p)
    ref_bands = O.pqmf_analysis(ref, g_sd["pqmf.analysis_weights"])
    fir = a_weighting_taps(16000).double()
    got = L.clip_losses_ragged(d_sd, disc.q, plan, enh, ref, bands, ref_bands, fir=fir)
    for r in range(rows):
        t, l0 = CUT[r], gplan.row_lengths[1][r]
        o_enh, o_bands = O.generator_forward(g_sd, O.cut_to_valid_length(corrupted[r]), p)
        o_ref = O.cut_to_valid_length(references[r])
        want = L.clip_losses_alone(d_sd, disc.q, o_enh, o_ref, o_bands, O.pqmf_analysis(o_ref, g_sd["pqmf.analysis_weights"]), fir=fir)
        assert o_enh.shape[2] == t and o_bands.shape[2] == l0
        for name in TERMS:
            a, b = float(got[name][r]), float(want[name])
            print(f"p={p} clip {r} {name}: ragged {a:.15g} alone {b:.15g} diff {abs(a - b):.1e}")
            assert abs(a - b) <= 1e-12, (name, r, a, b)


def test_equal_cuts_give_no_fills_and_still_per_row_values(nets):
    (gen, g_sd), disc, d_sd = nets[0][2], nets[1], nets[2]
    raw = (3050, 3040, 3100)   # one cut length: 3040
    gplan = ragged.plan(gen, raw, ragged.loss_margin(disc, 4))
    assert set(gplan.cut) == {3040} and gplan.margin == 0
    plan = ragged.disc_plan(disc, gplan.cut * 2, gplan.row_lengths[1] * 2, gplan.l_buf, gplan.buffer_lengths[1])
    assert not plan.ragged and all(not layer.fills for chain in plan.chains for layer in chain)
    enh = torch.cat([formula_audio(f"rlosses/eq/e{i}", 1, 3040).double() for i in range(3)])
    ref = torch.cat([formula_audio(f"rlosses/eq/r{i}", 1, 3040).double() for i in range(3)])
    ana = g_sd["pqmf.analysis_weights"]
    got = L.clip_losses_ragged(d_sd, disc.q, plan, enh, ref, O.pqmf_analysis(enh, ana), O.pqmf_analysis(ref, ana))
    values = set()
    for r in range(3):
        want = L.clip_losses_alone(d_sd, disc.q, enh[r : r + 1], ref[r : r + 1], O.pqmf_analysis(enh[r : r + 1], ana), O.pqmf_analysis(ref[r : r + 1], ana))
        for name in TERMS:
            assert abs(float(got[name][r]) - float(want[name])) <= 1e-12, (name, r)
        values.add(float(got["feature_matching_loss"][r]))
    assert len(values) == 3   # per-row values, not one batch mean
