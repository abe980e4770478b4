"""CPU (no GPU): which exact-fp32 weight-gradient route, which kernel instantiation and which plan every case of the table runs, asked
of the library's own dispatch decision (eben_conv1d_bwd_dw_f32_variant: what eben_conv1d_bwd_dw_workspace and eben_conv1d_bwd_dw
dispatch on), and that the table reaches every instantiation and every plan edge named below.  tests/test_gpu_dw_f32_routes.py runs
each case against the float64 oracle of tests/dw_oracle.py; a retuned plan that moves a case off its kernel, or off the edge it was
chosen for, fails here by name.  These routes serve every layer of the 32-true plan, the generator's backward under 32-split and
EBEN_GEN_BWD_MATH=f32, every bf16x3 / bf16x6 layer and every bf16 layer conv_dw3 declines.

DW2       conv_dw2_kernel<FM, FN, WAVES_M, XR> behind dw_pack_a_kernel<FM, WAVES_M> (conv_dw2.hip, make_dw2_plan): the row tile of
          128 / 96 / 64 / 32 rows that pads the rows per group least, times a small X tile (12 register slots per thread) or a wide
          one (20 slots on the 128- / 96-row tiles, 32 on the others).  All 8 + 4 instantiations are reached by default plans.
FALLBACK  conv_dw_kernel<1, 8, 1, 2> (conv_dw.hip, make_dw_plan): time chunks of 128, 64 or 32 steps; an X tile past the register
          prefetch's 5120 elements is staged directly (xfits 0).
TINY      tiny_dw_kernel<4>: at most 3 columns + bias over a row of 512 steps or more, one slab per batch item.
ONE_ROW   m1_dw_kernel: c_out = 1, k = 3, stride 1, c_in >= 64, one slab per batch item.

Split-K hand-over: block z owns chunks z, z + nsplit, ...; the double-buffered K loop of conv_dw2_kernel and the register prefetch of
conv_dw_kernel hand over between chunks only where nsplit < nchunks, which no layer of the suite's other tests has.  The hand-over
cases own 1 and 2 (dw2_hand_even_odd), 2 and 3 (dw2_hand_3, fb_hand) and 3 chunks (dw2_tiles384: 384 tiles, so no split at all).
"""
import ctypes
import os

import pytest

from tests.test_dw3_variants import BF16X3, BF16X6, DW2, DW3, FALLBACK, ONE_ROW, TINY, W, _refl
from vibravox_amd import ops

F32 = ops.MATH_F32
FIELDS = ("route", "FM", "FN", "WAVES_M", "XR", "bk", "xfits", "nsplit", "nchunks", "nnt", "nmt", "nct", "nch_max", "row_stride")
DW_XCAP = 5120   # conv_dw.hip: X-tile elements the register prefetch of conv_dw_kernel holds


class F(W):
    """One weight gradient and the 14 numbers of eben_conv1d_bwd_dw_f32_variant (FIELDS)."""

    def desc(self):
        """The descriptor eben_conv1d_bwd_dw is given: the layer as it is (no pre-mask outside bf16 math)."""
        return ops.conv_desc(self.spec(), self.batch, self.length, self.math)

    def plan(self):
        return dict(zip(FIELDS, self.expect))

    def has_bias(self):
        return self.bias and not self.spec().transposed


def conv(c_in, c_out, ksize, stride=1, dilation=1, groups=1, pad_l=0, pad_r=0, **kw):
    return dict(c_in=c_in, c_out=c_out, ksize=ksize, stride=stride, dilation=dilation, groups=groups, pad_l=pad_l, pad_r=pad_r, **kw)


def dw2(fm, fn, wm, xr, nsplit, nchunks, nnt, nmt, nct, nch_max, row_stride):
    return (DW2, fm, fn, wm, xr, 0, 0, nsplit, nchunks, nnt, nmt, nct, nch_max, row_stride)


def fb(bk, xfits, nsplit, nchunks, nnt, nmt, nct, nch_max, row_stride):
    return (FALLBACK, 0, 0, 0, 0, bk, xfits, nsplit, nchunks, nnt, nmt, nct, nch_max, row_stride)


def per_item(route, nslab, row_stride):
    return (route, 0, 0, 0, 0, 0, 0, nslab, 0, 0, 0, 0, 0, row_stride)


ENC_S2 = _refl(**conv(32, 64, 4, stride=2, pad_l=1, pad_r=1))
DEC_S8 = conv(256, 128, 16, stride=8, pad_l=4, transposed=True)
DEC_S4 = conv(128, 64, 8, stride=4, pad_l=2, transposed=True)
DEC_S2 = conv(64, 32, 4, stride=2, pad_l=1, transposed=True)

# plans confirmed by the query, then kept
CASES = {
    # ---- DW2: the eight conv_dw2_kernel instantiations
    "dw2_128_x12": F(conv(16, 256, 5, pad_l=2, pad_r=2), 2, 150, F32, True, dw2(2, 2, 2, 12, 6, 6, 1, 2, 3, 16, 81)),
    "dw2_128_x20": F(_refl(**conv(64, 128, 3, dilation=9, pad_l=9, pad_r=9)), 2, 131, F32, True, dw2(2, 2, 2, 20, 6, 6, 2, 1, 3, 44, 193)),
    "dw2_96_x12": F(conv(24, 96, 5, dilation=3, pad_l=6, pad_r=6), 2, 150, F32, True, dw2(3, 1, 1, 12, 6, 6, 1, 1, 3, 24, 121)),
    # 32 channels x 4 taps = 128 columns: the second column tile holds the bias column alone
    "dw2_96_x20": F(_refl(**conv(32, 96, 4, stride=2, pad_l=1, pad_r=1)), 2, 102, F32, True, dw2(3, 1, 1, 20, 2, 2, 2, 1, 1, 32, 129)),
    "dw2_64_x12": F(conv(16, 64, 5, pad_l=2, pad_r=2), 3, 300, F32, True, dw2(2, 1, 1, 12, 15, 15, 1, 1, 5, 16, 81)),
    "dw2_64_x32": F(ENC_S2, 3, 204, F32, True, dw2(2, 1, 1, 32, 6, 6, 2, 1, 2, 32, 129)),
    "dw2_32_x12": F(conv(16, 160, 3, pad_l=1, pad_r=1), 3, 1100, F32, True, dw2(1, 1, 1, 12, 54, 54, 1, 5, 18, 16, 49)),
    "dw2_32_x32": F(conv(96, 32, 1), 2, 200, F32, True, dw2(1, 1, 1, 32, 8, 8, 1, 1, 4, 96, 97)),
    # ---- DW2: grouped layers (24 rows per group on the 32-row tile; 192 rows per group on two 96-row tiles, 48 tiles)
    "dw2_grp24": F(conv(24, 96, 7, stride=2, dilation=3, groups=4, pad_l=3, pad_r=3), 3, 301, F32, True, dw2(1, 1, 1, 12, 9, 9, 1, 1, 3, 6, 43)),
    "dw2_wide_grp": F(conv(384, 768, 7, stride=2, dilation=2, groups=4, pad_l=3, pad_r=3), 2, 260, F32, True, dw2(3, 1, 1, 12, 4, 4, 6, 2, 2, 20, 673)),
    # ---- DW2: ConvTranspose1d (operands swapped; with a fused output activation the mask sits on the X side)
    "dw2_dec_s8_masked": F(dict(DEC_S8, out_slope=0.01), 3, 41, F32, False, dw2(2, 2, 2, 20, 3, 3, 17, 2, 1, 9, 2049)),
    "dw2_dec_s8": F(DEC_S8, 3, 41, F32, False, dw2(2, 2, 2, 20, 3, 3, 17, 2, 1, 9, 2049)),
    "dw2_dec_s4": F(dict(DEC_S4, in_slope=0.01), 3, 75, F32, False, dw2(2, 2, 2, 20, 6, 6, 5, 1, 2, 17, 513)),
    "dw2_dec_s2_masked": F(dict(DEC_S2, in_slope=0.01, out_slope=0.01), 2, 150, F32, False, dw2(2, 1, 1, 32, 6, 6, 2, 1, 3, 32, 129)),
    # ---- DW2: the split-operand maths that are exact fp32, and the fused activations of a Conv1d
    "dw2_bf16x3": F(ENC_S2, 3, 204, BF16X3, True, dw2(2, 1, 1, 32, 6, 6, 2, 1, 2, 32, 129)),
    "dw2_bf16x6": F(ENC_S2, 3, 204, BF16X6, True, dw2(2, 1, 1, 32, 6, 6, 2, 1, 2, 32, 129)),
    "dw2_in_act": F(conv(24, 96, 5, pad_l=2, pad_r=2, in_slope=0.01), 2, 100, F32, True, dw2(3, 1, 1, 12, 4, 4, 1, 1, 2, 24, 121)),
    "dw2_out_act": F(conv(16, 64, 5, pad_l=2, pad_r=2, out_slope=0.2), 2, 100, F32, True, dw2(2, 1, 1, 12, 4, 4, 1, 1, 2, 16, 81)),
    # ---- DW2: split-K hand-over.  105 chunks over 96 blocks (blocks own 1 and 2), over 48 (2 and 3); 384 tiles: one block owns all 3
    "dw2_hand_even_odd": F(conv(64, 256, 9, groups=4, pad_l=4, pad_r=4), 3, 2203, F32, True, dw2(2, 1, 1, 12, 96, 105, 2, 1, 35, 16, 145)),
    "dw2_hand_3": F(conv(256, 128, 7, groups=4, pad_l=3, pad_r=3), 3, 2203, F32, True, dw2(1, 1, 1, 12, 48, 105, 4, 1, 35, 20, 449)),
    "dw2_tiles384": F(conv(384, 9216, 3, groups=384, pad_l=1, pad_r=1), 1, 150, F32, True, dw2(1, 1, 1, 12, 1, 3, 1, 1, 3, 1, 4)),
    # ---- FALLBACK
    "fb_rows1": F(conv(32, 1, 3, pad_l=1, pad_r=1), 3, 251, F32, True, fb(128, 1, 6, 6, 1, 1, 2, 32, 97)),             # c_in < 64: not ONE_ROW
    "fb_rows3": F(conv(24, 9, 5, groups=3, pad_l=2, pad_r=2), 8, 100, F32, True, fb(128, 1, 8, 8, 1, 1, 1, 8, 41)),
    "fb_cin1": F(conv(1, 16, 15), 2, 700, F32, True, fb(128, 1, 12, 12, 1, 1, 6, 1, 16)),
    "fb_k41": F(conv(16, 16, 41, stride=4, groups=4, pad_l=20, pad_r=20), 2, 700, F32, True, fb(128, 1, 4, 4, 1, 1, 2, 4, 165)),
    "fb_pw128": F(conv(128, 128, 1), 8, 100, F32, True, fb(32, 1, 32, 32, 1, 8, 4, 128, 129)),                        # X tile over the DW2 budget
    "fb_direct": F(conv(512, 16, 1), 2, 100, F32, True, fb(32, 0, 8, 8, 3, 1, 4, 257, 513)),                          # the !xfits staging
    "fb_l5": F(conv(8, 8, 3, pad_l=1, pad_r=1), 1, 5, F32, True, fb(32, 1, 1, 1, 1, 1, 1, 8, 25)),
    "fb_reflect": F(_refl(**conv(4, 16, 7, pad_l=3, pad_r=3)), 2, 50, F32, True, fb(64, 1, 2, 2, 1, 1, 1, 4, 29)),    # 32 < l_out <= 64
    "fb_convT_masked": F(conv(16, 8, 4, stride=2, pad_l=1, transposed=True, out_slope=0.2), 3, 75, F32, False, fb(128, 1, 3, 3, 1, 1, 1, 8, 33)),
    "fb_cin63": F(conv(63, 1, 3, pad_l=1, pad_r=1), 3, 100, F32, True, fb(64, 1, 6, 6, 1, 1, 2, 63, 190)),            # c_in < 64: not ONE_ROW
    "fb_l511": F(conv(1, 8, 2, pad_r=1), 2, 511, F32, True, fb(128, 1, 8, 8, 1, 1, 4, 1, 3)),                         # one step short of TINY
    # split-K hand-over: 54 chunks over 24 blocks (2 and 3 each); 207 chunks of 32 steps over 64 blocks (3 and 4 each)
    "fb_hand": F(conv(64, 256, 5, groups=64, pad_l=2, pad_r=2), 3, 2203, F32, True, fb(128, 1, 24, 54, 1, 1, 18, 1, 6)),
    "fb_hand_bk32": F(conv(128, 384, 1), 3, 2203, F32, True, fb(32, 1, 64, 207, 1, 24, 69, 128, 129)),
    # ---- TINY
    "tiny_1x3": F(conv(1, 16, 3, pad_l=1, pad_r=1), 3, 600, F32, True, per_item(TINY, 3, 4)),
    "tiny_1x2_l512": F(conv(1, 8, 2, pad_r=1), 2, 512, F32, True, per_item(TINY, 2, 3)),
    "tiny_1x1": F(conv(1, 8, 1), 2, 700, F32, True, per_item(TINY, 2, 2)),
    "tiny_pqmf_l0": F(conv(4, 24, 3, dilation=2, groups=4, pad_l=1, pad_r=1), 3, 1003, F32, True, per_item(TINY, 3, 4)),
    "tiny_reflect": F(_refl(**conv(1, 6, 3, pad_l=1, pad_r=1)), 2, 515, F32, True, per_item(TINY, 2, 4)),
    "tiny_s2": F(conv(1, 8, 3, stride=2, pad_l=1, pad_r=1), 2, 1100, F32, True, per_item(TINY, 2, 4)),
    "tiny_out_act": F(conv(1, 16, 3, pad_l=1, pad_r=1, out_slope=0.2), 2, 600, F32, True, per_item(TINY, 2, 4)),
    # ---- ONE_ROW
    "m1_96": F(conv(96, 1, 3, pad_l=1, pad_r=1), 3, 100, F32, True, per_item(ONE_ROW, 3, 289)),
    "m1_70_dil2": F(conv(70, 1, 3, dilation=2, pad_l=2, pad_r=1), 1, 100, F32, True, per_item(ONE_ROW, 1, 211)),      # 70 = 4 x 16 + 6: two channels past the last wave's four
    "m1_out_act": F(conv(64, 1, 3, pad_l=1, pad_r=1, out_slope=0.2), 3, 130, F32, True, per_item(ONE_ROW, 3, 193)),
    "m1_in_act": F(conv(64, 1, 3, pad_l=1, pad_r=1, in_slope=0.2), 2, 130, F32, True, per_item(ONE_ROW, 2, 193)),
}

HAND_OVER = ("dw2_hand_even_odd", "dw2_hand_3", "dw2_tiles384", "fb_hand", "fb_hand_bk32")

# instantiations no default plan can reach, each with the make_dw2_plan rule that excludes it: none
UNREACHABLE = {}

ROW_CONFIGS = [(2, 2, 2), (3, 1, 1), (2, 1, 1), (1, 1, 1)]   # (FM, FN, WAVES_M) of the 128 / 96 / 64 / 32-row tiles
ALL_DW2 = {rc + (12,) for rc in ROW_CONFIGS} | {(2, 2, 2, 20), (3, 1, 1, 20), (2, 1, 1, 32), (1, 1, 1, 32)}   # + XR
ALL_PACK = {(2, 2), (3, 1), (2, 1), (1, 1)}   # dw_pack_a_kernel<FM, WAVES_M>


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def f32_variant(lib, desc):
    out = (ctypes.c_int * 14)()
    rc = lib.eben_conv1d_bwd_dw_f32_variant(ctypes.byref(desc), out, 14)
    return rc, tuple(out)


def plans(lib, route=None):
    """{name: the query's numbers by field} (the table's expectations are asserted equal to them by name)."""
    got = {n: dict(zip(FIELDS, f32_variant(lib, c.desc())[1])) for n, c in CASES.items()}
    return {n: p for n, p in got.items() if route is None or p["route"] == route}


def span(case, bk):
    s = case.spec()
    return (bk - 1) * s.stride + (s.ksize - 1) * s.dilation + 1


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_route_and_instantiation(lib, name):
    rc, v = f32_variant(lib, CASES[name].desc())
    assert rc == 0, lib.eben_last_error()
    assert v == CASES[name].expect, (name, dict(zip(FIELDS, v)))
    assert name.split("_")[0] == {TINY: "tiny", ONE_ROW: "m1", DW2: "dw2", FALLBACK: "fb"}[v[0]]


def test_table_reaches_every_dw2_instantiation(lib):
    reached = [tuple(p[f] for f in ("FM", "FN", "WAVES_M", "XR")) for p in plans(lib, DW2).values()]
    kernels = set(reached)
    assert not set(UNREACHABLE) & kernels
    assert kernels | set(UNREACHABLE) == ALL_DW2, sorted(ALL_DW2 - kernels - set(UNREACHABLE))
    assert {(k[0], k[2]) for k in kernels} == ALL_PACK
    assert all(reason for reason in UNREACHABLE.values())


def hand_over_conditions(got, l_outs):
    """Blocks that own several chunks, unevenly; one block with three or more; a last time chunk that is part padding."""
    assert any(p["nsplit"] < p["nchunks"] and p["nchunks"] % p["nsplit"] for p in got.values())
    assert any(-(-p["nchunks"] // p["nsplit"]) >= 3 for p in got.values())
    assert any(p["nsplit"] < p["nchunks"] and l_outs[n] % 64 for n, p in got.items())


def test_dw2_cases_hold_the_edges_they_were_chosen_for(lib):
    got = plans(lib, DW2)
    assert any(p["nmt"] == 1 for p in got.values()) and {2, 5} <= {p["nmt"] for p in got.values()}
    hand_over_conditions(got, {n: CASES[n].l_out() for n in got})
    assert all(got[n]["nsplit"] < got[n]["nchunks"] for n in HAND_OVER if n in got)
    # no split at all from 384 tiles up: one block walks every chunk of its tile
    t = got["dw2_tiles384"]
    assert t["nnt"] * t["nmt"] * CASES["dw2_tiles384"].spec().groups >= 384 and t["nsplit"] == 1 and t["nchunks"] == 3
    # a column tile that holds only the bias column
    b = CASES["dw2_96_x20"].spec()
    assert (b.c_in // b.groups) * b.ksize == 128 and got["dw2_96_x20"]["nnt"] == 2 and got["dw2_96_x20"]["row_stride"] == 129
    # grouped layers: 24 rows per group, and 48 tiles of 96 rows
    assert CASES["dw2_grp24"].spec().c_out // CASES["dw2_grp24"].spec().groups == 24
    w = got["dw2_wide_grp"]
    assert w["nnt"] * w["nmt"] * CASES["dw2_wide_grp"].spec().groups == 48 and (w["FM"], w["WAVES_M"]) == (3, 1)
    # transposed layers with and without the mask on the X side, on more than one instantiation
    tr = {n: CASES[n].spec() for n in got if CASES[n].spec().transposed}
    assert {s.out_slope != 1.0 for s in tr.values()} == {True, False}
    assert len({(got[n]["FM"], got[n]["XR"]) for n, s in tr.items() if s.out_slope != 1.0}) >= 2
    assert {BF16X3, BF16X6} <= {CASES[n].math for n in got}
    conv1d = [CASES[n].spec() for n in got if not CASES[n].spec().transposed]
    assert any(s.in_slope != 1.0 for s in conv1d) and any(s.out_slope != 1.0 for s in conv1d)
    assert any(s.reflect for s in conv1d) and any(s.groups > 1 for s in conv1d) and any(s.ksize == 1 for s in conv1d)


def test_fallback_cases_hold_the_edges_they_were_chosen_for(lib):
    got = plans(lib, FALLBACK)
    assert {p["bk"] for p in got.values()} == {128, 64, 32}
    # xfits as the kernel forms it, and both sides of it
    for n, p in got.items():
        assert p["xfits"] == (1 if p["nch_max"] * span(CASES[n], p["bk"]) <= DW_XCAP else 0), n
    assert got["fb_direct"]["xfits"] == 0 and got["fb_direct"]["nch_max"] == 257 and got["fb_direct"]["nnt"] == 3
    assert sum(p["xfits"] == 0 for p in got.values()) == 1
    assert got["fb_pw128"]["bk"] == 32 and got["fb_pw128"]["nmt"] == 8
    hand_over_conditions(got, {n: CASES[n].l_out() for n in got})
    assert all(got[n]["nsplit"] < got[n]["nchunks"] for n in HAND_OVER if n in got)
    assert {got[n]["bk"] for n in HAND_OVER if n in got} == {128, 32}
    rows = {n: CASES[n].spec() for n in got}
    assert any(s.c_out == 1 for s in rows.values())                                 # a single row
    assert any(s.c_out // s.groups == 3 for s in rows.values())                      # three rows per group
    assert any(CASES[n].l_out() == 5 and CASES[n].batch == 1 for n in got)
    assert any(s.reflect for s in rows.values()) and any(s.transposed and s.out_slope != 1.0 for s in rows.values())
    # the layers the streaming kernels decline by one channel / one step
    assert CASES["fb_cin63"].spec().c_in == 63 and CASES["fb_l511"].l_out() == 511


def test_tiny_cases_hold_the_edges_they_were_chosen_for(lib):
    got = plans(lib, TINY)
    specs = {n: CASES[n].spec() for n in got}
    assert {(s.c_in // s.groups) * s.ksize for s in specs.values()} == {3, 2, 1}
    assert all(p["row_stride"] == (specs[n].c_in // specs[n].groups) * specs[n].ksize + 1 <= 4 for n, p in got.items())
    assert all(p["nsplit"] == CASES[n].batch for n, p in got.items())
    assert any(s.groups == 4 and s.dilation == 2 for s in specs.values())
    assert any(s.reflect for s in specs.values()) and any(s.stride == 2 for s in specs.values())
    assert any(s.out_slope == 0.2 for s in specs.values())
    assert any(CASES[n].l_out() == 512 for n in got) and all(CASES[n].l_out() >= 512 for n in got)
    assert any(CASES[n].l_out() % 256 for n in got)
    # the same layer one step shorter is another route's
    a, b = CASES["tiny_1x2_l512"], CASES["fb_l511"]
    assert a.kw == b.kw and a.batch == b.batch and b.length == a.length - 1 and b.expect[0] == FALLBACK


def test_one_row_cases_hold_the_edges_they_were_chosen_for(lib):
    got = plans(lib, ONE_ROW)
    specs = {n: CASES[n].spec() for n in got}
    assert {96, 70} <= {s.c_in for s in specs.values()} and 70 % 16 and 70 % 4
    assert all(p["row_stride"] == 3 * specs[n].c_in + 1 and p["nsplit"] == CASES[n].batch for n, p in got.items())
    assert any(s.dilation == 2 for s in specs.values()) and any(s.pad_l != s.pad_r for s in specs.values())
    assert any(s.out_slope == 0.2 for s in specs.values()) and any(s.in_slope == 0.2 for s in specs.values())
    assert {1, 3} <= {CASES[n].batch for n in got}
    assert dict(CASES["m1_96"].kw, c_in=63) == dict(CASES["fb_cin63"].kw) and CASES["fb_cin63"].expect[0] == FALLBACK


def test_operands_stay_small():
    """About 4 M floats per operand at the most: the float64 oracle and the GPU run of a case take a second or so."""
    for name, case in CASES.items():
        s = case.spec()
        assert case.batch * max(s.c_in * case.length, s.c_out * case.l_out()) <= 4.2e6, name


def test_workspace_follows_the_route(lib):
    """eben_conv1d_bwd_dw_workspace reads the same decision: the slab count is the plan's, the row carries the bias column."""
    for name, case in CASES.items():
        d = case.desc()
        nslab, row_stride = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.eben_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(row_stride)) > 0
        w = case.spec().weight_shape()
        assert (nslab.value, row_stride.value) == (case.plan()["nsplit"], w[1] * w[2] + 1) == (case.expect[7], case.expect[13]), name


def test_dw3_layer_reports_its_route_alone(lib):
    from tests.test_dw3_variants import CASES as DW3_CASES

    rc, v = f32_variant(lib, DW3_CASES["enc_s2"].dw_desc())
    assert rc == 0 and v == (DW3,) + (0,) * 13


def test_both_queries_agree_on_the_route(lib):
    from tests.test_dw3_variants import dw_variant

    for name, case in CASES.items():
        assert dw_variant(lib, case.desc())[1] == (case.expect[0],) + (0,) * 12, name


def test_f32_variant_query_checks_its_arguments(lib):
    d = CASES["dw2_64_x12"].desc()
    out = (ctypes.c_int * 13)()
    assert lib.eben_conv1d_bwd_dw_f32_variant(ctypes.byref(d), out, 13) == -1
    assert lib.eben_conv1d_bwd_dw_f32_variant(ctypes.byref(d), None, 14) == -1
    bad = type(d).from_buffer_copy(d)
    bad.l_out += 1
    assert f32_variant(lib, bad)[0] == -1
