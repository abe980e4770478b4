"""CPU (no GPU): which weight-gradient route and which conv_dw3.hip instantiation every case of the table runs, asked of the library's
own dispatch decision (eben_conv1d_bwd_dw_variant: the function eben_conv1d_bwd_dw_workspace and eben_conv1d_bwd_dw dispatch on), and
that the table reaches every instantiation the dispatch can pick.  tests/test_gpu_dw3_routes.py runs each case against the float64
oracle of tests/dw_oracle.py; a retuned plan that moves a case off its instantiation, or off the edge it was chosen for, fails here by name.

conv_dw3_kernel<FM, FN, WAVES_M, XRB, SP> behind dw3_pack_a_kernel<MT> (conv_dw3.hip, make_dw3_plan): four row configurations -- the
row tile of 128 / 96 / 64 / 32 rows that pads the rows per group least: (FM, FN, WAVES_M) = (2, 2, 2) / (3, 1, 1) / (2, 1, 1) / (1, 1, 1),
MT = FM * WAVES_M 32-row tiles -- times three X-tile forms: eight staging units per thread (XRB 8: the strided and dilated layers'
long spans), four (XRB 4), and four with hi + lo tiles (SP: a Conv1d under EBEN_MATH_BF16X2, whose plans are held to four units).
All 12 + 4 instantiations are reached by default plans, so UNREACHABLE is empty.

The cases are the generator's layer forms under the bf16-mixed plan: reflect-padded strided convs, the latent / first / last convs,
ConvTranspose1d (operands swapped by the dispatcher; with a fused output activation the layer reaches the kernel pre-masked, as
ops.weight_grads hands it over: `dw_desc`), input activations applied on load, dilated ResidualUnit-style convs, zero-padded layers.
"""
import ctypes
import dataclasses
import os

import pytest

from vibravox_amd import ops

BF16, BF16X2, BF16X3, BF16X6 = ops.MATH_BF16, ops.MATH_BF16X2, ops.MATH_BF16X3, ops.MATH_BF16X6
TINY, ONE_ROW, DW3, DW2, FALLBACK = 0, 1, 2, 3, 4   # EBEN_DW_ROUTE_*
FIELDS = ("route", "FM", "FN", "WAVES_M", "XRB", "SP", "MT", "BKT", "nsplit", "nchunks", "nnt", "nmt", "nbg")


class W:
    """One weight gradient: ConvSpec kwargs, batch, length, math, bias, and the 13 numbers of eben_conv1d_bwd_dw_variant
    (FIELDS) -- for a fall-through case the route alone."""

    def __init__(self, kw, batch, length, math, bias, expect):
        self.kw, self.batch, self.length, self.math, self.bias = kw, batch, length, math, bias
        self.expect = tuple(expect) if isinstance(expect, tuple) else (expect,) + (0,) * 12

    def spec(self):
        return ops.ConvSpec(**self.kw)

    def premasked(self):
        """A transposed layer with a fused output activation reaches conv_dw3 with its gradient already masked (ops.weight_grads)."""
        s = self.spec()
        return s.transposed and s.out_slope != 1.0 and self.math in (BF16, BF16X2)

    def dw_spec(self):
        s = self.spec()
        return dataclasses.replace(s, out_slope=1.0) if self.premasked() else s

    def dw_desc(self):
        """The descriptor eben_conv1d_bwd_dw is given."""
        return ops.conv_desc(self.dw_spec(), self.batch, self.length, self.math)

    def l_out(self):
        return self.spec().out_len(self.length)

    def plan(self):
        return dict(zip(FIELDS, self.expect))

    def right_overhang(self):
        """Samples the last output's last tap reaches past the end of the input row (a Conv1d)."""
        s = self.spec()
        return (self.l_out() - 1) * s.stride - s.pad_l + (s.ksize - 1) * s.dilation - (self.length - 1)


def _refl(**kw):
    return dict(reflect=True, **kw)


ENC_S2 = _refl(c_in=32, c_out=64, ksize=4, stride=2, pad_l=1, pad_r=1)
ENC_S4 = _refl(c_in=64, c_out=128, ksize=8, stride=4, pad_l=3, pad_r=3)
ENC_S8 = _refl(c_in=128, c_out=256, ksize=16, stride=8, pad_l=7, pad_r=7, in_slope=0.01)
LATENT_UP = _refl(c_in=64, c_out=256, ksize=7, pad_l=3, pad_r=3, out_slope=0.01)
FIRST = _refl(c_in=4, c_out=32, ksize=3, pad_l=1, pad_r=1)
ROWS96 = dict(c_in=24, c_out=96, ksize=5, pad_l=2, pad_r=2)

# plans confirmed by the query, then kept.  Lengths: the right reflection overhang is non-zero, and smaller than the left pad on the
# stride-4 / 8 layers (303: 2 of 3; 103: 2 of 3; 1005: 4 of 7; stride 2 at 204 / 102: 1 of 1), l_out off the time chunk (BKT) and off the pack kernel's
# 32-step tile; batches 8 (half a group), 9 and 17 (one item past a group), 16 and 24, 33 (a trailing group of one item)
CASES = {
    "enc_s2": W(ENC_S2, 9, 204, BF16, True, (DW3, 2, 1, 1, 8, 0, 2, 8, 13, 13, 2, 1, 1)),
    "enc_s2_x2": W(ENC_S2, 9, 204, BF16X2, True, (DW3, 2, 1, 1, 4, 1, 2, 4, 26, 26, 2, 1, 1)),
    "enc_s4": W(ENC_S4, 16, 303, BF16, True, (DW3, 2, 2, 2, 8, 0, 4, 8, 10, 10, 5, 1, 1)),
    "enc_s4_x2": W(ENC_S4, 16, 303, BF16X2, True, (DW3, 2, 2, 2, 4, 1, 4, 4, 19, 19, 5, 1, 1)),
    # split-K hand-over: 32 chunks over 23 blocks (blocks own 1 and 2), 64 over 23 (2 and 3)
    "enc_s8_long": W(ENC_S8, 17, 1005, BF16, True, (DW3, 2, 2, 2, 8, 0, 4, 8, 23, 32, 17, 2, 2)),
    "enc_s8_long_x2": W(ENC_S8, 17, 1005, BF16X2, True, (DW3, 2, 2, 2, 4, 1, 4, 4, 23, 64, 17, 2, 2)),
    "latent_down": W(_refl(c_in=256, c_out=64, ksize=7, pad_l=3, pad_r=3, in_slope=0.01, out_slope=0.01), 8, 37, BF16, True,
                     (DW3, 2, 1, 1, 4, 0, 2, 16, 3, 3, 15, 1, 1)),
    "latent_up": W(LATENT_UP, 24, 37, BF16, True, (DW3, 2, 2, 2, 4, 0, 4, 16, 6, 6, 4, 2, 2)),
    "latent_up_x2": W(LATENT_UP, 24, 37, BF16X2, True, (DW3, 2, 2, 2, 4, 1, 4, 16, 6, 6, 4, 2, 2)),
    "first_conv": W(FIRST, 8, 130, BF16, True, (DW3, 1, 1, 1, 4, 0, 1, 32, 5, 5, 1, 1, 1)),
    "first_conv_x2": W(FIRST, 8, 130, BF16X2, True, (DW3, 1, 1, 1, 4, 1, 1, 32, 5, 5, 1, 1, 1)),
    "last_conv": W(_refl(c_in=32, c_out=4, ksize=3, pad_l=1, pad_r=1), 8, 130, BF16, True, (DW3, 1, 1, 1, 8, 0, 1, 16, 9, 9, 1, 1, 1)),
    "dec_s8": W(dict(c_in=256, c_out=128, ksize=16, stride=8, pad_l=4, transposed=True, out_slope=0.01), 9, 41, BF16, False,
                (DW3, 2, 2, 2, 8, 0, 4, 8, 6, 6, 17, 2, 1)),
    "dec_s4": W(dict(c_in=128, c_out=64, ksize=8, stride=4, pad_l=2, transposed=True, in_slope=0.01), 16, 75, BF16, False,
                (DW3, 2, 2, 2, 8, 0, 4, 8, 10, 10, 5, 1, 1)),
    # three batch groups, the last holding one item
    "dec_s2": W(dict(c_in=64, c_out=32, ksize=4, stride=2, pad_l=1, transposed=True, in_slope=0.01, out_slope=0.01), 33, 150, BF16, False,
                (DW3, 2, 1, 1, 8, 0, 2, 8, 57, 57, 2, 1, 3)),
    "rows96": W(ROWS96, 8, 100, BF16, True, (DW3, 3, 1, 1, 4, 0, 3, 16, 7, 7, 1, 1, 1)),
    "rows96_x2": W(ROWS96, 8, 100, BF16X2, True, (DW3, 3, 1, 1, 4, 1, 3, 16, 7, 7, 1, 1, 1)),
    "rows96_wide": W(_refl(c_in=32, c_out=96, ksize=4, stride=2, pad_l=1, pad_r=1), 8, 102, BF16, True, (DW3, 3, 1, 1, 8, 0, 3, 8, 7, 7, 2, 1, 1)),
    # 16 channels x 8 taps = 128 columns: the second column tile holds the bias column alone
    "bias_col_alone": W(_refl(c_in=16, c_out=32, ksize=8, stride=4, pad_l=3, pad_r=3), 8, 103, BF16, True, (DW3, 1, 1, 1, 4, 0, 1, 4, 7, 7, 2, 1, 1)),
    "dil9_32": W(_refl(c_in=32, c_out=32, ksize=3, dilation=9, pad_l=9, pad_r=9), 8, 70, BF16, True, (DW3, 1, 1, 1, 8, 0, 1, 8, 9, 9, 1, 1, 1)),
    # four-step chunks on the 156 KB budget (131 KB of LDS)
    "dil9_128": W(_refl(c_in=128, c_out=128, ksize=3, dilation=9, pad_l=9, pad_r=9), 8, 70, BF16, True, (DW3, 2, 2, 2, 8, 0, 4, 4, 18, 18, 4, 1, 1)),
}

# instantiations no default plan can reach, each with the make_dw3_plan rule that excludes it: none
UNREACHABLE = {}

ROW_CONFIGS = [(2, 2, 2), (3, 1, 1), (2, 1, 1), (1, 1, 1)]   # (FM, FN, WAVES_M) of the 128 / 96 / 64 / 32-row tiles
ALL_DW3 = {rc + form for rc in ROW_CONFIGS for form in ((8, 0), (4, 0), (4, 1))}   # + (XRB, SP)
ALL_PACK = {1, 2, 3, 4}   # dw3_pack_a_kernel<MT>

# bf16-math layers that must NOT reach conv_dw3, and the route that serves them
FALL_THROUGH = {
    "batch7": W(ENC_S2, 7, 204, BF16, True, DW2),                                         # fewer than 8 batch items per k-step group
    "rows3": W(dict(c_in=24, c_out=9, ksize=5, groups=3, pad_l=2, pad_r=2), 8, 100, BF16, True, FALLBACK),   # 3 rows per group
    "cols6": W(_refl(c_in=2, c_out=32, ksize=3, pad_l=1, pad_r=1), 8, 130, BF16, True, DW2),    # 6 columns per group
    "bf16x3": W(ENC_S2, 9, 204, BF16X3, True, DW2),                                       # operands split on both sides: exact fp32
    "bf16x6": W(ENC_S2, 9, 204, BF16X6, True, DW2),
    "convT_masked": W(dict(c_in=256, c_out=128, ksize=16, stride=8, pad_l=4, transposed=True, out_slope=0.01), 9, 41, BF16, False, DW2),   # not pre-masked
    "pointwise128": W(dict(c_in=128, c_out=128, ksize=1), 8, 100, BF16, True, FALLBACK),   # X tile of 128 channels: over the LDS budget
    "logits": W(dict(c_in=96, c_out=1, ksize=3, pad_l=1, pad_r=1), 8, 100, BF16, True, ONE_ROW),
    "tiny": W(dict(c_in=1, c_out=16, ksize=3, pad_l=1, pad_r=1), 8, 600, BF16, True, TINY),
}


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def dw_variant(lib, desc):
    out = (ctypes.c_int * 13)()
    rc = lib.eben_conv1d_bwd_dw_variant(ctypes.byref(desc), out, 13)
    return rc, tuple(out)


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_dw3_instantiation(lib, name):
    rc, v = dw_variant(lib, CASES[name].dw_desc())
    assert rc == 0, lib.eben_last_error()
    assert v == CASES[name].expect, (name, dict(zip(FIELDS, v)))


def test_table_reaches_every_dw3_instantiation(lib):
    reached = [dw_variant(lib, c.dw_desc())[1] for c in CASES.values()]
    assert all(v[0] == DW3 for v in reached)
    kernels = {v[1:6] for v in reached}
    assert not set(UNREACHABLE) & kernels
    assert kernels | set(UNREACHABLE) == ALL_DW3, sorted(ALL_DW3 - kernels - set(UNREACHABLE))
    assert {v[6] for v in reached} == ALL_PACK
    assert all(v[6] == v[1] * v[3] for v in reached)   # MT = FM * WAVES_M
    assert all(reason for reason in UNREACHABLE.values())


def test_table_holds_the_edges_it_was_chosen_for(lib):
    """Read off the query's numbers (the table's expectations were asserted equal to them above)."""
    got = {n: dict(zip(FIELDS, dw_variant(lib, c.dw_desc())[1])) for n, c in CASES.items()}
    assert {8, 9, 16, 17, 24, 33} <= {c.batch for c in CASES.values()}
    assert any(p["nmt"] == 1 for p in got.values()) and any(p["nmt"] > 1 for p in got.values())
    assert all(p["nbg"] == -(-CASES[n].batch // 16) for n, p in got.items())
    # blocks that own several chunks (the double-buffered hand-over of the K loop), unevenly; one block with three or more
    for math in (BF16, BF16X2):
        assert any(p["nsplit"] < p["nchunks"] and p["nchunks"] % p["nsplit"] for n, p in got.items() if CASES[n].math == math), math
    assert any(-(-p["nchunks"] // p["nsplit"]) >= 3 for p in got.values())
    assert any(CASES[n].l_out() % p["BKT"] for n, p in got.items())
    assert any(CASES[n].l_out() % 32 for n in got)
    # a column tile that holds only the bias column
    b = CASES["bias_col_alone"].spec()
    assert (b.c_in // b.groups) * b.ksize == 128 and got["bias_col_alone"]["nnt"] == 2
    # reflection: the right edge is mirrored in every reflect case, and by fewer samples than the left one (pad_l) on the stride-4 / 8
    # layers -- the two pads differ in effect though pad_l == pad_r
    refl = [c for c in CASES.values() if c.spec().reflect]
    assert all(0 < c.right_overhang() <= c.spec().pad_r for c in refl)
    assert all(c.right_overhang() < c.spec().pad_l for c in refl if c.spec().stride >= 4)
    # the hi + lo tiles of strided reflect layers drop to four-step chunks
    assert all(got[n]["BKT"] == 4 and got[n]["SP"] == 1 for n in ("enc_s2_x2", "enc_s4_x2", "enc_s8_long_x2"))


@pytest.mark.parametrize("name", list(FALL_THROUGH))
def test_layer_outside_dw3_takes_its_route(lib, name):
    case = FALL_THROUGH[name]
    d = ops.conv_desc(case.spec(), case.batch, case.length, case.math)   # as given: no pre-mask
    rc, v = dw_variant(lib, d)
    assert rc == 0, lib.eben_last_error()
    assert v == case.expect, (name, v)


def test_unmasked_transposed_layer_is_refused_by_dw3_and_taken_pre_masked(lib):
    case = CASES["dec_s8"]
    assert case.premasked()
    raw = ops.conv_desc(case.spec(), case.batch, case.length, case.math)
    assert dw_variant(lib, raw)[1][0] == DW2
    assert dw_variant(lib, case.dw_desc())[1][0] == DW3


def test_variant_query_checks_its_arguments(lib):
    d = CASES["enc_s2"].dw_desc()
    out = (ctypes.c_int * 12)()
    assert lib.eben_conv1d_bwd_dw_variant(ctypes.byref(d), out, 12) == -1
    assert lib.eben_conv1d_bwd_dw_variant(ctypes.byref(d), None, 13) == -1
    bad = type(d).from_buffer_copy(d)
    bad.l_out += 1
    assert dw_variant(lib, bad)[0] == -1


def test_workspace_follows_the_route(lib):
    """eben_conv1d_bwd_dw_workspace reads the same decision: the slab count is the plan's nsplit, the row carries the bias column."""
    for name, case in CASES.items():
        d = case.dw_desc()
        nslab, row_stride = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.eben_conv1d_bwd_dw_workspace(ctypes.byref(d), ctypes.byref(nslab), ctypes.byref(row_stride)) > 0
        w = case.spec().weight_shape()
        assert (nslab.value, row_stride.value) == (case.plan()["nsplit"], w[1] * w[2] + 1), name
