"""CPU (no GPU): which gc_kernel<FORM, RT, CT, NP> instantiation (gen_conv.hip) every launch of the case table runs, asked of the
library's own dispatch decision (eben_conv1d_variant, which reads the plan gc_launch dispatches on), and that the table reaches all 18
of them.  tests/test_gpu_gen_conv_variants.py runs each case against float64; a retuned gc_plan that moves a case off its
instantiation fails here by name.

FORM 0: Conv1d, 5 <= k <= 16 (runs of 8 taps of one channel; k = 16 takes two runs per channel, rpc_shift = 1); FORM 1: Conv1d k = 4
stride 2; FORM 2: ConvTranspose1d k = 2 S, S in (8, 4, 2).  (RT, CT): 32-row x 32-column tiles per wave; gc_plan prefers (1, 1) until it
needs more than one round of 1024 waves (256 blocks), so the wide shapes want batch x columns x rows: the cases get there with 192 or
256 rows (c_out x S / 2 for FORM 2) rather than with long signals.  NP: 3 pieces per operand (EBEN_MATH_BF16X6) or 2 (EBEN_MATH_BF16X3,
the arithmetic of the bf16-mixed training step's generator forward).

What the table exercises, per (RT, CT) (KC = k-steps per weight chunk: 8, 4, 2 for (1,1), (2,1), (2,2); KSP >= 8, so (2,1) cannot run
fewer than 2 chunks nor (2,2) fewer than 4, and a grid under 8 blocks is (1,1)'s alone: the wide shapes win past 256 blocks only):
  column tail          NU off 128 CT with a wave partly in range and one wholly out of it
  mixed tiles          interior waves on the fast path, both row ends on the slow one; CT = 2: a wave with one fast and one end tile
  padding              reflect and zero
  activation on load   in_slope != 1 in launches with fast and slow waves
  epilogue             bias, out_slope, residual; FORM 2 at S = 8, 4, 2
  padding k-steps      c_in 16 / 48 in FORM 1 and 2 (nkg / 2 = 4, 12, 2, 6: FORM 0 has nkg / 2 = c_in or c_in / 2, always whole chunks)
  chunk counts         KSP / KC of 1, 2, 3 (1,1); 2, 4 (2,1); 4, 8 (2,2)
  grid                 under 8 blocks and off a multiple of 8 (the XCD remap with xq = 0 and with xr != 0)
  batch 1, and an input 4 bytes off 16-byte alignment (`offset`)
"""
import ctypes
import os

import pytest

from vibravox_amd import ops

X3, X6 = ops.MATH_BF16X3, ops.MATH_BF16X6
GC = 4   # EBEN_VARIANT_GC


class G:
    """One forward launch: ConvSpec kwargs (activations included), batch, length, math, bias and residual flags, the expected
    (FORM, RT, CT, NP) of gc_kernel, and whether the input is a one-float offset view (4-byte but not 16-byte aligned rows)."""

    def __init__(self, kw, batch, length, math, bias, res, expect, offset=False):
        self.kw, self.batch, self.length, self.math, self.bias, self.res = kw, batch, length, math, bias, res
        self.expect, self.offset = tuple(expect), offset

    def spec(self):
        return ops.ConvSpec(**self.kw)

    def desc(self):
        return ops.conv_desc(self.spec(), self.batch, self.length, self.math)


def conv(c_in, c_out, k, s=1, pad=None, reflect=True, **kw):
    pad = (k - s) // 2 if pad is None else pad
    return dict(c_in=c_in, c_out=c_out, ksize=k, stride=s, pad_l=pad, pad_r=pad, reflect=reflect, **kw)


def convt(c_in, c_out, s, **kw):
    return dict(c_in=c_in, c_out=c_out, ksize=2 * s, stride=s, pad_l=s // 2, transposed=True, **kw)


A, OUT, AO = dict(in_slope=0.01), dict(out_slope=0.2), dict(in_slope=0.01, out_slope=0.2)

# found with gc_plan's cost model replayed on the host, then kept.  Every case has interior waves on the fast path, a wave at each row
# end on the slow one and a column tail (NU off the 128 CT tile: one wave partly in range, at least one wholly out); at CT = 2,
# NU = 370 (batch 1: 4200) puts a fast and an end tile into one wave at both ends.  In comments: grid blocks, chunks = KSP / KC.
CASES = {
    # (1, 1): anything small
    "f0_r1c1_x6_k7_b1": G(conv(48, 32, 7, **A), 1, 200, X6, False, False, (0, 1, 1, 3), offset=True),              # grid 2, 3 chunks
    "f0_r1c1_x3_k5_zero": G(conv(16, 32, 5, reflect=False, **AO), 3, 300, X3, True, True, (0, 1, 1, 2)),           # grid 9, 1 chunk
    "f0_r1c1_x6_k16_s8": G(conv(16, 32, 16, 8, **OUT), 2, 1100, X6, True, False, (0, 1, 1, 3)),                     # grid 4, 2 chunks
    "f0_r1c1_x3_k16_s8_b1": G(conv(16, 32, 16, 8, **A), 1, 2100, X3, False, True, (0, 1, 1, 2), offset=True),      # grid 3
    "f1_r1c1_x6_b1": G(conv(16, 32, 4, 2, **AO), 1, 700, X6, True, True, (1, 1, 1, 3), offset=True),               # 4 of 8 k-steps real
    "f1_r1c1_x3": G(conv(48, 64, 4, 2, **A), 3, 400, X3, False, False, (1, 1, 1, 2)),                              # grid 12, 12 of 16
    "f2_r1c1_x6_s8_b1": G(convt(16, 8, 8, **AO), 1, 200, X6, True, True, (2, 1, 1, 3)),                            # 2 of 8 k-steps real
    "f2_r1c1_x3_s4": G(convt(48, 16, 4, **A), 3, 300, X3, True, True, (2, 1, 1, 2)),                               # grid 18, 6 of 8
    "f2_r1c1_x3_s2": G(convt(80, 32, 2, **OUT), 2, 170, X3, True, True, (2, 1, 1, 2)),                             # 10 of 16, 2 chunks
    "f2_r1c1_x6_s2_b1": G(convt(208, 32, 2), 1, 170, X6, False, False, (2, 1, 1, 3)),                              # 26 of 32, 4 chunks
    # (2, 1): (1, 1) would need a second round of 1024 waves
    "f0_r2c1_x6_k7": G(conv(16, 192, 7, **A), 15, 330, X6, True, False, (0, 2, 1, 3)),                             # grid 135, 2 chunks
    "f0_r2c1_x3_k5_zero": G(conv(32, 256, 5, reflect=False, **AO), 17, 200, X3, True, True, (0, 2, 1, 2), offset=True),   # 4 chunks
    "f0_r2c1_x3_k16_s8": G(conv(16, 256, 16, 8, **A), 17, 1600, X3, False, False, (0, 2, 1, 2)),
    "f1_r2c1_x6": G(conv(16, 256, 4, 2, reflect=False, **A), 17, 400, X6, False, True, (1, 2, 1, 3), offset=True),
    "f1_r2c1_x3": G(conv(48, 192, 4, 2, **AO), 15, 660, X3, True, False, (1, 2, 1, 2), offset=True),               # grid 135
    "f2_r2c1_x6_s8": G(convt(16, 64, 8, **AO), 9, 200, X6, True, True, (2, 2, 1, 3)),
    "f2_r2c1_x3_s4": G(convt(48, 128, 4, **AO), 9, 200, X3, True, True, (2, 2, 1, 2)),
    "f2_r2c1_x3_s2_b1": G(convt(16, 256, 2, **A), 1, 2200, X3, False, True, (2, 2, 1, 2), offset=True),
    # (2, 2): (2, 1) would need a second round as well
    "f0_r2c2_x6_k7": G(conv(16, 256, 7, **A), 22, 370, X6, False, True, (0, 2, 2, 3), offset=True),                # 4 chunks
    "f0_r2c2_x3_k8_s4": G(conv(32, 192, 8, 4, **AO), 29, 1480, X3, True, False, (0, 2, 2, 2)),                     # grid 174, 8 chunks
    "f0_r2c2_x3_k16_s8": G(conv(16, 256, 16, 8, reflect=False, **A), 22, 2960, X3, True, True, (0, 2, 2, 2)),
    "f1_r2c2_x6": G(conv(16, 256, 4, 2, **AO), 22, 740, X6, True, True, (1, 2, 2, 3)),
    "f1_r2c2_x3": G(conv(48, 256, 4, 2, reflect=False, **A), 22, 740, X3, False, False, (1, 2, 2, 2), offset=True),
    "f2_r2c2_x6_s4": G(convt(16, 128, 4, **A), 11, 370, X6, True, True, (2, 2, 2, 3)),
    "f2_r2c2_x3_s8": G(convt(48, 64, 8, **AO), 11, 370, X3, True, True, (2, 2, 2, 2)),
    "f2_r2c2_x6_s2_b1": G(convt(16, 256, 2), 1, 4200, X6, False, True, (2, 2, 2, 3)),
    "f2_r2c2_x3_s2": G(convt(16, 256, 2, **A), 11, 370, X3, True, False, (2, 2, 2, 2), offset=True),
}

# instantiations no default plan reaches at batch <= 64 and length <= 8192, each with the gc_plan rule that excludes it: none
UNREACHABLE = {}

ALL_GC = {(form, rt, ct, np_) for form in (0, 1, 2) for (rt, ct) in ((1, 1), (2, 1), (2, 2)) for np_ in (2, 3)}


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def variant(lib, case):
    out = (ctypes.c_int * 8)()
    d = case.desc()
    rc = lib.eben_conv1d_variant(ctypes.byref(d), 0, 0, out, 8)
    return rc, tuple(out)


def gc_tuple(lib, name, case):
    rc, v = variant(lib, case)
    assert rc == 0, (name, lib.eben_last_error())
    assert v[0] == ops.CONV_ROUTE_GC and v[7] == GC and v[5:7] == (0, 0), (name, v)
    return v[1:5]


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_gc_instantiation(lib, name):
    case = CASES[name]
    d = case.desc()
    assert lib.eben_conv1d_kernel_generation(ctypes.byref(d), 0) == ops.CONV_ROUTE_GC, name
    got = gc_tuple(lib, name, case)
    assert got == case.expect, f"{name}: runs gc_kernel{got}, the case is written for {case.expect}"
    assert got[3] == (3 if case.math == X6 else 2), name


def test_table_reaches_every_gc_instantiation(lib):
    reached = {gc_tuple(lib, n, c) for n, c in CASES.items()}
    assert len(ALL_GC) == 18
    assert not set(UNREACHABLE) & reached, set(UNREACHABLE) & reached
    assert reached | set(UNREACHABLE) == ALL_GC, sorted(ALL_GC - reached - set(UNREACHABLE))
    assert all(reason for reason in UNREACHABLE.values())


def test_table_covers_the_edges_at_every_tile_shape():
    """What the module docstring lists, counted off the table per (RT, CT) -- host arithmetic on the specs only."""
    for shape in ((1, 1), (2, 1), (2, 2)):
        cs = [c for c in CASES.values() if c.expect[1:3] == shape]
        specs = [c.spec() for c in cs]
        assert {c.expect[3] for c in cs} == {2, 3}, shape
        assert {s.reflect for s in specs if not s.transposed} == {True, False}, shape
        assert {s.stride for s in specs if s.transposed} == {8, 4, 2}, shape
        assert {s.ksize for s in specs if not s.transposed} >= {4, 7, 16}, shape            # FORM 1, FORM 0 with one and two runs per channel
        for np_ in (2, 3):
            sub = [c for c in cs if c.expect[3] == np_]
            assert any(c.spec().in_slope != 1.0 for c in sub) and any(c.spec().out_slope != 1.0 for c in sub), (shape, np_)
            assert any(c.bias for c in sub) and any(c.res for c in sub) and any(c.offset for c in sub), (shape, np_)
        assert any(c.batch == 1 for c in cs), shape
        assert any(c.res and c.spec().transposed and c.spec().stride == 8 for c in cs), shape   # the 16-byte residual load
        assert any(c.spec().c_in in (16, 48) and (c.spec().transposed or c.spec().ksize == 4) for c in cs), shape   # padding k-steps
        # column tail: the last block's columns end inside one wave (32 CT columns) and leave at least one wave empty
        tile = 32 * shape[1]
        tails = [(c.length if c.spec().transposed else c.spec().out_len(c.length)) % (4 * tile) for c in cs]
        assert any(r % tile and r <= 3 * tile for r in tails), shape


def test_variant_query_reports_nothing_for_input_gradients_of_these_layers(lib):
    """Generation 5 serves forwards only: the input gradient of the same layer reports another generation and its own slots."""
    case = CASES["f0_r2c2_x6_k7"]
    out = (ctypes.c_int * 8)()
    d = case.desc()
    assert lib.eben_conv1d_variant(ctypes.byref(d), 1, 0, out, 8) == 0
    assert out[0] != ops.CONV_ROUTE_GC and out[7] != GC
