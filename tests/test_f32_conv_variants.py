"""CPU (no GPU): which kernel instantiation every launch of the case table runs on the exact-fp32 forward / input-gradient families,
asked of the library's own dispatch decision (eben_conv1d_variant_f32: the helpers thin_launch and tap2_launch dispatch on), and
that the table reaches every thin_kernel and tap2_kernel instantiation and the fallback.  tests/test_gpu_f32_conv_variants.py runs
each case against a float64 conv; a retuned plan that moves a case off its instantiation fails here by name.

thin_kernel<MT, BN, NP> (thinconv.hip, 12 instantiations): MT rows per thread (1 / 4 / 8 / 16 by the rows per group), BN threads (128
for launches of at most 128 positions, or when 256 need more than 72 KB of LDS), NP = 4 positions per thread on launches of at
least 4096 positions and 2048 blocks (back to 1 when four need more than 72 KB).  Past the template arguments the query reports
id_fast (0: the grid is too large for the multiply-high decomposition of the block id), pg_n (0: more than 8 stride phases, the
kernel computes its phase geometry itself) and the launch's LDS bytes.

tap2_kernel<FM, 4, XR, H16, IMT> (exact_fp32/tapconv2.hip, 15 instantiations): FM 32-row fragments per block (shrunk while fewer than
256 blocks would run, hence batch 8 on the tall ones), XR = 28 staging elements where 16 would leave a channel chunk less than two
weight chunks, the 16-row H16 form for 8..16 rows over a reduction the thin kernel refuses, and on the XR = 28 forms the
mask-on-load switch compiled in (IMT 0 / 1; -1: a run-time switch).  Past those: ncc channel chunks, nxbuf input-tile buffers, and
whether two buffers are the aligned hand-over.

Every instantiation of both is reachable with the default settings, so UNREACHABLE is empty.
"""
import ctypes
import os

import pytest

from vibravox_amd import ops

FWD, DX = 0, 1
TAP1, TAP2, THIN = ops.CONV_ROUTE_TAP1, ops.CONV_ROUTE_TAP2, ops.CONV_ROUTE_THIN
# the launch forms of the GPU test and the (direction, whether the gradient is masked as it is staged) each one is
FORMS = {"fwd": FWD, "fwd_res": FWD, "dx": DX, "dx_res": DX, "dx_ex": DX, "dx_fm": DX}


class C:
    """One launch: ConvSpec kwargs (the activations are the GPU test's), batch, length, direction (FWD: the layer's forward; DX: its
    input gradient), mask on load, the GPU test's launch form, the expected EBEN_CONV_ROUTE_* and the expected fields behind it --
    THIN: (MT, BN, NP, id_fast, pg_n, lds_bytes, 0); TAP2: (FM, XR, H16, IMT, ncc, nxbuf, aligned); TAP1: zeros."""

    def __init__(self, kw, batch, length, direction, mask_on_load, form, route, expect):
        self.kw, self.batch, self.length, self.direction, self.mask_on_load = kw, batch, length, direction, mask_on_load
        self.form, self.route, self.expect = form, route, tuple(expect)

    def spec(self):
        return ops.ConvSpec(**self.kw)

    def desc(self, spec=None, batch=None):
        return ops.conv_desc(spec or self.spec(), batch or self.batch, self.length, ops.MATH_F32)

    def elements(self):
        s = self.spec()
        return self.batch * (s.c_in * self.length + s.c_out * s.out_len(self.length))


# generated from the query, then kept: lengths off the tile and off the stride, rows off the row tile (3 / 6 / 12 rows on 4 / 8 / 16),
# several row tiles (32, 64 and 768 rows), one- and many-block launches, Conv1d and ConvTranspose1d in both passes
CASES = {
    "thin_mt1_bn256_reflect": C(dict(c_in=12, c_out=4, ksize=5, dilation=2, groups=4, pad_l=4, pad_r=4, reflect=True), 3, 1003, FWD, 0, "fwd", THIN, (1, 256, 1, 1, 1, 3192, 0)),
    "thin_mt4_bn256_mg3": C(dict(c_in=4, c_out=12, ksize=3, dilation=2, groups=4, pad_l=2, pad_r=2), 3, 1003, FWD, 0, "fwd_res", THIN, (4, 256, 1, 1, 1, 1048, 0)),
    "thin_mt8_bn256_mg6_fm": C(dict(c_in=24, c_out=48, ksize=7, stride=2, dilation=3, groups=4, pad_l=3, pad_r=3), 8, 999, DX, 0, "dx_fm", THIN, (8, 256, 1, 1, 2, 12816, 0)),
    "thin_mt8_bn256_mg6_fwd": C(dict(c_in=4, c_out=24, ksize=3, dilation=2, groups=4, pad_l=2, pad_r=2), 3, 1003, FWD, 0, "fwd", THIN, (8, 256, 1, 1, 1, 1048, 0)),
    "thin_mt16_bn256_mg12_dx": C(dict(c_in=48, c_out=32, ksize=7, stride=2, groups=4, pad_l=3, pad_r=3), 3, 1001, DX, 1, "dx", THIN, (16, 256, 1, 1, 2, 8352, 0)),
    "thin_mt16_bn256_melgan_l1": C(dict(c_in=16, c_out=64, ksize=41, stride=4, groups=4, pad_l=20, pad_r=20), 2, 2100, FWD, 0, "fwd", THIN, (16, 256, 1, 1, 1, 17152, 0)),
    "thin_mt16_bn256_mg768": C(dict(c_in=768, c_out=1, ksize=3, pad_l=1, pad_r=1), 4, 251, DX, 0, "dx_ex", THIN, (16, 256, 1, 1, 1, 1040, 0)),
    "thin_mt4_bn256_fold": C(dict(c_in=4, c_out=32, ksize=7, pad_l=3, pad_r=3, reflect=True), 2, 517, DX, 1, "dx_res", THIN, (4, 256, 1, 1, 1, 33792, 0)),
    "thin_mt1_bn256_pg0": C(dict(c_in=4, c_out=16, ksize=16, stride=16, groups=4), 2, 4803, DX, 1, "dx", THIN, (1, 256, 1, 1, 0, 4128, 0)),
    "thin_mt1_bn256_np_backoff": C(dict(c_in=4, c_out=80, ksize=8, stride=8, groups=4), 13, 32800, DX, 1, "dx", THIN, (1, 256, 1, 1, 8, 20640, 0)),
    "thin_mt16_bn256_tiny_k_mg64": C(dict(c_in=64, c_out=4, ksize=7, stride=2, pad_l=3, pad_r=3), 3, 333, DX, 1, "dx", THIN, (16, 256, 1, 1, 2, 4176, 0)),
    "thin_mt1_bn128_melgan_l0_dx": C(dict(c_in=1, c_out=16, ksize=15, pad_l=7, pad_r=7), 5, 100, DX, 0, "dx_res", THIN, (1, 128, 1, 1, 1, 9216, 0)),
    "thin_mt4_bn128_convT": C(dict(c_in=32, c_out=4, ksize=4, stride=2, pad_l=1, transposed=True), 3, 61, FWD, 0, "fwd", THIN, (4, 128, 1, 1, 2, 16768, 0)),
    "thin_mt16_bn128_convT_dx": C(dict(c_in=32, c_out=4, ksize=4, stride=2, pad_l=1, transposed=True), 3, 61, DX, 1, "dx", THIN, (16, 128, 1, 1, 1, 4192, 0)),
    "thin_mt8_bn128_k_lt_stride": C(dict(c_in=8, c_out=8, ksize=2, stride=4), 4, 97, DX, 0, "dx_ex", THIN, (8, 128, 1, 1, 4, 4160, 0)),
    "thin_mt16_bn128_first_conv": C(dict(c_in=2, c_out=32, ksize=3, pad_l=1, pad_r=1, reflect=True), 3, 125, FWD, 0, "fwd_res", THIN, (16, 128, 1, 1, 1, 1056, 0)),
    "thin_mt8_bn128_lds": C(dict(c_in=64, c_out=8, ksize=4, stride=4), 2, 2003, FWD, 0, "fwd_res", THIN, (8, 128, 1, 1, 1, 133120, 0)),
    "thin_mt1_bn128_id_slow": C(dict(c_in=4, c_out=4, ksize=64, stride=64, groups=4), 4096, 64, DX, 0, "dx_ex", THIN, (1, 128, 1, 0, 0, 520, 0)),
    "thin_np4_mt1": C(dict(c_in=16, c_out=16, ksize=3, groups=16, pad_l=1, pad_r=1), 32, 4100, FWD, 0, "fwd", THIN, (1, 256, 4, 1, 1, 4112, 0)),
    "thin_np4_mt4": C(dict(c_in=4, c_out=12, ksize=3, dilation=2, groups=4, pad_l=2, pad_r=2), 103, 4100, FWD, 0, "fwd_res", THIN, (4, 256, 4, 1, 1, 4120, 0)),
    "thin_np4_mt8": C(dict(c_in=4, c_out=24, ksize=7, stride=2, groups=4, pad_l=3, pad_r=3, reflect=True), 103, 8199, FWD, 0, "fwd", THIN, (8, 256, 4, 1, 1, 8232, 0)),
    "thin_np4_mt16": C(dict(c_in=4, c_out=36, ksize=3, groups=4, pad_l=1, pad_r=1), 103, 4100, FWD, 0, "fwd", THIN, (16, 256, 4, 1, 1, 4112, 0)),
    "thin_np4_mt4_melgan_l1_dx": C(dict(c_in=16, c_out=64, ksize=41, stride=4, groups=4, pad_l=20, pad_r=20), 28, 16400, DX, 0, "dx_ex", THIN, (4, 256, 4, 1, 4, 66304, 0)),
    "tap2_fm1_x16": C(dict(c_in=16, c_out=24, ksize=3, pad_l=1, pad_r=1), 3, 700, FWD, 0, "fwd_res", TAP2, (1, 16, 0, -1, 1, 1, 0)),
    "tap2_fm1_x16_reflect": C(dict(c_in=32, c_out=32, ksize=3, dilation=9, pad_l=9, pad_r=9, reflect=True), 3, 600, FWD, 0, "fwd", TAP2, (1, 16, 0, -1, 1, 1, 0)),
    "tap2_fm1_x16_fold": C(dict(c_in=32, c_out=32, ksize=3, dilation=3, pad_l=3, pad_r=3, reflect=True), 2, 333, DX, 1, "dx_res", TAP2, (1, 16, 0, -1, 1, 1, 0)),
    "tap2_fm1_x16_nx2": C(dict(c_in=32, c_out=24, ksize=15, stride=4, pad_l=7, pad_r=7), 2, 301, FWD, 0, "fwd", TAP2, (1, 16, 0, -1, 6, 2, 0)),
    "tap2_fm1_x16_aligned": C(dict(c_in=8, c_out=24, ksize=16, stride=16, pad_l=7, pad_r=7), 2, 1003, FWD, 0, "fwd_res", TAP2, (1, 16, 0, -1, 4, 2, 1)),
    "tap2_h16_x16": C(dict(c_in=8, c_out=8, ksize=41, stride=4, pad_l=20, pad_r=20), 2, 301, FWD, 0, "fwd", TAP2, (1, 16, 1, -1, 1, 1, 0)),
    "tap2_h16_x28_im0": C(dict(c_in=16, c_out=8, ksize=41, stride=4, pad_l=20, pad_r=20), 2, 301, FWD, 0, "fwd_res", TAP2, (1, 28, 1, 0, 4, 2, 0)),
    "tap2_h16_x28_im1": C(dict(c_in=8, c_out=64, ksize=41, stride=4, pad_l=20, pad_r=20), 2, 301, DX, 1, "dx", TAP2, (1, 28, 1, 1, 3, 2, 0)),
    "tap2_h16_x28_im1_convT_dx": C(dict(c_in=8, c_out=16, ksize=41, stride=4, pad_l=20, output_padding=1, transposed=True), 2, 75, DX, 1, "dx", TAP2, (1, 28, 1, 1, 4, 2, 0)),
    "tap2_fm1_x28_im0": C(dict(c_in=24, c_out=128, ksize=16, stride=8, pad_l=7, pad_r=7), 2, 301, DX, 0, "dx_ex", TAP2, (1, 28, 0, 0, 3, 2, 0)),
    "tap2_fm1_x28_im1": C(dict(c_in=24, c_out=128, ksize=16, stride=8, pad_l=7, pad_r=7), 2, 301, DX, 1, "dx", TAP2, (1, 28, 0, 1, 3, 2, 0)),
    "tap2_fm1_x28_nx3": C(dict(c_in=24, c_out=128, ksize=3, stride=2, pad_l=1, pad_r=1), 2, 301, DX, 0, "dx_res", TAP2, (1, 28, 0, 0, 3, 3, 0)),
    "tap2_fm2_x16": C(dict(c_in=1024, c_out=128, ksize=16, stride=16, groups=4, pad_l=7, pad_r=7), 1, 97, DX, 0, "dx_ex", TAP2, (2, 16, 0, -1, 1, 1, 0)),
    "tap2_fm2_x28_im0": C(dict(c_in=192, c_out=512, ksize=16, stride=8, groups=4, pad_l=7, pad_r=7), 8, 97, DX, 0, "dx_res", TAP2, (2, 28, 0, 0, 3, 2, 0)),
    "tap2_fm2_x28_im1": C(dict(c_in=192, c_out=512, ksize=16, stride=8, groups=4, pad_l=7, pad_r=7), 8, 97, DX, 1, "dx", TAP2, (2, 28, 0, 1, 3, 2, 0)),
    "tap2_fm3_x16": C(dict(c_in=192, c_out=32, ksize=16, stride=16, pad_l=7, pad_r=7), 8, 97, DX, 1, "dx", TAP2, (3, 16, 0, -1, 1, 1, 0)),
    "tap2_fm3_x28_im0": C(dict(c_in=384, c_out=384, ksize=16, stride=8, groups=4, pad_l=7, pad_r=7), 8, 97, DX, 0, "dx_ex", TAP2, (3, 28, 0, 0, 3, 2, 0)),
    "tap2_fm3_x28_im1": C(dict(c_in=384, c_out=384, ksize=16, stride=8, groups=4, pad_l=7, pad_r=7), 8, 97, DX, 1, "dx", TAP2, (3, 28, 0, 1, 3, 2, 0)),
    "tap2_fm4_x16": C(dict(c_in=2048, c_out=128, ksize=16, stride=16, groups=4, pad_l=7, pad_r=7), 1, 97, DX, 0, "dx_res", TAP2, (4, 16, 0, -1, 1, 1, 0)),
    "tap2_fm4_x28_im0": C(dict(c_in=512, c_out=96, ksize=16, stride=8, pad_l=7, pad_r=7), 8, 97, DX, 0, "dx_ex", TAP2, (4, 28, 0, 0, 3, 2, 0)),
    "tap2_fm4_x28_im1": C(dict(c_in=512, c_out=96, ksize=16, stride=8, pad_l=7, pad_r=7), 8, 97, DX, 1, "dx", TAP2, (4, 28, 0, 1, 3, 2, 0)),
    "tap2_convT_s8": C(dict(c_in=256, c_out=128, ksize=16, stride=8, pad_l=4, transposed=True), 2, 125, FWD, 0, "fwd", TAP2, (1, 28, 0, 0, 5, 2, 0)),
    "tap2_convT_s8_dx": C(dict(c_in=256, c_out=128, ksize=16, stride=8, pad_l=4, transposed=True), 2, 125, DX, 1, "dx", TAP2, (1, 16, 0, -1, 64, 2, 1)),
    "tap2_fm1_x16_dense_k5": C(dict(c_in=256, c_out=384, ksize=5, pad_l=2, pad_r=2), 2, 300, FWD, 0, "fwd", TAP2, (1, 16, 0, -1, 9, 2, 0)),
    "tap1_thin_lds_refusal": C(dict(c_in=128, c_out=8, ksize=2, stride=4), 2, 2003, FWD, 0, "fwd", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_65_phases": C(dict(c_in=4, c_out=8, ksize=130, stride=65), 2, 2003, DX, 0, "dx_ex", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_reflect_res": C(dict(c_in=64, c_out=4, ksize=7, pad_l=3, pad_r=3, reflect=True), 3, 333, FWD, 0, "fwd_res", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_fold": C(dict(c_in=64, c_out=4, ksize=7, pad_l=3, pad_r=3, reflect=True), 3, 333, DX, 1, "dx_res", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_mask_on_load": C(dict(c_in=64, c_out=4, ksize=7, dilation=2, pad_l=6, pad_r=6), 3, 333, DX, 1, "dx", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_logits_m1": C(dict(c_in=96, c_out=1, ksize=3, pad_l=1, pad_r=1, in_slope=1.0), 3, 251, FWD, 0, "fwd", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_convT": C(dict(c_in=64, c_out=4, ksize=16, stride=2, pad_l=7, transposed=True), 2, 131, FWD, 0, "fwd", TAP1, (0, 0, 0, 0, 0, 0, 0)),
    "tap1_convT_dx": C(dict(c_in=4, c_out=64, ksize=16, stride=2, pad_l=7, transposed=True), 2, 131, DX, 1, "dx", TAP1, (0, 0, 0, 0, 0, 0, 0)),
}

# instantiations no default plan can reach, each with the plan rule that excludes it: none (see the docstring)
UNREACHABLE = {}

ALL_THIN = {(mt, bn, np_) for mt in (1, 4, 8, 16) for bn, np_ in ((128, 1), (256, 1), (256, 4))}
ALL_TAP2 = ({(fm, 16, 0, -1) for fm in (1, 2, 3, 4)} | {(fm, 28, 0, im) for fm in (1, 2, 3, 4) for im in (0, 1)}
            | {(1, 16, 1, -1), (1, 28, 1, 0), (1, 28, 1, 1)})
NP4_CASES = [n for n, c in CASES.items() if c.route == THIN and c.expect[2] == 4]
ID_SLOW_CASE, ID_SLOW_SMALL_BATCH = "thin_mt1_bn128_id_slow", 8


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def variant(lib, case, which=None, mask_on_load=None, batch=None):
    out = (ctypes.c_int * 8)()
    d = case.desc(batch=batch)
    rc = lib.eben_conv1d_variant_f32(ctypes.byref(d), case.direction if which is None else which,
                                     case.mask_on_load if mask_on_load is None else mask_on_load, out, 8)
    return rc, tuple(out)


def answer(lib, case, **kw):
    rc, v = variant(lib, case, **kw)
    assert rc == 0, lib.eben_last_error()
    return v


def thin_geometry(case):
    """(rows per group, reduction channels per group, taps per phase, phases, positions per phase) of the launch, from the layer alone."""
    s = case.spec()
    c_in, c_out = (s.c_out, s.c_in) if s.transposed else (s.c_in, s.c_out)   # the canonical conv behind a ConvTranspose1d
    l_in = s.out_len(case.length) if s.transposed else case.length
    tap_dir = 1 - case.direction if s.transposed else case.direction
    if tap_dir == 0:
        return c_out // s.groups, c_in // s.groups, s.ksize, 1, s.out_len(case.length) if not s.transposed else case.length
    import math

    kstep = s.stride // math.gcd(s.stride, s.dilation)
    ly = l_in + (s.pad_l + s.pad_r if s.reflect else 0)
    return c_in // s.groups, c_out // s.groups, -(-s.ksize // kstep), s.stride, -(-ly // s.stride)


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_instantiation(lib, name):
    case = CASES[name]
    assert FORMS[case.form] == case.direction and (not case.mask_on_load or case.form in ("dx", "dx_res")), name
    v = answer(lib, case)
    assert v[0] == case.route, (name, v)
    assert v[1:] == case.expect, (name, v[1:])
    assert v[0] == lib.eben_conv1d_kernel_generation(ctypes.byref(case.desc()), case.direction)
    assert case.elements() <= 21_000_000, (name, case.elements())


def test_table_reaches_every_thin_and_tap2_instantiation(lib):
    thin = {answer(lib, c)[1:4] for c in CASES.values() if c.route == THIN}
    tap2 = {answer(lib, c)[1:5] for c in CASES.values() if c.route == TAP2}
    reached = {("thin",) + v for v in thin} | {("tap2",) + v for v in tap2}
    every = {("thin",) + v for v in ALL_THIN} | {("tap2",) + v for v in ALL_TAP2}
    assert len(ALL_THIN) == 12 and len(ALL_TAP2) == 15
    assert not set(UNREACHABLE) & reached, set(UNREACHABLE) & reached
    assert reached | set(UNREACHABLE) == every, sorted(every - reached - set(UNREACHABLE))
    assert all(reason for reason in UNREACHABLE.values())
    # every launch form on every family, ConvTranspose1d in both passes on every family
    for route in (TAP1, TAP2, THIN):
        mine = [c for c in CASES.values() if c.route == route]
        assert {c.form for c in mine} >= set(FORMS) - ({"dx_fm"} if route != THIN else set()), route
        assert {c.direction for c in mine if c.spec().transposed} == {FWD, DX}, route
        assert any(c.spec().reflect and c.direction == FWD for c in mine) and any(c.spec().reflect and c.direction == DX for c in mine), route


def test_the_fallback_takes_what_both_plans_refuse(lib):
    """TAP1 because the thin kernel's smallest tile needs more than 150 KB of LDS (and 8 rows over a 256-term reduction are not
    tap2's), and because a layer has more than 64 stride phases."""
    lds = CASES["tap1_thin_lds_refusal"]
    mg, cg, j, nph, nt = thin_geometry(lds)
    s = lds.spec()
    assert cg * j <= 256 and mg <= 32 and 4 * cg * s.stride * (128 + (j - 1) // s.stride + 2) > 150 * 1024
    assert answer(lib, lds) == (TAP1,) + (0,) * 7
    # the same layer with half the channels is the thin kernel's, on 128 threads and more than 72 KB
    v = answer(lib, CASES["thin_mt8_bn128_lds"])
    assert v[0] == THIN and v[2] == 128 and 72 * 1024 < v[6] <= 150 * 1024 and thin_geometry(CASES["thin_mt8_bn128_lds"])[4] > 128
    phases = CASES["tap1_65_phases"]
    assert thin_geometry(phases)[3] == 65 and answer(lib, phases) == (TAP1,) + (0,) * 7
    assert sum(c.route == TAP1 for c in CASES.values()) >= 2


def test_rarely_taken_thin_branches_are_in_the_table(lib):
    slow = answer(lib, CASES[ID_SLOW_CASE])
    assert slow[0] == THIN and slow[4] == 0                                       # block id by division
    fast = answer(lib, CASES[ID_SLOW_CASE], batch=ID_SLOW_SMALL_BATCH)
    assert fast[:4] == slow[:4] and fast[4] == 1                                  # ... and the same layer by multiply-high
    pg0 = answer(lib, CASES["thin_mt1_bn256_pg0"])
    assert pg0[0] == THIN and pg0[5] == 0 and pg0[4] == 1 and thin_geometry(CASES["thin_mt1_bn256_pg0"])[3] == 16
    # k < stride on an input gradient: phases that own no tap
    kls = CASES["thin_mt8_bn128_k_lt_stride"]
    assert kls.direction == DX and kls.spec().ksize < kls.spec().stride and answer(lib, kls)[0] == THIN
    # LDS back-off NP 4 -> 1: the launch is large enough for four positions per thread, whose tile would not fit
    back = CASES["thin_mt1_bn256_np_backoff"]
    mg, cg, j, nph, nt = thin_geometry(back)
    assert nt >= 4096 and -(-nt // 1024) * back.batch * nph * back.spec().groups >= 2048
    assert 4 * cg * (1024 + (j - 1) + 2) > 72 * 1024
    v = answer(lib, back)
    assert v[1:4] == (1, 256, 1) and v[6] <= 72 * 1024
    # rows off the row tile, and many row tiles from a tiny reduction
    for name, rows, mt in (("thin_mt8_bn256_mg6_fm", 6, 8), ("thin_np4_mt8", 6, 8), ("thin_mt16_bn256_mg12_dx", 12, 16),
                           ("thin_mt16_bn256_mg768", 768, 16), ("thin_mt16_bn256_tiny_k_mg64", 64, 16)):
        assert thin_geometry(CASES[name])[0] == rows and answer(lib, CASES[name])[1] == mt, name
    # the bit-identity partners of the GPU test: the NP = 4 layers on 2 batch items run NP = 1 of the same MT and BN
    assert len(NP4_CASES) >= 4 and {CASES[n].expect[0] for n in NP4_CASES} == {1, 4, 8, 16}
    assert any(thin_geometry(CASES[n])[3] == 4 for n in NP4_CASES)
    for n in NP4_CASES:
        small = answer(lib, CASES[n], batch=2)
        assert small[:4] == (THIN, CASES[n].expect[0], 256, 1), (n, small)


def test_rarely_taken_tap2_branches_are_in_the_table(lib):
    got = [answer(lib, c) for c in CASES.values() if c.route == TAP2]
    assert any(v[6] == 3 and v[5] > 1 for v in got)                               # three input-tile buffers
    assert any(v[6] == 2 and v[5] > 1 and v[7] == 0 for v in got)                 # two, a tile change mid weight chunk
    assert any(v[6] == 2 and v[5] > 1 and v[7] == 1 for v in got)                 # two, the aligned hand-over
    assert any(v[6] == 1 and v[5] == 1 for v in got)
    # channel chunks that do not divide the channels per group: 24 channels in 5 chunks of 6, 256 in 9 of 30
    assert CASES["tap2_convT_s8"].expect[4] == 5 and CASES["tap2_fm1_x16_dense_k5"].expect[4] == 9
    # the compiled-in mask on load at both tap directions: a Conv1d's input gradient and a ConvTranspose1d's
    im1 = [c for c in CASES.values() if c.route == TAP2 and c.expect[3] == 1]
    assert {c.spec().transposed for c in im1} == {False, True} and all(c.mask_on_load for c in im1)
    assert {c.expect[2] for c in CASES.values() if c.route == TAP2} == {0, 1}     # the H16 PLEN search


def test_query_refuses_what_the_launch_refuses(lib):
    case = CASES["thin_mt4_bn256_mg3"]
    assert variant(lib, case, which=0, mask_on_load=1)[0] == -1      # forwards never mask on load
    assert variant(lib, case, which=2)[0] == -1
    out = (ctypes.c_int * 4)()
    d = case.desc()
    assert lib.eben_conv1d_variant_f32(ctypes.byref(d), 0, 0, out, 4) == -1
    bad = ops.conv_desc(ops.ConvSpec(c_in=6, c_out=8, ksize=3, groups=4), 1, 97)
    full = (ctypes.c_int * 8)()
    assert lib.eben_conv1d_variant_f32(ctypes.byref(bad), 0, 0, full, 8) == -1
    # a grid past 2^31 - 1 blocks: thin_launch refuses it, so does the query
    huge = C(dict(c_in=4, c_out=4, ksize=64, stride=64, groups=4), 1 << 24, 64, DX, 0, "dx_ex", THIN, ())
    assert variant(lib, huge)[0] == -1 and b"grid" in lib.eben_last_error()
    # a layer of the bf16 kernels reports its route and nothing else; a bundle-layout layer without a kernel answers NONE
    spec = ops.ConvSpec(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1)
    bf = ops.conv_desc(spec, 1, 97, ops.MATH_BF16)
    assert lib.eben_conv1d_variant_f32(ctypes.byref(bf), 0, 0, full, 8) == 0 and tuple(full) == (ops.CONV_ROUTE_TAP3,) + (0,) * 7
    none = ops.conv_desc(ops.ConvSpec(c_in=4, c_out=4, ksize=3), 1, 97, ops.MATH_BF16 | 0x100)
    assert lib.eben_conv1d_kernel_generation(ctypes.byref(none), 0) == ops.CONV_ROUTE_NONE
    assert lib.eben_conv1d_variant_f32(ctypes.byref(none), 0, 0, full, 8) == 0 and tuple(full) == (0,) * 8
    # the bf16 query keeps answering zeros past the route for these families
    assert lib.eben_conv1d_variant(ctypes.byref(case.desc()), 0, 0, full, 8) == 0 and tuple(full) == (THIN,) + (0,) * 7
