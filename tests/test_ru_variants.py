"""CPU (no GPU): which kernel instantiation every ResidualUnit launch of the case table runs, with which geometry, asked of the library's
own dispatch decision (eben_ru_variant: the resolvers the launchers of exact_fp32/ru_fused.hip, ru_split.hip, ru_bl.hip and ru_dw.hip
dispatch on), and that the table reaches all 57 compute instantiations of the family.  tests/test_gpu_ru_variants.py runs each case
against float64; a retuned plan that moves a case off its instantiation fails here by name.

  ru_fwd_kernel<CT> / ru_bwd_kernel<CT>                 exact fp32, dilation 1..16                                        3 + 3
  ru3_fwd_kernel<CT, NW, NP, KSC, BL>                   NP 1..3 pieces; <4, 2, NP, 1> at 128 channels with EBEN_RU3_W128=2;
                                                        BL (eben_rubl_fwd): NP 2 or 3 at four waves                        12 + 6
  ru3_bwd_kernel<CT, NW, NP, G>                         <4, 2, NP, G> with EBEN_RU3_W128=2                                 12
  rubl_bwd_kernel<CT, NW, G>                            <1, 8, 1> / <2, 8, 2> with EBEN_RUBL_NW32=8 / _NW64=8, <4, 4, 1> with _G128=1      6
  rubl_dw_kernel<CT, RT, BKT>                           <2, 2, 64> with EBEN_RUBL_RT64=2, <4, 2, 32> with _RT128=2, <4, 1, 32> with _BKT128=32   6
  ru_dw_kernel<CT, NP, UN>                              <CT, 1, 1> with EBEN_RUDW_UNROLL=1                                 9

The knobs are read once per process, so a case with knobs is asked in a child process that has them set: one child per knob set
(KNOBS: three sets).  The lengths come from the geometry a case expects (and the query must report): with T the positions per block
and d the dilation, d + 1, 2 d, 2 d + 1 (both reflections inside the first columns; for L <= 2 d the two folds of the input gradient
land on the same columns), T - 1, T, T + 1, 2 T + 1, 2 T + d (the right fold reads the tile before the last), and a multiple of 4 long
enough for an interior tile (the float4 staging), aligned and one float off; for the weight gradients the slab length S takes T's
place, plus a clip shorter than one k-step.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, BF16X3, BF16X6 = 0, 1, 3, 4                      # EBEN_MATH_*
FWD, BL_FWD, BWD, BL_BWD, DW, BL_DW = range(6)              # EBEN_RU_OP_*
FAM_F32, FAM_SPLIT, FAM_BL_BWD, FAM_RU_DW, FAM_RUBL_DW = 1, 2, 3, 4, 5   # EBEN_RU_FAMILY_*
OP_NAME = {FWD: "fwd", BL_FWD: "blfwd", BWD: "bwd", BL_BWD: "blbwd", DW: "dw", BL_DW: "bldw"}
N_OUT = 13                                                  # EBEN_RU_VARIANT_N

# one child process per knob set; "C" apart because EBEN_RUBL_RT128=2 overrides EBEN_RUBL_BKT128
KNOBS = {
    "": {},
    "A": {"EBEN_RU3_W128": "2", "EBEN_RUDW_UNROLL": "1", "EBEN_RUDW_SEG": "64"},
    "B": {"EBEN_RUBL_NW32": "8", "EBEN_RUBL_NW64": "8", "EBEN_RUBL_G128": "1", "EBEN_RUBL_RT64": "2", "EBEN_RUBL_RT128": "2",
          "EBEN_RUBL_SEG32": "128", "EBEN_RUBL_SEG64": "64", "EBEN_RUBL_SEG128": "64"},
    "C": {"EBEN_RUBL_BKT128": "32", "EBEN_RUBL_SEG128": "128"},
}


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


class Inst:
    """One instantiation as the sources name it: entry point (op, math, channels, knob set) -> kernel family, template arguments
    (0 past the last), window width W (positions per block T = W - 2 d for the input gradients, W for the forwards; 0 for the weight
    gradients, whose T is the slab length) and the dynamic LDS bytes (None: depends on the dilation, see expected_lds)."""

    def __init__(self, op, math, channels, knobs, family, targs, width, lds):
        self.op, self.math, self.channels, self.knobs, self.family = op, math, channels, knobs, family
        self.targs, self.width, self.lds = tuple(targs) + (0,) * (5 - len(targs)), width, lds

    @property
    def key(self):
        return (self.family, 1 if self.op in (BWD, BL_BWD) else 0) + self.targs

    def tile(self, d):
        return self.width - 2 * d if self.op in (BWD, BL_BWD) else self.width


def _split_fwd_lds(ct, nw, np_, ksc):
    return 2 * ksc * np_ * ct * 64 * 16 + 4 * 32 * ct * (nw * 32 + 24)


def _split_bwd_lds(ct, nw, np_, g):
    return 2 * g * 2 * np_ * ct * 64 * 16 + 4 * 32 * ct * (nw * 32 + 4)


NP_OF = {BF16: 1, BF16X3: 2, BF16X6: 3}
BWD_G = {(1, 1): 1, (2, 1): 2, (4, 1): 2, (1, 2): 1, (2, 2): 2, (4, 2): 1, (1, 3): 1, (2, 3): 1, (4, 3): 1}   # (CT, NP) -> G, ru3_bwd

INSTS = []
for _c in (32, 64, 128):
    _ct = _c // 32
    INSTS.append(Inst(FWD, F32, _c, "", FAM_F32, (_ct,), 128, None))
    INSTS.append(Inst(BWD, F32, _c, "", FAM_F32, (_ct,), 128, 4 * (2048 * _ct + 32 * _ct * 132)))
    for _m in (BF16, BF16X3, BF16X6):
        _np = NP_OF[_m]
        INSTS.append(Inst(FWD, _m, _c, "", FAM_SPLIT, (_ct, 4, _np, 2, 0), 128, _split_fwd_lds(_ct, 4, _np, 2)))
        INSTS.append(Inst(BWD, _m, _c, "", FAM_SPLIT, (_ct, 4, _np, BWD_G[(_ct, _np)]), 128, _split_bwd_lds(_ct, 4, _np, BWD_G[(_ct, _np)])))
        if _m != BF16:
            INSTS.append(Inst(BL_FWD, _m, _c, "", FAM_SPLIT, (_ct, 4, _np, 2, 1), 128, _split_fwd_lds(_ct, 4, _np, 2)))
        if _c == 128:
            INSTS.append(Inst(FWD, _m, _c, "A", FAM_SPLIT, (4, 2, _np, 1, 0), 64, _split_fwd_lds(4, 2, _np, 1)))
            INSTS.append(Inst(BWD, _m, _c, "A", FAM_SPLIT, (4, 2, _np, BWD_G[(4, _np)]), 64, _split_bwd_lds(4, 2, _np, BWD_G[(4, _np)])))
    INSTS.append(Inst(DW, BF16, _c, "", FAM_RU_DW, (_ct, 1, 2), 0, 0))
    INSTS.append(Inst(DW, BF16X6, _c, "", FAM_RU_DW, (_ct, 3, 1), 0, 0))
    INSTS.append(Inst(DW, BF16, _c, "A", FAM_RU_DW, (_ct, 1, 1), 0, 0))
INSTS += [
    Inst(BL_BWD, 0, 32, "", FAM_BL_BWD, (1, 4, 1), 128, 12288), Inst(BL_BWD, 0, 64, "", FAM_BL_BWD, (2, 4, 2), 128, 32768),
    Inst(BL_BWD, 0, 128, "", FAM_BL_BWD, (4, 4, 2), 128, 65536),
    Inst(BL_BWD, 0, 32, "B", FAM_BL_BWD, (1, 8, 1), 256, 4096 + 4 * 256 * 16), Inst(BL_BWD, 0, 64, "B", FAM_BL_BWD, (2, 8, 2), 256, 16384 + 8 * 256 * 16),
    Inst(BL_BWD, 0, 128, "B", FAM_BL_BWD, (4, 4, 1), 128, 16384 + 16 * 128 * 16),
    Inst(BL_DW, 0, 32, "", FAM_RUBL_DW, (1, 1, 64), 0, 43008), Inst(BL_DW, 0, 64, "", FAM_RUBL_DW, (2, 1, 64), 0, 68608),
    Inst(BL_DW, 0, 128, "", FAM_RUBL_DW, (4, 1, 64), 0, 119808),
    Inst(BL_DW, 0, 64, "B", FAM_RUBL_DW, (2, 2, 64), 0, 32 * (16 * 68 + 8 * 68 + 8 * 132)), Inst(BL_DW, 0, 128, "B", FAM_RUBL_DW, (4, 2, 32), 0, 32 * (16 * 36 + 16 * 36 + 16 * 68)),
    Inst(BL_DW, 0, 128, "C", FAM_RUBL_DW, (4, 1, 32), 0, 32 * (8 * 36 + 16 * 36 + 16 * 68)),
    # a default instantiation under a slab-length knob of its own (EBEN_RUBL_SEG32)
    Inst(BL_DW, 0, 32, "B", FAM_RUBL_DW, (1, 1, 64), 0, 43008),
]

# the full set, written out from the sources: (family, 1 for an input-gradient kernel, template arguments) -- 6 + 18 + 12 + 6 + 6 + 9
ALL_RU = (
    {(FAM_F32, dx, ct, 0, 0, 0, 0) for dx in (0, 1) for ct in (1, 2, 4)}
    | {(FAM_SPLIT, 0, ct, 4, np_, 2, 0) for ct in (1, 2, 4) for np_ in (1, 2, 3)} | {(FAM_SPLIT, 0, 4, 2, np_, 1, 0) for np_ in (1, 2, 3)}
    | {(FAM_SPLIT, 0, ct, 4, np_, 2, 1) for ct in (1, 2, 4) for np_ in (2, 3)}
    | {(FAM_SPLIT, 1, 1, 4, 1, 1, 0), (FAM_SPLIT, 1, 2, 4, 1, 2, 0), (FAM_SPLIT, 1, 4, 4, 1, 2, 0), (FAM_SPLIT, 1, 4, 2, 1, 2, 0),
       (FAM_SPLIT, 1, 1, 4, 2, 1, 0), (FAM_SPLIT, 1, 2, 4, 2, 2, 0), (FAM_SPLIT, 1, 4, 4, 2, 1, 0), (FAM_SPLIT, 1, 4, 2, 2, 1, 0),
       (FAM_SPLIT, 1, 1, 4, 3, 1, 0), (FAM_SPLIT, 1, 2, 4, 3, 1, 0), (FAM_SPLIT, 1, 4, 4, 3, 1, 0), (FAM_SPLIT, 1, 4, 2, 3, 1, 0)}
    | {(FAM_BL_BWD, 1, 1, 4, 1, 0, 0), (FAM_BL_BWD, 1, 1, 8, 1, 0, 0), (FAM_BL_BWD, 1, 2, 4, 2, 0, 0), (FAM_BL_BWD, 1, 2, 8, 2, 0, 0),
       (FAM_BL_BWD, 1, 4, 4, 2, 0, 0), (FAM_BL_BWD, 1, 4, 4, 1, 0, 0)}
    | {(FAM_RUBL_DW, 0, 1, 1, 64, 0, 0), (FAM_RUBL_DW, 0, 2, 1, 64, 0, 0), (FAM_RUBL_DW, 0, 2, 2, 64, 0, 0), (FAM_RUBL_DW, 0, 4, 1, 64, 0, 0),
       (FAM_RUBL_DW, 0, 4, 1, 32, 0, 0), (FAM_RUBL_DW, 0, 4, 2, 32, 0, 0)}
    | {(FAM_RU_DW, 0, ct, np_, un, 0, 0) for ct in (1, 2, 4) for (np_, un) in ((1, 2), (1, 1), (3, 1))}
)
assert len(ALL_RU) == 57

# instantiations removed because a test found them wrong beyond a small repair, each with the reason: none
UNREACHABLE = {}


def slab_target(inst):
    """The slab-length target of a weight-gradient launch: the default (ru_dw.hip rdw_seg, ru_bl.hip rubl_seg) or the knob's."""
    env = KNOBS[inst.knobs]
    if inst.op == DW:
        return int(env.get("EBEN_RUDW_SEG", 512))
    return int(env.get(f"EBEN_RUBL_SEG{inst.channels}", 1024 if inst.channels == 32 else 512))


def slab_geometry(inst, length):
    """(slab length, slabs per item): the items are cut into equal slabs no longer than the target, rounded up to whole k-steps
    (16 positions, ru_dw_kernel) / whole chunks (64, rubl_dw_kernel)."""
    unit = 16 if inst.op == DW else 64
    target = max(slab_target(inst), 2 * unit if inst.op == DW else unit)
    seg = round_up(ceil_div(length, ceil_div(length, target)), unit)
    return seg, ceil_div(length, seg)


def expected_lds(inst, d):
    if inst.lds is not None:
        return inst.lds
    ct = inst.channels // 32   # ru_fwd_kernel: the staged rows hold 128 + 2 d positions and the alignment shift
    return 4 * (2048 * ct + 32 * ct * round_up(128 + 2 * d + 3, 4))


class Case:
    """One launch: instantiation, batch, length, dilation, LeakyReLU slope on the input, `post` addend of the input gradient, offset of
    every fp32 operand from a 16-byte boundary in floats.  `expect`: what eben_ru_variant must report."""

    def __init__(self, inst, batch, length, dilation, slope, post, offset):
        self.inst, self.batch, self.length, self.dilation, self.slope, self.post, self.offset = inst, batch, length, dilation, slope, post, offset
        self.op, self.math, self.channels, self.knobs, self.env = inst.op, inst.math, inst.channels, inst.knobs, KNOBS[inst.knobs]
        ct = self.channels // 32
        if self.op in (DW, BL_DW):
            seg, nseg = slab_geometry(inst, length)
            blocks = batch * nseg * (ct if self.op == DW else ct // inst.targs[1])
            geom = (seg, nseg, blocks, expected_lds(inst, dilation), seg, nseg, batch * nseg)
        else:
            t = inst.tile(dilation)
            geom = (t, ceil_div(length, t), batch * ceil_div(length, t), expected_lds(inst, dilation), 0, 0, 0)
        self.expect = (inst.family,) + inst.targs + geom

    @property
    def name(self):
        return (f"{OP_NAME[self.op]}_m{self.math}_c{self.channels}{'_k' + self.knobs if self.knobs else ''}_d{self.dilation}_L{self.length}"
                f"_b{self.batch}{'_s' if self.slope != 1.0 else ''}{'_p' if self.post else ''}{'_o' if self.offset else ''}")

    def args(self):
        return (self.op, self.math, self.batch, self.channels, self.length, self.dilation)


# (batch, slope, post, offset) dealt over an instantiation's lengths: every value of each with every instantiation
VARY = [(1, 1.0, False, 0), (3, 0.01, True, 1), (1, 0.01, False, 1), (3, 1.0, True, 0), (1, 1.0, True, 1), (3, 0.01, False, 0),
        (1, 0.01, True, 0), (3, 1.0, False, 1)]


def _build():
    cases = {}

    def add(inst, batch, length, d, slope, post, offset):
        c = Case(inst, batch, length, d, slope, post, offset)
        cases.setdefault(c.name, c)

    for inst in INSTS:
        if inst.op in (DW, BL_DW):
            d, s = 9, slab_target(inst)
            lengths = [d + 1, 2 * d, 2 * d + 1, 15, s - 1, s, s + 1]
            if s <= 128:   # the small slabs of the knob cases: several slabs per item, the last ones short
                lengths += [2 * s + 1, 2 * s + d]
            for i, length in enumerate(lengths):
                add(inst, *((VARY[i % 8][0], length, d) + VARY[i % 8][1:]))
            for i, (dd, length) in enumerate([(1, 2), (1, 3), (3, 4), (3, 6), (3, 7)]):
                add(inst, *((VARY[(i + 3) % 8][0], length, dd) + VARY[(i + 3) % 8][1:]))
            continue
        d = 9
        t = inst.tile(d)
        lengths = [d + 1, 2 * d, 2 * d + 1, t - 1, t, t + 1, 2 * t + 1, 2 * t + d]
        for i, length in enumerate(lengths):
            add(inst, *((VARY[i][0], length, d) + VARY[i][1:]))
        l4 = round_up(2 * t + 2 * d + 40, 4)   # tile 1 is interior: float4 staging when the operands are aligned, scalar when not
        add(inst, 3, l4, d, 0.01, True, 0)
        add(inst, 1, l4, d, 1.0, False, 1)
        for i, (dd, length) in enumerate([(1, 2), (1, 3), (3, 4), (3, 6), (3, 7)]):
            add(inst, *((VARY[(i + 3) % 8][0], length, dd) + VARY[(i + 3) % 8][1:]))
    # every dilation of each entry point at 32 channels, at lengths d + 1 and T + 1
    sweep = {(FWD, F32): 16, (BWD, F32): 16, (FWD, BF16X3): 9, (BL_FWD, BF16X3): 9, (BWD, BF16): 9, (BL_BWD, 0): 9, (DW, BF16): 9, (BL_DW, 0): 9}
    for inst in INSTS:
        if inst.channels != 32 or inst.knobs or (inst.op, inst.math) not in sweep:
            continue
        for d in range(1, sweep[(inst.op, inst.math)] + 1):
            t = slab_target(inst) if inst.op in (DW, BL_DW) else inst.tile(d)
            add(inst, 1 + 2 * (d % 2), d + 1, d, 1.0 if d % 2 else 0.01, bool(d & 2), d % 2)
            add(inst, 3 - 2 * (d % 2), t + 1, d, 0.01 if d % 2 else 1.0, not (d & 2), 1 - d % 2)
    return cases


CASES = _build()


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def variant(lib, op, math, batch, channels, length, dilation, n=N_OUT):
    out = (ctypes.c_int * max(n, 1))()
    rc = lib.eben_ru_variant(op, math, batch, channels, length, dilation, out, n)
    return rc, tuple(out)


def slabs_call(lib, case):
    return (lib.eben_ru_dw_slabs if case.op == DW else lib.eben_rubl_dw_slabs)(case.batch, case.channels, case.length)


_CHILD = ("import sys, json, ctypes; sys.path.insert(0, %r)\n"
          "from vibravox_amd import _lib\n"
          "lib = _lib.load(); res = {}\n"
          "for name, a, dw in json.load(sys.stdin):\n"
          "    out = (ctypes.c_int * %d)()\n"
          "    rc = lib.eben_ru_variant(*a, out, %d)\n"
          "    slabs = (lib.eben_ru_dw_slabs if dw == 1 else lib.eben_rubl_dw_slabs)(a[2], a[3], a[4]) if dw else 0\n"
          "    res[name] = [rc, list(out), slabs]\n"
          "json.dump(res, sys.stdout)\n" % (ROOT, N_OUT, N_OUT))
_child_cache = {}


def ask(lib, case):
    """(rc, eben_ru_variant's tuple, the _slabs call) of a case -- in a child process with the case's knobs where it has any (one child
    per knob set, asked once for all its cases)."""
    if not case.knobs:
        rc, v = variant(lib, *case.args())
        return rc, v, slabs_call(lib, case) if case.op in (DW, BL_DW) else 0
    if case.knobs not in _child_cache:
        todo = [(n, c.args(), {DW: 1, BL_DW: 2}.get(c.op, 0)) for n, c in CASES.items() if c.knobs == case.knobs]
        r = subprocess.run([sys.executable, "-c", _CHILD], input=json.dumps(todo), capture_output=True, text=True, timeout=300,
                           env={**os.environ, **case.env})
        assert r.returncode == 0, r.stderr[-2000:]
        _child_cache[case.knobs] = json.loads(r.stdout)
    rc, v, slabs = _child_cache[case.knobs][case.name]
    return rc, tuple(v), slabs


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_ru_instantiation(lib, name):
    case = CASES[name]
    rc, v, slabs = ask(lib, case)
    assert rc == 0, (name, rc)
    assert v[:6] == case.expect[:6], f"{name}: runs family {v[0]} <{v[1:6]}>, the case is written for family {case.expect[0]} <{case.expect[1:6]}>"
    assert v == case.expect, (name, v, case.expect)
    if case.op in (DW, BL_DW):
        assert v[12] == slabs and v[12] == case.batch * v[11] and v[10] * v[11] >= case.length > v[10] * (v[11] - 1), (name, v, slabs)
    else:
        assert v[6] * v[7] >= case.length > v[6] * (v[7] - 1) and v[8] == case.batch * v[7], (name, v)


def test_table_reaches_every_ru_instantiation(lib):
    reached = set()
    for case in CASES.values():
        rc, v, _ = ask(lib, case)
        assert rc == 0, case.name
        reached.add((v[0], 1 if case.op in (BWD, BL_BWD) else 0) + v[1:6])
    assert not set(UNREACHABLE) & reached, set(UNREACHABLE) & reached
    assert reached | set(UNREACHABLE) == ALL_RU, sorted(ALL_RU ^ (reached | set(UNREACHABLE)))
    assert all(reason for reason in UNREACHABLE.values())
    assert {i.key for i in INSTS} == ALL_RU - set(UNREACHABLE)


def test_table_covers_the_edges_it_promises():
    """Per instantiation: a multiple of 4 and a non-multiple, batch 1 and 3, both slopes, with and without post, both offsets; every
    dilation of each entry point at 32 channels at lengths d + 1 and T + 1."""
    by_inst = {}
    for c in CASES.values():
        by_inst.setdefault((c.inst.key, c.knobs, c.channels, c.math), []).append(c)
    for key, cs in by_inst.items():
        assert {c.length % 4 == 0 for c in cs} == {True, False}, key
        assert {c.batch for c in cs} >= {1, 3} and {c.slope for c in cs} == {1.0, 0.01}, key
        assert {c.post for c in cs} == {True, False} and {c.offset for c in cs} == {0, 1}, key
        assert any(c.length <= 2 * c.dilation for c in cs) and any(c.length < 16 for c in cs), key
    for op, top in ((FWD, 16), (BWD, 16), (BL_FWD, 9), (BL_BWD, 9), (DW, 9), (BL_DW, 9)):
        for d in range(1, top + 1):
            ls = {c.length for c in CASES.values() if c.op == op and c.channels == 32 and c.dilation == d and not c.knobs}
            assert d + 1 in ls and len(ls) >= 2, (op, d, ls)
    for op in (FWD, BWD):   # the split kernels' own range
        assert {c.dilation for c in CASES.values() if c.op == op and c.math != F32 and c.channels == 32} >= set(range(1, 10))
    # every slab-length knob changes the geometry of at least one case
    for knob in ("EBEN_RUDW_SEG", "EBEN_RUBL_SEG32", "EBEN_RUBL_SEG64", "EBEN_RUBL_SEG128"):
        assert any(knob in c.env and c.op in (DW, BL_DW) and (knob != "EBEN_RUDW_SEG" or c.op == DW)
                   and (c.op == DW or knob.endswith(str(c.channels))) and c.expect[11] >= 2 for c in CASES.values()), knob
    assert max(c.batch * c.channels * c.length for c in CASES.values()) <= 3 * 128 * 1100


def test_default_plan_of_the_existing_tests_shapes(lib):
    """With no knob set the query names today's instantiations for the shapes of the ResidualUnit tests in tests/test_gpu_ops.py."""
    for c, d, length, b in ((32, 1, 1000, 3), (32, 9, 8000, 2), (64, 9, 300, 3), (64, 1, 4000, 2), (128, 3, 1000, 2), (128, 9, 131, 2),
                            (32, 9, 20, 1), (128, 9, 999, 32), (64, 9, 3996, 2)):
        ct = c // 32
        for m in (F32, BF16, BF16X3, BF16X6):
            fam = FAM_F32 if m == F32 else FAM_SPLIT
            rc, v = variant(lib, FWD, m, b, c, length, d)
            assert rc == 0 and v[:9] == (fam,) + ((ct, 0, 0, 0, 0) if m == F32 else (ct, 4, NP_OF[m], 2, 0)) + (128, ceil_div(length, 128), b * ceil_div(length, 128))
            rc, v = variant(lib, BWD, m, b, c, length, d)
            bo = 128 - 2 * d
            assert rc == 0 and v[:9] == (fam,) + ((ct, 0, 0, 0, 0) if m == F32 else (ct, 4, NP_OF[m], BWD_G[(ct, NP_OF[m])], 0)) + (bo, ceil_div(length, bo), b * ceil_div(length, bo))
        rc, v = variant(lib, BL_FWD, BF16X6, b, c, length, d)
        assert rc == 0 and v[:7] == (FAM_SPLIT, ct, 4, 3, 2, 1, 128)
        rc, v = variant(lib, BL_BWD, 0, b, c, length, d)
        assert rc == 0 and v[:7] == (FAM_BL_BWD, ct, 4, 1 if ct == 1 else 2, 0, 0, 128 - 2 * d)
        rc, v = variant(lib, DW, BF16, b, c, length, d)
        assert rc == 0 and v[:4] == (FAM_RU_DW, ct, 1, 2) and v[12] == lib.eben_ru_dw_slabs(b, c, length)
        rc, v = variant(lib, DW, BF16X6, b, c, length, d)
        assert rc == 0 and v[:4] == (FAM_RU_DW, ct, 3, 1)
        rc, v = variant(lib, BL_DW, 0, b, c, length, d)
        assert rc == 0 and v[:4] == (FAM_RUBL_DW, ct, 1, 64) and v[12] == lib.eben_rubl_dw_slabs(b, c, length)
    # spot values of the slab geometry: 513 positions are two slabs of 272 (17 k-steps); 1025 at 32 channels two of 576 (9 chunks)
    assert variant(lib, DW, BF16, 2, 64, 513, 3)[1][10:] == (272, 2, 4)
    assert variant(lib, BL_DW, 0, 3, 32, 1025, 3)[1][10:] == (576, 2, 6)
    assert variant(lib, BL_DW, 0, 3, 128, 1025, 3)[1][10:] == (384, 3, 9)


def test_variant_query_refuses_what_the_launch_refuses(lib):
    EINVAL, EUNSUPPORTED = -1, -3

    def launch_rc(op, math, b, c, length, d):
        """The launch itself with null pointers: a shape it accepts fails on the pointers (EINVAL) after the geometry passed, so only the
        refusals are compared."""
        if op == FWD:
            return lib.eben_ru_fwd_ex(math, b, c, length, d, None, 1.0, 0.01, None, None, None, None, None)
        if op == BL_FWD:
            return lib.eben_rubl_fwd(math, b, c, length, d, None, 1.0, 0.01, None, None, None, None, None, None)
        if op == BWD:
            return lib.eben_ru_bwd_ex(math, b, c, length, d, None, None, 0.01, None, 1.0, None, None, None, None, None)
        if op == BL_BWD:
            return lib.eben_rubl_bwd(b, c, length, d, None, None, 0.01, None, 1.0, None, None, None, None, None, None)
        if op == DW:
            return lib.eben_ru_dw(math, b, c, length, d, None, None, 0.01, None, None, None, 1.0, None, None, None)
        return lib.eben_rubl_dw(b, c, length, d, None, None, None, None, None, None, None)

    refused = [
        (FWD, BF16X6, 1, 48, 100, 1), (FWD, F32, 1, 48, 100, 1), (BL_FWD, BF16X6, 1, 96, 100, 1), (BWD, BF16, 1, 16, 100, 1), (BL_BWD, 0, 1, 48, 100, 1),
        (DW, BF16, 1, 48, 100, 1), (BL_DW, 0, 1, 256, 100, 1),                                      # channel count
        (FWD, BF16X6, 1, 64, 100, 10), (FWD, BF16X6, 1, 64, 100, 0), (FWD, F32, 1, 64, 100, 17), (BWD, F32, 1, 64, 100, 0), (BL_FWD, BF16X3, 1, 64, 100, 10),
        (BWD, BF16X3, 1, 64, 100, 10), (BL_BWD, 0, 1, 64, 100, 10), (BL_DW, 0, 1, 64, 100, 10), (DW, BF16, 1, 64, 100, 0),   # dilation
        (FWD, BF16X6, 1, 64, 9, 9), (FWD, F32, 1, 64, 16, 16), (BL_FWD, BF16X6, 1, 64, 3, 3), (BWD, BF16, 1, 64, 5, 9), (BL_BWD, 0, 1, 64, 9, 9),
        (DW, BF16X6, 1, 64, 9, 9), (BL_DW, 0, 1, 64, 1, 1), (FWD, BF16, 0, 64, 100, 1),              # length <= dilation, no items
        (FWD, 7, 1, 64, 100, 3), (FWD, 2, 1, 64, 100, 3), (BWD, 7, 1, 64, 100, 3), (DW, BF16X3, 1, 64, 100, 3), (DW, F32, 1, 64, 100, 3),   # math
    ]
    for a in refused:
        rc, _ = variant(lib, *a)
        assert rc == EINVAL and rc == launch_rc(*a), (a, rc, launch_rc(*a))
    # the forward that saves bundle planes computes in two or three pieces
    a = (BL_FWD, BF16, 1, 64, 100, 3)
    assert variant(lib, *a)[0] == EUNSUPPORTED == launch_rc(*a)
    assert variant(lib, BL_FWD, F32, 1, 64, 100, 3)[0] == EINVAL == launch_rc(BL_FWD, F32, 1, 64, 100, 3)
    # the fp32 kernels take dilations the split kernels do not
    assert variant(lib, FWD, F32, 1, 64, 100, 12)[0] == 0 and variant(lib, BWD, F32, 1, 64, 100, 16)[0] == 0
    # a short or null out, an unknown op
    ok = (FWD, BF16, 1, 64, 100, 3)
    assert variant(lib, *ok, n=N_OUT - 1)[0] == EINVAL
    assert lib.eben_ru_variant(*ok, None, N_OUT) == EINVAL
    assert variant(lib, 6, BF16, 1, 64, 100, 3)[0] == EINVAL and variant(lib, -1, BF16, 1, 64, 100, 3)[0] == EINVAL
    assert variant(lib, *ok)[0] == 0
