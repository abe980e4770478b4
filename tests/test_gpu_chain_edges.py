"""GPU: the kernels at the two ends of the bundle-layout discriminator chains (vibravox_amd/csrc/bl_edge.hip) through the C ABI, against
the float64 restatements of tests/chain_edge_oracle.py, at every route and tile edge:

  bl_from_f32 / bl_to_f32          1, 255, 257 positions per row, a second pass of the stride loop past the 8192-block cap, with and without lo
  bl_head_fwd_kernel<4,6,3>        l_in 2 .. 513 at dilation 1 / 2 / 3, one job and three / four jobs per launch (a job's trailing block returns
  bl_head_fwd_kernel<1,16,15>      early), l_in 8 .. 513, two jobs; scale / bias / y_lo NULL; a row slice of a larger plane pair
  bl_head_dx_kernel<4,6,3>         the same lengths, both fold ranges on one element (l_in 3; 8 .. 15), jobs summed (3, 4, 2 on dx2, dilations
  bl_head_dx_kernel<1,16,15>       (1, 2): back on the one-position kernel), gradient planes hi + lo and hi alone (y_lo NULL: the engine's form)
  bl_head_dx2_kernel<16,15>        the 512-position tile and the two-position pair: 9, 511, 512, 513, 1025
  bl_head_dw_kernel<..>            rows x l_out below 32 (empty slices are zeros), 511 / 512 / 513, ragged slices, 33 slices, the 256-slice cap
  bl_tail_fwd_k_kernel<3>          1 .. 49 bundles per row (idle waves, the pair, the third issue, the second pass), lengths 1 .. 129, 768 / 1024
  bl_tail_fwd_kernel               channels; x_lo NULL, k 1 / 2 / 5 / 8, pad != (k - 1) / 2, the 64 KB LDS gate
  bl_tail_dx_kernel                lengths 1 / 255 / 256 / 257, k 1 / 3 / 8, the engine's stacked form (g_lo NULL), the full form, no feature
                                   matching, the identity map, an odd half; planted a == r, a == 0, both, and hi == 0 under lo > 0
  bl_tail_dw_k_kernel<3,4>         rows x l_out 200, 1023 / 1024 / 1025, 4097 (two ragged slices, rows inside a slice), the 32-slice cap, 768
  bl_tail_dw_kernel                channels, 1 / 2 / 3 branches, x_lo NULL, k 5, pad != (k - 1) / 2

Every output lives between sentinel margins that must come back untouched, every input is compared bit for bit with a copy taken before the
launch, every bound is derived in chain_edge_oracle.py (none was widened), every test prints its worst error as a fraction of its bound.

Knob routes: the module is its own child script.  A module-scoped fixture runs the case table `knob_cases` in three fresh processes, each
under `timeout -k 10 30`: a child takes about 3 s on an MI355X (8.7 s for the three, interpreter start and library load included); 15 s
is the fivefold margin, doubled for a first import of torch from a cold page cache.  (1) all knobs unset, (2) EBEN_HEAD_DX2=0
EBEN_TAIL_FWD_K=0 EBEN_TAIL_DW_UN=1, (3) EBEN_HEAD_DW_PAIRS=24 EBEN_HEAD_DW_SLABS=64 EBEN_TAIL_DW_PAIRS=2.  (1) and (2) must give the same
SHA-256 of every output of the MelGAN head's input gradient at dilation 1, the k = 3 tail forward and the k = 3 tail weight gradient ("same
products and sums in the same order"); (3) must report other slab counts and still meet the float64 bounds with the depth of its slice size.

Measured on an MI355X, worst over the cases, as a fraction of the derived bound (none was widened, no derivation had to be corrected):
conversions 0.50 with lo, 0.996 hi alone (the half ulp of the bf16 rounding is the bound and is attained); head forward 0.49 (hi + lo) and
0.99 (y_lo NULL); head input gradient 0.032 (PQMF) / 0.0036 (MelGAN); head weight gradient 0.041 / 0.031; tail forward 0.060; tail input
gradient 0.48 with g_lo, 0.996 in the engine's form (hi alone), no sign mismatch on any element; tail weight gradient 0.033; the knob
children 0.033 / 0.039 / 0.033, (1) and (2) bit-identical on all 21 cases, slab counts (1) -> (3): 33 -> 32, 256 -> 64, 2 -> 8.  The plane outputs
sit at half their bound because the split term 2^-16 |v| (2^-8 |v| for hi alone) dominates it; the fp32 outputs sit far inside theirs because
(n + c) U sum|terms| counts every product as a step of one chain while the kernels sum in trees.
The 64 KB LDS gate (1920 channels x 8 taps = 15360 weights, exactly 65536 bytes of LDS): the launch RUNS, 6.8e-6 of its bound; 1928 channels
are refused by the gate with EBEN_EINVAL.  The gate stays as it is.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from formula import formula_tensor  # noqa: E402

from tests import chain_edge_oracle as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
MARGIN = 64                    # elements of sentinel on each side of an output (128 / 256 bytes: views stay 16-byte aligned)
SENTINEL_F32 = 0x7FC0DEAD      # a quiet NaN with a payload no kernel produces
SENTINEL_BF16 = 0x7FAD         # the same for a bf16 plane
PQMF = dict(c_in=4, c_out=24, k=3, pad=1, rpad=1)
MELGAN = dict(c_in=1, c_out=16, k=15, pad=0, rpad=7)
FAMILY = dict(pqmf=PQMF, melgan=MELGAN)
SLOPE = 0.2


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`n` elements (fp32 or bf16) between two sentinel margins."""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.dtype = n, dtype
        if dtype is torch.float32:
            self.raw, self.pattern = torch.int32, SENTINEL_F32
        else:
            assert dtype is torch.bfloat16
            self.raw, self.pattern = torch.int16, SENTINEL_BF16
        self.full = torch.full((n + 2 * MARGIN,), self.pattern, dtype=self.raw, device=DEV)
        self.view = self.full[MARGIN:MARGIN + n].view(dtype)

    def ptr(self, offset=0):
        return self.view.data_ptr() + offset * self.view.element_size()

    def margins_intact(self):
        return bool((self.full[:MARGIN] == self.pattern).all()) and bool((self.full[MARGIN + self.n:] == self.pattern).all())

    def untouched(self, lo=0, hi=None):
        return bool((self.full[MARGIN + lo:MARGIN + (self.n if hi is None else hi)] == self.pattern).all())

    def all_written(self):
        return not bool((self.full[MARGIN:MARGIN + self.n] == self.pattern).any())


class PlaneOut:
    """Guarded hi (+ lo) planes of a (rows, channels, length) output."""

    def __init__(self, rows, channels, length, lo=True):
        self.rows, self.channels, self.length = rows, channels, length
        self.row_elems = channels * length
        self.hi = Guarded(rows * self.row_elems, torch.bfloat16)
        self.lo = Guarded(rows * self.row_elems, torch.bfloat16) if lo else None

    def planes(self):
        return [p for p in (self.hi, self.lo) if p is not None]

    def f32(self, g):
        return E.from_bundles(g.view.view(self.rows, self.channels // 8, self.length, 8).float())

    def value(self):
        return E.join(self.f32(self.hi), self.f32(self.lo) if self.lo else None)

    def margins_intact(self):
        return all(p.margins_intact() for p in self.planes())

    def untouched(self):
        return all(p.untouched() for p in self.planes())

    def digest(self):
        return [digest(p.view) for p in self.planes()]


class Inputs:
    """Every input of a launch with the copy taken before it."""

    def __init__(self):
        self.kept = []

    def keep(self, t):
        self.kept.append((t, t.clone()))
        return t

    def unchanged(self):
        raw = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
        return all(torch.equal(t.view(raw[t.dtype]), c.view(raw[t.dtype])) for t, c in self.kept)


def digest(t):
    raw = torch.int32 if t.dtype is torch.float32 else torch.int16
    return hashlib.sha256(t.contiguous().view(-1).view(raw).cpu().numpy().tobytes()).hexdigest()


def planes_in(x, inputs, lo=True):
    """bf16 planes (rows, C / 8, L, 8) of an fp32 tensor, made by the oracle's split (not by the library), and their fp32 values."""
    hi, l = E.split(x)
    ph = inputs.keep(E.to_bundles(hi).to(torch.bfloat16))
    pl = inputs.keep(E.to_bundles(l).to(torch.bfloat16)) if lo else None
    return ph, pl, hi, (l if lo else None)


def addr(t):
    return None if t is None else t.data_ptr()


def report(what, **figures):
    print(f"[chain-edges] {what}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


def fraction(got, ref, bound):
    """Worst |got - ref| as a fraction of the absolute bound (inf outside it or for a non-finite value)."""
    return E.bound_violation(got, ref, 1, bound / E.U)


# =====================================================================================================================================
# conversions
# =====================================================================================================================================
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7), 2.0 ** -126, 1.5e-45]


def conversion_input(shape, seed):
    n = shape[0] * shape[1] * shape[2]
    x = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV) * 3.7
    sp = torch.tensor(SPECIALS, device=DEV)
    for start in (0, n // 2, n - len(SPECIALS)):       # +-0, fp32 denormals, exact bf16 ties (both ways), at the start, inside and at the end
        if start >= 0 and n >= len(SPECIALS):
            x[start:start + len(SPECIALS)] = sp
    if n < len(SPECIALS):
        x[:n] = sp[:n]
    return x.view(shape)


@pytest.mark.parametrize("with_lo", [True, False])
@pytest.mark.parametrize("shape", [(1, 8, 1), (3, 24, 255), (2, 16, 257), (1, 264, 63551)])
def test_conversions_bit_for_bit(hip, shape, with_lo):
    """hi = bf16(x) (RNE), lo = bf16(x - hi), fp32(hi + lo) back, bit for bit.  (1, 264, 63551): 2 097 183 units, 31 more than
    8192 x 256: the stride loop's second pass."""
    b, c, l = shape
    units = b * (c // 8) * l
    if b * c * l > 10 ** 7:
        assert units > 8192 * 256
    inputs = Inputs()
    x = inputs.keep(conversion_input(shape, 100 + l))
    out = PlaneOut(b, c, l, lo=with_lo)
    assert hip.eben_bl_from_f32(x.data_ptr(), b, c, l, out.hi.ptr(), out.lo.ptr() if with_lo else None, stream()) == OK
    torch.cuda.synchronize()
    assert out.margins_intact() and inputs.unchanged()
    want_hi = x.to(torch.bfloat16)
    assert torch.equal(out.hi.view.view(torch.int16), E.to_bundles(want_hi).view(-1).view(torch.int16))
    assert torch.equal(want_hi.float().view(torch.int32), E.bf16_rne(x).view(torch.int32))          # torch's rounding is the oracle's
    if with_lo:
        want_lo = (x - want_hi.float()).to(torch.bfloat16)
        assert torch.equal(out.lo.view.view(torch.int16), E.to_bundles(want_lo).view(-1).view(torch.int16))
        assert E.split_violations(out.f32(out.hi), out.f32(out.lo)) == 0
    back = Guarded(b * c * l)
    assert hip.eben_bl_to_f32(out.hi.ptr(), out.lo.ptr() if with_lo else None, b, c, l, back.ptr(), stream()) == OK
    torch.cuda.synchronize()
    assert back.margins_intact() and out.margins_intact()
    want = E.join(out.f32(out.hi), out.f32(out.lo) if with_lo else None)
    assert torch.equal(back.view.view(torch.int32), want.reshape(-1).view(torch.int32))
    err = fraction(back.view.view(shape), x.double(), E.plane_bound(x, 0.0, lo=with_lo))
    report(f"conversions {shape} lo={with_lo}", fraction_of_bound=err)
    assert err <= 1.0


# =====================================================================================================================================
# chain heads
# =====================================================================================================================================
def head_job(h, x, v, scale, bias, y_hi, y_lo, l_in, dil, slope=SLOPE, l_out=None):
    from vibravox_amd._lib import EbenBlHeadJob

    j = EbenBlHeadJob()
    j.x, j.v, j.scale, j.bias, j.y_hi, j.y_lo = x, v, scale, bias, y_hi, y_lo
    j.c_in, j.c_out, j.l_in, j.ksize, j.dilation, j.pad, j.reflect_pad, j.out_slope = h["c_in"], h["c_out"], l_in, h["k"], dil, h["pad"], h["rpad"], slope
    j.l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"]) if l_out is None else l_out
    return j


def job_array(jobs):
    from vibravox_amd._lib import EbenBlHeadJob

    return (EbenBlHeadJob * len(jobs))(*jobs)


def head_weights(h, tag, inputs, scale=True, bias=True):
    v = inputs.keep(formula_tensor(f"ce/{tag}/v", (h["c_out"], 1, h["k"]), 1 / h["k"] ** 0.5).to(DEV))
    s = inputs.keep((1 + 0.3 * formula_tensor(f"ce/{tag}/s", (h["c_out"],))).to(DEV)) if scale else None
    b = inputs.keep(formula_tensor(f"ce/{tag}/b", (h["c_out"],), 0.1).to(DEV)) if bias else None
    return v, s, b


def run_head_fwd(hip, family, dils, l_in, batch, scale=True, bias=True, lo=True, rows_around=0):
    """One launch of len(dils) jobs.  rows_around: the planes have that many more rows on each side of the `batch` rows the launch is given."""
    h = FAMILY[family]
    inputs = Inputs()
    tag = f"hf/{family}/{l_in}/{batch}"
    x_all = inputs.keep(formula_tensor(tag + "/x", (batch + 2 * rows_around, h["c_in"], l_in)).to(DEV))
    x = x_all[rows_around:rows_around + batch]
    made, jobs = [], []
    for i, dil in enumerate(dils):
        v, s, b = head_weights(h, f"{tag}/{i}", inputs, scale, bias)
        l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
        out = PlaneOut(batch + 2 * rows_around, h["c_out"], l_out, lo=lo)
        off = rows_around * out.row_elems
        jobs.append(head_job(h, x.data_ptr(), v.data_ptr(), addr(s), addr(b), out.hi.ptr(off), out.lo.ptr(off) if lo else None, l_in, dil))
        made.append((out, v, s, b, dil))
    assert hip.eben_bl_head_fwd(job_array(jobs), len(jobs), batch, stream()) == OK
    torch.cuda.synchronize()
    assert inputs.unchanged()
    worst, digests = 0.0, []
    for out, v, s, b, dil in made:
        assert out.margins_intact()
        n0, n1 = rows_around * out.row_elems, (rows_around + batch) * out.row_elems
        for p in out.planes():      # the rows outside the slice
            assert p.untouched(0, n0) and p.untouched(n1, None)
            assert not bool((p.full[MARGIN + n0:MARGIN + n1] == p.pattern).any())
        ref, mag = E.head_fwd(x, v, s, b, dil, h["pad"], h["rpad"], SLOPE)
        hi = out.f32(out.hi)[rows_around:rows_around + batch]
        l = out.f32(out.lo)[rows_around:rows_around + batch] if lo else None
        if lo:
            assert E.split_violations(hi, l) == 0
        worst = max(worst, fraction(E.join(hi, l), ref, E.plane_bound(ref, E.head_fwd_k(h["k"]) * E.U * mag, lo=lo)))
        digests += out.digest()
    report(f"head_fwd {family} dil={dils} l_in={l_in} batch={batch} scale={scale} bias={bias} lo={lo} slice={rows_around}", fraction_of_bound=worst)
    return dict(frac=worst, digest=digests)


PQMF_LENGTHS = (2, 3, 254, 255, 256, 257, 513)
MELGAN_LENGTHS = (8, 15, 16, 255, 256, 257, 513)


@pytest.mark.parametrize("l_in", PQMF_LENGTHS)
def test_pqmf_head_forward(hip, l_in):
    """Dilations 1 / 2 / 3 one job at a time and as one three-job launch (l_out = l_in + 2, l_in, l_in - 2: around a block boundary at
    l_in 254 .. 257, so the trailing block of a job returns early); batch 1 and 3.  l_in = 2 has no dilation 3 (l_out = 0)."""
    dils = (1, 2, 3) if l_in > 2 else (1, 2)
    worst = max(run_head_fwd(hip, "pqmf", (d,), l_in, 1 + 2 * (i % 2))["frac"] for i, d in enumerate(dils))
    worst = max(worst, run_head_fwd(hip, "pqmf", dils, l_in, 3)["frac"], run_head_fwd(hip, "pqmf", dils, l_in, 1)["frac"])
    assert worst <= 1.0


@pytest.mark.parametrize("l_in,dil", [(n, 1) for n in MELGAN_LENGTHS] + [(15, 2), (16, 2), (257, 2)])
def test_melgan_head_forward(hip, l_in, dil):
    assert run_head_fwd(hip, "melgan", (dil,), l_in, 1 if l_in % 2 else 3)["frac"] <= 1.0


@pytest.mark.parametrize("family,dils,l_in", [("pqmf", (1, 2, 3, 1), 255), ("pqmf", (3, 2, 1, 2), 257), ("melgan", (1, 2), 257), ("melgan", (1, 1), 16)])
def test_head_forward_job_tables(hip, family, dils, l_in):
    """Four jobs (the table's limit) and the two-job MelGAN launch."""
    assert run_head_fwd(hip, family, dils, l_in, 3)["frac"] <= 1.0


@pytest.mark.parametrize("family", ["pqmf", "melgan"])
@pytest.mark.parametrize("what", ["no_scale", "no_bias", "no_lo", "row_slice"])
def test_head_forward_nullable_operands_and_row_slice(hip, family, what):
    kw = dict(no_scale=dict(scale=False), no_bias=dict(bias=False), no_lo=dict(lo=False), row_slice=dict(rows_around=2))[what]
    dils = (1, 2, 3) if family == "pqmf" else (1,)
    assert run_head_fwd(hip, family, dils, 257, 3, **kw)["frac"] <= 1.0


def run_head_dx(hip, family, dils, l_in, batch, lo=True, scale=True):
    h = FAMILY[family]
    inputs = Inputs()
    tag = f"hx/{family}/{l_in}/{batch}"
    jobs, ojobs = [], []
    for i, dil in enumerate(dils):
        v, s, _ = head_weights(h, f"{tag}/{i}", inputs, scale, False)
        l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
        ph, pl, hi, l = planes_in(formula_tensor(f"{tag}/{i}/g", (batch, h["c_out"], l_out)).to(DEV), inputs, lo)
        jobs.append(head_job(h, None, v.data_ptr(), addr(s), None, ph.data_ptr(), addr(pl), l_in, dil))
        ojobs.append((E.join(hi, l), v, s, dil, h["pad"], h["rpad"]))
    dx = Guarded(batch * h["c_in"] * l_in)
    assert hip.eben_bl_head_dx(job_array(jobs), len(jobs), batch, dx.ptr(), stream()) == OK
    torch.cuda.synchronize()
    assert dx.margins_intact() and dx.all_written() and inputs.unchanged()
    ref, mag = E.head_dx(ojobs, h["c_in"], l_in)
    frac = fraction(dx.view.view(ref.shape), ref, E.head_dx_k(len(dils), h["c_in"], h["c_out"], h["k"]) * E.U * mag)
    report(f"head_dx {family} dil={dils} l_in={l_in} batch={batch} lo={lo} scale={scale}", fraction_of_bound=frac)
    return dict(frac=frac, digest=[digest(dx.view)])


@pytest.mark.parametrize("l_in", PQMF_LENGTHS)
def test_pqmf_head_input_gradient(hip, l_in):
    """l_in = 3: both fold ranges of the reflection fall on element 1.  Gradient planes hi + lo and hi alone (y_lo NULL: the engine's form)."""
    dils = (1, 2, 3) if l_in > 2 else (1, 2)
    worst = max(run_head_dx(hip, "pqmf", (d,), l_in, 1 + 2 * (i % 2), lo=bool(i % 2))["frac"] for i, d in enumerate(dils))
    worst = max(worst, run_head_dx(hip, "pqmf", dils, l_in, 3, lo=False)["frac"], run_head_dx(hip, "pqmf", dils, l_in, 1, lo=True)["frac"])
    assert worst <= 1.0


@pytest.mark.parametrize("l_in,dil", [(n, 1) for n in MELGAN_LENGTHS + (9, 10, 11, 12, 13, 14, 511, 512, 1025)] + [(15, 2), (16, 2), (257, 2)])
def test_melgan_head_input_gradient(hip, l_in, dil):
    """Dilation 1: bl_head_dx2_kernel, two positions per thread, 512 per block -- rows that end inside a pair (odd l_in) and around the
    tile (511, 512, 513, 1025); l_in 8 .. 15: both fold ranges (7 wide) overlap.  Dilation 2: the one-position kernel."""
    worst = max(run_head_dx(hip, "melgan", (dil,), l_in, 3, lo=True)["frac"], run_head_dx(hip, "melgan", (dil,), l_in, 2, lo=False)["frac"])
    assert worst <= 1.0


@pytest.mark.parametrize("family,dils,l_in,lo", [("pqmf", (1, 2, 3, 2), 257, False), ("pqmf", (3, 1, 1, 2), 255, True), ("melgan", (1, 1), 513, False),
                                                 ("melgan", (1, 1), 9, True), ("melgan", (1, 2), 257, False), ("melgan", (2, 1), 16, True)])
def test_head_input_gradient_sums_the_jobs(hip, family, dils, l_in, lo):
    """Four PQMF jobs; two MelGAN jobs at dilation 1 (still two positions per thread); dilations (1, 2) in one launch: the one-position kernel."""
    assert run_head_dx(hip, family, dils, l_in, 3, lo=lo)["frac"] <= 1.0


@pytest.mark.parametrize("family,dils", [("pqmf", (1, 2, 3)), ("melgan", (1,)), ("melgan", (2,))])
def test_head_input_gradient_without_scale(hip, family, dils):
    assert run_head_dx(hip, family, dils, 257, 3, lo=False, scale=False)["frac"] <= 1.0


def run_head_dw(hip, family, dil, batch, l_in):
    h = FAMILY[family]
    inputs = Inputs()
    tag = f"hw/{family}/{dil}/{l_in}/{batch}"
    l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
    x = inputs.keep(formula_tensor(tag + "/x", (batch, h["c_in"], l_in)).to(DEV))
    ph, _, g_hi, _ = planes_in(formula_tensor(tag + "/g", (batch, h["c_out"], l_out)).to(DEV), inputs, lo=False)
    v, _, _ = head_weights(h, tag, inputs, False, False)
    job = head_job(h, x.data_ptr(), v.data_ptr(), None, None, ph.data_ptr(), None, l_in, dil)
    nslab, rs = ctypes.c_int(0), ctypes.c_int(0)
    nbytes = hip.eben_bl_head_dw_workspace(ctypes.byref(job), batch, ctypes.byref(nslab), ctypes.byref(rs))
    ns = nslab.value
    assert rs.value == h["k"] + 1 and nbytes == 4 * ns * h["c_out"] * rs.value and ns >= 32
    slabs = Guarded(nbytes // 4)
    assert hip.eben_bl_head_dw(ctypes.byref(job), batch, slabs.ptr(), nbytes, stream()) == OK
    torch.cuda.synchronize()
    assert slabs.margins_intact() and inputs.unchanged()
    assert slabs.all_written() and bool(torch.isfinite(slabs.view).all())                # every slab of the workspace
    total = batch * l_out
    per = E.slice_size(total, ns)
    s = slabs.view.view(ns, h["c_out"], rs.value)
    empty = [z for z in range(ns) if z * per >= total]
    if empty:
        assert not bool(s[empty[0]:].any())                                             # empty slices are zeros
    ref, mag = E.head_dw(g_hi, x, h["k"], dil, h["pad"], h["rpad"])
    d = E.head_dw_depth(total, ns)
    frac = fraction(s.double().sum(0), ref, d * E.U * mag)
    report(f"head_dw {family} dil={dil} pairs={total}", nslab=ns, per_slice=per, depth=d, fraction_of_bound=frac)
    return dict(frac=frac, digest=[digest(slabs.view)], nslab=ns)


# (family, dilation, batch, l_in): rows x l_out below 32; 511 / 512 / 513; 3 x 1001 = 3003 over 32 slices of 94 (boundaries inside rows);
# 51 000 = 33 slices; 393 300: the 256-slice cap
HEAD_DW = [("pqmf", 1, 1, 9), ("pqmf", 3, 3, 9), ("pqmf", 1, 1, 509), ("pqmf", 1, 1, 510), ("pqmf", 1, 1, 511), ("pqmf", 3, 1, 515), ("pqmf", 3, 3, 1003),
           ("pqmf", 1, 3, 16998), ("pqmf", 3, 3, 17002), ("pqmf", 1, 3, 131098),
           ("melgan", 1, 1, 17), ("melgan", 2, 2, 29), ("melgan", 1, 1, 511), ("melgan", 1, 1, 512), ("melgan", 1, 1, 513), ("melgan", 2, 1, 526),
           ("melgan", 2, 3, 1015), ("melgan", 1, 3, 17000), ("melgan", 2, 3, 17014), ("melgan", 1, 3, 131100)]


@pytest.mark.parametrize("family,dil,batch,l_in", HEAD_DW)
def test_head_weight_gradient(hip, family, dil, batch, l_in):
    r = run_head_dw(hip, family, dil, batch, l_in)
    h = FAMILY[family]
    pairs = batch * E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
    if pairs in (51000,):
        assert r["nslab"] == 33
    if pairs == 393300:
        assert r["nslab"] == 256
    assert r["frac"] <= 1.0


# =====================================================================================================================================
# chain tails
# =====================================================================================================================================
def tail_weights(channels, k, tag, inputs, scale=True, bias=True):
    v = inputs.keep(formula_tensor(f"ce/{tag}/v", (1, channels, k), 1 / (channels * k) ** 0.5).to(DEV))
    s = inputs.keep(torch.tensor([1.3], device=DEV)) if scale else None
    b = inputs.keep(torch.tensor([0.05], device=DEV)) if bias else None
    return v, s, b


def run_tail_fwd(hip, channels, length, k, pad, batch=2, lo=True, scale=True, bias=True, slope=1.0, expect=OK):
    inputs = Inputs()
    tag = f"tf/{channels}/{length}/{k}/{pad}"
    v, s, b = tail_weights(channels, k, tag, inputs, scale, bias)
    ph, pl, hi, l = planes_in(formula_tensor(tag + "/x", (batch, channels, length)).to(DEV), inputs, lo)
    l_out = E.tail_l_out(length, k, pad)
    y = Guarded(batch * l_out)
    rc = hip.eben_bl_tail_fwd(ph.data_ptr(), addr(pl), batch, channels, length, k, pad, v.data_ptr(), addr(s), addr(b), slope, y.ptr(), stream())
    torch.cuda.synchronize()
    assert y.margins_intact() and inputs.unchanged()
    if rc != OK or expect != OK:
        assert rc == expect and y.untouched()
        return dict(rc=rc)
    assert y.all_written()
    ref, mag = E.tail_fwd(E.join(hi, l), v, s, b, pad, slope)
    frac = fraction(y.view.view(ref.shape), ref, E.tail_fwd_k(channels, k) * E.U * mag)
    report(f"tail_fwd C={channels} L={length} k={k} pad={pad} lo={lo} scale={scale} bias={bias} slope={slope}", fraction_of_bound=frac)
    return dict(rc=rc, frac=frac, digest=[digest(y.view)])


@pytest.mark.parametrize("cb", [1, 16, 17, 32, 33, 48, 49, 96, 128])
def test_tail_forward_bundles_per_row(hip, cb):
    """k = 3, both planes, length 65 (a full block of 64 positions and one more): 1 bundle (15 idle waves), 16 (one per wave), 17 (wave 0
    takes the pair), 32, 33 (the third issue), 48, 49 (the second pass of the loop); 96 and 128: the 768- and 1024-channel logits layers."""
    assert run_tail_fwd(hip, 8 * cb, 65, 3, 1)["frac"] <= 1.0


@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 129])
def test_tail_forward_lengths(hip, length):
    assert run_tail_fwd(hip, 8 * 33, length, 3, 1, batch=3)["frac"] <= 1.0


@pytest.mark.parametrize("k,pad", [(3, 1), (3, 0), (3, 2), (1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (8, 0), (8, 4)])
def test_tail_forward_generic_kernel(hip, k, pad):
    """The kernel for any tap count: k = 3 without the lo plane, k = 1 / 2 / 5 / 8 with pad 0 and k / 2 (k even: pad != (k - 1) / 2, l_out != length)."""
    lo = k != 3
    assert run_tail_fwd(hip, 8 * 17, 65, k, pad, lo=lo)["frac"] <= 1.0
    assert run_tail_fwd(hip, 8 * 17, 65, k, pad, lo=True)["frac"] <= 1.0          # k = 3, pad 0 / 2 on the pipelined kernel too


@pytest.mark.parametrize("what", ["no_scale", "no_bias", "out_slope"])
@pytest.mark.parametrize("k", [3, 5])
def test_tail_forward_nullable_operands_and_slope(hip, what, k):
    kw = dict(no_scale=dict(scale=False), no_bias=dict(bias=False), out_slope=dict(slope=0.2))[what]
    assert run_tail_fwd(hip, 8 * 33, 65, k, k // 2, **kw)["frac"] <= 1.0


def test_tail_forward_at_the_lds_gate(hip):
    """channels x ksize = 15360: 4 x (15360 + 1024) bytes = exactly 64 KB of LDS, the gate's limit.  Runs within its bound (module docstring);
    one bundle more is refused before any launch."""
    r = run_tail_fwd(hip, 1920, 65, 8, 4)
    report("tail_fwd at the LDS gate", rc=r["rc"])
    assert r["rc"] == OK and r["frac"] <= 1.0
    assert run_tail_fwd(hip, 1928, 9, 8, 4, expect=EINVAL)["rc"] == EINVAL


def plant_planes(hi, lo, half):
    """Runs on the decision points of the tail's epilogue, in the enhanced rows [0, half) against the reference rows [half, 2 half) of
    (2 half, C, L) plane values: a == r, a == 0, both, and hi == 0 under a positive lo (no split gives it: the mask must follow hi)."""
    n = hi[:half].numel()
    idx = torch.arange(n, device=hi.device).view(hi[:half].shape)
    eq, za, both, hz = idx % 11 == 3, idx % 13 == 5, idx % 17 == 7, idx % 19 == 9
    for p in (hi, lo):
        p[:half][eq] = p[half:][eq]
        p[:half][za] = 0
        p[:half][both] = 0
        p[half:][both] = 0
    hi[:half][hz] = 0
    lo[:half][hz] = 0.125
    return eq | za | both | hz


def run_tail_dx(hip, channels, length, k, pad, half, form):
    """form: engine (four stacked seed blocks, seg = half, map (0, 0, 0, 1), fm_rows = ref_row_offset = half, g_lo NULL), full (the same
    with g_lo), nofm (fm_rows = 0, fm_sums NULL, act_lo NULL), identity (seg = 0: 2 half seed rows on their own embedding rows)."""
    inputs = Inputs()
    tag = f"tx/{channels}/{length}/{k}/{pad}/{half}"
    v, s, _ = tail_weights(channels, k, tag, inputs, True, False)
    hi, lo = E.split(formula_tensor(tag + "/a", (2 * half, channels, length)).to(DEV))
    planted = plant_planes(hi, lo, half)
    ph, pl = inputs.keep(E.to_bundles(hi).to(torch.bfloat16)), inputs.keep(E.to_bundles(lo).to(torch.bfloat16))
    rows = 2 * half if form == "identity" else 4 * half
    seg, seg_map = (0, None) if form == "identity" else (half, (0, 0, 0, 1))
    fm_rows = 0 if form == "nofm" else half
    l_out = E.tail_l_out(length, k, pad)
    seeds = inputs.keep(formula_tensor(tag + "/seed", (rows, l_out), 0.1).to(DEV))
    sums = inputs.keep(torch.tensor([3.5, 11.0], device=DEV))
    fm_gs = 4.0
    out = PlaneOut(rows, channels, length, lo=form != "engine")
    cmap = (ctypes.c_int * 4)(*seg_map) if seg_map else None
    rc = hip.eben_bl_tail_dx(seeds.data_ptr(), rows, channels, length, k, pad, v.data_ptr(), s.data_ptr(), ph.data_ptr(), None if form == "nofm" else pl.data_ptr(),
                             SLOPE, seg, cmap, fm_rows, half if fm_rows else 0, sums.data_ptr() if fm_rows else None, fm_gs, out.hi.ptr(),
                             out.lo.ptr() if out.lo else None, stream())
    assert rc == OK
    torch.cuda.synchronize()
    assert out.margins_intact() and inputs.unchanged() and all(p.all_written() for p in out.planes())
    ref, mag, parts = E.tail_dx(seeds, v, s, pad, hi, lo, SLOPE, seg, seg_map, fm_rows, half, sums, fm_gs, length)
    got = out.value()
    if out.lo:
        assert E.split_violations(out.f32(out.hi), out.f32(out.lo)) == 0
    frac = fraction(got, ref, E.plane_bound(ref, E.tail_dx_k(k) * E.U * mag, lo=bool(out.lo)))
    wrong = 0
    if fm_rows:
        # the feature-matching term decoded where mask and conv part are known: the nearest of the nine values k1 sd - k2 sa, every one of
        # them further from the next than the bound at hand; on ALL elements of the rows, the planted ones among them
        k1, k2 = parts["k1"], parts["k2"]
        values = torch.tensor([k1 * sd - k2 * sa for sd in (-1, 0, 1) for sa in (-1, 0, 1)], dtype=torch.float64, device=DEV)
        term = got[:fm_rows].double() / parts["mask"][:fm_rows] - parts["conv"][:fm_rows]
        code = (term.reshape(-1, 1) - values.reshape(1, -1)).abs().argmin(1)
        want = (3 * (parts["sd"][:fm_rows] + 1) + parts["sa"][:fm_rows] + 1).reshape(-1).long()
        wrong = E.pattern_mismatches(code, want)
        seen = set(torch.unique(want[planted.reshape(-1)]).tolist())
        assert 4 in seen and seen & {3, 5} and seen & {1, 7}, seen          # a == r == 0, a == r, a == 0 are all among the planted
    report(f"tail_dx C={channels} L={length} k={k} pad={pad} half={half} {form}", fraction_of_bound=frac, sign_mismatches=wrong)
    assert wrong == 0
    return dict(frac=frac, digest=out.digest())


@pytest.mark.parametrize("form", ["engine", "full", "nofm", "identity"])
@pytest.mark.parametrize("channels,length,k,pad,half", [(8, 1, 3, 1, 1), (8, 255, 3, 1, 2), (96, 256, 3, 1, 1), (8, 257, 3, 1, 3), (96, 257, 1, 0, 1),
                                                         (8, 256, 8, 4, 2), (96, 255, 8, 3, 3), (8, 257, 3, 2, 1), (96, 1, 1, 0, 3)])
def test_tail_input_gradient(hip, channels, length, k, pad, half, form):
    """Lengths 1 / 255 / 256 / 257 around the 256-position block, 8 and 96 channels, k 1 / 3 / 8, pad != (k - 1) / 2 (k 8 pad 4, k 3 pad 2),
    odd halves (1, 3), in the four forms."""
    assert run_tail_dx(hip, channels, length, k, pad, half, form)["frac"] <= 1.0


def tail_dw_un(k):
    """Pairs per thread and iteration of the kernel the launch takes: bl_tail_dw_k_kernel<3, 4> unless the knob turns it off."""
    return 4 if k == 3 and int(os.environ.get("EBEN_TAIL_DW_UN", "4")) > 1 else 1


def run_tail_dw(hip, channels, length, k, pad, rows, nbranch, lo=True):
    inputs = Inputs()
    tag = f"tw/{channels}/{length}/{k}/{pad}/{rows}/{nbranch}"
    l_out = E.tail_l_out(length, k, pad)
    seeds = inputs.keep(formula_tensor(tag + "/seed", (nbranch * rows, l_out)).to(DEV))
    ph, pl, hi, l = planes_in(formula_tensor(tag + "/x", (nbranch * rows, channels, length)).to(DEV), inputs, lo)
    nslab, rs = ctypes.c_int(0), ctypes.c_int(0)
    nbytes = hip.eben_bl_tail_dw_workspace(rows, channels, l_out, k, nbranch, ctypes.byref(nslab), ctypes.byref(rs))
    ns = nslab.value
    assert rs.value == channels * k + 1 and nbytes == 4 * nbranch * ns * rs.value and 1 <= ns <= 32
    slabs = Guarded(nbytes // 4)
    assert hip.eben_bl_tail_dw(seeds.data_ptr(), ph.data_ptr(), addr(pl), rows, nbranch, channels, length, k, pad, slabs.ptr(), nbytes, stream()) == OK
    torch.cuda.synchronize()
    assert slabs.margins_intact() and inputs.unchanged()
    assert slabs.all_written() and bool(torch.isfinite(slabs.view).all())          # the slab count the query reports is the one the launch uses
    ref, mag = E.tail_dw(seeds, E.join(hi, l), rows, nbranch, k, pad)
    d = E.tail_dw_depth(rows * l_out, ns, tail_dw_un(k))
    frac = fraction(slabs.view.view(nbranch, ns, rs.value).double().sum(1), ref, d * E.U * mag)
    report(f"tail_dw C={channels} L={length} k={k} pad={pad} rows={rows} branches={nbranch} lo={lo}", nslab=ns, depth=d, fraction_of_bound=frac)
    return dict(frac=frac, digest=[digest(slabs.view)], nslab=ns)


# (channels, length, k, pad, rows, branches, lo): rows x l_out 200, 1023, 1024, 1025 (one four-pair iteration of 256 threads); 17 x 241 = 4097:
# two slices of 2049 and 2048; 4 x 16400: the 32-slice cap; 768 channels; k = 5; pad != (k - 1) / 2 (l_out = length + 2, length - 2)
TAIL_DW = [(8, 200, 3, 1, 1, 1, True), (8, 1023, 3, 1, 1, 2, True), (16, 1024, 3, 1, 1, 3, True), (8, 1025, 3, 1, 1, 1, True), (8, 205, 3, 1, 5, 2, True),
           (16, 241, 3, 1, 17, 2, True), (8, 16400, 3, 1, 4, 1, True), (768, 250, 3, 1, 2, 2, True), (16, 241, 3, 1, 17, 1, False),
           (16, 241, 5, 2, 17, 2, True), (8, 1025, 5, 2, 1, 3, False), (8, 239, 3, 2, 17, 2, True), (8, 243, 5, 1, 17, 1, True)]


@pytest.mark.parametrize("channels,length,k,pad,rows,nbranch,lo", TAIL_DW)
def test_tail_weight_gradient(hip, channels, length, k, pad, rows, nbranch, lo):
    r = run_tail_dw(hip, channels, length, k, pad, rows, nbranch, lo)
    pairs = rows * E.tail_l_out(length, k, pad)
    if pairs == 4097:
        assert r["nslab"] == 2
    if pairs == 65600:
        assert r["nslab"] == 32
    assert r["frac"] <= 1.0


# =====================================================================================================================================
# knob routes: the case table in fresh child processes
# =====================================================================================================================================
CHILD_ENVS = [{}, dict(EBEN_HEAD_DX2="0", EBEN_TAIL_FWD_K="0", EBEN_TAIL_DW_UN="1"),
              dict(EBEN_HEAD_DW_PAIRS="24", EBEN_HEAD_DW_SLABS="64", EBEN_TAIL_DW_PAIRS="2")]
KNOBS = ("EBEN_HEAD_DX2", "EBEN_TAIL_FWD_K", "EBEN_TAIL_DW_UN", "EBEN_HEAD_DW_PAIRS", "EBEN_HEAD_DW_SLABS", "EBEN_TAIL_DW_PAIRS")
CHILD_SECONDS = 30
SAME_BITS = ("head_dx/", "tail_fwd/", "tail_dw/")        # what children 1 and 2 must agree on bit for bit
SLAB_COUNTS = ("head_dw/", "tail_dw/")


def knob_cases(hip):
    c = {}
    for l_in in (9, 513, 1025):
        c[f"head_dx/melgan/{l_in}/hi"] = run_head_dx(hip, "melgan", (1,), l_in, 3, lo=False)
        c[f"head_dx/melgan/{l_in}/hi+lo"] = run_head_dx(hip, "melgan", (1,), l_in, 2, lo=True)
    c["head_dx/melgan/2jobs"] = run_head_dx(hip, "melgan", (1, 1), 513, 3, lo=False)
    for cb, length in ((33, 65), (49, 129), (96, 65), (128, 65), (33, 1)):
        c[f"tail_fwd/{cb}/{length}"] = run_tail_fwd(hip, 8 * cb, length, 3, 1)
    for case in TAIL_DW[:9]:
        c["tail_dw/" + "/".join(str(x) for x in case)] = run_tail_dw(hip, *case)
    for family, dil, batch, l_in in (("pqmf", 1, 3, 16998), ("pqmf", 3, 3, 1003), ("pqmf", 1, 3, 131098), ("melgan", 1, 3, 17000), ("melgan", 1, 3, 131100)):
        c[f"head_dw/{family}/{dil}/{batch}/{l_in}"] = run_head_dw(hip, family, dil, batch, l_in)
    return c


def _child(out_path):
    from vibravox_amd import _lib

    res = knob_cases(_lib.load())
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    out = []
    for i, extra in enumerate(CHILD_ENVS):
        path = str(tmp_path_factory.mktemp(f"knobs{i}") / "res.json")
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(extra)
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env,
                           capture_output=True, text=True)
        # a child that ends by signal, time limit or non-zero status fails the fixture here: no further child is started
        assert p.returncode == 0, f"child {i + 1} ({extra}) exited {p.returncode}:\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        with open(path) as f:
            out.append(json.load(f))
    return out


def test_knob_children_meet_the_bounds(children):
    for i, res in enumerate(children):
        worst = max(r["frac"] for r in res.values())
        report(f"knob child {i + 1} {CHILD_ENVS[i]}", cases=len(res), worst_fraction_of_bound=worst)
        assert worst <= 1.0, {k: r["frac"] for k, r in res.items() if r["frac"] > 1.0}


def test_knob_off_routes_are_bit_identical(children):
    """EBEN_HEAD_DX2=0 (one position per thread), EBEN_TAIL_FWD_K=0 (the generic forward), EBEN_TAIL_DW_UN=1 (the generic weight gradient):
    the kernels' comments promise the same products and sums in the same order."""
    base, off = children[0], children[1]
    keys = [k for k in base if k.startswith(SAME_BITS)]
    assert len(keys) >= 20 and set(base) == set(off)
    differ = [k for k in keys if base[k]["digest"] != off[k]["digest"]]
    assert not differ, differ
    for k in base:
        if k.startswith(SLAB_COUNTS):
            assert base[k]["nslab"] == off[k]["nslab"]


def test_slab_knobs_change_the_workspace_queries(children):
    base, other = children[0], children[2]
    counts = {k: (base[k]["nslab"], other[k]["nslab"]) for k in base if k.startswith(SLAB_COUNTS)}
    report("slab counts (default, knobs)", **{k: f"{a}/{b}" for k, (a, b) in counts.items()})
    assert counts["head_dw/pqmf/1/3/16998"] == (33, 32) and counts["head_dw/pqmf/1/3/131098"] == (256, 64) and counts["head_dw/melgan/1/3/131100"] == (256, 64)
    assert counts["tail_dw/16/241/3/1/17/2/True"] == (2, 8) and counts["tail_dw/8/16400/3/1/4/1/True"] == (32, 32)
    assert sum(a != b for a, b in counts.values()) >= 8


# =====================================================================================================================================
# refusals: the documented error before any launch, every output still all sentinel
# =====================================================================================================================================
def test_head_refusals(hip):
    inputs = Inputs()
    h = PQMF
    l_in, batch = 40, 2
    x = inputs.keep(formula_tensor("ce/ref/x", (batch, 4, l_in)).to(DEV))
    v, s, b = head_weights(h, "ref", inputs)
    out = PlaneOut(batch, 24, 64)
    dx = Guarded(batch * 4 * l_in)
    slabs = Guarded(32 * 24 * 16)

    def job(**kw):
        hh = dict(h, **{k: kw.pop(k) for k in list(kw) if k in h})
        j = head_job(hh, x.data_ptr(), v.data_ptr(), s.data_ptr(), b.data_ptr(), out.hi.ptr(), out.lo.ptr(), kw.pop("l_in", l_in), kw.pop("dil", 1), l_out=kw.pop("l_out", None))
        for k, val in kw.items():
            setattr(j, k, val)
        return j

    def all_three(jobs, want):
        arr = job_array(jobs)
        assert hip.eben_bl_head_fwd(arr, len(jobs), batch, stream()) == want
        assert hip.eben_bl_head_dx(arr, len(jobs), batch, dx.ptr(), stream()) == want
        if len(jobs) == 1:
            assert hip.eben_bl_head_dw(arr, batch, slabs.ptr(), 4 * slabs.n, stream()) == want

    all_three([job(c_out=16, k=3)], EUNSUPPORTED)                         # 4 -> 16, k 3: neither built shape
    all_three([job(c_in=1, c_out=16, k=7, l_out=l_in + 2 + 2 - 6)], EUNSUPPORTED)
    all_three([job()] * 5, EINVAL)                                         # five jobs
    all_three([job(), job(l_in=l_in + 1)], EINVAL)                         # jobs with different l_in
    all_three([job(l_out=l_in + 3)], EINVAL)                               # l_out off the geometry
    all_three([job(l_in=1, l_out=3)], EINVAL)                              # reflect_pad >= l_in
    all_three([job(v=None)], EINVAL)
    all_three([job(y_hi=None)], EINVAL)
    assert hip.eben_bl_head_fwd(job_array([job(x=None)]), 1, batch, stream()) == EINVAL
    assert hip.eben_bl_head_dx(job_array([job()]), 1, batch, None, stream()) == EINVAL
    good = job()
    nbytes = hip.eben_bl_head_dw_workspace(ctypes.byref(good), batch, None, None)
    assert 0 < nbytes <= 4 * slabs.n
    assert hip.eben_bl_head_dw(ctypes.byref(good), batch, slabs.ptr(), nbytes - 1, stream()) == EWORKSPACE
    assert hip.eben_bl_head_dw(ctypes.byref(good), batch, None, nbytes, stream()) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched() and dx.untouched() and slabs.untouched() and inputs.unchanged()
    assert out.margins_intact() and dx.margins_intact() and slabs.margins_intact()


def test_tail_refusals(hip):
    inputs = Inputs()
    half, c, length = 2, 16, 20
    v = inputs.keep(formula_tensor("ce/ref/tv", (1, 2048, 8), 0.1).to(DEV))
    ph, pl, _, _ = planes_in(formula_tensor("ce/ref/ta", (2 * half, c, length)).to(DEV), inputs)
    seeds = inputs.keep(formula_tensor("ce/ref/ts", (4 * half, length + 8)).to(DEV))
    sums = inputs.keep(torch.tensor([3.5, 11.0], device=DEV))
    y = Guarded(4 * half * (length + 8))
    g = PlaneOut(4 * half, c, length)
    slabs = Guarded(3 * (c * 8 + 1))
    cmap = (ctypes.c_int * 4)(0, 0, 0, 1)
    st = stream()

    def fwd(channels=c, k=3, pad=1, x=ph, vv=v, out=y):
        return hip.eben_bl_tail_fwd(addr(x), pl.data_ptr(), 2 * half, channels, length, k, pad, addr(vv), None, None, 1.0, None if out is None else out.ptr(), st)

    def dxc(rows=4 * half, channels=c, k=3, pad=1, seg=half, smap=cmap, fm_rows=half, act_lo=pl, fsums=sums, sd=seeds, vv=v, act=ph, gh=g.hi, ln=length):
        return hip.eben_bl_tail_dx(addr(sd), rows, channels, ln, k, pad, addr(vv), None, addr(act), addr(act_lo), SLOPE, seg, smap, fm_rows, half, addr(fsums),
                                   0.37, None if gh is None else gh.ptr(), g.lo.ptr(), st)

    def dwc(channels=c, k=3, pad=1, ws=4 * slabs.n, sd=seeds, x=ph, out=slabs, rows=half, nbranch=2, ln=length):
        return hip.eben_bl_tail_dw(addr(sd), addr(x), pl.data_ptr(), rows, nbranch, channels, ln, k, pad, None if out is None else out.ptr(), ws, st)

    for call in (fwd, dxc, dwc):
        assert call(channels=12) == EINVAL                                  # channels not a multiple of 8
        assert call(k=0) == EINVAL and call(k=9) == EINVAL
        assert call(pad=-1) == EINVAL                                       # (new for the two gradients)
    assert fwd(x=None) == EINVAL and fwd(vv=None) == EINVAL and fwd(out=None) == EINVAL
    assert fwd(channels=2048, k=8) == EINVAL and fwd(channels=1928, k=8) == EINVAL        # channels x ksize past the 64 KB LDS gate
    # l_out <= 0: 3 positions under 8 taps without padding (new for the two gradients; the weight gradient reached an empty grid)
    assert hip.eben_bl_tail_fwd(ph.data_ptr(), pl.data_ptr(), 2 * half, c, 3, 8, 0, v.data_ptr(), None, None, 1.0, y.ptr(), st) == EINVAL
    assert dxc(k=8, pad=0, ln=3) == EINVAL and dwc(k=8, pad=0, ln=3) == EINVAL
    assert dxc(sd=None) == EINVAL and dxc(vv=None) == EINVAL and dxc(act=None) == EINVAL and dxc(gh=None) == EINVAL
    assert dxc(smap=None) == EINVAL                                         # seg > 0 without a map
    assert dxc(rows=4 * half + 1) == EINVAL                                 # rows > 4 seg
    assert dxc(act_lo=None) == EINVAL and dxc(fsums=None) == EINVAL         # feature-matching rows without the lo plane / the sums
    assert dxc(fm_rows=-1) == EINVAL and dxc(seg=-1) == EINVAL
    assert dwc(sd=None) == EINVAL and dwc(x=None) == EINVAL and dwc(out=None) == EINVAL and dwc(rows=0) == EINVAL and dwc(nbranch=0) == EINVAL
    nbytes = hip.eben_bl_tail_dw_workspace(half, c, length, 3, 2, None, None)
    assert 0 < nbytes <= 4 * slabs.n
    assert dwc(ws=nbytes - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert y.untouched() and g.untouched() and slabs.untouched() and inputs.unchanged()
    assert y.margins_intact() and g.margins_intact() and slabs.margins_intact()


def test_fm_sums_refuse_a_missing_lo_plane(hip):
    """eben_bl_fm_sums_codes reads both planes of every pair (the two-unit loop without a test): a NULL lo plane -- in the first pair or in
    pair 33, the second launch's -- is EBEN_EINVAL before ANY launch.  Never tested by launching."""
    inputs = Inputs()
    ph, pl, _, _ = planes_in(formula_tensor("ce/ref/fm", (2, 8, 40)).to(DEV), inputs)
    for npairs, bad in ((1, 0), (34, 33), (34, 0)):
        ptrs = [ph.data_ptr(), pl.data_ptr()] * npairs
        ptrs[2 * bad + 1] = None
        units = (ctypes.c_int64 * npairs)(*[40] * npairs)
        nbytes = hip.eben_bl_fm_sums_workspace(npairs)
        ws, sums, codes = Guarded(nbytes // 4), Guarded(2 * npairs), Guarded(8 * 40, torch.bfloat16)
        cp = (ctypes.c_void_p * npairs)(*[codes.ptr()] * npairs)
        assert hip.eben_bl_fm_sums_codes((ctypes.c_void_p * (2 * npairs))(*ptrs), units, cp, npairs, ws.ptr(), nbytes, sums.ptr(), stream()) == EINVAL
        assert hip.eben_bl_fm_sums((ctypes.c_void_p * (2 * npairs))(*ptrs), units, npairs, ws.ptr(), nbytes, sums.ptr(), stream()) == EINVAL
        ptrs[2 * bad + 1] = pl.data_ptr()
        ptrs[2 * bad] = None
        assert hip.eben_bl_fm_sums((ctypes.c_void_p * (2 * npairs))(*ptrs), units, npairs, ws.ptr(), nbytes, sums.ptr(), stream()) == EINVAL
        torch.cuda.synchronize()
        assert ws.untouched() and sums.untouched() and codes.untouched() and inputs.unchanged()


if __name__ == "__main__":
    _child(sys.argv[1])
