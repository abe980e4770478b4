"""GPU: every kernel route of eben_fir_decimate / eben_fir_interp_sum (direct.hip fir_plan: 1 the shuffle polyphase kernels, 2 fir1_kernel,
3 the whole-bank-in-LDS kernels, 4 the tap-tiled MFMA kernels of fir_bank.hip) at its tile edges, against the float64 reference of
tests/fir_oracle.py: one small case per edge through the raw entry points into fenced, NaN-filled, 16-byte-misaligned buffers; the banks
whose two directions take different kernels through autograd; PseudoQMFBanks(8, 64) and the default bank cut to 2 bands at module
level; the shuffle kernels bit for bit against the LDS form they replace.

Bounds: relative L2 error < 1e-5 (TOL of test_gpu_pqmf_banks.py) and max|got - ref| / max|ref| < 1e-5 (the FIR bound of
test_gpu_ops.py) -- the second because an L2 norm over a few thousand elements hides one wrong column.  Measured on an MI355X:
at most 1.7e-6 and 2.6e-6 (the 64 x 4096 bank at stride 1, interpolating: 4096-term fp32 sums)."""
import ctypes
import functools
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from tests import fir_oracle
from formula import formula_tensor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
FENCE = 64           # sentinel floats on each side of a payload
SENTINEL = -12345.678


def plan(lib, bands, ntaps, stride, which):
    out = (ctypes.c_int * 4)()
    assert lib.eben_fir_plan(bands, ntaps, stride, which, out, 4) == 0
    return list(out)


def errors(got, ref):
    """(relative L2, max-abs over max|ref|) of a finite result."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).norm() / (ref.norm() + 1e-300)), float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def reference(bands, ntaps, stride, off0, batch, lx, ly):
    """Inputs and float64 references of one case, computed once: A x by the strided convolution, A^T s by the transposed one."""
    tag = f"firroute/{bands}/{ntaps}/{stride}/{off0}/{batch}/{lx}/{ly}"
    x = formula_tensor(tag + "/x", (batch, 1, lx))
    w = formula_tensor(tag + "/w", (bands, ntaps), 1.0 / math.sqrt(ntaps))
    s = formula_tensor(tag + "/s", (batch, bands, ly))
    return x, w, s, fir_oracle.decimate(x.double(), w.double(), ly, stride, off0), fir_oracle.interp_sum(s.double(), w.double(), lx, stride, off0)


class Fenced:
    """A payload of n floats inside a larger allocation: NaN-filled, FENCE sentinel floats on either side, 65 floats (an odd number) past
    the allocation's start -- 4-byte but not 16-byte aligned."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((1 + FENCE + n + FENCE,), SENTINEL, dtype=torch.float32, device=DEV)
        self.payload = self.buf[1 + FENCE:1 + FENCE + n]
        self.wipe()
        assert self.payload.data_ptr() % 16 != 0 and self.payload.data_ptr() % 4 == 0

    def wipe(self):
        self.payload.fill_(float("nan"))

    def fences_untouched(self):
        want = torch.full((1 + FENCE,), SENTINEL, dtype=torch.float32).view(torch.int32)
        lo, hi = self.buf[:1 + FENCE].cpu().view(torch.int32), self.buf[1 + FENCE + self.n:].cpu().view(torch.int32)
        return torch.equal(lo, want) and torch.equal(hi, want[:FENCE])


def launch_fenced(launch, shape, ref, what):
    """Runs launch(payload) twice into a fenced buffer; returns the two error figures of the first result."""
    fb = Fenced(ref.numel())
    launch(fb.payload)
    torch.cuda.synchronize()
    assert fb.fences_untouched(), f"{what}: a store outside the output"
    first = fb.payload.clone()
    assert torch.isfinite(first).all(), f"{what}: {int((~torch.isfinite(first)).sum())} positions never written"
    l2, mx = errors(first.reshape(shape), ref)
    fb.wipe()
    launch(fb.payload)
    torch.cuda.synchronize()
    assert fb.fences_untouched(), f"{what}: a store outside the output (second launch)"
    assert torch.equal(fb.payload.view(torch.int32), first.view(torch.int32)), f"{what}: a second launch gives other bits"
    return l2, mx


# (bands, ntaps, stride, off0, batch, lx, ly), kernel decimating, kernel interpolating, band groups of an interpolating kernel 4
CASES = [
    # ---- kernel 4: the tap-tiled MFMA kernels
    ((40, 100, 7, -50, 2, 1500, 230), 4, 4, 1),      # row tile 1 holds 8 bands; odd stride; M = 15 odd; ntaps % stride = 2; chunk 2 ragged
    ((16, 2048, 2, -1000, 2, 700, 400), 4, 4, 2),    # band groups of 10 + 6: hand-over and a partial last group; 32 chunks per group
    ((64, 4096, 1, 0, 1, 300, 300), 4, 4, 32),       # 32 groups of 2; stride 1: one live row in the interpolating tile; off0 = 0
    ((64, 17, 3, 5, 2, 900, 310), 4, 4, 1),          # positive off0; fewer taps than one chunk; outputs past the input's end
    ((3, 1090, 44, -7, 2, 6000, 140), 4, 4, 1),      # interpolating row tile 1 holds 12 phases; M = 25 (Mp = 26); ntaps % stride = 34; off0 % stride != 0
    ((33, 64, 64, -63, 2, 4096, 65), 4, 4, 1),       # decimating row tile 1 holds ONE band; M = 1 (Mp = 2: half of every step padded); stride 64
    ((64, 4096, 64, -4095, 1, 3000, 111), 4, 4, 1),  # more than 64 KB of LDS in both directions (82 KB / 66 KB)
    ((5, 300, 9, -150, 2, 1, 1), 4, 4, 1),           # one input sample, one output frame
    ((5, 300, 9, 40, 2, 2000, 129), 4, 4, 1),        # positive off0; one column in a second block (P + 1)
    # ---- kernel 3: the whole-bank-in-LDS kernels
    ((8, 64, 8, -63, 2, 1000, 133), 3, 3, None),     # the PQMF 8 x 64 bank
    ((3, 32, 4, -31, 2, 500, 132), 3, 3, None),      # 3 bands: the PQMF shape the shuffle kernels decline
    ((1, 3, 1, -1, 2, 300, 300), 3, 3, None),        # fewer taps than fir1_kernel takes
    ((1, 1024, 32, -1023, 2, 4000, 157), 3, 3, None),  # one band of the default bank (per-band "synthesis") and its adjoint
    ((64, 16, 60, 3, 1, 5000, 90), 3, 3, None),      # the largest decimating tile: 65 360 B of dynamic LDS
    ((64, 16, 61, 3, 1, 5000, 90), 4, 3, None),      # one stride further: the two directions split
    ((64, 16, 1, -8, 2, 600, 600), 3, 4, 1),         # the split the other way round
    ((56, 16, 1, -8, 2, 600, 600), 3, 3, None),      # the largest interpolating tile: 65 248 B
    # ---- kernel 1: the shuffle polyphase kernels
    ((4, 32, 4, -31, 2, 1001, 258), 1, 1, None),     # lx % 4 != 0: the scalar tail of the quad loads
    ((2, 32, 4, 0, 2, 230, 57), 1, 1, None),         # exactly one wave's 57 outputs; off0 = 0
    ((2, 32, 4, 0, 2, 230, 58), 1, 1, None),         # ... and one more
    ((1, 32, 4, 2, 2, 64, 9), 1, 1, None),           # positive off0; a clip shorter than the windows span
    ((4, 32, 4, -31, 2, 912, 228), 1, 1, None),      # one block's 4 x 57 outputs
    ((4, 32, 4, -31, 2, 912, 229), 1, 1, None),      # ... and one more
    # ---- kernel 2: fir1_kernel
    ((1, 101, 1, 0, 2, 1500, 1400), 2, 2, None),     # ly != lx; off0 = 0
    ((1, 5, 1, -4, 2, 1025, 1025), 2, 2, None),      # one output past FIR1_BLOCK; ntaps % 4 = 1
    ((1, 5, 1, -4, 2, 1024, 1024), 2, 2, None),      # FIR1_BLOCK exactly
    ((1, 4, 1, 3, 2, 37, 37), 2, 2, None),           # the smallest tap count; positive off0
]
SPLIT = [c for c in CASES if c[1] != c[2]]


@pytest.mark.parametrize("shape,k_dec,k_int,groups", CASES, ids=["-".join(map(str, c[0])) for c in CASES])
def test_raw_entry_points_route_fences_and_float64(hip, shape, k_dec, k_int, groups):
    from vibravox_amd._lib import check, ptr, stream

    bands, ntaps, stride, off0, batch, lx, ly = shape
    p_dec, p_int = plan(hip, bands, ntaps, stride, 0), plan(hip, bands, ntaps, stride, 1)
    got_groups = -(-bands // p_int[3]) if p_int[0] == 4 else None
    print(shape, "route", p_dec[0], "/", p_int[0], "groups", got_groups)
    assert (p_dec[0], p_int[0]) == (k_dec, k_int) and got_groups == groups
    x, w, s, y_ref, xt_ref = reference(*shape)
    xd, wd, sd = x.to(DEV), w.to(DEV), s.to(DEV)
    dec = launch_fenced(lambda out: check(hip.eben_fir_decimate(ptr(xd), ptr(wd), ptr(out), batch, lx, ly, bands, ntaps, stride, off0, stream()),
                                          "fir_decimate"), (batch, bands, ly), y_ref, "decimate")
    itp = launch_fenced(lambda out: check(hip.eben_fir_interp_sum(ptr(sd), ptr(wd), ptr(out), batch, lx, ly, bands, ntaps, stride, off0, stream()),
                                          "fir_interp_sum"), (batch, 1, lx), xt_ref, "interp_sum")
    print(shape, "decimate l2 %.3g max %.3g" % dec, "interp_sum l2 %.3g max %.3g" % itp)
    assert max(dec + itp) < TOL, (dec, itp)


# ---- autograd: the backward of one direction is the other direction's kernel ---------------------------------------------------------
AUTOGRAD = SPLIT + [c for c in CASES if c[0] in ((64, 16, 60, 3, 1, 5000, 90), (16, 2048, 2, -1000, 2, 700, 400))]


@pytest.mark.parametrize("shape,k_dec,k_int,groups", AUTOGRAD, ids=["-".join(map(str, c[0])) for c in AUTOGRAD])
def test_autograd_picks_up_the_other_directions_kernel(hip, shape, k_dec, k_int, groups):
    """A x, grad <A x, s>, A^T s, grad <A^T s, x> where the plan sends the two directions of one bank to different kernels (4 / 3 and
    3 / 4), the bank one stride short of the split, and the bank of two band groups."""
    from vibravox_amd import ops

    assert len(SPLIT) == 2 and {(c[1], c[2]) for c in SPLIT} == {(4, 3), (3, 4)}
    bands, ntaps, stride, off0, batch, lx, ly = shape
    assert (plan(hip, bands, ntaps, stride, 0)[0], plan(hip, bands, ntaps, stride, 1)[0]) == (k_dec, k_int)
    x, w, s, y_ref, xt_ref = reference(*shape)
    wd = w.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.fir_decimate(xd, wd, ly, stride, off0)
    (y * s.to(DEV)).sum().backward()
    sd = s.to(DEV).requires_grad_(True)
    xt = ops.fir_interp_sum(sd, wd, lx, stride, off0)
    (xt * x.to(DEV)).sum().backward()
    errs = {"A x": errors(y, y_ref), "grad <A x, s>": errors(xd.grad, xt_ref), "A^T s": errors(xt, xt_ref), "grad <A^T s, x>": errors(sd.grad, y_ref)}
    print(shape, errs)
    assert max(max(e) for e in errs.values()) < TOL, errs


# ---- module level ------------------------------------------------------------------------------------------------------------------------
def float64_bank(pq, x64):
    """analysis, per-band synthesis of the float32-rounded analysis, and the round trip of PseudoQMFBanks in float64 convolutions of the
    module's own weights (pqmf.py:194-213)."""
    m, n = pq.decimation, pq.kernel_size
    aw, sw = pq.analysis_weights.detach().double().cpu(), pq.synthesis_weights.detach().double().cpu()
    syn = lambda a: F.conv_transpose1d(a, sw, stride=m, output_padding=m - 2, groups=m, padding=n - 1)   # noqa: E731
    ana = F.conv1d(x64, aw, stride=m, padding=n - 1)
    return ana, syn(ana.detach().float().double()), syn(ana).sum(1, keepdim=True)


@pytest.fixture(scope="module")
def bank_8x64():
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    return PseudoQMFBanks(8, 64).to(DEV)


@pytest.mark.parametrize("raw_length", [1000, 1213])
def test_bank_8x64_on_the_generic_kernels(hip, bank_8x64, raw_length):
    """PseudoQMFBanks(8, 64) routes to kernel 3 in both directions, per band too: analysis, synthesis_sum, per-band "synthesis" and the
    gradient of the round trip; a clip with (lx + 64) % 8 == 0 as it is, and one brought there by cut_tensor."""
    pq = bank_8x64
    assert [plan(hip, 8, 64, 8, 0)[0], plan(hip, 8, 64, 8, 1)[0], plan(hip, 1, 64, 8, 1)[0]] == [3, 3, 3]
    x = pq.cut_tensor(formula_tensor(f"pqmf8x64/{raw_length}/x", (2, 1, raw_length)))
    lx = x.shape[2]
    assert (lx + 64) % 8 == 0 and lx == {1000: 1000, 1213: 1208}[raw_length]
    s = formula_tensor(f"pqmf8x64/{raw_length}/s", (2, 1, lx))
    x64 = x.double().requires_grad_(True)
    ana64, per_band64, rec64 = float64_bank(pq, x64)
    (rec64 * s.double()).sum().backward()
    ana_in = ana64.detach().float().to(DEV)
    with torch.no_grad():
        total = pq.synthesis_sum(ana_in)
        per_band = pq(ana_in, "synthesis")
    xd = x.to(DEV).requires_grad_(True)
    ana = pq(xd, "analysis")
    rec = pq.synthesis_sum(ana)
    (rec * s.to(DEV)).sum().backward()
    assert ana.shape == (2, 8, (lx + 64) // 8) and per_band.shape == (2, 8, lx) and total.shape == rec.shape == (2, 1, lx)
    errs = {"analysis": errors(ana, ana64), "synthesis_sum": errors(total, per_band64.sum(1, keepdim=True)), "synthesis": errors(per_band, per_band64),
            "roundtrip": errors(rec, rec64), "gradient": errors(xd.grad, x64.grad)}
    print(raw_length, errs)
    assert max(max(e) for e in errs.values()) < TOL, errs


def test_default_bank_restricted_to_two_bands(hip):
    """PseudoQMFBanks()(x, "analysis", bands=2): kernel 4 with 2 of a row tile's 32 rows."""
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    pq = PseudoQMFBanks().to(DEV)
    assert plan(hip, 2, 1024, 32, 0)[0] == 4
    x = formula_tensor("pqmf32x1024/two_bands/x", (2, 1, 1500))
    with torch.no_grad():
        got = pq(x.to(DEV), "analysis", bands=2)
    ly = (1500 + 1022) // 32 + 1
    assert got.shape == (2, 2, ly)
    ref = fir_oracle.decimate(x.double(), pq.analysis_weights[:2, 0].detach().double().cpu(), ly, 32, -1023)
    errs = errors(got, ref)
    print("two bands of the default bank", errs)
    assert max(errs) < TOL, errs


# ---- the shuffle kernels against the LDS form ------------------------------------------------------------------------------------------
def shuffle_case(bands, lx=1001):
    """Inputs of the bit-identity test (the child process calls this too): the PQMF geometry of EBEN at a length with lx % 4 != 0."""
    ly = (lx + 30) // 4 + 1
    return (formula_tensor(f"shuffle/{bands}/x", (2, 1, lx)), formula_tensor(f"shuffle/{bands}/w", (bands, 32), 1.0 / math.sqrt(32)),
            formula_tensor(f"shuffle/{bands}/s", (2, bands, ly)), ly)


def shuffle_results(lib):
    from vibravox_amd import ops

    out = {}
    for bands in (1, 2, 4):
        x, w, s, ly = shuffle_case(bands)
        route = (plan(lib, bands, 32, 4, 0)[0], plan(lib, bands, 32, 4, 1)[0])
        out[bands] = (route, ops._fir_decimate(x.to(DEV), w.to(DEV), ly, bands, 32, 4, -31).cpu(),
                      ops._fir_interp_sum(s.to(DEV), w.to(DEV), x.shape[2], bands, 32, 4, -31).cpu())
    return out


def test_shuffle_kernels_are_bit_identical_to_the_lds_form(hip):
    """pqmf_analysis_kernel / pqmf_synthesis_kernel <1 | 2 | 4> (kernel 1) against fir_decimate_kernel / fir_interp_sum_kernel (kernel 3,
    EBEN_PQMF_SHUFFLE=0 in a second process, once for the three band counts): the same products in the same order, bit for bit."""
    code = ("import sys, torch; sys.path[:0] = [%r, %r]\n"
            "from tests import test_gpu_fir_routes as t\n"
            "from vibravox_amd import _lib\n"
            "torch.save(t.shuffle_results(_lib.load()), sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests", "golden")))
    mine = shuffle_results(hip)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "lds_form.pt")
        subprocess.run([sys.executable, "-c", code, path], check=True, env={**os.environ, "EBEN_PQMF_SHUFFLE": "0"}, timeout=300)
        theirs = torch.load(path)
    for bands in (1, 2, 4):
        (route, ana, syn), (route_lds, ana_lds, syn_lds) = mine[bands], theirs[bands]
        assert route == (1, 1) and route_lds == (3, 3), (bands, route, route_lds)
        assert torch.isfinite(ana).all() and torch.isfinite(syn).all()
        assert torch.equal(ana.view(torch.int32), ana_lds.view(torch.int32)), f"analysis, {bands} bands"
        assert torch.equal(syn.view(torch.int32), syn_lds.view(torch.int32)), f"synthesis_sum, {bands} bands"
