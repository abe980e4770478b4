"""GPU: FIR banks beyond the 1024 weights of the whole-bank-in-LDS kernels (csrc/fir_bank.hip) -- the raw entry points against float64
F.conv1d and its float64 autograd adjoint computed on the CPU here, PseudoQMFBanks() at its class defaults and EBENGenerator(4, 512, 2)
against outputs frozen from the reference (tests/golden/make_pqmf_banks_golden.py).

Bound: relative L2 error < 1e-5, the bound of test_gpu_ops.py::test_pqmf_analysis_synthesis; the reference's own fp32 convolution sits
at <= 4e-7 of float64 on these banks."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from formula import formula_audio, formula_state_dict, formula_tensor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


@pytest.fixture(scope="module")
def banks_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pqmf_banks_golden.npz"))


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def ref_decimate(x, w, ly, stride, off0):
    """float64 y[b,k,t] = sum_j w[k,j] x[b,0,t stride + off0 + j], zero outside the input (off0 <= 0)."""
    assert off0 <= 0
    lx, ntaps = x.shape[2], w.shape[1]
    right = max(0, (ly - 1) * stride + ntaps - (lx - off0))
    return F.conv1d(F.pad(x, (-off0, right)), w[:, None, :], stride=stride)[..., :ly]


@functools.lru_cache(maxsize=None)
def reference(bands, ntaps, stride, off0, batch, lx, ly):
    """Inputs and float64 references of one case, computed once: A x, and A^T s by float64 autograd."""
    tag = f"firbank/{bands}/{ntaps}/{stride}/{off0}/{batch}/{lx}/{ly}"
    x = formula_tensor(tag + "/x", (batch, 1, lx))
    w = formula_tensor(tag + "/w", (bands, ntaps), 1.0 / np.sqrt(ntaps))
    s = formula_tensor(tag + "/s", (batch, bands, ly))
    x64 = x.double().requires_grad_(True)
    y = ref_decimate(x64, w.double(), ly, stride, off0)
    (y * s.double()).sum().backward()
    return x, w, s, y.detach(), x64.grad.detach()


def check_case(bands, ntaps, stride, off0, batch, lx, ly):
    from vibravox_amd import ops

    x, w, s, y_ref, xt_ref = reference(bands, ntaps, stride, off0, batch, lx, ly)
    wd = w.to(DEV)
    # decimating bank and its autograd adjoint <A x, s>
    xd = x.to(DEV).requires_grad_(True)
    y = ops.fir_decimate(xd, wd, ly, stride, off0)
    (y * s.to(DEV)).sum().backward()
    # the band-summed interpolating bank on the same bank (for the PQMF-shaped cases lx = M L - N) and ITS autograd adjoint
    sd = s.to(DEV).requires_grad_(True)
    xt = ops.fir_interp_sum(sd, wd, lx, stride, off0)
    (xt * x.to(DEV)).sum().backward()
    errs = {"A x": rel_l2(y, y_ref), "grad <A x, s>": rel_l2(xd.grad, xt_ref), "A^T s": rel_l2(xt, xt_ref), "grad <A^T s, x>": rel_l2(sd.grad, y_ref)}
    print((bands, ntaps, stride, off0, batch, lx, ly), errs)
    assert max(errs.values()) < TOL, errs
    # fixed accumulation order: a second run is bitwise the same
    with torch.no_grad():
        assert torch.equal(ops.fir_decimate(x.to(DEV), wd, ly, stride, off0), y)
        assert torch.equal(ops.fir_interp_sum(s.to(DEV), wd, lx, stride, off0), xt)


def pqmf_frames(lx, ntaps, stride):
    return (lx + ntaps - 2) // stride + 1


CASES = [
    (32, 1024, 32, -1023, 2, 7328, None),   # the class default bank
    (5, 1024, 32, -1023, 1, 7328, None),    # a band count that fills no band block
    (16, 256, 16, -255, 3, 2128, None),
    (4, 512, 4, -511, 2, 3220, None),
    (64, 1024, 64, -1023, 1, 8512, None),
    (3, 700, 5, -123, 2, 4001, 900),        # outputs run past the end of the input; nothing PQMF-shaped
    (1, 4096, 1, -2048, 1, 5000, 5000),
]


@pytest.mark.parametrize("bands,ntaps,stride,off0,batch,lx,ly", CASES)
def test_fir_bank_entry_points_against_float64(hip, bands, ntaps, stride, off0, batch, lx, ly):
    out = (ctypes.c_int * 4)()
    for which in (0, 1):
        assert hip.eben_fir_plan(bands, ntaps, stride, which, out, 4) == 0 and out[0] == 4   # the new kernels, not the old ones
    check_case(bands, ntaps, stride, off0, batch, lx, pqmf_frames(lx, ntaps, stride) if ly is None else ly)


@pytest.mark.parametrize("frames", ["1", "P", "P+1"])
def test_default_bank_at_the_block_edges(hip, frames):
    """ly = 1, one block of output positions exactly, one position more; lx = M L - N (17 samples for the single frame)."""
    out = (ctypes.c_int * 4)()
    assert hip.eben_fir_plan(32, 1024, 32, 0, out, 4) == 0 and out[0] == 4
    p = out[1]
    ly = {"1": 1, "P": p, "P+1": p + 1}[frames]
    check_case(32, 1024, 32, -1023, 2, 17 if ly == 1 else 32 * ly - 1024, ly)


def test_domain_is_enforced_before_the_launch(hip):
    from vibravox_amd import _lib, ops

    x = torch.zeros(1, 1, 4096, device=DEV)
    for bands, ntaps, stride in ((65, 32, 4), (2, 4097, 4), (2, 2048, 65)):
        with pytest.raises(_lib.EbenError, match="outside"):
            ops.fir_decimate(x, torch.zeros(bands, ntaps, device=DEV), 16, stride, 0)
        with pytest.raises(_lib.EbenError, match="outside"):
            ops.fir_interp_sum(torch.zeros(1, bands, 16, device=DEV), torch.zeros(bands, ntaps, device=DEV), 4096, stride, 0)
    torch.cuda.synchronize()


# ---- module level: PseudoQMFBanks() with its default arguments -------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_bank(banks_golden):
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    pq = PseudoQMFBanks()
    assert (pq.decimation, pq.kernel_size) == (32, 1024)
    assert float(np.abs(pq.analysis_weights.numpy() - banks_golden["bank32x1024/analysis"]).max()) <= 1e-7
    return pq.to(DEV)


def test_default_bank_matches_the_reference_outputs(hip, banks_golden, default_bank):
    pq = default_bank
    x = formula_tensor("pqmf_in/32x1024", (2, 1, 7328))
    ana_ref = torch.from_numpy(banks_golden["out32x1024/analysis"])
    with torch.no_grad():
        ana = pq(x.to(DEV), "analysis")
        total = pq.synthesis_sum(ana_ref.to(DEV))
        per_band = pq(ana_ref.to(DEV), "synthesis")
    assert per_band.shape == (2, 32, 7328) and total.shape == (2, 1, 7328)
    errs = {"analysis": rel_l2(ana, ana_ref),
            "synthesis_sum": rel_l2(total[..., ::3], torch.from_numpy(banks_golden["out32x1024/synthesis_sum:every3"])),
            "synthesis": rel_l2(per_band[..., ::97], torch.from_numpy(banks_golden["out32x1024/synthesis:every97"]))}
    print(errs)
    assert max(errs.values()) < TOL, errs


def test_bank_16x256_matches_the_reference_outputs(hip, banks_golden):
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    pq = PseudoQMFBanks(16, 256).to(DEV)
    x = formula_tensor("pqmf_in/16x256", (3, 1, 2128))
    ana_ref = torch.from_numpy(banks_golden["out16x256/analysis"])
    with torch.no_grad():
        ana = pq(x.to(DEV), "analysis")
        total = pq.synthesis_sum(ana_ref.to(DEV))
        per_band = pq(ana_ref.to(DEV), "synthesis")
    errs = {"analysis": rel_l2(ana, ana_ref),
            "synthesis_sum": rel_l2(total[..., ::3], torch.from_numpy(banks_golden["out16x256/synthesis_sum:every3"])),
            "synthesis": rel_l2(per_band[..., ::29], torch.from_numpy(banks_golden["out16x256/synthesis:every29"]))}
    print(errs)
    assert max(errs.values()) < TOL, errs


def float64_roundtrip(pq, x64):
    m, n = pq.decimation, pq.kernel_size
    ana = F.conv1d(x64, pq.analysis_weights.detach().double().cpu(), stride=m, padding=n - 1)
    return F.conv_transpose1d(ana, pq.synthesis_weights.detach().double().cpu(), stride=m, output_padding=m - 2, groups=m,
                              padding=n - 1).sum(1, keepdim=True)


def snr_db(x, rec):
    x, rec = x.detach().double().cpu(), rec.detach().double().cpu()
    return float(10 * torch.log10((rec ** 2).mean() / ((x - rec) ** 2).mean()))


def test_default_bank_roundtrip_gradient_and_snr(hip, default_bank):
    pq = default_bank
    x = torch.rand(2, 1, 7328, generator=torch.Generator().manual_seed(3))
    s = formula_tensor("pqmf32/roundtrip_seed", (2, 1, 7328))
    x64 = x.double().requires_grad_(True)
    rec64 = float64_roundtrip(pq, x64)
    (rec64 * s.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    rec = pq.synthesis_sum(pq(xd, "analysis"))
    (rec * s.to(DEV)).sum().backward()
    errs = {"roundtrip": rel_l2(rec, rec64), "gradient": rel_l2(xd.grad, x64.grad)}
    snr, snr64 = snr_db(x, rec), snr_db(x, rec64)
    print(errs, "snr", snr, "float64", snr64)
    assert max(errs.values()) < TOL, errs
    # fp32 rounding sits some 60 dB below the bank's own reconstruction error
    assert snr64 > 50.0 and abs(snr - snr64) < 0.1, (snr, snr64)


# ---- EBENGenerator(m=4, n=512, p=2) -----------------------------------------------------------------------------------------------
def build_generator_512(banks_golden):
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    gen = EBENGenerator(m=4, n=512, p=2)
    shapes = {k: tuple(v.shape) for k, v in gen.state_dict().items()}
    sd = formula_state_dict(shapes, "G512")
    sd["pqmf.analysis_weights"] = torch.from_numpy(banks_golden["bank4x512/analysis"])
    sd["pqmf.synthesis_weights"] = torch.from_numpy(banks_golden["bank4x512/synthesis"])
    gen.load_state_dict(sd, strict=True)
    return gen.to(DEV)


@pytest.mark.parametrize("use_engine", [True, False])
def test_generator_n512_matches_the_reference(hip, banks_golden, use_engine):
    gen = build_generator_512(banks_golden)
    gen.use_engine = use_engine
    x = gen.cut_to_valid_length(formula_audio("g512_in", 1, 1536))
    assert x.shape[2] == 1536
    seed = formula_audio("g512_seed", 1, 1536, amp=1.0).to(DEV)
    want = {k: torch.from_numpy(banks_golden[f"gen512/{k}"]) for k in ("enhanced", "bands", "grad_in", "grad_first_conv", "grad_last_conv")}

    # the input as data (the engine's path when use_engine is on): outputs, and the parameter gradients at the ends of the chain
    enhanced, bands = gen(x.to(DEV))
    assert enhanced.shape == x.shape and bands.shape == (1, 4, 512)
    mse = float(((enhanced.detach().cpu().double() - want["enhanced"].double()) ** 2).mean())
    err_bands = rel_l2(bands, want["bands"])
    (enhanced * seed).sum().backward()
    # the bar of test_gpu_models.py for parameter gradients (the graph is discontinuous: isolated LeakyReLU mask flips)
    err_params = {k: rel_l2(p.grad, want[k]) for k, p in (("grad_first_conv", gen.first_conv.weight), ("grad_last_conv", gen.last_conv.weight))}
    print("use_engine", use_engine, "mse", mse, "bands", err_bands, err_params)
    assert mse < 1e-10 and err_bands < TOL
    assert max(err_params.values()) < 2e-3, err_params

    # the input asks for its gradient: through first_conv and through the lifted first bands (eben_generator.py:203-208)
    xd = x.to(DEV).requires_grad_(True)
    enhanced, bands = gen(xd)
    (enhanced * seed).sum().backward()
    err_in = rel_l2(xd.grad, want["grad_in"])
    print("use_engine", use_engine, "input gradient", err_in, "bands", rel_l2(bands, want["bands"]))
    assert rel_l2(bands, want["bands"]) < TOL and err_in < TOL
