"""CPU: the FIR-bank dispatch's host-side plan query (eben_fir_plan), its ABI, and the CPU-side bank design of
PseudoQMFBanks at sizes other than (4, 32) against banks frozen from the reference (tests/golden/make_pqmf_banks_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBEN_EUNSUPPORTED = -3


@pytest.fixture(scope="module")
def banks_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pqmf_banks_golden.npz"))


def plan(lib, bands, ntaps, stride, which):
    out = (ctypes.c_int * 4)(-1, -1, -1, -1)
    rc = lib.eben_fir_plan(bands, ntaps, stride, which, out, 4)
    return rc, list(out)


@pytest.mark.parametrize("which", [0, 1])
def test_fir_plan_reports_the_kernel_of_each_bank(which):
    from vibravox_amd import _lib

    lib = _lib.load()
    # what the three kernels of direct.hip took before the tap-tiled ones existed stays with them
    for (bands, ntaps, stride), kernel in (((4, 32, 4), 1), ((2, 32, 4), 1), ((1, 32, 4), 1), ((1, 101, 1), 2), ((8, 64, 8), 3),
                                           ((1, 1024, 32), 3), ((1, 3, 1), 3), ((3, 32, 4), 3)):
        rc, out = plan(lib, bands, ntaps, stride, which)
        assert rc == 0 and out[0] == kernel and out[1] > 0 and out[2] == 0 and out[3] > 0, ((bands, ntaps, stride), rc, out)
    # what they refused goes to fir_bank.hip
    for bands, ntaps, stride in ((32, 1024, 32), (2, 1024, 32), (4, 512, 4), (1, 4096, 1), (16, 256, 16), (64, 1024, 64), (64, 4096, 64),
                                 (64, 4096, 1), (3, 700, 5)):
        rc, out = plan(lib, bands, ntaps, stride, which)
        assert rc == 0 and out[0] == 4 and min(out[1:]) > 0, ((bands, ntaps, stride), rc, out)
    rc, out = plan(lib, 32, 1024, 32, which)
    assert out[2] == 64 and out[3] == 32 and out[1] == (128 if which == 0 else 128 * 32)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("bank", [(65, 16, 4), (4, 4097, 4), (4, 512, 65)])
def test_fir_plan_refuses_banks_outside_the_domain(which, bank):
    from vibravox_amd import _lib

    lib = _lib.load()
    rc, _ = plan(lib, *bank, which)
    assert rc == EBEN_EUNSUPPORTED
    msg = lib.eben_last_error().decode()
    assert "outside" in msg and all(str(v) in msg for v in bank), msg


def test_fir_plan_abi_is_declared_bound_and_exported():
    from vibravox_amd import _lib

    header = open(os.path.join(ROOT, "include", "eben_hip.h")).read()
    declared = set(re.findall(r"EBEN_API\s+[\w\s\*]+?\b(eben_\w+)\s*\(", header))
    lib = _lib.load()
    assert "eben_fir_plan" in declared and "eben_fir_plan" in _lib.SIGNATURES and hasattr(lib, "eben_fir_plan")
    assert int(re.search(r"#define EBEN_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.eben_version()
    assert lib.eben_fir_plan(4, 32, 4, 0, None, 4) < 0 and lib.eben_fir_plan(4, 32, 4, 0, (ctypes.c_int * 4)(), 3) < 0


@pytest.mark.parametrize("m,n", [(8, 64), (16, 256), (32, 1024), (4, 512)])
def test_bank_design_matches_the_reference(banks_golden, m, n):
    """max-abs <= 1e-7 on the banks (SURVEY.md appendix B's fallback rule), the same cutoff to 1e-9."""
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    pq = PseudoQMFBanks(m, n)
    tag = f"{m}x{n}"
    assert abs(pq._cutoff_ratio - float(banks_golden[f"bank{tag}/cutoff"])) <= 1e-9
    for name, got in (("analysis", pq.analysis_weights), ("synthesis", pq.synthesis_weights)):
        want = banks_golden[f"bank{tag}/{name}"]
        assert got.shape == want.shape == (m, 1, n)
        assert float(np.abs(got.detach().numpy().astype(np.float64) - want.astype(np.float64)).max()) <= 1e-7, (tag, name)


def test_cut_lengths_follow_the_bank_size():
    """cut_to_valid_length / cut_tensor at n != 32 (eben_generator.py:215-222, pqmf.py:217-232)."""
    import torch

    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator
    from vibravox_amd.torch_modules.dsp.pqmf import PseudoQMFBanks

    gen = EBENGenerator(m=4, n=512, p=2)
    for length in (1536, 1537, 2000, 16000):
        cut = gen.cut_to_valid_length(torch.zeros(1, 1, length)).shape[2]
        assert cut == length - (length + 512) % 256 and (cut + 512) % 256 == 0
    pq = PseudoQMFBanks(16, 256)
    for length in (2128, 2129, 2143):
        assert pq.cut_tensor(torch.zeros(1, 1, length)).shape[2] == length - (length + 256) % 16
