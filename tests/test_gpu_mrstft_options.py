"""GPU: MultiResolutionSTFTLoss with the options beyond multi_stft.yaml (stft_terms.hip through stft._WeightedTerms) against the float64
restatement of tests/stft_terms_oracle.py, the default configuration's isolation from the new entry points, and one EBEN training
step with the reference's mel option.

As in tests/test_gpu_stft.py, the device work runs in child processes (EBEN_STFT_GEMM, read once per process, picks the route of the
folded contractions), and each case is held to the per-mode bounds derived from its own conditioning: the loss to the mode's relative
tolerance, the input gradient in relative L2 to the larger of the mode's bound and MODEL_FACTOR x the float64 gradient's movement when
every spectrum is perturbed at the arithmetic's scale.

Run as a script (``python tests/test_gpu_mrstft_options.py cases|step OUT``) it is the child: it writes the device results to OUT."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_gpu_stft import FP32_GRADE, GRAD_CHECK_MAX, MODE_TOL, MODEL_FACTOR, MODES, U32  # noqa: E402

pytestmark = pytest.mark.gpu

REF3 = ((512, 1024, 2048), (50, 120, 240), (240, 600, 1200))   # the reference's three resolutions (fft, hop, win)
# name -> constructor options; every window, every weight set with and without mel, both distances
CONFIGS = {
    "mel128_hann_sc_log_L1": dict(scale="mel", n_bins=128),
    "mel128_hann_sc_log_L2": dict(scale="mel", n_bins=128, mag_distance="L2"),
    "mel128_kaiser_sc_log_L1": dict(scale="mel", n_bins=128, window="kaiser_window"),
    "mel128_hamming_sc_lin_L1": dict(scale="mel", n_bins=128, window="hamming_window", w_log_mag=0.0, w_lin_mag=1.0),
    "mel40_hann_mixed_L1": dict(scale="mel", n_bins=40, w_sc=0.5, w_log_mag=2.0, w_lin_mag=1.0),
    "mel40_bartlett_log_L2": dict(scale="mel", n_bins=40, window="bartlett_window", w_sc=0.0, mag_distance="L2"),
    "none_hann_sc_lin_L1": dict(w_log_mag=0.0, w_lin_mag=1.0),
    "none_hann_log_L2": dict(w_sc=0.0, mag_distance="L2"),
    "none_hann_sc_log_L2": dict(mag_distance="L2"),
    "none_hamming_mixed_L2": dict(window="hamming_window", w_sc=0.5, w_log_mag=2.0, w_lin_mag=1.0, mag_distance="L2"),
    "none_blackman_sc_lin_L2": dict(window="blackman_window", w_log_mag=0.0, w_lin_mag=1.0, mag_distance="L2"),
    "none_kaiser_log_L1": dict(window="kaiser_window", w_sc=0.0),
}
# name -> (rows, t, perceptual): the bench clip length at batch 4; ragged lengths (not a multiple of any hop); the edge rows
INPUTS = {"main": (4, 31968, True), "ragged": (3, 4001, False), "edge": (4, 8017, True)}


def _inputs(name):
    rows, t, _ = INPUTS[name]
    g = torch.Generator().manual_seed({"main": 11, "ragged": 12, "edge": 13}[name])
    y = 0.1 * torch.randn(rows, 1, t, generator=g)
    x = 0.1 * torch.randn(rows, 1, t, generator=g)
    if name == "edge":   # rows: silent in both; x == y bit for bit; silent in y only; an ordinary pair
        x[0], y[0], x[1], y[2] = 0.0, 0.0, y[1], 0.0
    return x, y


def _module(kw, perceptual, dev):
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss
    return MultiResolutionSTFTLoss(fft_sizes=REF3[0], hop_sizes=REF3[1], win_lengths=REF3[2], sample_rate=16000,
                                   perceptual_weighting=perceptual, **kw).to(dev)


def _run_child(kind, env, tmp, timeout):
    path = os.path.join(tmp, f"{kind}_{'_'.join(f'{k}{v}' for k, v in sorted(env.items()))}.pt")
    subprocess.run([sys.executable, os.path.abspath(__file__), kind, path], check=True, env={**os.environ, **env}, timeout=timeout, cwd=ROOT)
    return torch.load(path)


# ---------------------------------------------------------------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------------------------------------------------------------
def _cases_child(out_path):
    from vibravox_amd import _lib

    dev = torch.device("cuda")
    res = {}
    for cname, kw in CONFIGS.items():
        for iname, (rows, t, perceptual) in INPUTS.items():
            x, y = _inputs(iname)
            loss = _module(kw, perceptual, dev)
            for mode in MODES:
                loss.stft_math = mode
                xd = x.to(dev).requires_grad_(True)
                got = loss(xd, y.to(dev))
                out = {"maths": [p.math_for(mode) for p in loss._plans]}
                if iname == "edge":   # did row 1's x and y spectra come out bit for bit equal in every resolution?
                    same = True
                    for spec, _, frames, _, _ in got.grad_fn.saved:
                        same = same and bool(torch.equal(spec[0, :, frames:2 * frames], spec[0, :, (rows + 1) * frames:(rows + 2) * frames]))
                    out["spectra_equal"] = same
                got.backward()
                torch.cuda.synchronize()
                out.update(value=float(got.item()), grad=xd.grad.cpu())
                res[(cname, iname, mode)] = out

    # the default configuration never enters the new entry points: with their bindings raising, the module of multi_stft.yaml and one
    # given the same defaults explicitly run every mode, bit for bit alike; a non-default module does reach them
    lib = _lib.load()
    names = ("eben_stft_terms_fwd", "eben_stft_terms_bwd", "eben_stft_terms_total", "eben_stft_terms_workspace")
    saved = {n: getattr(lib, n) for n in names}

    def refuse(*_a, **_k):
        raise RuntimeError("the default configuration entered an stft_terms entry point")

    x, y = _inputs("main")
    plain = _module({}, True, dev)
    explicit = _module(dict(window="hann_window", w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0, scale=None, mag_distance="L1",
                            reduction="mean", output="loss"), True, dev)
    try:
        for n in names:
            setattr(lib, n, refuse)
        for mode in MODES:
            outs = []
            for m in (plain, explicit):
                m.stft_math = mode
                xd = x.to(dev).requires_grad_(True)
                v = m(xd, y.to(dev))
                v.backward()
                torch.cuda.synchronize()
                outs.append((v.detach().cpu(), xd.grad.cpu()))
            res[("default", mode)] = dict(value_equal=bool(torch.equal(outs[0][0], outs[1][0])), grad_equal=bool(torch.equal(outs[0][1], outs[1][1])),
                                          value=float(outs[0][0]), grad=outs[0][1])
        try:
            _module(dict(scale="mel", n_bins=128), True, dev)(x.to(dev), y.to(dev))
            res["patched_reached"] = False
        except RuntimeError as e:
            res["patched_reached"] = "stft_terms" in str(e)
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)
    torch.save(res, out_path)


STEP_BATCH, STEP_LEN, STEP_SEED = 4, 32000, 1234


def _step_child(out_path):
    import bench

    dev = torch.device("cuda")
    res = {}
    for precision in ("bf16-mixed", "32-true"):
        for literal in (False, True):
            mod = bench.build_module(dev, STEP_SEED)
            mod.reconstructive_loss_freq_fn = _module(dict(scale="mel", n_bins=128), True, dev)
            mod.set_precision(precision)
            mod.exploit_step_redundancy = not literal
            out = mod.training_step(bench.synthetic_batch(STEP_BATCH, STEP_LEN, STEP_SEED, dev))
            torch.cuda.synchronize()
            res[(precision, literal)] = dict(logged={k: float(v.detach().double().item()) for k, v in mod.logged.items() if v.numel() == 1},
                                             enhanced=out["enhanced"].detach().cpu(), reference=out["reference"].detach().cpu(),
                                             stft_math=mod.reconstructive_loss_freq_fn.stft_math)
    torch.save(res, out_path)


ROUTES = {"gemm1": {"EBEN_STFT_GEMM": "1"}, "gemm0": {"EBEN_STFT_GEMM": "0"}}


@pytest.fixture(scope="module", params=sorted(ROUTES))
def case_results(request, hip, tmp_path_factory):
    return request.param, _run_child("cases", ROUTES[request.param], str(tmp_path_factory.mktemp("mrstft_opt")), 1500)


@pytest.fixture(scope="module")
def step_results(hip, tmp_path_factory):
    return _run_child("step", {}, str(tmp_path_factory.mktemp("mrstft_step")), 1500)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 side
# ---------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _fir():
    from oracle import eben_oracle as O
    return O.a_weighting_fir(16000).double()


def _oracle(cname, iname):
    """float64 loss and input gradient, and the gradient's relative L2 movement under spectrum noise at fp32 and bf16-grade scale."""
    key = (cname, iname)
    if key not in _ORACLE:
        from stft_terms_oracle import mrstft_terms_loss
        x, y = _inputs(iname)
        kw = dict(CONFIGS[cname], fir=_fir() if INPUTS[iname][2] else None)
        geo = dict(fft_sizes=REF3[0], hop_sizes=REF3[1], win_lengths=REF3[2])
        rx = x.double().requires_grad_(True)
        ref = mrstft_terms_loss(rx, y.double(), **geo, **kw)
        ref.backward()
        model = {}
        for name, rel in (("fp32", U32), ("bf16", 2.0 ** -17)):
            fx = x.double().requires_grad_(True)
            mrstft_terms_loss(fx, y.double(), **geo, **kw, noise_rel=rel).backward()
            model[name] = float((fx.grad - rx.grad).norm() / rx.grad.norm())
        _ORACLE[key] = (float(ref.detach()), rx.grad.clone(), model)
    return _ORACLE[key]


def grad_bound(mode, model):
    bound = max(MODE_TOL[mode][1], MODEL_FACTOR * model["fp32" if mode in FP32_GRADE else "bf16"])
    return bound if bound < GRAD_CHECK_MAX else None


def _check(got, ref_value, ref_grad, model, mode, what):
    grad = got["grad"].double()
    assert math.isfinite(got["value"]) and torch.isfinite(grad).all(), what
    np.testing.assert_allclose(got["value"], ref_value, rtol=MODE_TOL[mode][0], err_msg=str(what))
    bound = grad_bound(mode, model)
    if bound is not None:
        err = float((grad - ref_grad).norm() / ref_grad.norm())
        assert err < bound, (what, err, bound, model)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("iname", ["main", "ragged"])
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_options_against_float64(case_results, cname, iname, mode):
    route, res = case_results
    got = res[(cname, iname, mode)]
    foldable = CONFIGS[cname].get("window", "hann_window") not in ("hamming_window", "kaiser_window")
    assert got["maths"] == [mode if foldable else "dense"] * 3, got["maths"]
    _check(got, *_oracle(cname, iname), mode, (route, cname, iname, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_options_silent_and_identical_rows(case_results, cname, mode):
    """Row 0 silent in x and y, row 1 with x == y bit for bit, row 2 silent in y only, row 3 ordinary: a finite loss, float64's exact
    zero gradient on rows 0 and 1, and the device's too -- on row 1 wherever its x and y spectra came out bit for bit equal."""
    route, res = case_results
    got = res[(cname, "edge", mode)]
    ref_value, ref_grad, model = _oracle(cname, "edge")
    assert float(ref_grad[0].abs().max()) == 0.0 and float(ref_grad[1].abs().max()) == 0.0
    _check(got, ref_value, ref_grad, model, mode, (route, cname, mode))
    assert float(got["grad"][0].abs().max()) == 0.0
    if got["spectra_equal"]:
        assert float(got["grad"][1].abs().max()) == 0.0
    else:
        warnings.warn(f"{route} {cname} {mode}: row 1's x and y spectra differ on the device; its zero gradient is held only in L2")


def test_gradient_checks_cover_most_cases():
    """The conditioning filter leaves a gradient assertion on most (configuration, input) pairs of every mode."""
    pairs = [(c, i) for c in CONFIGS for i in ("main", "ragged")]
    for mode in MODES:
        checked = [p for p in pairs if grad_bound(mode, _oracle(*p)[2]) is not None]
        assert len(checked) >= (0.9 if mode in FP32_GRADE else 0.6) * len(pairs), (mode, len(checked), len(pairs))


@pytest.mark.parametrize("mode", MODES)
def test_default_configuration_stays_on_its_kernels(case_results, mode):
    route, res = case_results
    got = res[("default", mode)]
    assert res["patched_reached"], "the patched bindings were not reached by a mel module: the isolation check proves nothing"
    assert got["value_equal"] and got["grad_equal"], (route, mode)
    from oracle import eben_oracle as O
    x, y = _inputs("main")
    ref = O.mrstft_loss(x.double(), y.double(), fft_sizes=REF3[0], hop_sizes=REF3[1], win_lengths=REF3[2], perceptual_weighting=True, fir=_fir())
    np.testing.assert_allclose(got["value"], float(ref), rtol=MODE_TOL[mode][0])


@pytest.mark.parametrize("precision", ["bf16-mixed", "32-true"])
def test_train_step_with_the_mel_loss(step_results, precision):
    """One EBEN step (bench's module, batch 4) with the reference's mel option: the logged frequency loss is finite and is the float64
    restatement of that step's enhanced / reference; the engine step agrees with the literal one (exploit_step_redundancy=False) --
    at the bf16 step's tolerances for "bf16-mixed" (test_gpu_models.BF16_STEP_TOLERANCES), the fp32 replays' for "32-true"."""
    from stft_terms_oracle import mrstft_terms_loss
    from tests.test_gpu_models import BF16_STEP_TOLERANCES as TOL

    eng, lit = step_results[(precision, False)], step_results[(precision, True)]
    # the engine step writes the plan's stft_math into the loss module (eben.py); the literal step runs the module's own
    assert eng["stft_math"] == ("folded_x3" if precision == "bf16-mixed" else "folded")
    key = "train/generator/reconstructive_loss_freq"
    for run in (eng, lit):
        v = run["logged"][key]
        assert math.isfinite(v)
        ref = mrstft_terms_loss(run["enhanced"].double(), run["reference"].double(), fft_sizes=REF3[0], hop_sizes=REF3[1],
                                win_lengths=REF3[2], scale="mel", n_bins=128, fir=_fir())
        np.testing.assert_allclose(v, float(ref), rtol=MODE_TOL[run["stft_math"]][0], err_msg=precision)
    assert set(eng["logged"]) == set(lit["logged"])
    for k, v in lit["logged"].items():
        if precision == "bf16-mixed":
            rtol = TOL["feature_matching_loss"] if "feature_matching" in k else TOL["backprop_loss"] if "backprop" in k else TOL["loss"]
        else:
            rtol = 2e-3 if "backprop" in k else 5e-4
        assert abs(eng["logged"][k] - v) <= rtol * abs(v), (precision, k, eng["logged"][k], v)


if __name__ == "__main__":
    {"cases": _cases_child, "step": _step_child}[sys.argv[1]](sys.argv[2])
