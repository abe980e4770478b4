"""GPU: the MRSTFT loss's framing and overlap-add kernels (stft.hip) and MultiResolutionSTFTLoss against float64 restatements.

Kernels: eben_stft_frames, eben_stft_frames_folded (split 0 / 1) and eben_overlap_add_ex / eben_overlap_add_folded against an explicit
index restatement of what they are specified to compute, never against each other; both launches of each (LDS transpose / tile and the
gather kernels) through EBEN_STFT_FRAMES_T / EBEN_OLA_TILED, which are read once per process -- so every route runs its whole grid in a
child process of its own.  Module: one resolution per case against oracle.mrstft_loss in float64 (torch.stft), every stft_math, both
contraction routes (EBEN_STFT_GEMM) and both loss totals (EBEN_FUSED_LOSS_GLUE, and nine resolutions for the unfused one), plus rows of
silence and a row whose enhanced signal equals its reference bit for bit.

Run as a script (``python tests/test_gpu_stft.py kernels|module OUT``) it is the child: it writes the device results to OUT."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24   # unit roundoff of fp32
OLA_U = 512        # stft.hip: samples per block of overlap_add_folded_t_kernel

# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
# (win, hop), pad = win/2: the three default resolutions; a tiled overlap-add with pad > OLA_U; a tile over the 64 KB LDS cap (gather);
# gaps between frames (hop > win); hop 1-2 tiles of more than 256 frames (gather); win/2 not a multiple of 64
KGEOM = [(240, 50), (600, 120), (1200, 240), (2048, 1024), (4096, 512), (64, 300), (16, 1), (32, 2), (126, 3)]
KROWS = 2


def _klengths(win):
    pad = win // 2
    ts = {pad + 1, 2 * pad, 2 * pad + 1, 511, 512, 513, 2 * pad + 3 * OLA_U + 77}
    if win in (240, 600, 1200):
        ts.add(31968)
    return sorted(t for t in ts if t > pad and t > 1)


KCASES = [(w, h, t) for w, h in KGEOM for t in _klengths(w)]


def _kid(win, hop, t):
    return f"w{win}_h{hop}_t{t}"


def _kinputs(win, hop, t):
    """The seeded inputs of one kernel case (CPU, float32): signal, frame-space gradients in the flat (win, rows*frames) layout and in a
    padded (rows, win, frames + 5) one, their folded counterparts, and the base the accumulating launches add to."""
    frames = t // hop + 1
    cols, h = KROWS * frames, win // 2
    g = torch.Generator().manual_seed(win * 100003 + hop * 1009 + t)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(frames=frames, sig=r(KROWS, t), g=r(win, cols), gs=r(KROWS, win, frames + 5), gf=r(2 * h, cols),
                gfs=r(KROWS, 2 * h, frames + 5), base=r(KROWS, t))


def _kernel_child(out_path):
    from vibravox_amd._lib import check, load, ptr, stream

    lib, dev = load(), torch.device("cuda")
    res = {}
    for win, hop, t in KCASES:
        inp = _kinputs(win, hop, t)
        frames, pad, h = inp["frames"], win // 2, win // 2
        cols = KROWS * frames
        d = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
        o = {}
        fr = torch.empty(win, cols, device=dev)
        check(lib.eben_stft_frames(ptr(d["sig"]), ptr(fr), KROWS, t, win, hop, pad, frames, stream()), "stft_frames")
        o["fr"] = fr
        for split in (0, 1):
            ff = torch.full(((3 if split else 1) * 2 * h, cols), float("nan"), device=dev)
            check(lib.eben_stft_frames_folded(ptr(d["sig"]), ptr(ff), KROWS, t, win, hop, pad, frames, split, stream()), "stft_frames_folded")
            o[f"ff{split}"] = ff
        for reflect in (0, 1):
            for acc in (0, 1):
                x = d["base"].clone() if acc else torch.full((KROWS, t), float("nan"), device=dev)
                check(lib.eben_overlap_add_ex(ptr(d["g"]), ptr(x), KROWS, t, win, frames, hop, pad, reflect, acc, frames, cols, stream()), "ola")
                o[f"ola{reflect}{acc}"] = x
        x = d["base"].clone()   # (rows, win, frames + 5): row stride win * (frames + 5), sample stride frames + 5
        check(lib.eben_overlap_add_ex(ptr(d["gs"]), ptr(x), KROWS, t, win, frames, hop, pad, 1, 1, win * (frames + 5), frames + 5, stream()),
              "ola_strided")
        o["ola_s"] = x
        for acc in (0, 1):
            x = d["base"].clone() if acc else torch.full((KROWS, t), float("nan"), device=dev)
            check(lib.eben_overlap_add_folded(ptr(d["gf"]), ptr(x), KROWS, t, win, frames, hop, pad, acc, frames, cols, stream()), "ola_folded")
            o[f"olaf{acc}"] = x
        x = d["base"].clone()
        check(lib.eben_overlap_add_folded(ptr(d["gfs"]), ptr(x), KROWS, t, win, frames, hop, pad, 1, 2 * h * (frames + 5), frames + 5, stream()),
              "ola_folded_strided")
        o["olaf_s"] = x
        torch.cuda.synchronize()
        res[_kid(win, hop, t)] = {k: v.cpu() for k, v in o.items()}
        res[_kid(win, hop, t)]["tiled"] = lib.eben_overlap_add_folded_tiled(t, win, hop, pad)   # the launch those calls took
    torch.save(res, out_path)


def _run_child(kind, env, tmp, timeout):
    path = os.path.join(tmp, f"{kind}_{'_'.join(f'{k}{v}' for k, v in sorted(env.items()))}.pt")
    subprocess.run([sys.executable, os.path.abspath(__file__), kind, path], check=True, env={**os.environ, **env}, timeout=timeout, cwd=ROOT)
    return torch.load(path)


KROUTES = {"lds": {"EBEN_STFT_FRAMES_T": "1", "EBEN_OLA_TILED": "1"}, "gather": {"EBEN_STFT_FRAMES_T": "0", "EBEN_OLA_TILED": "0"}}


@pytest.fixture(scope="module", params=sorted(KROUTES))
def kernel_results(request, hip, tmp_path_factory):
    return request.param, _run_child("kernels", KROUTES[request.param], str(tmp_path_factory.mktemp("stft_k")), 1200)


def test_kernel_grid_covers_both_overlap_add_launches(kernel_results):
    """Which launch eben_overlap_add_folded took for every case, as the library's own gate reports it: the LDS tile for the default
    resolutions, pad > OLA_U and hop > win; the gather kernel over the LDS cap and for hop 1-2 tiles of more than 256 frames; only the
    gather kernel under EBEN_OLA_TILED=0."""
    route, res = kernel_results
    tiled = {(w, h) for w, h, t in KCASES if res[_kid(w, h, t)]["tiled"]}
    if route == "gather":
        assert not tiled
        return
    assert {(240, 50), (600, 120), (1200, 240), (2048, 1024), (64, 300)} <= tiled
    assert not tiled & {(4096, 512), (16, 1), (32, 2), (126, 3)}
    for w, h, t in KCASES:   # and never with the reflected ends overlapping inside one tile
        assert not res[_kid(w, h, t)]["tiled"] or t > w, (w, h, t)


def _reflect_index(win, hop, pad, frames, t):
    """(win, frames) signal index of window sample j of frame f (reflect-padded by pad), and the unreflected one."""
    q0 = torch.arange(frames).unsqueeze(0) * hop + torch.arange(win).unsqueeze(1) - pad
    q = torch.where(q0 < 0, -q0, q0)
    q = torch.where(q >= t, 2 * (t - 1) - q, q)
    assert int(q.min()) >= 0 and int(q.max()) < t
    return q, q0


def _ola64(buf, q, keep, t):
    """float64 overlap-add of buf (rows, win, frames) onto (rows, t): sample q[j, f] of each row gets buf[r, j, f] where keep."""
    out = torch.zeros(buf.shape[0], t, dtype=torch.float64)
    idx, src = q[keep], buf.double()[:, keep]
    for r in range(buf.shape[0]):
        out[r].index_add_(0, idx, src[r])
    return out


def _unfold64(bf, absolute=False):
    """(rows, 2h, frames) [dE ; dO] -> (rows, win, frames): sample h + m gets dE[|m|] + sign(m) dO[|m|], sample 0 nothing
    (absolute: |dE[|m|]| + |dO[|m|]|, a bound on every term)."""
    rows, h2, frames = bf.shape
    h = h2 // 2
    e, o = bf[:, :h].double(), bf[:, h:].double()
    if absolute:
        e, o = e.abs(), o.abs()
    d = torch.zeros(rows, 2 * h, frames, dtype=torch.float64)
    d[:, h] = e[:, 0]
    d[:, h + 1:] = e[:, 1:] + o[:, 1:]
    d[:, 1:h] = ((e[:, 1:] + o[:, 1:]) if absolute else (e[:, 1:] - o[:, 1:])).flip(1)
    return d


def _flat(g, frames):
    """(win, rows*frames) -> (rows, win, frames)"""
    return g.reshape(g.shape[0], KROWS, frames).transpose(0, 1)


def _check_ola(got, ref, bound, what):
    assert torch.isfinite(got).all(), what
    err = (got.double() - ref).abs()
    worst = int(torch.argmax(err - bound))
    assert bool((err <= bound).all()), (what, float(err.flatten()[worst]), float(bound.flatten()[worst]))


@pytest.mark.parametrize("win,hop,t", KCASES, ids=[_kid(*c) for c in KCASES])
def test_framing_and_overlap_add_against_float64(kernel_results, win, hop, t):
    route, res = kernel_results
    check_kernel_case(res[_kid(win, hop, t)], win, hop, t, route)


def check_kernel_case(o, win, hop, t, route):
    inp = _kinputs(win, hop, t)
    frames, pad, h = inp["frames"], win // 2, win // 2
    q, q0 = _reflect_index(win, hop, pad, frames, t)

    # framing is a copy: bit for bit
    want = inp["sig"][:, q].transpose(0, 1).reshape(win, KROWS * frames)
    assert torch.equal(o["fr"], want)
    # folded parts: one fp32 add each (CPU float32 rounds the same), O[0] = 0; split: [hi ; lo ; hi] per group, RNE bf16
    m = torch.arange(1, h)
    e = torch.cat((want[h:h + 1], want[h + m] + want[h - m]))
    od = torch.cat((torch.zeros_like(want[:1]), want[h + m] - want[h - m]))
    assert torch.equal(o["ff0"], torch.cat((e, od))), route
    parts = []
    for v in (e, od):
        hi = v.to(torch.bfloat16).float()
        parts += [hi, (v - hi).to(torch.bfloat16).float(), hi]
    assert torch.equal(o["ff1"], torch.cat(parts))

    # overlap-add: float64 scatter of the same terms; each output sums <= 3 (win/hop + 1) fp32 terms (+ the accumulated base), so
    # |err| <= n u sum|terms| with n that count (+1 more fp32 add per term for the folded form's dE +- dO)
    n = 3 * (win // hop + 1) + 1
    inside = (q0 >= 0) & (q0 < t)
    everywhere = torch.ones_like(inside)
    base = inp["base"].double()
    g = _flat(inp["g"], frames)
    for reflect in (0, 1):
        qq, keep = (q, everywhere) if reflect else (q0.clamp(0, t - 1), inside)
        ref, mag = _ola64(g, qq, keep, t), _ola64(g.abs(), qq, keep, t)
        for acc in (0, 1):
            r, s = (ref + base, mag + base.abs()) if acc else (ref, mag)
            _check_ola(o[f"ola{reflect}{acc}"], r, n * U32 * s + 1e-30, (route, "ola", reflect, acc))
    gs = inp["gs"][:, :, :frames]
    _check_ola(o["ola_s"], _ola64(gs, q, everywhere, t) + base, n * U32 * (_ola64(gs.abs(), q, everywhere, t) + base.abs()), (route, "ola strided"))
    gf = _flat(inp["gf"], frames)
    nf = 2 * n
    for buf, key, acc in ((gf, "olaf0", 0), (gf, "olaf1", 1), (inp["gfs"][:, :, :frames], "olaf_s", 1)):
        ref, mag = _ola64(_unfold64(buf), q, everywhere, t), _ola64(_unfold64(buf, absolute=True), q, everywhere, t)
        if acc:
            ref, mag = ref + base, mag + base.abs()
        _check_ola(o[key], ref, nf * U32 * mag + 1e-30, (route, key))

    # adjoint pairs: <frames(s), g> = <s, OLA(g)> in float64 sums of the fp32 results, to the OLA outputs' bound (and the folded
    # parts' own rounding)
    sig = inp["sig"].double()
    lhs = float((o["fr"].double() * inp["g"].double()).sum())
    rhs = float((sig * o["ola10"].double()).sum())
    tol = float((sig.abs() * n * U32 * _ola64(g.abs(), q, everywhere, t)).sum()) + 1e-9
    assert abs(lhs - rhs) <= tol, (route, "dense adjoint", lhs, rhs, tol)
    lhs = float((o["ff0"].double() * inp["gf"].double()).sum())
    rhs = float((sig * o["olaf0"].double()).sum())
    tol = (float((sig.abs() * nf * U32 * _ola64(_unfold64(gf, absolute=True), q, everywhere, t)).sum())
           + U32 * float((o["ff0"].double().abs() * inp["gf"].double().abs()).sum()) + 1e-9)
    assert abs(lhs - rhs) <= tol, (route, "folded adjoint", lhs, rhs, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# MultiResolutionSTFTLoss
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ["folded", "dense", "bf16x3", "folded_x3", "folded_x6"]
# (loss rtol, gradient relative L2): test_gpu_ops.STFT_MATH_TOL for the modes it has; "folded_x6" (fp32-grade split products) takes
# "folded"'s, "folded_x3" (two bf16 pieces, ~2^-17) "bf16x3"'s
MODE_TOL = {"folded": (2e-5, 2e-3), "dense": (2e-5, 2e-3), "bf16x3": (5e-5, 1e-2), "folded_x6": (2e-5, 2e-3), "folded_x3": (5e-5, 1e-2)}
# The gradient's relative L2 error is not a property of the kernels alone: d|log X - log Y| / dX = sign(.) / |X| is largest on the
# smallest bins, where any rounding moves it most (and flips the sign).  torch.stft itself in float32 misses 2e-3 at some of these
# inputs (up to 3.5e-3, e.g. (32, 2, 32) with A-weighting).  So each case measures its own conditioning: the float64 gradient's error
# when every spectrum is perturbed at the arithmetic's scale (_perturbed_mrstft: 2^-24 for the fp32-grade modes, 2^-17 for the
# bf16-grade ones), and the device is held to the larger of the mode's bound and MODEL_FACTOR x that error.  Where that bound is not
# below GRAD_CHECK_MAX (0.25: an all-zero gradient is 1 away, a sign-flipped one 2) the input is too ill-conditioned for the gradient to
# say anything and only the loss value is checked; test_mrstft_gradient_checks_cover_every_mode keeps that from becoming the rule.
# The contractions themselves are held to elementwise rounding bounds, free of that conditioning, by test_windowed_dft_contractions.
MODEL_FACTOR = 5.0
GRAD_CHECK_MAX = 0.25
FP32_GRADE = ("folded", "dense", "folded_x6")

# (n_fft, hop, win): the kernel geometries at a power-of-two n_fft, and the parities the even-only plan got wrong
MGEOM = [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200), (2048, 1024, 2048), (4096, 512, 4096), (128, 300, 64), (16, 1, 16), (32, 2, 32),
         (128, 3, 126), (512, 50, 241), (511, 50, 240), (511, 50, 241)]
MROWS = [(2, 1), (3, 2)]
MT = 4000   # a multiple of hop 50: the frame count of (512, 50, 241) / (511, 50, 240) differs from the even-only plan's exactly there
NINE = [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200), (256, 25, 128), (512, 64, 512), (1024, 256, 1024), (511, 50, 241), (128, 3, 126),
        (64, 300, 64)]
EDGE_RES = [((512, 1024, 2048), (50, 120, 240), (240, 600, 1200)), ((511,), (50,), (241,))]


def _gid(g):
    return "x".join(map(str, g))


def _mcases():
    cases = []
    for geom in MGEOM:
        for perceptual in (True, False):
            for bc in MROWS:
                cases.append(("single", (geom,), perceptual, bc, "indep"))
        for perceptual in (True, False):
            cases.append(("scaled", (geom,), perceptual, (2, 1), "scaled"))
    for perceptual in (True, False):
        cases.append(("nine", tuple(NINE), perceptual, (2, 1), "indep"))
    for k, res in enumerate(EDGE_RES):
        cases.append(("edge", tuple(zip(*res)), True, (4, 1), "edge"))
    return cases


MCASES = _mcases()


def _mkey(kind, geoms, perceptual, bc, pair):
    return f"{kind}_{'+'.join(_gid(g) for g in geoms)}_p{int(perceptual)}_b{bc[0]}c{bc[1]}_{pair}"


def _minputs(bc, pair):
    from formula import formula_audio

    b, c = bc
    rows = b * c
    if pair == "edge":   # rows: silent in both; silent in y only; x == y bit for bit; an ordinary pair
        x, y = formula_audio("stft_e_x", rows, MT), formula_audio("stft_e_y", rows, MT)
        x[0], y[0], y[1], y[2] = 0.0, 0.0, 0.0, x[2]
    else:
        x = formula_audio(f"stft_{rows}_x", rows, MT)
        y = formula_audio(f"stft_{rows}_y", rows, MT)
        if pair == "scaled":   # Y = 0.6 X: log X - log Y = 0.51 on every unclamped bin, no sign of the log term near a flip
            y = 0.6 * x
    return x.reshape(b, c, MT), y.reshape(b, c, MT)


# windowed-DFT contractions (StftPlan.dft / dft_t, the GEMMs of the loss's forward and backward) at every folded-capable geometry of
# MGEOM and one dense-only one; CROWS rows of CT samples
CGEOM = [g for g in MGEOM if g[0] % 2 == 0 and g[2] % 2 == 0] + [(512, 50, 241)]
CROWS, CT = 3, 2500   # CT > 4096 // 2
# |err| <= (PRODUCT_REL[mode] + (K + 2) u) sum_k |w_k| |v_k| per output (K terms accumulated in fp32): fp32 products are exact before
# the accumulation's rounding; "folded_x6" splits each operand into three bf16 pieces (fp32-grade, bounded here at 2^-20 per
# product); "bf16x3" / "folded_x3" drop the lo x lo term and round the lo pieces, 3 x 2^-16 per product at most
PRODUCT_REL = {"folded": 0.0, "dense": 0.0, "folded_x6": 2.0 ** -20, "bf16x3": 3 * 2.0 ** -16, "folded_x3": 3 * 2.0 ** -16}


def _cinputs(n_fft, hop, win):
    g = torch.Generator().manual_seed(n_fft * 31 + hop * 7 + win)
    sig = torch.randn(CROWS, CT, generator=g)
    frames = (CT + 2 * (n_fft // 2) - n_fft) // hop + 1
    dspec = torch.randn(2 * (n_fft // 2 + 1), CROWS * frames, generator=g)
    return sig, dspec, frames


def _contraction_child():
    from vibravox_amd._lib import check, load, ptr, stream
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    lib, dev = load(), torch.device("cuda")
    res = {}
    for n_fft, hop, win in CGEOM:
        (plan,) = MultiResolutionSTFTLoss(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,)).to(dev)._build_plans()
        sig, dspec, frames = _cinputs(n_fft, hop, win)
        assert plan.frames(CT) == frames
        sig, dspec, cols = sig.to(dev), dspec.to(dev).unsqueeze(0), CROWS * frames
        for mode in MODES:
            math = plan.math_for(mode)
            if math == "dense":
                fr = torch.empty((1, win, cols), device=dev)
                check(lib.eben_stft_frames(ptr(sig), ptr(fr), CROWS, CT, win, hop, plan.pad, frames, stream()), "frames")
            else:
                fr = torch.empty((1, plan.folded_parts(math)[0].c_in, cols), device=dev)
                check(lib.eben_stft_frames_folded(ptr(sig), ptr(fr), CROWS, CT, win, hop, plan.pad, frames, 1 if math == "bf16x3" else 0,
                                                  stream()), "frames_folded")
            spec, dfr = plan.dft(math, fr, cols), plan.dft_t(math, dspec, cols)
            torch.cuda.synchronize()
            res[(_gid((n_fft, hop, win)), mode)] = dict(math=math, spec=spec[0].cpu(), dfr=dfr[0].cpu())
    return res


def _module_child(out_path):
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    dev = torch.device("cuda")
    res = {"contractions": _contraction_child()}
    for kind, geoms, perceptual, bc, pair in MCASES:
        x, y = _minputs(bc, pair)
        n_fft, hop, win = zip(*geoms)
        loss = MultiResolutionSTFTLoss(fft_sizes=n_fft, hop_sizes=hop, win_lengths=win, sample_rate=16000, perceptual_weighting=perceptual).to(dev)
        for mode in MODES:
            loss.stft_math = mode
            xd = x.to(dev).requires_grad_(True)
            got = loss(xd, y.to(dev))
            out = {}
            if pair == "edge":   # did the device spectra of row 2's x and y come out bit for bit equal, in every resolution?
                # reads _MRSTFTFn's ctx (grad_fn): saved = [(spec, sums, frames, math)] per resolution, spec's columns x rows then y rows
                rows = bc[0] * bc[1]
                same = True
                for spec, sums, frames, _ in got.grad_fn.saved:
                    xs, ys = spec[0, :, 2 * frames:3 * frames], spec[0, :, (rows + 2) * frames:(rows + 3) * frames]
                    same = same and bool(torch.equal(xs, ys))
                out["spectra_equal"] = same
            got.backward()
            torch.cuda.synchronize()
            out.update(value=float(got.item()), grad=xd.grad.cpu())
            res[(_mkey(kind, geoms, perceptual, bc, pair), mode)] = out
    torch.save(res, out_path)


MROUTES = {"gemm1_glue1": {"EBEN_STFT_GEMM": "1", "EBEN_FUSED_LOSS_GLUE": "1"}, "gemm0_glue0": {"EBEN_STFT_GEMM": "0", "EBEN_FUSED_LOSS_GLUE": "0"}}


@pytest.fixture(scope="module", params=sorted(MROUTES))
def module_results(request, hip, tmp_path_factory):
    return request.param, _run_child("module", MROUTES[request.param], str(tmp_path_factory.mktemp("stft_m")), 1200)


_ORACLE = {}


def _perturbed_mrstft(x, y, geoms, perceptual, rel):
    """The oracle's loss in float64 with every spectrum perturbed by seeded noise of rel x (max|signal| sqrt(win)) -- the scale of an
    fp32 windowed DFT's rounding at rel = 2^-24: how far rounding alone can move this input's gradient."""
    from oracle import eben_oracle as O

    b, c, t = x.shape
    if perceptual:
        k = O.a_weighting_fir(16000).double().view(1, 1, -1)
        x = torch.nn.functional.conv1d(x.reshape(b * c, 1, t), k, padding=k.shape[-1] // 2).view(b, c, t)
        y = torch.nn.functional.conv1d(y.reshape(b * c, 1, t), k, padding=k.shape[-1] // 2).view(b, c, t)
    g = torch.Generator().manual_seed(1)
    total = 0.0
    for n_fft, hop, win in geoms:
        def mag(s):
            s = s.reshape(-1, t)
            sp = torch.stft(s, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), return_complex=True)
            scale = float(s.detach().abs().max()) * win ** 0.5 * rel
            sp = sp + scale * torch.complex(torch.randn(sp.shape, generator=g, dtype=torch.float64), torch.randn(sp.shape, generator=g, dtype=torch.float64))
            return torch.sqrt(torch.clamp(sp.real ** 2 + sp.imag ** 2, min=1e-8))
        xm, ym = mag(x), mag(y)
        total = total + (torch.norm(ym - xm, p="fro", dim=[-1, -2]) / torch.norm(ym, p="fro", dim=[-1, -2])).mean()
        total = total + (torch.log(xm) - torch.log(ym)).abs().mean()
    return total / len(geoms)


def _oracle(kind, geoms, perceptual, bc, pair):
    """float64 loss and gradient, and the relative L2 gradient error the perturbation model gives at fp32 and at bf16-grade scale."""
    key = _mkey(kind, geoms, perceptual, bc, pair)
    if key not in _ORACLE:
        from oracle import eben_oracle as O

        x, y = _minputs(bc, pair)
        rx = x.double().requires_grad_(True)
        n_fft, hop, win = zip(*geoms)
        fir = O.a_weighting_fir(16000).double() if perceptual else None
        ref = O.mrstft_loss(rx, y.double(), fft_sizes=n_fft, hop_sizes=hop, win_lengths=win, perceptual_weighting=perceptual, fir=fir)
        ref.backward()
        model = {}
        for name, rel in (("fp32", U32), ("bf16", 2.0 ** -17)):
            fx = x.double().requires_grad_(True)
            _perturbed_mrstft(fx, y.double(), geoms, perceptual, rel).backward()
            model[name] = float((fx.grad - rx.grad).norm() / rx.grad.norm())
        _ORACLE[key] = (ref.item(), rx.grad.clone(), model)
    return _ORACLE[key]


def grad_bound(mode, model):
    """The relative L2 gradient bound of a mode on an input of the given conditioning, or None where the input cannot carry one."""
    bound = max(MODE_TOL[mode][1], MODEL_FACTOR * model["fp32" if mode in FP32_GRADE else "bf16"])
    return bound if bound < GRAD_CHECK_MAX else None


def _check_module(got, ref_value, ref_grad, model, mode, what):
    rtol = MODE_TOL[mode][0]
    grad = got["grad"].double()
    assert math.isfinite(got["value"]) and torch.isfinite(grad).all(), what
    np.testing.assert_allclose(got["value"], ref_value, rtol=rtol, err_msg=str(what))
    bound = grad_bound(mode, model)
    if bound is not None:
        err = float((grad - ref_grad).norm() / ref_grad.norm())
        assert err < bound, (what, err, model)   # sign(log X - log Y) flips at the noise: compared in L2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", CGEOM, ids=[_gid(g) for g in CGEOM])
def test_windowed_dft_contractions(module_results, geom, mode):
    """StftPlan.dft (spectrum of the frames) and dft_t (its adjoint, the backward's frame gradients) on the route the child ran
    (EBEN_STFT_GEMM), elementwise against float64 products of the plan's own basis: a zero, a sign flip, a dropped group or a mis-packed
    transpose is off by the size of the terms, far past the rounding bound."""
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    route, res = module_results
    got = res["contractions"][(_gid(geom), mode)]
    n_fft, hop, win = geom
    (plan,) = MultiResolutionSTFTLoss(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,))._build_plans()
    assert got["math"] == plan.math_for(mode)
    sig, dspec, frames = _cinputs(n_fft, hop, win)
    q, _ = _reflect_index(win, hop, plan.pad, frames, CT)
    fr = sig.double()[:, q].transpose(0, 1).reshape(win, CROWS * frames)       # (win, cols), exact
    basis = plan.basis_f[:, :, 0].double()                                      # (2*bins, win)
    bins, h = plan.bins, win // 2
    rel = PRODUCT_REL[mode]

    def check(out, ref, mag, k, what):
        bound = (rel + (k + 2) * U32) * mag + 1e-30
        err = (out.double() - ref).abs()
        assert torch.isfinite(out).all() and bool((err <= bound).all()), (route, mode, what, float((err / bound).max()))

    d = dspec.double()
    if got["math"] == "dense":
        check(got["spec"], basis @ fr, basis.abs() @ fr.abs(), win, "dft")
        check(got["dfr"], basis.t() @ d, basis.abs().t() @ d.abs(), 2 * bins, "dft_t")
    else:
        # the folded contraction as the plan defines it: the right half of the basis (window samples h + m) against E[m] = s[h+m] +
        # s[h-m] (real rows) and O[m] = s[h+m] - s[h-m] (imaginary rows) -- which equals basis @ frames only up to the float32 basis'
        # own (anti)symmetry, e.g. not on the Nyquist imaginary row, whose entries are sin(pi n) rounding residues
        w = basis[:, h:]
        m = torch.arange(1, h)
        e = torch.cat((fr[h:h + 1], fr[h + m] + fr[h - m]))
        o = torch.cat((torch.zeros_like(fr[:1]), fr[h + m] - fr[h - m]))
        a = torch.cat((fr[h:h + 1].abs(), fr[h + m].abs() + fr[h - m].abs()))   # also bounds the fp32 rounding of E and O
        check(got["spec"], torch.cat((w[:bins] @ e, w[bins:] @ o)), torch.cat((w[:bins].abs() @ a, w[bins:].abs() @ a)), h + 1, "dft")
        # [dE ; dO]: the real rows' and the imaginary rows' window samples h + m, m < h
        ref = torch.cat((w[:bins].t() @ d[:bins], w[bins:].t() @ d[bins:]))
        mag = torch.cat((w[:bins].abs().t() @ d[:bins].abs(), w[bins:].abs().t() @ d[bins:].abs()))
        check(got["dfr"], ref, mag, bins, "dft_t")


def test_mrstft_gradient_checks_cover_every_mode():
    """The conditioning filter of the module tests leaves a gradient assertion on most cases of every mode."""
    for mode in MODES:
        cases = [c for c in MCASES if c[0] != "edge"]
        checked = [c for c in cases if grad_bound(mode, _oracle(*c)[2]) is not None]
        assert len(checked) >= (0.9 if mode in FP32_GRADE else 0.6) * len(cases), (mode, len(checked), len(cases))
        assert {c[1][0] for c in checked if c[0] == "scaled"} >= {g for g in MGEOM if g[0] not in (1024, 4096)}, mode


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in MCASES if c[0] in ("single", "scaled", "nine")],
                         ids=[_mkey(*c) for c in MCASES if c[0] in ("single", "scaled", "nine")])
def test_mrstft_module_against_float64(module_results, case, mode):
    route, res = module_results
    got = res[(_mkey(*case), mode)]
    _check_module(got, *_oracle(*case), mode, (route, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in MCASES if c[0] == "edge"], ids=[_mkey(*c) for c in MCASES if c[0] == "edge"])
def test_mrstft_module_silent_and_identical_rows(module_results, case, mode, record_property):
    """Row 0 silent in x and y, row 1 silent in y only, row 2 with x == y bit for bit, row 3 ordinary.  float64 gives rows 0 and 2 a
    gradient of exactly 0 (the norm's and |.|'s subgradient at 0).  Row 2's device gradient is exactly 0 when its x and y spectra come
    out bit for bit equal on the device (the zero spectral distance takes no inf * 0 path); were they not, it would differ from 0 by the
    mode's noise and be held only by the L2 bound over the whole gradient."""
    route, res = module_results
    got = res[(_mkey(*case), mode)]
    ref_value, ref_grad, model = _oracle(*case)
    assert float(ref_grad[0].abs().max()) == 0.0 and float(ref_grad[2].abs().max()) == 0.0
    _check_module(got, ref_value, ref_grad, model, mode, (route, mode))
    grad = got["grad"]
    assert float(grad[0].abs().max()) == 0.0
    record_property("row2_spectra_bitwise_equal", got["spectra_equal"])
    if got["spectra_equal"]:
        assert float(grad[2].abs().max()) == 0.0
    else:
        warnings.warn(f"{route} {mode}: row 2's x and y spectra differ on the device; its zero gradient is held only in L2")


if __name__ == "__main__":
    {"kernels": _kernel_child, "module": _module_child}[sys.argv[1]](sys.argv[2])
