"""GPU: the per-clip test losses in ragged batches -- the row-sum kernels through ``ops`` against float64 torch on fenced, misaligned,
NaN-slacked buffers; ``MultiResolutionSTFTLoss.forward_ragged`` and ``DiscriminatorEBENMultiScales.forward_ragged`` against the float64
oracle of every row ALONE and against the same build's batch-1 call on that row; ``EBENLightningModule.evaluate_clips(losses=True)``
against the oracle and the loop of batch-1 ``test_step``.

Bars.  Kernels: rtol 1e-5 against float64 on the same float32 inputs, the bar ``test_feature_and_hinge_losses`` holds the batch kernels
to (every element adds a few float32 roundings of 2^-24 to sums of like-signed terms; logf adds about an ulp of |log m| <= 20).  MRSTFT
rows: the mode's loss rtol of tests/test_gpu_stft.py's MODE_TOL, and no further from the oracle than twice the batch-1 forward of the
row.  End to end: |v - f64| <= max(rtol |f64|, 2 |batch-1 - f64|) with rtol 2e-5 for the MRSTFT and 1e-5 for feature matching and the
hinge terms."""
import functools

import numpy as np
import pytest
import torch

from formula import formula_audio, formula_tensor
from oracle import eben_oracle as O
from tests import ragged_losses_oracle as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RAW = (4321, 3300, 3040, 2790, 2530)
CUT = (4320, 3296, 3040, 2784, 2528)
FENCE = 64
SENTINEL = 12345.0
STFT = dict(fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240))
STFT_RTOL = {"folded": 2e-5, "bf16x3": 5e-5}   # tests/test_gpu_stft.py MODE_TOL[mode][0]
E2E_RTOL = {"reconstructive_loss_freq": 2e-5, "feature_matching_loss": 1e-5, "adv_loss_gen": 1e-5, "real_loss": 1e-5, "fake_loss": 1e-5}
NETWORK = {"reconstructive_loss_freq": "generator", "feature_matching_loss": "generator", "adv_loss_gen": "generator",
           "real_loss": "discriminator", "fake_loss": "discriminator"}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # NaN == NaN


def fenced(shape, lens, tag, off=1):
    """A ``shape`` = (rows, channels, l_buf) view ``off`` floats off the 16-byte grid inside a fenced allocation: formula values in
    front of each row's end, NaN behind it.  Returns (host image, device allocation, view, float64 host body)."""
    rows, channels, l_buf = shape
    n = rows * channels * l_buf
    flat = torch.full((FENCE + off + n + FENCE,), SENTINEL, dtype=torch.float32)
    body = formula_tensor(tag, shape)
    for r, ln in enumerate(lens):
        body[r, :, max(min(ln, l_buf), 0):] = float("nan")
    flat[FENCE + off : FENCE + off + n] = body.reshape(-1)
    dev = flat.to(DEV)
    view = dev[FENCE + off : FENCE + off + n].view(shape)
    assert view.data_ptr() % 16 == 4 * off
    return flat, dev, view, body.double()


def table(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_off", [1, 3])   # b misaligned like a (16-byte loads behind a scalar head) / differently (the scalar loop)
def test_fm_sums_rows_against_float64(hip, b_off):
    from vibravox_amd import ops

    rows = 4
    shapes = [(1, 5001), (3, 5001), (24, 5001), (1, 37), (3, 37), (24, 37), (24, 4099)]   # 24 x 2 pieces > the 32 blocks of a row
    lens_of = {5001: (5001, 1, 4099, 2050), 37: (37, 1, 30, 7), 4099: (4096, 4099, 5, 4097)}
    pairs, held, want = [], [], []
    for i, (c, l_buf) in enumerate(shapes):
        lens = lens_of[l_buf]
        fa, da, va, a64 = fenced((rows, c, l_buf), lens, f"fmr/a{i}")
        fb, db, vb, b64 = fenced((rows, c, l_buf), lens, f"fmr/b{i}", off=b_off)
        pairs.append((va, vb, table(lens)))
        held.append((fa, da, fb, db))
        want.append([[float((a64[r, :, :n] - b64[r, :, :n]).abs().sum()), float(a64[r, :, :n].abs().sum())] for r, n in enumerate(lens)])
    got = ops.fm_sums_rows(pairs, rows)
    again = ops.fm_sums_rows(pairs, rows)
    torch.cuda.synchronize()
    assert got.shape == (len(shapes), rows, 2) and same_bits(got, again)
    np.testing.assert_allclose(got.double().cpu().numpy(), np.array(want), rtol=1e-5)
    for fa, da, fb, db in held:   # inputs and fences as they were
        assert same_bits(da.cpu(), fa) and same_bits(db.cpu(), fb)


def test_hinge_rows_against_float64(hip):
    from vibravox_amd import ops

    rows = 4
    terms, held, want = [], [], []
    for i, (l_buf, lens, target) in enumerate([(37, (37, 1, 30, 7), 1.0), (37, (37, 1, 30, 7), -1.0), (1501, (1501, 1, 1499, 258), 1.0),
                                                (1501, (1500, 257, 3, 1501), -1.0)]):
        fx, dx, vx, x64 = fenced((rows, 1, l_buf), lens, f"hinge_rows/{i}")
        terms.append((vx, target, table(lens)))
        held.append((fx, dx))
        want.append([float(torch.relu(1 - target * x64[r, 0, :n]).mean()) for r, n in enumerate(lens)])
    got = ops.hinge_rows(terms, rows)
    again = ops.hinge_rows(terms, rows)
    torch.cuda.synchronize()
    assert same_bits(got, again)
    np.testing.assert_allclose(got.double().cpu().numpy(), np.array(want), rtol=1e-5)
    for fx, dx in held:
        assert same_bits(dx.cpu(), fx)


def test_row_kernels_give_nan_for_lengths_out_of_range(hip):
    from vibravox_amd import ops

    rows, l_buf = 3, 37
    lens = (38, -1, 20)
    fa, da, va, a64 = fenced((rows, 3, l_buf), lens, "bad/a")
    fb, db, vb, b64 = fenced((rows, 3, l_buf), lens, "bad/b")
    sums = ops.fm_sums_rows([(va, vb, table(lens))], rows).cpu()
    hinge = ops.hinge_rows([(va[:, :1, :].contiguous(), 1.0, table(lens))], rows).cpu()
    assert torch.isnan(sums[0, :2]).all() and torch.isnan(hinge[0, :2]).all()
    np.testing.assert_allclose(float(sums[0, 2, 0]), float((a64[2, :, :20] - b64[2, :, :20]).abs().sum()), rtol=1e-5)
    assert torch.isfinite(hinge[0, 2])
    assert same_bits(da.cpu(), fa) and same_bits(db.cpu(), fb)


@pytest.mark.parametrize("n_fft,hop,win", [(512, 50, 240), (511, 50, 241)])
def test_stft_loss_sums_rows_against_float64(hip, n_fft, hop, win):
    from vibravox_amd import stft
    from vibravox_amd._lib import check, stream
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    rows, t, eps = 4, 2000, 1e-8
    loss = MultiResolutionSTFTLoss(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,)).to(DEV)
    (p,) = loss._build_plans()
    frames = p.frames(t)
    sig = torch.cat([formula_audio(f"sums_rows/{n_fft}/{i}", 1, t) for i in range(2 * rows)]).to(DEV)
    spec = stft._stft_spectrum(p, p.math_for("folded"), sig, t, frames)   # (1, 2 bins, 2 rows frames): x rows, then y rows
    of_row = (frames, 1, frames - 1, 17)
    sums = torch.empty((rows, 3), dtype=torch.float32, device=DEV)
    nbytes = hip.eben_stft_loss_sums_rows_workspace(rows)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    cols = 2 * rows * frames
    check(hip.eben_stft_loss_sums_rows(spec.data_ptr(), spec.data_ptr() + 4 * rows * frames, rows, p.bins, frames, table(of_row).data_ptr(), frames,
                                       cols, p.bins * cols, eps, ws.data_ptr(), nbytes, sums.data_ptr(), stream()), "stft_loss_sums_rows")
    s = spec.double().cpu().reshape(2, p.bins, 2, rows, frames)   # (re / im, bin, x / y, row, frame)
    mag = torch.sqrt(torch.clamp(s[0] ** 2 + s[1] ** 2, min=eps))
    want = []
    for r, f in enumerate(of_row):
        xm, ym = mag[:, 0, r, :f], mag[:, 1, r, :f]
        want.append([float(((ym - xm) ** 2).sum()), float((ym ** 2).sum()), float((torch.log(xm) - torch.log(ym)).abs().sum())])
    np.testing.assert_allclose(sums.double().cpu().numpy(), np.array(want), rtol=1e-5)
    full = torch.empty((rows, 3), dtype=torch.float32, device=DEV)
    check(hip.eben_stft_loss_sums_ex(spec.data_ptr(), spec.data_ptr() + 4 * rows * frames, rows, p.bins, frames, frames, cols, p.bins * cols, eps,
                                     ws.data_ptr(), nbytes, full.data_ptr(), stream()), "stft_loss_sums")
    assert same_bits(sums[0], full[0])   # a full row walks the same elements in the same order as eben_stft_loss_sums_ex


# ---- MultiResolutionSTFTLoss.forward_ragged ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stft_case(weighting):
    """The five pairs, packed (zero behind every row), and per row the float64 oracle of the row alone (computed once)."""
    from vibravox_amd.torch_modules.losses.mrstft_loss import a_weighting_taps

    x = [formula_audio(f"rl/stft/x{i}", 1, t) for i, t in enumerate(CUT)]
    y = [formula_audio(f"rl/stft/y{i}", 1, t) for i, t in enumerate(CUT)]
    l_buf = max(CUT) + 1280
    px, py = torch.zeros((len(CUT), 1, l_buf)), torch.zeros((len(CUT), 1, l_buf))
    for r, t in enumerate(CUT):
        px[r, 0, :t], py[r, 0, :t] = x[r][0, 0], y[r][0, 0]
    fir = a_weighting_taps(16000).double() if weighting else None
    ref = [float(O.mrstft_loss(a.double(), b.double(), perceptual_weighting=weighting, fir=fir, **STFT)) for a, b in zip(x, y)]
    return x, y, px.to(DEV), py.to(DEV), ref


@pytest.mark.parametrize("mode", ["folded", "bf16x3"])
@pytest.mark.parametrize("weighting", [True, False])
def test_mrstft_forward_ragged_gives_every_row_its_own_loss(hip, weighting, mode):
    from vibravox_amd import stft
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    x, y, px, py, ref = stft_case(weighting)
    loss = MultiResolutionSTFTLoss(sample_rate=16000, perceptual_weighting=weighting, **STFT).to(DEV)
    loss.stft_math = mode
    got = loss.forward_ragged(px, py, CUT)
    assert got.shape == (len(CUT),) and got.dtype is torch.float32 and not got.requires_grad

    def garbage(sig, lens2):   # behind the rows of the filtered copy, in front of the mirror fill
        for r, t in enumerate(CUT + CUT):
            sig[r, :, t:] = float("nan")

    stft.mrstft_rows_probe = garbage
    try:
        poisoned = loss.forward_ragged(px, py, CUT)
    finally:
        stft.mrstft_rows_probe = None
    assert same_bits(poisoned, got)
    with torch.no_grad():
        alone = [float(loss(a.to(DEV), b.to(DEV))) for a, b in zip(x, y)]
    for r, (v, b1, f64) in enumerate(zip(got.tolist(), alone, ref)):
        print(f"[mrstft rows {mode} aw={weighting}] row {r}: ragged {v:.8g} batch-1 {b1:.8g} f64 {f64:.10g} | err {abs(v - f64):.2e} vs {abs(b1 - f64):.2e}")
    for r, (v, b1, f64) in enumerate(zip(got.tolist(), alone, ref)):
        assert abs(v - f64) <= STFT_RTOL[mode] * abs(f64), (r, v, f64)
        assert abs(v - f64) <= 2 * abs(b1 - f64), (r, v, b1, f64)


def test_mrstft_forward_ragged_refusals(hip):
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    _, _, px, py, _ = stft_case(False)
    loss = MultiResolutionSTFTLoss(**STFT).to(DEV)
    with pytest.raises(RuntimeError, match="no backward"):
        loss.forward_ragged(px.clone().requires_grad_(True), py, CUT)
    with pytest.raises(ValueError, match="clip 3 "):
        loss.forward_ragged(px, py, CUT[:3] + (600, CUT[4]))   # the largest reflect pad is 600: 601 samples at least
    with pytest.raises(ValueError, match="clip 0 "):
        loss.forward_ragged(px[:, :, :4400].contiguous(), py[:, :, :4400].contiguous(), CUT)   # 80 samples of slack behind row 0
    with pytest.raises(NotImplementedError, match="w_lin_mag=1.0"):
        MultiResolutionSTFTLoss(w_lin_mag=1.0, **STFT).to(DEV).forward_ragged(px, py, CUT)
    with pytest.raises(NotImplementedError, match="scale='mel'"):
        MultiResolutionSTFTLoss(scale="mel", n_bins=64, sample_rate=16000, **STFT).to(DEV).forward_ragged(px, py, CUT)


# ---- the discriminators' ragged forward -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def networks():
    """Generator and discriminator from a fixed seed, on the device, with their float64 oracle state dicts."""
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    torch.manual_seed(20)
    gen, disc = EBENGenerator(m=4, n=32, p=2), DiscriminatorEBENMultiScales(q=3, min_channels=24)
    g_sd = {k: v.detach().double() for k, v in gen.state_dict().items()}
    d_sd = {k: v.detach().double() for k, v in disc.state_dict().items()}
    return gen.to(DEV), disc.to(DEV), g_sd, d_sd


def test_discriminator_forward_ragged_gives_every_row_its_own_embeddings(hip, record_property):
    from vibravox_amd import ragged

    _, disc, _, d_sd = networks()
    band_lengths = tuple((t + 32) // 4 for t in CUT)
    plan = ragged.disc_plan(disc, CUT, band_lengths)
    assert plan.audio_l_buf == 5600 and plan.bands_l_buf == 1152
    rows = len(CUT)
    audio = torch.full((rows, 1, plan.audio_l_buf), float("nan"))
    bands = torch.full((rows, 4, plan.bands_l_buf), float("nan"))
    for r, (t, l0) in enumerate(zip(CUT, band_lengths)):
        audio[r, 0, :t] = formula_audio(f"rl/disc/a{r}", 1, t)[0, 0]
        bands[r, :, :l0] = formula_tensor(f"rl/disc/b{r}", (4, l0))
    audio_dev, bands_dev = audio.to(DEV), bands.to(DEV)
    emb, lens = disc.forward_ragged(bands_dev, audio_dev, plan)
    assert same_bits(audio_dev.cpu(), audio) and same_bits(bands_dev.cpu(), bands)   # the caller's buffers, bit for bit
    assert [len(chain) for chain in emb] == [9, 9, 9, 8]
    for c in range(4):
        assert lens[c].dtype is torch.int32 and lens[c].is_cuda and lens[c].cpu().tolist() == [list(level) for level in plan.lengths(c)]
    bit_equal = True
    for r, (t, l0) in enumerate(zip(CUT, band_lengths)):
        a, b = audio[r : r + 1, :, :t], bands[r : r + 1, :, :l0]
        want = O.discriminator_forward(d_sd, b.double(), a.double(), 3)
        with torch.no_grad():
            alone = disc(b.to(DEV).contiguous(), a.to(DEV).contiguous())
        for c in range(4):
            for lv, (e, w, b1) in enumerate(zip(emb[c], want[c], alone[c])):
                n = plan.lengths(c)[lv][r]
                assert w.shape[2] == n == b1.shape[2], (c, lv, r)
                mine = e[r : r + 1, :, :n]
                err, err1 = float((mine.double().cpu() - w).abs().max()), float((b1.double().cpu() - w).abs().max())
                assert torch.isfinite(mine).all() and err <= 2 * err1, (r, c, lv, err, err1)
                bit_equal = bit_equal and same_bits(mine, b1)
    print(f"[disc forward_ragged] every row bit-equal to its batch-1 forward: {bit_equal}")
    record_property("rows_bit_equal_to_batch1", bit_equal)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _module(feature_matching=True):
    from functools import partial

    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    gen, disc, _, _ = networks()
    opt = partial(FusedAdam, lr=3e-4)
    return EBENLightningModule(sample_rate=16000, generator=gen, discriminator=disc, generator_optimizer=opt, discriminator_optimizer=opt,
                               reconstructive_loss_freq_fn=MultiResolutionSTFTLoss(sample_rate=16000, perceptual_weighting=True, **STFT).to(DEV),
                               feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales() if feature_matching else None,
                               adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales())


@functools.lru_cache(maxsize=None)
def pairs():
    """The five pairs and per clip the float64 oracle's five terms of the clip alone (computed once)."""
    from vibravox_amd.torch_modules.losses.mrstft_loss import a_weighting_taps

    _, _, g_sd, d_sd = networks()
    cor = [formula_audio(f"rl/e2e/bc{i}", 1, t) for i, t in enumerate(RAW)]
    ref = [formula_audio(f"rl/e2e/air{i}", 1, t) for i, t in enumerate(RAW)]
    fir, ana = a_weighting_taps(16000).double(), g_sd["pqmf.analysis_weights"]
    oracle = []
    for c, g in zip(cor, ref):
        enh, bands = O.generator_forward(g_sd, O.cut_to_valid_length(c.double()), 2)
        g64 = O.cut_to_valid_length(g.double())
        oracle.append({k: float(v) for k, v in L.clip_losses_alone(d_sd, 3, enh, g64, bands, O.pqmf_analysis(g64, ana), fir=fir, **STFT).items()})
    return [c.to(DEV) for c in cor], [g.to(DEV) for g in ref], oracle


def test_module_evaluate_clips_with_losses_against_the_batch1_loop(hip):
    from vibravox_amd import ragged

    mod = _module()
    cor, ref, oracle = pairs()
    margin = ragged.loss_margin(mod.discriminator, 4, mod.reconstructive_loss_freq_fn)
    budget = 3 * (CUT[1] + margin)
    assert margin == 1280 and len(ragged.compose_batches(mod.generator, RAW, budget, margin)[0]) == 2
    out = mod.evaluate_clips(cor, ref, max_batch_samples=budget, losses=True)
    keys = {f"{NETWORK[name]}/{name}" for name in NETWORK}
    assert set(out) == {"si_sdr", "stoi"} | keys
    assert set(mod.logged) == {"test/torchmetrics_si_sdr", "test/torchmetrics_stoi"} | {f"test/{k}" for k in keys}
    for k in keys:
        assert out[k].shape == (5,) and out[k].dtype is torch.float32 and out[k].is_cuda
        assert abs(float(mod.logged[f"test/{k}"]) - float(out[k].double().mean())) <= 1e-6 * abs(float(out[k].double().mean()))
    loop = []
    for c, g in zip(cor, ref):
        mod.logged.clear()
        mod.test_step({"audio_body_conducted": c, "audio_airborne": g})
        loop.append({name: float(mod.logged[f"test/{NETWORK[name]}/{name}"]) for name in NETWORK})
    worst = {}
    for i in range(5):
        for name in NETWORK:
            v, b1, f64 = float(out[f"{NETWORK[name]}/{name}"][i]), loop[i][name], oracle[i][name]
            print(f"[evaluate_clips losses] clip {i} {name}: ragged {v:.8g} batch-1 {b1:.8g} f64 {f64:.10g} | err {abs(v - f64):.2e} vs {abs(b1 - f64):.2e}")
            worst[name] = max(worst.get(name, 0.0), abs(v - f64) / abs(f64))
    print(f"[evaluate_clips losses] worst relative error against float64: {worst}")
    for i in range(5):
        for name in NETWORK:
            v, b1, f64 = float(out[f"{NETWORK[name]}/{name}"][i]), loop[i][name], oracle[i][name]
            assert abs(v - f64) <= max(E2E_RTOL[name] * abs(f64), 2 * abs(b1 - f64)), (i, name, v, b1, f64)


def test_module_evaluate_clips_without_losses_is_what_it_was(hip):
    mod = _module()
    cor, ref, _ = pairs()
    out = mod.evaluate_clips(cor, ref)
    assert set(out) == {"si_sdr", "stoi"} and set(mod.logged) == {"test/torchmetrics_si_sdr", "test/torchmetrics_stoi"}


def test_no_feature_matching_fn_no_feature_matching_sums(hip, monkeypatch):
    from vibravox_amd import ops

    def refuse(*args, **kwargs):
        raise AssertionError("feature-matching sums without a feature-matching loss")

    monkeypatch.setattr(ops, "fm_sums_rows", refuse)
    mod = _module(feature_matching=False)
    cor, ref, oracle = pairs()
    out = mod.evaluate_clips(cor, ref, losses=True)
    assert set(out) == {"si_sdr", "stoi", "generator/reconstructive_loss_freq", "generator/adv_loss_gen", "discriminator/real_loss",
                        "discriminator/fake_loss"}
    assert "test/generator/feature_matching_loss" not in mod.logged and "test/discriminator/fake_loss" in mod.logged
    for i in range(5):   # one batch here, two above: the same values either way, to the end-to-end bar's rtol
        assert abs(float(out["discriminator/real_loss"][i]) - oracle[i]["real_loss"]) <= 1e-4 * abs(oracle[i]["real_loss"])


def test_short_clip_is_refused_before_anything_runs(hip):
    from vibravox_amd import inference

    mod = _module()
    cor, ref, _ = pairs()
    short = formula_audio("rl/e2e/short", 1, 2300).to(DEV)   # cut 2272: 576 band samples, the dilation-3 chain needs 631
    with pytest.raises(ValueError, match=r"clip 2 .*dilation 3"):
        mod.evaluate_clips(cor[:2] + [short], ref[:2] + [short], losses=True)
    assert not mod.logged
    assert set(mod.evaluate_clips(cor[:2] + [short], ref[:2] + [short])) == {"si_sdr", "stoi"}   # the metrics alone take it
    with pytest.raises(ValueError, match="MultiResolutionSTFTLoss"):
        inference.LossTerms(discriminator=mod.discriminator, freq_loss=torch.nn.L1Loss())
    terms = inference.LossTerms(discriminator=mod.discriminator, time_loss=torch.nn.L1Loss())
    out = inference.evaluate_clips(mod.generator, cor[:2], ref[:2], loss_terms=terms, return_enhanced=True)
    assert set(out) == {"si_sdr", "stoi", "enhanced", "generator/reconstructive_loss_temp"}
    for i in range(2):
        want = torch.nn.functional.l1_loss(out["enhanced"][i], ref[i][:, :, : CUT[i]])
        assert abs(float(out["generator/reconstructive_loss_temp"][i]) - float(want)) <= 1e-6 * float(want)
