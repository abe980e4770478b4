"""GPU: recordings to resident clips -- the two kernels of ``csrc/corpus.hip`` (``corpus.pcm_to_rows``), ``ResidentCorpus.load``, the
local datamodules and two training steps on their batches.

One oracle throughout: the numpy conversion of a file's samples (``tests/corpus_fixtures.oracle``: each conversion is exact), and for a
file at another rate ``augment.resample`` of that decoded clip alone.  Every comparison is ``torch.equal``."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import corpus_fixtures as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = 12345.0
FORMATS = ("PCM16", "PCM24", "PCM32", "FLOAT32")


def pack(items, channel_of=lambda x: x.shape[1] - 1):
    """``items``: (samples (frames, channels), fmt).  Returns the byte buffer on the device -- every chunk at a 16-byte boundary, 0xA5
    between and behind the chunks, which no conversion turns into zero -- and the descriptor table, taking every file's last channel."""
    from vibravox_amd import corpus

    rows = np.zeros(len(items), dtype=corpus.ROW_DTYPE)
    blob = bytearray()
    for r, (x, fmt) in enumerate(items):
        blob += b"\xa5" * (-len(blob) % 16)
        rows[r] = (len(blob), x.shape[0], x.shape[1], channel_of(x), FORMATS.index(fmt))
        blob += F.encode(x, fmt)
    blob += b"\xa5" * (32 + -len(blob) % 16)
    return torch.frombuffer(blob, dtype=torch.uint8).to(DEV), rows


def flat_store(lengths, gap=3):
    """A 1-D store of sentinels with rows of ``lengths`` placed ``gap`` floats apart, 1 float off the 16-byte grid: (store, offsets)."""
    offsets, at = [], 1 + gap
    for n in lengths:
        offsets.append(at)
        at += n + gap
    return torch.full((at + 1,), SENTINEL, dtype=torch.float32, device=DEV), offsets


def check_flat(store, offsets, wants):
    got = store.cpu()
    keep = torch.ones(got.numel(), dtype=torch.bool)
    for off, w in zip(offsets, wants):
        assert torch.equal(got[off:off + w.numel()], w.cpu()), off
        keep[off:off + w.numel()] = False
    assert bool((got[keep] == SENTINEL).all())   # the float before a row's first and after its last, and everything else, untouched


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_equals_the_numpy_conversion(hip, fmt, channels):
    from vibravox_amd import corpus

    frames = [1, 2, 7, 8, 9, 4097]
    items = [(F.samples(fmt, n, channels, 10 * n + channels), fmt) for n in frames]
    data, rows = pack(items)
    wants = [torch.from_numpy(F.oracle(x, fmt, channels - 1)) for x, _ in items]
    for pitch in (4097, 4110):
        out = torch.full((len(frames), pitch), float("nan"), dtype=torch.float32, device=DEV)
        got, lens = corpus.pcm_to_rows(data, rows, out=out, pitch=pitch)
        assert got is out and lens.dtype is torch.int32 and lens.tolist() == frames
        for r, w in enumerate(wants):
            assert torch.equal(got[r, :frames[r]].cpu(), w), (r, pitch)
            assert bool((got[r, frames[r]:] == 0).all()), (r, pitch)          # exact zeros behind lens[r]
    store, offsets = flat_store(frames)
    corpus.pcm_to_rows(data, rows, offsets=offsets, out=store)
    check_flat(store, offsets, wants)


def test_decode_takes_any_channel_and_skips_empty_rows(hip):
    from vibravox_amd import corpus

    x = F.samples("PCM16", 2500, 3, 3)
    items = [(x, "PCM16")] * 3 + [(x[:0], "PCM16")]
    data, rows = pack(items)
    rows["channel"][:3] = [0, 1, 2]
    rows["channel"][3] = 0
    got, lens = corpus.pcm_to_rows(data, rows)
    assert lens.tolist() == [2500, 2500, 2500, 0] and bool((got[3] == 0).all())
    for c in range(3):
        assert torch.equal(got[c].cpu(), torch.from_numpy(F.oracle(x, "PCM16", c)))


# ---- fused resample ---------------------------------------------------------------------------------------------------------------------
RATIOS = [(48000, 16000), (44100, 16000), (8000, 16000)]   # 3:1, 441:160, 1:2
LAYOUTS = [("PCM16", 1), ("PCM16", 2), ("PCM24", 1), ("PCM32", 3), ("FLOAT32", 2)]   # the 16-byte-load path first, then every plainer one


def fused_lengths(freqs):
    from vibravox_amd import rate

    orig, new, width = rate.ratio(*freqs)
    tile = rate.tile(orig, new, width)
    assert (tile["outputs_per_block"] * orig) % new == 0
    span = tile["outputs_per_block"] * orig // new     # input samples whose outputs fill one block's tile exactly
    return [1, width - 1, width, width + orig, span - 1, span, span + 1, 3 * span + 5]


@functools.lru_cache(maxsize=None)
def fused_case(freqs, layout):
    """The rows of one (ratio, layout), packed, and per row ``augment.resample`` of the numpy-decoded clip alone (computed once)."""
    from vibravox_amd import augment

    fmt, channels = layout
    items = [(F.samples(fmt, n, channels, n + channels), fmt) for n in fused_lengths(freqs)]
    data, rows = pack(items)
    wants = [augment.resample(torch.from_numpy(F.oracle(x, fmt, channels - 1)).to(DEV), *freqs) for x, _ in items]
    return data, rows, wants


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("freqs", RATIOS, ids=lambda v: f"{v[0]}to{v[1]}")
def test_fused_resample_equals_resample_of_the_decoded_clip(hip, freqs, layout):
    from vibravox_amd import corpus, rate

    data, rows, wants = fused_case(freqs, layout)
    counts = [rate.resampled_length(int(n), *freqs) for n in rows["frames"]]
    assert counts == [w.numel() for w in wants]
    for slack in (0, 13):
        pitch = max(counts) + slack
        out = torch.full((len(counts), pitch), float("nan"), dtype=torch.float32, device=DEV)
        got, lens = corpus.pcm_to_rows(data, rows, rates=freqs, out=out, pitch=pitch)
        assert lens.tolist() == counts
        for r, w in enumerate(wants):
            assert torch.equal(got[r, :counts[r]], w), (r, slack)
            assert bool((got[r, counts[r]:] == 0).all()), (r, slack)
    store, offsets = flat_store(counts)
    corpus.pcm_to_rows(data, rows, rates=freqs, offsets=offsets, out=store)
    check_flat(store, offsets, wants)


def test_fused_resample_equals_the_two_launches_it_replaces(hip):
    from vibravox_amd import corpus, rate

    freqs = (48000, 16000)
    data, rows, wants = fused_case(freqs, ("PCM16", 1))
    decoded, lens = corpus.pcm_to_rows(data, rows)
    two, two_lens = rate.resample_ragged(decoded, lens, *freqs)
    one, one_lens = corpus.pcm_to_rows(data, rows, rates=freqs)
    assert torch.equal(one, two) and torch.equal(one_lens, two_lens)


# ---- ResidentCorpus.load ----------------------------------------------------------------------------------------------------------------
def write_split(root, subset, split, sensors, specs, seed=0):
    """specs: [(stem, fmt, frames, rate, channels)]; every sensor gets its own content.  Returns {sensor: {stem: (samples, fmt, rate)}}."""
    made = {}
    for s_i, sensor in enumerate(sensors):
        made[sensor] = {}
        for k, (stem, fmt, frames, rate, channels) in enumerate(specs):
            x = F.samples(fmt, frames, channels, seed + 100 * s_i + k)
            if fmt != "FLOAT32":   # a tenth of full scale: losses and metrics then see levels a recording has
                x = x // 10
            else:
                x = (x * np.float32(0.1)).astype(np.float32)
            F.write_wav(os.path.join(root, subset, split, sensor, stem + ".wav"), x, fmt, rate)
            made[sensor][stem] = (x, fmt, rate)
    return made


def oracle_clip(entry, sample_rate=16000):
    from vibravox_amd import augment

    x, fmt, rate = entry
    clip = torch.from_numpy(F.oracle(x, fmt, 0)).to(DEV)
    return clip if rate == sample_rate else augment.resample(clip, rate, sample_rate)


def test_load_fills_the_store_in_groups(hip, tmp_path):
    from vibravox_amd import corpus

    specs = [(f"u{k:02d}", FORMATS[k % 4], 900 + 517 * k, (16000, 48000)[(k // 2) % 2], 1 + k % 2) for k in range(12)]
    sensors = ["headset_microphone", "throat_microphone"]
    made = write_split(tmp_path, "speech_clean", "train", sensors, specs)
    sizes = [corpus.wav_info(os.path.join(tmp_path, "speech_clean", "train", s, st[0] + ".wav")).data_bytes for s in sensors for st in specs]
    budget = 2 * max(corpus._group_bytes(1, corpus._up(b)) for b in sizes)   # the smallest staging whose halves take exactly three groups
    while len(corpus.plan_groups(sizes, budget // 2)) > 3:
        budget += 2048
    assert len(corpus.plan_groups(sizes, budget // 2)) == 3
    c = corpus.ResidentCorpus.load(tmp_path, "speech_clean", "train", sensors, 16000, DEV, max_stage_bytes=budget)
    torch.cuda.synchronize()   # the only wait: load itself left none behind
    assert c.stems == [s[0] for s in specs] and len(c) == 12 and c.roles == sensors
    assert c.lengths == [n if r == 16000 else -(-n // 3) for _, _, n, r, _ in specs]
    for sensor in sensors:
        assert c.store[sensor].shape == (sum(c.lengths),)
        for i, stem in enumerate(c.stems):
            assert torch.equal(c.clip(i, sensor), oracle_clip(made[sensor][stem])), (sensor, stem)
        assert [v.data_ptr() for v in c.clips(sensor)] == [c.store[sensor].data_ptr() + 4 * o for o in c.offsets[:-1]]   # views, no copies
    one = corpus.ResidentCorpus.load(tmp_path, "speech_clean", "train", sensors, 16000, DEV)   # everything in one group
    assert all(torch.equal(one.store[s], c.store[s]) for s in sensors)


# ---- loaders ----------------------------------------------------------------------------------------------------------------------------
SENSOR = "throat_microphone"
SPEECH = [("a", "PCM16", 3000, 16000, 1), ("b", "PCM16", 36000, 48000, 1), ("c", "PCM24", 7999, 16000, 1), ("d", "FLOAT32", 8001, 16000, 2),
          ("e", "PCM32", 20000, 16000, 1), ("f", "PCM16", 9000, 16000, 1)]          # at 16 kHz: shorter and longer than 500 ms = 8000 samples
NOISE = [("n0", "PCM16", 30000, 16000, 1), ("n1", "PCM16", 96000, 48000, 1), ("n2", "FLOAT32", 25000, 16000, 1)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("corpus")
    made = {}
    for split, seed in (("train", 0), ("validation", 1000), ("test", 2000)):
        made["speech_clean", split] = write_split(root, "speech_clean", split, ["headset_microphone", SENSOR], SPEECH, seed)
        made["speechless_noisy", split] = write_split(root, "speechless_noisy", split, [SENSOR], NOISE, seed + 500)
        made["speech_noisy", split] = write_split(root, "speech_noisy", split, [SENSOR], SPEECH[:3], seed + 700)
    second = tmp_path_factory.mktemp("corpus2")
    for split, seed in (("validation", 3000), ("test", 4000)):
        made["second", split] = write_split(second, "speech_clean", split, ["headset_microphone", SENSOR], SPEECH[:2], seed)
    return root, second, made


def oracle_items(made, stems=None):
    body, air = made[SENSOR], made["headset_microphone"]
    return [{"audio_body_conducted": oracle_clip(body[s]), "audio_airborne": oracle_clip(air[s])} for s in (stems or sorted(body))]


def same_batch(got, want):
    return got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("config", ["constant_length", "pad_time_masking"])
def test_train_batches_equal_the_collator_on_host_decoded_clips(hip, tree, config):
    from vibravox_amd import augment, collate
    from vibravox_amd.lightning_datamodules import LocalBWEDataModule

    root, _, made = tree
    if config == "constant_length":
        strategy, aug = "constant_length-500-ms", lambda: augment.WaveformDataAugmentation(16000)
    else:
        strategy, aug = "pad", lambda: augment.WaveformDataAugmentation(16000, p_data_augmentation=1, p_speed_perturbation=0, p_pitch_shift=0,
                                                                         p_time_masking=1)
    dm = LocalBWEDataModule(16000, root=root, sensor=SENSOR, collate_strategy=strategy, data_augmentation=aug(), batch_size=4, device=DEV)
    dm.setup("fit")
    loader = dm.train_dataloader()
    assert len(loader) == 2
    torch.manual_seed(11)
    got = list(loader)
    items, direct_aug = oracle_items(made["speech_clean", "train"]), aug()
    torch.manual_seed(11)
    want = [collate.bwe_collate(items[lo:lo + 4], 16000, strategy, False, direct_aug) for lo in (0, 4)]
    assert len(got) == 2 and all(same_batch(g, w) for g, w in zip(got, want))
    assert got[0]["audio_body_conducted"].shape == (4, 1, 8000 if config == "constant_length" else 12000)
    assert len(list(loader)) == 2                                        # re-iterable: a second epoch


def test_eval_batches_are_centre_crops_and_the_secondary_root_yields_the_dict(hip, tree):
    from vibravox_amd import collate
    from vibravox_amd.lightning_datamodules import LocalBWEDataModule

    root, second, made = tree
    dm = LocalBWEDataModule(16000, root=root, root_secondary=second, sensor=SENSOR, collate_strategy="constant_length-500-ms", batch_size=8, device=DEV)
    dm.setup("fit")
    dm.setup("test")
    for split, loaders in (("validation", dm.val_dataloader()), ("test", dm.test_dataloader())):
        assert set(loaders) == {"principal", "secondary"}
        for which, key, n in (("principal", ("speech_clean", split), 6), ("secondary", ("second", split), 2)):
            items = oracle_items(made[key])
            got = list(loaders[which])
            assert len(got) == len(loaders[which]) == n                  # min(1, 8 // 4) = 1 and 1: batches of one
            for g, item in zip(got, items):
                assert same_batch(g, collate.bwe_collate([item], 16000, "constant_length-500-ms", True, None))
        long = oracle_items(made["speech_clean", split], ["e"])[0]["audio_airborne"]     # 20000 samples: the centre 8000
        assert torch.equal(list(loaders["principal"])[4]["audio_airborne"][0, 0], long[6000:14000])
    single = LocalBWEDataModule(16000, root=root, sensor=SENSOR, batch_size=8, device=DEV)
    single.setup("test")
    assert not isinstance(single.test_dataloader(), dict)
    with pytest.raises(RuntimeError, match="setup"):
        single.train_dataloader()


@pytest.mark.parametrize("snr_range", [None, (0, 10)])
def test_noisy_batches_equal_the_collator_on_host_decoded_clips(hip, tree, snr_range):
    from vibravox_amd import collate
    from vibravox_amd.lightning_datamodules import LocalNoisyBWEDataModule

    root, _, made = tree
    dm = LocalNoisyBWEDataModule(16000, root=root, sensor=SENSOR, collate_strategy="constant_length-500-ms", batch_size=4, snr_range=snr_range, device=DEV)
    dm.setup("fit")
    noise = [oracle_clip(made["speechless_noisy", "train"][SENSOR][s]) for s in sorted(made["speechless_noisy", "train"][SENSOR])]
    items = oracle_items(made["speech_clean", "train"])
    torch.manual_seed(23)
    got = list(dm.train_dataloader())
    torch.manual_seed(23)
    want = []
    for lo in (0, 4):
        batch = [dict(item, audio_body_conducted_speechless_noisy=noise[int(torch.randint(0, len(noise), (1,)))]) for item in items[lo:lo + 4]]
        want.append(collate.noisy_bwe_collate(batch, 16000, "constant_length-500-ms", False, snr_range, dm.data_augmentation))
    assert len(got) == 2 and all(same_batch(g, w) for g, w in zip(got, want))
    val = dm.val_dataloader()
    assert set(val) == {"synthetic", "real"} and len(val["synthetic"]) == 6 and len(val["real"]) == 3
    real = [oracle_clip(made["speech_noisy", "validation"][SENSOR][s]) for s in ("a", "b", "c")]
    for g, clip in zip(val["real"], real):
        assert set(g) == {"audio_body_conducted"} and torch.equal(g["audio_body_conducted"][0, 0], clip)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_two_training_steps_and_a_test_split_from_files(hip, tree, tmp_path):
    from functools import partial

    from vibravox_amd.inference import evaluate_clips
    from vibravox_amd.lightning_datamodules import LocalBWEDataModule
    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator
    from vibravox_amd.torch_modules.losses.feature_loss import FeatureLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.hinge_loss import HingeLossForDiscriminatorMelganMultiScales
    from vibravox_amd.torch_modules.losses.mrstft_loss import MultiResolutionSTFTLoss

    root, _, made = tree
    torch.manual_seed(3)
    opt = partial(FusedAdam, lr=3e-4, betas=(0.5, 0.9))
    mod = EBENLightningModule(
        sample_rate=16000, generator=EBENGenerator(m=4, n=32, p=2).to(DEV), discriminator=DiscriminatorEBENMultiScales(q=4, min_channels=24).to(DEV),
        generator_optimizer=opt, discriminator_optimizer=opt,
        reconstructive_loss_freq_fn=MultiResolutionSTFTLoss(fft_sizes=(512, 1024, 2048), hop_sizes=(50, 120, 240), win_lengths=(240, 600, 1200),
                                                            sample_rate=16000, perceptual_weighting=True).to(DEV),
        feature_matching_loss_fn=FeatureLossForDiscriminatorMelganMultiScales(), adversarial_loss_fn=HingeLossForDiscriminatorMelganMultiScales(),
        dynamic_loss_balancing="ema")
    dm = LocalBWEDataModule(16000, root=root, sensor=SENSOR, collate_strategy="constant_length-500-ms", batch_size=2, device=DEV)
    dm.setup("fit")
    steps = 0
    for step, batch in zip(range(2), dm.train_dataloader()):
        assert batch["audio_body_conducted"].shape == (2, 1, 8000)
        mod.training_step(batch, step)
        assert mod.logged and all(bool(torch.isfinite(v).all()) for v in mod.logged.values()), mod.logged
        steps += 1
    assert steps == 2
    three = [("p", "PCM16", 36000, 48000, 1), ("q", "PCM24", 20000, 16000, 1), ("r", "FLOAT32", 9000, 16000, 2)]   # 0.75 s, 1.25 s, 0.56 s
    pairs = write_split(tmp_path, "speech_clean", "test", ["headset_microphone", SENSOR], three, 9000)
    dm3 = LocalBWEDataModule(16000, root=tmp_path, sensor=SENSOR, batch_size=2, device=DEV)
    dm3.setup("test")
    got = mod.evaluate_clips(*dm3.test_clips())
    items = oracle_items(pairs)
    want = evaluate_clips(mod.generator, [i["audio_body_conducted"] for i in items], [i["audio_airborne"] for i in items])
    for name in ("si_sdr", "stoi"):
        assert got[name].shape == (3,) and torch.equal(got[name], want[name]) and bool(torch.isfinite(got[name]).all()), name
