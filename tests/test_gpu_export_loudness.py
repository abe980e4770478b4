"""GPU: the loudness-normalised export.  ``eben_pcm_encode_ragged_gain`` against ``eben_pcm_encode_ragged`` (bytes), then
``inference.enhance_to_pcm(loudness=)`` and ``export.enhance_corpus(loudness=)`` against the same steps taken one after the other:
``enhance_clips``, ``metrics.loudness_gain``, ``corpus.rows_to_pcm`` on the scaled rows.  Every comparison of files is on bytes.

The level of a written file.  A PCM32 file read back holds, per sample, ``x * g`` after three roundings of relative size 2^-24 each -- the
gain to float32, the product to float32, the decoder's int32 to float32 -- (the 2^-32 step of the format itself is below them for every
sample above 2^-8 and negligible against the signal's rms below).  However the three errors line up, the weighted signal moves by at most
``3 * 2^-24 * 1.585 * |x|`` (1.585: the K-weighting's largest gain, its 4 dB shelf), so with a weighted rms of no less than a tenth of
the plain rms (asserted on every clip) the loudness moves by at most ``20 log10(1 + 3 * 2^-24 * 15.85) = 2.5e-5 LU``; measuring the
file adds one float32 ulp of the result (1.9e-6 at -23) and so does the reported level: ``FILE_BAR = 3e-5 LU``.
[MI355X] observed (``test_enhance_to_pcm_normalises_in_the_encode_launch`` prints it with -s): largest |L(file) - expected| 0.0 LU over
the 5 files with a loudness, all at the target (every file read back measures the float32 -23.0 exactly); the sixth has no block."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import corpus_fixtures as F
from tests import export_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
IN, MODEL = 48000, 16000
FILL = 0xA5
FILE_BAR = 3e-5
SPECIAL = np.array([1.0, -1.0, np.inf, -np.inf, np.nan, -0.0, 1e-45, 0.99999994], dtype=np.float32)


def planted(n, seed):
    """Noise scaled to +-1.2 (a few samples of a long row leave [-1, 1)) with the special values at both ends of a row that has room."""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    if n:
        x *= np.float32(1.2 / max(1e-9, float(np.abs(x).max())))
    k = min(n, len(SPECIAL))
    x[:k] = SPECIAL[:k]
    if n >= 2 * len(SPECIAL):
        x[n - len(SPECIAL):] = SPECIAL[::-1]
    return x


@pytest.mark.parametrize("fmt", ["PCM16", "PCM24", "PCM32", "FLOAT32"])
def test_gain_encoder_writes_the_bytes_of_the_plain_encoder(hip, fmt):
    from vibravox_amd import _lib, corpus

    tile = _lib.pcm_encode_tile()
    lengths = [0, 1, 7, 9, tile - 1, tile, tile + 1, 2 * tile + 5]
    pitch, base = 2 * tile + 7, 3
    contents = [planted(n, 300 + r) for r, n in enumerate(lengths)]
    host = np.full(base + len(lengths) * pitch, np.nan, dtype=np.float32)   # what lies behind a row is neither read nor counted
    for r, x in enumerate(contents):
        host[base + r * pitch:base + r * pitch + len(x)] = x
    whole = torch.from_numpy(host).to(DEV)
    src = whole[base:]                                                      # the rows start everywhere on the 4-byte grid
    assert src.data_ptr() % 16 == 12 and pitch % 4
    (group,) = corpus.plan_image(lengths, fmt, 1 << 30)
    rows = np.zeros(len(lengths), dtype=corpus.ENC_ROW_DTYPE)
    for r, n in enumerate(lengths):
        rows[r] = (r * pitch, group.starts[r] + corpus.HEADER_BYTES, n, corpus.FORMATS.index(fmt))

    def run(source, gains):
        image = torch.full((group.nbytes + 64,), FILL, dtype=torch.uint8, device=DEV)
        clipped = torch.full((len(lengths),), -7, dtype=torch.int32, device=DEV)
        assert corpus.rows_to_pcm(source, rows, image, clipped, gains) is clipped
        return image, clipped

    plain_image, plain_clipped = run(src, None)
    ones = torch.ones(len(lengths), dtype=torch.float32, device=DEV)
    image, clipped = run(src, ones)
    assert torch.equal(image, plain_image) and torch.equal(clipped, plain_clipped)      # gains of exactly 1.0: the existing entry's bytes
    assert bool((plain_image[group.nbytes:] == FILL).all())
    # other gains: the bytes of the plain entry on x * g, the product formed in float32 by torch
    g = torch.tensor([0.5, 1.7, 0.3333333, 2.0, 0.8912509, 1.0, 0.0316227, 1.1220185], dtype=torch.float32, device=DEV)
    scaled = whole.clone()
    for r in range(len(lengths)):
        lo = base + r * pitch
        scaled[lo:lo + pitch] = whole[lo:lo + pitch] * g[r]
    want_image, want_clipped = run(scaled[base:], None)
    image, clipped = run(src, g)
    assert torch.equal(image, want_image) and torch.equal(clipped, want_clipped)
    assert not torch.equal(image, plain_image)
    if fmt != "FLOAT32":
        assert int(clipped[-1]) != int(plain_clipped[-1])                              # 1.12 x a row that already clips: more samples leave the range
    assert torch.equal(whole.cpu().view(torch.int32), torch.from_numpy(host).view(torch.int32))   # the source is only read
    with pytest.raises(ValueError, match="gains"):
        corpus.rows_to_pcm(src, rows, image, clipped, g[:3])
    with pytest.raises(ValueError, match="gains"):
        corpus.rows_to_pcm(src, rows, image, clipped, g.double())


# ---- enhance_to_pcm ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generator(seed=5):
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    torch.manual_seed(seed)
    return EBENGenerator(m=4, n=32, p=2).to(DEV).eval()


def randn(n, seed):
    return 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def collect(gen, clips, **kw):
    """The files of ``enhance_to_pcm`` as bytes per clip, the clipped counts, the levels (None without ``loudness``) and the group count."""
    from vibravox_amd.inference import enhance_to_pcm

    files, counts, levels, groups = {}, {}, {}, 0
    for item in enhance_to_pcm(gen, clips, **kw):
        assert len(item) == (5 if kw.get("loudness") is not None else 4)
        indices, image, spans, clipped = item[:4]
        view = image.numpy()
        for k, (i, (a, b), c) in enumerate(zip(indices, spans, clipped)):
            files[i], counts[i] = bytes(view[a:b]), c
            if len(item) == 5:
                assert len(item[4]) == len(indices)
                levels[i] = item[4][k]
        groups += 1
    assert sorted(files) == list(range(len(clips)))
    return files, counts, (levels if levels else None), groups


def step_by_step(gen, clips, fmt, rate, target, peak, **kw):
    """``enhance_clips`` (resampled to ``rate``), then ``loudness_gain`` on every result alone, then ``rows_to_pcm`` on the scaled row."""
    from vibravox_amd import augment, corpus
    from vibravox_amd.inference import enhance_clips
    from vibravox_amd.metrics import loudness_gain

    out = []
    for y in enhance_clips(gen, clips, **kw):
        y = y.reshape(-1)
        if rate != MODEL:
            y = augment.resample(y, MODEL, rate).reshape(-1)
        level, pk, g = loudness_gain(y, rate, None, target, peak)
        scaled = (y * g).contiguous()
        n = scaled.numel()
        rows = np.zeros(1, dtype=corpus.ENC_ROW_DTYPE)
        rows[0] = (0, 0, n, corpus.FORMATS.index(fmt))
        image = torch.zeros(corpus._up(n * O.BYTES[fmt]), dtype=torch.uint8, device=DEV)
        clipped = corpus.rows_to_pcm(scaled, rows, image)
        out.append((corpus.wav_header(rate, n, fmt) + bytes(image[: n * O.BYTES[fmt]].cpu().numpy()), int(clipped[0]), float(level), float(pk),
                    float(g), y))
    return out


LENGTHS = [12000, 6000, 20800, 7777, 9000, 16001]   # 0.4 ... 1.3 s at the model's rate, not in order of length; 6000: too short for a block


def test_enhance_to_pcm_normalises_in_the_encode_launch(hip, monkeypatch):
    from vibravox_amd import corpus
    from vibravox_amd.metrics import integrated_loudness

    gen = generator()
    clips = [randn(n, n).to(DEV) for n in LENGTHS]
    launches = []
    real = corpus.rows_to_pcm
    monkeypatch.setattr(corpus, "rows_to_pcm", lambda *a, **k: (launches.append(a[4] if len(a) > 4 else k.get("gains")), real(*a, **k))[1])
    files, counts, levels, groups = collect(gen, clips, format="PCM32", loudness=-23.0, max_batch_samples=30000, max_stage_bytes=50000 * 4)
    assert groups >= 2 and len(launches) >= 3 and all(g is not None and g.is_cuda for g in launches)   # the gains reach every launch on the device
    monkeypatch.undo()
    want = step_by_step(gen, clips, "PCM32", MODEL, -23.0, -1.0, max_batch_samples=30000)
    worst, bound, plain = 0.0, 0, 0
    ceiling = 10.0 ** (-1.0 / 20.0)
    for i, (data, clipped, level, pk, g, y) in enumerate(want):
        assert files[i] == data and counts[i] == clipped == 0, i
        assert np.float32(levels[i][0]).view(np.int32) == np.float32(level).view(np.int32) and levels[i][1] == g, i
        back = torch.from_numpy(O.decode(files[i][44:], "PCM32")).to(DEV)
        assert float(back.abs().max()) <= ceiling * (1 + 2.0 ** -22)
        if not math.isfinite(level):
            assert g == 1.0 and LENGTHS[i] == 6000
            continue
        rms = float(y.double().pow(2).mean().sqrt())
        assert rms / 10.0 ** ((level + 0.691) / 20.0) <= 10.0, i                      # the condition FILE_BAR is derived under
        hit = 10.0 ** ((-23.0 - level) / 20.0) * pk > ceiling
        expected = level + 20.0 * math.log10(g) if hit else -23.0
        bound, plain = bound + hit, plain + (not hit)
        got = float(integrated_loudness(back, MODEL))
        worst = max(worst, abs(got - expected))
        assert abs(got - expected) <= FILE_BAR, (i, got, expected)
    print(f"[PCM32 files read back] largest |L(file) - expected| = {worst:.3e} LU over {plain} files at the target and {bound} at the ceiling")
    assert plain >= 1
    # a ceiling that binds on every file: the files peak at it, and their level is the measured one plus the gain
    files, counts, levels, _ = collect(gen, clips, format="PCM32", loudness=-23.0, peak=-30.0)
    low = step_by_step(gen, clips, "PCM32", MODEL, -23.0, -30.0)
    for i, (data, clipped, level, pk, g, y) in enumerate(low):
        assert files[i] == data and counts[i] == 0, i
        if math.isfinite(level):
            assert abs(g - 10.0 ** (-30.0 / 20.0) / pk) <= 2.0 ** -23 * g, i
            back = torch.from_numpy(O.decode(files[i][44:], "PCM32")).to(DEV)
            assert abs(float(back.abs().max()) - 10.0 ** (-30.0 / 20.0)) <= 2.0 ** -22 * 10.0 ** (-30.0 / 20.0)
            assert abs(float(integrated_loudness(back, MODEL)) - (level + 20.0 * math.log10(g))) <= FILE_BAR, i


def test_enhance_to_pcm_measures_at_the_output_rate(hip):
    gen = generator()
    clips = [randn(3 * n, n).to(DEV) for n in LENGTHS]          # the same clips' lengths at 48 kHz
    files, counts, levels, _ = collect(gen, clips, format="PCM16", input_rate=IN, output_rate=IN, loudness=-20.0, peak=-3.0, max_batch_samples=30000)
    want = step_by_step(gen, clips, "PCM16", IN, -20.0, -3.0, max_batch_samples=30000, input_rate=IN)
    for i, (data, clipped, level, pk, g, y) in enumerate(want):
        assert files[i] == data and counts[i] == clipped, i
        assert np.float32(levels[i][0]).view(np.int32) == np.float32(level).view(np.int32) and levels[i][1] == g, i
    assert sum(math.isfinite(w[2]) for w in want) >= 5


def test_without_loudness_nothing_changes(hip):
    from vibravox_amd import corpus
    from vibravox_amd.inference import enhance_clips

    gen = generator()
    clips = [randn(n, n).to(DEV) for n in LENGTHS]
    want = enhance_clips(gen, clips, max_batch_samples=30000)
    for fmt in ("PCM16", "FLOAT32"):
        files, counts, levels, _ = collect(gen, clips, format=fmt, max_batch_samples=30000, max_stage_bytes=50000 * O.BYTES[fmt])   # four-tuples
        assert levels is None
        for i, y in enumerate(want):
            raw, clipped = O.encode(y.cpu().numpy(), fmt)
            assert files[i] == corpus.wav_header(MODEL, y.shape[-1], fmt) + raw and counts[i] == clipped, (fmt, i)


# ---- enhance_corpus ---------------------------------------------------------------------------------------------------------------------
SENSOR = "throat_microphone"
STEMS = {"a": ("PCM16", 30000), "b": ("PCM24", 19500), "c": ("FLOAT32", 48003), "d": ("PCM32", 23331)}   # frames at 48 kHz


def test_enhance_corpus_reports_the_levels(hip, tmp_path):
    from vibravox_amd import corpus, export

    root = str(tmp_path / "in")
    for k, (stem, (fmt, frames)) in enumerate(STEMS.items()):
        x = F.samples(fmt, frames, 1, k)
        if fmt != "FLOAT32":
            x = x // 4
        F.write_wav(os.path.join(root, "speech_clean", "test", SENSOR, stem + ".wav"), x, fmt, IN)
    gen = generator(1)
    loaded = corpus.ResidentCorpus.load(root, "speech_clean", "test", [SENSOR], MODEL, DEV)
    assert loaded.stems == list(STEMS)

    def files(out_root):
        out = {}
        for stem in STEMS:
            with open(os.path.join(out_root, "speech_clean", "test", SENSOR, stem + ".wav"), "rb") as f:
                out[stem] = f.read()
        return out

    plain = export.enhance_corpus({SENSOR: gen}, root, str(tmp_path / "plain"), "speech_clean", "test")
    assert sorted(plain[SENSOR]) == ["clipped", "files", "format", "rate", "seconds", "skipped"]            # today's keys, no more
    unscaled = step_by_step(gen, loaded.clips(SENSOR), "PCM16", MODEL, -23.0, -1.0)
    report = export.enhance_corpus({SENSOR: gen}, root, str(tmp_path / "level"), "speech_clean", "test", loudness=-23.0)
    assert sorted(report[SENSOR]) == ["clipped", "files", "format", "loudness", "rate", "seconds", "skipped"]
    assert {k: v for k, v in report[SENSOR].items() if k not in ("loudness", "clipped")} == {k: v for k, v in plain[SENSOR].items() if k != "clipped"}
    written = files(str(tmp_path / "level"))
    assert list(report[SENSOR]["loudness"]) == sorted(STEMS)
    for stem, (data, clipped, level, pk, g, y) in zip(STEMS, unscaled):
        assert written[stem] == data, stem
        lufs, gain_db = report[SENSOR]["loudness"][stem]
        assert np.float32(lufs).view(np.int32) == np.float32(level).view(np.int32) and gain_db == 20.0 * math.log10(g), stem
        assert report[SENSOR]["clipped"].get(stem, 0) == clipped
    assert written != files(str(tmp_path / "plain"))
    # a loaded corpus, a lower ceiling, another format and rate; and the refusals that come before any work
    again = export.enhance_corpus({SENSOR: gen}, loaded, str(tmp_path / "low"), "speech_clean", "test", loudness=-23.0, peak=-12.0, format="PCM24",
                                  output_rate=IN, max_stage_bytes=400000)   # several groups: halves of 200 000 bytes, the largest file 144 053
    low = step_by_step(gen, loaded.clips(SENSOR), "PCM24", IN, -23.0, -12.0)
    written = files(str(tmp_path / "low"))
    for stem, (data, clipped, level, pk, g, y) in zip(STEMS, low):
        assert written[stem] == data and again[SENSOR]["loudness"][stem][1] == 20.0 * math.log10(g), stem
    with pytest.raises(ValueError, match="100 ms hops"):
        export.enhance_corpus({SENSOR: gen}, loaded, str(tmp_path / "odd"), "speech_clean", "test", loudness=-23.0, output_rate=11025)
    assert not os.path.exists(str(tmp_path / "odd"))
