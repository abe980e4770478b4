"""GPU: rows of float32 to the bytes of WAVE files (csrc/pcm_encode.hip) against the numpy oracle of tests/export_oracle.py, and the two
layers on top of it: ``inference.enhance_to_pcm`` against ``enhance_clips`` and ``export.enhance_corpus`` from a directory to a directory.
Every comparison is on bytes or integers."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import corpus_fixtures as F
from tests import export_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
IN, MODEL = 48000, 16000
SPECIAL = np.array([1.0, -1.0, np.inf, -np.inf, np.nan, -0.0, 1e-45], dtype=np.float32)   # the host test's; the last: a denormal
FILL = 0xA5


def noise(n, seed):
    """Seeded normal noise scaled to +-1.2: a few samples of a long row leave [-1, 1)."""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    return x * np.float32(1.2 / max(1e-9, float(np.abs(x).max()))) if n else x


def planted(n, seed):
    """A row's content: noise with the special values at its start and, where there is room, mirrored at its end; half-way cases
    (k + 0.5) / 32768 in the middle of a long row."""
    x = noise(n, seed)
    k = min(n, len(SPECIAL))
    x[:k] = SPECIAL[:k]
    if n >= 2 * len(SPECIAL):
        x[n - len(SPECIAL):] = SPECIAL[::-1]
    if n >= 64:
        ks = np.array([-32768, -3, -2, -1, 0, 1, 2, 101, 32766, 32767], dtype=np.float64)
        x[n // 2:n // 2 + len(ks)] = ((ks + 0.5) / 32768).astype(np.float32)
    return x


def place(lengths, order, fmt):
    """Data offsets of the rows when they lie in the image in ``order``, and the image's size."""
    from vibravox_amd import corpus

    (group,) = corpus.plan_image([lengths[j] for j in order], fmt, 1 << 30)
    at = [0] * len(lengths)
    for start, j in zip(group.starts, order):
        at[j] = start + corpus.HEADER_BYTES
    return at, group.nbytes


def expected_image(nbytes, contents, at, formats):
    want = np.full(nbytes, FILL, dtype=np.uint8)
    counts = []
    for x, a, fmt in zip(contents, at, formats):
        raw, clipped = O.encode(x, fmt)
        assert len(raw) == len(x) * O.BYTES[fmt]
        want[a:a + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        counts.append(clipped)
    return want, counts


@pytest.mark.parametrize("base", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["PCM16", "PCM24", "PCM32", "FLOAT32"])
def test_encode_matches_the_oracle_at_every_tile_edge_and_alignment(hip, fmt, base):
    from vibravox_amd import _lib, corpus

    tile = _lib.pcm_encode_tile()
    lengths = [0, 1, 7, 8, 9, tile - 1, tile, tile + 1, 2 * tile + 5]
    pitch = 2 * tile + 7
    assert pitch % 4 and len({(base + r * pitch) % 4 for r in range(len(lengths))}) == 4   # the rows start everywhere on the 4-byte grid
    contents = [planted(n, 100 * base + r) for r, n in enumerate(lengths)]
    host = np.full(base + len(lengths) * pitch, np.nan, dtype=np.float32)   # what lies behind a row must be neither read nor counted
    for r, x in enumerate(contents):
        host[base + r * pitch:base + r * pitch + len(x)] = x
    whole = torch.from_numpy(host).to(DEV)
    src = whole[base:]   # the pointer itself `base` floats off the 16-byte grid
    assert whole.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 4 * base
    order = [int(j) for j in np.random.default_rng(7).permutation(len(lengths))]
    assert order != sorted(order)
    at, nbytes = place(lengths, order, fmt)
    rows = np.zeros(len(lengths), dtype=corpus.ENC_ROW_DTYPE)
    for r, n in enumerate(lengths):
        rows[r] = (r * pitch, at[r], n, corpus.FORMATS.index(fmt))
    image = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device=DEV)
    clipped = torch.full((len(lengths),), -7, dtype=torch.int32, device=DEV)   # the call zeroes the counts itself
    assert corpus.rows_to_pcm(src, rows, image, clipped) is clipped
    want, counts = expected_image(nbytes + 64, contents, at, [fmt] * len(lengths))
    assert torch.equal(image.cpu(), torch.from_numpy(want))   # the rows' bytes, and 0xA5 everywhere else, the 44 bytes in front of each row included
    assert clipped.cpu().tolist() == counts
    if fmt == "FLOAT32":
        assert counts == [0] * len(lengths)
    else:
        assert counts[-1] >= 8 and counts[0] == 0   # the planted values at both ends, and whatever noise left [-1, 1)
    assert torch.equal(whole.cpu().view(torch.int32), torch.from_numpy(host).view(torch.int32))   # the source is only read


def test_every_pcm16_and_pcm24_code_survives_decode_and_encode_on_the_device(hip):
    from vibravox_amd import corpus

    for fmt, bits, pieces in (("PCM16", 16, 1), ("PCM24", 24, 2)):
        codes = np.arange(-(1 << (bits - 1)), 1 << (bits - 1), dtype=np.int64).reshape(-1, 1)
        raw = torch.from_numpy(np.frombuffer(F.encode(codes, fmt), dtype=np.uint8).copy()).to(DEV)
        per = len(codes) // pieces   # a multiple of 16 bytes in both formats
        table = np.zeros(pieces, dtype=corpus.ROW_DTYPE)
        enc = np.zeros(pieces, dtype=corpus.ENC_ROW_DTYPE)
        for k in range(pieces):
            table[k] = (k * per * bits // 8, per, 1, 0, corpus.FORMATS.index(fmt))
            enc[k] = (k * per, k * per * bits // 8, per, corpus.FORMATS.index(fmt))
        floats, _ = corpus.pcm_to_rows(raw, table)
        assert floats.shape == (pieces, per)
        image = torch.full_like(raw, FILL)
        clipped = corpus.rows_to_pcm(floats, enc, image)
        assert torch.equal(image, raw), fmt
        assert clipped.cpu().tolist() == [0] * pieces
        del raw, floats, image


def test_encode_reads_clips_of_a_flat_store_in_mixed_formats(hip):
    """Rows given by offsets into a 1-D store, as the clips of a ResidentCorpus lie, one behind the other; every row in a format of its
    own, placed in the image in reverse order."""
    from vibravox_amd import _lib, corpus

    tile = _lib.pcm_encode_tile()
    lengths = [5, tile + 1, 300, 0, 2 * tile + 1, 33]
    formats = ["PCM16", "PCM24", "PCM32", "FLOAT32", "PCM16", "FLOAT32"]
    offsets = np.concatenate(([0], np.cumsum(lengths)))
    contents = [planted(n, 40 + r) for r, n in enumerate(lengths)]
    store = torch.from_numpy(np.concatenate(contents)).to(DEV)
    at, end = [0] * len(lengths), 0
    for j in reversed(range(len(lengths))):
        at[j] = corpus._up(end + corpus.HEADER_BYTES)
        end = at[j] + lengths[j] * O.BYTES[formats[j]]
    nbytes = corpus._up(end)
    rows = np.zeros(len(lengths), dtype=corpus.ENC_ROW_DTYPE)
    for r, n in enumerate(lengths):
        rows[r] = (offsets[r], at[r], n, corpus.FORMATS.index(formats[r]))
    image = torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)
    clipped = corpus.rows_to_pcm(store, rows, image)
    want, counts = expected_image(nbytes, contents, at, formats)
    assert torch.equal(image.cpu(), torch.from_numpy(want))
    assert clipped.cpu().tolist() == counts and counts[3] == counts[5] == 0


# ---- enhance_to_pcm ---------------------------------------------------------------------------------------------------------------------
def make_generator(seed, scale=None):
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    class Loud(EBENGenerator):
        """The same generator with its output scaled: what a model that overshoots the format's range looks like."""
        gain = 1.0

        def forward_ragged(self, padded, lengths):
            enhanced, bands = super().forward_ragged(padded, lengths)
            return enhanced * self.gain, bands

    torch.manual_seed(seed)
    gen = (EBENGenerator if scale is None else Loud)(m=4, n=32, p=2)
    if scale is not None:
        gen.gain = float(scale)
    return gen.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def shared_generator():
    return make_generator(5)


def randn(n, seed):
    return 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def collect(gen, clips, **kw):
    """The files of ``enhance_to_pcm`` as bytes per clip, their clipped counts, and the number of groups; each image is checked and
    copied while it is the generator's to give."""
    from vibravox_amd.inference import enhance_to_pcm

    files, counts, groups, seen = {}, {}, 0, []
    for indices, image, spans, clipped in enhance_to_pcm(gen, clips, **kw):
        assert image.dtype is torch.uint8 and image.device.type == "cpu" and image.is_pinned()
        assert len(indices) == len(spans) == len(clipped)
        view = image.numpy()
        last = 0
        for i, (a, b), c in zip(indices, spans, clipped):
            assert last <= a < b <= len(view) and (a + 44) % 16 == 0
            files[i], counts[i], last = bytes(view[a:b]), c, b
        seen += indices
        groups += 1
    assert seen == list(range(len(clips)))
    return files, counts, groups


@pytest.mark.parametrize("fmt", ["PCM16", "PCM24"])
def test_enhance_to_pcm_writes_what_enhance_clips_returns(hip, fmt, monkeypatch):
    from vibravox_amd import corpus
    from vibravox_amd.inference import enhance_clips

    gen = shared_generator()
    lengths = [12000, 3200, 20800, 7777, 9000, 16001, 5000]   # 0.2 ... 1.3 s at the model's rate, not in order of length
    clips = [randn(n, n).to(DEV) for n in lengths]
    want = enhance_clips(gen, clips, max_batch_samples=30000)
    launches = []
    real = corpus.rows_to_pcm
    monkeypatch.setattr(corpus, "rows_to_pcm", lambda *a, **k: (launches.append(len(a[1])), real(*a, **k))[1])
    files, counts, groups = collect(gen, clips, format=fmt, max_batch_samples=30000, max_stage_bytes=50000 * O.BYTES[fmt])
    assert groups >= 2 and len(launches) >= 3 and sum(launches) == len(clips)   # one encode launch per batch, every clip in one of them
    for i, y in enumerate(want):
        raw, clipped = O.encode(y.cpu().numpy(), fmt)
        assert files[i][:44] == corpus.wav_header(MODEL, y.shape[-1], fmt), i
        assert files[i][44:] == raw, i
        assert counts[i] == clipped, i
    one, _, groups = collect(gen, clips, format=fmt)   # one batch, one group: the same files
    assert groups == 1 and one == files


def test_enhance_to_pcm_from_and_to_the_recording_rate(hip):
    from vibravox_amd import augment, corpus
    from vibravox_amd.inference import enhance_clips

    gen = shared_generator()
    lengths = [36000, 9600, 62400, 23331, 27000, 48003, 15000]   # the same clips' lengths at 48 kHz
    clips = [randn(n, n).to(DEV) for n in lengths]
    want = enhance_clips(gen, clips, max_batch_samples=30000, input_rate=IN)
    files, counts, groups = collect(gen, clips, format="PCM16", input_rate=IN, output_rate=IN, max_batch_samples=30000, max_stage_bytes=300000)
    assert groups >= 2
    for i, y in enumerate(want):
        up = augment.resample(y, MODEL, IN)
        raw, clipped = O.encode(up.cpu().numpy(), "PCM16")
        assert files[i][:44] == corpus.wav_header(IN, up.shape[-1], "PCM16"), i
        assert files[i][44:] == raw and counts[i] == clipped, i
    at_model, _, _ = collect(gen, clips, format="PCM16", input_rate=IN, max_batch_samples=30000)   # output_rate None: the model's rate
    for i, y in enumerate(want):
        assert at_model[i] == corpus.wav_header(MODEL, y.shape[-1], "PCM16") + O.encode(y.cpu().numpy(), "PCM16")[0], i


# ---- enhance_corpus ---------------------------------------------------------------------------------------------------------------------
SENSORS = ("throat_microphone", "forehead_accelerometer")
STEMS = {"a": ("PCM16", 30000), "b": ("PCM24", 9600), "c": ("FLOAT32", 48003), "d": ("PCM32", 23331), "e": ("PCM16", 15000)}   # frames at 48 kHz


def write_tree(root):
    for s_k, sensor in enumerate(SENSORS):
        for k, (stem, (fmt, frames)) in enumerate(STEMS.items()):
            x = F.samples(fmt, frames, 1, 10 * s_k + k)
            if fmt != "FLOAT32":
                x = x // 4   # a quarter of full scale
            F.write_wav(os.path.join(root, "speech_clean", "test", sensor, stem + ".wav"), x, fmt, IN)
        F.write_wav(os.path.join(root, "speech_clean", "test", sensor, "empty.wav"), F.samples("PCM16", 0, 1, 0), "PCM16", IN)


def tree_bytes(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


def test_enhance_corpus_from_a_directory_to_a_directory(hip, tmp_path):
    from vibravox_amd import corpus, export
    from vibravox_amd.inference import enhance_clips

    root, out_root = str(tmp_path / "in"), str(tmp_path / "out")
    write_tree(root)
    generators = {SENSORS[0]: make_generator(1), SENSORS[1]: make_generator(2)}
    loaded = corpus.ResidentCorpus.load(root, "speech_clean", "test", SENSORS, MODEL, DEV)
    assert loaded.stems == list(STEMS) and loaded.skipped == ["empty"]
    want = {s: enhance_clips(generators[s], loaded.clips(s)) for s in SENSORS}
    assert not torch.equal(want[SENSORS[0]][0], want[SENSORS[1]][0])

    report = export.enhance_corpus(generators, root, out_root, "speech_clean", "test")
    names = sorted(os.path.join("speech_clean", "test", s, stem + ".wav") for s in SENSORS for stem in STEMS)
    written = tree_bytes(out_root)
    assert sorted(written) == names   # every expected file, no .part file, nothing for the skipped stem
    back = corpus.ResidentCorpus.load(out_root, "speech_clean", "test", SENSORS, MODEL, DEV)
    assert back.stems == loaded.stems and back.skipped == []
    for s in SENSORS:
        seconds = 0.0
        for k, y in enumerate(want[s]):
            raw, _ = O.encode(y.cpu().numpy(), "PCM16")
            assert torch.equal(back.clip(k, s).cpu(), torch.from_numpy(O.decode(raw, "PCM16"))), (s, k)
            seconds += y.shape[-1] / MODEL
        assert report[s]["files"] == len(STEMS) and report[s]["skipped"] == ["empty"] and report[s]["rate"] == MODEL
        assert abs(report[s]["seconds"] - seconds) < 1e-9
        assert report[s]["clipped"] == {stem: O.encode(y.cpu().numpy(), "PCM16")[1] for stem, y in zip(STEMS, want[s])
                                        if O.encode(y.cpu().numpy(), "PCM16")[1]}

    with pytest.raises(FileExistsError):
        export.enhance_corpus(generators, root, out_root, "speech_clean", "test")
    assert tree_bytes(out_root) == written   # nothing was touched
    # a loaded corpus in the directory's place, and a stage so small that every sensor's files leave in several groups
    again = export.enhance_corpus(generators, loaded, out_root, "speech_clean", "test", overwrite=True, max_stage_bytes=70000)
    assert tree_bytes(out_root) == written and again == report


def test_enhance_corpus_reports_the_stems_that_clipped(hip, tmp_path):
    from vibravox_amd import corpus, export
    from vibravox_amd.inference import enhance_clips

    root, out_root = str(tmp_path / "in"), str(tmp_path / "out")
    write_tree(root)
    sensor = SENSORS[0]
    loaded = corpus.ResidentCorpus.load(root, "speech_clean", "test", [sensor], MODEL, DEV)
    peaks = [float(y.abs().max()) for y in enhance_clips(make_generator(1), loaded.clips(sensor))]
    loud = make_generator(1, scale=1.0 / (0.5 * (min(peaks) + max(peaks))))   # the loudest clip leaves [-1, 1), the quietest stays inside
    want = enhance_clips(loud, loaded.clips(sensor))
    counts = {stem: O.encode(y.cpu().numpy(), "PCM16")[1] for stem, y in zip(STEMS, want)}
    assert any(counts.values())
    report = export.enhance_corpus({sensor: loud}, root, out_root, "speech_clean", "test")
    assert report[sensor]["clipped"] == {stem: c for stem, c in counts.items() if c}
    for k, (stem, y) in enumerate(zip(STEMS, want)):
        with open(os.path.join(out_root, "speech_clean", "test", sensor, stem + ".wav"), "rb") as f:
            assert f.read() == corpus.wav_header(MODEL, y.shape[-1], "PCM16") + O.encode(y.cpu().numpy(), "PCM16")[0], stem
