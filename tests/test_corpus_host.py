"""CPU (no GPU): the WAVE header reader, the directory scan, the store and epoch plans of vibravox_amd.corpus, and the argument checks
of the two entry points of csrc/corpus.hip."""
import ctypes
import os

import numpy as np
import pytest

from tests import corpus_fixtures as F
from vibravox_amd import corpus
from vibravox_amd.inference import resampled_length


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


# ---- wav_info ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", corpus.FORMATS)
@pytest.mark.parametrize("extensible", [False, True])
def test_wav_info_reads_each_accepted_format(tmp_path, fmt, extensible):
    x = F.samples(fmt, 37, 2, 1)
    p = F.write_wav(tmp_path / "a.wav", x, fmt, 44100, extensible=extensible)
    info = corpus.wav_info(p)
    assert info == (44100, 2, 37, fmt, 12 + 8 + (40 if extensible else 16) + 8, 37 * 2 * F.BITS[fmt] // 8)
    with open(p, "rb") as f:
        f.seek(info.data_offset)
        raw = f.read(info.data_bytes)
    assert raw == F.encode(x, fmt)


def test_wav_info_skips_unknown_chunks_and_honours_the_pad_byte(tmp_path):
    x = F.samples("PCM16", 11, 1, 2)
    plain = corpus.wav_info(F.write_wav(tmp_path / "plain.wav", x, "PCM16", 16000))
    listed = corpus.wav_info(F.write_wav(tmp_path / "list.wav", x, "PCM16", 16000, before_data=[(b"LIST", b"INFOabcd"), (b"fact", b"\x0b\0\0\0")]))
    assert listed == plain._replace(data_offset=plain.data_offset + 16 + 12)
    odd = corpus.wav_info(F.write_wav(tmp_path / "odd.wav", x, "PCM16", 16000, before_data=[(b"note", b"abc")]))   # 3 bytes + 1 pad
    assert odd == plain._replace(data_offset=plain.data_offset + 8 + 4)
    for p, info in (("list.wav", listed), ("odd.wav", odd)):
        with open(tmp_path / p, "rb") as f:
            f.seek(info.data_offset)
            assert f.read(info.data_bytes) == F.encode(x, "PCM16")


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_a_data_size_of_zero_or_all_ones_runs_to_the_end_of_the_file(tmp_path, size):
    x = F.samples("PCM24", 9, 3, 3)
    info = corpus.wav_info(F.write_wav(tmp_path / "s.wav", x, "PCM24", 48000, data_size=size))
    assert (info.frames, info.data_bytes) == (9, 81)


def test_refused_files_raise_a_value_error_naming_the_file(tmp_path):
    x16 = F.samples("PCM16", 8, 1, 4)
    cases = {
        "eight_bit.wav": (dict(x=x16.astype(np.uint8), fmt="raw", bits=8, tag=1), "8-bit"),
        "float64.wav": (dict(x=x16.astype("<f8"), fmt="raw", bits=64, tag=3), "64-bit float"),
        "adpcm.wav": (dict(x=x16.astype(np.uint8), fmt="raw", bits=4, tag=2), "ADPCM"),
        "rf64.wav": (dict(x=x16, fmt="PCM16", riff=b"RF64"), "RF64"),
    }
    for name, (kw, word) in cases.items():
        kw = dict(kw)
        p = F.write_wav(tmp_path / name, kw.pop("x"), kw.pop("fmt"), 16000, **kw)
        with pytest.raises(ValueError) as e:
            corpus.wav_info(p)
        assert name in str(e.value) and word in str(e.value), str(e.value)
    good = open(F.write_wav(tmp_path / "good.wav", x16, "PCM16", 16000), "rb").read()
    for cut, name in ((7, "cut7.wav"), (20, "cut20.wav"), (36, "cut36.wav")):   # inside RIFF, inside fmt, in front of data
        (tmp_path / name).write_bytes(good[:cut])
        with pytest.raises(ValueError) as e:
            corpus.wav_info(tmp_path / name)
        assert name in str(e.value) and "truncated" in str(e.value), str(e.value)
    (tmp_path / "short.wav").write_bytes(good[:-4])   # the data chunk says more than the file holds
    with pytest.raises(ValueError, match="short.wav"):
        corpus.wav_info(tmp_path / "short.wav")


# ---- scan and the store plan -----------------------------------------------------------------------------------------------------------
def _tree(root, subset, split, files):
    """files: {sensor: {stem: (fmt, frames, rate)}}"""
    for sensor, items in files.items():
        os.makedirs(os.path.join(root, subset, split, sensor), exist_ok=True)
        for k, (stem, (fmt, frames, rate)) in enumerate(items.items()):
            F.write_wav(os.path.join(root, subset, split, sensor, stem + ".wav"), F.samples(fmt, frames, 1, k), fmt, rate)


def test_scan_pairs_by_stem_and_skips_empty_files(tmp_path):
    _tree(tmp_path, "speech_clean", "train", {
        "headset_microphone": {"b": ("PCM16", 30, 48000), "a": ("PCM16", 10, 16000), "only_air": ("PCM16", 5, 16000), "empty": ("PCM16", 0, 16000)},
        "throat_microphone": {"a": ("FLOAT32", 10, 16000), "b": ("PCM24", 30, 48000), "only_body": ("PCM16", 5, 16000), "empty": ("PCM16", 0, 16000)},
    })
    sc = corpus.scan(tmp_path, "speech_clean", "train", ["headset_microphone", "throat_microphone"])
    assert sc.stems == ["a", "b"] and sc.skipped == ["empty"]
    assert [i.format for i in sc.infos["throat_microphone"]] == ["FLOAT32", "PCM24"]
    assert [os.path.basename(p) for p in sc.paths["headset_microphone"]] == ["a.wav", "b.wav"]
    same = corpus.scan(tmp_path, "speech_clean", "train", ["headset_microphone", "headset_microphone"])
    assert same.stems == ["a", "b", "only_air"] and list(same.infos) == ["headset_microphone"]
    with pytest.raises(ValueError, match="split"):
        corpus.scan(tmp_path, "speech_clean", "dev", ["headset_microphone"])
    with pytest.raises(FileNotFoundError):
        corpus.scan(tmp_path, "speech_clean", "test", ["headset_microphone"])


@pytest.mark.parametrize("other", [("PCM16", 31, 48000), ("PCM16", 30, 44100)])
def test_scan_raises_when_a_pair_differs_in_frames_or_rate(tmp_path, other):
    _tree(tmp_path, "speech_clean", "train", {"headset_microphone": {"a": ("PCM16", 30, 48000)}, "throat_microphone": {"a": other}})
    with pytest.raises(ValueError, match="same length"):
        corpus.scan(tmp_path, "speech_clean", "train", ["headset_microphone", "throat_microphone"])


def test_store_offsets_are_the_running_sum_of_resampled_length():
    infos = [corpus.WavInfo(r, 1, f, "PCM16", 44, 2 * f) for r, f in ((48000, 1), (16000, 77), (44100, 4411), (8000, 3), (48000, 3000), (16000, 1))]
    offsets, lengths = corpus.plan_store(infos, 16000)
    assert lengths == [resampled_length(i.frames, i.rate, 16000) for i in infos] == [1, 77, 1601, 6, 1000, 1]
    assert offsets == [0] + list(np.cumsum(lengths))


def test_groups_cover_the_files_in_order_within_the_staging_budget():
    sizes = [100, 3, 50, 16, 200, 1]
    groups = corpus.plan_groups(sizes, 400)
    assert groups[0][0] == 0 and groups[-1][1] == len(sizes) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    for lo, hi in groups:
        assert corpus._group_bytes(hi - lo, sum(corpus._up(b) for b in sizes[lo:hi])) <= 400
    assert len(groups) > 1
    with pytest.raises(ValueError, match="staging"):
        corpus.plan_groups([1000], 400)


# ---- epoch plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_plan_gives_every_rank_the_same_steps_and_no_item_twice(world, shuffle, drop_last):
    n, bs = 10, 2
    for epoch in (0, 1):
        plans = [corpus.epoch_plan(n, bs, shuffle=shuffle, drop_last=drop_last, seed=7, epoch=epoch, rank=r, world_size=world) for r in range(world)]
        assert len({len(p) for p in plans}) == 1 and len(plans[0]) >= 1
        assert len({tuple(len(b) for b in p) for p in plans}) == 1          # the same batch sizes step by step
        per_rank = [[i for b in p for i in b] for p in plans]
        seen = [i for items in per_rank for i in items]
        assert len(seen) == len(set(seen))
        # the order every rank drew: the union, interleaved back, is a prefix of one permutation of the items
        again = corpus.epoch_plan(n, n, shuffle=shuffle, seed=7, epoch=epoch)
        order = again[0]
        assert sorted(order) == list(range(n))
        k = len(per_rank[0])
        assert [per_rank[j % world][j // world] for j in range(k * world)] == order[:k * world]
        assert k * world >= (n // world) * world - (bs - 1) * world
        assert plans == [corpus.epoch_plan(n, bs, shuffle=shuffle, drop_last=drop_last, seed=7, epoch=epoch, rank=r, world_size=world) for r in range(world)]
    if not shuffle and world == 1:
        assert corpus.epoch_plan(n, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
        assert corpus.epoch_plan(n, 4, drop_last=True) == [[0, 1, 2, 3], [4, 5, 6, 7]]


def test_epoch_plan_changes_with_the_epoch_and_leaves_the_global_generator_alone():
    import torch

    torch.manual_seed(5)
    want = torch.randint(0, 1000, (4,))
    torch.manual_seed(5)
    a = corpus.epoch_plan(10, 10, shuffle=True, seed=1, epoch=0)
    b = corpus.epoch_plan(10, 10, shuffle=True, seed=1, epoch=1)
    assert torch.equal(torch.randint(0, 1000, (4,)), want)
    assert a != b and a == corpus.epoch_plan(10, 10, shuffle=True, seed=1, epoch=0)
    with pytest.raises(ValueError):
        corpus.epoch_plan(10, 2, rank=2, world_size=2)


# ---- the entry points' argument checks ---------------------------------------------------------------------------------------------------
def _table(*rows):
    t = np.zeros(len(rows), dtype=corpus.ROW_DTYPE)
    for k, r in enumerate(rows):
        t[k] = r
    return t


@pytest.mark.parametrize("entry", ["decode", "resample"])
def test_entry_points_refuse_bad_arguments_without_gpu(lib, entry):
    """Every call is refused on the host (EBEN_EINVAL and a message) before any launch: the device pointers are made up and never
    dereferenced, only the host tables are read."""
    from vibravox_amd._lib import PCM_F32, PCM_S16, PCM_S24

    P = ctypes.c_void_p
    ok_rows = _table((0, 100, 1, 0, PCM_S16), (208, 30, 2, 1, PCM_S24), (400, 7, 3, 2, PCM_F32))
    ok_offs = np.array([0, 100, 130], dtype="<i8")
    good = dict(data=P(0x10000), data_bytes=1024, rows=ok_rows, rows_dev=P(0x20000), k=P(0x30000), offs=None, offs_dev=None, out=P(0x40000),
                out_lens=P(0x50000), n=3, extent=100, orig=3, new=1, width=19)
    if entry == "resample":
        good.update(extent=34)

    def call(**kw):
        a = dict(good, **kw)
        rows_host = a["rows"].ctypes.data if isinstance(a["rows"], np.ndarray) else a["rows"]
        offs_host = a["offs"].ctypes.data if isinstance(a["offs"], np.ndarray) else a["offs"]
        if entry == "decode":
            return lib.eben_pcm_decode_ragged(a["data"], a["data_bytes"], rows_host, a["rows_dev"], offs_host, a["offs_dev"], a["out"], a["out_lens"],
                                              a["n"], a["extent"], None)
        return lib.eben_pcm_resample_ragged(a["data"], a["data_bytes"], rows_host, a["rows_dev"], a["k"], offs_host, a["offs_dev"], a["out"],
                                            a["out_lens"], a["n"], a["extent"], a["orig"], a["new"], a["width"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in lib.eben_last_error(), (kw, lib.eben_last_error())

    pointers = ["data", "rows", "rows_dev", "out", "out_lens"] + (["k"] if entry == "resample" else [])
    for name in pointers:
        refused(b"null", **{name: None})
    for name, bad in (("data", 0x10008), ("rows_dev", 0x20004), ("out", 0x40002), ("out_lens", 0x50002), ("offs_dev", 0x60004)):
        kw = {name: P(bad)}
        if name == "offs_dev":
            kw.update(offs=ok_offs, extent=137)
        refused(b"misaligned", **kw)
    if entry == "resample":
        refused(b"misaligned", k=P(0x30002))
        refused(b"fits no tile", orig=5000)
        refused(b"ratio", new=0)
    refused(b"offsets", offs=ok_offs)                       # one of the two offset tables only
    for n in (0, -1, 65536):
        refused(b"rows", n=n)
    refused(b"unknown format", rows=_table((0, 100, 1, 0, 4)), n=1)
    refused(b"unknown format", rows=_table((0, 100, 1, 0, -1)), n=1)
    refused(b"channel 1 of 1", rows=_table((0, 100, 1, 1, PCM_S16)), n=1)
    refused(b"channel 3 of 3", rows=_table((0, 7, 3, 3, PCM_F32)), n=1)
    refused(b"channels", rows=_table((0, 7, 0, 0, PCM_F32)), n=1)
    refused(b"frames", rows=_table((0, -1, 1, 0, PCM_S16)), n=1)
    refused(b"multiple of 16", rows=_table((8, 10, 1, 0, PCM_S16)), n=1)
    refused(b"multiple of 16", rows=_table((-16, 10, 1, 0, PCM_S16)), n=1)
    refused(b"buffer of 1024", rows=_table((1008, 9, 1, 0, PCM_S16)), n=1)          # 18 bytes from 1008
    refused(b"too small", extent=good["extent"] - 1)                               # the pitch against the longest row
    flat_extent = 137 if entry == "decode" else 34 + 10 + 3
    flat_offs = ok_offs if entry == "decode" else np.array([0, 34, 44], dtype="<i8")
    flat = dict(offs=flat_offs, offs_dev=P(0x60000), out_lens=None)
    refused(b"store of", extent=flat_extent - 1, **flat)                            # the last row past the store
    overlap = flat_offs.copy()
    overlap[1] -= 1
    refused(b"first free float", extent=flat_extent, **dict(flat, offs=overlap))
    refused(b"out_lens", out_lens=None)                                             # padded rows need the length table


# ---- run.py: epochs and ranks -------------------------------------------------------------------------------------------------------------
def test_run_restarts_a_reiterable_loader_and_passes_the_rank(monkeypatch):
    import itertools

    import run

    class Loader:
        epochs = 0

        def __iter__(self):
            Loader.epochs += 1
            return iter([Loader.epochs * 10, Loader.epochs * 10 + 1])

    assert list(itertools.islice(run._batches(Loader()), 5)) == [10, 11, 20, 21, 30]
    endless = (k for k in itertools.count())                                   # the synthetic module's generator: taken as it is
    assert list(itertools.islice(run._batches(endless), 3)) == [0, 1, 2]
    with pytest.raises(RuntimeError, match="no batch"):
        next(run._batches([]))
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfg = run.compose(["lightning_datamodule=local_bwe", "lightning_datamodule.root=/somewhere"])["lightning_datamodule"]
    node = run._with_rank(cfg)
    assert (node["rank"], node["world_size"], node["root"]) == (1, 2, "/somewhere") and "rank" not in cfg
    assert run._with_rank(dict(cfg, rank=0))["rank"] == 0                      # what the config says stays
    noisy = run._with_rank(run.compose(["lightning_datamodule=local_noisybwe"])["lightning_datamodule"])
    assert noisy["_target_"].endswith("LocalNoisyBWEDataModule") and noisy["world_size"] == 2 and noisy["snr_range"] is None
    synthetic = run.compose([])["lightning_datamodule"]
    assert run._with_rank(synthetic) == synthetic                              # a constructor without rank / world_size gets neither
