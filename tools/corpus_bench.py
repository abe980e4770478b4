"""Recordings on disk to resident clips: what `ResidentCorpus.load` costs, against what the package could do before it.

    python tools/corpus_bench.py [--files 2048] [--iters 3] [--kernel-iters 30] [--batches 50] [--out FILE]

The corpus is generated here, under a temporary directory that is removed at the end: `--files` mono PCM16 files of 1 .. 12 s at 48 kHz
(seed 0), half of them under `headset_microphone`, half under `throat_microphone`, as pairs.  Every pass reads the files from the page
cache (the generation leaves them there, and a warm-up pass comes first).
(a) `ResidentCorpus.load` of both sensors: host clock around the call and the device synchronise behind it; median of `--iters`.
(b) The same files the way the parent commit can: numpy decode on the host (int16 -> float32 / 32768), upload of padded float32 rows in
    groups of 256 files, `rate.resample_ragged`; the two alternate with (a).
(c) The kernels alone on the uploaded bytes of one 256-file group: `eben_pcm_resample_ragged` (one launch, flat store) against
    `eben_pcm_decode_ragged` into padded rows followed by `eben_resample_ragged` (two launches), each with the bytes it has to read and
    write per second, beside a device-to-device torch copy of the same byte count; the three alternate, HIP events around a pass.
(d) ms per training batch of 32 x 2.5 s from `LocalBWEDataModule.train_dataloader()` beside `SyntheticBWEDataModule`'s randn + upload.
Prints one JSON line per measurement and a summary; `--out` writes both to a file."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IN, MODEL = 48000, 16000
SENSORS = ("headset_microphone", "throat_microphone")


def write_pcm16(path: str, x: np.ndarray, rate: int) -> None:
    body = x.astype("<i2").tobytes()
    head = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16)
    with open(path, "wb") as f:
        f.write(head + b"data" + struct.pack("<I", len(body)) + body)


def timed(torch, fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import corpus, rate
    from vibravox_amd.inference import resampled_length
    from vibravox_amd.lightning_datamodules import LocalBWEDataModule
    from vibravox_amd.synthetic import SyntheticBWEDataModule

    assert torch.cuda.is_available(), "corpus_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda", 0)
    pairs = max(1, args.files // 2)
    rng = np.random.RandomState(0)
    frames = [int(t) for t in rng.randint(1 * IN, 12 * IN + 1, size=pairs)]
    root = tempfile.mkdtemp(prefix="corpus_bench_")
    lines = []
    try:
        for sensor in SENSORS:
            os.makedirs(os.path.join(root, "speech_clean", "train", sensor))
            for k, n in enumerate(frames):
                write_pcm16(os.path.join(root, "speech_clean", "train", sensor, f"u{k:05d}.wav"), rng.randint(-3000, 3000, size=n), IN)
        audio_s = len(SENSORS) * sum(frames) / IN
        pcm_bytes = 2 * len(SENSORS) * sum(frames)

        # ---- (a) and (b): the whole load, alternating ------------------------------------------------------------------------------------
        def resident():
            c = corpus.ResidentCorpus.load(root, "speech_clean", "train", SENSORS, MODEL, dev)
            torch.cuda.synchronize()
            return c

        def parent():
            sc = corpus.scan(root, "speech_clean", "train", SENSORS)
            kept = []
            for sensor in SENSORS:
                for lo in range(0, len(sc.stems), 256):
                    infos, paths = sc.infos[sensor][lo:lo + 256], sc.paths[sensor][lo:lo + 256]
                    host = torch.zeros((len(infos), max(i.frames for i in infos)), dtype=torch.float32, pin_memory=True)
                    view = host.numpy()
                    for r, (i, p) in enumerate(zip(infos, paths)):
                        with open(p, "rb") as f:
                            f.seek(i.data_offset)
                            view[r, :i.frames] = np.frombuffer(f.read(i.data_bytes), "<i2").astype(np.float32) / np.float32(32768)
                    kept.append(rate.resample_ragged(host.to(dev, non_blocking=True), [i.frames for i in infos], IN, MODEL))
            torch.cuda.synchronize()
            return kept

        paths = [("numpy_decode_upload_resample_ragged", parent), ("ResidentCorpus.load", resident)]
        first = {name: fn() for name, fn in paths}   # warm-up: page cache, code objects, pinned and device allocations
        c = first["ResidentCorpus.load"]
        equal = all(torch.equal(c.clip(k, SENSORS[0]), first["numpy_decode_upload_resample_ragged"][k // 256][0][k % 256, :c.lengths[k]])
                    for k in range(0, len(c), 97))
        del first
        times = {name: [] for name, _ in paths}
        for _ in range(args.iters):
            for name, fn in paths:
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        for name, _ in paths:
            s = statistics.median(times[name])
            lines.append(dict(part="a" if name.startswith("Resident") else "b", path=name, files=len(SENSORS) * pairs, audio_hours=round(audio_s / 3600, 3),
                              pcm_bytes=pcm_bytes, median_s=round(s, 3), min_s=round(min(times[name]), 3), max_s=round(max(times[name]), 3),
                              audio_hours_per_second=round(audio_s / 3600 / s, 3), gigabytes_of_pcm_per_second=round(pcm_bytes / s / 1e9, 2),
                              sampled_clips_equal=equal))
            print(json.dumps(lines[-1]), flush=True)

        # ---- (c) the kernels alone on one group's bytes -----------------------------------------------------------------------------------
        sc = corpus.scan(root, "speech_clean", "train", SENSORS[:1])
        infos, fpaths = sc.infos[SENSORS[0]][:256], sc.paths[SENSORS[0]][:256]
        rows = np.zeros(len(infos), dtype=corpus.ROW_DTYPE)
        blob = bytearray()
        for r, (i, p) in enumerate(zip(infos, fpaths)):
            blob += b"\0" * (-len(blob) % 16)
            rows[r] = (len(blob), i.frames, 1, 0, 0)
            with open(p, "rb") as f:
                f.seek(i.data_offset)
                blob += f.read(i.data_bytes)
        data = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        n_in = [int(v) for v in rows["frames"]]
        n_out = [resampled_length(v, IN, MODEL) for v in n_in]
        offsets = [0]
        for v in n_out:
            offsets.append(offsets[-1] + v)
        store = torch.empty(offsets[-1], dtype=torch.float32, device=dev)
        pitch_in, pitch_out = max(n_in), max(n_out)
        decoded = torch.empty((len(rows), pitch_in), dtype=torch.float32, device=dev)
        padded = torch.empty((len(rows), pitch_out), dtype=torch.float32, device=dev)
        fused_bytes = 2 * sum(n_in) + 4 * sum(n_out)
        two_bytes = 2 * sum(n_in) + 4 * decoded.numel() + 4 * sum(n_in) + 4 * padded.numel()

        def fused():
            corpus.pcm_to_rows(data, rows, rates=(IN, MODEL), offsets=offsets[:-1], out=store)

        def two():
            d, lens = corpus.pcm_to_rows(data, rows, out=decoded, pitch=pitch_in)
            rate.resample_ragged(d, lens, IN, MODEL, out=padded)

        copies = {}
        for name, nbytes in (("fused", fused_bytes), ("two", two_bytes)):
            src = torch.empty(nbytes // 8, device=dev)
            copies[name] = (src, torch.empty_like(src))
        kpaths = [("pcm_resample_ragged_one_launch", fused, fused_bytes), ("copy_of_the_fused_bytes", lambda: copies["fused"][1].copy_(copies["fused"][0]), fused_bytes),
                  ("pcm_decode_ragged_then_resample_ragged", two, two_bytes), ("copy_of_the_two_launch_bytes", lambda: copies["two"][1].copy_(copies["two"][0]), two_bytes)]
        for _, fn, _ in kpaths:
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(store[offsets[r]:offsets[r + 1]], padded[r, :n_out[r]]) for r in range(0, len(rows), 17))
        kt = {name: [] for name, _, _ in kpaths}
        for _ in range(args.kernel_iters):
            for name, fn, _ in kpaths:
                kt[name].append(timed(torch, fn))
        for name, _, nbytes in kpaths:
            ms = statistics.median(kt[name])
            lines.append(dict(part="c", path=name, rows=len(rows), bytes_read_plus_written=nbytes, median_ms=round(ms, 4), min_ms=round(min(kt[name]), 4),
                              max_ms=round(max(kt[name]), 4), gigabytes_per_second=round(nbytes / (ms * 1e-3) / 1e9, 1), results_equal=same))
            print(json.dumps(lines[-1]), flush=True)
        del data, store, decoded, padded, copies

        # ---- (d) a training batch ---------------------------------------------------------------------------------------------------------
        dm = LocalBWEDataModule(MODEL, root=root, sensor=SENSORS[1], collate_strategy="constant_length-2500-ms", batch_size=32, device=dev)
        dm.corpora[("principal", "train")] = c   # the split loaded above
        loader = dm.train_dataloader()
        synthetic = SyntheticBWEDataModule(MODEL, 32, 2500, device=dev).train_dataloader()

        def endless():
            while True:
                yield from loader

        sources = [("SyntheticBWEDataModule_randn_upload", synthetic), ("LocalBWEDataModule_train_dataloader", endless())]
        bt = {name: [] for name, _ in sources}
        for name, it in sources:
            for _ in range(3):
                next(it)
        torch.cuda.synchronize()
        for _ in range(args.iters):
            for name, it in sources:
                t0 = time.perf_counter()
                for _ in range(args.batches):
                    batch = next(it)
                torch.cuda.synchronize()
                bt[name].append((time.perf_counter() - t0) * 1e3 / args.batches)
                del batch
        for name, _ in sources:
            ms = statistics.median(bt[name])
            lines.append(dict(part="d", path=name, batch="32 x 2.5 s", batches_per_round=args.batches, median_ms_per_batch=round(ms, 3),
                              min_ms_per_batch=round(min(bt[name]), 3), max_ms_per_batch=round(max(bt[name]), 3),
                              audio_seconds_per_second=round(32 * 2.5 / (ms * 1e-3), 0)))
            print(json.dumps(lines[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)

    by = {d["path"]: d for d in lines}
    a, b = by["ResidentCorpus.load"], by["numpy_decode_upload_resample_ragged"]
    f1, f2 = by["pcm_resample_ragged_one_launch"], by["pcm_decode_ragged_then_resample_ragged"]
    d1, d0 = by["LocalBWEDataModule_train_dataloader"], by["SyntheticBWEDataModule_randn_upload"]
    summary = [
        f"corpus_bench on {torch.cuda.get_device_name(0)}: {a['files']} mono PCM16 files of 1-12 s at 48 kHz ({a['audio_hours']} h of audio, {pcm_bytes} bytes)",
        f"  (a) ResidentCorpus.load                  : {a['median_s']:8.3f} s  (min {a['min_s']}, max {a['max_s']}; host clock to the synchronise, medians of "
        f"{args.iters} alternated passes, files in the page cache): {a['audio_hours_per_second']} audio-hours/s, {a['gigabytes_of_pcm_per_second']} GB of PCM/s",
        f"  (b) numpy decode, upload, resample_ragged: {b['median_s']:8.3f} s  (min {b['min_s']}, max {b['max_s']}): {b['audio_hours_per_second']} audio-hours/s; "
        f"(a) is {b['median_s'] / a['median_s']:.2f}x its speed; sampled clips equal: {a['sampled_clips_equal']}",
        f"  (c) fused kernel, one launch             : {f1['median_ms']:8.4f} ms  {f1['gigabytes_per_second']} GB/s read + written ({f1['bytes_read_plus_written']} bytes; "
        f"copy of the same bytes {by['copy_of_the_fused_bytes']['median_ms']} ms, {by['copy_of_the_fused_bytes']['gigabytes_per_second']} GB/s)",
        f"      decode, then resample_ragged         : {f2['median_ms']:8.4f} ms  {f2['gigabytes_per_second']} GB/s read + written ({f2['bytes_read_plus_written']} bytes; "
        f"copy of the same bytes {by['copy_of_the_two_launch_bytes']['median_ms']} ms, {by['copy_of_the_two_launch_bytes']['gigabytes_per_second']} GB/s): the fused "
        f"launch takes {f1['median_ms'] / f2['median_ms']:.2f}x the two launches' time; results equal: {f1['results_equal']}",
        f"  (d) loader batch of 32 x 2.5 s           : {d1['median_ms_per_batch']:8.3f} ms  ({d1['audio_seconds_per_second']:.0f} audio-s/s); synthetic randn + upload "
        f"{d0['median_ms_per_batch']} ms ({d0['audio_seconds_per_second']:.0f} audio-s/s)",
    ]
    print("\n".join(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(d) for d in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
