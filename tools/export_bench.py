"""Enhanced recordings from disk to disk: what `export.enhance_corpus` costs, against what the package could do before it.

    python tools/export_bench.py [--files 256] [--iters 3] [--kernel-iters 30] [--out FILE]

The corpus is generated here, under a temporary directory that is removed at the end: `--files` mono PCM16 recordings of 1 .. 12 s at
48 kHz (seed 0) under `throat_microphone`; the generator is an `EBENGenerator(4, 32, 2)` with seeded random weights.  Every pass reads
the files from the page cache (the generation leaves them there, and a warm-up pass comes first) and writes into a fresh directory.
(a) `enhance_corpus` disk to disk, PCM16 at the model's rate: host clock around the call and the device synchronise behind it; median of
    `--iters`.
(b) The same files the way the parent commit can: `ResidentCorpus.load`, `enhance_clips`, then per clip `.cpu()`, a numpy conversion
    (rint, clip, int16) and a header written with `struct`; the two alternate.  The ratio (a) / (b) is stated.
(c) The encode launch alone on one padded batch buffer of 256 rows of 1 .. 12 s at 16 kHz, PCM16 and FLOAT32: HIP events around a pass,
    the bytes it reads plus writes per second, beside a device-to-device torch copy of the same byte count; and the pair
    `rate.resample_ragged` + encode at 16 -> 48 kHz.
(d) Where (a)'s time goes: its stages run one after the other with the device synchronised behind each -- load, forwards, encode
    launches, the copy to pinned memory, the writes.
Prints one JSON line per measurement and a summary; `--out` writes both to a file."""
from __future__ import annotations

import argparse
import concurrent.futures
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
SENSOR = "throat_microphone"
SUBSET, SPLIT = "speech_clean", "test"


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
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from vibravox_amd import corpus, export, inference, ragged, rate
    from vibravox_amd.torch_modules.dnn.eben_generator import EBENGenerator

    assert torch.cuda.is_available(), "export_bench times the device path: it needs an MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    gen = EBENGenerator(m=4, n=32, p=2).to(dev).eval()
    rng = np.random.RandomState(0)
    frames = [int(t) for t in rng.randint(1 * IN, 12 * IN + 1, size=args.files)]
    root = tempfile.mkdtemp(prefix="export_bench_")
    lines = []
    try:
        src_root = os.path.join(root, "in")
        os.makedirs(os.path.join(src_root, SUBSET, SPLIT, SENSOR))
        for k, n in enumerate(frames):
            write_pcm16(os.path.join(src_root, SUBSET, SPLIT, SENSOR, f"u{k:05d}.wav"), rng.randint(-3000, 3000, size=n), IN)
        audio_s = sum(frames) / IN
        outs = iter(os.path.join(root, f"out{k}") for k in range(10 ** 6))

        # ---- (a) and (b): disk to disk, alternating ---------------------------------------------------------------------------------------
        def disk_to_disk():
            out = next(outs)
            export.enhance_corpus({SENSOR: gen}, src_root, out, SUBSET, SPLIT)
            torch.cuda.synchronize()
            return out

        def parent():
            out = next(outs)
            c = corpus.ResidentCorpus.load(src_root, SUBSET, SPLIT, [SENSOR], MODEL, dev)
            enhanced = inference.enhance_clips(gen, c.clips(SENSOR))
            os.makedirs(os.path.join(out, SUBSET, SPLIT, SENSOR))
            for stem, y in zip(c.stems, enhanced):
                x = y.cpu().numpy()
                body = np.clip(np.rint(x * np.float32(32768)), -32768, 32767).astype("<i2").tobytes()
                head = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, MODEL, 2 * MODEL, 2, 16)
                with open(os.path.join(out, SUBSET, SPLIT, SENSOR, stem + ".wav"), "wb") as f:
                    f.write(head + b"data" + struct.pack("<I", len(body)) + body)
            torch.cuda.synchronize()
            return out

        def same_files(a: str, b: str) -> bool:
            da, db = os.path.join(a, SUBSET, SPLIT, SENSOR), os.path.join(b, SUBSET, SPLIT, SENSOR)
            names = sorted(os.listdir(da))
            return names == sorted(os.listdir(db)) and all(open(os.path.join(da, n), "rb").read() == open(os.path.join(db, n), "rb").read() for n in names)

        paths = [("load_enhance_clips_cpu_numpy_struct", parent), ("enhance_corpus", disk_to_disk)]
        first = {name: fn() for name, fn in paths}   # warm-up: page cache, code objects, pinned and device allocations
        equal = same_files(*first.values())
        out_bytes = sum(os.path.getsize(os.path.join(first["enhance_corpus"], SUBSET, SPLIT, SENSOR, n))
                        for n in os.listdir(os.path.join(first["enhance_corpus"], SUBSET, SPLIT, SENSOR)))
        for d in first.values():
            shutil.rmtree(d)
        times = {name: [] for name, _ in paths}
        for _ in range(args.iters):
            for name, fn in paths:
                t0 = time.perf_counter()
                d = fn()
                times[name].append(time.perf_counter() - t0)
                shutil.rmtree(d)
        for name, _ in paths:
            s = statistics.median(times[name])
            lines.append(dict(part="a" if name == "enhance_corpus" else "b", path=name, files=args.files, audio_seconds=round(audio_s, 1),
                              bytes_written=out_bytes, median_s=round(s, 3), min_s=round(min(times[name]), 3), max_s=round(max(times[name]), 3),
                              audio_seconds_per_second=round(audio_s / s, 1), files_equal=equal))
            print(json.dumps(lines[-1]), flush=True)

        # ---- (c) the encode launch alone on one batch buffer ----------------------------------------------------------------------------------
        n_rows = 256
        lens = [int(t) for t in np.random.RandomState(1).randint(1 * MODEL, 12 * MODEL + 1, size=n_rows)]
        pitch = max(lens) + 3   # no multiple of 4 floats: the rows start everywhere on the 4-byte grid
        buf = 0.3 * torch.randn((n_rows, pitch), device=dev)
        up_lens = [inference.resampled_length(t, MODEL, IN) for t in lens]
        kpaths, keep = [], []
        for fmt, counts, label in (("PCM16", lens, "encode_pcm16"), ("FLOAT32", lens, "encode_float32"), ("PCM16", up_lens, "resample_ragged_16_to_48_then_encode_pcm16")):
            (group,) = corpus.plan_image(counts, fmt, 1 << 34)
            image = torch.empty(group.nbytes, dtype=torch.uint8, device=dev)
            clipped = torch.empty(n_rows, dtype=torch.int32, device=dev)
            table = np.zeros(n_rows, dtype=corpus.ENC_ROW_DTYPE)
            width = corpus.BYTES_PER_SAMPLE[fmt]
            if counts is lens:
                for r in range(n_rows):
                    table[r] = (r * pitch, group.starts[r] + corpus.HEADER_BYTES, counts[r], corpus.FORMATS.index(fmt))
                nbytes = (4 + width) * sum(counts)
                fn = (lambda table=table, image=image, clipped=clipped: corpus.rows_to_pcm(buf, table, image, clipped))
            else:
                up = torch.empty((n_rows, inference.resampled_length(pitch, MODEL, IN)), dtype=torch.float32, device=dev)
                for r in range(n_rows):
                    table[r] = (r * up.shape[1], group.starts[r] + corpus.HEADER_BYTES, counts[r], corpus.FORMATS.index(fmt))
                # resample: reads the rows, writes the whole padded rows; encode: reads the samples, writes their bytes
                nbytes = 4 * sum(lens) + 4 * up.numel() + (4 + width) * sum(counts)

                def fn(table=table, image=image, clipped=clipped, up=up):
                    rate.resample_ragged(buf, lens, MODEL, IN, out=up)
                    corpus.rows_to_pcm(up, table, image, clipped)
            a = torch.empty(nbytes // 8, device=dev)
            b = torch.empty_like(a)
            keep.append((image, clipped, a, b))
            kpaths.append((label, fn, nbytes))
            kpaths.append(("copy_of_the_bytes_of_" + label, (lambda a=a, b=b: b.copy_(a)), nbytes))
        for _, fn, _ in kpaths:
            fn()
        torch.cuda.synchronize()
        kt = {name: [] for name, _, _ in kpaths}
        for _ in range(args.kernel_iters):
            for name, fn, _ in kpaths:
                kt[name].append(timed(torch, fn))
        for name, _, nbytes in kpaths:
            ms = statistics.median(kt[name])
            lines.append(dict(part="c", path=name, rows=n_rows, bytes_read_plus_written=nbytes, median_ms=round(ms, 4), min_ms=round(min(kt[name]), 4),
                              max_ms=round(max(kt[name]), 4), gigabytes_per_second=round(nbytes / (ms * 1e-3) / 1e9, 1)))
            print(json.dumps(lines[-1]), flush=True)
        del keep, kpaths, buf

        # ---- (d) the stages of (a), one after the other ------------------------------------------------------------------------------------------
        stage = {k: [] for k in ("load", "forwards", "encode", "copy_to_pinned", "writes")}
        for it in range(args.iters + 1):   # the first pass warms up and is dropped
            def clock(name, t0):
                torch.cuda.synchronize()
                if it:
                    stage[name].append(time.perf_counter() - t0)

            t0 = time.perf_counter()
            c = corpus.ResidentCorpus.load(src_root, SUBSET, SPLIT, [SENSOR], MODEL, dev)
            clock("load", t0)
            clips = c.clips(SENSOR)
            lengths = [x.shape[-1] for x in clips]
            counts = [ragged.cut_length(gen, t) for t in lengths]
            (group,) = corpus.plan_image(counts, "PCM16", 1 << 34)
            t0 = time.perf_counter()
            with torch.no_grad():
                batches, _ = ragged.compose_batches(gen, lengths, inference.MAX_BATCH_SAMPLES)
                done = [(idx, plan, enh) for idx, plan, enh, _ in inference._batch_forwards(gen, clips, lengths, batches, False, None, MODEL)]
            clock("forwards", t0)
            image = torch.empty(group.nbytes, dtype=torch.uint8, device=dev)
            host = torch.empty(group.nbytes, dtype=torch.uint8, pin_memory=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for idx, plan, enh in done:
                table = np.zeros(len(idx), dtype=corpus.ENC_ROW_DTYPE)
                for r, i in enumerate(idx):
                    table[r] = (r * enh.shape[-1], group.starts[i] + corpus.HEADER_BYTES, counts[i], 0)
                corpus.rows_to_pcm(enh, table, image)
            clock("encode", t0)
            t0 = time.perf_counter()
            host.copy_(image, non_blocking=True)
            clock("copy_to_pinned", t0)
            out = next(outs)
            os.makedirs(os.path.join(out, SUBSET, SPLIT, SENSOR))
            view = memoryview(host.numpy())
            t0 = time.perf_counter()
            with concurrent.futures.ThreadPoolExecutor(max_workers=corpus.MAX_READ_THREADS) as pool:
                for k, stem in enumerate(c.stems):
                    a = group.starts[k]
                    host.numpy()[a:a + corpus.HEADER_BYTES] = np.frombuffer(corpus.wav_header(MODEL, counts[k], "PCM16"), dtype=np.uint8)
                    pool.submit(export._write_file, os.path.join(out, SUBSET, SPLIT, SENSOR, stem + ".wav"), view[a:a + corpus.HEADER_BYTES + 2 * counts[k]])
            clock("writes", t0)
            shutil.rmtree(out)
            del done, image, host, view, c, clips
        for name, ts in stage.items():
            lines.append(dict(part="d", stage=name, median_s=round(statistics.median(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4)))
            print(json.dumps(lines[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)

    by = {d.get("path", d.get("stage")): d for d in lines}
    a, b = by["enhance_corpus"], by["load_enhance_clips_cpu_numpy_struct"]
    summary = [
        f"export_bench on {torch.cuda.get_device_name(0)}: {a['files']} mono PCM16 recordings of 1-12 s at 48 kHz ({a['audio_seconds']} s of audio), "
        f"EBENGenerator(4, 32, 2), PCM16 files at 16 kHz ({a['bytes_written']} bytes)",
        f"  (a) enhance_corpus, disk to disk                 : {a['median_s']:8.3f} s  (min {a['min_s']}, max {a['max_s']}; host clock to the synchronise, medians of "
        f"{args.iters} alternated passes, files in the page cache): {a['audio_seconds_per_second']} audio-s/s",
        f"  (b) load, enhance_clips, .cpu(), numpy, struct   : {b['median_s']:8.3f} s  (min {b['min_s']}, max {b['max_s']}): {b['audio_seconds_per_second']} audio-s/s; "
        f"(a) / (b) = {a['median_s'] / b['median_s']:.3f}; files equal byte for byte: {a['files_equal']}",
    ]
    for label in ("encode_pcm16", "encode_float32", "resample_ragged_16_to_48_then_encode_pcm16"):
        k, cp = by[label], by["copy_of_the_bytes_of_" + label]
        summary.append(f"  (c) {label:45s}: {k['median_ms']:8.4f} ms  {k['gigabytes_per_second']} GB/s read + written ({k['bytes_read_plus_written']} bytes; "
                       f"copy of the same bytes {cp['median_ms']} ms, {cp['gigabytes_per_second']} GB/s)")
    total = sum(by[s]["median_s"] for s in ("load", "forwards", "encode", "copy_to_pinned", "writes"))
    summary.append("  (d) stages of (a), run one after the other       : " + ", ".join(f"{s} {by[s]['median_s']:.4f} s" for s in ("load", "forwards", "encode", "copy_to_pinned", "writes"))
                   + f"; sum {total:.3f} s against (a)'s {a['median_s']} s")
    print("\n".join(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(d) for d in lines) + "\n" + "\n".join(summary) + "\n")


if __name__ == "__main__":
    main()
