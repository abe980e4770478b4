"""Enhanced recordings on disk: a split of a corpus through one trained EBEN generator per sensor, written as WAVE files.

The job the reference's inference script exists for (``scripts/eben_enhanced_vibravox.py``: one generator per body-conducted sensor over
a split, the results stored) from a directory to a directory: ``corpus.ResidentCorpus.load`` brings
``root/<subset>/<split>/<sensor>/<stem>.wav`` to the device, ``inference.enhance_to_pcm`` turns every sensor's clips into the bytes of
their files -- the conversion in one ``eben_pcm_encode_ragged`` launch per ragged batch, one copy per group to pinned memory -- and
writer threads put them under ``out_root/<subset>/<split>/<sensor>/<stem>.wav``, the same layout, so ``ResidentCorpus.load(out_root, ...)``
reads them back.

    python -m vibravox_amd.export --generator throat_microphone=DIR [--generator ...] ROOT OUT_ROOT SUBSET SPLIT [--format PCM16] [--output-rate 16000|input]
                               [--loudness -23 [--peak -1]]

``DIR`` is a ``save_pretrained`` directory of an ``EBENGenerator``.  Prints the report as JSON.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import json
import math
import os
import sys
from typing import Dict, List, Mapping, Optional, Union

import torch

from . import corpus as C
from .inference import MAX_BATCH_SAMPLES, enhance_to_pcm


def _write_file(path: str, data: memoryview) -> None:
    part = path + ".part"
    with open(part, "wb", buffering=0) as f:
        done = 0
        while done < len(data):
            done += f.write(data[done:])
    os.replace(part, path)   # a reader never sees a file that is not complete


def enhance_corpus(generators: Mapping[str, object], root: Union[str, "C.ResidentCorpus"], out_root: str, subset: str, split: str, *,
                   format: str = "PCM16", output_rate: Union[None, int, str] = None, model_rate: int = 16000, overwrite: bool = False,
                   max_stage_bytes: int = 1 << 30, channel: int = 0, max_batch_samples: int = MAX_BATCH_SAMPLES, device="cuda",
                   loudness: Optional[float] = None, peak: float = -1.0) -> Dict[str, dict]:
    """Every recording of ``root/<subset>/<split>/<sensor>/`` for the sensors of ``generators`` (sensor -> generator, on the device),
    enhanced by its sensor's generator and written to ``out_root/<subset>/<split>/<sensor>/<stem>.wav`` as a mono file of ``format``.

    ``root``: a directory, loaded with ``ResidentCorpus.load`` at ``model_rate`` (any of the four sample formats, any rate, resampled on
    the way in), or a ``ResidentCorpus`` that already holds the sensors at ``model_rate``.  ``output_rate``: None writes at the model's
    rate, as the reference does; a number writes ``augment.resample`` of every result at that rate; ``"input"`` writes every file at
    its recording's rate (needs the directory: a loaded corpus no longer knows it).  Each sensor runs in passes of its own through
    ``inference.enhance_to_pcm``, in groups of at most ``max_stage_bytes``; at most ``corpus.MAX_READ_THREADS`` threads write a group's
    files, each as ``<stem>.wav.part`` renamed when complete, while the device works on the next group.  ``overwrite=False``: raises
    ``FileExistsError`` before anything is loaded or computed when a target exists.

    Returns the report ``{sensor: {"files", "seconds", "rate" (None when per file), "format", "clipped": {stem: samples that left the
    format's range}, "skipped": stems the scan left out}}``.

    ``loudness`` (LUFS): every file is written at that integrated loudness (ITU-R BS.1770-4) with its sample peak at or below ``peak``
    dBFS, measured on the device at the rate it is written at and applied inside the encode launch
    (``inference.enhance_to_pcm(loudness=, peak=)``).  The report then also holds ``"loudness": {stem: [measured LUFS, gain in dB]}`` per
    sensor -- the level the generator produced and what was applied; a recording without a finite loudness reads ``[-inf, 0.0]``."""
    sensors = list(generators)
    if not sensors:
        raise ValueError("enhance_corpus: no generator")
    if format not in C.FORMATS:
        raise ValueError(f"enhance_corpus: format must be one of {', '.join(C.FORMATS)}, got {format!r}")
    model_rate = int(model_rate)
    if loudness is not None:
        loudness, peak = float(loudness), float(peak)
        if not (math.isfinite(loudness) and math.isfinite(peak)):
            raise ValueError(f"enhance_corpus: loudness and peak must be finite, got {loudness} LUFS and {peak} dBFS")
    per_file = isinstance(output_rate, str)
    if per_file and output_rate != "input":
        raise ValueError(f"enhance_corpus: output_rate is None, a rate or 'input', got {output_rate!r}")
    if isinstance(root, C.ResidentCorpus):
        loaded: Optional[C.ResidentCorpus] = root
        if per_file:
            raise ValueError("enhance_corpus: output_rate='input' needs the corpus directory: a loaded corpus does not keep its files' rates")
        if loaded.sample_rate != model_rate:
            raise ValueError(f"enhance_corpus: the corpus is at {loaded.sample_rate} Hz, the model at {model_rate}")
        missing = [s for s in sensors if s not in loaded.store]
        if missing:
            raise ValueError(f"enhance_corpus: the corpus holds {loaded.roles}, not {missing}")
        stems, skipped, in_rates = list(loaded.stems), list(loaded.skipped), None
    else:
        loaded = None
        sc = C.scan(root, subset, split, sensors)
        if not sc.stems:
            raise ValueError(f"{os.path.join(root, subset, split)}: no recording present under every one of {sensors}")
        stems, skipped = list(sc.stems), list(sc.skipped)
        in_rates = [i.rate for i in sc.infos[sensors[0]]]   # a stem's files have one rate (scan checks it)
    paths = {s: [os.path.join(out_root, subset, split, s, stem + ".wav") for stem in stems] for s in sensors}
    if not overwrite:
        for s in sensors:
            for p in paths[s]:
                if os.path.exists(p):
                    raise FileExistsError(f"{p} exists (overwrite=False); nothing was computed")
    if loaded is None:
        loaded = C.ResidentCorpus.load(root, subset, split, sensors, model_rate, device, max_stage_bytes=max_stage_bytes, channel=channel)
        if loaded.stems != stems:
            raise RuntimeError(f"enhance_corpus: {os.path.join(root, subset, split)} changed between the scan and the load")
    # passes: the clips that are written at one rate go through enhance_to_pcm together
    if per_file:
        passes = [(r, [k for k, v in enumerate(in_rates) if v == r]) for r in sorted(set(in_rates))]
    else:
        passes = [(model_rate if output_rate is None else int(output_rate), list(range(len(stems))))]
    if loudness is not None:
        for out_rate, _ in passes:
            if out_rate <= 0 or out_rate % 10:
                raise ValueError(f"enhance_corpus: loudness is measured over 100 ms hops, which {out_rate} Hz does not divide into whole samples")
    report: Dict[str, dict] = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(C.MAX_READ_THREADS, max(1, len(stems)))) as pool:
        for s in sensors:
            os.makedirs(os.path.join(out_root, subset, split, s), exist_ok=True)
            seconds, clipped_stems, level_stems = 0.0, {}, {}
            for out_rate, items in passes:
                clips = [loaded.clip(k, s) for k in items]
                for indices, image, spans, clipped, *levels in enhance_to_pcm(generators[s], clips, format=format, output_rate=out_rate,
                                                                              model_rate=model_rate, max_batch_samples=max_batch_samples,
                                                                              max_stage_bytes=max_stage_bytes, loudness=loudness, peak=peak):
                    view = memoryview(image.numpy())
                    writes = [pool.submit(_write_file, paths[s][items[i]], view[a:b]) for i, (a, b) in zip(indices, spans)]
                    for i, (a, b), c in zip(indices, spans, clipped):
                        seconds += (b - a - C.HEADER_BYTES) // C.BYTES_PER_SAMPLE[format] / out_rate
                        if c:
                            clipped_stems[stems[items[i]]] = c
                    for i, (lufs, g) in zip(indices, levels[0] if levels else ()):
                        level_stems[stems[items[i]]] = [lufs, 20.0 * math.log10(g) if g > 0.0 else float("-inf")]
                    for w in writes:   # the image is this group's until the generator is advanced: the next group is already queued on the device
                        w.result()
            report[s] = dict(files=len(stems), seconds=seconds, rate=None if per_file else passes[0][0], format=format,
                             clipped=dict(sorted(clipped_stems.items())), skipped=list(skipped))
            if loudness is not None:
                report[s]["loudness"] = dict(sorted(level_stems.items()))
    return report


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m vibravox_amd.export", description="Enhance a split of a corpus on disk and write the results as WAVE files.")
    ap.add_argument("--generator", action="append", required=True, metavar="SENSOR=DIR",
                    help="a save_pretrained directory of the EBENGenerator for that sensor; once per sensor")
    ap.add_argument("root")
    ap.add_argument("out_root")
    ap.add_argument("subset")
    ap.add_argument("split", choices=C.SPLITS)
    ap.add_argument("--format", default="PCM16", choices=C.FORMATS)
    ap.add_argument("--output-rate", default=None, help="a rate in Hz, or 'input' for each recording's own (default: the model's)")
    ap.add_argument("--model-rate", type=int, default=16000)
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                    help="write every file at this integrated loudness (ITU-R BS.1770-4), e.g. -23; default: the level the generator produced")
    ap.add_argument("--peak", type=float, default=-1.0, metavar="DBFS", help="with --loudness: the ceiling of a file's sample peak (default -1.0)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)

    from .torch_modules.dnn.eben_generator import EBENGenerator

    generators = {}
    for item in args.generator:
        sensor, sep, directory = item.partition("=")
        if not sep or not sensor or not directory:
            ap.error(f"--generator takes SENSOR=DIR, got {item!r}")
        generators[sensor] = EBENGenerator.from_pretrained(directory).to(args.device).eval()
    rate = args.output_rate if args.output_rate in (None, "input") else int(args.output_rate)
    report = enhance_corpus(generators, args.root, args.out_root, args.subset, args.split, format=args.format, output_rate=rate,
                            model_rate=args.model_rate, overwrite=args.overwrite, device=args.device, loudness=args.loudness, peak=args.peak)
    torch.cuda.synchronize()
    json.dump(report, sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
