"""Recordings on disk to clips resident in HBM: the layer between a directory of WAVE files and the on-device collators.

The reference gets its clips from the Hugging Face hub and decodes and resamples every item again every epoch in host workers; here
the corpus is decoded and resampled ONCE, on the device, and stays there: ``collate.bwe_collate`` then assembles every batch from views
into the store in the one gather launch it already is.

Host side (no GPU):

  * ``wav_info``: a RIFF/WAVE header reader for PCM16 / PCM24 / PCM32 / FLOAT32, plain or extensible headers;
  * ``scan``: ``root/<subset>/<split>/<sensor>/<stem>.wav``, the stems present under every requested sensor, paired and checked;
  * ``plan_store`` / ``plan_groups``: where every clip goes in the flat store, and which files travel together through the staging buffer;
  * ``epoch_plan``: an epoch's batches for one rank of a data-parallel run.

Device side: ``ResidentCorpus.load`` reads the files' ``data`` chunks as they lie on disk into a pinned staging buffer, uploads bytes and
descriptor tables in one copy per group, and converts them in one launch per (group, sensor, rate): ``eben_pcm_decode_ragged`` for
files already at the model's rate, ``eben_pcm_resample_ragged`` -- the conversion fused into ``rate.resample_ragged``'s kernel -- for the
others (``csrc/corpus.hip``).  Every clip is bit for bit ``augment.resample`` of the numpy-decoded file.

The way out (``export.enhance_corpus``, ``inference.enhance_to_pcm``) is the mirror image: ``wav_header`` writes the canonical mono
header, ``plan_image`` places files in group images with every data start on a 16-byte boundary, and ``rows_to_pcm``
(``eben_pcm_encode_ragged``, ``csrc/pcm_encode.hip``) converts rows of float32, where they lie, into the files' bytes in one launch.
"""
from __future__ import annotations

import concurrent.futures
import os
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .inference import resampled_length

SPLITS = ("train", "validation", "test")
AIRBORNE = "headset_microphone"
FORMATS = ("PCM16", "PCM24", "PCM32", "FLOAT32")          # index = EBEN_PCM_*
BYTES_PER_SAMPLE = {"PCM16": 2, "PCM24": 3, "PCM32": 4, "FLOAT32": 4}
MAX_READ_THREADS = 16
ALIGN = 16                                                # every chunk and table starts on a 16-byte boundary of the staging buffer

_PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # KSDATAFORMAT_SUBTYPE_*: the format tag, then these 14 bytes
ROW_DTYPE = np.dtype([("byte_offset", "<i8"), ("frames", "<i4"), ("channels", "<i4"), ("channel", "<i4"), ("format", "<i4")])   # EbenPcmRow
ENC_ROW_DTYPE = np.dtype([("src_offset", "<i8"), ("byte_offset", "<i8"), ("samples", "<i4"), ("format", "<i4")])   # EbenPcmEncRow


class WavInfo(NamedTuple):
    rate: int
    channels: int
    frames: int
    format: str        # one of FORMATS
    data_offset: int   # of the first frame, in the file
    data_bytes: int    # of whole frames


def wav_info(path: str) -> WavInfo:
    """``(rate, channels, frames, format, data_offset, data_bytes)`` of a RIFF/WAVE file, from its header alone.  Unknown chunks are
    skipped (with the pad byte behind an odd size); a ``data`` size of 0 or 0xFFFFFFFF means "to the end of the file".  ``ValueError``
    naming the file and what was found for anything that is not PCM16 / PCM24 / PCM32 / FLOAT32."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12:
            raise ValueError(f"{path}: a truncated header ({len(head)} bytes)")
        if head[:4] == b"RF64":
            raise ValueError(f"{path}: an RF64 file, not supported")
        if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file (starts with {head[:4]!r} ... {head[8:12]!r})")
        fmt = None
        pos = 12
        while True:
            f.seek(pos)
            ch = f.read(8)
            if len(ch) < 8:
                raise ValueError(f"{path}: a truncated header: no {'data' if fmt else 'fmt'} chunk before the end of the file")
            cid, csize = ch[:4], struct.unpack("<I", ch[4:])[0]
            body = pos + 8
            if cid == b"fmt ":
                raw = f.read(min(csize, 40))
                if csize < 16 or len(raw) < min(csize, 40):
                    raise ValueError(f"{path}: a truncated header: a fmt chunk of {csize} bytes, {len(raw)} of them in the file")
                tag, channels, rate, _, block, bits = struct.unpack("<HHIIHH", raw[:16])
                if tag == 0xFFFE:
                    if len(raw) < 40:
                        raise ValueError(f"{path}: a truncated header: an extensible fmt chunk of {csize} bytes")
                    sub = raw[24:40]
                    if sub[2:] != _PCM_GUID_TAIL:
                        raise ValueError(f"{path}: an extensible header with the unknown subformat {sub.hex()}")
                    tag = struct.unpack("<H", sub[:2])[0]
                fmt = (tag, channels, rate, block, bits)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: a data chunk in front of the fmt chunk")
                break
            pos = body + csize + (csize & 1)
    tag, channels, rate, block, bits = fmt
    name = {(1, 16): "PCM16", (1, 24): "PCM24", (1, 32): "PCM32", (3, 32): "FLOAT32"}.get((tag, bits))
    if name is None:
        what = {1: "PCM", 2: "ADPCM", 3: "float", 6: "A-law", 7: "mu-law", 17: "IMA ADPCM"}.get(tag, f"format tag {tag:#x}")
        raise ValueError(f"{path}: {bits}-bit {what}, not one of {', '.join(FORMATS)}")
    if channels < 1 or rate < 1:
        raise ValueError(f"{path}: {channels} channels at {rate} Hz")
    frame = channels * BYTES_PER_SAMPLE[name]
    if block != frame:
        raise ValueError(f"{path}: a block of {block} bytes for {channels} channels of {name}")
    avail = max(0, size - body)
    nbytes = avail if csize in (0, 0xFFFFFFFF) else csize
    if nbytes > avail:
        raise ValueError(f"{path}: a truncated file: the data chunk says {nbytes} bytes, {avail} are there")
    frames = nbytes // frame
    return WavInfo(rate, channels, frames, name, body, frames * frame)


HEADER_BYTES = 44   # of the canonical header ``wav_header`` writes


def wav_header(rate: int, frames: int, format: str) -> bytes:
    """The canonical 44-byte RIFF/WAVE header of a mono file of ``frames`` samples: a ``fmt`` chunk of 16 bytes (tag 1 for the PCM
    formats, 3 for FLOAT32) and the ``data`` chunk's 8 bytes; the samples follow.  ``wav_info`` of header + data returns
    ``(rate, 1, frames, format, 44, frames * bytes)``.  ``ValueError`` for a data chunk whose size does not fit 32 bits (no RF64, as in
    the reader)."""
    rate, frames = int(rate), int(frames)
    if format not in BYTES_PER_SAMPLE:
        raise ValueError(f"wav_header: format must be one of {', '.join(FORMATS)}, got {format!r}")
    if not 1 <= rate <= 0xFFFFFFFF // 4 or frames < 0:
        raise ValueError(f"wav_header: {frames} frames at {rate} Hz")
    width = BYTES_PER_SAMPLE[format]
    nbytes = frames * width
    if 36 + nbytes > 0xFFFFFFFF:
        raise ValueError(f"wav_header: {frames} frames of {format} are {nbytes} bytes of data, too many for the 32-bit sizes of a RIFF file (no RF64)")
    return (b"RIFF" + struct.pack("<I", 36 + nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3 if format == "FLOAT32" else 1, 1, rate, rate * width,
                                                                                 width, 8 * width) + b"data" + struct.pack("<I", nbytes))


class ImageGroup(NamedTuple):
    lo: int               # files [lo, hi) travel in this image
    hi: int
    starts: List[int]     # of each file (its header) in the image; its data starts HEADER_BYTES behind, on a 16-byte boundary
    nbytes: int           # of the image, a multiple of 16


def plan_image(sample_counts: Sequence[int], format: str, max_bytes: int) -> List[ImageGroup]:
    """The counterpart of ``plan_groups`` on the way out: consecutive runs of mono files of ``sample_counts`` samples whose spans fit
    ``max_bytes`` together, at most 65535 files a run.  A file is one contiguous slice ``[start, start + 44 + samples * bytes)`` of its
    group's image, placed so that its data starts on a 16-byte boundary (where ``eben_pcm_encode_ragged`` writes it); the header goes into
    the 44 bytes in front.  ``ValueError`` for a file that does not fit alone."""
    if format not in BYTES_PER_SAMPLE:
        raise ValueError(f"plan_image: format must be one of {', '.join(FORMATS)}, got {format!r}")
    width = BYTES_PER_SAMPLE[format]
    groups: List[ImageGroup] = []
    lo, starts, end = 0, [], 0
    for k, n in enumerate(sample_counts):
        n = int(n)
        if n < 0:
            raise ValueError(f"file {k} has {n} samples")
        body = n * width
        alone = _up(_up(HEADER_BYTES) + body)
        if alone > max_bytes:
            raise ValueError(f"file {k} needs {alone} bytes of staging, max_stage_bytes allows {max_bytes}")
        data = _up(end + HEADER_BYTES)
        if starts and (_up(data + body) > max_bytes or len(starts) >= 65535):
            groups.append(ImageGroup(lo, k, starts, _up(end)))
            lo, starts, data = k, [], _up(HEADER_BYTES)
        starts.append(data - HEADER_BYTES)
        end = data + body
    if starts:
        groups.append(ImageGroup(lo, len(sample_counts), starts, _up(end)))
    return groups


class Scan(NamedTuple):
    stems: List[str]                      # sorted, present under every sensor, with frames
    infos: Dict[str, List[WavInfo]]       # sensor -> one per stem
    paths: Dict[str, List[str]]
    skipped: List[str]                    # stems left out because a file of theirs has zero frames


def scan(root: str, subset: str, split: str, sensors: Sequence[str]) -> Scan:
    """The stems of ``root/<subset>/<split>/<sensor>/<stem>.wav`` present under every one of ``sensors``, sorted, with their headers.
    Raises when the files of one stem differ in rate or frame count (the reference's ``set_audio_duration`` assertion, before anything is
    uploaded).  Stems with a zero-frame file go to ``skipped``."""
    if split not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
    sensors = list(dict.fromkeys(sensors))
    if not sensors:
        raise ValueError("scan needs at least one sensor")
    found = []
    for s in sensors:
        d = os.path.join(root, subset, split, s)
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d}: no such directory (expected root/<subset>/<split>/<sensor>/<stem>.wav)")
        found.append({n[:-4] for n in os.listdir(d) if n.endswith(".wav")})
    stems, skipped = [], []
    infos: Dict[str, List[WavInfo]] = {s: [] for s in sensors}
    paths: Dict[str, List[str]] = {s: [] for s in sensors}
    for stem in sorted(set.intersection(*found)):
        ps = [os.path.join(root, subset, split, s, stem + ".wav") for s in sensors]
        each = [wav_info(p) for p in ps]
        for p, i in zip(ps[1:], each[1:]):
            if (i.rate, i.frames) != (each[0].rate, each[0].frames):
                raise ValueError(f"{stem}: {ps[0]} has {each[0].frames} frames at {each[0].rate} Hz, {p} has {i.frames} at {i.rate} Hz: the sensors "
                                 f"of a pair must have the same length")
        if any(i.frames == 0 for i in each):
            skipped.append(stem)
            continue
        stems.append(stem)
        for s, p, i in zip(sensors, ps, each):
            infos[s].append(i)
            paths[s].append(p)
    return Scan(stems, infos, paths, skipped)


def plan_store(infos: Sequence[WavInfo], sample_rate: int) -> Tuple[List[int], List[int]]:
    """``(offsets, lengths)`` of the clips in the flat store: a clip is ``resampled_length(frames, rate, sample_rate)`` samples and starts
    where the one before it ends; ``offsets`` has one more entry, the size of the store."""
    lengths = [i.frames if i.rate == sample_rate else resampled_length(i.frames, i.rate, sample_rate) for i in infos]
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    return offsets, lengths


def _up(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _group_bytes(n_rows: int, chunk_bytes: int) -> int:
    return _up(n_rows * ROW_DTYPE.itemsize) + _up(n_rows * 8) + chunk_bytes


def plan_groups(chunk_sizes: Sequence[int], max_bytes: int) -> List[Tuple[int, int]]:
    """Consecutive runs ``[lo, hi)`` of files whose chunks (each rounded up to 16 bytes) and tables fit ``max_bytes`` together, at most
    65535 files a run.  ``ValueError`` for a file that does not fit alone."""
    groups, lo, acc = [], 0, 0
    for k, b in enumerate(chunk_sizes):
        b = _up(b)
        if _group_bytes(1, b) > max_bytes:
            raise ValueError(f"file {k} needs {_group_bytes(1, b)} bytes of staging, max_stage_bytes allows {max_bytes}")
        if k > lo and (_group_bytes(k - lo + 1, acc + b) > max_bytes or k - lo >= 65535):
            groups.append((lo, k))
            lo, acc = k, 0
        acc += b
    if len(chunk_sizes) > lo:
        groups.append((lo, len(chunk_sizes)))
    return groups


def epoch_plan(n_items: int, batch_size: int, *, shuffle: bool = False, drop_last: bool = False, seed: int = 0, epoch: int = 0, rank: int = 0,
               world_size: int = 1) -> List[List[int]]:
    """The batches (lists of item indices) of one epoch for ``rank``.  The epoch's order is drawn once, from a generator of its own seeded
    by ``(seed, epoch)`` -- the same on every rank, and no draw is taken from the global generator the collators use; rank r takes the
    items ``r::world_size`` of it, and every rank is cut to the same number of items, hence of steps, so no rank waits in a gradient
    collective for one that has run out.  Without ``shuffle`` the order is the items' own."""
    n_items, batch_size, rank, world_size = int(n_items), int(batch_size), int(rank), int(world_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} of {world_size}")
    if shuffle:
        g = torch.Generator().manual_seed((int(seed) * 0x9E3779B1 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        order = torch.randperm(n_items, generator=g).tolist()
    else:
        order = list(range(n_items))
    per = n_items // world_size
    mine = order[rank::world_size][:per]
    steps = per // batch_size if drop_last else (per + batch_size - 1) // batch_size
    return [mine[s * batch_size:(s + 1) * batch_size] for s in range(steps)]


def _read_into(path: str, offset: int, dest: memoryview) -> None:
    with open(path, "rb", buffering=0) as f:
        f.seek(offset)
        got = 0
        while got < len(dest):
            n = f.readinto(dest[got:])
            if not n:
                raise IOError(f"{path}: {got} of {len(dest)} bytes of the data chunk could be read")
            got += n


def pcm_to_rows(data: torch.Tensor, rows: np.ndarray, *, rates: Optional[Tuple[int, int]] = None, offsets: Optional[Sequence[int]] = None,
                out: Optional[torch.Tensor] = None, pitch: Optional[int] = None):
    """The two entry points of ``csrc/corpus.hip`` on a byte buffer that is already on the device.  ``data``: a uint8 device tensor (its
    storage 16-byte aligned) holding the files' frames; ``rows``: a ``ROW_DTYPE`` array, one descriptor per row, uploaded here.
    ``rates=(orig_freq, new_freq)`` resamples on the way (``eben_pcm_resample_ragged``), else the rows are decoded only.  Padded form
    (``offsets`` None): returns ``(out (rows, pitch), out_lens int32 device)``, ``pitch`` by default the longest row.  Flat form:
    ``offsets[r]`` is where row r starts in the 1-D ``out`` (required); returns ``(out, None)``.  One launch, nothing waits."""
    from . import rate as _rate
    from ._lib import check, load, ptr, stream

    rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    n = len(rows)
    if data.dtype is not torch.uint8 or not data.is_cuda or not data.is_contiguous():
        raise ValueError(f"pcm_to_rows: data must be a contiguous uint8 device tensor, got {data.dtype} on {data.device}")
    rows_dev = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(data.device, non_blocking=True)
    if rates is not None:
        orig, new, width = _rate.ratio(*rates)
        if orig == new:
            raise ValueError(f"pcm_to_rows: nothing to resample: {rates[0]} Hz -> {rates[1]} Hz")
        count = lambda f: resampled_length(int(f), orig, new)   # noqa: E731
    else:
        count = int
    if offsets is None:
        if pitch is None:
            pitch = max(1, max((count(f) for f in rows["frames"]), default=1))
        if out is None:
            out = torch.empty((n, pitch), dtype=torch.float32, device=data.device)
        out_lens = torch.empty(n, dtype=torch.int32, device=data.device)
        off_host = off_dev = None
        extent, lens_ptr = int(pitch), out_lens.data_ptr()
    else:
        if out is None or out.dim() != 1:
            raise ValueError("pcm_to_rows: the flat form writes into a 1-D out")
        offs = np.ascontiguousarray(offsets, dtype="<i8")
        offs_dev = torch.from_numpy(offs).to(data.device, non_blocking=True)
        off_host, off_dev = offs.ctypes.data, offs_dev.data_ptr()
        out_lens, extent, lens_ptr = None, out.numel(), None
    lib = load()
    if rates is None:
        check(lib.eben_pcm_decode_ragged(data.data_ptr(), data.numel(), rows.ctypes.data, rows_dev.data_ptr(), off_host, off_dev, ptr(out), lens_ptr, n,
                                         extent, stream()), "pcm_decode_ragged")
    else:
        table = _rate._table(rates[0], rates[1], data.device)[0]
        check(lib.eben_pcm_resample_ragged(data.data_ptr(), data.numel(), rows.ctypes.data, rows_dev.data_ptr(), ptr(table), off_host, off_dev, ptr(out),
                                           lens_ptr, n, extent, orig, new, width, stream()), "pcm_resample_ragged")
    return out, out_lens


def rows_to_pcm(src: torch.Tensor, rows: np.ndarray, image: torch.Tensor, clipped: Optional[torch.Tensor] = None,
                gains: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``csrc/pcm_encode.hip`` on buffers that are on the device: the way back of ``pcm_to_rows``.  ``src``: a contiguous float32 device
    tensor of any shape, addressed flat; ``rows``: an ``ENC_ROW_DTYPE`` array, one descriptor per row (``src_offset`` in floats,
    ``byte_offset`` a multiple of 16, ``samples``, ``format`` an index of ``FORMATS``), uploaded here; ``image``: a contiguous uint8
    device tensor (its storage 16-byte aligned) that receives the rows' bytes and nothing else.  Returns ``clipped``, an int32 device
    tensor with the clipped-sample count of every row (allocated here unless given).  One launch, nothing waits.

    ``gains``: a contiguous float32 device tensor with one factor per row; every sample is then converted from ``x * gains[r]``, rounded
    to float32 first (``eben_pcm_encode_ragged_gain``, the same kernel body).  The table may come straight from
    ``metrics.loudness_gain``: only the kernel reads it."""
    from ._lib import check, load, ptr, stream

    rows = np.ascontiguousarray(rows, dtype=ENC_ROW_DTYPE)
    n = len(rows)
    if image.dtype is not torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError(f"rows_to_pcm: image must be a contiguous uint8 device tensor, got {image.dtype} on {image.device}")
    if clipped is None:
        clipped = torch.empty(n, dtype=torch.int32, device=image.device)
    elif clipped.dtype is not torch.int32 or tuple(clipped.shape) != (n,) or clipped.device != image.device or not clipped.is_contiguous():
        raise ValueError(f"rows_to_pcm: clipped must be a contiguous int32 ({n},) tensor on {image.device}, got {clipped.dtype} {tuple(clipped.shape)}")
    rows_dev = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(image.device, non_blocking=True)
    if gains is not None:
        if gains.dtype is not torch.float32 or tuple(gains.shape) != (n,) or gains.device != image.device or not gains.is_contiguous():
            raise ValueError(f"rows_to_pcm: gains must be a contiguous float32 ({n},) tensor on {image.device}, got {gains.dtype} {tuple(gains.shape)}")
        check(load().eben_pcm_encode_ragged_gain(ptr(src), src.numel(), rows.ctypes.data, rows_dev.data_ptr(), image.data_ptr(), image.numel(),
                                                 clipped.data_ptr(), gains.data_ptr(), n, stream()), "pcm_encode_ragged_gain")
        return clipped
    check(load().eben_pcm_encode_ragged(ptr(src), src.numel(), rows.ctypes.data, rows_dev.data_ptr(), image.data_ptr(), image.numel(), clipped.data_ptr(), n,
                                        stream()), "pcm_encode_ragged")
    return clipped


class ResidentCorpus:
    """One split of a corpus in HBM: per sensor one flat float32 tensor at ``sample_rate`` holding every clip one behind the other."""

    def __init__(self, stems: List[str], sample_rate: int, offsets: List[int], lengths: List[int], store: Dict[str, torch.Tensor], skipped: List[str]):
        self.stems, self.sample_rate, self.offsets, self.lengths, self.store, self.skipped = stems, sample_rate, offsets, lengths, store, skipped

    def __len__(self) -> int:
        return len(self.stems)

    @property
    def roles(self) -> List[str]:
        return list(self.store)

    def clip(self, i: int, role: str) -> torch.Tensor:
        """Clip ``i`` of sensor ``role``: a 1-D view into the store, what ``collate.bwe_collate`` takes."""
        if not -len(self.stems) <= i < len(self.stems):
            raise IndexError(f"clip {i} of {len(self.stems)}")
        i %= len(self.stems)
        return self.store[role][self.offsets[i]:self.offsets[i + 1]]

    def clips(self, role: str) -> List[torch.Tensor]:
        """All clips of a sensor, in ``stems`` order: the list ``inference.evaluate_clips`` / ``enhance_clips`` take."""
        return [self.clip(i, role) for i in range(len(self.stems))]

    @classmethod
    def load(cls, root: str, subset: str, split: str, sensors: Sequence[str], sample_rate: int, device="cuda",
             max_stage_bytes: int = 1 << 30, channel: int = 0) -> "ResidentCorpus":
        """Scans, allocates each sensor's store exactly once (its size is known from the headers) and fills it group by group: files are
        read by at most 16 threads straight into their aligned places of a pinned staging buffer (two halves of ``max_stage_bytes`` / 2
        when the corpus needs more than one group, so the reads of a group overlap the upload of the one before); one async copy uploads a
        group's bytes and tables; one launch per (group, sensor, rate) converts them.  Nothing on the device is per file, and nothing here
        waits for a kernel.  ``channel``: which channel of a multi-channel file is the sensor's signal."""
        from . import rate as _rate
        from ._lib import EbenError, check, load, ptr, stream

        sample_rate = int(sample_rate)
        device = torch.device(device)
        if device.type != "cuda":
            raise EbenError(f"ResidentCorpus.load runs only on an MI355X HIP device (got '{device}'); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        sc = scan(root, subset, split, sensors)
        roles = list(sc.infos)
        if not sc.stems:
            raise ValueError(f"{os.path.join(root, subset, split)}: no recording present under every one of {roles}")
        offsets, lengths = plan_store(sc.infos[roles[0]], sample_rate)
        for r in roles:
            for st, i in zip(sc.stems, sc.infos[r]):
                if channel >= i.channels:
                    raise ValueError(f"{st} ({r}): channel {channel} of a file with {i.channels}")
        # jobs in (role, item) order: a launch's rows then write ascending ranges of one store
        jobs = [(r, k) for r in roles for k in range(len(sc.stems))]
        sizes = [sc.infos[r][k].data_bytes for r, k in jobs]
        groups = plan_groups(sizes, max_stage_bytes)
        if len(groups) > 1:
            groups = plan_groups(sizes, max_stage_bytes // 2)
        half = max(_group_bytes(hi - lo, sum(_up(b) for b in sizes[lo:hi])) for lo, hi in groups)
        n_halves = 2 if len(groups) > 1 else 1
        need = 4 * offsets[-1] * len(roles) + half
        with torch.cuda.device(device):
            free, _ = torch.cuda.mem_get_info(device)
            if need > free:
                raise MemoryError(f"the corpus needs {need} bytes on {device} ({4 * offsets[-1]} per sensor for {len(roles)} sensors plus {half} of "
                                  f"staging), {free} are free: a corpus larger than HBM is out of scope")
            store = {r: torch.empty(offsets[-1], dtype=torch.float32, device=device) for r in roles}
            dev_stage = torch.empty(half, dtype=torch.uint8, device=device)
            host_stage = torch.empty(n_halves * half, dtype=torch.uint8, pin_memory=True)
            host_np = host_stage.numpy()
            copied = [None] * n_halves
            lib = load()
            with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_READ_THREADS, len(jobs))) as pool:
                for g, (lo, hi) in enumerate(groups):
                    h = g % n_halves
                    if copied[h] is not None:
                        copied[h].synchronize()   # the upload that read this half has finished (a copy, never a kernel)
                    n = hi - lo
                    base = h * half
                    rows = host_np[base:base + n * ROW_DTYPE.itemsize].view(ROW_DTYPE)
                    off_at = _up(n * ROW_DTYPE.itemsize)
                    outs = host_np[base + off_at:base + off_at + 8 * n].view("<i8")
                    at = off_at + _up(8 * n)
                    # rows of a group sorted by (role, rate): every launch's rows are one run of the table (jobs are in role order already)
                    order = sorted(range(lo, hi), key=lambda j: (roles.index(jobs[j][0]), sc.infos[jobs[j][0]][jobs[j][1]].rate, j))
                    place = {}
                    for j in range(lo, hi):
                        place[j] = at
                        at += _up(sizes[j])
                    reads = []
                    for row, j in enumerate(order):
                        r, k = jobs[j]
                        i = sc.infos[r][k]
                        rows[row] = (place[j], i.frames, i.channels, channel, FORMATS.index(i.format))
                        outs[row] = offsets[k]
                        reads.append(pool.submit(_read_into, sc.paths[r][k], i.data_offset, memoryview(host_np[base + place[j]:base + place[j] + sizes[j]])))
                    for fu in reads:
                        fu.result()
                    dev_stage[:at].copy_(host_stage[base:base + at], non_blocking=True)
                    copied[h] = torch.cuda.Event()
                    copied[h].record()
                    row = 0
                    while row < n:
                        r, k = jobs[order[row]]
                        rt = sc.infos[r][k].rate
                        end = row
                        while end < n and jobs[order[end]][0] == r and sc.infos[r][jobs[order[end]][1]].rate == rt:
                            end += 1
                        rows_host = rows.ctypes.data + row * ROW_DTYPE.itemsize
                        rows_dev = dev_stage.data_ptr() + row * ROW_DTYPE.itemsize
                        outs_host, outs_dev = outs.ctypes.data + 8 * row, dev_stage.data_ptr() + off_at + 8 * row
                        if rt == sample_rate:
                            check(lib.eben_pcm_decode_ragged(dev_stage.data_ptr(), at, rows_host, rows_dev, outs_host, outs_dev, ptr(store[r]), None,
                                                             end - row, offsets[-1], stream()), "pcm_decode_ragged")
                        else:
                            orig, new, width = _rate.ratio(rt, sample_rate)
                            table = _rate._table(rt, sample_rate, device)[0]
                            check(lib.eben_pcm_resample_ragged(dev_stage.data_ptr(), at, rows_host, rows_dev, ptr(table), outs_host, outs_dev,
                                                               ptr(store[r]), None, end - row, offsets[-1], orig, new, width, stream()),
                                  "pcm_resample_ragged")
                        row = end
            # dev_stage is released to torch's allocator here; the kernels queued on this stream still own it in stream order
        return cls(list(sc.stems), sample_rate, offsets, lengths, store, list(sc.skipped))
