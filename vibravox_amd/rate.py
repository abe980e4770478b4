"""Input at the recording's rate: windowed-sinc resampling of ragged batches and of audio that is still arriving.

The reference's inference script puts ``torchaudio.transforms.Resample(48_000, 16_000)`` in front of every forward
(``scripts/eben_enhanced_vibravox.py``); here that step is ``augment.resample``'s arithmetic on two more buffer shapes, one kernel
family (``csrc/rate.hip``):

  * ``resample_ragged``: rows of different lengths in one padded buffer, each resampled as if alone, exact zeros behind every row -- it
    writes straight into the buffer ``EBENGenerator.forward_ragged`` reads;
  * ``StreamResampler``: a signal pushed chunk by chunk with carried state; the concatenation of what ``push`` and ``finish`` return is
    ``augment.resample`` of the whole signal, bit for bit.

With the rates reduced to ``orig : new`` and ``taps = 2 * width + orig``, output ``q * new + p`` sums the inputs ``q * orig - width + j``,
``j < taps``, and skips those outside the signal.  Everything below the two executors is arithmetic on positions (host only, no GPU):

  * finality: an output is final once every input it reads has arrived, so after ``n_in`` inputs ``final_outputs(n_in)`` =
    ``new * ((n_in - width) // orig)`` outputs are (all ``new`` phases of a ``q`` read the same inputs); at the end of the signal the rest
    follows, up to ``inference.resampled_length(total)``, against the zeros behind the signal's own end;
  * carry: the next output, ``q_next = emitted / new``, reads from ``q_next * orig - width`` on, so a push keeps the inputs from there --
    never more than ``taps - 1`` of them -- in front of the new chunk: the tape ``[carry | chunk]``;
  * buffer view: the tape holds the stream positions ``[pos0, pos0 + len)``.  Positions are Python ints and never reach the device: a
    launch gets the phase ``p0`` of its first output and the tape index ``base0 = q0 * orig - width - pos0`` of that output's tap 0, both
    small whatever the position, so a stream may run past 2^31 samples.

``Schedule`` turns a push into one ``RatePush`` of such buffer-relative numbers; ``StreamResampler`` executes it (``eben_stream_splice``
into the tape's ping-pong twin -- the carry is never updated by the launch that reads it -- then ``eben_resample_stream``);
``tests/rate_oracle.py`` executes it in float64.  ``ChunkFront`` is the resampler in front of a consumer of whole chunks
(``streaming.StreamingEnhancer(input_rate=...)``).  ``SlotFront`` is the same front for independent sessions in the slots of one state
(``streaming.StreamPool(input_rates=...)``): a ``Schedule`` and a parity per slot on the host, and two launches for all slots of a tick
(``eben_rate_splice_slots``, ``eben_resample_slots``: per-slot descriptors by value), executed by ``SlotTapes``.  ``SlotBack`` is its
mirror behind the model (``streaming.StreamPool(output_rates=...)``): a ``Schedule(model_rate, output_rate)`` and a parity per slot, and
ONE launch for all sessions of a run that splices, resamples and encodes to PCM bytes (``eben_stream_pcm_out``, ``csrc/stream_pcm.hip``),
executed by ``BackTapes``; ``pcm_chunks_in`` is the PCM front of a tick (``eben_pcm_chunks_in``).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import struct
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from .inference import resampled_length   # outputs of a whole signal: ceil(new * n_in / orig)

LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99   # augment.sinc_resample_kernel's defaults: the table augment.resample uses


def ratio(orig_freq: int, new_freq: int) -> Tuple[int, int, int]:
    """(orig, new, width) of ``augment.resample(x, orig_freq, new_freq)``: the reduced ratio and the table's half width in input samples."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"sample rates must be positive, got {orig_freq} and {new_freq}")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    return orig, new, math.ceil(LOWPASS_FILTER_WIDTH * orig / (min(orig, new) * ROLLOFF))


def final_outputs(n_in: int, orig: int, new: int, width: int) -> int:
    """Outputs that read nothing beyond the first ``n_in`` inputs: output q * new + p reads up to input q * orig + width + orig - 1."""
    n_in = int(n_in)
    return new * ((n_in - width) // orig) if n_in >= width else 0


def carry_start(emitted: int, orig: int, new: int, width: int) -> int:
    """The first input the output ``emitted`` reads (not below 0): what lies in front of it is never needed again."""
    return max(0, (emitted // new) * orig - width)


def tile(orig: int, new: int, width: int) -> dict:
    """The kernel's tile for a ratio (``eben_resample_plan``; no GPU needed): ``q_per_block``, ``outputs_per_block``, ``window_floats``
    of input staged in LDS and ``table_in_lds``."""
    from ._lib import check, load

    out = (ctypes.c_int * 4)()
    check(load().eben_resample_plan(orig, new, width, out, 4), "resample_plan")
    return dict(q_per_block=out[0], outputs_per_block=out[1], window_floats=out[2], table_in_lds=bool(out[3]))


@dataclasses.dataclass(frozen=True)
class RatePush:
    """One push in buffer-relative numbers: the new tape is ``[previous tape[prev_off : prev_off + n_carry] | the n_new pushed samples]``;
    on it, ``n_out`` outputs, the first of phase ``p0`` with its tap 0 at tape index ``base0``; ``end``: the tape's right end is the
    signal's own."""
    prev_off: int
    n_carry: int
    n_new: int
    p0: int
    base0: int
    n_out: int
    end: bool

    @property
    def length(self) -> int:
        return self.n_carry + self.n_new

    def piece(self, skip: int, orig: int, new: int) -> Tuple[int, int]:
        """(p0, base0) of a launch that starts at this push's output ``skip``."""
        q, p = divmod(self.p0 + skip, new)
        return p, self.base0 + q * orig


class Schedule:
    """Positions of one stream: ``push(n)`` / ``push(n, final=True)`` return the ``RatePush`` of that push; the executor owns the tapes.
    After a final push the schedule is spent until ``reset()``."""

    def __init__(self, orig_freq: int, new_freq: int):
        self.orig, self.new, self.width = ratio(orig_freq, new_freq)
        if self.orig == self.new:
            raise ValueError(f"nothing to resample: {orig_freq} Hz -> {new_freq} Hz")
        self.taps = 2 * self.width + self.orig
        self.reset()

    def reset(self) -> None:
        self.pushed = 0      # inputs so far
        self.emitted = 0     # outputs handed out
        self.start = 0       # stream position of the tape's first sample
        self.finished = False

    @property
    def lookahead(self) -> int:
        """Input samples past an output's own position that its value depends on, at most."""
        return self.width + self.orig - 1

    def push(self, n_in: int, final: bool = False) -> RatePush:
        n_in = int(n_in)
        if self.finished:
            raise RuntimeError("this stream has finished; reset() starts a new one")
        if n_in < 0:
            raise ValueError(f"a push takes a number of samples, got {n_in}")
        total = self.pushed + n_in
        target = resampled_length(total, self.orig, self.new) if final else final_outputs(total, self.orig, self.new, self.width)
        q0, p0 = divmod(self.emitted, self.new)
        keep = carry_start(self.emitted, self.orig, self.new, self.width)
        if not self.start <= keep <= self.pushed:
            raise RuntimeError(f"rate schedule: the tape holds [{self.start}, {self.pushed}), the next output reads from {keep}")
        op = RatePush(keep - self.start, self.pushed - keep, n_in, p0, q0 * self.orig - self.width - keep, target - self.emitted, bool(final))
        if op.n_carry > self.taps - 1:
            raise RuntimeError(f"rate schedule: a carry of {op.n_carry} samples, more than taps - 1 = {self.taps - 1}")
        self.pushed, self.emitted, self.start, self.finished = total, target, keep, bool(final)
        return op

    def advance(self, n_in: int) -> None:
        """The state ``n_in`` further inputs would have left, a whole number of ``orig``, without their operations: once the carry no
        longer starts at position 0 every position moves with the input and the buffer-relative numbers repeat."""
        n_in = int(n_in)
        if n_in < 0 or n_in % self.orig:
            raise ValueError(f"advance takes a whole number of {self.orig} input samples, got {n_in}")
        if self.finished:
            raise RuntimeError("this stream has finished; reset() starts a new one")
        if (self.emitted // self.new) * self.orig < self.width:
            raise RuntimeError("advance: the stream is still at its left edge (the next output reads in front of position 0)")
        k = n_in // self.orig
        self.pushed, self.emitted, self.start = self.pushed + n_in, self.emitted + k * self.new, self.start + n_in


def input_chunk_samples(chunk_samples: int, orig_freq: int, new_freq: int, multiple: int = 1) -> int:
    """Input samples per push that become exactly ``chunk_samples`` at the new rate: ``chunk_samples * orig / new``.  ``ValueError``
    naming the smallest ``chunk_samples`` that works (a multiple of ``multiple`` too) when that is no integer."""
    orig, new, _ = ratio(orig_freq, new_freq)
    chunk_samples = int(chunk_samples)
    if chunk_samples <= 0 or (chunk_samples * orig) % new:
        least = multiple * new // math.gcd(multiple, new)
        raise ValueError(f"chunk_samples = {chunk_samples} at {new_freq} Hz is {chunk_samples} * {orig} / {new} samples at {orig_freq} Hz, not a whole "
                         f"number: the smallest chunk_samples that works is {least}")
    return chunk_samples * orig // new


# ---- the executors ---------------------------------------------------------------------------------------------------------------------
def _table(orig_freq: int, new_freq: int, device):
    """``augment.resample``'s own table for the pair of rates, from its cache."""
    from . import augment

    key = (int(orig_freq), int(new_freq), device)
    if key not in augment._kernel_cache:
        augment._kernel_cache[key] = augment.sinc_resample_kernel(orig_freq, new_freq, device=device)
    return augment._kernel_cache[key]


def _rows_of(x, what: str, rows: Optional[int] = None):
    """``x`` as (rows, samples): a contiguous float32 (rows, T) or (rows, 1, T) tensor on a HIP device."""
    from ._lib import EbenError

    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1) or x.dtype is not torch.float32 or (
            rows is not None and x.shape[0] != rows):
        got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{what}: expected a float32 ({'rows' if rows is None else rows}, T) or ({'rows' if rows is None else rows}, 1, T) tensor, got {got}")
    if not x.is_cuda:
        raise EbenError(f"{what} runs only on an MI355X HIP device (got a tensor on '{x.device}'); there is no CPU path")
    return x.contiguous().reshape(x.shape[0], x.shape[-1])


def resample_ragged(x: torch.Tensor, lengths, orig_freq: int, new_freq: int, out: Optional[torch.Tensor] = None):
    """Row r of ``x`` (rows, T) or (rows, 1, T) holds a signal of ``lengths[r]`` samples (what lies behind is never read: it may be
    anything).  Returns ``(out, out_lengths)``: ``out[r]`` starts with ``augment.resample`` of that signal alone, bit for bit,
    ``out_lengths[r] = ceil(new * lengths[r] / orig)`` samples (int32, on the device), and is exactly zero behind them up to the row's
    end.  ``lengths``: a sequence of ints, checked here and copied ``non_blocking``, or an int32 device tensor used as it is (the kernel
    clamps each entry into [0, T]).  ``out``: a contiguous float32 buffer of the same rank and rows, at least
    ``ceil(new * T / orig)`` samples a row (default: exactly that); one launch, nothing waits for the device."""
    from ._lib import check, load, ptr, stream

    orig, new, width = ratio(orig_freq, new_freq)
    if orig == new:
        raise ValueError(f"resample_ragged: nothing to resample: {orig_freq} Hz -> {new_freq} Hz")
    x2 = _rows_of(x, "resample_ragged")
    rows, t = x2.shape
    if t < 1:
        raise ValueError("resample_ragged: rows of no samples")
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype is not torch.int32 or tuple(lengths.shape) != (rows,) or lengths.device != x.device or not lengths.is_contiguous():
            raise ValueError(f"resample_ragged: a length table must be a contiguous int32 ({rows},) tensor on {x.device}, got {lengths.dtype} "
                             f"{tuple(lengths.shape)} on {lengths.device}")
        lens = lengths
    else:
        lengths = [int(v) for v in lengths]
        if len(lengths) != rows:
            raise ValueError(f"resample_ragged: {len(lengths)} lengths for {rows} rows")
        for r, v in enumerate(lengths):
            if not 0 <= v <= t:
                raise ValueError(f"resample_ragged: row {r} is said to hold {v} samples of a buffer of {t}")
        lens = torch.tensor(lengths, dtype=torch.int32).to(x.device, non_blocking=True)
    need = resampled_length(t, orig, new)
    if out is None:
        out = torch.empty(x.shape[:-1] + (need,), dtype=torch.float32, device=x.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype is not torch.float32 or out.device != x.device or not out.is_contiguous()
          or out.dim() not in (2, 3) or out.shape[0] != rows or out.numel() != rows * out.shape[-1] or out.shape[-1] < need):
        got = f"{out.dtype} {tuple(out.shape)}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"resample_ragged: out must be a contiguous float32 ({rows}, >= {need}) or ({rows}, 1, >= {need}) tensor on {x.device}, got {got}")
    out_lens = torch.empty(rows, dtype=torch.int32, device=x.device)
    table = _table(orig_freq, new_freq, x.device)[0]
    check(load().eben_resample_ragged(ptr(x2), lens.data_ptr(), ptr(table), ptr(out), out_lens.data_ptr(), rows, t, out.shape[-1], orig, new, width,
                                      stream()), "resample_ragged")
    return out, out_lens


class StreamResampler:
    """``augment.resample(signal, orig_freq, new_freq)`` on a signal that is still arriving, ``rows`` signals in lockstep: ``push`` a
    float32 device chunk (rows, n) or (rows, 1, n) and get the newly final samples, ``final_outputs`` of everything pushed less what was
    returned before; ``finish(tail=None)`` returns the rest, up to ``resampled_length(total)``.  The concatenation is the whole-signal
    call's result bit for bit.  ``reset()`` starts a new stream on the same state.  The state -- two tapes of ``taps - 1`` carried samples
    plus a chunk -- is allocated once, by ``prepare`` or at the first push for that push's length (``chunk_samples``: the longest chunk
    to come); a longer chunk later is refused.  Nothing here waits for the device."""

    def __init__(self, orig_freq: int, new_freq: int, rows: int = 1, chunk_samples: Optional[int] = None):
        if int(rows) < 1:
            raise ValueError(f"rows must be positive, got {rows}")
        self.orig_freq, self.new_freq, self.rows = int(orig_freq), int(new_freq), int(rows)
        self.schedule = Schedule(orig_freq, new_freq)
        self.chunk_samples = None if chunk_samples is None else int(chunk_samples)
        if self.chunk_samples is not None and self.chunk_samples < 1:
            raise ValueError(f"chunk_samples must be positive, got {chunk_samples}")
        self.state: Optional[List[torch.Tensor]] = None   # the tape and its twin, (rows, taps - 1 + chunk_samples) each
        self._cur = 0
        self._table = None

    def prepare(self, device, chunk_samples: Optional[int] = None) -> "StreamResampler":
        """Allocates the state on ``device`` now instead of at the first push (it is allocated once either way)."""
        device = torch.empty(0, device=device).device
        if self.state is not None and self.state[0].device == device:
            return self
        if chunk_samples is not None:
            self.chunk_samples = int(chunk_samples)
        if self.chunk_samples is None or self.chunk_samples < 1:
            raise ValueError("StreamResampler: prepare needs chunk_samples, the longest chunk to come")
        cap = self.schedule.taps - 1 + self.chunk_samples
        self.state = [torch.empty((self.rows, cap), dtype=torch.float32, device=device) for _ in range(2)]
        self._table = _table(self.orig_freq, self.new_freq, device)[0]
        return self

    def reset(self) -> None:
        self.schedule.reset()   # the first push of a stream carries nothing over: the tapes need no clearing

    def _advance(self, chunk: Optional[torch.Tensor], final: bool):
        """Splices ``chunk`` (rows, n) behind the carry into the twin tape; returns (tape, the push's ``RatePush``)."""
        from ._lib import check, load, ptr, stream

        n = 0 if chunk is None else chunk.shape[1]
        if self.state is None:
            if chunk is None:
                raise ValueError("StreamResampler: nothing was pushed")
            self.prepare(chunk.device, self.chunk_samples if self.chunk_samples is not None else n)
        if n > self.chunk_samples:
            raise ValueError(f"StreamResampler: a chunk of {n} samples, the state was allocated for {self.chunk_samples}")
        op = self.schedule.push(n, final)
        prev, dst = self.state[self._cur], self.state[self._cur ^ 1]
        if op.length:
            cap = dst.shape[1]
            check(load().eben_stream_splice(ptr(dst), cap, ptr(prev) if op.n_carry else None, cap if op.n_carry else 0, op.prev_off, op.n_carry,
                                            ptr(chunk) if n else None, n, 0, n, None, 0, 0, self.rows, stream()), "stream_splice")
            self._cur ^= 1
        return dst, op

    def _emit(self, tape: torch.Tensor, op: RatePush, out: torch.Tensor, out_pitch: int, first_out: int, skip: int, count: int) -> None:
        """Outputs [skip, skip + count) of push ``op`` to ``out[r, first_out : first_out + count]`` (rows of ``out_pitch`` floats)."""
        from ._lib import check, load, ptr, stream

        if count == 0:
            return
        s = self.schedule
        p0, base0 = op.piece(skip, s.orig, s.new)
        check(load().eben_resample_stream(ptr(tape), ptr(self._table), ptr(out), self.rows, tape.shape[1], op.length, out_pitch, first_out, count, p0,
                                          base0, 1 if op.end else 0, s.orig, s.new, s.width, stream()), "resample_stream")

    def _run(self, chunk, final: bool):
        lead = (self.rows,) if chunk is None or chunk.dim() == 2 else (self.rows, 1)
        c2 = None if chunk is None else _rows_of(chunk, "StreamResampler", self.rows)
        if c2 is not None and c2.shape[1] == 0:
            c2 = None
        if c2 is None and self.state is None:
            raise ValueError("StreamResampler: nothing was pushed")
        tape, op = self._advance(c2, final)
        out = torch.empty(lead + (op.n_out,), dtype=torch.float32, device=tape.device)
        self._emit(tape, op, out, max(op.n_out, 1), 0, 0, op.n_out)
        return out

    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        return self._run(chunk, False)

    def finish(self, tail: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._run(tail, True)


class ChunkFront:
    """A ``StreamResampler`` in front of a consumer of whole chunks of ``chunk_samples`` at the new rate: the final samples wait in a
    device FIFO -- two buffers of exactly one chunk, filled in place by the resampling launches -- and each full one is handed to
    ``sink`` at once (the other buffer is filled meanwhile; everything is ordered by the stream)."""

    def __init__(self, orig_freq: int, new_freq: int, chunk_samples: int, rows: int, multiple: int = 1):
        self.chunk_samples = int(chunk_samples)
        self.input_chunk_samples = input_chunk_samples(chunk_samples, orig_freq, new_freq, multiple)
        self.resampler = StreamResampler(orig_freq, new_freq, rows, self.input_chunk_samples)
        s = self.resampler.schedule
        self.lag = self.chunk_samples - final_outputs(self.input_chunk_samples, s.orig, s.new, s.width)   # outputs a steady push is behind by
        if not 0 < self.lag < self.chunk_samples:
            raise ValueError(f"chunk_samples = {chunk_samples} does not cover the resampler's look-ahead of {s.lookahead} input samples")
        self.rows = int(rows)
        self.fifo: Optional[List[torch.Tensor]] = None
        self.reset()

    def reset(self) -> None:
        self.resampler.reset()
        self.held, self._cur = 0, 0

    @property
    def pushed(self) -> int:
        return self.resampler.schedule.pushed

    def prepare(self, device) -> None:
        device = torch.empty(0, device=device).device
        if self.fifo is None or self.fifo[0].device != device:
            self.resampler.prepare(device)
            self.fifo = [torch.empty((self.rows, 1, self.chunk_samples), dtype=torch.float32, device=device) for _ in range(2)]

    def feed(self, chunk: Optional[torch.Tensor], final: bool, sink: Callable[[torch.Tensor], None]) -> Optional[torch.Tensor]:
        """``chunk`` (rows, 1, n) at the input rate, or None; every chunk the FIFO fills goes to ``sink``.  With ``final`` returns what is
        left, (rows, 1, r) with r < chunk_samples, or None when nothing is."""
        c2 = None if chunk is None else chunk.reshape(self.rows, chunk.shape[-1])
        tape, op = self.resampler._advance(c2, final)
        done = 0
        while done < op.n_out:
            take = min(self.chunk_samples - self.held, op.n_out - done)
            self.resampler._emit(tape, op, self.fifo[self._cur], self.chunk_samples, self.held, done, take)
            self.held, done = self.held + take, done + take
            if self.held == self.chunk_samples:
                sink(self.fifo[self._cur])
                self.held, self._cur = 0, self._cur ^ 1
        if not final or self.held == 0:
            return None
        return self.fifo[self._cur][:, :, : self.held].contiguous()


# ---- independent sessions in the slots of one state (streaming.StreamPool with input_rates) -------------------------------------------
class SlotSplice(NamedTuple):
    """Slot ``slot``: tape ``tape`` := ``[the other tape[prev_off : prev_off + n_carry] | row src_row of the compact input, n_new samples]``.
    The compact input of a tick holds one row per splice of the same ``n_new``, in the order of the list (sessions at different rates
    push chunks of different lengths: each length is a compact input of its own)."""
    slot: int
    src_row: int
    prev_off: int
    n_carry: int
    n_new: int
    tape: int


class SlotPiece(NamedTuple):
    """``n_out`` outputs of slot ``slot``'s tape ``tape`` (``length`` samples) at ratio ``ratio`` to FIFO buffer ``fifo``, from
    ``first_out`` on; ``p0``, ``base0``, ``end`` as in ``RatePush``."""
    slot: int
    ratio: int
    tape: int
    length: int
    p0: int
    base0: int
    n_out: int
    end: bool
    fifo: int
    first_out: int


class SlotChunk(NamedTuple):
    """What a slot's FIFO hands on: the first ``samples`` of its buffer ``fifo`` -- a whole chunk, or the shorter rest at the end."""
    slot: int
    fifo: int
    samples: int


@dataclasses.dataclass
class _Slot:
    ratio: int
    schedule: Schedule
    tape: int = 0      # the current tape of the slot's two
    fifo: int = 0      # the FIFO buffer being filled ...
    held: int = 0      # ... and the samples it holds
    last: Optional[RatePush] = None     # the latest push
    steady: Optional[RatePush] = None   # the push that repeats, once two in a row were equal past the left edge
    replay: dict = dataclasses.field(default_factory=dict)   # tape parity -> (splice numbers, pieces, chunks) of a steady push
    lazy: int = 0      # steady pushes the schedule has not been advanced by yet


class SlotFront:
    """``ChunkFront``'s bookkeeping per slot (host only, no GPU needed): every slot has a ``Schedule`` of its own ratio and its own parity
    of tapes and FIFO buffers, so a slot that does not push costs nothing.  ``feed`` turns the pushes of a tick into the descriptor
    lists of ``eben_rate_splice_slots`` and ``eben_resample_slots`` and the chunks each FIFO completed; ``SlotTapes`` executes them on
    the device, ``tests/pool_rate_oracle.py`` in float64."""

    def __init__(self, chunk_samples: int, slots: int, input_rates, model_rate: int = 16000, multiple: int = 1):
        from ._lib import RATE_MAX_RATIOS

        self.chunk_samples, self.slots, self.model_rate = int(chunk_samples), int(slots), int(model_rate)
        self.rates: List[int] = []                 # the declared rates that need resampling; a slot's ``ratio`` indexes these lists
        self.ratios: List[Tuple[int, int, int]] = []
        self.input_chunk: List[int] = []
        for r in input_rates:
            r = int(r)
            if r == self.model_rate or r in self.rates:
                continue
            n_in = input_chunk_samples(self.chunk_samples, r, self.model_rate, multiple)
            orig, new, width = ratio(r, self.model_rate)
            lag = self.chunk_samples - final_outputs(n_in, orig, new, width)
            if not 0 < lag < self.chunk_samples:
                raise ValueError(f"chunk_samples = {chunk_samples} does not cover the look-ahead of {width + orig - 1} input samples at {r} Hz")
            self.rates.append(r)
            self.ratios.append((orig, new, width))
            self.input_chunk.append(n_in)
        if len(self.rates) > RATE_MAX_RATIOS:
            raise ValueError(f"{len(self.rates)} input rates to resample, at most {RATE_MAX_RATIOS}")
        self.tape_samples = max((2 * w + o - 1 + n for (o, _, w), n in zip(self.ratios, self.input_chunk)), default=0)
        self.slot: List[Optional[_Slot]] = [None] * self.slots

    def open(self, slot: int, input_rate: int) -> None:
        """Slot ``slot`` starts a stream at ``input_rate`` (one of ``rates``): nothing is carried over, the tapes need no clearing."""
        self.slot[slot] = _Slot(self.rates.index(int(input_rate)), Schedule(input_rate, self.model_rate))

    def release(self, slot: int) -> None:
        self.slot[slot] = None

    def outputs_after(self, slot: int, n_tail: int) -> int:
        """Samples at the model's rate of the slot's whole stream if it ended with ``n_tail`` more input samples."""
        st = self.slot[slot]
        pushed = st.schedule.pushed + st.lazy * self.input_chunk[st.ratio]
        return resampled_length(pushed + int(n_tail), st.schedule.orig, st.schedule.new)

    def _apply(self, slot: int, st: _Slot, op: RatePush, final: bool):
        """Push ``op`` on the slot's tapes and FIFO: (the splice's numbers behind slot and row, or None; its pieces; its chunks)."""
        c = self.chunk_samples
        orig, new, _ = self.ratios[st.ratio]
        splice = None
        if op.length:
            st.tape ^= 1
            splice = (op.prev_off, op.n_carry, op.n_new, st.tape)
        pieces, out, done = [], [], 0
        while done < op.n_out:
            take = min(c - st.held, op.n_out - done)
            p0, base0 = op.piece(done, orig, new)
            pieces.append(SlotPiece(slot, st.ratio, st.tape, op.length, p0, base0, take, op.end, st.fifo, st.held))
            st.held, done = st.held + take, done + take
            if st.held == c:
                out.append(SlotChunk(slot, st.fifo, c))
                st.held, st.fifo = 0, st.fifo ^ 1
        if final and st.held:
            out.append(SlotChunk(slot, st.fifo, st.held))
        return splice, pieces, out

    def feed(self, pushes, final: bool = False):
        """``pushes``: (slot, samples pushed) per session, each slot once.  Returns ``(splices, pieces, chunks)``: the two descriptor lists
        and per slot the ``SlotChunk`` its FIFO completed, in order -- none at a stream's first push, one at every later push, and with
        ``final`` possibly a whole chunk and then the shorter rest.

        Once a slot's carry no longer starts at position 0 its ``RatePush`` repeats (every position moves with the input), and with it
        the descriptors, up to the parity of tapes and FIFO buffers: a steady push replays them and costs a counter here; the schedule
        is advanced (``Schedule.advance``) when the stream ends."""
        splices: List[SlotSplice] = []
        pieces: List[SlotPiece] = []
        chunks: dict = {}
        rows: dict = {}   # pushed length -> rows of that compact input so far
        for slot, n_in in pushes:
            st, n_in = self.slot[slot], int(n_in)
            if slot in chunks or st is None:
                raise RuntimeError(f"rate front: slot {slot} is {'named twice' if slot in chunks else 'not open'}")
            whole = self.input_chunk[st.ratio]
            if not (0 <= n_in < whole if final else n_in == whole):
                raise ValueError(f"rate front: a push of slot {slot} takes {whole} samples, the final one fewer, got {n_in}")
            if st.steady is not None and not final:
                st.lazy += 1
                parity = st.tape ^ 1   # of the tape this push writes
                hit = st.replay.get(parity)
                if hit is None:
                    hit = st.replay[parity] = self._apply(slot, st, st.steady, False)
                else:   # what _apply does to the slot in the steady state: both parities flip, the FIFO holds what it held
                    st.tape, st.fifo = st.tape ^ 1, st.fifo ^ 1
                splice, mine, out = hit
            else:
                if st.lazy:
                    st.schedule.advance(st.lazy * whole)
                    st.lazy = 0
                op = st.schedule.push(n_in, final)
                s = st.schedule
                if not final and op == st.last and op.n_out == self.chunk_samples and (s.emitted // s.new) * s.orig >= s.width:
                    st.steady = op
                st.last = op
                splice, mine, out = self._apply(slot, st, op, final)
            if splice is not None:
                splices.append(SlotSplice(slot, rows.get(n_in, 0) if n_in else 0, *splice))
                if n_in:
                    rows[n_in] = rows.get(n_in, 0) + 1
            pieces.extend(mine)
            chunks[slot] = list(out)
        return splices, pieces, chunks


# EbenRateSplice and EbenRatePiece as bytes: a table of 128 descriptors packed this way costs a tenth of 128 ctypes constructors
_SPLICE_POD, _PIECE_POD = struct.Struct("=6i"), struct.Struct("=6i4B")


class SlotTapes:
    """The device state of a ``SlotFront`` and the executor of its lists: two tapes ``(slots, tape_samples)``, two FIFO buffers
    ``(slots, 1, chunk_samples)`` and the declared ratios' tables (``augment.resample``'s own), allocated here once."""

    def __init__(self, front: SlotFront, device):
        from ._lib import EbenRateRatio

        self.front, self.device = front, torch.empty(0, device=device).device
        self.tapes = [torch.empty((front.slots, front.tape_samples), dtype=torch.float32, device=self.device) for _ in range(2)]
        self.fifo = [torch.empty((front.slots, 1, front.chunk_samples), dtype=torch.float32, device=self.device) for _ in range(2)]
        self.tables = [_table(r, front.model_rate, self.device)[0] for r in front.rates]
        self.ratios = (EbenRateRatio * len(self.tables))(*[EbenRateRatio(t.data_ptr(), o, n, w, 0) for t, (o, n, w) in zip(self.tables, front.ratios)])
        self._rows = [f.split(1, dim=0) for f in self.fifo]   # a (1, 1, chunk_samples) view per buffer and slot, built once

    def chunk(self, c: SlotChunk) -> torch.Tensor:
        row = self._rows[c.fifo][c.slot]
        return row if c.samples == row.shape[2] else row[:, :, : c.samples]

    def run(self, splices, pieces, inputs: dict) -> None:
        """``inputs``: slot -> the (1, 1, n) chunk it pushes.  One splice launch per pushed length (and ``RATE_MAX_SPLICES`` slots), then one
        resampling launch per ``RATE_MAX_PIECES`` pieces; nothing waits."""
        from ._lib import RATE_MAX_PIECES, RATE_MAX_SPLICES, EbenRatePiece, EbenRateSplice, check, load, ptr, stream

        lib, f = load(), self.front
        by_length: dict = {}
        for s in splices:
            by_length.setdefault(s.n_new, []).append(s)
        for n_new, group in by_length.items():
            src = None
            if n_new:
                src = inputs[group[0].slot] if len(group) == 1 else torch.cat([inputs[s.slot] for s in group], dim=0)
            for i in range(0, len(group), RATE_MAX_SPLICES):
                part = group[i : i + RATE_MAX_SPLICES]
                table = (EbenRateSplice * len(part)).from_buffer_copy(b"".join([_SPLICE_POD.pack(*s) for s in part]))
                check(lib.eben_rate_splice_slots(ptr(self.tapes[0]), ptr(self.tapes[1]), f.tape_samples, f.slots, ptr(src), n_new, len(group), table,
                                                 len(part), stream()), "rate_splice_slots")
        for i in range(0, len(pieces), RATE_MAX_PIECES):
            part = pieces[i : i + RATE_MAX_PIECES]
            table = (EbenRatePiece * len(part)).from_buffer_copy(b"".join([_PIECE_POD.pack(p.length, p.p0, p.base0, p.n_out, p.end, p.first_out, p.slot,
                                                                                           p.ratio, p.tape, p.fifo) for p in part]))
            check(lib.eben_resample_slots(ptr(self.tapes[0]), ptr(self.tapes[1]), f.tape_samples, ptr(self.fifo[0]), ptr(self.fifo[1]), f.chunk_samples,
                                          f.slots, self.ratios, len(self.tables), table, len(part), stream()), "resample_slots")


# ---- the way out: sessions that leave as PCM at the caller's rate (streaming.StreamPool with output_rates) ----------------------------
class BackPiece(NamedTuple):
    """One session of one run, for ``eben_stream_pcm_out``: slot ``slot`` emitted row ``src_row`` of the run's compact output, ``n_new``
    samples at the model's rate.  ``ratio`` -1: they leave as they are (``n_out == n_new``).  Else tape ``tape`` of the slot :=
    ``[the other tape[prev_off : prev_off + n_carry] | those samples]`` and ``n_out`` outputs of it at ratio ``ratio`` with ``p0``,
    ``base0``, ``end`` as in ``RatePush``.  The outputs go to the image as ``format`` (an index of ``corpus.FORMATS``) from
    ``byte_offset`` on, a multiple of 16."""
    slot: int
    src_row: int
    ratio: int
    tape: int
    prev_off: int
    n_carry: int
    n_new: int
    p0: int
    base0: int
    n_out: int
    end: bool
    format: int
    byte_offset: int

    @property
    def nbytes(self) -> int:
        return self.n_out * PCM_BYTES[self.format]


PCM_FORMATS = ("PCM16", "PCM24", "PCM32", "FLOAT32")   # corpus.FORMATS: index = EBEN_PCM_*
PCM_BYTES = (2, 3, 4, 4)                               # bytes per sample


def pcm_format(format, who: str = "rate") -> int:
    """The index of a format name; ``ValueError`` naming the four that exist."""
    if format not in PCM_FORMATS:
        raise ValueError(f"{who}: format must be one of {', '.join(PCM_FORMATS)}, got {format!r}")
    return PCM_FORMATS.index(format)


@dataclasses.dataclass
class _BackSlot:
    ratio: int                      # -1: leaves at the model's rate
    schedule: Optional[Schedule]
    format: int
    tape: int = 0                   # the current tape of the slot's two


class SlotBack:
    """``SlotFront``'s mirror behind the model (host only, no GPU needed): every slot has a ``Schedule(model_rate, output_rate)`` and a
    parity of tapes of its own.  ``emit`` turns "slot s emitted k samples (final or not)" into the pieces of one ``eben_stream_pcm_out``
    call and the byte range of every session in one image: each session's bytes contiguous, each starting at a 16-byte boundary.
    ``BackTapes`` executes the pieces on the device.  Any ratio the kernels' tile admits may be declared: there is no whole-chunk
    condition on this side, the number of samples a push returns simply varies (``final_outputs``).  ``max_emit``: the most samples a
    slot emits in one run (a finish hands over the model's latency and a tail at once); the tapes are sized for it."""

    def __init__(self, chunk_samples: int, slots: int, output_rates, model_rate: int = 16000, max_emit: Optional[int] = None):
        from ._lib import RATE_MAX_RATIOS

        self.chunk_samples, self.slots, self.model_rate = int(chunk_samples), int(slots), int(model_rate)
        self.max_emit = max(self.chunk_samples, int(max_emit or 0))
        self.declared = tuple(int(r) for r in output_rates)
        self.rates: List[int] = []                 # the declared rates that need resampling; a slot's ``ratio`` indexes these lists
        self.ratios: List[Tuple[int, int, int]] = []
        for r in self.declared:
            if r == self.model_rate or r in self.rates:
                continue
            orig, new, width = ratio(self.model_rate, r)
            tile_of_back(orig, new, width)         # refuses a ratio that fits no tile, in the library's words
            self.rates.append(r)
            self.ratios.append((orig, new, width))
        if len(self.rates) > RATE_MAX_RATIOS:
            raise ValueError(f"{len(self.rates)} output rates to resample, at most {RATE_MAX_RATIOS}")
        self.tape_samples = max((2 * w + o - 1 + self.max_emit for o, _, w in self.ratios), default=0)
        self.slot: List[Optional[_BackSlot]] = [None] * self.slots

    def check(self, output_rate: Optional[int], format: Optional[str], who: str = "rate") -> Tuple[Optional[int], int]:
        """(the rate to resample to or None, the format's index) of a session that asks for ``output_rate`` and ``format``; ``ValueError``
        for a rate that was not declared or a format that does not exist.  Only a rate: FLOAT32."""
        fmt = pcm_format("FLOAT32" if format is None else format, who)
        if output_rate is None or int(output_rate) == self.model_rate:
            return None, fmt
        if int(output_rate) not in self.rates:
            raise ValueError(f"{who}: a session that leaves at {int(output_rate)} Hz in a pool that declared output_rates = {self.declared} "
                             f"(the model's {self.model_rate} Hz needs no declaration)")
        return int(output_rate), fmt

    def open(self, slot: int, output_rate: Optional[int], format: Optional[str]) -> None:
        """Slot ``slot`` starts a stream that leaves at ``output_rate`` as ``format``: nothing is carried over, the tapes need no clearing."""
        r, fmt = self.check(output_rate, format)
        self.slot[slot] = _BackSlot(-1, None, fmt) if r is None else _BackSlot(self.rates.index(r), Schedule(self.model_rate, r), fmt)

    def release(self, slot: int) -> None:
        self.slot[slot] = None

    def lookahead(self, slot: int) -> int:
        """Model-rate samples past an output's own position that its value depends on, at most."""
        st = self.slot[slot]
        return 0 if st.schedule is None else st.schedule.lookahead

    def emit(self, emits):
        """``emits``: (slot, row of the run's compact output, samples emitted, final) per session of one run, each slot once.
        Returns ``(pieces, ranges, image_bytes)``: the pieces of the call, per slot the ``(byte_offset, samples)`` of its outputs in the
        image, and the image's size.  A session that emitted nothing and goes on has no piece and an empty range."""
        pieces: List[BackPiece] = []
        ranges: dict = {}
        at = 0
        for slot, row, k, final in emits:
            st, k = self.slot[slot], int(k)
            if slot in ranges or st is None:
                raise RuntimeError(f"rate back: slot {slot} is {'named twice' if slot in ranges else 'not open'}")
            if not 0 <= k <= self.max_emit:
                raise RuntimeError(f"rate back: slot {slot} emitted {k} samples in one run, the tapes were sized for {self.max_emit}")
            at = -(-at // 16) * 16
            if st.schedule is None:
                piece = BackPiece(slot, row, -1, 0, 0, 0, k, 0, 0, k, bool(final), st.format, at) if k else None
            elif k == 0 and not final:
                piece = None
            else:
                op = st.schedule.push(k, final)
                if op.length:
                    st.tape ^= 1
                    piece = BackPiece(slot, row, st.ratio, st.tape, op.prev_off, op.n_carry, op.n_new, op.p0, op.base0, op.n_out, op.end, st.format, at)
                else:
                    piece = None
            if piece is None:
                ranges[slot] = (at, 0)
                continue
            pieces.append(piece)
            ranges[slot] = (at, piece.n_out)
            at += piece.nbytes
        return pieces, ranges, at


def tile_of_back(orig: int, new: int, width: int) -> dict:
    """``eben_stream_pcm_out``'s tile for a ratio (``eben_stream_pcm_plan``; no GPU needed): ``outputs_per_block``, ``window_floats`` of
    input staged in LDS and ``table_route`` (0 through L2, 1 in LDS, 2 in LDS with one value per tap).  (1, 1, 0): no resampling."""
    from ._lib import check, load

    out = (ctypes.c_int * 3)()
    check(load().eben_stream_pcm_plan(orig, new, width, out, 3), "stream_pcm_plan")
    return dict(outputs_per_block=out[0], window_floats=out[1], table_route=out[2])


_BACK_POD = struct.Struct("=7iH2Bb3B")   # EbenStreamPcmPiece as bytes


def pack_back_pieces(pieces):
    """The ``EbenStreamPcmPiece`` table of a list of ``BackPiece``."""
    from ._lib import EbenStreamPcmPiece

    return (EbenStreamPcmPiece * len(pieces)).from_buffer_copy(b"".join([_BACK_POD.pack(
        p.prev_off, p.n_carry, p.n_new, p.p0, p.base0, p.n_out, p.byte_offset, p.src_row, p.slot, p.tape, p.ratio, p.format, 1 if p.end else 0, 0) for p in pieces]))


class BackTapes:
    """The device state of a ``SlotBack`` and the executor of its pieces: two tapes ``(slots, tape_samples)``, the ``clipped`` table (int32,
    one counter per slot, accumulated by the kernel and zeroed when a slot is opened) and the declared ratios' tables
    (``augment.resample``'s own), allocated here once.  The image of a call is allocated by that call."""

    def __init__(self, back: SlotBack, device):
        from ._lib import EbenRateRatio

        self.back, self.device = back, torch.empty(0, device=device).device
        self.tapes = [torch.empty((back.slots, max(back.tape_samples, 1)), dtype=torch.float32, device=self.device) for _ in range(2)]
        self.clipped = torch.zeros(back.slots, dtype=torch.int32, device=self.device)
        self.tables = [_table(back.model_rate, r, self.device)[0] for r in back.rates]
        self.ratios = (EbenRateRatio * max(len(self.tables), 1))(*[EbenRateRatio(t.data_ptr(), o, n, w, 0) for t, (o, n, w) in zip(self.tables, back.ratios)])
        self._counts = self.clipped.unbind(0)   # a 0-dim view per slot, built once

    def count(self, slot: int) -> torch.Tensor:
        return self._counts[slot]

    def run(self, pieces, image_bytes: int, src: Optional[torch.Tensor], image: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``src``: the run's compact output (rows, 1, k) or (rows, k), or None when nothing was emitted.  Returns the image (uint8, 1-D,
        allocated here unless given); one launch per ``STREAM_PCM_MAX_PIECES`` pieces, nothing waits."""
        from ._lib import STREAM_PCM_MAX_PIECES, check, load, ptr, stream

        b = self.back
        if image is None:
            image = torch.empty(max(int(image_bytes), 16), dtype=torch.uint8, device=self.device)
        rows, pitch = (0, 0) if src is None else (src.shape[0], src.shape[-1])
        for i in range(0, len(pieces), STREAM_PCM_MAX_PIECES):
            part = pieces[i : i + STREAM_PCM_MAX_PIECES]
            check(load().eben_stream_pcm_out(ptr(self.tapes[0]), ptr(self.tapes[1]), self.tapes[0].shape[1], b.slots, ptr(src), pitch, rows, self.ratios,
                                             len(self.tables), image.data_ptr(), image.numel(), self.clipped.data_ptr(), pack_back_pieces(part), len(part),
                                             stream()), "stream_pcm_out")
        return image


def pcm_chunks_in(chunks, dst: torch.Tensor) -> None:
    """``eben_pcm_chunks_in``: ``chunks`` is a list of ``(bytes, samples, format index, dst_row)`` with ``bytes`` a uint8 device tensor (any
    alignment); row ``dst_row`` of the float32 ``(rows, pitch)`` buffer ``dst`` receives the converted samples.  One launch per
    ``PCM_MAX_CHUNKS`` chunks, nothing waits."""
    from ._lib import PCM_MAX_CHUNKS, EbenPcmChunk, check, load, ptr, stream

    for i in range(0, len(chunks), PCM_MAX_CHUNKS):
        part = chunks[i : i + PCM_MAX_CHUNKS]
        table = (EbenPcmChunk * len(part))(*[EbenPcmChunk(t.data_ptr(), n, f, r) for t, n, f, r in part])
        check(load().eben_pcm_chunks_in(table, len(part), ptr(dst), dst.shape[0], dst.shape[1], stream()), "pcm_chunks_in")
