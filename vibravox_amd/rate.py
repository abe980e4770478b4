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
(``streaming.StreamingEnhancer(input_rate=...)``).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Callable, List, Optional, Tuple

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
