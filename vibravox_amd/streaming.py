"""Streaming inference of the EBEN generator: audio that is still arriving, enhanced chunk by chunk with carried state.

The generator is a finite-context network.  A layer's output at position o reads only the input samples its taps reach, so once a
tensor is exact up to some frontier, every consumer can be run on ``[carry | new]`` -- the samples in front of the new ones that its
first new output still reaches, then the new ones -- and each sample of each layer is computed exactly once.  The conv kernels are
the whole-clip ones: they apply their edge rule at both ends of whatever buffer they get, so the outputs next to a buffer's ends
are junk unless the end is the stream's own (position 0, or the cut length after ``finish``), and the schedule keeps only the
outputs whose taps stay inside the buffer.

Everything here is arithmetic on positions (host only, no GPU needed):

  * ``nodes_of`` makes a stream node of every entry of the generator's layer table (``gen_layers.layers``: order, kind, and which
    encoder output a layer produces or adds come from there; no module path is parsed here), between the two PQMF banks.
  * ``Schedule`` tracks, per tensor, the stream positions ``[S, F)`` its buffer holds and from where the next push still needs it, and
    turns one push into a list of ``Splice`` / ``Launch`` operations with buffer-relative offsets.  Warm-up (growing buffers with a
    true left edge), the steady state and ``finish`` (a true right edge) are the same rules; in the steady state the list repeats.
  * ``plan`` runs a schedule to its steady state and reads off, per tensor: rate, new samples per push, frontier lag, carry, buffer
    length and capacity; and ``lookahead`` / ``latency``.
  * ``StreamingEnhancer`` executes the operations on the device through ``GeneratorEngine``, which finds a node's launch in the same
    table by its path; ``tests/stream_oracle.py`` executes the same operations in float64 on poisoned buffers.
  * ``PoolBook`` keeps independent sessions -- streams that begin, pause and end whenever they like -- in the slots of one shared state:
    the steady-state list is position-free and every position of a ``Schedule`` moves by a constant per steady push
    (``Schedule.advance``), so all sessions that push in a tick share ONE run of ``plan.steady`` with a mask of the slots that advance.
    ``StreamPool`` executes its per-tick lists on the device; ``tests/pool_oracle.py`` executes them in float64.

  * A stream that arrives at the recording's rate (``StreamingEnhancer(input_rate=...)``) passes through ``rate.ChunkFront`` first: a
    carried-state resampler whose final samples reach the enhancer in whole chunks, one chunk later.  Nothing of the schedule changes.
    In a ``StreamPool(input_rates=...)`` every session has a rate of its own: ``rate.SlotFront`` keeps a resampler schedule and a FIFO per
    slot, one splice launch and one resampling launch serve all slots that push in a tick (``FrontRun``), and the chunk a session's
    FIFO completes is its push of that tick (``Hand``).
  * The way out mirrors that front: ``StreamPool(output_rates=...)`` / ``StreamingEnhancer(output_rate=, output_format=)`` hand every
    run's emitted samples to ``rate.SlotBack``, whose one launch resamples them per slot with carried state and stores them as PCM
    bytes; ``input_format=`` lets the pushes arrive as PCM bytes, decoded by one launch per tick.

Audio hold-back: ``cut_to_valid_length`` drops up to ``multiple - 1`` samples from the end of a clip, so a sample pushed now may turn
out to lie behind the stream's valid length.  The analysis bank therefore treats only ``ragged.cut_length(pushed)`` samples as
final (for pushes of whole multiples that is ``pushed - n % multiple``): nothing computed ever depends on a sample that is dropped.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

from . import ragged


@dataclasses.dataclass(frozen=True)
class Node:
    name: str        # module path, as in ragged.plan; its input tape has the same name
    kind: str        # "analysis" | "conv" | "unit" | "convT" | "lift" | "synthesis"
    c_in: int
    c_out: int
    ksize: int
    stride: int
    dilation: int
    pad_l: int
    pad_r: int
    reflect: bool
    rate: int                    # audio samples per sample of its INPUT
    add: Optional[str] = None    # hold tape added to the new samples of its input (the decoder's skip add)
    feeds: Tuple[str, ...] = ()  # hold / output tapes that receive its new exact outputs


@dataclasses.dataclass(frozen=True)
class Splice:
    """dst := [prev[prev_off : prev_off + n_carry] | src[src_off : src_off + n_new] (+ add[add_off : ...])]; the dst buffer is
    n_carry + n_new long afterwards (0: emptied, nothing runs).  Names: ``tape:X`` a state buffer (written through its ping-pong
    twin), ``out:X`` the latest output of node X, ``input`` the pushed chunk, ``emit:X`` a tensor handed to the caller."""
    dst: str
    prev: Optional[str]
    prev_off: int
    n_carry: int
    src: Optional[str]
    src_off: int
    n_new: int
    add: Optional[str] = None
    add_off: int = 0


@dataclasses.dataclass(frozen=True)
class Launch:
    """Node ``node`` on its tape of ``l_in`` samples (``lift``: on ``out:last_conv`` and ``tape:lift.operand``) -> ``out:node`` of
    ``l_out``; its outputs [lo, hi) are the new exact ones, everything outside is junk or was delivered before."""
    node: str
    l_in: int
    l_out: int
    lo: int
    hi: int


@dataclasses.dataclass
class _Tape:
    name: str
    channels: int
    rate: int
    S: int = 0      # stream position of the buffer's first sample
    F: int = 0      # ... behind its last one: the tensor's exact frontier as delivered here
    keep: int = 0   # the next splice keeps [keep, F)


def _ceil(a: int, b: int) -> int:
    return -((-a) // b)


def nodes_of(gen) -> List[Node]:
    """The generator as stream nodes: a node per entry of the layer table (``gen_layers.layers``, at the resolutions of ``ragged``'s
    walk) with the two PQMF banks and the tanh lift added."""
    m, n, p = gen.pqmf.decimation, gen.pqmf.kernel_size, gen.p
    out = [Node("pqmf.analysis", "analysis", 1, p, n, m, 1, n - 1, n - 1, False, 1, feeds=("first_bands",))]
    levels, steps = ragged._walk(gen, (gen.multiple * 64 - n,), 0)
    rate = [1] + [m * (levels[1][0] // lv[0]) for lv in levels[1:]]
    for layer, lv in steps:
        spec = layer.spec
        out.append(Node(layer.path, layer.kind, spec.c_in, spec.c_in if layer.kind == "unit" else spec.c_out, spec.ksize, spec.stride,
                        spec.dilation, spec.pad_l, spec.pad_l if spec.transposed else spec.pad_r, bool(spec.reflect), rate[lv],
                        None if layer.add is None else f"skip.{layer.add}", () if layer.skip is None else (f"skip.{layer.skip}",)))
    out.append(Node("lift", "lift", m, m, 1, 1, 1, 0, 0, False, m, feeds=("bands",)))
    out.append(Node("pqmf.synthesis", "synthesis", m, 1, n, m, 1, 0, 0, False, m, feeds=("enhanced",)))
    return out


class Schedule:
    """Positions of one stream (all rows advance in lockstep).  ``push(n)`` / ``push(n, final=True)`` return the operations of that
    push; the executor owns the buffers.  After a final push the schedule is spent until ``reset()``."""

    def __init__(self, gen, chunk_samples: int):
        chunk_samples = int(chunk_samples)
        if chunk_samples <= 0 or chunk_samples % gen.multiple:
            raise ValueError(f"chunk_samples must be a positive multiple of {gen.multiple}, got {chunk_samples}")
        self.gen, self.chunk = gen, chunk_samples
        self.m, self.n = gen.pqmf.decimation, gen.pqmf.kernel_size
        self.nodes = nodes_of(gen)
        self.by_name = {nd.name: nd for nd in self.nodes}
        self.out_chunk = {"enhanced": chunk_samples, "bands": chunk_samples // self.m}
        self._steady: Optional[tuple] = None   # plan.steady, once advance() has asked for it
        self.reset()

    def reset(self) -> None:
        self.pushed, self.finished = 0, False
        self._last: Optional[tuple] = None   # the operations of the latest push
        self.tapes: Dict[str, _Tape] = {}
        for nd in self.nodes:
            if nd.kind != "lift":
                self.tapes[nd.name] = _Tape(nd.name, nd.c_in, nd.rate)
            for f in nd.feeds:   # holds and outputs: at the rate of the producing node's OUTPUT
                self.tapes[f] = _Tape(f, nd.c_out, self.out_rate(nd))
        self.tapes["lift.operand"] = _Tape("lift.operand", self.gen.p, self.m)
        self.out_f = {nd.name: 0 for nd in self.nodes}   # exact frontier of each node's output
        self.emitted = {"enhanced": 0, "bands": 0}

    def out_rate(self, nd: Node) -> int:
        if nd.kind == "analysis":
            return self.m
        if nd.kind == "synthesis":
            return 1
        return nd.rate // nd.stride if nd.kind == "convT" else nd.rate * nd.stride

    # ---- one node on the tape [S, F): (base, l_out, lo, hi, keep) or None when it cannot run ----------------------------------------
    def _geometry(self, nd: Node, S: int, F: int, end: bool):
        """``base``: stream position of output 0; [lo, hi): the exact outputs; ``keep``: the first input the output ``hi`` reads (for a
        strided conv rounded down to its stride, where the next buffer may start)."""
        L, k, s, d, pl = F - S, nd.ksize, nd.stride, nd.dilation, nd.pad_l
        if L <= 0:
            return None
        if nd.kind in ("analysis", "conv", "unit"):
            if S % s:
                raise RuntimeError(f"stream schedule: {nd.name} starts at {S}, not a multiple of its stride {s}")
            span = (k - 1) * d
            if L + pl + nd.pad_r - span < 1 or (nd.reflect and max(pl, nd.pad_r) >= L) or (nd.kind == "unit" and d >= L):
                return None
            base, l_out = S // s, (L + pl + nd.pad_r - span - 1) // s + 1
            lo = base + _ceil(pl, s)
        elif nd.kind == "convT":   # output o sums the inputs i with 0 <= o + pad - i stride <= k - 1
            base, l_out = S * s, (L - 1) * s - 2 * pl + k
            lo = base + k - s - pl
        else:                      # synthesis: x[u] sums the frames t with u <= t m <= u + n - 1; m L - n outputs, none reads in front of S
            base, l_out = S * s, s * L - k
            lo = base
        if l_out < 1:
            return None
        # the analysis bank treats only cut_length(pushed) samples as final
        hi = base + l_out if end else min(base + l_out, _frontier(nd, ragged.cut_length(self.gen, F) if nd.kind == "analysis" else F))
        if nd.kind == "convT":
            keep = _ceil(hi + pl - k + 1, s)
        elif nd.kind == "synthesis":
            keep = _ceil(hi, s)
        else:
            keep = (hi * s - pl) // s * s
        return base, l_out, 0 if S == 0 else lo, hi, max(0, keep)

    def _feed(self, ops: list, tape: _Tape, src: Optional[str], base: int, lo: int, hi: int, add: Optional[_Tape] = None) -> None:
        """The new exact samples [lo, hi) of ``src`` (whose sample 0 sits at ``base``) behind what the tape keeps."""
        if lo != tape.F or not tape.S <= tape.keep <= tape.F:
            raise RuntimeError(f"stream schedule: {tape.name} holds [{tape.S}, {tape.F}), keeps from {tape.keep}, fed [{lo}, {hi})")
        n_carry, n_new = tape.F - tape.keep, hi - lo
        if n_new == 0 and tape.keep == tape.S:
            return
        add_off = 0
        if add is not None and n_new:
            if not (add.S <= lo and hi <= add.F):
                raise RuntimeError(f"stream schedule: {add.name} holds [{add.S}, {add.F}), {tape.name} adds [{lo}, {hi})")
            add_off = lo - add.S
        ops.append(Splice("tape:" + tape.name, "tape:" + tape.name if n_carry else None, tape.keep - tape.S if n_carry else 0, n_carry,
                          src if n_new else None, lo - base if n_new else 0, n_new,
                          "tape:" + add.name if add is not None and n_new else None, add_off))
        tape.S, tape.F = tape.keep, hi
        if add is not None:
            add.keep = hi

    def _emit(self, ops: list, name: str, src: str, base: int, lo: int, hi: int, final: bool) -> None:
        """Output ``name`` leaves in whole chunks (everything at the end); what is not out yet waits in its tape."""
        tape, c = self.tapes[name], self.out_chunk[name]
        held, n_new, off = tape.F - tape.S, hi - lo, lo - base
        if lo != tape.F:
            raise RuntimeError(f"stream schedule: output {name} holds up to {tape.F}, fed [{lo}, {hi})")
        if final or held + n_new >= c:
            take = n_new if final else c - held
            if held + take:
                ops.append(Splice("emit:" + name, "tape:" + name if held else None, 0, held, src if take else None, off if take else 0, take))
            rest = n_new - take
            ops.append(Splice("tape:" + name, None, 0, 0, src if rest else None, off + take if rest else 0, rest))
            self.emitted[name] += held + take
            tape.S, tape.F = hi - rest, hi
        elif n_new:
            ops.append(Splice("tape:" + name, "tape:" + name if held else None, 0, held, src, off, n_new))
            tape.F = hi
        tape.keep = tape.S

    def push(self, n_in: int, final: bool = False) -> List[object]:
        if self.finished:
            raise RuntimeError("this stream has finished; reset() starts a new one")
        if n_in < 0 or (not final and n_in != self.chunk) or (final and n_in >= self.chunk):
            raise ValueError(f"a push takes {self.chunk} samples, the final one fewer, got {n_in}")
        total = self.pushed + n_in
        end_audio = total
        if final:
            ragged.plan(self.gen, [total])   # refuses a stream below the shortest clip, in the words of the batch forward
            end_audio = ragged.cut_length(self.gen, total)
            self.finished = True
        ops: List[object] = []
        a = self.tapes["pqmf.analysis"]
        if end_audio < a.keep:
            raise RuntimeError(f"stream schedule: the stream ends at {end_audio}, in front of what the analysis keeps ({a.keep})")
        n_carry, n_new = min(a.F, end_audio) - a.keep, max(0, end_audio - a.F)
        if n_new or a.keep != a.S or end_audio < a.F:
            ops.append(Splice("tape:pqmf.analysis", "tape:pqmf.analysis" if n_carry else None, a.keep - a.S if n_carry else 0, n_carry,
                              "input" if n_new else None, 0, n_new))
        a.S, a.F = a.keep, end_audio
        self.pushed = total
        fresh = ("input", 0, 0, 1)   # (name, base, lo, hi) of the producer's new exact outputs; None: nothing new
        last_len = 0
        for i, nd in enumerate(self.nodes):
            if nd.kind == "lift":
                if fresh is None:
                    continue
                _, base, lo, hi = fresh
                fb, lc = self.tapes["first_bands"], self.tapes["last_conv"]
                if not (fb.S <= base and base + last_len <= fb.F):
                    raise RuntimeError(f"stream schedule: first_bands holds [{fb.S}, {fb.F}), the lift reads [{base}, {base + last_len})")
                ops.append(Splice("tape:lift.operand", None, 0, 0, "tape:first_bands", base - fb.S, last_len))
                ops.append(Launch("lift", last_len, last_len, lo - base, hi - base))
                op = self.tapes["lift.operand"]
                op.S = op.keep = base
                op.F = base + last_len
                fb.keep = lc.keep   # where last_conv's next output starts
                fresh = ("out:lift", base, lo, hi)
                self.out_f["lift"] = hi
                self._emit(ops, "bands", "out:lift", base, lo, hi, final)
                continue
            tape = self.tapes[nd.name]
            if i > 0 and fresh is not None:
                self._feed(ops, tape, *fresh, add=self.tapes[nd.add] if nd.add else None)
            if fresh is None and not final:
                continue
            g = self._geometry(nd, tape.S, tape.F, final)
            done = self.out_f[nd.name]
            if g is None or g[3] <= done:
                if final and g is None:
                    raise RuntimeError(f"stream schedule: {nd.name} cannot run on the last {tape.F - tape.S} samples")
                fresh = None
                continue
            base, l_out, lo, hi, keep = g
            if lo > done:
                raise RuntimeError(f"stream schedule: {nd.name} delivered up to {done}, its buffer yields [{lo}, {hi})")
            ops.append(Launch(nd.name, tape.F - tape.S, l_out, done - base, hi - base))
            fresh = ("out:" + nd.name, base, done, hi)
            self.out_f[nd.name], tape.keep, last_len = hi, max(tape.S, min(keep, tape.F)), l_out
            for f in nd.feeds:
                if f in self.out_chunk:
                    self._emit(ops, f, *fresh, final)
                else:
                    self._feed(ops, self.tapes[f], *fresh)
        if final:   # an output whose producer had nothing new at the end still hands over what it holds
            for name in self.out_chunk:
                t = self.tapes[name]
                if t.F > t.S:
                    self._emit(ops, name, None, t.F, t.F, t.F, True)
        self._last = tuple(ops)
        return ops

    def advance(self, k: int) -> None:
        """The state ``k`` further pushes would have left, without their operations.  Only in the steady state (the latest push returned
        ``plan.steady``): from there on a push moves every position by a constant -- one chunk at the tensor's own rate -- and repeats
        its list, so the pushes of a session that lives in a ``StreamPool`` slot need no host arithmetic until it leaves."""
        k = int(k)
        if k < 0:
            raise ValueError(f"advance takes a number of pushes, got {k}")
        if self.finished:
            raise RuntimeError("this stream has finished; reset() starts a new one")
        if self._steady is None:
            self._steady = plan(self.gen, self.chunk).steady
        if self._last != self._steady:
            raise RuntimeError("advance: the schedule is not in its steady state (its latest push did not return plan.steady)")
        for t in self.tapes.values():
            d = k * (self.chunk // t.rate)
            t.S, t.F, t.keep = t.S + d, t.F + d, t.keep + d
        for nd in self.nodes:
            self.out_f[nd.name] += k * (self.chunk // self.out_rate(nd))
        for name, c in self.out_chunk.items():
            self.emitted[name] += k * c
        self.pushed += k * self.chunk


def _frontier(nd: Node, f: int) -> int:
    """Outputs of ``nd`` that read nothing but its first ``f`` inputs (the left edge is the stream's own)."""
    if f <= 0:
        return 0
    if nd.kind in ("analysis", "conv", "unit"):   # o stride - pad_l + (k - 1) dil <= f - 1
        return max(0, (f - 1 - (nd.ksize - 1) * nd.dilation + nd.pad_l) // nd.stride + 1)
    if nd.kind == "convT":                        # floor((o + pad) / stride) <= f - 1
        return max(0, f * nd.stride - nd.pad_l)
    if nd.kind == "synthesis":                    # of the m f - n outputs a buffer of f frames yields
        return max(0, f * nd.stride - nd.ksize)
    return f


def exact_frontier(gen, audio: int) -> int:
    """Enhanced samples that depend on nothing but the first ``audio`` input samples, by the schedule's rules (no hold-back)."""
    f = audio
    for nd in nodes_of(gen):
        f = _frontier(nd, f)
    return f


@dataclasses.dataclass(frozen=True)
class TensorPlan:
    name: str        # the layer whose input it is, or first_bands / skip.i (holds), lift.operand, bands / enhanced (outputs)
    channels: int
    rate: int        # audio samples per sample
    new: int         # samples gained per push in the steady state
    lag: int         # pushed / rate - exact frontier, in its own samples
    carry: int       # samples in front of the new ones that the next push still needs
    length: int      # carry + new: the steady-state buffer
    capacity: int    # samples per (row, channel) of its two state buffers: covers warm-up and finish


@dataclasses.dataclass(frozen=True)
class StreamPlan:
    chunk_samples: int
    multiple: int
    hold: int                          # pushed samples the analysis bank does not treat as final yet
    lookahead: int                     # input samples past an output sample that its value depends on (the largest over the phases)
    latency: int                       # pushed - emitted in the steady state
    warmup_pushes: int                 # pushes before the first one that returns samples
    tensors: Tuple[TensorPlan, ...]
    steady: Tuple[object, ...]         # the operations of a steady-state push
    state_floats: int                  # floats of state per stream (both buffers of every tensor)

    def tensor(self, name: str) -> TensorPlan:
        return next(t for t in self.tensors if t.name == name)


def plan(gen, chunk_samples: int) -> StreamPlan:
    """The steady state of ``Schedule(gen, chunk_samples)``.  ``ValueError`` unless ``chunk_samples`` is a positive multiple of
    ``gen.multiple``: then every tensor gains a constant count per push and every strided layer keeps its phase."""
    sch = Schedule(gen, chunk_samples)
    chunk, n = sch.chunk, sch.n
    prev, warm = None, None
    for j in range(4096):
        ops = sch.push(chunk)
        if warm is None and any(isinstance(o, Splice) and o.dst == "emit:enhanced" for o in ops):
            warm = j
        if warm is not None and ops == prev:
            break
        prev = ops
    else:
        raise RuntimeError("the stream schedule did not settle")
    steady = tuple(ops)
    dsts = ((o, *o.dst.split(":", 1)) for o in steady if isinstance(o, Splice))
    new = {key: (o.n_carry, o.n_new) for o, kind, key in dsts if kind == "tape"}
    tensors = []
    for name, t in sch.tapes.items():
        carry, fresh = new[name]
        lag = sch.pushed // t.rate - t.F
        if name in sch.out_chunk:   # an output leaves in whole chunks; its tape holds what does not fill the next one yet
            held, c = t.F - t.S, sch.out_chunk[name]
            tensors.append(TensorPlan(name, t.channels, t.rate, c, lag, held, held, c))
            continue
        # finish() delivers everything up to the stream's end at once: the lag, the last chunk and the banks' span on top of the carry
        cap = carry + fresh + lag + n // t.rate + 4
        tensors.append(TensorPlan(name, t.channels, t.rate, fresh, lag, carry, carry + fresh, cap))
    base = 64 * gen.multiple
    lookahead = max(a - exact_frontier(gen, a) for a in range(base, base + gen.multiple))
    return StreamPlan(chunk, gen.multiple, chunk - ragged.cut_length(gen, chunk), lookahead, sch.pushed - sch.emitted["enhanced"], warm,
                      tuple(tensors), steady, sum(2 * t.channels * t.capacity for t in tensors))


# ---- the public driver ----------------------------------------------------------------------------------------------------------------
class _Driver:
    """What the two drivers share: the plan, the state's device, the check of a pushed chunk and the tensors a call returns."""

    _who = ""     # the class as its messages name it
    _per = ""     # ... and whose the chunk is
    _last = ""    # the call that takes the shorter last chunk

    def __init__(self, generator, chunk_samples: int, return_bands: bool):
        self.generator, self.return_bands = generator, bool(return_bands)
        self.plan = plan(generator, chunk_samples)
        self.chunk_samples = self.plan.chunk_samples
        self.state = None   # device buffers: allocated by prepare() or at the first push, on the chunk's device

    @property
    def latency(self) -> int:
        return self.plan.latency

    @property
    def lookahead(self) -> int:
        return self.plan.lookahead

    def _allocate(self, device, rows: int) -> bool:
        """The state of ``rows`` rows on ``device``; True when it was allocated by this call."""
        import torch

        from . import gen_engine

        device = torch.empty(0, device=device).device   # "cuda" -> cuda:0
        if self.state is not None and self.state.device == device:
            return False
        self.state = gen_engine.engine_of(self.generator).stream_state(self.plan, rows, device)
        return True

    def _no_grad(self, what: str) -> None:
        import torch

        if torch.is_grad_enabled():
            raise RuntimeError(f"{self._who}: {what} has no backward; call it under torch.no_grad()")

    def _check(self, chunk, rows: int, what: str, samples: Optional[int] = None) -> None:
        """``chunk``: ``rows`` rows of one chunk, or of fewer samples in the call that ends a stream.  ``samples``: the chunk's length
        where it is not ``chunk_samples`` (a chunk at the recording's rate)."""
        import torch

        last = what == self._last
        samples = self.chunk_samples if samples is None else samples
        if (not isinstance(chunk, torch.Tensor) or chunk.dim() != 3 or tuple(chunk.shape[:2]) != (rows, 1) or chunk.dtype is not torch.float32
                or not (chunk.shape[2] < samples if last else chunk.shape[2] == samples)):
            got = f"{chunk.dtype} {tuple(chunk.shape)}" if isinstance(chunk, torch.Tensor) else type(chunk).__name__
            raise ValueError(f"{self._who}: {what} expects a float32 ({rows}, 1, {samples}) tensor{self._per}"
                             f"{' or a shorter last one' if last else ''}, got {got}")
        if not chunk.is_cuda:
            from ._lib import EbenError

            raise EbenError(f"{self._who} runs only on an MI355X HIP device (got a tensor on '{chunk.device}'); there is no CPU path")

    def _emitted(self, out: dict, rows: int, device) -> list:
        """[enhanced] or [enhanced, bands] of a run's emits: ``(rows, c, 0)`` where nothing was emitted."""
        import torch

        names = (("enhanced", 1), ("bands", self.generator.pqmf.decimation))[: 2 if self.return_bands else 1]
        return [t if (t := out.get(name)) is not None else torch.empty((rows, c, 0), dtype=torch.float32, device=device) for name, c in names]


class StreamingEnhancer(_Driver):
    """``generator`` on audio that is still arriving: ``push`` a ``(streams, 1, chunk_samples)`` float32 device tensor, get the newly
    final enhanced samples ``(streams, 1, k)`` -- k is 0 during warm-up and exactly ``chunk_samples`` from the first non-empty return on;
    ``finish()`` (optionally with the last, shorter chunk) returns the rest, up to ``ragged.cut_length(generator, total pushed)``.  The
    concatenation is what ``generator(cut_to_valid_length(whole clip))`` returns.  Rows advance in lockstep.  ``return_bands``: every
    call returns ``(enhanced, bands)``, the bands with the same semantics at their rate.  Nothing here waits for the device.

    ``input_rate`` (other than ``model_rate``): the stream arrives at the recording's rate, as in the reference's inference script
    (``Resample(48_000, 16_000)`` in front of the model).  ``push`` then takes ``(streams, 1, input_chunk_samples)`` with
    ``input_chunk_samples = chunk_samples * orig / new`` over the reduced ratio -- a ``ValueError`` names the smallest ``chunk_samples``
    for which that is a whole number -- and ``finish`` a shorter tail; the results stay at the model's rate, and their concatenation is
    ``generator(cut_to_valid_length(augment.resample(whole clip, input_rate, model_rate)))``.  A ``rate.StreamResampler`` in front keeps
    the final model-rate samples in a device FIFO and hands the enhancer whole chunks; at the end it makes as many pushes as the FIFO
    holds, then ``finish`` with the rest.  Known cost: the resampler's look-ahead is ``width + orig - 1`` input samples (7 model-rate
    samples at 3:1), so a push completes one chunk less that lag and the enhancer gets chunk k - 1 at push k: one ``chunk_samples`` of
    extra latency (16 ms at 256), which ``input_latency`` states in input samples.

    ``output_format`` (one of ``corpus.FORMATS``), ``output_rate``: the enhanced samples leave as PCM bytes, at a rate of their own -- per
    call a uint8 ``(streams, k * bytes per sample)`` view into ``image`` (every row starts at a 16-byte boundary), k by
    ``rate.final_outputs`` at ``output_rate``; ``finish`` hands over what the resampler held back (``output_lookahead`` model-rate
    samples).  Only ``output_rate``: float32 ``(streams, 1, k)`` at that rate.  ``clipped``: int32 ``(streams,)`` on the device, the samples
    the encoder clamped so far.  ``input_format``: ``push`` takes uint8 ``(streams, input_chunk_samples * bytes per sample)`` of that
    format, ``finish`` a shorter tail.  Both are the pool's kernels (``eben_stream_pcm_out``, ``eben_pcm_chunks_in``) with slot = row:
    one launch each per 64 rows and run."""

    _who, _last = "StreamingEnhancer", "finish"

    def __init__(self, generator, chunk_samples: int, streams: int = 1, return_bands: bool = False, input_rate: Optional[int] = None,
                 model_rate: int = 16000, output_rate: Optional[int] = None, output_format: Optional[str] = None, input_format: Optional[str] = None):
        if int(streams) < 1:
            raise ValueError(f"streams must be positive, got {streams}")
        self.streams = int(streams)
        super().__init__(generator, chunk_samples, return_bands)
        self._schedule = Schedule(generator, chunk_samples)
        self.output_rate = int(model_rate) if output_rate is None else int(output_rate)
        self.output_format, self.input_format = output_format, input_format
        self._back = self._back_tapes = self._staging = None   # rate.SlotBack and rate.BackTapes with slot = row; the decoded PCM chunk
        self.clipped = self.image = None
        self.output_lookahead = 0
        if output_format is not None or self.output_rate != int(model_rate):
            from . import rate

            if self.streams > 256:
                raise ValueError(f"StreamingEnhancer: at most 256 streams leave as PCM or at a rate of their own, got {streams}")
            most = max(self.plan.latency, self.plan.warmup_pushes * self.chunk_samples) + self.chunk_samples
            self._back = rate.SlotBack(self.chunk_samples, self.streams, (self.output_rate,), model_rate, most)
            self._back.check(self.output_rate, output_format, "StreamingEnhancer")
            self._open_back()
            self.output_lookahead = self._back.lookahead(0)
        if input_format is not None:
            from . import rate

            rate.pcm_format(input_format, "StreamingEnhancer")
        self._front = None   # rate.ChunkFront: the resampler and its FIFO, when the stream arrives at another rate
        if input_rate is not None and int(input_rate) != int(model_rate):
            from . import rate

            self._front = rate.ChunkFront(input_rate, model_rate, self.chunk_samples, self.streams, generator.multiple)
            self._ratio = rate.ratio(input_rate, model_rate)[:2]

    @property
    def input_chunk_samples(self) -> int:
        """Samples per push: ``chunk_samples`` at the rate the stream arrives at."""
        return self.chunk_samples if self._front is None else self._front.input_chunk_samples

    @property
    def input_latency(self) -> int:
        """Input samples pushed minus the input samples the emitted ones correspond to, in the steady state: ``latency`` without
        ``input_rate``; with it one chunk more (the FIFO in front), at the input's rate."""
        if self._front is None:
            return self.plan.latency
        orig, new = self._ratio
        return self._front.input_chunk_samples + _ceil(self.plan.latency * orig, new)

    def _open_back(self) -> None:
        for r in range(self.streams):
            self._back.open(r, self.output_rate, self.output_format)

    def prepare(self, device) -> "StreamingEnhancer":
        """Allocates the state on ``device`` now instead of at the first push (it is allocated once either way)."""
        self._allocate(device, self.streams)
        if self._front is not None:
            self._front.prepare(device)
        if self._back is not None and (self._back_tapes is None or self._back_tapes.device != self.state.device):
            from . import rate

            self._back_tapes = rate.BackTapes(self._back, self.state.device)
            self.clipped = self._back_tapes.clipped
        if self.input_format is not None and (self._staging is None or self._staging.device != self.state.device):
            import torch

            self._staging = torch.zeros((self.streams, 1, self.input_chunk_samples), dtype=torch.float32, device=self.state.device)
        return self

    def reset(self) -> None:
        """Ready for a new stream; the state buffers stay."""
        self._schedule.reset()
        if self.state is not None:
            self.state.reset()
        if self._front is not None:
            self._front.reset()
        if self._back is not None:
            self._open_back()
            if self.clipped is not None:
                self.clipped.zero_()

    def _leave(self, src, final: bool):
        """The way out of one run: ``src`` its ``enhanced`` (streams, 1, k) or None.  Returns the rows' bytes (or float32 samples) in a
        fresh image, every row at a 16-byte boundary."""
        import torch

        from . import rate

        k = 0 if src is None else src.shape[2]
        pieces, ranges, _ = self._back.emit([(r, r, k, final) for r in range(self.streams)])
        n, b = ranges[0][1], 4 if self.output_format is None else rate.PCM_BYTES[rate.PCM_FORMATS.index(self.output_format)]
        pitch = -(-(n * b) // 16) * 16
        self.image = torch.empty(max(16, self.streams * pitch), dtype=torch.uint8, device=self.state.device)
        if pieces:
            self._back_tapes.run(pieces, self.image.numel(), src, self.image)
        rows = self.image[: self.streams * pitch].view(self.streams, pitch)[:, : n * b]
        if self.output_format is not None:
            return rows
        return rows.view(torch.float32).unsqueeze(1) if n else torch.empty((self.streams, 1, 0), dtype=torch.float32, device=self.state.device)

    def _nothing(self, device):
        """What a call returns that ran nothing."""
        import torch

        got = self._emitted({}, self.streams, device)
        if self.output_format is not None:
            got[0] = torch.empty((self.streams, 0), dtype=torch.uint8, device=device)
        return tuple(got) if self.return_bands else got[0]

    def _run(self, chunk, n_in: int, final: bool):
        from . import gen_engine

        engine = gen_engine.engine_of(self.generator)
        device = chunk.device if chunk is not None else self.state.device if self.state is not None else next(self.generator.parameters()).device
        self.prepare(device)
        out = engine.stream_run(self.state, self._schedule.push(n_in, final), chunk)
        got = self._emitted(out, self.streams, device)
        if self._back is not None:
            got[0] = self._leave(out.get("enhanced"), final)
        return tuple(got) if self.return_bands else got[0]

    def _joined(self, results: list, device):
        """What a call returns for the runs it made: none (empty tensors), one, or several in order."""
        import torch

        if not results:
            return self._nothing(device)
        if len(results) == 1:
            return results[0]
        if self.return_bands:
            return tuple(torch.cat(parts, dim=-1) for parts in zip(*results))
        return torch.cat(results, dim=-1)

    def _decoded(self, chunk, what: str):
        """A pushed chunk of PCM bytes, uint8 (streams, n * bytes per sample), as float32 (streams, 1, n): one launch per 64 rows."""
        import torch

        from . import rate

        fmt = rate.PCM_FORMATS.index(self.input_format)
        b, last = rate.PCM_BYTES[fmt], what == self._last
        want = self.input_chunk_samples * b
        if (not isinstance(chunk, torch.Tensor) or chunk.dtype is not torch.uint8 or chunk.dim() != 2 or chunk.shape[0] != self.streams or chunk.shape[1] % b
                or not (chunk.shape[1] < want if last else chunk.shape[1] == want)):
            got = f"{chunk.dtype} {tuple(chunk.shape)}" if isinstance(chunk, torch.Tensor) else type(chunk).__name__
            raise ValueError(f"StreamingEnhancer: {what} expects a uint8 ({self.streams}, {want}) tensor of {self.input_format} bytes"
                             f"{' or a shorter last one of whole samples' if last else ''}, got {got}")
        if not chunk.is_cuda:
            from ._lib import EbenError

            raise EbenError(f"StreamingEnhancer runs only on an MI355X HIP device (got a tensor on '{chunk.device}'); there is no CPU path")
        self.prepare(chunk.device)
        chunk, n = chunk.contiguous(), chunk.shape[1] // b
        rate.pcm_chunks_in([(chunk[r], n, fmt, r) for r in range(self.streams)], self._staging.view(self.streams, self._staging.shape[2]))
        return self._staging[:, :, :n].contiguous()

    def _run_rated(self, chunk, final: bool):
        """A chunk at the recording's rate: through the resampler into the FIFO, every chunk the FIFO fills through the enhancer."""
        device = chunk.device if chunk is not None else self.state.device if self.state is not None else next(self.generator.parameters()).device
        self.prepare(device)
        if final:   # a stream below the shortest clip is refused in the words of the batch forward, before anything runs
            orig, new = self._ratio
            ragged.plan(self.generator, [_ceil(new * (self._front.pushed + (0 if chunk is None else chunk.shape[2])), orig)])
        results: list = []
        rest = self._front.feed(chunk, final, lambda full: results.append(self._run(full, self.chunk_samples, False)))
        if final:
            results.append(self._run(rest, 0 if rest is None else rest.shape[2], True))
        return self._joined(results, device)

    def push(self, chunk):
        self._no_grad("push")
        if self.input_format is not None:
            chunk = self._decoded(chunk, "push")
        if self._front is not None:
            self._check(chunk, self.streams, "push", self._front.input_chunk_samples)
            return self._run_rated(chunk.contiguous(), False)
        self._check(chunk, self.streams, "push")
        return self._run(chunk.contiguous(), self.chunk_samples, False)

    def finish(self, tail=None):
        """The rest of the stream.  ``tail``: the last ``(streams, 1, r)`` samples, ``r < input_chunk_samples`` (what did not fill a
        chunk).  ``ValueError`` when everything pushed is shorter than the shortest clip the generator accepts."""
        self._no_grad("finish")
        if tail is not None and tail.shape[-1] == 0:
            tail = None
        if tail is not None and self.input_format is not None:
            tail = self._decoded(tail, "finish")
        if tail is not None:
            self._check(tail, self.streams, "finish", self.input_chunk_samples)
            tail = tail.contiguous()
        if self._front is not None:
            return self._run_rated(tail, True)
        return self._run(tail, 0 if tail is None else tail.shape[2], True)


# ---- independent sessions in the slots of one shared state ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class PrivatePush:
    """Session ``session`` pushes alone: ``ops`` on the batch-1 state ``private`` (``fresh``: the state starts a new stream first)."""
    session: "Session"
    private: int
    ops: Tuple[object, ...]
    fresh: bool


@dataclasses.dataclass(frozen=True)
class PooledRun:
    """One run of ``plan.steady`` over all slots: bit r of ``mask`` (64-bit words) = slot r advances; ``order``: the sessions of the set
    bits in slot order, which is the row order of the compact input and of the compact emits."""
    mask: Tuple[int, ...]
    order: Tuple["Session", ...]


@dataclasses.dataclass(frozen=True)
class Move:
    """``into_pool``: the steady-state buffers of state ``private`` go to row ``slot`` of the pool's state; else the other way round, into a
    state that is set to the steady lengths first."""
    session: "Session"
    private: int
    slot: int
    into_pool: bool


@dataclasses.dataclass(frozen=True)
class FrontRun:
    """The resampling front of the sessions that arrive at a recording rate (``rate.SlotFront.feed``): ``splices`` of the chunks that
    ``order`` pushed into their slots' tapes, then ``pieces`` into their FIFO buffers."""
    splices: Tuple[object, ...]
    pieces: Tuple[object, ...]
    order: Tuple["Session", ...]


@dataclasses.dataclass(frozen=True)
class Hand:
    """From here on ``session``'s chunk is what its FIFO completed (``rate.SlotChunk``), at the model's rate; None: it has none."""
    session: "Session"
    chunk: object


class Session:
    """Handle of one stream in a ``StreamPool``: ``phase`` is "warming", "pooled" or "closed".  ``input_rate``: the rate its audio arrives
    at; ``input_chunk_samples``: samples per push at that rate; ``input_latency``: input samples pushed minus those the emitted ones
    correspond to in the steady state (``StreamingEnhancer``'s properties of the same names)."""

    def __init__(self, book: "PoolBook", slot: int, private: int, schedule: Schedule, input_rate: Optional[int] = None,
                 output_rate: Optional[int] = None, output_format: Optional[str] = None, input_format: Optional[str] = None):
        self.book, self.slot, self.schedule = book, slot, schedule
        # the way out: ``output_rate`` the rate its results leave at, ``output_format`` one of ``corpus.FORMATS`` (None: float32),
        # ``output_lookahead`` the model-rate samples the resampler behind the model holds back, ``clipped`` a 0-dim int32 device view of
        # the samples the encoder clamped so far (set by the pool).  ``input_format``: its pushes are PCM bytes of that format.
        self.egress = output_format is not None or (output_rate is not None and output_rate != book.model_rate)
        self.output_rate = book.model_rate if output_rate is None else output_rate
        self.output_format, self.input_format = output_format, input_format
        self.output_lookahead = book.back.lookahead(slot) if self.egress else 0
        self.clipped = None
        self.rated = input_rate is not None   # its chunks pass through the book's rate front first
        self.input_rate = book.model_rate if input_rate is None else input_rate
        self.input_chunk_samples, self.input_latency = book.chunk, book.plan.latency
        if self.rated:
            front = book.front
            orig, new, _ = front.ratios[front.rates.index(input_rate)]
            self.input_chunk_samples = front.input_chunk[front.rates.index(input_rate)]
            self.input_latency = self.input_chunk_samples + _ceil(book.plan.latency * orig, new)
        self.private = private   # id of the batch-1 state it warms up or finishes on; -1 while it needs none
        self.phase = "warming"
        self.pushes = 0          # private pushes so far
        self.pooled_pushes = 0   # pushes made in the slot that ``schedule`` has not been advanced by yet

    def __repr__(self) -> str:
        return f"Session(slot {self.slot}, {self.phase})"


class PoolBook:
    """Who is where (host only, no GPU needed): slots, private states, mask words and compact order, and per tick the list of
    ``PooledRun`` / ``PrivatePush`` / ``Move`` entries that ``StreamPool`` executes on the device and ``tests/pool_oracle.py`` in float64.
    A session warms up and finishes on a private batch-1 state with its own ``Schedule`` and lives in a slot in between; a pooled push
    costs a counter increment here."""

    def __init__(self, gen, chunk_samples: int, slots: int = 64, stream_plan: Optional[StreamPlan] = None, input_rates=(), model_rate: int = 16000,
                 output_rates=()):
        slots = int(slots)
        if not 1 <= slots <= 256:
            raise ValueError(f"slots must lie in 1 ... 256, got {slots}")
        self.gen, self.slots = gen, slots
        self.plan = stream_plan if stream_plan is not None else plan(gen, chunk_samples)
        self.chunk = self.plan.chunk_samples
        self.model_rate = int(model_rate)
        self.input_rates = tuple(int(r) for r in input_rates)   # the recording rates this pool admits, beside the model's own
        self.front = None   # rate.SlotFront: a resampler and a FIFO per slot, when a declared rate is not the model's
        if any(r != self.model_rate for r in self.input_rates):
            from . import rate

            self.front = rate.SlotFront(self.chunk, slots, self.input_rates, self.model_rate, gen.multiple)
        self.output_rates = tuple(int(r) for r in output_rates)   # the rates sessions may leave at, beside the model's own
        self.back = None    # rate.SlotBack: a resampler schedule per slot behind the model, once declared or first asked for
        if self.output_rates:
            self._back()
        self.pcm_in = False   # a session pushed PCM bytes: the pool keeps a staging buffer
        self.words = (slots + 63) // 64
        self.free_slots = list(range(slots))
        self.free_private: List[int] = []
        self.n_private = 0            # private states handed out so far: ids 0 ... n_private - 1
        self.spare: List[Schedule] = []
        self.moved = tuple(t.name for t in self.plan.tensors if t.length and t.name != "lift.operand")   # the tensors that hold state

    def _take_private(self) -> int:
        if self.free_private:
            return self.free_private.pop(0)
        self.n_private += 1
        return self.n_private - 1

    def _give_private(self, i: int) -> None:
        self.free_private.append(i)
        self.free_private.sort()

    def _back(self):
        if self.back is None:
            from . import rate

            # the most a session emits in one run: at the end, the model's latency (or a whole warm-up) and a tail at once
            most = max(self.plan.latency, self.plan.warmup_pushes * self.chunk) + self.chunk
            self.back = rate.SlotBack(self.chunk, self.slots, self.output_rates, self.model_rate, most)
        return self.back

    def open(self, input_rate: Optional[int] = None, output_rate: Optional[int] = None, output_format: Optional[str] = None,
             input_format: Optional[str] = None) -> Session:
        if not self.free_slots:
            raise RuntimeError(f"StreamPool: all {self.slots} slots hold an open session")
        if input_rate is not None and int(input_rate) == self.model_rate:
            input_rate = None
        if input_rate is not None:
            input_rate = int(input_rate)
            if self.front is None or input_rate not in self.front.rates:
                raise ValueError(f"StreamPool: a session at {input_rate} Hz in a pool that declared input_rates = {self.input_rates} "
                                 f"(the model's {self.model_rate} Hz needs no declaration)")
        if output_rate is not None and int(output_rate) == self.model_rate:
            output_rate = None
        if output_rate is not None or output_format is not None or input_format is not None:
            from . import rate

            if input_format is not None:
                rate.pcm_format(input_format, "StreamPool")
            if output_rate is not None or output_format is not None:
                output_rate = self._back().check(output_rate, output_format, "StreamPool")[0]
        if self.spare:
            schedule = self.spare.pop()
            schedule.reset()
        else:
            schedule = Schedule(self.gen, self.chunk)
            schedule._steady = self.plan.steady
        slot = self.free_slots.pop(0)
        if output_rate is not None or output_format is not None:
            self.back.open(slot, output_rate, output_format)
        session = Session(self, slot, -1, schedule, input_rate, output_rate, output_format, input_format)   # a private state is taken at the first push, the slot now
        if session.rated:
            self.front.open(session.slot, input_rate)
        self.pcm_in = self.pcm_in or input_format is not None
        return session

    def check(self, sessions) -> None:
        seen = set()
        for s in sessions:
            if not isinstance(s, Session) or s.book is not self:
                raise ValueError("StreamPool: not a session of this pool")
            if s.phase == "closed":
                raise RuntimeError("StreamPool: this session is closed")
            if id(s) in seen:
                raise ValueError("StreamPool: a session is named twice")
            seen.add(id(s))

    def tick(self, sessions) -> List[object]:
        """The entries of a tick in which exactly ``sessions`` push one chunk each; the others stay where they are."""
        sessions = list(sessions)
        self.check(sessions)
        rated = sorted((s for s in sessions if s.rated), key=lambda s: s.slot)
        if not rated:
            return self._pushes(sessions)
        # a chunk at a recording rate goes through the front; the chunk its FIFO completes (none at a stream's first push) is the
        # session's push of this tick
        splices, pieces, chunks = self.front.feed([(s.slot, s.input_chunk_samples) for s in rated])
        entries: List[object] = [FrontRun(tuple(splices), tuple(pieces), tuple(rated))]
        entries.extend(Hand(s, chunks[s.slot][0]) for s in rated if chunks[s.slot])
        return entries + self._pushes([s for s in sessions if not s.rated or chunks[s.slot]])

    def _pushes(self, sessions) -> List[object]:
        """The entries of one chunk at the model's rate for each of ``sessions``."""
        entries: List[object] = []
        pooled = sorted((s for s in sessions if s.phase == "pooled"), key=lambda s: s.slot)
        if pooled:
            mask = [0] * self.words
            for s in pooled:
                mask[s.slot >> 6] |= 1 << (s.slot & 63)
                s.pooled_pushes += 1
            entries.append(PooledRun(tuple(mask), tuple(pooled)))
        for s in sessions:
            if s.phase != "warming":
                continue
            ops = tuple(s.schedule.push(self.chunk))
            if s.private < 0:
                s.private = self._take_private()
            entries.append(PrivatePush(s, s.private, ops, s.pushes == 0))
            s.pushes += 1
            if ops == self.plan.steady:
                entries.append(Move(s, s.private, s.slot, True))
                self._give_private(s.private)
                s.private, s.phase = -1, "pooled"
        return entries

    def close(self, session: Session, n_tail: int = 0) -> List[object]:
        """The entries that finish ``session`` with a tail of ``n_tail`` samples; its slot is free afterwards.  A refusal of the final push
        (a tail of a chunk or more, a stream below the shortest clip) leaves the session open."""
        self.check([session])
        s, entries = session, []
        if s.rated:
            # the tail is at the recording's rate: what the FIFO completes with it is first, possibly, one more whole chunk -- an ordinary
            # push of this session -- and then the rest, which ends the stream
            if not 0 <= n_tail < s.input_chunk_samples:
                raise ValueError(f"a push takes {s.input_chunk_samples} samples, the final one fewer, got {n_tail}")
            ragged.plan(self.gen, [self.front.outputs_after(s.slot, n_tail)])   # refuses a stream below the shortest clip before anything moves
            splices, pieces, chunks = self.front.feed([(s.slot, n_tail)], final=True)
            entries.append(FrontRun(tuple(splices), tuple(pieces), (s,)))
            n_tail = 0
            for c in chunks[s.slot]:
                entries.append(Hand(s, c))
                if c.samples == self.chunk:
                    entries.extend(self._pushes([s]))
                else:
                    n_tail = c.samples
            if n_tail == 0:
                entries.append(Hand(s, None))   # the stream ends without a rest
            self.front.release(s.slot)
        if s.phase == "pooled":
            s.schedule.advance(s.pooled_pushes)
            s.pooled_pushes = 0
            ops = tuple(s.schedule.push(n_tail, final=True))
            s.private = self._take_private()
            entries.append(Move(s, s.private, s.slot, False))
            entries.append(PrivatePush(s, s.private, ops, False))
        else:
            ops = tuple(s.schedule.push(n_tail, final=True))
            if s.private < 0:
                s.private = self._take_private()
            entries.append(PrivatePush(s, s.private, ops, s.pushes == 0))
        self._give_private(s.private)
        self.free_slots.append(s.slot)
        self.free_slots.sort()
        self.spare.append(s.schedule)
        s.phase, s.private = "closed", -1
        return entries


class StreamPool(_Driver):
    """Independent streams through one ``generator``: ``open()`` a session whenever a stream begins, ``step({session: chunk})`` with the
    ``(1, 1, chunk_samples)`` float32 device chunks of the sessions that have one this tick, ``close(session, tail)`` when it ends.  Per
    session the returns are those of ``StreamingEnhancer.push`` / ``finish`` on a stream of its own.  A session warms up and finishes
    alone on a private batch-1 state; in between it lives in one of ``slots`` rows of a shared state, and every session that pushed in a
    tick is served by ONE run of the steady-state list over all rows, with masked splices (``eben_stream_splice_rows``) that leave the
    rows of the others as they are.  Nothing here waits for the device.

    ``input_rates``: the recording rates this pool admits beside ``model_rate``, declared up front so that everything is allocated once
    (each must give a whole ``rate.input_chunk_samples``; the ``ValueError`` names the smallest ``chunk_samples`` that works).
    ``open(input_rate=r)`` opens a session whose ``step`` takes ``(1, 1, session.input_chunk_samples)`` at its own rate and whose ``close``
    takes a shorter tail; per session the returns are those of ``StreamingEnhancer(..., input_rate=r)``: nothing at the first push, one
    ``chunk_samples`` of extra latency (``session.input_latency``).  All rated sessions of a tick share one splice launch per pushed
    length and one resampling launch (``eben_rate_splice_slots``, ``eben_resample_slots``).  Without ``input_rates`` the pool is what it
    was.

    ``output_rates``: the rates sessions may leave at beside ``model_rate``, declared up front for the same reason (any ratio the
    resampling tile admits).  ``open(..., output_rate=, output_format=, input_format=)`` opens a session that leaves as PCM bytes at a
    rate of its own and/or arrives as PCM bytes (see ``open``): ``rate.SlotBack`` keeps a resampler schedule per slot behind the model,
    one ``eben_stream_pcm_out`` behind every run that emitted serves all its sessions, one ``eben_pcm_chunks_in`` in front of a tick
    decodes every PCM session's frame.  A pool that declares ``output_rates`` and uses none makes today's entries and library calls."""

    _who, _per, _last = "StreamPool", " per session", "close"

    def __init__(self, generator, chunk_samples: int, slots: int = 64, return_bands: bool = False, input_rates=(), model_rate: int = 16000,
                 output_rates=()):
        super().__init__(generator, chunk_samples, return_bands)   # ``state``: the shared one
        self.book = PoolBook(generator, chunk_samples, slots, self.plan, input_rates, model_rate, output_rates)
        self.slots = self.book.slots
        self.private = {}      # id -> batch-1 StreamState, allocated when the book first hands the id out and kept
        self.tapes = None      # rate.SlotTapes: the front's tapes, FIFO buffers and tables, when the pool admits recording rates
        self.back = None       # rate.BackTapes: the tapes, tables and clipped counts of the way out, when a session leaves as PCM or at a rate
        self.image = None      # the byte image of the latest run that left this way (allocated by that run)
        self.staging = None    # (slots, 1, longest input chunk) float32: where the PCM bytes of a tick are decoded to

    def prepare(self, device, private: int = 0) -> "StreamPool":
        """Allocates the shared state on ``device`` now instead of at the first step, and ``private`` batch-1 states for sessions that
        warm up or finish at the same time (further ones are allocated when first needed, and kept).  Another device while sessions at a
        recording rate are open is refused: the front's schedules would go on from tapes that were never written."""
        before = self.state
        if self._allocate(device, self.slots):
            if self.tapes is not None and any(st is not None for st in self.book.front.slot):
                self.state = before
                raise RuntimeError(f"StreamPool: sessions at a recording rate are open on {self.tapes.device}; their tapes do not move to "
                                   f"'{device}': close them first")
            for t in self.plan.tensors:
                self.state.length[t.name] = t.length
            self.private = {}
        if self.book.front is not None and (self.tapes is None or self.tapes.device != self.state.device):
            from . import rate

            self.tapes = rate.SlotTapes(self.book.front, self.state.device)
        if self.book.back is not None and (self.back is None or self.back.device != self.state.device):
            from . import rate

            if self.back is not None and any(s is not None for s in self.book.back.slot):
                raise RuntimeError(f"StreamPool: sessions that leave at a rate of their own are open on {self.back.device}; their tapes do not "
                                   f"move to '{device}': close them first")
            self.back = rate.BackTapes(self.book.back, self.state.device)
        if self.book.pcm_in and (self.staging is None or self.staging.device != self.state.device):
            import torch

            front = self.book.front
            pitch = max([self.chunk_samples] + (list(front.input_chunk) if front is not None else []))
            self.staging = torch.zeros((self.slots, 1, pitch), dtype=torch.float32, device=self.state.device)
            self._staged = self.staging.split(1, dim=0)
        for i in range(min(int(private), self.slots)):
            self._private_state(i)
        return self

    def open(self, input_rate: Optional[int] = None, *, output_rate: Optional[int] = None, output_format: Optional[str] = None,
             input_format: Optional[str] = None) -> Session:
        """A session for a stream that begins now.  ``input_rate``: the rate its audio arrives at, one of the declared ``input_rates``
        (None or ``model_rate``: the model's own); ``ValueError`` for a rate that was not declared.

        ``output_format`` (one of ``corpus.FORMATS``): ``step`` and ``close`` return this session's samples as a uint8 device tensor of
        ``k * bytes per sample`` bytes, a view into ``pool.image`` -- the image of that run, freshly allocated, in which every session's
        bytes are contiguous and start at a 16-byte boundary, so one ``copy_(non_blocking=True)`` to pinned memory moves a whole tick.
        ``output_rate`` (one of the declared ``output_rates``; the model's needs no declaration): the samples leave at that rate, k by
        ``rate.final_outputs`` (``session.output_lookahead`` model-rate samples are held back until ``close``); alone it gives float32
        ``(1, 1, k)``.  ``session.clipped``: a 0-dim int32 device view of the samples the encoder has clamped (or found NaN) so far.
        ``input_format``: ``step`` takes a uint8 device tensor of ``session.input_chunk_samples * bytes per sample`` bytes of that
        format (any alignment), ``close`` a shorter one; one launch decodes all such sessions of a tick."""
        session = self.book.open(input_rate, output_rate, output_format, input_format)
        if session.egress:   # the counter lives on the device: one that has not been chosen yet is the generator's
            self.prepare(self.state.device if self.state is not None else next(self.generator.parameters()).device)
            session.clipped = self.back.count(session.slot)
            session.clipped.zero_()
        return session

    def _leave(self, src, sessions, final, enhanced: list) -> None:
        """The way out of one run: ``src`` its compact ``enhanced`` (rows, 1, k) or None, row a that of ``sessions[a]``.  One
        ``eben_stream_pcm_out`` for all sessions that leave as PCM or at a rate; ``enhanced[a]`` becomes that session's view of the image."""
        import torch

        from . import rate

        k = 0 if src is None else src.shape[2]
        mine = [(a, s) for a, s in enumerate(sessions) if s.egress]
        pieces, ranges, nbytes = self.book.back.emit([(s.slot, a, k, s is final) for a, s in mine])
        if pieces:
            self.image = self.back.run(pieces, nbytes, src)
        else:
            self.image = torch.empty(16, dtype=torch.uint8, device=self.state.device)
        for a, s in mine:
            off, n = ranges[s.slot]
            if s.output_format is None:
                enhanced[a] = self.image[off : off + 4 * n].view(torch.float32).view(1, 1, n)
            else:
                enhanced[a] = self.image[off : off + n * rate.PCM_BYTES[rate.PCM_FORMATS.index(s.output_format)]]

    def _private_state(self, i: int):
        from . import gen_engine

        if i not in self.private:
            self.private[i] = gen_engine.engine_of(self.generator).stream_state(self.plan, 1, self.state.device)
        return self.private[i]

    def _results(self, out, sessions, results: dict, final=None) -> None:
        """The emitted tensors, a row per session, as what each session's call returns (rows are split in one call: a view per session
        built one by one costs more host time at 64 sessions than the mask does)."""
        import torch

        per_name = [t.split(1, dim=0) if len(sessions) > 1 else (t,) for t in self._emitted(out, len(sessions), self.state.device)]
        if self.back is not None and any(s.egress for s in sessions):
            per_name[0] = list(per_name[0])
            self._leave(out.get("enhanced"), sessions, final, per_name[0])
        for a, s in enumerate(sessions):
            got = (per_name[0][a], per_name[1][a]) if self.return_bands else per_name[0][a]
            if s in results:   # a close at a recording rate whose FIFO completed one more chunk: that push, then the final one
                got = tuple(torch.cat(pair, dim=-1) for pair in zip(results[s], got)) if self.return_bands else torch.cat((results[s], got), dim=-1)
            results[s] = got

    def _decode(self, chunks: dict) -> dict:
        """The sessions that push PCM bytes: one ``eben_pcm_chunks_in`` for all of them, their chunks replaced by views of the staging buffer."""
        from . import rate

        pcm = [(s, c) for s, c in chunks.items() if s.input_format is not None]
        if not pcm:
            return chunks
        table = []
        for s, c in pcm:
            fmt = rate.PCM_FORMATS.index(s.input_format)
            n = c.numel() // rate.PCM_BYTES[fmt]
            table.append((c, n, fmt, s.slot))
            chunks[s] = self._staged[s.slot][:, :, :n]
        rate.pcm_chunks_in(table, self.staging.view(self.slots, self.staging.shape[2]))
        return chunks

    def _check_bytes(self, chunk, session: Session, what: str) -> None:
        """``chunk``: a session's PCM bytes, one chunk of them, or fewer whole samples in the call that ends the stream."""
        import torch

        from . import rate

        b = rate.PCM_BYTES[rate.PCM_FORMATS.index(session.input_format)]
        want, last = session.input_chunk_samples * b, what == self._last
        if (not isinstance(chunk, torch.Tensor) or chunk.dtype is not torch.uint8 or chunk.dim() != 1 or chunk.stride(0) != 1 or chunk.numel() % b
                or not (chunk.numel() < want if last else chunk.numel() == want)):
            got = f"{chunk.dtype} {tuple(chunk.shape)}" if isinstance(chunk, torch.Tensor) else type(chunk).__name__
            raise ValueError(f"{self._who}: {what} expects a uint8 ({want},) tensor of {session.input_format} bytes{self._per}"
                             f"{' or a shorter last one of whole samples' if last else ''}, got {got}")
        if not chunk.is_cuda:
            from ._lib import EbenError

            raise EbenError(f"{self._who} runs only on an MI355X HIP device (got a tensor on '{chunk.device}'); there is no CPU path")

    def _execute(self, entries, chunks, final_entry=None) -> dict:
        import torch

        from . import gen_engine

        engine = gen_engine.engine_of(self.generator)
        results = {}
        for e in entries:
            if isinstance(e, PooledRun):
                compact = chunks[e.order[0]] if len(e.order) == 1 else torch.cat([chunks[s] for s in e.order], dim=0)
                self._results(engine.stream_run_pooled(self.state, self.plan.steady, compact, e.mask, len(e.order)), e.order, results)
            elif isinstance(e, FrontRun):
                self.tapes.run(e.splices, e.pieces, {s.slot: chunks[s] for s in e.order if s in chunks})
            elif isinstance(e, Hand):
                chunks.pop(e.session, None)
                if e.chunk is not None:
                    chunks[e.session] = self.tapes.chunk(e.chunk)
            elif isinstance(e, PrivatePush):
                state = self._private_state(e.private)
                if e.fresh:
                    state.reset()
                self._results(engine.stream_run(state, e.ops, chunks.get(e.session)), (e.session,), results, e.session if e is final_entry else None)
            else:
                engine.stream_move(self.state, e.slot, self._private_state(e.private), self.book.moved, e.into_pool)
        return results

    def step(self, chunks: dict) -> dict:
        """One tick: ``{session: chunk}`` -> ``{session: newly final samples}`` (``(enhanced, bands)`` with ``return_bands``)."""
        self._no_grad("step")
        if not isinstance(chunks, dict):
            raise ValueError(f"StreamPool: step expects a dict of session -> chunk, got {type(chunks).__name__}")
        self.book.check(chunks)
        for s, chunk in chunks.items():
            if s.input_format is not None:
                self._check_bytes(chunk, s, "step")
            else:
                self._check(chunk, 1, "step", s.input_chunk_samples)
        if not chunks:
            return {}
        chunks = {s: c.contiguous() for s, c in chunks.items()}
        self.prepare(next(iter(chunks.values())).device)
        results = self._execute(self.book.tick(chunks), self._decode(dict(chunks)))
        if len(results) < len(chunks):   # a stream at a recording rate completes no chunk at its first push
            got = self._emitted({}, 1, self.state.device)
            nothing = tuple(got) if self.return_bands else got[0]
            return {s: results[s] if s in results else self._nothing(s, nothing) for s in chunks}
        return {s: results[s] for s in chunks}

    def _nothing(self, session: Session, nothing):
        """What a session gets in a tick that ran nothing for it."""
        import torch

        if session.output_format is None:
            return nothing
        empty = torch.empty(0, dtype=torch.uint8, device=self.state.device)
        return (empty, nothing[1]) if self.return_bands else empty

    def close(self, session: Session, tail=None):
        """The rest of ``session``'s stream, as ``StreamingEnhancer.finish``; its slot is free for the next ``open()``."""
        import torch

        self._no_grad("close")
        self.book.check([session])
        if tail is not None and isinstance(tail, torch.Tensor) and tail.shape[-1] == 0:
            tail = None
        if tail is not None:
            if session.input_format is not None:
                self._check_bytes(tail, session, "close")
            else:
                self._check(tail, 1, "close", session.input_chunk_samples)
            tail = tail.contiguous()
        self.prepare(tail.device if tail is not None else self.state.device if self.state is not None
                     else next(self.generator.parameters()).device)
        chunks = {} if tail is None else self._decode({session: tail})
        entries = self.book.close(session, 0 if tail is None else chunks[session].shape[2])
        got = self._execute(entries, chunks, entries[-1])[session]
        if session.egress:
            self.book.back.release(session.slot)
        return got
