"""Test-side float64 executor of ``vibravox_amd.rate.SlotFront`` and of a ``streaming.PoolBook`` with rated sessions (TEST INFRASTRUCTURE).

``OracleTapes`` is written from the semantics ``include/eben_hip.h`` states for ``eben_rate_splice_slots`` and ``eben_resample_slots`` and
is the specification of those two kernels: a splice writes ``[carry | new]`` of the named slot into the named tape from the OTHER tape
and from row ``src_row`` of the compact input of its pushed length; a piece sums a tap row as ``tests/rate_oracle.py`` does -- products in
ascending j, indices outside ``[0, len)`` an exact 0.0 -- so what a session's FIFO hands on can be compared with the whole-signal sum for
EQUALITY.

Poison: NaN sits in every slot without a session (nothing ever writes there), in a tape outside ``[carry | new]`` (the row is refilled
with NaN before each splice and the tape just read is poisoned at once: the next launch must read the twin), and in a FIFO buffer
behind what is held (the row is refilled with NaN when a piece starts it at 0).
"""
import numpy as np
import torch

from tests import pool_oracle as P
from tests import rate_oracle as RO
from vibravox_amd import augment, rate, streaming

NAN = float("nan")


class OracleTapes:
    """``rate.SlotTapes`` in float64 on the CPU: ``run(splices, pieces, inputs)`` and ``chunk(c)``."""

    def __init__(self, front):
        self.front = front
        self.tapes = np.full((2, front.slots, front.tape_samples), NAN)
        self.fifo = np.full((2, front.slots, front.chunk_samples), NAN)
        self.tables = [augment.sinc_resample_kernel(r, front.model_rate)[0].numpy().astype(np.float64) for r in front.rates]
        self.log = []   # (splices, pieces) of every run

    def run(self, splices, pieces, inputs):
        """``inputs``: slot -> the float64 samples (n,) it pushes."""
        self.log.append((tuple(splices), tuple(pieces)))
        cap = self.front.tape_samples
        compact = {}   # pushed length -> the rows of that compact input, in the order of the list
        for s in splices:
            if s.n_new:
                compact.setdefault(s.n_new, []).append(np.asarray(inputs[s.slot], dtype=np.float64))
        seen = set()
        for s in splices:
            assert s.slot not in seen and 0 <= s.slot < self.front.slots and s.tape in (0, 1), s
            seen.add(s.slot)
            total = s.n_carry + s.n_new
            assert 0 < total <= cap and s.n_carry >= 0 and s.n_new >= 0, s
            out, inp = self.tapes[s.tape], self.tapes[1 - s.tape]
            row = np.full(cap, NAN)
            if s.n_carry:
                assert 0 <= s.prev_off and s.prev_off + s.n_carry <= cap, s
                row[: s.n_carry] = inp[s.slot, s.prev_off : s.prev_off + s.n_carry]
            if s.n_new:
                src = compact[s.n_new][s.src_row]
                assert src.shape == (s.n_new,), (s, src.shape)
                row[s.n_carry : total] = src
            out[s.slot] = row
            inp[s.slot] = NAN
        for p in pieces:
            orig, new, width = self.front.ratios[p.ratio]
            assert 0 <= p.first_out and p.first_out + p.n_out <= self.front.chunk_samples and p.n_out > 0, p
            values, _ = RO.tape_outputs(self.tables[p.ratio], self.tapes[p.tape][p.slot][None], p.length, p.p0, p.base0, p.n_out, orig, new, p.end)
            row = self.fifo[p.fifo][p.slot]
            if p.first_out == 0:
                row[:] = NAN
            assert np.isnan(row[p.first_out : p.first_out + p.n_out]).all(), (p, "two pieces write one range")
            row[p.first_out : p.first_out + p.n_out] = values[0]

    def chunk(self, c):
        return self.fifo[c.fifo][c.slot, : c.samples].copy()


class RatedOraclePool(P.OraclePool):
    """``tests.pool_oracle.OraclePool`` for a book with ``input_rates``: the front's two lists run in float64 before the entries it knows."""

    def __init__(self, gen, sd, chunk_samples, slots, input_rates=(), model_rate=16000):
        super().__init__(gen, sd, chunk_samples, slots)
        self.book = streaming.PoolBook(gen, chunk_samples, slots, input_rates=input_rates, model_rate=model_rate)
        self.tapes = OracleTapes(self.book.front) if self.book.front is not None else None

    def open(self, input_rate=None):
        return self.book.open(input_rate)

    def _execute(self, entries, chunks):
        chunks, results = dict(chunks), {}
        for e in entries:
            if isinstance(e, streaming.FrontRun):
                self.log.append(e)
                self.tapes.run(e.splices, e.pieces, {s.slot: chunks[s][0, 0].numpy() for s in e.order if s in chunks})
            elif isinstance(e, streaming.Hand):
                self.log.append(e)
                chunks.pop(e.session, None)
                if e.chunk is not None:
                    chunks[e.session] = torch.from_numpy(self.tapes.chunk(e.chunk)).reshape(1, 1, -1)
            else:
                for s, got in super()._execute([e], chunks).items():
                    results[s] = tuple(torch.cat(pair, dim=2) for pair in zip(results[s], got)) if s in results else got
        return results

    def step(self, chunks):
        results = self._execute(self.book.tick(chunks), chunks)
        return {s: results.get(s, self._result({}, None)) for s in chunks}


# ---- scenarios with mixed rates: tests.pool_oracle.scenario's comings and goings, every session at a rate of its own --------------------
def rated_scenario(lengths, rates, model_rate=16000):
    """``P.scenario(lengths)`` with a rate per session: (name, INPUT samples, start, skips, rate).  ``lengths`` are at the model's rate; a
    session's input is that long at its own rate, plus a few samples so that the tails differ."""
    out = []
    for i, ((name, total, start, skips), r) in enumerate(zip(P.scenario(lengths), rates)):
        orig, new, _ = rate.ratio(r, model_rate)
        out.append((name, total if r == model_rate else total * orig // new + i, start, skips, r))
    return tuple(out)


RATES_256 = (48000, 32000, 8000, 16000, 48000)      # A ... E of the scenario on 4 slots
RATES_1280 = (48000, 44100, 24000, 8000, 16000)     # ... on 5 slots
SCENARIO_1280 = (12000, 12000, 12000, 4000, 12000)


def run_rated_scenario(pool, clips, spec):
    """``P.run_scenario`` for sessions at rates of their own: a session pushes ``session.input_chunk_samples`` of ``clips[name]`` every
    tick it does not skip while that many are left, then closes with its tail.  Returns (per name the list of returns, slots, sessions)."""
    pending = {name: (total, start, set(skips), r) for name, total, start, skips, r in spec}
    live, pos, outs, slots, sessions = {}, {}, {name: [] for name in pending}, {}, {}
    tick, closed = 0, set()
    while pending or live:
        for name, (total, start, skips, r) in list(pending.items()):
            if start == tick or (isinstance(start, str) and start in closed):
                live[name] = (pool.open(r), total, skips)
                sessions[name] = live[name][0]
                slots[name], pos[name] = live[name][0].slot, 0
                del pending[name]
        feed, ending = {}, []
        for name, (session, total, skips) in live.items():
            if tick in skips:
                continue
            n = session.input_chunk_samples
            if total - pos[name] >= n:
                feed[session] = clips[name][:, :, pos[name] : pos[name] + n]
                pos[name] += n
            else:
                ending.append(name)
        by_session = {live[name][0]: name for name in live}
        for session, res in pool.step(feed).items():
            outs[by_session[session]].append(res)
        for name in ending:
            session, total, _ = live.pop(name)
            outs[name].append(pool.close(session, clips[name][:, :, pos[name] : total]))
            closed.add(name)
        tick += 1
        assert tick < 400
    return outs, slots, sessions
