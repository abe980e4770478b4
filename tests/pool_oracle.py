"""Test-side float64 executor of a ``vibravox_amd.streaming.PoolBook`` (TEST INFRASTRUCTURE): the per-tick entry lists of the
bookkeeping, run on poisoned float64 buffers with the layers of ``tests/stream_oracle.py``.

The masked splice below is written from the semantics ``include/eben_hip.h`` states for ``eben_stream_splice_rows`` and is the
specification of that kernel: with a = the number of active slots below r, an active slot r gets ``[prev[r] | src (+ add)]`` -- src and
add at row a when the source is the compact input, at row r otherwise --, written at row a of a compact destination (an emit) or at
row r; an inactive slot gets ``idle[r, :, :carry + new]`` when the tape holds state and nothing otherwise.

Poison: NaN sits in every slot of the shared state that holds no pooled session (a slot is refilled with NaN when its session moves
out), in every buffer outside ``[carry | new]`` (the twin buffer is refilled with NaN before each splice, so an inactive slot without
``idle`` reads NaN, which is stricter than "writes nothing"), and over every layer output outside its exact range.
"""
import torch

from tests import stream_oracle as S
from vibravox_amd import streaming

NAN = S.NAN


class _PoolState(S.OracleStream):
    """``slots`` rows of steady-state buffers; ``run_steady`` is one masked run of ``plan.steady``."""

    def __init__(self, gen, sd, chunk_samples, slots):
        super().__init__(gen, sd, chunk_samples, rows=slots)
        for t in self.plan.tensors:
            self.length[t.name] = t.length

    def _masked(self, op, chunks, active, emitted):
        total = op.n_carry + op.n_new
        kind, key = op.dst.split(":", 1)
        if total == 0:
            assert kind == "tape"
            self.length[key] = 0
            return
        compact_src = op.src == "input"

        def rows_of(name, off, n, compact):
            t, length = self._read(name, chunks)
            assert 0 <= off and off + n <= length, op
            return [t[(a if compact else r)][:, off : off + n] for a, r in enumerate(active)]

        parts = [[] for _ in active]
        if op.n_carry:
            for p, x in zip(parts, rows_of(op.prev, op.prev_off, op.n_carry, False)):
                p.append(x)
        if op.n_new:
            new = rows_of(op.src, op.src_off, op.n_new, compact_src)
            if op.add is not None:
                new = [x + y for x, y in zip(new, rows_of(op.add, op.add_off, op.n_new, compact_src))]
            for p, x in zip(parts, new):
                p.append(x)
        spliced = [torch.cat(p, dim=1) for p in parts]
        if kind == "emit":
            emitted[key] = torch.stack(spliced).clone()   # compact: one row per active slot, in slot order
            return
        assert total <= self.bufs[key][0].shape[2], (op, "past the plan's capacity")
        cur, other = self.bufs[key][self.cur[key]], self.bufs[key][1 - self.cur[key]]
        assert self.length[key] == total or key == "lift.operand", op
        other.fill_(NAN)
        if key != "lift.operand":                         # idle = the tape's current view: the state of the others moves over unchanged
            other[:, :, :total] = cur[:, :, :total]
        for r, x in zip(active, spliced):
            other[r].fill_(NAN)
            other[r][:, :total] = x
        self.cur[key], self.length[key] = 1 - self.cur[key], total

    def run_steady(self, chunks, mask):
        active = [r for r in range(self.rows) if (mask[r >> 6] >> (r & 63)) & 1]
        assert chunks.shape[0] == len(active) > 0
        emitted = {}
        for op in self.plan.steady:
            if isinstance(op, streaming.Splice):
                self._masked(op, chunks, active, emitted)
            else:
                self._launch(op)
        return emitted

    def poison_slot(self, r):
        for pair in self.bufs.values():
            for t in pair:
                t[r].fill_(NAN)


class OraclePool:
    """``open`` / ``step`` / ``close`` like ``streaming.StreamPool``, float64 on the CPU; ``log`` keeps every entry executed."""

    def __init__(self, gen, sd, chunk_samples, slots):
        self.gen, self.sd, self.chunk = gen, sd, chunk_samples
        self.book = streaming.PoolBook(gen, chunk_samples, slots)
        self.pool = _PoolState(gen, sd, chunk_samples, slots)
        self.private = {}
        self.log = []

    def open(self):
        return self.book.open()

    def _private(self, i):
        if i not in self.private:
            self.private[i] = S.OracleStream(self.gen, self.sd, self.chunk)
        return self.private[i]

    def _fresh(self, st):
        for name, pair in st.bufs.items():
            for t in pair:
                t.fill_(NAN)
            st.cur[name] = st.length[name] = 0
        st.out = {}

    def _move(self, e):
        st = self._private(e.private)
        lengths = {t.name: t.length for t in self.pool.plan.tensors}
        if not e.into_pool:
            self._fresh(st)
        for name in self.book.moved:
            n = lengths[name]
            row = self.pool.bufs[name][self.pool.cur[name]][e.slot]
            if e.into_pool:
                assert st.length[name] == n == self.pool.length[name], name
                row.fill_(NAN)
                row[:, :n] = st.bufs[name][st.cur[name]][0, :, :n]
            else:
                st.bufs[name][st.cur[name]][0, :, :n] = row[:, :n]
                st.length[name] = n
        if not e.into_pool:
            self.pool.poison_slot(e.slot)

    def _result(self, emitted, row):
        m = self.gen.pqmf.decimation
        out = []
        for name, c in (("enhanced", 1), ("bands", m)):
            t = emitted.get(name)
            t = torch.zeros(1, c, 0, dtype=torch.float64) if t is None else t if row is None else t[row : row + 1]
            out.append(t)
        return tuple(out)

    def _execute(self, entries, chunks):
        results = {}
        for e in entries:
            self.log.append(e)
            if isinstance(e, streaming.PooledRun):
                emitted = self.pool.run_steady(torch.cat([chunks[s] for s in e.order], dim=0), e.mask)
                for a, s in enumerate(e.order):
                    results[s] = self._result(emitted, a)
            elif isinstance(e, streaming.PrivatePush):
                st = self._private(e.private)
                if e.fresh:
                    self._fresh(st)
                chunk = chunks.get(e.session, torch.zeros(1, 1, 0, dtype=torch.float64))
                emitted = {}
                for op in e.ops:
                    if isinstance(op, streaming.Splice):
                        st._splice(op, chunk, emitted)
                    else:
                        st._launch(op)
                results[e.session] = self._result(emitted, None)
            else:
                self._move(e)
        return results

    def step(self, chunks):
        results = self._execute(self.book.tick(chunks), chunks)
        return {s: results[s] for s in chunks}

    def close(self, session, tail=None):
        n = 0 if tail is None else tail.shape[2]
        return self._execute(self.book.close(session, n), {} if n == 0 else {session: tail})[session]


# ---- the scenario of the pool tests: sessions that come, pause and go at different ticks ----------------------------------------------
def scenario(lengths):
    """(name, samples, opening tick or the name of the session whose closing it follows, ticks skipped) per session."""
    a, b, c, d, e = lengths
    return (("A", a, 0, ()), ("B", b, 5, ()), ("C", c, 9, (12, 13, 30, 31)), ("D", d, 2, ()), ("E", e, "A", ()))


SCENARIO_256 = (8000, 6500, 5000, 3000, 8000)
SCENARIO_1024 = (12000, 12000, 12000, 3000, 12000)


def run_scenario(pool, clips, chunk, spec):
    """Drives ``pool`` (an ``OraclePool`` or a ``StreamPool``) through ``spec`` with ``clips[name]`` (1, 1, T) on the pool's device.  A session
    pushes a chunk every tick it does not skip while a whole chunk is left, then closes with its tail.  Returns per session name the
    list of returns (a pair (enhanced, bands) each) in order, and the slot it had."""
    pending = {name: (total, start, set(skips)) for name, total, start, skips in spec}
    live, pos, outs, slots = {}, {}, {name: [] for name in pending}, {}
    tick = 0
    closed = set()
    while pending or live:
        for name, (total, start, skips) in list(pending.items()):
            if start == tick or (isinstance(start, str) and start in closed):
                live[name] = (pool.open(), total, skips)
                slots[name], pos[name] = live[name][0].slot, 0
                del pending[name]
        feed, ending = {}, []
        for name, (session, total, skips) in live.items():
            if tick in skips:
                continue
            if total - pos[name] >= chunk:
                feed[session] = clips[name][:, :, pos[name] : pos[name] + chunk]
                pos[name] += chunk
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
    return outs, slots
