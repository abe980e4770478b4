"""Float64 oracle of the resampling routes (``vibravox_amd/rate.py``, ``csrc/rate.hip``): the direct sum with the float32 table cast
up, and an executor of ``rate.Schedule``'s pushes on NaN-poisoned tapes.

Both sum a tap row the same way -- products in ascending j, accumulated one after the other, indices outside the signal contributing
an exact 0.0 -- so a streamed signal can be compared with the whole-signal sum for EQUALITY, not closeness."""
import numpy as np


def tape_outputs(k64, tape, length, p0, base0, n_out, orig, new, end):
    """Outputs of a launch on ``tape`` (rows, capacity) float64, of which [0, length) is the buffer: output n has phase (p0 + n) % new and
    its tap 0 at index base0 + ((p0 + n) // new) * orig.  Returns (values (rows, n_out), sum_j |k_j x_j| (rows, n_out)).  Indices outside
    [0, length) are never read; when the right end is not the signal's own (``end`` False) asking for one at or behind ``length`` is a
    mistake of the plan and fails here."""
    rows, taps = tape.shape[0], k64.shape[1]
    if n_out == 0:
        return np.zeros((rows, 0)), np.zeros((rows, 0))
    q, p = np.divmod(p0 + np.arange(n_out, dtype=np.int64), new)
    idx = (base0 + q * orig)[:, None] + np.arange(taps, dtype=np.int64)[None, :]
    if not end:
        assert idx.max() < length, f"the plan asks for tape index {idx.max()} of {length} samples that do not end the signal"
    inside = (idx >= 0) & (idx < length)
    xs = tape[:, np.clip(idx, 0, max(length - 1, 0))] if length else np.zeros((rows,) + idx.shape)
    prod = np.where(inside[None], k64[p][None] * xs, 0.0)
    return np.cumsum(prod, axis=2)[:, :, -1], np.abs(prod).sum(axis=2)


def direct(x64, table, orig, new, width):
    """The whole-signal sum: ``x64`` (rows, T) float64, ``table`` the float32 (new, taps) kernel table.  (values, sum |k x|), each
    (rows, ceil(new T / orig))."""
    k64 = np.asarray(table, dtype=np.float64)
    assert k64.shape == (new, 2 * width + orig)
    t = x64.shape[1]
    return tape_outputs(k64, x64, t, 0, -width, -(-new * t // orig), orig, new, True)


def run_schedule(schedule, table, signal, chunks, capacity_chunk=None):
    """Pushes ``signal`` (rows, T) float64 through ``schedule`` (a fresh ``rate.Schedule``): ``chunks`` samples per push, then one final
    push with whatever is left (possibly nothing).  The two tapes are ``taps - 1 + capacity_chunk`` long and NaN wherever nothing was
    written; a tape is poisoned again once its twin has taken over.  Returns (the outputs of every call, the ``RatePush`` of each)."""
    k64 = np.asarray(table, dtype=np.float64)
    rows, total = signal.shape
    cap = schedule.taps - 1 + (capacity_chunk if capacity_chunk is not None else max(list(chunks) + [total - sum(chunks), 1]))
    tapes = [np.full((rows, cap), np.nan), np.full((rows, cap), np.nan)]
    cur, pos, outs, ops = 0, 0, [], []
    for n, final in [(c, False) for c in chunks] + [(total - sum(chunks), True)]:
        assert n >= 0 and pos + n <= total
        op = schedule.push(n, final)
        prev, dst = tapes[cur], tapes[cur ^ 1]
        if op.length:
            assert op.length <= cap and op.prev_off >= 0 and op.prev_off + op.n_carry <= cap
            dst[:, : op.n_carry] = prev[:, op.prev_off : op.prev_off + op.n_carry]
            dst[:, op.n_carry : op.length] = signal[:, pos : pos + n]
            prev[:] = np.nan
            cur ^= 1
        values, _ = tape_outputs(k64, dst, op.length, op.p0, op.base0, op.n_out, schedule.orig, schedule.new, op.end)
        outs.append(values)
        ops.append(op)
        pos += n
    return outs, ops
