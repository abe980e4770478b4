"""CPU: independent streaming sessions (vibravox_amd/streaming.py: ``Schedule.advance``, ``PoolBook``, ``StreamPool``) -- the schedule
advanced without pushes, the bookkeeping's per-tick lists executed in float64 on poisoned buffers (tests/pool_oracle.py), and the
refusals of the pool and of the two host entries ``eben_stream_splice_rows`` / ``eben_copy_segments``.

Bound of the float64 comparison: 1e-12, the bar of test_stream_plan.py (the same float64 convolutions on the same values; only where a
sample sits inside the tensor handed to the convolution differs)."""
import copy
import ctypes
import functools
import os

import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests import pool_oracle as P
from tests import ragged_oracle as R
from vibravox_amd import ragged, streaming


@functools.lru_cache(maxsize=None)
def generator(n):
    return R.formula_generator(2, n)


def fields(sch):
    return ({k: (t.S, t.F, t.keep) for k, t in sch.tapes.items()}, dict(sch.out_f), dict(sch.emitted), sch.pushed, sch.finished)


def to_steady(gen, chunk, steady):
    sch = streaming.Schedule(gen, chunk)
    for _ in range(4096):
        if tuple(sch.push(chunk)) == steady:
            return sch
    raise AssertionError("no steady push")


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("n", [32, 512])
def test_advance_equals_the_pushes_it_stands_for(n, chunk):
    gen, _ = generator(n)
    steady = streaming.plan(gen, chunk).steady
    pushed = to_steady(gen, chunk, steady)    # pushed on and on below: k pushes past the first steady one at each stop
    done = 0
    for k in (0, 1, 7, 1000):
        for _ in range(k - done):
            assert tuple(pushed.push(chunk)) == steady
        done = k
        jumped = to_steady(gen, chunk, steady)
        jumped.advance(k)
        assert fields(jumped) == fields(pushed), k
        a, b = copy.deepcopy(jumped), copy.deepcopy(pushed)
        assert a.push(chunk) == b.push(chunk) == list(steady) and fields(a) == fields(b)
        a, b = copy.deepcopy(jumped), copy.deepcopy(pushed)
        assert a.push(100, final=True) == b.push(100, final=True) and fields(a) == fields(b)
        jumped.advance(0)
        jumped.advance(3)                     # ... and again from an advanced schedule
        b = copy.deepcopy(pushed)
        for _ in range(3):
            b.push(chunk)
        assert fields(jumped) == fields(b)


def test_advance_refuses_outside_the_steady_state():
    gen, _ = generator(32)
    sch = streaming.Schedule(gen, 256)
    with pytest.raises(RuntimeError, match="steady"):
        sch.advance(1)
    for _ in range(3):
        sch.push(256)
    with pytest.raises(RuntimeError, match="steady"):
        sch.advance(1)
    with pytest.raises(RuntimeError, match="steady"):
        sch.advance(0)
    sch = to_steady(gen, 256, streaming.plan(gen, 256).steady)
    with pytest.raises(ValueError):
        sch.advance(-1)
    sch.advance(2)
    sch.push(100, final=True)
    with pytest.raises(RuntimeError, match="finished"):
        sch.advance(1)


# ---- the pool in float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk,lengths", [(32, 256, P.SCENARIO_256), (512, 256, P.SCENARIO_256), (32, 1024, P.SCENARIO_1024)])
def test_pool_sessions_equal_their_own_whole_clips(n, chunk, lengths):
    gen, sd = generator(n)
    spec = P.scenario(lengths)
    clips = {name: formula_audio(f"pool/{name}", 1, total).double() for name, total, _, _ in spec}
    pool = P.OraclePool(gen, sd, chunk, slots=4)
    outs, slots = P.run_scenario(pool, clips, chunk, spec)
    assert slots["E"] == slots["A"] and len({slots[k] for k in "ABC"}) == 3   # (at chunk 1024 D has gone before B comes)
    worst = 0.0
    for name, total, _, _ in spec:
        cut = ragged.cut_length(gen, total)
        o_enh, o_bands = O.generator_forward(sd, clips[name][:, :, :cut], 2)
        enhanced, bands = torch.cat([o[0] for o in outs[name]], dim=2), torch.cat([o[1] for o in outs[name]], dim=2)
        assert enhanced.shape == o_enh.shape == (1, 1, cut) and bands.shape == o_bands.shape
        assert not torch.isnan(enhanced).any() and not torch.isnan(bands).any(), name
        err = max(float((enhanced - o_enh).abs().max()), float((bands - o_bands).abs().max()))
        assert err < 1e-12, (name, err)
        worst = max(worst, err)
        sizes = [o[0].shape[2] for o in outs[name][:-1]]
        first = next((i for i, k in enumerate(sizes) if k), len(sizes))
        assert all(k == 0 for k in sizes[:first]) and all(k == chunk for k in sizes[first:]), (name, sizes)
    # who was pooled: every session but D, which closes while warming -- by the list, so private pushes alone cannot pass
    runs = [e for e in pool.log if isinstance(e, streaming.PooledRun)]
    pooled_ticks = {}
    by_session = {}
    for e in pool.log:
        if isinstance(e, streaming.Move):
            by_session.setdefault(e.session, []).append(e.into_pool)
    assert all(v == [True, False] for v in by_session.values()) and len(by_session) == 4
    moved_slots = sorted(e.slot for e in pool.log if isinstance(e, streaming.Move) and e.into_pool)
    assert moved_slots == sorted([slots["A"], slots["B"], slots["C"], slots["E"]])
    for run in runs:
        assert sum(bin(w).count("1") for w in run.mask) == len(run.order) >= 1
        assert [s.slot for s in run.order] == sorted(s.slot for s in run.order)
        for s in run.order:
            assert (run.mask[s.slot >> 6] >> (s.slot & 63)) & 1
            pooled_ticks[s] = pooled_ticks.get(s, 0) + 1
    per_session = list(pooled_ticks.values())
    assert len(per_session) == 4 and min(per_session) >= 1
    assert any(len(run.order) >= 2 for run in runs) and any(len(run.order) == 1 for run in runs)
    assert pool.book.free_slots == [0, 1, 2, 3] and pool.book.n_private <= 4
    print(f"n {n} chunk {chunk}: worst |pool - whole clip| {worst:.1e}, {len(runs)} pooled runs, pooled pushes per session {sorted(per_session)}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_the_book_refuses_misuse():
    gen, _ = generator(32)
    book = streaming.PoolBook(gen, 256, slots=2)
    a, b = book.open(), book.open()
    assert (a.slot, b.slot) == (0, 1)
    with pytest.raises(RuntimeError, match="slots"):
        book.open()
    other = streaming.PoolBook(gen, 256, slots=2).open()
    with pytest.raises(ValueError, match="not a session of this pool"):
        book.tick([other])
    with pytest.raises(ValueError, match="twice"):
        book.tick([a, a])
    with pytest.raises(ValueError, match="not a session"):
        book.tick(["a"])
    with pytest.raises(ValueError, match="too short"):
        book.close(a, 100)                   # nothing pushed: below the shortest clip; the session stays open
    assert a.phase == "warming" and book.tick([a])
    for _ in range(4):
        book.tick([a, b])
    assert book.close(a, 10) and a.phase == "closed"
    with pytest.raises(RuntimeError, match="closed"):
        book.tick([a])
    with pytest.raises(RuntimeError, match="closed"):
        book.close(a)
    assert book.open().slot == 0             # the freed slot
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match="slots"):
            streaming.PoolBook(gen, 256, slots=bad)
    with pytest.raises(ValueError, match="multiple of 256"):
        streaming.PoolBook(gen, 300)


def test_the_pool_refuses_misuse_before_it_touches_a_device():
    gen, _ = generator(32)
    pool = streaming.StreamPool(gen, 256, slots=1)
    assert pool.latency == pool.plan.latency and pool.lookahead == pool.plan.lookahead and pool.chunk_samples == 256
    s = pool.open()
    with pytest.raises(RuntimeError, match="slots"):
        pool.open()
    good = torch.zeros(1, 1, 256)
    with pytest.raises(RuntimeError, match="no backward"):
        pool.step({s: good})
    with pytest.raises(RuntimeError, match="no backward"):
        pool.close(s)
    with torch.no_grad():
        for bad in (torch.zeros(2, 1, 256), good[:, :, :255], torch.zeros(1, 1, 512), good[0], good.double(), torch.zeros(1, 2, 256), None):
            with pytest.raises(ValueError, match="expects"):
                pool.step({s: bad})
        with pytest.raises(ValueError, match="expects"):
            pool.close(s, good)              # a whole chunk is a step
        with pytest.raises(ValueError, match="dict"):
            pool.step([s])
        with pytest.raises(ValueError, match="not a session of this pool"):
            pool.step({streaming.StreamPool(gen, 256, slots=1).open(): good})
        from vibravox_amd._lib import EbenError

        with pytest.raises(EbenError, match="no CPU path"):
            pool.step({s: good})
        with pytest.raises(EbenError, match="no CPU path"):
            pool.close(s, good[:, :, :100])
        assert s.phase == "warming" and s.pushes == 0   # nothing above has moved the session
        assert pool.step({}) == {}


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_splice_rows_argument_errors_without_gpu(lib):
    """The host entry refuses bad arguments before any launch (EBEN_EINVAL = -1 and a message)."""
    V = ctypes.c_void_p
    dst, prev, src, add, idle = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000   # never dereferenced: every call below is refused

    def call(dst=dst, dp=100, prev=prev, pp=50, po=10, nc=40, src=src, sp=60, so=0, nn=60, add=add, ap=70, ao=10, idle=idle, ip=100, rc=24, ch=8,
             mask=(0b101,), sc=0, dc=0, null_mask=False):
        words = None if null_mask else (ctypes.c_uint64 * 4)(*mask)
        return lib.eben_stream_splice_rows(V(dst), dp, V(prev), pp, po, nc, V(src), sp, so, nn, V(add), ap, ao, V(idle), ip, rc, ch, words, sc, dc, None)

    msg = lib.eben_last_error
    for k in ("dst", "prev", "src"):
        assert call(**{k: 0}) == -1 and b"null" in msg(), k
    assert call(null_mask=True) == -1 and b"null" in msg()
    for k in ("dst", "prev", "src", "add", "idle"):
        assert call(**{k: 0x600002}) == -1 and b"misaligned" in msg(), k
    assert call(po=11) == -1 and b"prev" in msg()
    assert call(so=1) == -1 and b"src" in msg()
    assert call(ao=11) == -1 and b"add" in msg()
    assert call(dp=99) == -1 and b"dst" in msg()
    assert call(ip=99) == -1 and b"idle" in msg()       # carry + new past idle's pitch
    assert call(po=-1) == -1 and call(so=-1) == -1 and call(ao=-1) == -1 and call(nc=-1) == -1 and call(nn=-1) == -1
    assert call(nc=0, nn=0) == -1 and call(rc=0) == -1
    assert call(ch=7) == -1 and b"multiple" in msg()
    assert call(ch=0) == -1 and b"multiple" in msg()
    assert call(rc=257 * 8) == -1 and b"slots" in msg()
    assert call(mask=(0b1000,)) == -1 and b"at or above" in msg()           # 3 slots: bit 3
    assert call(rc=70 * 8, mask=(1, 1 << 6)) == -1 and b"at or above" in msg()   # 70 slots: bit 70
    assert call(prev=dst + 4 * (24 * 100 - 1)) == -1 and b"overlaps prev" in msg()   # the last float of dst's extent
    assert call(src=dst - 4 * (24 * 60 - 1)) == -1 and b"overlaps src" in msg()      # the last float of src's extent
    assert call(add=dst) == -1 and b"overlaps add" in msg()
    assert call(idle=dst + 4 * 100) == -1 and b"overlaps idle" in msg()
    # compact extents count the active slots: two of three here
    assert call(src=dst - 4 * (16 * 60 - 1), sc=1) == -1 and b"overlaps src" in msg()
    assert call(prev=dst + 4 * (16 * 100 - 1), dc=1) == -1 and b"overlaps prev" in msg()


def test_copy_segments_argument_errors_without_gpu(lib):
    from vibravox_amd._lib import EbenCopySegment

    def call(segs, count=None):
        table = (EbenCopySegment * max(1, len(segs)))(*[EbenCopySegment(d, s, n) for d, s, n in segs])
        return lib.eben_copy_segments(table, len(segs) if count is None else count, None)

    msg = lib.eben_last_error
    a, b = 0x100000, 0x200000
    assert call([(0, b, 4)]) == -1 and b"null" in msg()
    assert call([(a, 0, 4)]) == -1 and b"null" in msg()
    assert call([(a + 2, b, 4)]) == -1 and b"misaligned" in msg()
    assert call([(a, b + 1, 4)]) == -1 and b"misaligned" in msg()
    assert call([(a, b, -1)]) == -1 and b"floats" in msg()
    assert call([(a, b, 4)], count=-1) == -1 and b"segments" in msg()
    assert call([(a + 64 * i, b + 64 * i, 4) for i in range(65)]) == -1 and b"segments" in msg()
    assert call([(a, a + 12, 4)]) == -1 and b"overlaps src" in msg()                       # its own source, by the last float
    assert call([(a, b, 4), (a + 64, a - 12, 4)]) == -1 and b"overlaps src" in msg()       # another segment's source
    assert call([(a, b, 4), (a + 12, b + 64, 4)]) == -1 and b"overlaps dst" in msg()
    assert lib.eben_copy_segments(None, 1, None) == -1 and b"null" in msg()
    assert call([], count=0) == 0 and call([(a, b, 0), (a, b, 0)]) == 0                    # nothing to copy: no launch
