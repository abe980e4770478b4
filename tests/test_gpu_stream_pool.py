"""GPU: independent streaming sessions -- ``eben_stream_splice_rows`` and ``eben_copy_segments`` through their raw entry points against
torch indexing, bit for bit in fenced, 4-byte-misaligned buffers, and ``streaming.StreamPool`` on the scenario of
tests/test_stream_pool_plan.py (sessions that come, pause and go at different ticks) against the float64 oracle of each session's own
whole clip.

Bars, those of test_gpu_stream.py: max|.| < 2e-5 on enhanced and bands and MSE < 1e-10 against the oracle, and no further from the oracle
than twice the whole-clip device forward of the same clip is, in max and in RMS.  The distance to ``StreamingEnhancer(streams=1)`` on
the same audio is printed, not asserted."""
import ctypes
import functools

import pytest
import torch

from formula import formula_audio
from oracle import eben_oracle as O
from tests import pool_oracle as P
from tests import ragged_oracle as R
from tests.test_gpu_stream import FENCE, dist, fenced, fences_intact, same_bits, stream_through

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def words_of(slots, which):
    active = {"all": range(slots), "none": (), "last": (slots - 1,), "alternate": range(0, slots, 2)}[which]
    words = [0, 0, 0, 0]
    for r in active:
        words[r >> 6] |= 1 << (r & 63)
    return list(active), (ctypes.c_uint64 * 4)(*words)


def inner(dev, rows, pitch):
    return dev[FENCE + 1 : FENCE + 1 + rows * pitch]


# ---- the masked splice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [5, 32])
@pytest.mark.parametrize("slots", [3, 70])
def test_splice_rows_equals_torch_indexing(hip, slots, channels):
    from vibravox_amd._lib import check, stream

    rc = slots * channels
    for n_carry in (0, 9, 700):
        for n_new in (1, 257):
            total = n_carry + n_new
            # a different pitch for each tensor; dst once exactly as long as what is written
            pitch = dict(dst=total + (0 if n_carry == 9 else 3), prev=n_carry + 13, src=n_new + 7, add=n_new + 5, idle=total + 2)
            tag = f"splice_rows/{slots}/{channels}/{n_carry}/{n_new}"
            dev, view, clean = {}, {}, {}
            for k, p in pitch.items():
                _, dev[k], v = fenced(rc, p, f"{tag}/{k}")
                view[k], clean[k] = v.view(slots, channels, p), dev[k].clone()
            plain = clean["dst"].clone()   # where eben_stream_splice writes
            for which in ("all", "none", "last", "alternate"):
                active, words = words_of(slots, which)
                act = torch.tensor(active, dtype=torch.long, device=DEV)
                idle_rows = torch.tensor([r for r in range(slots) if r not in set(active)], dtype=torch.long, device=DEV)
                n_act = len(active)
                for sc in (0, 1):
                    for dc in (0, 1):
                        for with_idle in (False, True):
                            if which == "none" and not with_idle and sc + dc:
                                continue   # nothing to write and no launch: covered once, by the plain form
                            for with_add in (False, True):
                                for last in (False, True):   # offsets 0, then the last ones that fit
                                    po, so, ao = (13, 7, 5) if last else (0, 0, 0)
                                    dev["dst"].copy_(clean["dst"])
                                    check(hip.eben_stream_splice_rows(
                                        view["dst"].data_ptr(), pitch["dst"], view["prev"].data_ptr() if n_carry else None, pitch["prev"], po, n_carry,
                                        view["src"].data_ptr(), pitch["src"], so, n_new, view["add"].data_ptr() if with_add else None, pitch["add"], ao,
                                        view["idle"].data_ptr() if with_idle else None, pitch["idle"], rc, channels, words, sc, dc, stream()),
                                        "stream_splice_rows")
                                    want = clean["dst"].clone()
                                    w = inner(want, rc, pitch["dst"]).view(slots, channels, pitch["dst"])
                                    rows_in = torch.arange(n_act, device=DEV) if sc else act
                                    new = view["src"][rows_in][:, :, so : so + n_new]
                                    if with_add:
                                        new = new + view["add"][rows_in][:, :, ao : ao + n_new]
                                    vals = torch.cat((view["prev"][act][:, :, po : po + n_carry], new), dim=2)
                                    if dc:
                                        w[:n_act, :, :total] = vals
                                    else:
                                        w[act, :, :total] = vals
                                        if with_idle:
                                            w[idle_rows, :, :total] = view["idle"][idle_rows][:, :, :total]
                                    # inactive slots without idle, the rest of each pitch and the fences keep what they held
                                    assert same_bits(dev["dst"], want), (n_carry, n_new, which, sc, dc, with_idle, with_add, last)
                                    if which == "all" and not sc and not dc:
                                        plain.copy_(clean["dst"])
                                        p_view = inner(plain, rc, pitch["dst"])
                                        check(hip.eben_stream_splice(p_view.data_ptr(), pitch["dst"], view["prev"].data_ptr() if n_carry else None,
                                                                     pitch["prev"], po, n_carry, view["src"].data_ptr(), pitch["src"], so, n_new,
                                                                     view["add"].data_ptr() if with_add else None, pitch["add"], ao, rc, stream()),
                                                                     "stream_splice")
                                        assert same_bits(plain, dev["dst"])
            assert fences_intact(dev["dst"].cpu())
            for k in ("prev", "src", "add", "idle"):
                assert same_bits(dev[k], clean[k]), k        # the sources are only read


def test_splice_rows_refuses_bad_arguments_and_writes_nothing(hip):
    from vibravox_amd._lib import stream

    slots, ch = 3, 2
    rc = slots * ch
    f_dst, d_dst, v_dst = fenced(rc, 100, "splice_rows/bad/dst")
    ptrs = {k: fenced(rc, p, "splice_rows/bad/" + k) for k, p in (("prev", 50), ("src", 60), ("add", 70), ("idle", 100))}
    good = dict(dst=v_dst.data_ptr(), dp=100, prev=ptrs["prev"][2].data_ptr(), pp=50, po=10, nc=40, src=ptrs["src"][2].data_ptr(), sp=60, so=0, nn=60,
                add=ptrs["add"][2].data_ptr(), ap=70, ao=10, idle=ptrs["idle"][2].data_ptr(), ip=100, rc=rc, ch=ch, mask=(0b101,), sc=0, dc=0)

    def call(**kw):
        a = dict(good, **kw)
        words = None if a["mask"] is None else (ctypes.c_uint64 * 4)(*a["mask"])
        return hip.eben_stream_splice_rows(a["dst"], a["dp"], a["prev"], a["pp"], a["po"], a["nc"], a["src"], a["sp"], a["so"], a["nn"], a["add"], a["ap"],
                                           a["ao"], a["idle"], a["ip"], a["rc"], a["ch"], words, a["sc"], a["dc"], stream())

    d = good["dst"]
    bad = [dict(dst=None), dict(prev=None), dict(src=None), dict(mask=None), dict(dst=d + 2), dict(src=good["src"] + 1), dict(idle=good["idle"] + 2),
           dict(add=good["add"] + 3), dict(po=11), dict(so=1), dict(ao=11), dict(dp=99), dict(ip=99), dict(po=-1), dict(so=-1), dict(ao=-1),
           dict(nc=-1), dict(nn=-1), dict(nc=0, nn=0), dict(rc=0), dict(ch=4), dict(ch=0), dict(rc=257 * ch), dict(mask=(0b1000,)),
           dict(mask=(1 << 63,)),
           dict(prev=d), dict(src=d + 4 * 40), dict(add=d + 4 * (rc * 100 - 1)), dict(idle=d - 4 * (rc * 100 - 1)), dict(prev=d - 4 * (rc * 50 - 1)),
           dict(src=d - 4 * (2 * ch * 60 - 1), sc=1), dict(idle=d + 4 * (2 * ch * 100 - 1), dc=1)]   # compact extents: two active slots
    for kw in bad:
        assert call(**kw) == -1, kw
        assert hip.eben_last_error()
    torch.cuda.synchronize()
    assert same_bits(d_dst.cpu(), f_dst)          # nothing was written
    assert call(mask=(0,), idle=None) == 0        # no bit set, nothing to write: fine, and no launch
    torch.cuda.synchronize()
    assert same_bits(d_dst.cpu(), f_dst)
    assert call() == 0                            # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not same_bits(d_dst.cpu(), f_dst) and fences_intact(d_dst.cpu())


# ---- the segment copy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 45, 64])
def test_copy_segments_equals_torch_indexing(hip, count):
    from vibravox_amd._lib import EbenCopySegment, check, stream

    lengths = [4097, 1, 2, 3, 255, 256, 257, 1024][: count] + [1 + (977 * i) % 4097 for i in range(max(0, count - 8))]
    assert len(lengths) == count and 1 <= min(lengths) and max(lengths) == 4097
    gaps = [4 * (i % 3) + 1 for i in range(count)]           # segments start 4 bytes off the 16-byte grid, sentinel floats between them
    span = sum(lengths) + sum(gaps) + 4 * count
    f_src, d_src, v_src = fenced(1, span, f"segments/{count}/src")
    f_dst, d_dst, v_dst = fenced(1, span, f"segments/{count}/dst")
    want = f_dst.clone()
    table, pos_s, pos_d = [], 0, 3
    for n, gap in zip(lengths, gaps):
        pos_s, pos_d = (pos_s + 3) // 4 * 4, (pos_d + 3) // 4 * 4   # inner index 0 sits 4 bytes past a 16-byte boundary: keep every start there
        table.append(EbenCopySegment(v_dst.data_ptr() + 4 * pos_d, v_src.data_ptr() + 4 * pos_s, n))
        assert table[-1].dst % 16 == 4 and table[-1].src % 16 == 4
        want[FENCE + 1 + pos_d : FENCE + 1 + pos_d + n] = f_src[FENCE + 1 + pos_s : FENCE + 1 + pos_s + n]
        pos_s, pos_d = pos_s + n + gap, pos_d + n + gap
    assert max(pos_s, pos_d) <= span
    check(hip.eben_copy_segments((EbenCopySegment * count)(*table), count, stream()), "copy_segments")
    got = d_dst.cpu()
    assert same_bits(got, want) and fences_intact(got) and same_bits(d_src.cpu(), f_src)


def test_copy_segments_refuses_bad_arguments_and_writes_nothing(hip):
    from vibravox_amd._lib import EbenCopySegment, stream

    f_dst, d_dst, v_dst = fenced(1, 4096, "segments/bad/dst")
    _, _, v_src = fenced(1, 4096, "segments/bad/src")
    a, b = v_dst.data_ptr(), v_src.data_ptr()

    def call(segs, count=None):
        table = (EbenCopySegment * max(1, len(segs)))(*[EbenCopySegment(d, s, n) for d, s, n in segs])
        return hip.eben_copy_segments(table, len(segs) if count is None else count, stream())

    good = [(a, b, 100), (a + 4 * 200, b + 4 * 200, 50)]
    bad = [[(None, b, 4)], [(a, None, 4)], [(a + 2, b, 4)], [(a, b + 1, 4)], [(a, b, -1)], [(a + 64 * i, b + 64 * i, 4) for i in range(65)],
           [(a, a + 4 * 99, 100)], good + [(a + 4 * 1000, a + 4 * 249, 10)], good + [(a + 4 * 99, b + 4 * 1000, 10)]]
    for segs in bad:
        assert call(segs) == -1, segs
        assert hip.eben_last_error()
    assert call(good, count=-1) == -1
    torch.cuda.synchronize()
    assert same_bits(d_dst.cpu(), f_dst)
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not same_bits(d_dst.cpu(), f_dst) and fences_intact(d_dst.cpu())


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, chunk, names="ABCDE", tag="pool"):
    """The generator on the device, the scenario's clips, and per session: the float64 oracle of its own cut whole clip, the same build's
    whole-clip forward and a ``StreamingEnhancer(streams=1)`` over the same audio (all computed once)."""
    from vibravox_amd.streaming import StreamingEnhancer

    gen, sd = R.formula_generator(2, n)
    spec = tuple(s for s in P.scenario(P.SCENARIO_1024 if chunk == 1024 else P.SCENARIO_256) if s[0] in names)
    clips = {name: formula_audio(f"{tag}/{name}", 1, total) for name, total, _, _ in spec}
    refs = {name: O.generator_forward(sd, O.cut_to_valid_length(clip.double(), n=n), 2) for name, clip in clips.items()}
    gen = gen.to(DEV)
    whole, alone = {}, {}
    with torch.no_grad():
        for name, clip in clips.items():
            whole[name] = gen(gen.cut_to_valid_length(clip.to(DEV)))
            alone[name] = stream_through(StreamingEnhancer(gen, chunk, return_bands=True), clip)[:2]
    return gen, spec, clips, refs, whole, alone


def run(pool, spec, clips):
    with torch.no_grad():
        outs, slots = P.run_scenario(pool, {k: v.to(DEV) for k, v in clips.items()}, pool.chunk_samples, spec)
    joined = {name: (torch.cat([o[0] for o in res], dim=2), torch.cat([o[1] for o in res], dim=2)) for name, res in outs.items()}
    return joined, {name: [o[0].shape[2] for o in res] for name, res in outs.items()}, slots


def check_sessions(pool, spec, got, sizes, refs, whole, alone, tag):
    chunk = pool.chunk_samples
    for name, total, _, _ in spec:
        (enhanced, bands), (o_enh, o_bands) = got[name], refs[name]
        assert enhanced.shape == o_enh.shape == whole[name][0].shape and bands.shape == o_bands.shape, name
        (e_max, e_mse), (b_max, b_mse) = dist(enhanced, o_enh), dist(bands, o_bands)
        (e1_max, e1_mse), (b1_max, b1_mse) = dist(whole[name][0], o_enh), dist(whole[name][1], o_bands)
        apart = max(float((enhanced - alone[name][0]).abs().max()), float((bands - alone[name][1]).abs().max()))
        print(f"{tag} session {name}: pool enhanced max {e_max:.2e} mse {e_mse:.2e} bands max {b_max:.2e} | whole clip enhanced max {e1_max:.2e} mse "
              f"{e1_mse:.2e} bands max {b1_max:.2e} | max |pool - StreamingEnhancer(streams=1)| {apart:.2e}")
        assert e_max < 2e-5 and b_max < 2e-5 and e_mse < 1e-10 and b_mse < 1e-10, (name, e_max, b_max, e_mse, b_mse)
        assert e_max <= 2 * e1_max and b_max <= 2 * b1_max, (name, e_max, e1_max, b_max, b1_max)
        assert e_mse ** 0.5 <= 2 * e1_mse ** 0.5 and b_mse ** 0.5 <= 2 * b1_mse ** 0.5, (name, e_mse, e1_mse, b_mse, b1_mse)
        # 0 through warm-up, a chunk from then on; pushed - returned is the latency while the session runs
        steps = sizes[name][:-1]
        first = next((i for i, k in enumerate(steps) if k), len(steps))
        assert all(k == 0 for k in steps[:first]) and all(k == chunk for k in steps[first:]), (name, steps)
        if first < len(steps):
            assert first == pool.plan.warmup_pushes
            assert all((i + 1) * chunk - sum(steps[: i + 1]) == pool.latency for i in range(first, len(steps))), name
        assert sum(sizes[name]) == o_enh.shape[2]


@pytest.mark.parametrize("chunk", [256, 1024])
def test_pool_sessions_equal_their_own_whole_clips(hip, chunk):
    from vibravox_amd.streaming import StreamPool

    gen, spec, clips, refs, whole, alone = case(32, chunk)
    pool = StreamPool(gen, chunk, slots=4, return_bands=True)
    got, sizes, slots = run(pool, spec, clips)
    assert slots["E"] == slots["A"]
    check_sessions(pool, spec, got, sizes, refs, whole, alone, f"chunk={chunk}")
    assert all(k == 0 for k in sizes["D"][:-1])   # D never left its warm-up


def poisoned_pool(gen, chunk):
    from vibravox_amd.streaming import StreamPool

    pool = StreamPool(gen, chunk, slots=4, return_bands=True).prepare(DEV, private=4)
    for state in [pool.state] + list(pool.private.values()):
        for pair in state.buffers.values():
            for t in pair:
                t.fill_(float("nan"))
    return pool


def test_no_state_is_read_before_it_is_written_and_no_slot_leaks(hip):
    from vibravox_amd.streaming import StreamPool

    gen, spec, clips, _, _, _ = case(32, 256)
    clean, clean_sizes, _ = run(StreamPool(gen, 256, slots=4, return_bands=True), spec, clips)
    pool = poisoned_pool(gen, 256)
    got, sizes, _ = run(pool, spec, clips)
    assert len(pool.private) == 4 and sizes == clean_sizes
    for name in clean:
        assert torch.equal(got[name][0], clean[name][0]) and torch.equal(got[name][1], clean[name][1]), name
        assert not torch.isnan(got[name][0]).any() and not torch.isnan(got[name][1]).any(), name
    for name in clean:   # the others' audio is NaN: their slots, rows of every layer's launch, must not reach this session
        others = {k: (v if k == name else torch.full_like(v, float("nan"))) for k, v in clips.items()}
        got, _, _ = run(poisoned_pool(gen, 256), spec, others)
        assert torch.equal(got[name][0], clean[name][0]) and torch.equal(got[name][1], clean[name][1]), name


def test_a_second_scenario_reuses_the_pool_without_allocating(hip):
    from vibravox_amd.streaming import StreamPool

    gen, spec, clips, _, _, _ = case(32, 256)
    second = {name: formula_audio(f"pool/second/{name}", 1, clip.shape[2]) for name, clip in clips.items()}
    pool = StreamPool(gen, 256, slots=4, return_bands=True)
    run(pool, spec, clips)
    addresses = lambda: [t.data_ptr() for state in [pool.state] + [pool.private[i] for i in sorted(pool.private)] for pair in state.buffers.values() for t in pair]
    before, state = addresses(), pool.state
    assert pool.book.free_slots == [0, 1, 2, 3]
    again, sizes, _ = run(pool, spec, second)
    assert pool.state is state and addresses() == before                      # no reallocation
    fresh, fresh_sizes, _ = run(StreamPool(gen, 256, slots=4, return_bands=True), spec, second)
    assert sizes == fresh_sizes
    for name in fresh:
        assert torch.equal(again[name][0], fresh[name][0]) and torch.equal(again[name][1], fresh[name][1]), name


def test_pool_with_a_512_tap_bank_and_a_late_joiner(hip):
    from vibravox_amd.streaming import StreamPool

    gen, spec, clips, refs, whole, alone = case(512, 256, names="AB")
    pool = StreamPool(gen, 256, slots=4, return_bands=True)
    assert pool.plan.tensor("pqmf.analysis").carry > 256
    got, sizes, _ = run(pool, spec, clips)
    check_sessions(pool, spec, got, sizes, refs, whole, alone, "n=512 chunk=256")


def test_pool_returns_enhanced_alone_by_default(hip):
    from vibravox_amd.streaming import StreamPool

    gen, spec, clips, refs, _, _ = case(32, 1024)
    pool = StreamPool(gen, 1024, slots=2)
    x = clips["A"].to(DEV)
    with torch.no_grad():
        s = pool.open()
        outs = [pool.step({s: x[:, :, i * 1024 : (i + 1) * 1024]})[s] for i in range(x.shape[2] // 1024)]
        outs.append(pool.close(s, x[:, :, x.shape[2] // 1024 * 1024 :]))
        assert all(isinstance(o, torch.Tensor) and o.shape[:2] == (1, 1) for o in outs)
        assert dist(torch.cat(outs, dim=2), refs["A"][0])[0] < 2e-5
        with pytest.raises(RuntimeError, match="closed"):
            pool.step({s: x[:, :, :1024]})
