"""GPU: streaming generator inference -- the splice kernel through its raw entry point against torch indexing, and
``streaming.StreamingEnhancer`` / ``inference.enhance_stream`` against the float64 oracle of the WHOLE clip and against the same build's
whole-clip forward.

Bars, those of test_gpu_ragged.py: max|.| < 2e-5 on enhanced and bands and MSE < 1e-10 against the oracle; and a streamed clip may be no
further from the oracle than twice the whole-clip forward is, in max and in RMS (where a sample sits among the kernels' tiles can move
a rounding, nothing more)."""
import functools

import pytest
import torch

from formula import formula_audio, formula_tensor
from oracle import eben_oracle as O
from tests import ragged_oracle as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FENCE = 64
SENTINEL = 12345.0
TOTAL = 8000    # cut 7904 with the 32-tap banks, 7936 with the 512-tap ones


# ---- the splice kernel ------------------------------------------------------------------------------------------------------------
def fenced(rows_channels, pitch, tag):
    """A (rows x channels, pitch) view 4 bytes off the 16-byte grid inside a fenced allocation, formula values inside."""
    n = rows_channels * pitch
    flat = torch.full((FENCE + 1 + n + FENCE,), SENTINEL, dtype=torch.float32)
    flat[FENCE + 1 : FENCE + 1 + n] = formula_tensor(tag, (n,))
    dev = flat.to(DEV)
    view = dev[FENCE + 1 : FENCE + 1 + n].view(rows_channels, pitch)
    assert view.data_ptr() % 16 == 4
    return flat, dev, view


def body(flat, rows_channels, pitch):
    return flat[FENCE + 1 : FENCE + 1 + rows_channels * pitch].view(rows_channels, pitch)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fences_intact(got):
    return float(got[:FENCE].min()) == SENTINEL == float(got[:FENCE].max()) == float(got[-FENCE:].min()) == float(got[-FENCE:].max()) == float(got[FENCE])


@pytest.mark.parametrize("channels", [5, 32])
def test_splice_equals_torch_indexing(hip, channels):
    from vibravox_amd._lib import check, stream

    rc = 2 * channels
    for n_carry in (0, 1, 9, 700):
        for n_new in (1, 64, 257):
            # a different pitch for each of the four tensors; dst once exactly as long as what is written
            pitches = dict(dst=n_carry + n_new + (0 if n_new == 64 else 3), prev=n_carry + 13, src=n_new + 7, add=n_new + 5)
            for with_add in (False, True):
                for last in (False, True):   # offsets 0, then the last ones that fit
                    po, so, ao = (13, 7, 5) if last else (0, 0, 0)
                    tag = f"splice/{channels}/{n_carry}/{n_new}"
                    f_dst, d_dst, v_dst = fenced(rc, pitches["dst"], tag + "/dst")
                    f_prev, d_prev, v_prev = fenced(rc, pitches["prev"], tag + "/prev")
                    f_src, d_src, v_src = fenced(rc, pitches["src"], tag + "/src")
                    f_add, d_add, v_add = fenced(rc, pitches["add"], tag + "/add")
                    check(hip.eben_stream_splice(v_dst.data_ptr(), pitches["dst"], v_prev.data_ptr() if n_carry else None, pitches["prev"], po, n_carry,
                                                 v_src.data_ptr(), pitches["src"], so, n_new, v_add.data_ptr() if with_add else None, pitches["add"], ao,
                                                 rc, stream()), "stream_splice")
                    want = f_dst.clone()
                    w = body(want, rc, pitches["dst"])
                    w[:, :n_carry] = body(f_prev, rc, pitches["prev"])[:, po : po + n_carry]
                    new = body(f_src, rc, pitches["src"])[:, so : so + n_new]
                    if with_add:
                        new = new + body(f_add, rc, pitches["add"])[:, ao : ao + n_new]
                    w[:, n_carry : n_carry + n_new] = new
                    got = d_dst.cpu()
                    assert same_bits(got, want), (n_carry, n_new, with_add, last)     # the rest of dst's pitch and the fences included
                    assert fences_intact(got)
                    for flat, dev in ((f_prev, d_prev), (f_src, d_src), (f_add, d_add)):
                        assert same_bits(dev.cpu(), flat)                             # the sources are only read


def test_splice_refuses_bad_arguments_and_writes_nothing(hip):
    from vibravox_amd._lib import stream

    rc = 6
    f_dst, d_dst, v_dst = fenced(rc, 100, "splice/bad/dst")
    _, _, v_prev = fenced(rc, 50, "splice/bad/prev")
    _, _, v_src = fenced(rc, 60, "splice/bad/src")
    _, _, v_add = fenced(rc, 70, "splice/bad/add")
    good = dict(dst=v_dst.data_ptr(), dp=100, prev=v_prev.data_ptr(), pp=50, po=10, nc=40, src=v_src.data_ptr(), sp=60, so=0, nn=60,
                add=v_add.data_ptr(), ap=70, ao=10, rc=rc)

    def call(**kw):
        a = dict(good, **kw)
        return hip.eben_stream_splice(a["dst"], a["dp"], a["prev"], a["pp"], a["po"], a["nc"], a["src"], a["sp"], a["so"], a["nn"], a["add"], a["ap"],
                                      a["ao"], a["rc"], stream())

    bad = [dict(dst=None), dict(prev=None), dict(src=None), dict(dst=good["dst"] + 2), dict(src=good["src"] + 1), dict(po=11), dict(so=1),
           dict(ao=11), dict(dp=99), dict(po=-1), dict(so=-1), dict(ao=-1), dict(nc=-1), dict(nn=-1), dict(nc=0, nn=0), dict(rc=0),
           dict(prev=good["dst"]), dict(src=good["dst"] + 4 * 40), dict(add=good["dst"] + 4 * (rc * 100 - 1)),     # dst aliases a source
           dict(prev=good["dst"] - 4 * (rc * 50 - 1))]                                                             # ... by its last float
    for kw in bad:
        assert call(**kw) == -1, kw
        assert hip.eben_last_error()
    torch.cuda.synchronize()
    assert same_bits(d_dst.cpu(), f_dst)          # nothing was written
    assert call() == 0                            # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not same_bits(d_dst.cpu(), f_dst) and fences_intact(d_dst.cpu())


# ---- the enhancer -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(p, n=32, rows=1):
    """The generator on the device, a clip of ``rows`` different rows, per row the float64 oracle of the cut whole clip and the same
    build's whole-clip forward with its distance from that oracle (all computed once)."""
    gen, sd = R.formula_generator(p, n)
    clip = formula_audio(f"stream/{n}/{rows}", rows, TOTAL)
    refs = [O.generator_forward(sd, O.cut_to_valid_length(clip[r : r + 1].double(), n=n), p) for r in range(rows)]
    gen = gen.to(DEV)
    with torch.no_grad():
        whole = gen(gen.cut_to_valid_length(clip.to(DEV)))
    return gen, clip, refs, whole


def dist(got, ref):
    d = got.detach().double().cpu() - ref
    return float(d.abs().max()), float((d ** 2).mean())


def stream_through(enhancer, clip):
    """The clip in pushes of the enhancer's chunk and a final shorter one: (enhanced, bands) concatenated, the sizes of the returns."""
    chunk, total = enhancer.chunk_samples, clip.shape[2]
    x = clip.to(DEV)
    outs, pos = [], 0
    with torch.no_grad():
        while total - pos >= chunk:
            outs.append(enhancer.push(x[:, :, pos : pos + chunk]))
            pos += chunk
        outs.append(enhancer.finish(x[:, :, pos:]))
    return torch.cat([o[0] for o in outs], dim=2), torch.cat([o[1] for o in outs], dim=2), [o[0].shape[2] for o in outs]


def check_rows(refs, whole, enhanced, bands, tag):
    """Every row against the oracle of its own whole clip, and no further from it than twice the whole-clip device forward is."""
    worst = 0.0
    for r, (o_enh, o_bands) in enumerate(refs):
        assert enhanced.shape[2] == o_enh.shape[2] == whole[0].shape[2] and bands.shape[2] == o_bands.shape[2]
        (e_max, e_mse), (b_max, b_mse) = dist(enhanced[r : r + 1], o_enh), dist(bands[r : r + 1], o_bands)
        (e1_max, e1_mse), (b1_max, b1_mse) = dist(whole[0][r : r + 1], o_enh), dist(whole[1][r : r + 1], o_bands)
        apart = max(float((enhanced[r] - whole[0][r]).abs().max()), float((bands[r] - whole[1][r]).abs().max()))
        worst = max(worst, apart)
        print(f"{tag} row {r}: stream enhanced max {e_max:.2e} mse {e_mse:.2e} bands max {b_max:.2e} | whole clip enhanced max {e1_max:.2e} mse "
              f"{e1_mse:.2e} bands max {b1_max:.2e} | max |stream - whole-clip device forward| {apart:.2e}")
        assert e_max < 2e-5 and b_max < 2e-5 and e_mse < 1e-10 and b_mse < 1e-10, (r, e_max, b_max, e_mse, b_mse)
        assert e_max <= 2 * e1_max and b_max <= 2 * b1_max, (r, e_max, e1_max, b_max, b1_max)
        assert e_mse ** 0.5 <= 2 * e1_mse ** 0.5 and b_mse ** 0.5 <= 2 * b1_mse ** 0.5, (r, e_mse, e1_mse, b_mse, b1_mse)
    return worst


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("p", [2, 1])
def test_enhancer_equals_the_whole_clip(hip, p, chunk):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, refs, whole = case(p)
    enhancer = StreamingEnhancer(gen, chunk, return_bands=True)
    enhanced, bands, sizes = stream_through(enhancer, clip)
    assert enhanced.shape == (1, 1, 7904) and bands.shape == (1, 4, 1984)
    first = next(i for i, k in enumerate(sizes) if k)
    assert first == enhancer.plan.warmup_pushes and all(k == chunk for k in sizes[first:-1]) and all(k == 0 for k in sizes[:first])
    assert TOTAL // chunk * chunk - sum(sizes[:-1]) == enhancer.latency
    check_rows(refs, whole, enhanced, bands, f"p={p} chunk={chunk}")


def test_rows_advance_in_lockstep_each_with_its_own_content(hip):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, refs, whole = case(2, rows=3)
    assert not torch.equal(clip[0], clip[1]) and not torch.equal(clip[1], clip[2])
    enhanced, bands, _ = stream_through(StreamingEnhancer(gen, 1024, streams=3, return_bands=True), clip)
    assert enhanced.shape == (3, 1, 7904)
    check_rows(refs, whole, enhanced, bands, "streams=3")


def test_enhancer_with_a_512_tap_bank(hip):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, refs, whole = case(2, 512)
    enhancer = StreamingEnhancer(gen, 256, return_bands=True)
    assert enhancer.plan.tensor("pqmf.analysis").carry > 256 and enhancer.plan.hold == 0
    enhanced, bands, _ = stream_through(enhancer, clip)
    assert enhanced.shape == (1, 1, 7936) and bands.shape == (1, 4, 2112)
    check_rows(refs, whole, enhanced, bands, "n=512 chunk=256")


def test_reset_starts_a_new_stream_on_the_same_state(hip):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, _, _ = case(2)
    a, b = clip, formula_audio("stream/other", 1, 5000)
    enhancer = StreamingEnhancer(gen, 512, return_bands=True)
    stream_through(enhancer, a)
    state = enhancer.state
    addresses = [t.data_ptr() for pair in state.buffers.values() for t in pair]
    with torch.no_grad(), pytest.raises(RuntimeError, match="finished"):
        enhancer.push(a.to(DEV)[:, :, :512])
    enhancer.reset()
    again = stream_through(enhancer, b)
    assert enhancer.state is state and addresses == [t.data_ptr() for pair in state.buffers.values() for t in pair]   # no reallocation
    fresh = stream_through(StreamingEnhancer(gen, 512, return_bands=True), b)
    assert again[2] == fresh[2] and torch.equal(again[0], fresh[0]) and torch.equal(again[1], fresh[1])
    enhancer.reset()   # mid-stream as well
    with torch.no_grad():
        enhancer.push(a.to(DEV)[:, :, :512])
    enhancer.reset()
    third = stream_through(enhancer, b)
    assert torch.equal(third[0], fresh[0]) and torch.equal(third[1], fresh[1])


def test_no_state_is_read_before_it_is_written(hip):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, _, _ = case(2)
    clean = stream_through(StreamingEnhancer(gen, 256, return_bands=True), clip)
    poisoned = StreamingEnhancer(gen, 256, return_bands=True).prepare(DEV)
    for pair in poisoned.state.buffers.values():
        for t in pair:
            t.fill_(float("nan"))
    got = stream_through(poisoned, clip)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])
    assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()


def test_enhance_stream_equals_the_whole_clip(hip):
    from vibravox_amd.inference import enhance_stream

    gen, clip, refs, whole = case(2)
    x = clip.to(DEV)
    enhanced, bands = enhance_stream(gen, x, chunk_samples=1024)
    assert enhanced.shape == whole[0].shape == (1, 1, 7904) and bands.shape == whole[1].shape
    check_rows(refs, whole, enhanced, bands, "enhance_stream")
    in_one, bands_one = enhance_stream(gen, x)   # the default chunk is longer than the clip: everything comes out of finish()
    check_rows(refs, whole, in_one, bands_one, "enhance_stream, one chunk")
    with pytest.raises(ValueError, match="too short"):
        enhance_stream(gen, x[:, :, :991])


def test_enhancer_refuses_autograd_wrong_shapes_and_cpu_tensors(hip):
    from vibravox_amd._lib import EbenError
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, _, _ = case(2)
    enhancer = StreamingEnhancer(gen, 256, streams=2)
    good = torch.zeros(2, 1, 256, device=DEV)
    with pytest.raises(RuntimeError, match="no backward"):
        enhancer.push(good)
    with pytest.raises(RuntimeError, match="no backward"):
        enhancer.finish()
    with torch.no_grad():
        for bad in (good[:1], good[:, :, :255], torch.zeros(2, 1, 512, device=DEV), good[:, 0], good.double(), torch.zeros(2, 2, 256, device=DEV)):
            with pytest.raises(ValueError, match="expects"):
                enhancer.push(bad)
        with pytest.raises(ValueError, match="expects"):
            enhancer.finish(good)              # a whole chunk is a push
        with pytest.raises(EbenError, match="no CPU path"):
            enhancer.push(good.cpu())
        assert enhancer.push(good).shape == (2, 1, 0)   # nothing above has moved the stream
        with pytest.raises(ValueError, match="too short"):
            enhancer.finish(good[:, :, :100])  # 356 samples in all
