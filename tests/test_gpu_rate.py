"""GPU: the resampling kernels of ``csrc/rate.hip`` through ``rate.resample_ragged``, ``rate.StreamResampler``, ``rate.ChunkFront`` and
the raw stream entry point.

Two references.  ``augment.resample`` -- ``eben_resample``, the whole-signal kernel the new ones restate -- on each row or stream alone:
the results must be EQUAL (``torch.equal``).  And the float64 direct sum (``tests/rate_oracle.py``): the error of ``taps`` fused
accumulations is at most ``taps u / (1 - taps u) * sum_j |k_j x_j|`` with ``u = 2^-24``, per sample; no other tolerance is used."""
import functools

import numpy as np
import pytest
import torch

from tests import rate_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RATIOS = [(48000, 16000), (48000, 32000), (8000, 16000), (44100, 16000)]   # 3:1, 3:2, 1:2, 441:160
FENCE = 64
SENTINEL = 12345.0
U = 2.0 ** -24


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def ragged_case(freqs):
    """One batch for a ratio: rows of the lengths where the kernel can go wrong, NaN behind every row, and per row the parent's
    ``augment.resample`` of it alone and the float64 sum with its bound (all computed once)."""
    from vibravox_amd import augment, rate

    orig, new, width = rate.ratio(*freqs)
    tile = rate.tile(orig, new, width)
    span = tile["q_per_block"] * orig          # input samples whose outputs fill one block's tile exactly
    l_in = 2 * span + 37                       # three blocks a row, the last one partial
    k = 5
    lengths = [1, width, width + 1, orig * k, orig * k + 1, span - 1, span, span + 1, 2 * span + 5, l_in, 2]
    x = randn((len(lengths), l_in), sum(freqs))
    table = augment.sinc_resample_kernel(*freqs)[0]
    refs, sums, bounds = [], [], []
    xd = x.to(DEV)
    for r, n in enumerate(lengths):
        refs.append(augment.resample(xd[r : r + 1, :n].contiguous(), *freqs)[0])
        want, mag = RO.direct(x[r : r + 1, :n].double().numpy(), table.numpy(), orig, new, width)
        sums.append(want[0])
        bounds.append(mag[0])
    poisoned = x.clone()
    for r, n in enumerate(lengths):
        poisoned[r, n:] = float("nan")
    return dict(orig=orig, new=new, width=width, taps=2 * width + orig, tile=tile, lengths=lengths, x=x, poisoned=poisoned.to(DEV), refs=refs,
                sums=sums, bounds=bounds)


def fenced_out(rows, pitch):
    """A (rows, pitch) NaN-filled view inside a fenced allocation, 4 bytes off the 16-byte grid."""
    flat = torch.full((FENCE + 1 + rows * pitch + FENCE,), SENTINEL, dtype=torch.float32, device=DEV)
    view = flat[FENCE + 1 : FENCE + 1 + rows * pitch].view(rows, pitch)
    view.fill_(float("nan"))
    return flat, view


def fences_intact(flat):
    f = flat.cpu()
    return bool((f[: FENCE + 1] == SENTINEL).all()) and bool((f[-FENCE:] == SENTINEL).all())


@pytest.mark.parametrize("freqs", RATIOS)
def test_ragged_rows_equal_the_whole_signal_call_on_each_row_alone(hip, freqs):
    from vibravox_amd import rate

    c = ragged_case(freqs)
    orig, new, lengths = c["orig"], c["new"], c["lengths"]
    rows, l_in = c["poisoned"].shape
    need = rate.resampled_length(l_in, orig, new)
    for slack in (0, 13):   # the narrowest buffer the entry accepts, and one with room behind the longest row
        flat, out = fenced_out(rows, need + slack)
        got, out_lens = rate.resample_ragged(c["poisoned"], lengths, *freqs, out=out)
        assert got is out and out_lens.dtype is torch.int32
        want_lens = [rate.resampled_length(n, orig, new) for n in lengths]
        assert out_lens.cpu().tolist() == want_lens
        assert fences_intact(flat)
        gamma = c["taps"] * U / (1 - c["taps"] * U)
        for r, n_out in enumerate(want_lens):
            row = out[r]
            assert torch.equal(row[:n_out], c["refs"][r]), (freqs, lengths[r])
            assert bool((row[n_out:] == 0).all()) and row[n_out:].numel() == need + slack - n_out, (freqs, lengths[r])
            err = np.abs(row[:n_out].double().cpu().numpy() - c["sums"][r])
            worst = float((err / np.maximum(gamma * c["bounds"][r], 1e-300)).max())
            print(f"{freqs} row of {lengths[r]}: max error / bound = {worst:.3f}")
            assert (err <= gamma * c["bounds"][r]).all(), (freqs, lengths[r], worst)
    plain, plain_lens = rate.resample_ragged(c["poisoned"].reshape(rows, 1, l_in), lengths, *freqs)   # (rows, 1, T) in, the default buffer out
    assert plain.shape == (rows, 1, need) and torch.equal(plain[:, 0], out[:, :need]) and torch.equal(plain_lens, out_lens)


@pytest.mark.parametrize("freqs", [(48000, 16000), (44100, 16000)])
def test_a_corrupt_length_table_yields_clamped_rows_and_leaves_the_neighbours_alone(hip, freqs):
    from vibravox_amd import augment, rate

    c = ragged_case(freqs)
    orig, new = c["orig"], c["new"]
    x = c["x"].to(DEV)   # no NaN: a clamped row reads its whole buffer
    rows, l_in = x.shape
    lengths = list(c["lengths"])
    bad_low, bad_high = 3, 6
    table = list(lengths)
    table[bad_low], table[bad_high] = -5, l_in + 100
    need = rate.resampled_length(l_in, orig, new)
    flat, out = fenced_out(rows, need + 5)
    _, out_lens = rate.resample_ragged(x, torch.tensor(table, dtype=torch.int32, device=DEV), *freqs, out=out)
    assert fences_intact(flat)
    want_lens = [rate.resampled_length(min(max(n, 0), l_in), orig, new) for n in table]
    assert out_lens.cpu().tolist() == want_lens and want_lens[bad_low] == 0 and want_lens[bad_high] == need
    assert bool((out[bad_low] == 0).all())
    assert torch.equal(out[bad_high, :need], augment.resample(x[bad_high : bad_high + 1], *freqs)[0]) and bool((out[bad_high, need:] == 0).all())
    for r in range(rows):
        if r not in (bad_low, bad_high):
            assert torch.equal(out[r, : want_lens[r]], c["refs"][r]) and bool((out[r, want_lens[r]:] == 0).all()), r
    with pytest.raises(ValueError, match="is said to hold"):   # host lengths are checked on the host
        rate.resample_ragged(x, table, *freqs)


# ---- the stream route --------------------------------------------------------------------------------------------------------------
def stream_through(resampler, signal, chunk):
    """``signal`` (rows, T) on the device in pushes of ``chunk`` and a finish with what is left (None when nothing is)."""
    total, pos, outs = signal.shape[1], 0, []
    while total - pos >= chunk:
        outs.append(resampler.push(signal[:, pos : pos + chunk].contiguous()))
        pos += chunk
    outs.append(resampler.finish(signal[:, pos:].contiguous() if pos < total else None))
    return outs


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("freqs,chunk", [((48000, 16000), 768), ((48000, 32000), 384), ((48000, 16000), 7001), ((48000, 32000), 3100)])
def test_stream_resampler_equals_the_whole_signal_call(hip, freqs, chunk, rows):
    from vibravox_amd import augment, rate

    orig, new, width = rate.ratio(*freqs)
    k = 3
    resampler = rate.StreamResampler(*freqs, rows=rows).prepare(DEV, chunk)
    state = resampler.state
    for t in state:
        t.fill_(float("nan"))
    second = None
    for total in (k * chunk, k * chunk + 1, (k + 1) * chunk - 1):
        x = randn((rows, total), total + rows).to(DEV)
        assert rows == 1 or not torch.equal(x[0], x[1])
        want = augment.resample(x, *freqs)
        outs = stream_through(resampler, x, chunk)
        got = torch.cat(outs, dim=1)
        assert got.shape == want.shape and torch.equal(got, want), (freqs, chunk, total)
        finals = [rate.final_outputs(n * chunk, orig, new, width) for n in range(total // chunk + 1)]
        assert [o.shape[1] for o in outs[:-1]] == [b - a for a, b in zip(finals, finals[1:])]
        assert outs[-1].shape[1] == rate.resampled_length(total, orig, new) - finals[-1]
        with pytest.raises(RuntimeError, match="finished"):
            resampler.push(x[:, :chunk].contiguous())
        resampler.reset()   # the next signal starts on the same state
        second = (x, want)
    assert resampler.state is state
    x, want = second
    resampler.push(x[:, :chunk].contiguous())
    resampler.reset()       # mid-stream as well
    assert torch.equal(torch.cat(stream_through(resampler, x, chunk), dim=1), want)
    three = x.reshape(rows, 1, -1)   # (rows, 1, T) chunks give (rows, 1, k) results
    resampler.reset()
    first = resampler.push(three[:, :, :chunk].contiguous())
    assert first.shape == (rows, 1, rate.final_outputs(chunk, orig, new, width)) and torch.equal(first[:, 0], want[:, : first.shape[2]])
    with pytest.raises(ValueError, match="allocated for"):
        resampler.push(torch.zeros(rows, chunk + 1, device=DEV))


@pytest.mark.parametrize("freqs,chunk_samples", [((48000, 32000), 256), ((44100, 16000), 1280)])
def test_chunk_front_hands_over_whole_chunks(hip, freqs, chunk_samples):
    from vibravox_amd import augment, rate

    rows = 2
    front = rate.ChunkFront(*freqs, chunk_samples, rows, 256)
    front.prepare(DEV)
    for t in front.fifo + front.resampler.state:
        t.fill_(float("nan"))
    ic = front.input_chunk_samples
    x = randn((rows, 1, 3 * ic + 2 * ic // 3), ic).to(DEV)
    want = augment.resample(x, *freqs)
    got, counts, pos = [], [], 0
    while x.shape[2] - pos >= ic:
        before = len(got)
        assert front.feed(x[:, :, pos : pos + ic].contiguous(), False, lambda c: got.append(c.clone())) is None
        counts.append(len(got) - before)
        pos += ic
    rest = front.feed(x[:, :, pos:].contiguous(), True, lambda c: got.append(c.clone()))
    assert counts == [0, 1, 1] and all(c.shape == (rows, 1, chunk_samples) for c in got)
    assert rest is not None and 0 < rest.shape[2] < chunk_samples
    assert torch.equal(torch.cat(got + [rest], dim=2), want)


@pytest.mark.parametrize("freqs", [(48000, 32000), (44100, 16000)])
def test_stream_entry_starts_at_any_phase(hip, freqs):
    """The raw entry on a tape that is the whole signal: launches that start at outputs of odd phase, with the first output's phase and
    tap index as ``RatePush.piece`` gives them, written at an offset of a wider row."""
    from vibravox_amd import augment, rate
    from vibravox_amd._lib import check, stream

    orig, new, width = rate.ratio(*freqs)
    rows, total = 2, 4 * 441 + 3
    x = randn((rows, total), total).to(DEV)
    want = augment.resample(x, *freqs)
    n_all = want.shape[1]
    table = augment.sinc_resample_kernel(*freqs)[0].to(DEV)
    whole = rate.RatePush(0, 0, total, 0, -width, n_all, True)
    for skip, count in ((1, n_all - 1), (7, 300), (new + 1, n_all - new - 1), (n_all - 1, 1)):
        p0, base0 = whole.piece(skip, orig, new)
        assert p0 == skip % new and p0 != 0
        flat, out = fenced_out(rows, count + 9)
        check(hip.eben_resample_stream(x.data_ptr(), table.data_ptr(), out.data_ptr(), rows, total, total, count + 9, 5, count, p0, base0, 1, orig, new,
                                       width, stream()), "resample_stream")
        assert fences_intact(flat)
        assert torch.equal(out[:, 5 : 5 + count], want[:, skip : skip + count]), (freqs, skip)
        assert bool(torch.isnan(out[:, :5]).all()) and bool(torch.isnan(out[:, 5 + count:]).all())   # nothing else was written
