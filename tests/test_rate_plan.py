"""CPU: the position arithmetic of ``vibravox_amd/rate.py`` -- finality, carry, the push plan executed in float64 on poisoned tapes
(``tests/rate_oracle.py``), positions past 2^33 -- and the host-side argument checks of the ``csrc/rate.hip`` entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import rate_oracle as RO
from vibravox_amd import rate

RATIOS = [(48000, 16000), (48000, 32000), (8000, 16000), (44100, 16000)]   # 3:1, 3:2, 1:2, 441:160


def reads_up_to(n, orig, new, width):
    """The last input index output n reads (every tap counts, also one whose table entry is 0)."""
    return (n // new) * orig - width + (2 * width + orig) - 1


@pytest.mark.parametrize("freqs", RATIOS + [(32000, 16000)])
def test_final_outputs_and_carry_against_brute_force(freqs):
    orig, new, width = rate.ratio(*freqs)
    taps = 2 * width + orig
    assert (orig, new) == (freqs[0] // math.gcd(*freqs), freqs[1] // math.gcd(*freqs))
    for n_in in range(0, 6 * orig + 3 * taps):
        final = 0
        while reads_up_to(final, orig, new, width) <= n_in - 1:
            final += 1
        assert rate.final_outputs(n_in, orig, new, width) == final, n_in
        assert final <= rate.resampled_length(n_in, orig, new)
        first_read = max(0, (final // new) * orig - width)   # of the next output
        assert rate.carry_start(final, orig, new, width) == first_read
        s = rate.Schedule(*freqs)
        op = s.push(n_in)
        assert (op.n_out, op.n_carry, op.n_new, op.p0, op.base0, op.end) == (final, 0, n_in, 0, -width, False)
        nxt = s.push(orig)   # what the next push keeps: from the next output's first input on, never more than taps - 1 samples
        assert nxt.prev_off == first_read and nxt.n_carry == n_in - first_read <= taps - 1
        assert s.lookahead == width + orig - 1


def test_lengths_agree_with_the_public_helpers():
    from vibravox_amd import augment, inference

    for freqs in RATIOS:
        orig, new, width = rate.ratio(*freqs)
        table, w, o, n = augment.sinc_resample_kernel(*freqs)
        assert (w, o, n) == (width, orig, new) and tuple(table.shape) == (new, 2 * width + orig)
        for t in (0, 1, width, 1000, 12345):
            assert rate.resampled_length(t, orig, new) == inference.resampled_length(t, *freqs)


def signal(rows, total, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((rows, total))


def chunk_cases(freqs):
    """(chunk, totals): chunks of ``orig`` samples and of a StreamingEnhancer's ``input_chunk_samples``; totals of k chunks, one sample
    more and less, and one shorter than ``width``."""
    orig, new, width = rate.ratio(*freqs)
    taps = 2 * width + orig
    small = orig
    k_small = -(-2 * taps // small) + 3
    model_chunk = 256 * new // math.gcd(256, new)
    big = rate.input_chunk_samples(model_chunk, *freqs, 256)
    assert big * new == model_chunk * orig
    out = [(small, [k_small * small, k_small * small + 1, k_small * small - 1, max(width - 1, 1)]),
           (big, [2 * big, 2 * big + 1, 2 * big - 1, max(width - 1, 1)])]
    return out


@pytest.mark.parametrize("freqs", RATIOS)
def test_plan_in_float64_reproduces_the_whole_signal_exactly(freqs):
    from vibravox_amd import augment

    orig, new, width = rate.ratio(*freqs)
    table = augment.sinc_resample_kernel(*freqs)[0].numpy()
    for chunk, totals in chunk_cases(freqs):
        for total in totals:
            x = signal(2, total, total)
            want, _ = RO.direct(x, table, orig, new, width)
            outs, ops = RO.run_schedule(rate.Schedule(*freqs), table, x, [chunk] * (total // chunk), chunk)
            got = np.concatenate(outs, axis=1)
            assert not np.isnan(got).any(), (chunk, total)
            assert got.shape == want.shape and np.array_equal(got, want), (chunk, total)
            pushed, sizes = 0, []
            for o in outs[:-1]:
                sizes.append(rate.final_outputs(pushed + chunk, orig, new, width) - rate.final_outputs(pushed, orig, new, width))
                pushed += chunk
            assert [o.shape[1] for o in outs[:-1]] == sizes
            assert sum(o.shape[1] for o in outs) == rate.resampled_length(total, orig, new)
            assert all(op.n_carry <= 2 * width + orig - 1 for op in ops)
            if total % chunk == 0:   # finish() without a tail
                assert ops[-1].n_new == 0 and ops[-1].end


def test_uneven_chunks_and_a_spent_schedule():
    from vibravox_amd import augment

    freqs = (48000, 32000)
    orig, new, width = rate.ratio(*freqs)
    table = augment.sinc_resample_kernel(*freqs)[0].numpy()
    x = signal(1, 500, 7)
    s = rate.Schedule(*freqs)
    outs, _ = RO.run_schedule(s, table, x, [1, 2, 40, 0, 7, 133, 90])   # and a tail of 227 samples
    assert np.array_equal(np.concatenate(outs, axis=1), RO.direct(x, table, orig, new, width)[0])
    with pytest.raises(RuntimeError, match="finished"):
        s.push(3)
    s.reset()
    assert s.push(500, final=True).n_out == rate.resampled_length(500, orig, new)
    with pytest.raises(ValueError, match="nothing to resample"):
        rate.Schedule(16000, 16000)


@pytest.mark.parametrize("freqs", RATIOS)
def test_positions_past_2_to_the_33_issue_the_same_buffer_relative_operations(freqs):
    orig, new, width = rate.ratio(*freqs)
    chunk = rate.input_chunk_samples(256 * new // math.gcd(256, new), *freqs, 256)
    near = rate.Schedule(*freqs)
    with pytest.raises(RuntimeError, match="left edge"):
        near.advance(orig)
    near.push(chunk)
    near.push(chunk)
    steady = near.push(chunk)           # the first push whose tape AND whose predecessor's no longer start at position 0
    assert steady.prev_off > 0 and near.push(chunk) == steady
    far = rate.Schedule(*freqs)
    far.push(chunk)
    far.push(chunk)
    jump = ((1 << 33) // orig + 1) * orig
    far.advance(jump)
    assert far.pushed > 1 << 33 and far.start > 1 << 33 and far.emitted == near.emitted - 2 * steady.n_out + jump // orig * new
    op = far.push(chunk)
    assert op == steady
    for v in (op.prev_off, op.n_carry, op.n_new, op.p0, op.base0, op.n_out):
        assert -(1 << 20) < v < 1 << 20   # buffer-relative: small whatever the position
    last = far.push(5, final=True)
    assert far.emitted == rate.resampled_length(far.pushed, orig, new) and last.n_out < 1 << 20
    with pytest.raises(ValueError, match="whole number"):
        rate.Schedule(*freqs).advance(orig + 1) if orig > 1 else rate.Schedule(*freqs).advance(-1)


def test_a_chunk_that_is_no_whole_number_of_input_samples_is_refused():
    from tests import ragged_oracle as R
    from vibravox_amd.streaming import StreamingEnhancer

    assert rate.input_chunk_samples(256, 48000, 16000, 256) == 768
    assert rate.input_chunk_samples(1280, 44100, 16000, 256) == 3528
    with pytest.raises(ValueError, match="smallest chunk_samples that works is 1280"):
        rate.input_chunk_samples(256, 44100, 16000, 256)
    gen, _ = R.formula_generator(1)
    with pytest.raises(ValueError, match="smallest chunk_samples that works is 1280"):
        StreamingEnhancer(gen, 256, input_rate=44100)
    rated = StreamingEnhancer(gen, 256, input_rate=48000)
    plain = StreamingEnhancer(gen, 256)
    assert rated.input_chunk_samples == 768 and plain.input_chunk_samples == 256
    assert rated.input_latency == 768 + 3 * plain.latency and plain.input_latency == plain.latency
    same = StreamingEnhancer(gen, 256, input_rate=16000)
    assert same.input_chunk_samples == 256 and same.input_latency == plain.latency


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_tile_constants_without_gpu(lib):
    for freqs in RATIOS:
        orig, new, width = rate.ratio(*freqs)
        t = rate.tile(orig, new, width)
        taps = 2 * width + orig
        assert t["q_per_block"] >= 1 and t["outputs_per_block"] == t["q_per_block"] * new <= 1024
        assert t["window_floats"] == t["q_per_block"] * orig + taps - 1 <= 4096
        assert t["table_in_lds"] == (new * taps * 4 <= 8192)
    assert rate.tile(3, 1, 19)["table_in_lds"] and not rate.tile(441, 160, 17)["table_in_lds"]
    out = (ctypes.c_int * 4)()
    assert lib.eben_resample_plan(3, 1, 19, out, 3) < 0 and lib.eben_resample_plan(3, 1, 19, None, 4) < 0
    assert lib.eben_resample_plan(0, 1, 19, out, 4) < 0 and lib.eben_resample_plan(3, 1, -1, out, 4) < 0
    assert lib.eben_resample_plan(5000, 1, 6, out, 4) < 0 and b"fits no tile" in lib.eben_last_error()


def test_ragged_entry_refuses_bad_arguments_without_gpu(lib):
    """Every call below is refused on the host (EBEN_EINVAL and a message): the pointers are never dereferenced, no device is touched."""
    P = ctypes.c_void_p
    good = dict(x=P(0x1000), lens=P(0x2000), k=P(0x3000), out=P(0x4000), out_lens=P(0x5000), rows=3, l_in=300, l_out=100, orig=3, new=1, width=19)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eben_resample_ragged(a["x"], a["lens"], a["k"], a["out"], a["out_lens"], a["rows"], a["l_in"], a["l_out"], a["orig"], a["new"],
                                        a["width"], None)

    for name in ("x", "lens", "k", "out", "out_lens"):
        assert call(**{name: None}) == -1 and b"null" in lib.eben_last_error(), name
        assert call(**{name: P(0x1002)}) == -1 and b"misaligned" in lib.eben_last_error(), name
    for bad in (dict(rows=0), dict(rows=-1), dict(rows=65536), dict(l_in=0), dict(l_out=0), dict(l_out=99), dict(l_in=301), dict(orig=0), dict(new=0),
                dict(width=-1), dict(orig=5000), dict(new=1025), dict(l_in=0x7fff0001, l_out=0x7fff0000)):
        assert call(**bad) == -1, bad
    assert call(l_out=99) == -1 and b"l_out_buf" in lib.eben_last_error()


def test_stream_entry_refuses_bad_arguments_without_gpu(lib):
    P = ctypes.c_void_p
    # a tape of 40 carried + 768 new samples at 3:1, its 256 outputs starting at tap index 0: the last one reads up to 3 * 255 + 40 = 805
    good = dict(tape=P(0x1000), k=P(0x3000), out=P(0x4000), rows=2, pitch=900, len=808, out_pitch=256, first=0, n_out=256, p0=0, base0=0, end=0,
                orig=3, new=1, width=19)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eben_resample_stream(a["tape"], a["k"], a["out"], a["rows"], a["pitch"], a["len"], a["out_pitch"], a["first"], a["n_out"], a["p0"],
                                        a["base0"], a["end"], a["orig"], a["new"], a["width"], None)

    for name in ("tape", "k", "out"):
        assert call(**{name: None}) == -1 and b"null" in lib.eben_last_error(), name
        assert call(**{name: P(0x1001)}) == -1 and b"misaligned" in lib.eben_last_error(), name
    for bad in (dict(rows=0), dict(rows=65536), dict(pitch=0), dict(len=-1), dict(len=901), dict(out_pitch=0), dict(first=-1), dict(n_out=-1),
                dict(first=1), dict(n_out=257), dict(p0=-1), dict(p0=1), dict(orig=0), dict(new=0), dict(width=-1),
                dict(len=805),                         # the last output's last tap lies at index 805: one sample short
                dict(base0=3),                         # ... and so it does when everything starts one q later
                dict(end=1, len=765, base0=-19)):      # at the signal's end, from position 0: 765 samples have 255 outputs
        assert call(**bad) == -1, bad
    assert call(len=805) == -1 and b"not the signal's end" in lib.eben_last_error()
    assert call(end=1, len=765, base0=-19) == -1 and b"reach past" in lib.eben_last_error()
    assert call(n_out=0, tape=P(0x1000)) == 0   # nothing to do: no launch


def test_resample_ragged_validates_on_the_host():
    x = torch.zeros(2, 10)
    with pytest.raises(ValueError, match="nothing to resample"):
        rate.resample_ragged(x, [1, 2], 16000, 16000)
    with pytest.raises(ValueError, match="expected a float32"):
        rate.resample_ragged(x.double(), [1, 2], 48000, 16000)
    with pytest.raises(ValueError, match="expected a float32"):
        rate.resample_ragged(torch.zeros(2, 2, 10), [1, 2], 48000, 16000)
    from vibravox_amd._lib import EbenError

    with pytest.raises(EbenError, match="no CPU path"):
        rate.resample_ragged(x, [1, 2], 48000, 16000)
