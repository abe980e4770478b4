"""CPU: the host side of corpus evaluation in ragged batches -- the three ``eben_*_ragged`` entries' exports and refusals, the
validation of a host-side ``lengths`` in ``vibravox_amd.metrics``, the refusals of ``inference.evaluate_clips`` (all of them before any
device work) and the 16 kHz length helper."""
import ctypes
import math

import pytest
import torch

from tests import ragged_oracle as R
from vibravox_amd import inference
from vibravox_amd._lib import EbenError, load


@pytest.fixture(scope="module")
def lib():
    return load()


@pytest.fixture(scope="module")
def gen():
    return R.formula_generator(1, 32)[0]


def test_library_exports_the_ragged_entries_at_abi_5(lib):
    for name in ("eben_si_sdr_ragged", "eben_stoi_ragged_workspace", "eben_stoi_ragged"):
        assert getattr(lib, name) is not None
    assert lib.eben_version() == 6


@pytest.mark.parametrize("fs", [16000, 10000, 48000])
def test_ragged_workspace_covers_the_dense_one(lib, fs):
    for rows, t in ((0, 100), (3, 0), (-1, 100), (3, -5)):
        assert lib.eben_stoi_ragged_workspace(rows, t, fs) == 0
    assert lib.eben_stoi_ragged_workspace(3, 100, 0) == 0
    for rows, t in ((1, 1), (1, 257), (5, 4100), (8, 40003), (64, 192000)):
        assert lib.eben_stoi_ragged_workspace(rows, t, fs) >= lib.eben_stoi_workspace(rows, t, fs) > 0


def test_raw_entries_refuse_bad_arguments_before_any_launch(lib):
    """The pointers are host memory: nothing may be launched on them (no GPU here anyway) -- every call returns in the checks."""
    x = (ctypes.c_float * 64)()
    lens = (ctypes.c_int32 * 4)(16, 16, 16, 16)
    out = (ctypes.c_float * 4)()
    msg = lambda: lib.eben_last_error()
    assert lib.eben_si_sdr_ragged(None, x, 4, 16, lens, out, None) == -1 and b"null" in msg()
    assert lib.eben_si_sdr_ragged(x, None, 4, 16, lens, out, None) == -1
    assert lib.eben_si_sdr_ragged(x, x, 4, 16, None, out, None) == -1
    assert lib.eben_si_sdr_ragged(x, x, 4, 16, lens, None, None) == -1
    assert lib.eben_si_sdr_ragged(x, x, 0, 16, lens, out, None) == -1 and b"rows" in msg()
    assert lib.eben_si_sdr_ragged(x, x, 65536, 16, lens, out, None) == -1
    assert lib.eben_si_sdr_ragged(x, x, 4, 0, lens, out, None) == -1
    ws = (ctypes.c_char * 4096)()
    table = (ctypes.c_float * 9)()
    args = lambda **kw: [kw.get(k, d) for k, d in (("clean", x), ("processed", x), ("rows", 4), ("t_max", 16), ("lengths", lens), ("fs", 16000),
                                                   ("table", table), ("taps", 9), ("ws", ws), ("ws_bytes", 4096), ("out", out), ("stream", None))]
    for key in ("clean", "processed", "lengths", "ws", "out"):
        assert lib.eben_stoi_ragged(*args(**{key: None})) == -1 and b"null" in msg(), key
    for kw in (dict(rows=0), dict(rows=65536), dict(t_max=0), dict(t_max=-3), dict(fs=0), dict(table=None), dict(taps=8), dict(taps=0)):
        assert lib.eben_stoi_ragged(*args(**kw)) == -1, kw
    need = lib.eben_stoi_ragged_workspace(4, 16, 16000)
    assert need <= 4096
    assert lib.eben_stoi_ragged(*args(ws_bytes=need - 1)) != 0 and b"workspace" in msg()


def test_cpu_tensors_raise_eben_error_with_lengths_too():
    from vibravox_amd.metrics import ScaleInvariantSignalDistortionRatio, si_sdr, stoi

    p, g = torch.randn(3, 400), torch.randn(3, 400)
    for lengths in ([400, 300, 1], torch.tensor([400, 300, 1]), torch.tensor([400, 300, 1], dtype=torch.int32)):
        with pytest.raises(EbenError):
            si_sdr(p, g, lengths=lengths)
        with pytest.raises(EbenError):
            stoi(p, g, 16000, lengths=lengths)
    with pytest.raises(EbenError):
        ScaleInvariantSignalDistortionRatio().update(p, g, lengths=[400, 300, 1])


@pytest.mark.parametrize("lengths,row", [([400, 0, 5], 1), ([400, 300, 401], 2), ([-1, 300, 5], 0), (torch.tensor([400, 300, 401]), 2),
                                         (torch.tensor([[400], [0], [7]]), 1)])
def test_host_lengths_out_of_range_name_the_row(lengths, row):
    from vibravox_amd.metrics import ShortTimeObjectiveIntelligibility, si_sdr, stoi

    p, g = torch.randn(3, 400), torch.randn(3, 400)
    for call in (lambda: si_sdr(p, g, lengths=lengths), lambda: stoi(p, g, 16000, lengths=lengths),
                 lambda: ShortTimeObjectiveIntelligibility(16000)(p, g, lengths=lengths)):
        with pytest.raises(ValueError, match=rf"row {row} "):
            call()


def test_host_lengths_of_the_wrong_count_or_type_are_refused():
    from vibravox_amd.metrics import si_sdr, stoi

    p, g = torch.randn(2, 3, 400), torch.randn(2, 3, 400)
    for lengths in ([400] * 5, [400] * 7, [], torch.full((5,), 400)):
        with pytest.raises(ValueError, match="6 rows"):
            si_sdr(p, g, lengths=lengths)
        with pytest.raises(ValueError, match="6 rows"):
            stoi(p, g, 16000, lengths=lengths)
    with pytest.raises(ValueError, match="integer"):
        si_sdr(p, g, lengths=torch.full((6,), 400.0))
    with pytest.raises(ValueError, match="integer"):
        si_sdr(p, g, lengths=[400, 400, 400, 400, 400, 399.5])


def test_evaluate_clips_refuses_bad_pairs_before_any_device_work(gen):
    clip = lambda t: torch.zeros(1, 1, t)
    ok = [clip(2000), clip(1500)]
    with pytest.raises(ValueError, match="pair 1"):
        inference.evaluate_clips(gen, ok, [clip(2000), clip(1499)])
    with pytest.raises(ValueError, match="2 corrupted clips and 1 references"):
        inference.evaluate_clips(gen, ok, ok[:1])
    with pytest.raises(ValueError, match="clip 1"):    # below the shortest clip the generator takes: refused by ragged.plan, by index
        inference.evaluate_clips(gen, [clip(2000), clip(700), clip(3000)], [clip(2000), clip(700), clip(3000)])
    with pytest.raises(ValueError, match="corrupted clip 1"):
        inference.evaluate_clips(gen, [clip(2000), torch.zeros(2, 1500)], ok)
    with pytest.raises(ValueError, match="reference clip 0"):
        inference.evaluate_clips(gen, ok, [clip(2000).double(), clip(1500)])
    with pytest.raises(ValueError, match="reference clip 1"):
        inference.evaluate_clips(gen, ok, [clip(2000), torch.zeros(1, 1, 1, 1500)])
    with pytest.raises(ValueError, match="sample_rate"):
        inference.evaluate_clips(gen, ok, ok, sample_rate=0)
    with pytest.raises(ValueError):
        inference.evaluate_clips(gen, [], [])


@pytest.mark.parametrize("orig", [48000, 44100])
@pytest.mark.parametrize("length", [1, 2, 3, 44101])
def test_length_at_16k_is_the_resamplers(orig, length):
    g = math.gcd(orig, 16000)
    o, n = orig // g, 16000 // g
    assert inference.resampled_length(length, orig, 16000) == int(math.ceil(n * length / o))    # augment.resample's t_out
    assert inference.resampled_length(length, 16000, 16000) == length
