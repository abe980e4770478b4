"""GPU: the integrated loudness of ITU-R BS.1770-4 (``eben_loudness`` through ``vibravox_amd.metrics.loudness_gain``), the metric class
and ``inference.evaluate_clips(metrics=("lufs_diff",))`` on top of it.

Rows per rate (``tests/loudness_oracle.py`` ``row_lengths``): one sample short of a block (``-inf``, gain 1), one block, around the
second block, the first chunk's edge (4095 / 4096 / 4097: no block yet, the peak alone), the first chunk edge behind a whole block,
about a second (several chunks, the carry) and three seconds with one stretch under each gate; 16 kHz, 44.1 kHz (hops that are no
multiple of a thread's 16 samples) and 48 kHz.

Bar against the float64 oracle of every row ALONE: ``|L - oracle| <= ulp32(oracle) + 100 * ORACLE_SPREAD`` -- one float32 ulp because
the output is the float32 rounding of a float64 value, and a hundred times the oracle's own two-route disagreement (9.6e-13 LU,
``tests/test_loudness_oracle.py`` prints it) for a third order of the recurrence and of the sums.  The peak is bit-equal to ``max |x|``;
the gain is within one float32 ulp of the float64 formula on the oracle's ``L``.  No block of any row lies within 0.5 LU of a gate
(asserted on the oracle there), so a flipped block cannot hide behind the bar.

Bit equality (compared as int32, so NaN equals NaN and -inf equals -inf): every row of a padded batch with NaN behind every row's end
has the bits of the dense call on that row alone, also reversed and in a wider buffer.

[MI355X] observed maxima over the 8 rows with a block of each rate (``test_rows_of_different_lengths_against_the_oracle`` prints them
with -s): ``|L - oracle|`` 9.3e-7 LU at 16 kHz (0.490 float32 ulp of the oracle value, the row of 3 s), 5.9e-7 at 44.1 kHz (0.309 ulp, the
row of 44 137 samples), 9.4e-7 at 48 kHz (0.493 ulp, the row of 48 037 samples), each against a bar of 1.9e-6 -- the float32 rounding of the
result and nothing else; the gain 0.487 / 0.408 / 0.481 float32 ulp from the formula; the peak bit-equal; 70 s at 16 kHz (697 blocks)
6.3e-7 LU.  Ragged against every row alone, reversed, widened, with a device table, dense: 0 bit differences."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import loudness_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SLACK = 37                      # t_max is larger than the longest row
TARGET, CEILING = -23.0, -1.0


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def padded(rows_of, t, order):
    """The rows (1-D arrays, each its own length) in a (rows, t) device buffer, NaN behind every row's end."""
    body = np.full((len(order), t), np.nan, np.float32)
    for r, i in enumerate(order):
        body[r, : len(rows_of[i])] = rows_of[i]
    return torch.from_numpy(body).to(DEV)


def run_ragged(rows_of, fs, extra=0, reverse=False, lengths=None, target=TARGET, peak=CEILING):
    """The rows (reversed, in a buffer ``extra`` wider) through ``metrics.loudness_gain``: (3, rows) float32 -- loudness, peak, gain -- in
    the rows' own order.  ``lengths``: a device table that replaces the rows' own lengths."""
    from vibravox_amd.metrics import loudness_gain

    order = list(range(len(rows_of)))[::-1] if reverse else list(range(len(rows_of)))
    t = max(len(x) for x in rows_of) + SLACK + extra
    x = padded(rows_of, t, order)
    keep = x.clone()
    got = loudness_gain(x, fs, [len(rows_of[i]) for i in order] if lengths is None else lengths, target, peak)
    for v in got:
        assert v.shape == (len(order),) and v.dtype is torch.float32 and v.is_cuda
    assert same_bits(x, keep)       # the input is untouched
    back = torch.tensor(np.argsort(order), device=DEV)
    return torch.stack([v.index_select(0, back) for v in got])


def alone(rows_of, fs):
    """The dense call on every row alone: a (1, n) buffer of its own, no lengths."""
    from vibravox_amd.metrics import loudness_gain

    cols = []
    for x in rows_of:
        got = loudness_gain(torch.from_numpy(np.ascontiguousarray(x[None])).to(DEV), fs, None, TARGET, CEILING)
        cols.append(torch.stack([v.reshape(()) for v in got]))
    return torch.stack(cols, dim=1)


@functools.lru_cache(maxsize=None)
def batch(fs):
    rows_of = O.inputs(fs)
    return rows_of, run_ragged(rows_of, fs), alone(rows_of, fs)


@pytest.mark.parametrize("fs", O.RATES)
def test_rows_of_different_lengths_against_the_oracle(hip, fs):
    rows_of, got, _ = batch(fs)
    got = got.cpu().numpy()
    want = O.table(fs)
    level = np.array([w[0] for w in want])
    finite = np.isfinite(level)
    assert finite.sum() >= 8 and (~finite).sum() == 4
    # rows without a block: -inf, gain 1
    assert np.all(got[0][~finite] == -np.inf) and np.all(got[2][~finite] == 1.0)
    err = np.abs(got[0][finite].astype(np.float64) - level[finite])
    bar = O.bar(level[finite])
    worst = int(np.argmax(err / bar))
    lengths = np.array([len(x) for x in rows_of])[finite]
    print(f"[{fs} Hz] largest |L - oracle| = {err.max():.3e} LU ({(err / O.ulp32(level[finite])).max():.3f} float32 ulp of the oracle value); "
          f"closest to its bar: the row of {lengths[worst]} samples, {err[worst]:.3e} of {bar[worst]:.3e}")
    assert np.isfinite(got[0][finite]).all() and (err <= bar).all(), (lengths[worst], err[worst], bar[worst])
    # the peak: max |x|, bit for bit
    assert np.array_equal(got[1].view(np.int32), np.array([w[1] for w in want], dtype=np.float32).view(np.int32))
    # the gain: the float64 formula on the oracle's L, rounded to float32 -- one ulp for the device's own L and pow
    formula = np.array([O.gain(w[0], w[1], TARGET, CEILING) for w in want])
    gerr = np.abs(got[2].astype(np.float64) - formula) / O.ulp32(formula)
    print(f"[{fs} Hz] largest |gain - formula| = {gerr.max():.3f} float32 ulp; gains {formula[finite].min():.3f} ... {formula[finite].max():.3f}")
    assert (gerr <= 1.0).all(), gerr


@pytest.mark.parametrize("fs", O.RATES)
def test_every_row_has_the_bits_of_the_call_on_it_alone(hip, fs):
    rows_of, got, each = batch(fs)
    assert same_bits(got, each), (got, each)
    # wherever the row stands and however wide the buffer is
    assert same_bits(run_ragged(rows_of, fs, reverse=True), each)
    assert same_bits(run_ragged(rows_of, fs, extra=5000), each)
    # a device table of lengths is used as it is
    lens = torch.tensor([len(x) for x in rows_of], dtype=torch.int32, device=DEV)
    assert same_bits(run_ragged(rows_of, fs, lengths=lens), each)
    # dense: rows of one length without a table are those rows with one
    from vibravox_amd.metrics import integrated_loudness, loudness_gain

    n = len(rows_of[-2])
    dense = torch.from_numpy(np.stack([x[:n] for x in rows_of[-2:]])).to(DEV)
    a, b = loudness_gain(dense, fs), loudness_gain(dense, fs, [n, n])
    assert all(same_bits(u, v) for u, v in zip(a, b)) and same_bits(integrated_loudness(dense.reshape(2, 1, n), fs).reshape(2), a[0])


def test_special_rows(hip):
    fs = 16000
    x = O.inputs(fs)[-1]
    h = fs // 10
    loud = x.copy()
    loud[1000] = 5.0                                                   # one spike: a crest factor at which the ceiling binds, not the target
    quiet = (x.astype(np.float64) * 1e-5).astype(np.float32)           # everything under the absolute gate
    rows_of = [np.zeros(3 * fs, np.float32), quiet, loud, x, np.zeros(0, np.float32), x[: 4 * h]]
    got = run_ragged(rows_of, fs).cpu().numpy()
    level, peak, gain = got
    assert level[0] == -np.inf and peak[0] == 0.0 and gain[0] == 1.0                     # silence
    assert level[1] == -np.inf and peak[1] == np.abs(quiet).max() and gain[1] == 1.0      # under the gate
    assert level[4] == -np.inf and peak[4] == 0.0 and gain[4] == 1.0                     # a row of no samples
    ceiling = 10.0 ** (CEILING / 20.0)
    want_loud = O.loudness(loud, fs)
    assert abs(level[2] - want_loud) <= O.bar(np.array([want_loud]))[0]
    assert 10.0 ** ((TARGET - want_loud) / 20.0) * float(np.abs(loud).max()) > ceiling   # the plain gain would pass the ceiling
    bound = ceiling / float(np.abs(loud).max())
    assert abs(gain[2] - bound) <= O.ulp32(np.array([bound]))[0]
    # on x itself the target binds, not the ceiling; a lower ceiling binds on it
    want_x = O.loudness(x, fs)
    assert abs(gain[3] - 10.0 ** ((TARGET - want_x) / 20.0)) <= O.ulp32(np.array([gain[3]]))[0]
    low = run_ragged(rows_of, fs, peak=-20.0).cpu().numpy()
    bound = 10.0 ** (-20.0 / 20.0) / float(np.abs(x).max())
    assert abs(low[2][3] - bound) <= O.ulp32(np.array([bound]))[0] and np.array_equal(low[0].view(np.int32), level.view(np.int32))
    # a device table with lengths outside [0, t_max]: those rows are NaN (gain 1), the others are what they were
    t = max(len(r) for r in rows_of) + SLACK
    lens = torch.tensor([len(r) for r in rows_of], dtype=torch.int32, device=DEV)
    lens[0], lens[3] = -1, t + 1
    bad = run_ragged(rows_of, fs, lengths=lens).cpu().numpy()
    assert np.isnan(bad[0][[0, 3]]).all() and np.isnan(bad[1][[0, 3]]).all() and (bad[2][[0, 3]] == 1.0).all()
    keep = [1, 2, 4, 5]
    assert np.array_equal(bad[:, keep].view(np.int32), got[:, keep].view(np.int32))
    # NaN samples make the row NaN, and only that row
    poisoned = [r.copy() for r in rows_of]
    poisoned[3][fs] = np.nan
    nan = run_ragged(poisoned, fs).cpu().numpy()
    assert np.isnan(nan[0][3]) and np.isnan(nan[1][3]) and nan[2][3] == 1.0
    assert np.array_equal(np.delete(nan, 3, axis=1).view(np.int32), np.delete(got, 3, axis=1).view(np.int32))


def test_a_long_row_runs_the_block_loop_past_a_workgroup(hip):
    """70 s at 16 kHz: 697 blocks, more than the 256 threads of the finishing workgroup, 274 chunks through the carry."""
    fs = 16000
    rng = np.random.default_rng(77)
    x = (0.05 * rng.standard_normal(70 * fs)).astype(np.float32)
    x[20 * fs : 30 * fs] *= np.float32(1e-5)
    x[40 * fs : 50 * fs] *= np.float32(0.05)
    z = O.blocks(x, fs)
    want, l, rel, kept = O.gated(z)
    assert len(z) == 697 and 400 < kept.sum() < 697 and np.abs(l - O.ABSOLUTE_GATE).min() >= 0.5 and np.abs(l[l > -70] - rel).min() >= 0.5
    from vibravox_amd.metrics import integrated_loudness

    got = float(integrated_loudness(torch.from_numpy(x).to(DEV), fs))
    print(f"[70 s at 16 kHz] |L - oracle| = {abs(got - want):.3e} LU, bar {O.bar(np.array([want]))[0]:.3e}")
    assert abs(got - want) <= O.bar(np.array([want]))[0]


def test_raw_entry_refuses_on_device_pointers(hip):
    """The refusals of ``tests/test_loudness_oracle.py`` hold with device memory too, and leave the outputs as they were."""
    from vibravox_amd import _lib

    lib = _lib.load()
    x = torch.zeros(4, 2000, device=DEV)
    out = torch.full((3, 4), 7.0, device=DEV)
    need = lib.eben_loudness_workspace(4, 2000, 16000)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    call = lambda **kw: lib.eben_loudness(kw.get("x", x.data_ptr()), kw.get("rows", 4), kw.get("t_max", 2000), None, kw.get("fs", 16000),
                                          kw.get("target", -23.0), kw.get("peak", -1.0), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                          kw.get("ws", ws.data_ptr()), kw.get("ws_bytes", need), _lib.stream())
    for kw in (dict(x=None), dict(rows=0), dict(rows=65536), dict(t_max=0), dict(fs=44101), dict(fs=0), dict(target=float("nan")),
               dict(peak=float("inf")), dict(ws=None), dict(ws=ws.data_ptr() + 4), dict(ws_bytes=need - 1), dict(x=x.data_ptr() + 2)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert out[0].tolist() == [-math.inf] * 4 and out[1].tolist() == [0.0] * 4 and out[2].tolist() == [1.0] * 4


def test_metric_class_and_lufs_diff(hip):
    from tests import ragged_oracle as R
    from vibravox_amd import inference
    from vibravox_amd.metrics import IntegratedLoudness, integrated_loudness

    fs = 16000
    rows_of = O.inputs(fs)
    level = np.array([w[0] for w in O.table(fs)])
    finite = np.isfinite(level)
    metric = IntegratedLoudness(fs)
    t = max(len(x) for x in rows_of)
    first = metric(padded(rows_of, t, list(range(len(rows_of)))), [len(x) for x in rows_of])
    assert abs(float(first) - level[finite].mean()) <= 1e-5
    metric.update(torch.from_numpy(rows_of[-1]).to(DEV))
    assert abs(float(metric.compute()) - (level[finite].sum() + level[-1]) / (finite.sum() + 1)) <= 1e-5
    metric.reset()
    with pytest.raises(RuntimeError):
        metric.compute()
    # lufs_diff: L(enhanced) - L(reference) at 16 kHz on the cut clips, one value per pair in input order
    gen = R.formula_generator(1, 32)[0].to(DEV).eval()
    clips = [torch.from_numpy(rows_of[i]).to(DEV).reshape(1, 1, -1) for i in (-1, -2, 1)]
    refs = [0.5 * c for c in clips]
    out = inference.evaluate_clips(gen, clips, refs, metrics=("si_sdr", "lufs_diff"), return_enhanced=True)
    assert out["lufs_diff"].shape == (3,) and out["lufs_diff"].dtype is torch.float32
    for k, (e, r) in enumerate(zip(out["enhanced"], refs)):
        n = e.shape[-1]
        want = integrated_loudness(e.reshape(-1), fs) - integrated_loudness(r.reshape(-1)[:n].contiguous(), fs)
        assert same_bits(out["lufs_diff"][k].reshape(1), want.reshape(1)), k
