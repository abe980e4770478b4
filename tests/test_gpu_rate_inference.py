"""GPU: inference on input at the recording's rate -- ``enhance_clips`` / ``evaluate_clips`` / ``StreamingEnhancer`` / ``enhance_stream``
with ``input_rate=48000`` against the same calls on clips resampled beforehand with ``augment.resample`` (the parent's whole-signal
kernel).  The resampling routes are bit-equal to that kernel row by row and stream by stream, so everything behind them sees the same
buffers: the results are compared with ``torch.equal``."""
import functools

import pytest
import torch

from tests import ragged_oracle as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
IN, MODEL = 48000, 16000


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def generator():
    gen, _ = R.formula_generator(1)   # EBENGenerator(4, 32, 1)
    return gen.to(DEV)


def test_enhance_clips_at_the_recording_rate(hip):
    from vibravox_amd import augment
    from vibravox_amd.inference import enhance_clips

    gen = generator()
    lengths = (3300, 7777, 20000, 20001, 47999)   # 1100 ... 16000 samples at the model's rate; two clips share a cut length
    shapes = ((-1,), (1, -1), (1, 1, -1), (-1,), (1, -1))
    clips = [(0.1 * randn((n,), n)).to(DEV).reshape(s) for n, s in zip(lengths, shapes)]
    before = [c.clone() for c in clips]
    at_model = [augment.resample(c, IN, MODEL) for c in clips]
    assert [c.shape[-1] for c in at_model] == [1100, 2593, 6667, 6667, 16000]
    for budget in (1 << 22, 20000):   # one ragged batch; several, among them batches of one clip and of equal cut lengths
        want, want_bands = enhance_clips(gen, at_model, return_bands=True, max_batch_samples=budget)
        got, got_bands = enhance_clips(gen, clips, return_bands=True, max_batch_samples=budget, input_rate=IN)
        for i in range(len(clips)):
            assert got[i].shape == want[i].shape and torch.equal(got[i], want[i]), (budget, i)
            assert torch.equal(got_bands[i], want_bands[i]), (budget, i)
            assert not torch.isnan(got[i]).any()
    assert all(torch.equal(a, b) for a, b in zip(clips, before))   # the clips are only read
    # without input_rate, or at the model's own, the call is today's
    plain = enhance_clips(gen, at_model)
    assert all(torch.equal(a, b) for a, b in zip(plain, want))
    assert all(torch.equal(a, b) for a, b in zip(enhance_clips(gen, at_model, input_rate=MODEL), plain))
    assert all(torch.equal(a, b) for a, b in zip(enhance_clips(gen, at_model, input_rate=None, model_rate=MODEL), plain))
    with pytest.raises(ValueError, match="too short"):
        enhance_clips(gen, [clips[0][:2900]], input_rate=IN)   # 967 samples at the model's rate
    with pytest.raises(ValueError, match="positive"):
        enhance_clips(gen, clips, input_rate=0)


def test_evaluate_clips_at_the_recording_rate(hip):
    from vibravox_amd import augment
    from vibravox_amd.inference import evaluate_clips

    gen = generator()
    lengths = (48003, 36000, 27001, 23331)
    reference = [(0.1 * randn((n,), n) * torch.sin(torch.arange(n) / 1500.0) ** 2).to(DEV) for n in lengths]
    corrupted = [(r.cpu() + 0.05 * randn((n,), n + 1)).to(DEV) for r, n in zip(reference, lengths)]
    cor16, ref16 = [augment.resample(c, IN, MODEL) for c in corrupted], [augment.resample(c, IN, MODEL) for c in reference]
    for budget in (1 << 22, 20000):
        want = evaluate_clips(gen, cor16, ref16, return_enhanced=True, max_batch_samples=budget)
        got = evaluate_clips(gen, corrupted, reference, return_enhanced=True, max_batch_samples=budget, input_rate=IN)
        for name in ("si_sdr", "stoi"):
            assert got[name].shape == (len(lengths),) and torch.equal(got[name], want[name]), (budget, name, got[name], want[name])
            assert torch.isfinite(got[name]).all()
        assert all(torch.equal(a, b) for a, b in zip(got["enhanced"], want["enhanced"]))
    same = evaluate_clips(gen, cor16, ref16, input_rate=MODEL)
    assert torch.equal(same["si_sdr"], want["si_sdr"]) and torch.equal(same["stoi"], want["stoi"])
    with pytest.raises(ValueError, match="its reference"):
        evaluate_clips(gen, corrupted, [r[:-1] for r in reference], input_rate=IN)
    # the Lightning module passes input_rate through
    from functools import partial

    from vibravox_amd.lightning_modules.eben import EBENLightningModule
    from vibravox_amd.optim import FusedAdam
    from vibravox_amd.torch_modules.dnn.eben_discriminator import DiscriminatorEBENMultiScales

    opt = partial(FusedAdam, lr=3e-4)
    mod = EBENLightningModule(sample_rate=MODEL, generator=gen, discriminator=DiscriminatorEBENMultiScales(q=4, min_channels=24).to(DEV),
                              generator_optimizer=opt, discriminator_optimizer=opt)
    through = mod.evaluate_clips(corrupted, reference, input_rate=IN)
    assert torch.equal(through["si_sdr"], want["si_sdr"]) and torch.equal(through["stoi"], want["stoi"])


def stream_through(enhancer, clip):
    """``clip`` (rows, 1, T) in pushes of the enhancer's input chunk and a finish with the rest: the returns in order."""
    chunk, total, pos, outs = enhancer.input_chunk_samples, clip.shape[2], 0, []
    with torch.no_grad():
        while total - pos >= chunk:
            outs.append(enhancer.push(clip[:, :, pos : pos + chunk]))
            pos += chunk
        outs.append(enhancer.finish(clip[:, :, pos:]))
    return outs


@functools.lru_cache(maxsize=None)
def stream_case(rows=1):
    """A clip at 48 kHz of about 20 chunks of 256 model-rate samples plus 37 input samples, and the whole-clip forward of its resampling."""
    from vibravox_amd import augment

    gen = generator()
    clip = (0.1 * randn((rows, 1, 20 * 768 + 37), 20 + rows)).to(DEV)
    with torch.no_grad():
        whole = gen(gen.cut_to_valid_length(augment.resample(clip, IN, MODEL)))
    return gen, clip, whole


@pytest.mark.parametrize("rows", [1, 2])
def test_streaming_enhancer_at_the_recording_rate(hip, rows):
    from vibravox_amd.streaming import StreamingEnhancer

    gen, clip, whole = stream_case(rows)
    enhancer = StreamingEnhancer(gen, 256, streams=rows, return_bands=True, input_rate=IN).prepare(DEV)
    for pair in enhancer.state.buffers.values():   # no state is read before it is written: the generator's, the FIFO, the resampler's tapes
        for t in pair:
            t.fill_(float("nan"))
    for t in enhancer._front.fifo + enhancer._front.resampler.state:
        t.fill_(float("nan"))
    assert enhancer.input_chunk_samples == 768 and enhancer.chunk_samples == 256
    outs = stream_through(enhancer, clip)
    enhanced, bands = torch.cat([o[0] for o in outs], dim=2), torch.cat([o[1] for o in outs], dim=2)
    assert enhanced.shape == whole[0].shape and torch.equal(enhanced, whole[0])
    assert bands.shape == whole[1].shape and torch.equal(bands, whole[1])
    # the enhancer gets chunk k - 1 at push k: the first samples come one push later than from a stream at the model's rate
    plain = StreamingEnhancer(gen, 256, streams=rows, return_bands=True)
    sizes = [o[0].shape[2] for o in outs]
    first = next(i for i, k in enumerate(sizes) if k)
    assert first == plain.plan.warmup_pushes + 1 and all(k == 0 for k in sizes[:first]) and all(k == 256 for k in sizes[first:-1])
    pushes = len(outs) - 1
    assert enhancer.input_latency == 768 + 3 * plain.latency == pushes * 768 - 3 * sum(sizes[:-1])
    # reset() starts a new stream on the same state
    state, fifo = enhancer.state, enhancer._front.fifo
    enhancer.reset()
    again = stream_through(enhancer, clip)
    assert enhancer.state is state and enhancer._front.fifo is fifo
    assert torch.equal(torch.cat([o[0] for o in again], dim=2), whole[0])


def test_enhance_stream_at_the_recording_rate(hip):
    from vibravox_amd import augment
    from vibravox_amd.inference import enhance_stream

    gen, clip, whole = stream_case(2)
    enhanced, bands = enhance_stream(gen, clip, chunk_samples=256, input_rate=IN)
    assert torch.equal(enhanced, whole[0]) and torch.equal(bands, whole[1])
    in_one, bands_one = enhance_stream(gen, clip, input_rate=IN)   # the default chunk is longer than the clip: everything comes out of finish()
    assert torch.equal(in_one, whole[0]) and torch.equal(bands_one, whole[1])
    # without input_rate, or at the model's own, the call is today's
    at_model = augment.resample(clip, IN, MODEL)
    today = enhance_stream(gen, at_model, chunk_samples=256)
    assert torch.equal(today[0], whole[0])
    for kw in (dict(input_rate=None), dict(input_rate=MODEL), dict(input_rate=8000, model_rate=8000)):
        same = enhance_stream(gen, at_model, chunk_samples=256, **kw)
        assert torch.equal(same[0], today[0]) and torch.equal(same[1], today[1])
    with pytest.raises(ValueError, match="too short"):
        enhance_stream(gen, clip[:, :, :2900], input_rate=IN)
    with pytest.raises(ValueError, match="smallest chunk_samples that works is 1280"):
        enhance_stream(gen, clip, chunk_samples=256, input_rate=44100)


def test_rated_enhancer_refuses_autograd_wrong_shapes_and_cpu_tensors(hip):
    from vibravox_amd._lib import EbenError
    from vibravox_amd.streaming import StreamingEnhancer

    gen = generator()
    enhancer = StreamingEnhancer(gen, 256, streams=2, input_rate=IN)
    good = torch.zeros(2, 1, 768, device=DEV)
    with pytest.raises(RuntimeError, match="no backward"):
        enhancer.push(good)
    with pytest.raises(RuntimeError, match="no backward"):
        enhancer.finish()
    with torch.no_grad():
        for bad in (good[:1], good[:, :, :767], good[:, :, :256], torch.zeros(2, 1, 769, device=DEV), good[:, 0], good.double(),
                    torch.zeros(2, 2, 768, device=DEV)):
            with pytest.raises(ValueError, match=r"expects a float32 \(2, 1, 768\)"):
                enhancer.push(bad)
        with pytest.raises(ValueError, match="expects"):
            enhancer.finish(good)              # a whole chunk is a push
        with pytest.raises(EbenError, match="no CPU path"):
            enhancer.push(good.cpu())
        assert enhancer.push(good).shape == (2, 1, 0)   # nothing above has moved the stream
        with pytest.raises(ValueError, match="too short"):
            enhancer.finish(good[:, :, :300])  # 1068 input samples in all: 356 at the model's rate
        assert enhancer.push(good).shape == (2, 1, 0)   # ... nor has the refused finish
