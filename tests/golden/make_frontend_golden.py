"""Generate tests/golden/frontend_golden.npz from the REFERENCE functions of vibravox/utils.py
(mix_speech_and_noise_with_rescaling, set_audio_duration).  Build container only (needs /root/reference);
``torchaudio.functional.lowpass_biquad`` (imported at utils.py:4, unused here) is stubbed in a temp dir, as
make_collate_golden.py does.  Inputs are its ragged ``items()``.

Recorded:
  mixr/seed{s}/r{k}/noisy{i}, scaled{i}   the reference mixer's two outputs, snr_range k = 0: (-3, 5), 1: (0, 0)
  mixr/seed{s}/r{k}/gain                  the gains of that call: the reference's lines (utils.py:163-184) replayed under the same seed,
                                          asserted to reproduce the recorded scaled noise bit for bit
  mixr/seed{s}/r{k}/start                 the noise offsets it drew
  bwe/seed{s}/det{d}/bc{i}, air{i}        set_audio_duration(body, 800, airborne, det) on the raw clips
  check:gain_rel                          worst |gain - gain64| / gain64, gain64 the same chain on float64-mean powers rounded once

Usage:  python tests/golden/make_frontend_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_collate_golden import items  # noqa: E402

SNR_RANGES = [(-3.0, 5.0), (0.0, 0.0)]


def main():
    stub = tempfile.mkdtemp(prefix="ta_stub_")
    os.makedirs(os.path.join(stub, "torchaudio"))
    open(os.path.join(stub, "torchaudio", "__init__.py"), "w").close()
    with open(os.path.join(stub, "torchaudio", "functional.py"), "w") as f:
        f.write("def lowpass_biquad(*a, **k):\n    raise NotImplementedError\n")
    sys.path.insert(0, stub)
    sys.path.insert(0, "/root/reference")
    from vibravox.utils import mix_speech_and_noise_with_rescaling, set_audio_duration

    g = {}
    batch = items()
    speech = [b["audio_body_conducted"] for b in batch]
    noise = [b["audio_body_conducted_speechless_noisy"] for b in batch]
    worst = 0.0
    for seed in (0, 1):
        for k, rng in enumerate(SNR_RANGES):
            torch.manual_seed(seed)
            noisy, scaled = mix_speech_and_noise_with_rescaling(speech, noise, snr_range=rng)
            torch.manual_seed(seed)
            gains, starts = [], []
            for i, (s, n) in enumerate(zip(speech, noise)):
                start = torch.randint(0, n.size(0) - s.size(0), (1,)).item()
                snr = torch.empty(1).uniform_(rng[0], rng[1])
                snr_linear = 10 ** (snr / 10.0)
                gain = torch.sqrt(torch.mean(s ** 2) / (torch.mean(n ** 2) * snr_linear))
                assert torch.equal(n[start: start + s.size(0)] * gain, scaled[i]), "the replay left the reference's arithmetic"
                p64 = [torch.tensor(np.float32(np.mean(v.numpy().astype(np.float64) ** 2))) for v in (s, n)]
                gain64 = torch.sqrt(p64[0] / (p64[1] * snr_linear))
                worst = max(worst, abs(float(gain) - float(gain64)) / float(gain64))
                gains.append(gain)
                starts.append(start)
                g[f"mixr/seed{seed}/r{k}/noisy{i}"] = noisy[i].numpy()
                g[f"mixr/seed{seed}/r{k}/scaled{i}"] = scaled[i].numpy()
            g[f"mixr/seed{seed}/r{k}/gain"] = torch.cat(gains).numpy()
            g[f"mixr/seed{seed}/r{k}/start"] = np.array(starts, np.int64)
        for det in (False, True):
            torch.manual_seed(seed)
            for i, b in enumerate(batch):
                a, ab = set_audio_duration(audio=b["audio_body_conducted"], desired_samples=800, audio_bis=b["audio_airborne"], deterministic=det)
                g[f"bwe/seed{seed}/det{int(det)}/bc{i}"] = a.numpy()
                g[f"bwe/seed{seed}/det{int(det)}/air{i}"] = ab.numpy()
    g["check:gain_rel"] = np.array(worst)
    np.savez_compressed(os.path.join(HERE, "frontend_golden.npz"), **g)
    print("wrote", len(g), "arrays; check:gain_rel =", worst)


if __name__ == "__main__":
    main()
