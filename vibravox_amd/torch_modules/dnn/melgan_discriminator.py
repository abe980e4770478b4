"""MelGAN waveform discriminators on the HIP grouped tap-conv kernels.

Drop-ins for ``vibravox/torch_modules/dnn/melgan_discriminator.py``:

  * ``DiscriminatorMelGAN`` (:76-169).  Same ``discriminator`` ModuleList indices -> same ``state_dict`` keys
    (``discriminator.0.1...``, ``discriminator.1.0...``, ..., ``discriminator.6...``); LeakyReLU(alpha) is fused in the
    conv epilogue.
  * ``MelganMultiScalesDiscriminator`` (:17-73): one ``DiscriminatorMelGAN`` per scale, fed the audio resampled to
    ``sample_rate // 2**s`` by torchaudio's ``Resample(..., resampling_method="sinc_interp_kaiser")``, restated on the
    device by ``ops.multirate_downsample`` (HIP forward and adjoint, ``csrc/multirate.hip``).
"""
from __future__ import annotations

from typing import List

import torch
from torch import nn

from ... import ops
from ..utils import normalized_conv1d

# (c_in, c_out, kernel, stride, padding, groups) -- melgan_discriminator.py:89-156
MELGAN_LAYERS = (
    (1, 16, 15, 1, 0, 1),
    (16, 64, 41, 4, 20, 4),
    (64, 256, 41, 4, 20, 4),
    (256, 1024, 41, 4, 20, 4),
    (1024, 1024, 41, 4, 20, 4),
    (1024, 1024, 5, 1, 2, 1),
    (1024, 1, 3, 1, 1, 1),
)


class ReflectionPad1d(nn.Module):
    def __init__(self, padding: int):
        super().__init__()
        self.padding = padding

    def forward(self, x):
        return ops.reflect_pad(x, self.padding, self.padding)


class DiscriminatorMelGAN(nn.Module):
    def __init__(self, alpha_leaky_relu: float):
        super().__init__()
        layers = []
        last = len(MELGAN_LAYERS) - 1
        for i, (ci, co, k, s, p, g) in enumerate(MELGAN_LAYERS):
            conv = normalized_conv1d(in_channels=ci, out_channels=co, kernel_size=k, stride=s, padding=p, groups=g,
                                     out_slope=1.0 if i == last else alpha_leaky_relu)
            if i == 0:
                layers.append(nn.Sequential(ReflectionPad1d(7), conv))
            elif i < last:
                layers.append(nn.Sequential(conv))
            else:
                layers.append(conv)
        self.discriminator = nn.ModuleList(layers)

    def forward(self, audio):
        embeddings = [audio]
        for module in self.discriminator:
            embeddings.append(module(embeddings[-1]))
        return embeddings


class KaiserResample(nn.Module):
    """torchaudio ``Resample(orig_freq, new_freq, resampling_method="sinc_interp_kaiser")`` on the device, differentiable.

    Holds no tensors: torchaudio registers its kernel as a non-persistent buffer, so it never appears in ``state_dict()``;
    here the table lives in ``ops``' per-(rates, device) cache instead.  (torchaudio is not installed here, so that
    ``persistent=False`` registration is an assumption this module's state_dict contract rests on, not a pinned fact.)
    """

    def __init__(self, orig_freq: int, new_freq: int):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        return ops.kaiser_resample(waveform, self.orig_freq, self.new_freq)

    def extra_repr(self) -> str:
        return f"orig_freq={self.orig_freq}, new_freq={self.new_freq}, resampling_method='sinc_interp_kaiser'"


class MelganMultiScalesDiscriminator(nn.Module):
    """Aggregation of MelGAN discriminators over the audio downsampled to ``sample_rate // 2**s``, s < scales.

    ``state_dict()`` holds only ``discriminators.{s}.discriminator...`` keys (``downsamplers`` are stateless, see
    ``KaiserResample``), and the discriminators are built in the reference's order, so one ``torch.manual_seed`` gives the
    reference's weights.  ``forward`` resamples every scale at once (``ops.multirate_downsample``: one fused HIP launch
    forward and one backward when ``sample_rate`` is divisible by ``2**(scales-1)``, the general rational path otherwise).
    """

    def __init__(self, sample_rate: int, scales: int = 3, alpha_leaky_relu: float = 0.2):
        super().__init__()
        self.sample_rate, self.scales = int(sample_rate), int(scales)
        self.discriminators = nn.ModuleList()
        self.downsamplers = nn.ModuleList()
        for scale in range(scales):
            self.discriminators.append(DiscriminatorMelGAN(alpha_leaky_relu))
            self.downsamplers.append(KaiserResample(orig_freq=sample_rate, new_freq=sample_rate // 2 ** scale))

    def forward(self, audio: torch.Tensor) -> List[List[torch.Tensor]]:
        """audio (batch, 1, samples) -> per scale, the discriminator's embeddings at each layer (batch, channel, time)."""
        return [self.discriminators[scale](signal) for scale, signal in enumerate(self.get_downsampled_versions(audio))]

    def get_downsampled_versions(self, audio: torch.Tensor) -> List[torch.Tensor]:
        """audio (batch, 1, samples) -> [Resample(sample_rate, sample_rate // 2**s)(audio) for s < scales]."""
        return ops.multirate_downsample(audio, self.sample_rate, self.scales)
