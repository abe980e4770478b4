"""EBEN multi-scale discriminators on the HIP grouped tap-conv kernels.

Drop-in for ``vibravox/torch_modules/dnn/eben_discriminator.py:10-163``:
``DiscriminatorEBENMultiScales(q, min_channels)`` = three dilated PQMF-band discriminators
(dilation 1, 2, 3) + one MelGAN discriminator; ``forward(bands, audio) -> List[List[Tensor]]`` with
element 0 the input and the last element the logits.  Attribute tree / ``state_dict`` keys
(``pqmf_discriminators.{i}.discriminator.{0.1,1.0,...,7}``, ``melgan_discriminator...``) are kept.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from ..utils import normalized_conv1d
from .melgan_discriminator import DiscriminatorMelGAN, ReflectionPad1d

try:
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover

    class PyTorchModelHubMixin:  # type: ignore
        pass


class DiscriminatorEBEN(nn.Module):
    """eben_discriminator.py:54-163: grouped dilated conv stack on the q last PQMF bands."""

    def __init__(self, dilation=1, q: int = 3, min_channels: int = 24):
        super().__init__()
        self.dilation = dilation
        assert min_channels % q == 0, "min_channels must be a multiple of q"
        c = min_channels
        # (c_in, c_out, kernel, stride, padding, groups, dilation, activated)
        table = [(q, c, 3, 1, 1, q, dilation, True)]
        table += [(c * 2 ** (i - 1), c * 2 ** i, 7, 2, 3, q, dilation, True) for i in range(1, 6)]
        table += [(c * 32, c * 32, 5, 1, 2, q, dilation, True), (c * 32, 1, 3, 1, 1, 1, 1, False)]
        layers = []
        for i, (ci, co, k, s, p, g, d, act) in enumerate(table):
            conv = normalized_conv1d(ci, co, kernel_size=(k,), stride=(s,), padding=(p,), dilation=d, groups=g,
                                     out_slope=0.2 if act else 1.0)
            if i == 0:
                layers.append(nn.Sequential(ReflectionPad1d(1), conv))
            elif act:
                layers.append(nn.Sequential(conv))
            else:
                layers.append(conv)
        self.discriminator = nn.ModuleList(layers)

    def forward(self, bands):
        embeddings = [bands]
        for module in self.discriminator:
            embeddings.append(module(embeddings[-1]))
        return embeddings


class DiscriminatorEBENMultiScales(nn.Module, PyTorchModelHubMixin):
    def __init__(self, q: int = 3, min_channels: int = 24):
        super().__init__()
        self.q = q
        self.pqmf_discriminators = torch.nn.ModuleList(
            [DiscriminatorEBEN(dilation=d, q=q, min_channels=min_channels) for d in (1, 2, 3)]
        )
        self.melgan_discriminator = DiscriminatorMelGAN(alpha_leaky_relu=0.2)

    #: run the four independent sub-discriminators on separate HIP streams (forward here, backward by
    #: autograd on the same streams): their kernels are latency-bound with small grids on the deep
    #: layers, so overlapping them fills CUs that a single stream leaves idle.
    concurrent_streams: bool = os.environ.get("EBEN_D_STREAMS", "1") != "0"

    def forward(self, bands, audio):
        sub = bands[:, -self.q :, :]
        if not (self.concurrent_streams and bands.is_cuda):
            embeddings = [dis(sub) for dis in self.pqmf_discriminators]
            embeddings.append(self.melgan_discriminator(audio))
            return embeddings
        if sub.data_ptr() != bands.data_ptr() or not sub.is_contiguous():
            sub = sub.contiguous()
        main = torch.cuda.current_stream()
        if getattr(self, "_streams", None) is None or self._streams[0].device != bands.device:
            self._streams = [torch.cuda.Stream(device=bands.device) for _ in range(4)]
        nets = list(self.pqmf_discriminators) + [self.melgan_discriminator]
        inputs = [sub, sub, sub, audio]
        embeddings = []
        for net, x, st in zip(nets, inputs, self._streams):
            st.wait_stream(main)
            x.record_stream(st)
            with torch.cuda.stream(st):
                embeddings.append(net(x))
        for st, scale in zip(self._streams, embeddings):
            main.wait_stream(st)
            for t in scale[1:]:
                t.record_stream(main)
        return embeddings

    @torch.no_grad()
    def forward_ragged(self, bands, audio, plan):
        """Rows of different lengths in one pass (inference): ``bands`` (rows, m, plan.bands_l_buf) and ``audio`` (rows, 1,
        plan.audio_l_buf) hold row r on ``[0, plan.band_lengths[r])`` / ``[0, plan.cut[r])`` -- usually the enhanced and the reference
        branch stacked as 2R rows -- with ``plan = ragged.disc_plan(self, ...)``.  Returns ``(embeddings, lens)``: ``forward``'s
        lists, every row equal to its own batch-1 forward on ``[0, lens[chain][level, row])`` (device int32, level 0 the input) and
        junk behind.  In front of each layer the plan's ``eben_edge_fill`` calls run on that layer's input, then the layer's ordinary
        module; the inputs are copied first, so the caller's ``bands`` and ``audio`` stay as they are."""
        from ... import ops, ragged

        rows = len(plan.cut)
        if (bands.dim() != 3 or audio.dim() != 3 or bands.shape[0] != rows or bands.shape[2] != plan.bands_l_buf or bands.shape[1] < self.q
                or audio.shape != (rows, 1, plan.audio_l_buf)):
            raise ValueError(f"forward_ragged: expected ({rows}, >= {self.q}, {plan.bands_l_buf}) bands and ({rows}, 1, {plan.audio_l_buf}) audio "
                             f"for this plan, got {tuple(bands.shape)} and {tuple(audio.shape)}")
        nets = list(self.pqmf_discriminators) + [self.melgan_discriminator]
        tables = [plan.lengths(c) for c in range(len(plan.chains))]
        flat = torch.tensor([row for table in tables for row in table], dtype=torch.int32).to(bands.device, non_blocking=True)   # the one upload
        lens, at = [], 0
        for table in tables:
            lens.append(flat[at : at + len(table)])
            at += len(table)
        sub = bands[:, -self.q :, :]
        if not plan.ragged:   # equal rows need no fill: the batched forward
            return [net(x) for net, x in zip(nets, (sub, sub, sub, audio))], lens
        sub, audio = sub.clone(memory_format=torch.contiguous_format), audio.clone(memory_format=torch.contiguous_format)
        modes = {ragged.ZERO: ops.FILL_ZERO, ragged.MIRROR: ops.FILL_MIRROR}
        embeddings = []
        for c, (net, x) in enumerate(zip(nets, (sub, sub, sub, audio))):
            chain = [x]
            for level, (layer, module) in enumerate(zip(plan.chains[c], net.discriminator)):
                if x.shape[2] != layer.in_buffer:
                    raise RuntimeError(f"ragged plan out of step with the forward: {layer.path} on {tuple(x.shape)}")
                for mode, count in layer.fills:
                    ops.edge_fill(x, lens[c][level], modes[mode], count)
                x = module(x)
                chain.append(x)
            embeddings.append(chain)
        return embeddings, lens
