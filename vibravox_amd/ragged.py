"""Ragged-batch plan of the EBEN generator's inference: clips of any lengths in one pass (host only, no GPU needed).

A conv's output at position l reads only the input samples its taps reach, so the edge rule of a layer -- reflect, zero, or the end of
a transposed conv -- matters only for outputs whose taps cross the end of the buffer.  Rows of different lengths share one buffer when
every row has some slack behind its own end and, in front of each layer, that slack holds what the row's own edge rule would have
supplied: the mirror ``x[L + j] = x[L - 2 - j]`` for reflect-padded layers, zero for zero-padded and transposed ones.  The layer's
ordinary kernel then computes the row's outputs ``[0, L_out)`` exactly as the row's own batch-1 forward does; what it writes beyond is
junk nobody reads, and the next fill overwrites the part that matters.

``plan`` walks the generator's layer table (``gen_layers.layers``: the order ``GeneratorEngine.forward`` launches, a ResidualUnit
standing as its dilated conv) and derives, from each entry's ``ConvSpec``, how many samples past a row's last one the row's last
output reads -- the fill count in front of that layer -- and from the largest such reach the margin every row needs.  ``compose_batches`` deals a corpus into such batches.
"""
from __future__ import annotations

import dataclasses
from typing import List, Sequence, Tuple

from .gen_layers import layers

MIRROR, ZERO, ZERO_ALL = "mirror", "zero", "zero_all"   # ZERO_ALL: the whole slack (the input and the two outputs); count = what is needed


@dataclasses.dataclass(frozen=True)
class Fill:
    layer: str   # module path of the layer whose input is filled (the dilated conv of a ResidualUnit stands for the unit)
    mode: str    # MIRROR | ZERO | ZERO_ALL
    count: int   # samples at that layer's rate
    level: int   # row of RaggedPlan.row_lengths / index of RaggedPlan.buffer_lengths of the tensor filled


@dataclasses.dataclass(frozen=True)
class RaggedPlan:
    lengths: Tuple[int, ...]                    # the clips' own lengths
    cut: Tuple[int, ...]                        # EBENGenerator.cut_to_valid_length of each: the rows' lengths in samples
    l_buf: int                                  # samples per row of the padded buffer
    margin: int                                 # l_buf - max(cut); 0 when all rows are equal
    buffer_lengths: Tuple[int, ...]             # per resolution: audio, bands, then behind each encoder block
    row_lengths: Tuple[Tuple[int, ...], ...]    # [resolution][row]
    fills: Tuple[Fill, ...]                     # in launch order; empty when all rows are equal

    @property
    def ragged(self) -> bool:
        return self.margin != 0


def cut_length(gen, length: int) -> int:
    """``gen.cut_to_valid_length`` on a length."""
    return length - (length + gen.pqmf.kernel_size) % gen.multiple


def reach(spec, l_in: int) -> int:
    """Input samples past the row's last one that the row's last output reads (<= 0: none)."""
    l_out = spec.out_len(l_in)
    if spec.transposed:   # output o sums inputs i with 0 <= o + pad - i stride <= (k - 1) dil: the last one is floor((o + pad) / stride)
        return (l_out - 1 + spec.pad_l) // spec.stride - (l_in - 1)
    return (l_out - 1) * spec.stride - spec.pad_l + (spec.ksize - 1) * spec.dilation - (l_in - 1)


def _walk(gen, audio_lengths: Sequence[int], rows: int):
    """Row lengths per resolution and, per entry of ``gen_layers.layers``, (layer, resolution of its input).  The first ``rows`` entries
    of ``audio_lengths`` are clips (checked against the layers' reflect pads), any further ones buffers."""
    m, n = gen.pqmf.decimation, gen.pqmf.kernel_size
    levels = [tuple(audio_lengths), tuple((t + n - 2) // m + 1 for t in audio_lengths)]
    cur, steps = 1, []
    for layer in layers(gen):
        path, spec, lens = layer.path, layer.spec, levels[cur]
        if spec.reflect:
            for r in range(rows):
                if max(spec.pad_l, spec.pad_r) >= lens[r]:
                    raise ValueError(f"clip {r} ({audio_lengths[r]} samples after cut_to_valid_length) is too short: {path} reflect-pads "
                                     f"{max(spec.pad_l, spec.pad_r)} onto a row of {lens[r]}")
        steps.append((layer, cur))
        out = tuple(spec.out_len(l) for l in lens)
        if out != lens:
            if out not in levels:
                levels.append(out)
            cur = levels.index(out)
    if cur != 1:
        raise ValueError("the generator's decoder does not return to the resolution of the bands")
    return levels, steps


def plan(gen, lengths: Sequence[int]) -> RaggedPlan:
    """The ragged batch of clips of ``lengths`` samples through ``gen``.  Raises ``ValueError`` naming the clip whose own forward the
    generator would refuse (a reflect pad not smaller than the row: fewer than four latent frames)."""
    lengths = tuple(int(t) for t in lengths)
    if not lengths:
        raise ValueError("no clips")
    cut = tuple(cut_length(gen, t) for t in lengths)
    for r, t in enumerate(cut):
        if t <= 0:
            raise ValueError(f"clip {r} ({lengths[r]} samples) is too short: nothing is left after cut_to_valid_length")
    rows = len(cut)
    levels, steps = _walk(gen, cut, rows)
    if len(set(cut)) == 1:   # today's batched forward
        return RaggedPlan(lengths, cut, cut[0], 0, tuple(lv[0] for lv in levels), tuple(levels), ())
    m, n = gen.pqmf.decimation, gen.pqmf.kernel_size
    # the analysis bank (zero pad n - 1, stride m): the row's last band sample reads the audio up to (L0 - 1) m
    fills = [Fill("pqmf.analysis", ZERO_ALL, max((l0 - 1) * m - (t - 1) for t, l0 in zip(cut, levels[1])), 0)]
    for layer, lv in steps:
        count = max(reach(layer.spec, l) for l in set(levels[lv]))
        if count > 0:
            fills.append(Fill(layer.path, MIRROR if layer.spec.reflect else ZERO, count, lv))
    # The synthesis bank: a row's own samples read no frame past its last one (the transposed form's reach is 0), but the n samples behind
    # its end do; one filter span of zeroed frames, n / m, keeps those the bank's own tail and junk-free.  The bands are an output, so
    # all of their slack is zeroed.
    fills.append(Fill("pqmf.synthesis", ZERO_ALL, n // m, 1))
    fills.append(Fill("enhanced", ZERO_ALL, n, 0))   # behind the synthesis: the bank's tail of n samples behind each row, zeroed like the rest
    # the largest reach in audio samples, rounded up to whole latent frames
    rate = [1] + [m * (levels[1][0] // lv[0]) for lv in levels[1:]]
    need = max(f.count * rate[f.level] for f in fills)
    margin = -(-need // gen.multiple) * gen.multiple
    l_buf = max(cut) + margin
    full, _ = _walk(gen, cut + (l_buf,), rows)
    if len(full) != len(levels):
        raise ValueError("the padded buffer does not follow the rows' resolutions")
    for f in fills:
        if any(l + f.count > full[f.level][-1] for l in full[f.level][:-1]):
            raise ValueError(f"{f.layer}: a fill of {f.count} does not fit the margin of {margin} samples")
    return RaggedPlan(lengths, cut, l_buf, margin, tuple(lv[-1] for lv in full), tuple(lv[:-1] for lv in full), tuple(fills))


def compose_batches(gen, lengths: Sequence[int], max_batch_samples: int) -> Tuple[List[List[int]], List[int]]:
    """Deals clips into ragged batches of at most ``max_batch_samples`` buffer samples (rows x l_buf): sorted by cut length, filled
    greedily.  Returns (batches of clip indices, back) with ``back[i]`` the position of clip ``i`` in the concatenation of the batches.
    A clip longer than the budget is a batch of its own."""
    whole = plan(gen, lengths)   # refuses a clip that is too short by its index; the margin is the same for every ragged batch
    cut = whole.cut
    order = sorted(range(len(cut)), key=lambda i: (cut[i], i))
    batches: List[List[int]] = []
    for i in order:
        if batches:
            b = batches[-1]
            l_buf = cut[i] if cut[b[0]] == cut[i] else cut[i] + whole.margin
            if (len(b) + 1) * l_buf <= max_batch_samples:
                b.append(i)
                continue
        batches.append([i])
    back = [0] * len(cut)
    for pos, i in enumerate(i for b in batches for i in b):
        back[i] = pos
    return batches, back
