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

``disc_plan`` does the same for the four chains of ``DiscriminatorEBENMultiScales`` (the per-clip test losses of
``inference.evaluate_clips``): the discriminators read the generator's outputs where they lie, so ``loss_margin`` is the slack they
need there and ``plan`` / ``compose_batches`` take it as a least margin.
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


def plan(gen, lengths: Sequence[int], min_margin: int = 0) -> RaggedPlan:
    """The ragged batch of clips of ``lengths`` samples through ``gen``.  Raises ``ValueError`` naming the clip whose own forward the
    generator would refuse (a reflect pad not smaller than the row: fewer than four latent frames).  ``min_margin``: audio samples of
    slack that whoever reads the outputs needs behind every row (``loss_margin``); a ragged batch's margin is at least that."""
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
    need = max(max(f.count * rate[f.level] for f in fills), int(min_margin))
    margin = -(-need // gen.multiple) * gen.multiple
    l_buf = max(cut) + margin
    full, _ = _walk(gen, cut + (l_buf,), rows)
    if len(full) != len(levels):
        raise ValueError("the padded buffer does not follow the rows' resolutions")
    for f in fills:
        if any(l + f.count > full[f.level][-1] for l in full[f.level][:-1]):
            raise ValueError(f"{f.layer}: a fill of {f.count} does not fit the margin of {margin} samples")
    return RaggedPlan(lengths, cut, l_buf, margin, tuple(lv[-1] for lv in full), tuple(lv[:-1] for lv in full), tuple(fills))


def compose_batches(gen, lengths: Sequence[int], max_batch_samples: int, min_margin: int = 0) -> Tuple[List[List[int]], List[int]]:
    """Deals clips into ragged batches of at most ``max_batch_samples`` buffer samples (rows x l_buf): sorted by cut length, filled
    greedily.  Returns (batches of clip indices, back) with ``back[i]`` the position of clip ``i`` in the concatenation of the batches.
    A clip longer than the budget is a batch of its own.  ``min_margin`` as for ``plan``."""
    whole = plan(gen, lengths, min_margin)   # refuses a clip that is too short by its index; the margin is the same for every ragged batch
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


# ----------------------------------------------------------------------------------------------------------------------------------
# the discriminators (DiscriminatorEBENMultiScales): the same idea on the four chains, for the per-clip test losses
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DiscLayer:
    path: str                               # "pqmf_discriminators.2.discriminator.0", "melgan_discriminator.discriminator.4", ...
    fills: Tuple[Tuple[str, int], ...]      # (mode, count) in front of the layer, in the order they are written; empty: none
    in_lengths: Tuple[int, ...]             # every row's own input length ...
    out_lengths: Tuple[int, ...]            # ... and output length: the row's own conv arithmetic
    in_buffer: int                          # samples per row of the layer's input buffer ...
    out_buffer: int                         # ... and of its output


@dataclasses.dataclass(frozen=True)
class DiscPlan:
    cut: Tuple[int, ...]                    # the rows' lengths in audio samples
    band_lengths: Tuple[int, ...]           # and in band samples
    audio_l_buf: int                        # samples per row of the audio buffer
    bands_l_buf: int                        # and of the bands
    audio_margin: int                       # audio_l_buf - max(cut); 0 when all rows are equal
    bands_margin: int
    chains: Tuple[Tuple[DiscLayer, ...], ...]   # dilation 1, 2, 3, then MelGAN

    @property
    def ragged(self) -> bool:
        return self.audio_margin != 0

    def lengths(self, chain: int) -> Tuple[Tuple[int, ...], ...]:
        """[embedding][row] of a chain: its input, then behind each layer -- the valid extents of ``forward``'s embeddings."""
        layers_ = self.chains[chain]
        return (layers_[0].in_lengths,) + tuple(la.out_lengths for la in layers_)


def _disc_chains(disc):
    """Per chain (name, what it reads, [(path, reflection pad in front, ConvSpec)]) of a DiscriminatorEBENMultiScales."""
    def parts(prefix, net):
        out = []
        for i, module in enumerate(net.discriminator):
            spec = getattr(module, "spec", None)
            if spec is not None:
                out.append((f"{prefix}.discriminator.{i}", 0, spec))
                continue
            pad, conv = 0, None
            for j, sub in enumerate(module):
                if getattr(sub, "spec", None) is not None and conv is None:
                    conv = (f"{prefix}.discriminator.{i}.{j}", sub.spec)
                elif conv is None and isinstance(getattr(sub, "padding", None), int):
                    pad += sub.padding
                else:
                    raise ValueError(f"{prefix}.discriminator.{i}: not a reflection pad and a conv")
            if conv is None or conv[1].transposed or conv[1].reflect:
                raise ValueError(f"{prefix}.discriminator.{i}: not a zero-padded conv")
            out.append((conv[0], pad, conv[1]))
        return out

    chains = [(f"pqmf_discriminators.{i} (dilation {net.dilation})", "bands", parts(f"pqmf_discriminators.{i}", net))
              for i, net in enumerate(disc.pqmf_discriminators)]
    chains.append(("melgan_discriminator", "audio", parts("melgan_discriminator", disc.melgan_discriminator)))
    return chains


def _disc_out_len(pad: int, spec, l_in: int) -> int:
    """Output length of a layer, 0 when its own forward fails: the reflection pad needs more than ``pad`` samples, the conv an output."""
    if l_in <= pad:
        return 0
    return max(0, spec.out_len(l_in + 2 * pad))


def _chain_lengths(layers_, l_in: int):
    """[l_in, behind layer 0, ...], cut short at the first layer that yields nothing."""
    out = [l_in]
    for _, pad, spec in layers_:
        out.append(_disc_out_len(pad, spec, out[-1]))
        if out[-1] <= 0:
            break
    return out


def disc_shortest(disc, pqmf=None) -> dict:
    """The shortest rows ``disc``'s own batch-1 forward accepts: ``{"bands": band samples, "audio": audio samples, "chains": per chain
    its own limit at the rate of what it reads}`` and, with the generator's ``pqmf``, ``"cut"``: the shortest cut length -- band
    samples are (cut + n) / m of a bank of m bands and n taps, cut + n a multiple of 64 m."""
    limits = []
    for _, _, layers_ in _disc_chains(disc):
        lo = 1
        while len(_chain_lengths(layers_, lo)) <= len(layers_) or _chain_lengths(layers_, lo)[-1] <= 0:
            lo += 1   # lengths are monotone in the input's, and the limit is a few hundred samples
            if lo > 1 << 20:
                raise ValueError("a discriminator chain yields no output at any length")
        limits.append(lo)
    out = {"chains": tuple(limits), "bands": max(limits[:-1]), "audio": limits[-1]}
    if pqmf is not None:
        m, n, multiple = pqmf.decimation, pqmf.kernel_size, 64 * pqmf.decimation
        need = max(out["bands"] * m - n, out["audio"], 1)
        out["cut"] = -(-(need + n) // multiple) * multiple - n
    return out


def _disc_reach(pad: int, spec, l_in: int) -> int:
    """``reach`` of a conv behind a reflection pad of ``pad``, in samples of the unpadded input."""
    l_out = spec.out_len(l_in + 2 * pad)
    return (l_out - 1) * spec.stride - spec.pad_l - pad + (spec.ksize - 1) * spec.dilation - (l_in - 1)


def _chain_margin(layers_) -> int:
    """Samples of slack a chain needs behind a row of its input: a layer's last output reads at most its padding past the row, so the
    largest padding x stride product in front, in whole steps of the chain's total stride (every level's buffer then ends a whole
    number of that level's samples behind every row)."""
    rate, worst = 1, 0
    for _, pad, spec in layers_:
        worst = max(worst, (pad + spec.pad_r) * rate)
        rate *= spec.stride
    return -(-worst // rate) * rate


def loss_margin(disc, decimation: int, freq_loss=None) -> int:
    """Audio samples of slack the per-clip losses need behind every row of a ragged batch (``plan``'s ``min_margin``): a layer's last
    output reads at most its padding past the row, so per chain the largest padding x stride product in front, in whole steps of the
    chain's total stride (the stride-4 k41 conv at 1/64 of the audio rate reads 20 frames: 1280 samples) -- the band chains' times the
    bank's decimation -- and the largest reflect pad of ``freq_loss``'s resolutions."""
    need = 0
    for _, reads, layers_ in (_disc_chains(disc) if disc is not None else ()):
        need = max(need, _chain_margin(layers_) * (decimation if reads == "bands" else 1))
    if freq_loss is not None:
        need = max(need, max(n_fft // 2 - (n_fft - win) // 2 for n_fft, win in zip(freq_loss.fft_sizes, freq_loss.win_lengths)))
    return need


def disc_plan(discriminator, cut_lengths: Sequence[int], band_lengths: Sequence[int], audio_l_buf: int = None,
              bands_l_buf: int = None) -> DiscPlan:
    """The ragged batch of rows of ``cut_lengths`` audio samples and ``band_lengths`` band samples through the four chains of a
    ``DiscriminatorEBENMultiScales``: per chain and layer every row's own output length and the fills in front of the layer.  A
    reflection pad followed by a zero-padded conv (the band chains' first layer: ``ReflectionPad1d(1)``, then padding 1) needs
    ``x[len] = x[len - 2]`` and ``x[len + 1] = 0`` behind a row -- two fills, zero over the whole reach, then the mirror over its
    first samples.  The buffers are the generator's (``audio_l_buf``, ``bands_l_buf``: samples per row; default the longest row plus
    this plan's own margin); every fill must fit them at every level.  Raises ``ValueError`` naming the row whose own batch-1
    forward the discriminator would refuse, and the chain that refuses it."""
    cut, bands = tuple(int(t) for t in cut_lengths), tuple(int(t) for t in band_lengths)
    if not cut or len(cut) != len(bands):
        raise ValueError(f"disc_plan: {len(cut)} audio lengths and {len(bands)} band lengths")
    chains = _disc_chains(discriminator)
    limits = disc_shortest(discriminator)["chains"]
    for r in range(len(cut)):
        for (name, reads, _), limit in zip(chains, limits):
            have = bands[r] if reads == "bands" else cut[r]
            if have < limit:
                raise ValueError(f"clip {r} ({cut[r]} samples after cut_to_valid_length, {bands[r]} band samples) is too short: {name} "
                                 f"needs {limit} {reads} samples")
    equal = len(set(cut)) == 1 and len(set(bands)) == 1   # today's batched forward, unless the buffers are wider than the rows
    if audio_l_buf is None:
        audio_l_buf = max(cut) + (0 if equal else max(_chain_margin(la) for _, reads, la in chains if reads == "audio"))
    if bands_l_buf is None:
        bands_l_buf = max(bands) + (0 if equal else max(_chain_margin(la) for _, reads, la in chains if reads == "bands"))
    if audio_l_buf < max(cut) or bands_l_buf < max(bands):
        raise ValueError(f"disc_plan: buffers of {audio_l_buf} / {bands_l_buf} samples for rows of up to {max(cut)} / {max(bands)}")
    equal = equal and audio_l_buf == cut[0] and bands_l_buf == bands[0]
    out = []
    for name, reads, layers_ in chains:
        lens, buf = (bands, bands_l_buf) if reads == "bands" else (cut, audio_l_buf)
        chain = []
        for path, pad, spec in layers_:
            nxt, nxt_buf = tuple(_disc_out_len(pad, spec, l) for l in lens), _disc_out_len(pad, spec, buf)
            fills = ()
            if not equal:
                count = max(_disc_reach(pad, spec, l) for l in set(lens))
                if count > 0:
                    fills = ((ZERO, count),) * (count > pad) + ((MIRROR, min(pad, count)),) * (pad > 0)
                for mode, c in fills:
                    for r, l in enumerate(lens):
                        if l + c > buf or (mode == MIRROR and c > l - 1):
                            raise ValueError(f"{path}: a {mode} fill of {c} behind row {r} ({l} samples) does not fit a buffer of {buf}")
            chain.append(DiscLayer(path, fills, lens, nxt, buf, nxt_buf))
            lens, buf = nxt, nxt_buf
        out.append(tuple(chain))
    return DiscPlan(cut, bands, audio_l_buf, bands_l_buf, audio_l_buf - max(cut), bands_l_buf - max(bands), tuple(out))
