"""The multi-resolution STFT loss over libeben_hip.so: plans, the windowed-DFT contractions, one autograd function over two term sets
and the per-row sums of ragged buffers (kernels: csrc/stft.hip, stft_terms.hip, pw_gemm.hip, ragged_losses.hip).

Per resolution: ``eben_stft_frames`` writes the reflect-padded frames of ALL signals (x and y rows) as one (win, R*frames) matrix, the
windowed DFT is one dense GEMM over it (pointwise tap-conv, batch 1 -- a strided conv per item would pad every item's 134 / 267 frames
to whole 128-column tiles), the loss sums read the flat (2*bins, R*frames) spectrum through strides; backward: d(spec) in the same flat
form, d(frames) = basis^T . d(spec) as one GEMM, overlap-add back onto the waveform.  ``plan.math`` "folded" / "bf16x3" (even window
lengths): the frames are written as their even and odd parts about the window centre and the GEMMs become 2-group contractions over
win/2 channels (``StftPlan.parts``)."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from . import ops
from ._lib import check, load, ptr, stream
from .ops import MATH_BF16, MATH_BF16X3, MATH_BF16X6, MATH_F32, ConvSpec, PackedWeights, _empty, _fir_decimate, _fir_interp_sum, _iptr, conv_desc, pack_weights

#: StftPlan.math -> EBEN_MATH_* of the folded windowed-DFT contractions ("bf16x3": single bf16 operands over the concatenated
#: [hi ; lo ; hi] x [W_hi ; W_hi ; W_lo] reduction; "folded_x3" / "folded_x6": the tap-conv's own split operands, tapconv3.hip)
_STFT_CONV_MATH = {"bf16x3": MATH_BF16, "folded_x3": MATH_BF16X3, "folded_x6": MATH_BF16X6}

#: the folded windowed-DFT contractions on the grouped GEMM kernel (pw_gemm.hip) instead of the pointwise tap-conv
STFT_GEMM = os.environ.get("EBEN_STFT_GEMM", "1") != "0"


@dataclass
class Contraction:
    """One direction of one math's windowed DFT: a pointwise conv ``spec`` with weights ``basis`` (c_out, c_in / groups, 1)."""
    spec: ConvSpec
    basis: torch.Tensor
    cache: PackedWeights = field(default_factory=PackedWeights)
    image: Optional[torch.Tensor] = None   # the basis packed for eben_gemm_fwd, built on first use -- the bases are constants

    @classmethod
    def of(cls, basis: torch.Tensor, groups: int) -> "Contraction":
        return cls(ConvSpec(c_in=groups * basis.shape[1], c_out=basis.shape[0], ksize=1, groups=groups), basis)


@dataclass
class StftPlan:
    n_fft: int
    hop: int
    win: int
    bins: int
    pad: int
    basis_f: torch.Tensor  # (2*bins, win, 1) windowed DFT rows: [cos ; -sin]
    basis_t: torch.Tensor  # (win, 2*bins, 1) = basis transposed
    #: the window's float32 sample 0 is exactly 0 and w[h + m] == w[h - m] (hann, blackman, bartlett): the folded forms drop sample 0
    #: and read only the right half of the basis, so hamming or kaiser (w[0] != 0) take "dense"
    foldable: bool = True
    #: mel projection of the magnitudes (eben_stft_terms_fwd / _bwd): (n_mels, fb_lo, fb_off, fb_w, bin_m, bin_w), or None
    mel: Optional[tuple] = None
    #: "dense": one (2*bins x win) GEMM per resolution; "folded": even / odd parts of the frames, two groups of win/2
    #: channels (half the products, exact fp32); "bf16x3": the folded form with hi / lo bf16 operand splits on the bf16 MFMA
    math: str = "folded"
    contractions: dict = field(default_factory=dict)   # math -> (forward, adjoint) Contraction, built on first use

    @classmethod
    def build(cls, n_fft: int, hop: int, win: int, basis_f: torch.Tensor, basis_t: torch.Tensor, foldable: bool = True,
              mel: Optional[tuple] = None) -> "StftPlan":
        # the window centred in n_fft (torch.stft puts it (n_fft - win)//2 samples into the frame) + center=True reflect
        # padding of n_fft//2 == frames of length `win` taken at reflect padding n_fft//2 - (n_fft - win)//2 (the window is
        # zero outside its `win` samples); win/2 when n_fft and win are both even
        return cls(n_fft=n_fft, hop=hop, win=win, bins=n_fft // 2 + 1, pad=n_fft // 2 - (n_fft - win) // 2, basis_f=basis_f, basis_t=basis_t,
                   foldable=foldable, mel=mel)

    def frames(self, t: int) -> int:
        """Frames of a length-t signal: torch.stft(center=True) pads n_fft // 2 on each side and steps an n_fft window by hop."""
        return (t + 2 * (self.n_fft // 2) - self.n_fft) // self.hop + 1

    def math_for(self, math: str) -> str:
        """The arithmetic a plan runs: the folded forms need the window's centre h = win / 2 on the DFT's symmetry point n_fft / 2
        (win and n_fft even, frames at reflect padding win / 2) and a window they can fold (``foldable``); every other plan takes
        "dense"."""
        return math if self.foldable and self.win % 2 == 0 and self.n_fft % 2 == 0 and self.pad == self.win // 2 else "dense"

    def parts(self, math: str):
        """(forward, adjoint) contractions of ``math``.  "dense": (win -> 2*bins) and its transpose.  Folded
        (eben_stft_frames_folded): forward, 2 groups x (nsub*h -> bins) with rows basis[:, h:] (x [W_hi, W_hi, W_lo] for bf16x3);
        adjoint, 2 groups x (nsub*bins -> h), its transpose."""
        parts = self.contractions.get(math)
        if parts is None:
            if math == "dense":
                parts = (Contraction.of(self.basis_f, 1), Contraction.of(self.basis_t, 1))
            else:
                h, bins = self.win // 2, self.bins
                w = self.basis_f[:, h:, 0].contiguous()                       # (2*bins, h)
                wt = w.reshape(2, bins, h).transpose(1, 2).contiguous()       # (2, h, bins): group g, output row m, reduction k
                nsub = 1
                if math == "bf16x3":
                    def split(a, dim):
                        hi = a.to(torch.bfloat16).to(torch.float32)
                        lo = (a - hi).to(torch.bfloat16).to(torch.float32)
                        return torch.cat((hi, hi, lo), dim=dim)
                    w, wt, nsub = split(w, 1), split(wt, 2), 3
                parts = (Contraction.of(w.unsqueeze(-1).contiguous(), 2), Contraction.of(wt.reshape(2 * h, nsub * bins, 1).contiguous(), 2))
            self.contractions[math] = parts
        return parts

    def folded_parts(self, math: str):
        """``parts(math)`` laid out flat, (spec_f, basis_f, spec_t, basis_t, cache_fwd, cache_bwd): what the tests unpack."""
        f, t = self.parts(math)
        return f.spec, f.basis, t.spec, t.basis, f.cache, t.cache

    def dft(self, math: str, fr: torch.Tensor, cols: int) -> torch.Tensor:
        """(1, 2*bins, cols) windowed DFT of a frame matrix: fr is (1, win, cols) from eben_stft_frames for "dense", else the
        (1, c_in, cols) parts from eben_stft_frames_folded (split for "bf16x3")."""
        return _contract(self, math, 0, fr, cols)

    def dft_t(self, math: str, dspec: torch.Tensor, cols: int) -> torch.Tensor:
        """The adjoint of ``dft``: (1, 2*bins, cols) -> (1, win, cols) frame gradients ("dense") or the (1, 2*(win/2), cols) [dE ; dO]
        parts eben_overlap_add_folded takes."""
        return _contract(self, math, 1, dspec, cols)


def _contract(p: StftPlan, math: str, which: int, x: torch.Tensor, cols: int) -> torch.Tensor:
    """x (1, c_in, cols) through the forward (which 0) or adjoint (1) contraction of ``math``: (1, c_out, cols)."""
    lib, st = load(), stream()
    c = p.parts(math)[which]
    cmath = _STFT_CONV_MATH.get(math, MATH_F32)
    what = ("stft_fwd", "stft_bwd_gemm")[which]
    if which == 1 and math == "bf16x3":
        split = torch.empty((1, c.spec.c_in, cols), dtype=torch.float32, device=x.device)
        check(lib.eben_split3(ptr(x), ptr(split), 2, p.bins, cols, st), "split3")
        x = split
    out = torch.empty((1, c.spec.c_out, cols), dtype=torch.float32, device=x.device)
    if STFT_GEMM and math in ("folded_x3", "folded_x6"):
        # the folded contraction as what it is, a 2-group GEMM (pw_gemm.hip): no input tile, no staging pass per row tile
        m, k = c.spec.c_out // 2, c.spec.c_in // 2
        if c.image is None:
            c.image = torch.empty(lib.eben_gemm_packed_floats(cmath, 2, m, k), dtype=torch.float32, device=x.device)
            check(lib.eben_gemm_pack(cmath, 2, m, k, ptr(c.basis), ptr(c.image), st), "gemm_pack")
        check(lib.eben_gemm_fwd(cmath, 2, m, k, cols, ptr(x), ptr(c.image), ptr(out), st), what)
    else:
        d = conv_desc(c.spec, 1, cols, cmath)
        pw = pack_weights(c.spec, d, c.basis, None, c.cache, False)
        check(lib.eben_conv1d_fwd(ctypes.byref(d), ptr(x), ptr(pw.wp_fwd), None, None, ptr(out), st), what)
    return out


def _stft_spectrum(p: StftPlan, math: str, sig: torch.Tensor, t: int, frames: int) -> torch.Tensor:
    """(1, 2*bins, R*frames) windowed DFT of every row of sig (R, 1, t): eben_stft_frames ("dense") or eben_stft_frames_folded, then
    the plan's contraction."""
    lib, st = load(), stream()
    nrows = sig.shape[0]
    cols = nrows * frames
    if math == "dense":
        fr = torch.empty((1, p.win, cols), dtype=torch.float32, device=sig.device)
        check(lib.eben_stft_frames(ptr(sig), ptr(fr), nrows, t, p.win, p.hop, p.pad, frames, st), "stft_frames")
    else:
        fr = torch.empty((1, p.parts(math)[0].spec.c_in, cols), dtype=torch.float32, device=sig.device)
        check(lib.eben_stft_frames_folded(ptr(sig), ptr(fr), nrows, t, p.win, p.hop, p.pad, frames, 1 if math == "bf16x3" else 0, st),
              "stft_frames_folded")
    return p.dft(math, fr, cols)


def _stft_spectrum_adjoint(p: StftPlan, math: str, dspec: torch.Tensor, dsig: torch.Tensor, t: int, frames: int, accumulate: bool) -> None:
    """dsig (R, 1, t) (+)= the adjoint of ``_stft_spectrum`` applied to dspec (1, 2*bins, R*frames)."""
    lib, st = load(), stream()
    rows = dsig.shape[0]
    xcols = rows * frames
    # d(frames)[j, (r, f)] = sum_m basis[m, j] dspec[m, (r, f)]: one dense GEMM, then overlap-add
    dfr = p.dft_t(math, dspec, xcols)
    if math == "dense":
        check(lib.eben_overlap_add_ex(ptr(dfr), ptr(dsig), rows, t, p.win, frames, p.hop, p.pad, 1, 1 if accumulate else 0, frames, xcols, st),
              "overlap_add")
    else:
        check(lib.eben_overlap_add_folded(ptr(dfr), ptr(dsig), rows, t, p.win, frames, p.hop, p.pad, 1 if accumulate else 0, frames, xcols, st),
              "overlap_add_folded")


def _stacked_rows(x: torch.Tensor, y: torch.Tensor, fir: Optional[torch.Tensor]) -> torch.Tensor:
    """(2 rows, 1, t): the rows of x, then those of y, through the A-weighting FIR when there is one."""
    t = x.shape[-1]
    sig = torch.cat((x.reshape(-1, 1, t), y.reshape(-1, 1, t)), dim=0)
    if fir is not None:
        nt = fir.numel()
        sig = _fir_decimate(sig, fir, t, 1, nt, 1, -(nt // 2))
    return sig


class _YamlTerms:
    """The term set of multi_stft.yaml: spectral convergence + log-magnitude L1 on the linear scale (stft.hip)."""

    def sums(self, p: StftPlan, spec, rows: int, frames: int, eps: float):
        lib, cols = load(), 2 * rows * frames
        sums = torch.empty((rows, 3), dtype=torch.float32, device=spec.device)
        ws_bytes = lib.eben_stft_loss_sums_workspace(rows)
        # y rows: same strides, column offset rows*frames
        check(lib.eben_stft_loss_sums_ex(ptr(spec), ptr(spec) + 4 * rows * frames, rows, p.bins, frames, frames, cols, p.bins * cols, eps,
                                         ptr(_empty(ws_bytes, spec)), ws_bytes, ptr(sums), stream()), "stft_loss_sums")
        return (sums,)

    def total(self, plans, saved, rows: int):
        n = len(plans)
        if n <= 8 and ops.FUSED_LOSS_GLUE:   # the value from the per-row sums of all resolutions: one launch instead of ~8 one-element torch kernels per resolution
            total = torch.empty((), dtype=torch.float32, device=saved[0][0].device)
            check(load().eben_stft_loss_total((ctypes.c_void_p * n)(*[ptr(sv[1]) for sv in saved]),
                                              (ctypes.c_float * n)(*[1.0 / float(rows * p.bins * sv[2]) for p, sv in zip(plans, saved)]), n, rows,
                                              ptr(total), stream()), "stft_loss_total")
            return total
        total = None
        for p, (_, sums, frames, _) in zip(plans, saved):
            term = torch.sqrt(sums[:, 0] / sums[:, 1]).mean() + sums[:, 2].sum() / float(rows * p.bins * frames)
            total = term if total is None else total + term
        return total / n

    def dspec(self, p: StftPlan, sv, rows: int, eps: float, gout, scale: float):
        spec, sums, frames = sv[:3]
        cols, xcols = 2 * rows * frames, rows * frames
        dspec = torch.empty((1, 2 * p.bins, xcols), dtype=torch.float32, device=gout.device)
        check(load().eben_stft_loss_bwd_ex(ptr(spec), ptr(spec) + 4 * xcols, rows, p.bins, frames, frames, cols, p.bins * cols, eps, ptr(sums),
                                           ptr(gout), scale, ptr(dspec), frames, xcols, p.bins * xcols, stream()), "stft_loss_bwd")
        return dspec


#: eben_stft_terms_* term mask bits
STFT_TERM_SC, STFT_TERM_LOG, STFT_TERM_LIN = 1, 2, 4


class _WeightedTerms:
    """Every other term set: the weighted SC / log / lin terms under L1 or L2, on an optional mel projection per plan
    (``StftPlan.mel``; stft_terms.hip)."""

    def __init__(self, weights: Sequence[float], l2: bool):
        self.weights = w_sc, w_log, w_lin = tuple(float(w) for w in weights)
        self.mask = (STFT_TERM_SC if w_sc else 0) | (STFT_TERM_LOG if w_log else 0) | (STFT_TERM_LIN if w_lin else 0)
        self.l2 = int(l2)

    def sums(self, p: StftPlan, spec, rows: int, frames: int, eps: float):
        lib = load()
        sums = torch.empty((rows, 4), dtype=torch.float32, device=spec.device)
        if p.mel is not None:
            n_out, fb_lo, fb_off, fb_w = p.mel[:4]
            mags = torch.empty((2, rows, n_out, frames), dtype=torch.float32, device=spec.device)
            mel_ptrs = (_iptr(fb_lo), _iptr(fb_off), ptr(fb_w))
        else:
            n_out, mags, mel_ptrs = p.bins, None, (None, None, None)
        ws_bytes = lib.eben_stft_terms_workspace(rows)
        check(lib.eben_stft_terms_fwd(ptr(spec), rows, p.bins, frames, eps, n_out, *mel_ptrs, self.mask, self.l2, ptr(mags),
                                      ptr(_empty(ws_bytes, spec)), ws_bytes, ptr(sums), stream()), "stft_terms_fwd")
        return sums, mags

    def total(self, plans, saved, rows: int):
        n = len(plans)
        inv_counts = [1.0 / float(rows * (p.bins if p.mel is None else p.mel[0]) * sv[2]) for p, sv in zip(plans, saved)]
        total = torch.empty((), dtype=torch.float32, device=saved[0][0].device)
        check(load().eben_stft_terms_total((ctypes.c_void_p * n)(*[ptr(sv[1]) for sv in saved]), (ctypes.c_float * n)(*inv_counts), n, rows,
                                           self.mask, *self.weights, ptr(total), stream()), "stft_terms_total")
        return total

    def dspec(self, p: StftPlan, sv, rows: int, eps: float, gout, scale: float):
        spec, sums, frames, _, mags = sv
        dspec = torch.empty((1, 2 * p.bins, rows * frames), dtype=torch.float32, device=gout.device)
        if p.mel is not None:
            n_out, bin_m, bin_w = p.mel[0], p.mel[4], p.mel[5]
            adj = (_iptr(bin_m), ptr(bin_w), ptr(mags))
        else:
            n_out, adj = p.bins, (None, None, None)
        check(load().eben_stft_terms_bwd(ptr(spec), rows, p.bins, frames, eps, n_out, *adj, self.mask, self.l2, *self.weights, ptr(sums),
                                         ptr(gout), scale, ptr(dspec), stream()), "stft_terms_bwd")
        return dspec


class _MRSTFTFn(torch.autograd.Function):
    """auraloss MultiResolutionSTFTLoss(x, y) (see mrstft_loss.py).  Framing, windowed DFT, its adjoint, the overlap-add and the FIR are
    the same for every configuration; ``terms`` (_YamlTerms or _WeightedTerms) supplies the per-plan sums, the total and d(spec).
    ``ctx.saved``: per plan (spec, sums, frames, math[, mags])."""

    @staticmethod
    def forward(ctx, x, y, fir, plans: List[StftPlan], eps: float, terms):
        x, y = x.contiguous(), y.contiguous()
        b, c, t = x.shape
        rows = b * c
        sig = _stacked_rows(x, y, fir)
        saved = []
        for p in plans:
            frames = p.frames(t)
            math = p.math_for(p.math)
            spec = _stft_spectrum(p, math, sig, t, frames)
            sums, *kept = terms.sums(p, spec, rows, frames, eps)
            saved.append((spec, sums, frames, math, *kept))
        ctx.plans, ctx.eps, ctx.geom, ctx.saved, ctx.fir, ctx.terms = plans, eps, (b, c, t, rows), saved, fir, terms
        return terms.total(plans, saved, rows)

    @staticmethod
    def backward(ctx, gout):
        b, c, t, rows = ctx.geom
        gout = gout.contiguous().reshape(1)
        dsig = torch.empty((rows, 1, t), dtype=torch.float32, device=gout.device)
        for i, (p, sv) in enumerate(zip(ctx.plans, ctx.saved)):
            dspec = ctx.terms.dspec(p, sv, rows, ctx.eps, gout, 1.0 / len(ctx.plans))
            _stft_spectrum_adjoint(p, sv[3], dspec, dsig, t, sv[2], i > 0)
        if ctx.fir is not None:
            nt = ctx.fir.numel()
            dsig = _fir_interp_sum(dsig, ctx.fir, t, 1, nt, 1, -(nt // 2))
        return dsig.reshape(b, c, t), None, None, None, None, None


def mrstft(x: torch.Tensor, y: torch.Tensor, fir: Optional[torch.Tensor], plans: List[StftPlan], eps: float = 1e-8) -> torch.Tensor:
    """MultiResolutionSTFTLoss as configured by multi_stft.yaml."""
    return _MRSTFTFn.apply(x, y.detach(), fir, plans, eps, _YamlTerms())


def mrstft_terms(x: torch.Tensor, y: torch.Tensor, fir: Optional[torch.Tensor], plans: List[StftPlan], eps: float, weights: Sequence[float],
                 l2: bool) -> torch.Tensor:
    """MultiResolutionSTFTLoss with weights (w_sc, w_log_mag, w_lin_mag), mag_distance L2 (l2) or L1 and the plans' windows and mel
    projections (eben_stft_terms_*); at least one weight non-zero, at most 16 resolutions."""
    return _MRSTFTFn.apply(x, y.detach(), fir, plans, eps, _WeightedTerms(weights, l2))


#: called with the (2 rows, 1, l_buf) A-weighted signal of ``mrstft_sums_rows`` and its row lengths, in front of the mirror fill (tests
#: write garbage behind the rows there: nothing of it may reach a result)
mrstft_rows_probe = None


def mrstft_sums_rows(x: torch.Tensor, y: torch.Tensor, lens2: torch.Tensor, frames_of_row, fir: Optional[torch.Tensor], plans: List[StftPlan],
                     eps: float, fill: int) -> List[torch.Tensor]:
    """Per plan the (rows, 3) sums of ``_YamlTerms.sums`` with every row on its own frames: x and y (rows, 1, l_buf), zero behind each
    row; ``lens2`` (2 rows,) int32 on the device, the row lengths twice; ``frames_of_row[i]`` (rows,) int32, plan i's frames of each row.
    The FIR's zero padding finds the zeros behind a row, one mirror fill of ``fill`` samples (the largest reflect pad; 0: rows as long
    as the buffer) stands for every plan's reflect padding, then framing and contraction run on the whole buffer."""
    lib, st = load(), stream()
    rows, _, t = x.shape
    sig = _stacked_rows(x, y, fir)
    if mrstft_rows_probe is not None:
        mrstft_rows_probe(sig, lens2)
    if fill:
        ops.edge_fill(sig, lens2, ops.FILL_MIRROR, fill)
    out = []
    for p, fr in zip(plans, frames_of_row):
        frames = p.frames(t)
        cols = 2 * rows * frames
        spec = _stft_spectrum(p, p.math_for(p.math), sig, t, frames)
        sums = torch.empty((rows, 3), dtype=torch.float32, device=x.device)
        ws_bytes = lib.eben_stft_loss_sums_rows_workspace(rows)
        check(lib.eben_stft_loss_sums_rows(ptr(spec), ptr(spec) + 4 * rows * frames, rows, p.bins, frames, _iptr(fr), frames, cols, p.bins * cols, eps,
                                           ptr(_empty(ws_bytes, x)), ws_bytes, ptr(sums), st), "stft_loss_sums_rows")
        out.append(sums)
    return out
