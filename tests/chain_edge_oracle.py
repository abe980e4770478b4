"""Float64 restatements of the two ends of the bundle-layout discriminator chains -- the fp32 <-> plane conversions, the chain heads
(ReflectionPad1d + grouped Conv1d + bias + LeakyReLU: forward, input gradient, weight gradient) and the chain tails (the logits layer
C -> 1: forward, input gradient with the feature-matching term and the LeakyReLU mask, weight gradient) -- written from the formulas in
include/eben_hip.h ("Chain heads", "Chain tails", eben_bl_from_f32), independent of the library (torch only; every function works on CPU
and device tensors).  The convolutions are spelt out as index gathers: tests/test_chain_edge_oracle.py holds them against torch's own
conv / conv_transpose / reflect pad under autograd.

Error bounds (U = 2^-24, the fp32 unit roundoff; u_b = 2^-8, the bf16 one; the comparison helpers are those of step_tail_oracle.py).
  * An fp32 value formed from n accumulated products:  (n + c) U sum|terms|, the sum taken in float64 over the magnitudes ENTERING the
    operations (|w| against |x|, |bias|, the feature-matching coefficients), c = the roundings that are no accumulation step (the
    weight-norm scale, the bias, the LeakyReLU slope, the coefficient divisions); written at each function.  Every kernel sums in a tree
    or in chains far shorter than n, so the second-order terms of the usual gamma_n = n U / (1 - n U) stay inside.
  * A value stored as planes hi = bf16(v), lo = bf16(v - hi):  v - hi is exact in fp32 and |v - hi| <= u_b |v|, lo rounds it once more,
    so |hi + lo - v| <= u_b^2 |v| = 2^-16 |v| (plus the bf16 denormal quantum 2^-133 where lo underflows); hi alone lies within u_b |v|.
    `plane_bound` adds that to the value's own bound, with |v| <= |ref| + bound.
  * A plane pair is a split at all only if |lo| <= half a bf16 ulp of hi: `split_violations`.
  * Weight-gradient slabs are summed over the slices in float64 by the caller; a column is then bounded by d U sum|g x| with d the longest
    chain of fp32 additions one sum passes through: the fused multiply-adds of one thread, six wave steps, three block steps
    (`head_dw_depth`, `tail_dw_depth`, read off the kernels' loops for the slice size at hand).
"""
import torch

from tests.step_tail_oracle import U, bound_violation, pattern_mismatches, sgn, worst_error  # noqa: F401  (re-exported to the tests)

UB = 2.0 ** -8             # bf16 unit roundoff (8 significant bits, round to nearest even)
BF16_TINY = 2.0 ** -133    # the smallest bf16 denormal


def f64(t):
    return t.detach().to(torch.float64)


# ---- planes ------------------------------------------------------------------------------------------------------------------------
def bf16_rne(v):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32: integer arithmetic on the bit pattern (finite inputs)."""
    bits = v.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32).reshape(v.shape)


def split(v):
    """(hi, lo) = (bf16(v), bf16(v - hi)) as fp32 tensors; v - hi is exact in fp32 (hi shares v's leading 8 bits or is the next power of two)."""
    v = v.detach().to(torch.float32)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)


def join(hi, lo=None):
    """fp32(hi + lo): ONE fp32 addition, as every kernel that reads both planes forms its operand."""
    hi = hi.detach().to(torch.float32)
    return hi if lo is None else hi + lo.detach().to(torch.float32)


def to_bundles(x):
    """(B, C, L) -> the bundle layout (B, C / 8, L, 8)."""
    b, c, l = x.shape
    return x.reshape(b, c // 8, 8, l).permute(0, 1, 3, 2).contiguous()


def from_bundles(p):
    """(B, C / 8, L, 8) -> (B, C, L)."""
    b, cb, l, _ = p.shape
    return p.permute(0, 1, 3, 2).reshape(b, cb * 8, l)


def split_violations(hi, lo):
    """Elements whose lo is more than half a bf16 ulp of hi (ulp(hi) = 2^(e - 7), e = hi's exponent; the denormal quantum below the
    normal range).  hi = 0 admits lo = 0 only."""
    hi, lo = f64(hi).abs(), f64(lo).abs()
    e = torch.floor(torch.log2(hi.clamp_min(2.0 ** -126)))
    half_ulp = torch.where(hi > 0, torch.exp2(e - 8), torch.zeros_like(hi))
    return int((lo > half_ulp).sum())


def plane_bound(ref, value_bound, lo=True):
    """Absolute bound of hi + lo (lo=True) or hi alone against `ref` when the fp32 value the planes were split from lies within
    `value_bound` of it."""
    mag = f64(ref).abs() + value_bound
    return value_bound + (UB * UB * mag + BF16_TINY if lo else UB * mag + BF16_TINY)


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


# ---- chain heads -------------------------------------------------------------------------------------------------------------------
def head_index(l_in, l_out, k, dil, pad, rpad, device=None):
    """For every (output position t, tap j): the row index read and whether anything is read at all.  Position p = t - pad + j dil of
    the reflect-padded row (length l_in + 2 rpad), zero outside it; inside, u = |p - rpad| folded back at the far end."""
    t = torch.arange(l_out, device=device)[:, None]
    j = torch.arange(k, device=device)[None, :]
    p = t - pad + j * dil
    live = (p >= 0) & (p < l_in + 2 * rpad)
    u = (p - rpad).abs()
    u = torch.where(u >= l_in, 2 * (l_in - 1) - u, u)
    return u.clamp(0, l_in - 1), live


def head_l_out(l_in, k, dil, pad, rpad):
    return l_in + 2 * rpad + 2 * pad - dil * (k - 1)


def _head_gather(x, c_out, k, dil, pad, rpad):
    """x (B, c_in, l_in) -> the operand of every product, (B, c_out, l_out, k); output channel co reads input channel co / (c_out / c_in)."""
    x = f64(x)
    _, c_in, l_in = x.shape
    l_out = head_l_out(l_in, k, dil, pad, rpad)
    u, live = head_index(l_in, l_out, k, dil, pad, rpad, x.device)
    xg = x[:, :, u] * live.to(torch.float64)                         # (B, c_in, l_out, k)
    return xg.repeat_interleave(c_out // c_in, dim=1)


HEAD_FWD_C = 3   # the scale, the bias, the LeakyReLU slope


def head_fwd(x, v, scale, bias, dil, pad, rpad, slope):
    """(y, mag): y = lrelu((sum_j v[co, j] xp[ci, t - pad + j dil]) scale[co] + bias[co]); the layer is linear in v, the scale is applied
    once per channel to the finished sum.  k fused multiply-adds, then scale, bias and slope:  (k + 3) U mag,
    mag = |scale| sum_j |v| |x| + |bias|.                                                                             n = k, c = 3"""
    v = f64(v)
    c_out, _, k = v.shape
    xg = _head_gather(x, c_out, k, dil, pad, rpad)
    w = v.reshape(1, c_out, 1, k)
    sc = f64(scale).reshape(1, c_out, 1) if scale is not None else 1.0
    bs = f64(bias).reshape(1, c_out, 1) if bias is not None else 0.0
    pre = (w * xg).sum(-1) * sc + bs
    mag = (w.abs() * xg.abs()).sum(-1) * (sc.abs() if scale is not None else 1.0) + (bs.abs() if bias is not None else 0.0)
    return lrelu(pre, slope), mag


def head_fwd_k(k):
    return k + HEAD_FWD_C


def _head_dx_one(g, v, scale, l_in, dil, pad, rpad):
    """One job: conv^T of g (B, c_out, l_out) onto the padded row, folded through the reflection.  (dx, mag), (B, c_in, l_in)."""
    g, v = f64(g), f64(v)
    _, c_out, l_out = g.shape
    k = v.shape[-1]
    w = v.reshape(c_out, k) * (f64(scale).reshape(c_out, 1) if scale is not None else 1.0)
    u, live = head_index(l_in, l_out, k, dil, pad, rpad, g.device)
    lv = live.to(torch.float64)
    terms = g[:, :, :, None] * w[None, :, None, :] * lv                                 # (B, c_out, l_out, k): the term of x[u[t, j]]
    return terms, g.abs()[:, :, :, None] * w.abs()[None, :, None, :] * lv, u


def head_dx(jobs, c_in, l_in):
    """(dx, mag) summed over `jobs` = [(g (B, c_out, l_out), v, scale or None, dil, pad, rpad)]:
        dx[b, ci, u] = sum over jobs, co in group ci, (t, j) with source(t, j) = u of  v[co, j] scale[co] g[b, co, t]
    -- the adjoint of head_fwd's gather, so the reflection's folds are in it by construction.  With n the number of products one
    element can receive (jobs x channels per group x k taps x three images: itself and one fold per row end) and c = 2 (the scale; the
    folded path forms v scale as a product of its own):  (n + 2) U mag.                                           c = 2"""
    dx = mag = None
    for g, v, scale, dil, pad, rpad in jobs:
        t, ta, u = _head_dx_one(g, v, scale, l_in, dil, pad, rpad)
        b, c_out, l_out, k = t.shape
        og = c_out // c_in
        idx = u.reshape(-1)
        parts = []
        for terms in (t, ta):
            grouped = terms.reshape(b, c_in, og, l_out * k).sum(2)                    # (B, c_in, l_out k)
            parts.append(torch.zeros((b, c_in, l_in), dtype=torch.float64, device=terms.device).index_add_(2, idx, grouped))
        dx = parts[0] if dx is None else dx + parts[0]
        mag = parts[1] if mag is None else mag + parts[1]
    return dx, mag


def head_dx_k(njobs, c_in, c_out, k):
    return njobs * (c_out // c_in) * k * 3 + 2


def head_dw(g_hi, x, k, dil, pad, rpad):
    """(dw, mag), (c_out, k + 1): column j = sum_{b, t} g[b, co, t] xp[b, ci(co), t - pad + j dil], column k = sum g (the bias).  The
    gradient operand is the HI plane alone (g_hi: its values as (B, c_out, l_out)): no rounding before the products."""
    g = f64(g_hi)
    c_out = g.shape[1]
    xg = _head_gather(x, c_out, k, dil, pad, rpad)
    dw = torch.cat(((g[..., None] * xg).sum((0, 2)), g.sum((0, 2))[:, None]), 1)
    mag = torch.cat(((g.abs()[..., None] * xg.abs()).sum((0, 2)), g.abs().sum((0, 2))[:, None]), 1)
    return dw, mag


def slice_size(total, nslab):
    return (total + nslab - 1) // nslab


def head_dw_depth(total, nslab):
    """bl_head_dw_kernel: a thread takes two (batch item, position) pairs per iteration, 512 pairs per block and iteration, one fused
    multiply-add per pair and sum; then wave_sum (six steps) and red[0] + red[1] + red[2] + red[3] (three)."""
    per = slice_size(total, nslab)
    return 2 * ((per + 511) // 512) + 6 + 3


# ---- chain tails -------------------------------------------------------------------------------------------------------------------
def tail_l_out(length, k, pad):
    return length + 2 * pad - (k - 1)


def _tail_gather(x, k, pad):
    """x (B, C, L) -> x[b, c, t - pad + j], zero outside the row: (B, C, l_out, k)."""
    x = f64(x)
    l = x.shape[-1]
    l_out = tail_l_out(l, k, pad)
    q = torch.arange(l_out, device=x.device)[:, None] - pad + torch.arange(k, device=x.device)[None, :]
    live = (q >= 0) & (q < l)
    return x[:, :, q.clamp(0, l - 1)] * live.to(torch.float64)


TAIL_FWD_C = 3   # the scale (on each weight), the bias, the output slope


def tail_fwd(x, v, scale, bias, pad, slope):
    """(y (B, l_out), mag): y = lrelu(sum_{c, j} (v[c, j] scale) x[b, c, t - pad + j] + bias, slope); x = the operand the kernel forms,
    join(hi, lo) or hi.  C k products:  (C k + 3) U mag,  mag = |scale| sum |v| |x| + |bias|.                          n = C k, c = 3"""
    v = f64(v)
    _, c, k = v.shape
    xg = _tail_gather(x, k, pad)
    sc = float(f64(scale).reshape(-1)[0]) if scale is not None else 1.0
    bs = float(f64(bias).reshape(-1)[0]) if bias is not None else 0.0
    w = v.reshape(1, c, 1, k)
    pre = (w * xg).sum((1, 3)) * sc + bs
    mag = (w.abs() * xg.abs()).sum((1, 3)) * abs(sc) + abs(bs)
    return lrelu(pre, slope), mag


def tail_fwd_k(channels, k):
    return channels * k + TAIL_FWD_C


def tail_map(rows, seg, seg_map, device=None):
    """map(b) = seg_map[b / seg] seg + b % seg; the identity for seg = 0."""
    b = torch.arange(rows, device=device)
    if seg <= 0:
        return b
    return torch.tensor(list(seg_map), device=device)[b // seg] * seg + b % seg


def fm_coefficients(fm_gs, s1, s2):
    return fm_gs / s2, fm_gs * s1 / (s2 * s2)


TAIL_DX_C = 6


def tail_dx(seeds, v, scale, pad, act_hi, act_lo, mask_slope, seg, seg_map, fm_rows, ref_off, fm_sums, fm_gs, length):
    """(g, mag, parts): the input gradient of the logits layer with the epilogue of the stacked backward, (rows, C, length):
        g[b, c, t] = ( sum_j v[c, j] scale seed[b, t + pad - j]
                       + (b < fm_rows ? k1 sgn(fp32(a - r)) - k2 sgn(a) : 0) ) lrelu'(a_hi[map(b), c, t])
    a = fp32(hi + lo) of row b, r the same of row b + ref_off (one fp32 addition each; the fp32 difference has the exact sign of the real
    one), k1 = fm_gs / s2, k2 = fm_gs s1 / s2^2, the mask from the HI plane alone (lrelu'(0) = slope).  act_hi / act_lo: the planes'
    values as (rows2, C, length) tensors; seeds (rows, l_out).
    Roundings: the conv part k fused multiply-adds on weights scaled once (k + 1), two additions of the feature-matching terms and the
    mask product (k + 4); the k2 term three of its own (two products, one division), its addition, the one after it and the mask (6); the k1
    term one, two additions and the mask (4):  (k + 6) U mag,  mag = (|scale| sum |v| |seed| + |k1| |sgn| + |k2| |sgn|) |mask|.  n = k, c = 6
    parts = dict(conv, mask, sd, sa): the pieces, for the sign-pattern check on planted elements."""
    seeds, v = f64(seeds), f64(v)
    rows, l_out = seeds.shape
    _, c, k = v.shape
    sc = float(f64(scale).reshape(-1)[0]) if scale is not None else 1.0
    q = torch.arange(length, device=seeds.device)[:, None] + pad - torch.arange(k, device=seeds.device)[None, :]
    live = ((q >= 0) & (q < l_out)).to(torch.float64)
    sg = seeds[:, q.clamp(0, max(l_out - 1, 0))] * live                                  # (rows, length, k)
    w = v.reshape(c, k) * sc
    conv = torch.einsum("btj,cj->bct", sg, w)
    mag = torch.einsum("btj,cj->bct", sg.abs(), w.abs())
    sd = torch.zeros_like(conv)
    sa = torch.zeros_like(conv)
    k1 = k2 = 0.0
    if fm_rows > 0:
        s1, s2 = (float(s) for s in f64(fm_sums).reshape(-1)[:2])
        k1, k2 = fm_coefficients(float(fm_gs), s1, s2)
        a = join(act_hi[:fm_rows], act_lo[:fm_rows])
        r = join(act_hi[ref_off:ref_off + fm_rows], act_lo[ref_off:ref_off + fm_rows])
        sd[:fm_rows] = sgn(f64(a - r))                  # the fp32 difference: its sign is the exact one
        sa[:fm_rows] = sgn(f64(a))
    mask_rows = f64(act_hi)[tail_map(rows, seg, seg_map, seeds.device)]
    mask = torch.where(mask_rows > 0, torch.ones_like(mask_rows), torch.full_like(mask_rows, mask_slope))
    g = (conv + k1 * sd - k2 * sa) * mask
    mag = (mag + abs(k1) * sd.abs() + abs(k2) * sa.abs()) * mask.abs()
    return g, mag, dict(conv=conv, mask=mask, sd=sd, sa=sa, k1=k1, k2=k2)


def tail_dx_k(k):
    return k + TAIL_DX_C


def tail_dw(seeds, x, rows, nbranch, k, pad):
    """(dw, mag), (nbranch, C k + 1): branch br pairs seed rows and operand rows [br rows, (br + 1) rows):
        dw[br, c k + j] = sum_{b, t} seed[b, t] x[b, c, t - pad + j],  the last column = sum seed (the bias).
    x = the operand the kernel forms (join(hi, lo) or hi), (nbranch rows, C, L); seeds (nbranch rows, l_out)."""
    seeds = f64(seeds)
    xg = _tail_gather(x, k, pad)                                                       # (R, C, l_out, k)
    c = xg.shape[1]
    dws, mags = [], []
    for br in range(nbranch):
        s = seeds[br * rows:(br + 1) * rows]
        g = xg[br * rows:(br + 1) * rows]
        dws.append(torch.cat((torch.einsum("bt,bctj->cj", s, g).reshape(c * k), s.sum().reshape(1))))
        mags.append(torch.cat((torch.einsum("bt,bctj->cj", s.abs(), g.abs()).reshape(c * k), s.abs().sum().reshape(1))))
    return torch.stack(dws), torch.stack(mags)


def tail_dw_depth(total, nslab, un):
    """bl_tail_dw_k_kernel<3, 4> (un = 4) / bl_tail_dw_kernel (un = 1): `un` pairs per thread and iteration, 256 un pairs per block and
    iteration, one fused multiply-add per pair and sum; wave_sum (six steps), four partial sums (three)."""
    per = slice_size(total, nslab)
    return un * ((per + 256 * un - 1) // (256 * un)) + 6 + 3
