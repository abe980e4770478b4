"""CPU: tests/chain_edge_oracle.py against torch in float64, and the teeth of the criteria tests/test_gpu_chain_edges.py applies.

Part (a): every restatement equals torch's own reflect pad / conv1d / conv_transpose1d under autograd in float64, on tiny shapes that
include the smallest legal rows (l_in = reflect_pad + 1: both fold ranges on one element).
Part (b): an fp32 evaluation of the right formula passes `bound_violation <= 1` with the derived bounds; seven wrong evaluations fail."""
import pytest
import torch
import torch.nn.functional as F

from tests import chain_edge_oracle as E

F32, F64 = torch.float32, torch.float64
PQMF = dict(c_in=4, c_out=24, k=3, pad=1, rpad=1)
MELGAN = dict(c_in=1, c_out=16, k=15, pad=0, rpad=7)
HEAD_SHAPES = [(PQMF, 1, 2), (PQMF, 1, 3), (PQMF, 2, 9), (PQMF, 3, 3), (PQMF, 3, 5), (PQMF, 3, 12),
               (MELGAN, 1, 8), (MELGAN, 1, 9), (MELGAN, 1, 23), (MELGAN, 2, 15), (MELGAN, 2, 16), (MELGAN, 2, 31)]


def rnd(shape, seed, dtype=F64, amp=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype) * amp


def head_params(h, seed, dtype=F64):
    return rnd((h["c_out"], 1, h["k"]), seed, dtype, 0.5), 1 + 0.3 * rnd((h["c_out"],), seed + 1, dtype), rnd((h["c_out"],), seed + 2, dtype, 0.1)


def torch_head(x, w, bias, h, dil, slope):
    return F.leaky_relu(F.conv1d(F.pad(x, (h["rpad"],) * 2, mode="reflect"), w, bias, dilation=dil, padding=h["pad"], groups=h["c_in"]), slope)


# ---- (a) the oracle against torch --------------------------------------------------------------------------------------------------
def test_plane_split_is_torchs_bfloat16_rounding():
    x = rnd((4099,), 1, F32)
    x[:8] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])   # zeros, denormals, exact ties
    hi, lo = E.split(x)
    assert torch.equal(hi.view(torch.int32), x.to(torch.bfloat16).float().view(torch.int32))
    assert torch.equal(lo.view(torch.int32), (x - hi).to(torch.bfloat16).float().view(torch.int32))
    assert float(hi[6]) == 1.0 and float(hi[7]) == 1.0 + 2.0 ** -6                    # ties to even, both ways
    assert E.split_violations(hi, lo) == 0
    assert float(((E.join(hi, lo).double() - x.double()).abs() - E.plane_bound(x, 0.0)).max()) <= 0
    assert float(((hi.double() - x.double()).abs() - E.plane_bound(x, 0.0, lo=False)).max()) <= 0
    bad = lo.clone()
    bad[100] = hi[100] * 2.0 ** -7                                                    # a whole ulp of hi
    assert E.split_violations(hi, bad) == 1
    y = rnd((2, 16, 5), 2, F32)
    assert torch.equal(E.from_bundles(E.to_bundles(y)), y) and E.to_bundles(y).shape == (2, 2, 5, 8)
    assert float(E.to_bundles(y)[1, 1, 3, 2]) == float(y[1, 10, 3])


@pytest.mark.parametrize("h,dil,l_in", HEAD_SHAPES, ids=lambda v: "head" if isinstance(v, dict) else str(v))
def test_head_restatements_follow_autograd(h, dil, l_in):
    batch = 2
    v, scale, bias = head_params(h, 10 * l_in + dil)
    x = rnd((batch, h["c_in"], l_in), 7 + l_in)
    w = (v * scale.reshape(-1, 1, 1)).clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    ref = torch_head(xr, w, br, h, dil, 0.2)
    assert ref.shape[-1] == E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
    y, mag = E.head_fwd(x, v, scale, bias, dil, h["pad"], h["rpad"], 0.2)
    assert float((y - ref.detach()).abs().max()) < 1e-14 and bool((mag >= y.abs() - 1e-14).all())
    y0, _ = E.head_fwd(x, v, None, None, dil, h["pad"], h["rpad"], 1.0)
    assert float((y0 - torch_head(x, v, None, h, dil, 1.0)).abs().max()) < 1e-14
    # input gradient of the pre-activation (the kernels receive the masked gradient) and weight / bias gradient
    g = rnd(ref.shape, 11 + l_in)
    pre = F.conv1d(F.pad(xr, (h["rpad"],) * 2, mode="reflect"), w, br, dilation=dil, padding=h["pad"], groups=h["c_in"])
    (pre * g).sum().backward()
    dx, dmag = E.head_dx([(g, v, scale, dil, h["pad"], h["rpad"])], h["c_in"], l_in)
    assert float((dx - xr.grad).abs().max()) < 1e-13 and bool((dmag >= dx.abs() - 1e-13).all())
    wr = v.clone().requires_grad_(True)                      # the weight gradient is that of the direction v with scale = 1: d / dv of conv(x, v)
    (F.conv1d(F.pad(x, (h["rpad"],) * 2, mode="reflect"), wr, None, dilation=dil, padding=h["pad"], groups=h["c_in"]) * g).sum().backward()
    dw, _ = E.head_dw(g, x, h["k"], dil, h["pad"], h["rpad"])
    assert float((dw[:, :h["k"]] - wr.grad.reshape(h["c_out"], h["k"])).abs().max()) < 1e-13
    assert float((dw[:, h["k"]] - br.grad).abs().max()) < 1e-13


def test_head_input_gradient_sums_the_jobs():
    l_in = 7
    x = rnd((2, 4, l_in), 3).requires_grad_(True)
    jobs, total = [], 0
    for dil in (1, 2, 3):
        v, scale, _ = head_params(PQMF, 40 + dil)
        pre = F.conv1d(F.pad(x, (1, 1), mode="reflect"), v * scale.reshape(-1, 1, 1), None, dilation=dil, padding=1, groups=4)
        g = rnd(pre.shape, 50 + dil)
        total = total + (pre * g).sum()
        jobs.append((g, v, scale, dil, 1, 1))
    total.backward()
    dx, _ = E.head_dx(jobs, 4, l_in)
    assert float((dx - x.grad).abs().max()) < 1e-13


TAIL_SHAPES = [(8, 1, 1, 0), (8, 1, 3, 1), (16, 2, 3, 1), (8, 5, 5, 2), (24, 9, 8, 4), (8, 9, 8, 0), (16, 4, 2, 1), (8, 6, 2, 0), (8, 3, 3, 2)]


@pytest.mark.parametrize("channels,length,k,pad", TAIL_SHAPES)
def test_tail_restatements_follow_autograd(channels, length, k, pad):
    half, slope, gs = 2, 0.2, 0.37
    l_out = E.tail_l_out(length, k, pad)
    assert l_out > 0
    v = rnd((1, channels, k), 60 + k, amp=0.3)
    scale, bias = torch.tensor([1.3], dtype=F64), torch.tensor([0.05], dtype=F64)
    w = v * scale
    hi, lo = E.split(rnd((2 * half, channels, length), 61 + length, F32))
    e = E.join(hi, lo).double()                             # the embedding: what the planes hold
    y, mag = E.tail_fwd(e, v, scale, bias, pad, 0.2)
    ref = F.leaky_relu(F.conv1d(e, w, bias, padding=pad), 0.2)[:, 0]
    assert float((y - ref).abs().max()) < 1e-14 and bool((mag >= y.abs() - 1e-14).all())
    # weight gradient, two branches
    seeds = rnd((4 * half, l_out), 62)
    sd = seeds[2 * half:]
    dw, _ = E.tail_dw(sd, e, half, 2, k, pad)
    for br in range(2):
        wr = v.clone().requires_grad_(True)
        (F.conv1d(e[br * half:(br + 1) * half], wr, None, padding=pad)[:, 0] * sd[br * half:(br + 1) * half]).sum().backward()
        assert float((dw[br, :-1] - wr.grad.reshape(-1)).abs().max()) < 1e-13
        assert float(dw[br, -1] - sd[br * half:(br + 1) * half].sum()) == pytest.approx(0, abs=1e-13)
    # input gradient: four stacked seed blocks [fm | adv | fake | real] on the embedding rows (0, 0, 0, 1), the feature-matching term on
    # the first; autograd through e = lrelu(pre) block by block (sign(pre) = sign(e), so the mask and the signs are those of the planes)
    s1, s2 = float((e[:half] - e[half:]).abs().sum()), float(e[:half].abs().sum())
    got, _, _ = E.tail_dx(seeds, v, scale, pad, hi, lo, slope, half, (0, 0, 0, 1), half, half, torch.tensor([s1, s2], dtype=F64), gs, length)
    pre0 = torch.where(e > 0, e, e / slope)
    for blk, src in enumerate((0, 0, 0, 1)):
        pre = pre0.clone().requires_grad_(True)
        emb = F.leaky_relu(pre, slope)
        rows = slice(src * half, (src + 1) * half)
        loss = (F.conv1d(emb[rows], w, None, padding=pad)[:, 0] * seeds[blk * half:(blk + 1) * half]).sum()
        if blk == 0:
            loss = loss + gs * (emb[:half] - emb[half:].detach()).abs().sum() / emb[:half].abs().sum()
        loss.backward()
        want = pre.grad[rows]
        assert float((got[blk * half:(blk + 1) * half] - want).abs().max()) < 1e-12, blk
    # the identity map and no feature matching: the plain transposed conv times the mask of the row itself
    got2, _, _ = E.tail_dx(seeds, v, scale, pad, hi.repeat(2, 1, 1), None, slope, 0, None, 0, 0, None, 0.0, length)
    base = F.conv_transpose1d(seeds[:, None], w, padding=pad, output_padding=0)
    assert base.shape[-1] == length
    assert float((got2 - base * (1.0 - (1.0 - slope) * (hi.repeat(2, 1, 1) <= 0).double())).abs().max()) < 1e-13
    assert E.tail_map(7, 2, (0, 0, 0, 1)).tolist() == [0, 1, 0, 1, 0, 1, 2]


def test_depths_follow_the_kernels_loops():
    assert E.head_dw_depth(512 * 32, 32) == 2 + 9 and E.head_dw_depth(513 * 32, 32) == 4 + 9 and E.head_dw_depth(5, 32) == 2 + 9
    assert E.tail_dw_depth(1024, 1, 4) == 4 + 9 and E.tail_dw_depth(1025, 1, 4) == 8 + 9 and E.tail_dw_depth(1025, 1, 1) == 5 + 9
    assert E.slice_size(4097, 2) == 2049


# ---- (b) the teeth: fp32 evaluations, right and wrong ------------------------------------------------------------------------------
def head_fwd_f32(x, v, scale, bias, h, dil, slope, tap_off_by_one=False, per_tap_scale=None):
    """The head forward in fp32 torch.  tap_off_by_one: tap 1 reads one position further.  per_tap_scale: a factor per TAP on every
    product (what a kernel would do that indexed a scale vector by the tap and did not test its job's scale for NULL)."""
    l_in = x.shape[-1]
    l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
    t = torch.arange(l_out)[:, None]
    j = torch.arange(h["k"])[None, :]
    p = t - h["pad"] + j * dil + ((j == 1).long() if tap_off_by_one else 0)
    live = (p >= 0) & (p < l_in + 2 * h["rpad"])
    u = (p - h["rpad"]).abs()
    u = torch.where(u >= l_in, 2 * (l_in - 1) - u, u).clamp(0, l_in - 1)
    xg = (x[:, :, u] * live.to(F32)).repeat_interleave(h["c_out"] // h["c_in"], dim=1)
    w = v.reshape(1, h["c_out"], 1, h["k"])
    if per_tap_scale is not None:
        w = w * per_tap_scale.reshape(1, 1, 1, -1)
    a = (w * xg).sum(-1)
    if scale is not None:
        a = a * scale.reshape(1, -1, 1)
    if bias is not None:
        a = a + bias.reshape(1, -1, 1)
    return torch.where(a > 0, a, a * slope)


def head_dx_f32(jobs, h, l_in, skip_far_fold=False):
    """conv^T onto the padded row in fp32, then the two folds of the reflection written out; skip_far_fold drops the one at the row's end."""
    P = h["rpad"]
    dx = torch.zeros((jobs[0][0].shape[0], h["c_in"], l_in), dtype=F32)
    for g, v, scale, dil, pad, rpad in jobs:
        w = v if scale is None else v * scale.reshape(-1, 1, 1)
        dxp = F.conv_transpose1d(g, w, dilation=dil, padding=pad, groups=h["c_in"])
        assert dxp.shape[-1] == l_in + 2 * P
        dx = dx + dxp[..., P:P + l_in]
        for u in range(l_in):
            if 1 <= u <= P:
                dx[..., u] += dxp[..., P - u]
            if l_in - 1 - P <= u <= l_in - 2 and not skip_far_fold:
                dx[..., u] += dxp[..., P + 2 * (l_in - 1) - u]
    return dx


def tail_dx_f32(seeds, v, scale, pad, hi, lo, slope, seg, seg_map, fm_rows, ref_off, sums, gs, mask_from_sum=False, sgn0_plus=False):
    w = v * scale
    val = F.conv_transpose1d(seeds[:, None], w, padding=pad)
    a_all = hi + lo
    if fm_rows:
        s1, s2 = sums
        k1, k2 = gs / s2, gs * s1 / (s2 * s2)
        a, r = a_all[:fm_rows], a_all[ref_off:ref_off + fm_rows]
        sign = (lambda t: torch.where(t >= 0, 1.0, -1.0).to(F32)) if sgn0_plus else torch.sign
        val[:fm_rows] += k1 * sign(a - r) - k2 * sign(a)
    m = (a_all if mask_from_sum else hi)[E.tail_map(seeds.shape[0], seg, seg_map)]
    return val * torch.where(m > 0, 1.0, slope).to(F32)


def tail_dw_f32(seeds, x, rows, nbranch, k, pad, nslab, drop_bias_of=None):
    """Slabs (nbranch, nslab, C k + 1) in fp32: slice z of a branch = (batch item, position) pairs [z per, (z + 1) per) in row-major order."""
    c, l = x.shape[1], x.shape[2]
    l_out = E.tail_l_out(l, k, pad)
    q = torch.arange(l_out)[:, None] - pad + torch.arange(k)[None, :]
    xg = x[:, :, q.clamp(0, l - 1)] * ((q >= 0) & (q < l)).to(F32)                 # (R, C, l_out, k)
    total, per = rows * l_out, E.slice_size(rows * l_out, nslab)
    out = torch.zeros((nbranch, nslab, c * k + 1), dtype=F32)
    for br in range(nbranch):
        s = seeds[br * rows:(br + 1) * rows].reshape(total)
        g = xg[br * rows:(br + 1) * rows].permute(0, 2, 1, 3).reshape(total, c * k)
        for z in range(nslab):
            lo_, hi_ = z * per, min((z + 1) * per, total)
            if lo_ < hi_:
                out[br, z, :-1] = (s[lo_:hi_, None] * g[lo_:hi_]).sum(0)
                out[br, z, -1] = 0.0 if drop_bias_of == (br, z) else s[lo_:hi_].sum()
    return out


def violation(got, ref, k, mag, planes=None):
    bound = k * E.U * mag
    if planes is not None:
        bound = E.plane_bound(ref, bound, lo=planes)
    return E.bound_violation(got, ref, 1, bound / E.U)


def through_planes(val, lo=True):
    hi, l = E.split(val)
    return E.join(hi, l if lo else None)


@pytest.mark.parametrize("h,dil,l_in", [(PQMF, 2, 9), (PQMF, 2, 3), (MELGAN, 2, 16), (MELGAN, 2, 40)], ids=lambda v: "head" if isinstance(v, dict) else str(v))
def test_head_forward_bound_separates_a_shifted_tap_and_a_per_tap_scale(h, dil, l_in):
    v, scale, bias = head_params(h, 70 + l_in, F32)
    x = rnd((3, h["c_in"], l_in), 71, F32)
    ref, mag = E.head_fwd(x, v, scale, bias, dil, h["pad"], h["rpad"], 0.2)
    k = E.head_fwd_k(h["k"])
    assert violation(through_planes(head_fwd_f32(x, v, scale, bias, h, dil, 0.2)), ref, k, mag, planes=True) <= 1
    assert violation(through_planes(head_fwd_f32(x, v, scale, bias, h, dil, 0.2), lo=False), ref, k, mag, planes=False) <= 1
    assert violation(through_planes(head_fwd_f32(x, v, scale, bias, h, dil, 0.2), lo=False), ref, k, mag, planes=True) > 1    # hi alone is no hi + lo
    assert violation(through_planes(head_fwd_f32(x, v, scale, bias, h, dil, 0.2, tap_off_by_one=True)), ref, k, mag, planes=True) > 1
    # scale NULL: the factor is 1, once per channel
    ref0, mag0 = E.head_fwd(x, v, None, bias, dil, h["pad"], h["rpad"], 0.2)
    assert violation(through_planes(head_fwd_f32(x, v, None, bias, h, dil, 0.2)), ref0, k, mag0, planes=True) <= 1
    per_tap = 1 + 0.3 * rnd((h["k"],), 72, F32)
    assert violation(through_planes(head_fwd_f32(x, v, None, bias, h, dil, 0.2, per_tap_scale=per_tap)), ref0, k, mag0, planes=True) > 1


@pytest.mark.parametrize("h,dils,l_in", [(PQMF, (1, 2, 3), 3), (PQMF, (1, 2, 3), 9), (MELGAN, (1, 1), 8), (MELGAN, (1, 2), 15), (MELGAN, (1,), 33)],
                         ids=lambda v: "head" if isinstance(v, dict) else str(v))
def test_head_input_gradient_bound_separates_a_missing_fold(h, dils, l_in):
    jobs32 = []
    for i, dil in enumerate(dils):
        v, scale, _ = head_params(h, 80 + i, F32)
        l_out = E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"])
        g = E.join(*E.split(rnd((2, h["c_out"], l_out), 81 + i, F32)))
        jobs32.append((g, v, scale, dil, h["pad"], h["rpad"]))
    ref, mag = E.head_dx(jobs32, h["c_in"], l_in)
    k = E.head_dx_k(len(dils), h["c_in"], h["c_out"], h["k"])
    assert violation(head_dx_f32(jobs32, h, l_in), ref, k, mag) <= 1
    assert violation(head_dx_f32(jobs32, h, l_in, skip_far_fold=True), ref, k, mag) > 1


def tail_operands(channels, length, k, pad, half, seed):
    v = rnd((1, channels, k), seed, F32, 0.3)
    hi, lo = E.split(rnd((2 * half, channels, length), seed + 1, F32))
    # planted: a == r, a == 0, both, and hi = 0 under a positive lo (no split produces it; the mask must still follow hi)
    hi[0, 0, 0], lo[0, 0, 0] = hi[half, 0, 0], lo[half, 0, 0]
    hi[0, 1, 0] = lo[0, 1, 0] = 0.0
    hi[0, 2, 0] = lo[0, 2, 0] = hi[half, 2, 0] = lo[half, 2, 0] = 0.0
    hi[0, 3, 0], lo[0, 3, 0] = 0.0, 0.25
    seeds = rnd((4 * half, E.tail_l_out(length, k, pad)), seed + 2, F32)
    return v, hi, lo, seeds


@pytest.mark.parametrize("channels,length,k,pad", [(8, 1, 3, 1), (8, 5, 3, 1), (16, 7, 8, 4), (8, 6, 1, 0), (8, 4, 3, 2)])
def test_tail_bounds_separate_the_wrong_epilogues_and_operands(channels, length, k, pad):
    half, slope, gs = 2, 0.2, 0.37
    v, hi, lo, seeds = tail_operands(channels, length, k, pad, half, 90 + length)
    scale, bias, sums = torch.tensor([1.3]), torch.tensor([0.05]), torch.tensor([3.5, 11.0])
    # forward: the operand is hi + lo
    x = E.join(hi, lo)
    ref, mag = E.tail_fwd(x, v, scale, bias, pad, 1.0)
    right = F.conv1d(x, v * scale, bias, padding=pad)[:, 0]
    assert violation(right, ref, E.tail_fwd_k(channels, k), mag) <= 1
    assert violation(F.conv1d(hi, v * scale, bias, padding=pad)[:, 0], ref, E.tail_fwd_k(channels, k), mag) > 1          # lo dropped
    # input gradient
    args = (seeds, v, scale, pad, hi, lo, slope, half, (0, 0, 0, 1), half, half)
    ref, mag, parts = E.tail_dx(*args, sums, gs, length)
    kk = E.tail_dx_k(k)
    got = tail_dx_f32(*args, (3.5, 11.0), gs)
    assert violation(through_planes(got), ref, kk, mag, planes=True) <= 1
    assert violation(through_planes(got, lo=False), ref, kk, mag, planes=False) <= 1
    assert violation(through_planes(tail_dx_f32(*args, (3.5, 11.0), gs, mask_from_sum=True)), ref, kk, mag, planes=True) > 1
    assert violation(through_planes(tail_dx_f32(*args, (3.5, 11.0), gs, sgn0_plus=True)), ref, kk, mag, planes=True) > 1
    assert set(parts["sd"][:half].reshape(-1).tolist()) == {-1.0, 0.0, 1.0} and 0.0 in parts["sa"][:half].reshape(-1).tolist()
    # weight gradient: two slices, the slabs summed in float64
    sd = seeds[2 * half:]
    ref, mag = E.tail_dw(sd, x, half, 2, k, pad)
    total = half * E.tail_l_out(length, k, pad)
    if total >= 2:
        d = E.tail_dw_depth(total, 2, 4 if k == 3 else 1)
        assert violation(tail_dw_f32(sd, x, half, 2, k, pad, 2).double().sum(1), ref, d, mag) <= 1
        assert violation(tail_dw_f32(sd, x, half, 2, k, pad, 2, drop_bias_of=(1, 1)).double().sum(1), ref, d, mag) > 1
        assert violation(tail_dw_f32(sd, hi, half, 2, k, pad, 2).double().sum(1), ref, d, mag) > 1                     # lo dropped


def test_head_weight_gradient_bound_separates_a_lost_bias_slice():
    h, dil, l_in, batch, nslab = PQMF, 3, 40, 3, 32
    x = rnd((batch, 4, l_in), 95, F32)
    l_out = E.head_l_out(l_in, 3, dil, 1, 1)
    g_hi, g_lo = E.split(rnd((batch, 24, l_out), 96, F32))
    ref, mag = E.head_dw(g_hi, x, 3, dil, 1, 1)
    total, per = batch * l_out, E.slice_size(batch * l_out, nslab)
    xg = head_gather_f32(x, h, dil)
    terms = torch.cat((g_hi[..., None] * xg, g_hi[..., None]), -1).permute(1, 3, 0, 2).reshape(24, 4, total)     # (co, column, pair)
    slabs = torch.stack([terms[..., z * per:min((z + 1) * per, total)].sum(-1) if z * per < total else torch.zeros(24, 4) for z in range(nslab)])
    d = E.head_dw_depth(total, nslab)
    assert violation(slabs.double().sum(0), ref, d, mag) <= 1
    lost = slabs.clone()
    lost[5, :, 3] = 0
    assert violation(lost.double().sum(0), ref, d, mag) > 1
    full = torch.cat(((g_hi + g_lo)[..., None] * xg, (g_hi + g_lo)[..., None]), -1).sum((0, 2))
    assert violation(full, ref, d, mag) > 1                                                                      # the operand is the hi plane alone


def head_gather_f32(x, h, dil):
    l_in = x.shape[-1]
    u, live = E.head_index(l_in, E.head_l_out(l_in, h["k"], dil, h["pad"], h["rpad"]), h["k"], dil, h["pad"], h["rpad"])
    return (x[:, :, u] * live.to(F32)).repeat_interleave(h["c_out"] // h["c_in"], dim=1)
