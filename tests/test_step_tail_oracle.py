"""CPU: tests/step_tail_oracle.py against torch in float64, and the teeth of the criteria tests/test_gpu_step_tail.py applies.

Part (b) emulates the block structure of the kernels in numpy fp32 (Adam's 4096-element blocks and 48-tensor table chunks, the
feature-matching partial sums per 32-pair launch, the sign gradient, the stacked seeds) and feeds the right formula and six wrong ones
through the same comparison helpers with the same bounds: the fp32 emulation must be accepted, each wrong variant rejected."""
import math

import numpy as np
import pytest
import torch

from oracle import eben_oracle as O
from tests import step_tail_oracle as S

F32 = np.float32
HYPER = (float(F32(3e-4)), (0.5, float(F32(0.9))), float(F32(1e-8)))   # the configured Adam, as the fp32 values the entry point receives


def rng_state(n, seed, gscale, psize=1.0):
    r = np.random.default_rng(seed)
    p = (r.standard_normal(n) * psize).astype(F32)
    g = (r.standard_normal(n) * gscale).astype(F32)
    m = (r.standard_normal(n) * gscale).astype(F32)
    v = ((r.standard_normal(n) * gscale) ** 2).astype(F32)
    return p, m, v, g


# ---- (a) the oracle against torch --------------------------------------------------------------------------------------------------
def test_adam_step_follows_torch_adam_over_five_steps():
    torch.manual_seed(0)
    lr, betas, eps, wd, gs = 3e-4, (0.5, 0.9), 1e-8, 0.01, 0.125
    p0 = torch.randn(301, dtype=torch.float64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 6):
        g = torch.randn(301, dtype=torch.float64) * 1e-2
        ref.grad = g * gs                                   # torch sees the gradient already scaled
        opt.step()
        p, m, v = S.adam_step(p, m, v, g, step, lr, betas, eps, wd, gs)
        st = opt.state[ref]
        assert float((p - ref.detach()).abs().max()) < 1e-15
        assert float((m - st["exp_avg"]).abs().max()) < 1e-17 and float((v - st["exp_avg_sq"]).abs().max()) < 1e-19


def test_loss_gradients_follow_autograd_of_the_oracle_losses():
    torch.manual_seed(1)
    shapes = [[(2, 1, 50), (2, 8, 50), (2, 16, 25), (2, 1, 25)], [(2, 1, 40), (2, 4, 41), (2, 12, 20), (2, 1, 20)]]
    ea = [[torch.randn(s, dtype=torch.float64).requires_grad_(True) for s in sc] for sc in shapes]
    eb = [[torch.randn(s, dtype=torch.float64) for s in sc] for sc in shapes]
    inv_count = 1.0 / (len(ea) * len(ea[-1][1:-1]))
    gout = 0.7
    (O.feature_loss(ea, eb) * gout).backward()
    for sa, sb in zip(ea, eb):
        for a, b in zip(sa[1:-1], sb[1:-1]):
            s1, s2 = S.fm_sums(a, b)
            assert s1 == pytest.approx(float((a.detach() - b).abs().sum()), rel=1e-14) and s2 == pytest.approx(float(a.detach().abs().sum()), rel=1e-14)
            grad, scale = S.fm_grad(a, b, s1, s2, gout, inv_count)
            assert float((grad - a.grad).abs().max()) < 1e-15 * float(scale.max())
            assert S.pattern_mismatches(S.fm_decode(grad, s1, s2, gout, inv_count), S.fm_codes(a, b).reshape(-1)) == 0
    for target in (1.0, -1.0):
        logits = [[None, torch.randn(2, 1, 33, dtype=torch.float64).requires_grad_(True)] for _ in range(3)]
        (O.hinge_loss(logits, target) * 1.3).backward()
        assert O.hinge_loss(logits, target).item() == pytest.approx(np.mean([S.hinge_mean(sc[-1], target) for sc in logits]), rel=1e-14)
        for sc in logits:
            assert float((S.hinge_grad(sc[-1], target, 1.3, 1.0 / 3) - sc[-1].grad).abs().max()) < 1e-17
    a, b = torch.randn(7, dtype=torch.float64), torch.randn(7, dtype=torch.float64)
    seeds = S.hinge_seeds(a, b, 0.9, (0.25, 0.5, 0.75))
    assert torch.equal(seeds[:7], torch.zeros(7, dtype=torch.float64))
    assert torch.equal(seeds[7:14], S.hinge_grad(a, 1.0, 0.9, 0.25)) and torch.equal(seeds[14:21], S.hinge_grad(a, -1.0, 0.9, 0.5))
    assert torch.equal(seeds[21:], S.hinge_grad(b, 1.0, 0.9, 0.75))


def test_elementwise_restatements_follow_torch():
    torch.manual_seed(2)
    x = torch.randn(3, 4, 31, dtype=torch.float64)
    x[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-40, -1e-40], dtype=torch.float64)
    for slope in (0.01, 0.2):
        xr = x.clone().requires_grad_(True)
        y = torch.nn.functional.leaky_relu(xr, slope)
        dy = torch.randn_like(x)
        (y * dy).sum().backward()
        assert torch.equal(S.leaky_relu(x, slope), y.detach()) and torch.equal(S.leaky_relu_grad(dy, x, slope), xr.grad)
    lift = torch.randn(3, 2, 31, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    out = torch.tanh(xr + torch.cat((lift, torch.zeros(3, 2, 31, dtype=torch.float64)), 1))
    dout = torch.randn_like(x)
    (out * dout).sum().backward()
    assert torch.equal(S.tanh_lift(x, lift, 2), out.detach()) and torch.equal(S.tanh_lift(x, None, 0), torch.tanh(x))
    assert float((S.tanh_grad(dout, out)[0] - xr.grad).abs().max()) < 1e-15
    assert S.l2norm(x) == pytest.approx(float(torch.linalg.vector_norm(x)), rel=1e-14)
    sums = torch.rand(5, 2, dtype=torch.float64) + 0.5
    hinge = torch.rand(4, 3, dtype=torch.float64)
    got = S.disc_losses(sums.reshape(-1), 1 / 24, hinge.reshape(-1))
    assert got[0].item() == pytest.approx(sum(float(a / b) for a, b in sums) / 24, rel=1e-14)
    assert torch.allclose(got[1:], hinge.mean(0), rtol=1e-14, atol=0)
    res = [torch.rand(5, 3, dtype=torch.float64) + 0.1 for _ in range(3)]
    want = np.mean([float(sum(math.sqrt(r[0] / r[1]) for r in s) / 5 + sum(float(r[2]) for r in s) * ic) for s, ic in zip(res, (0.1, 0.2, 0.3))])
    assert S.stft_loss_total(res, (0.1, 0.2, 0.3)) == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("lx,pl,pr", [(2, 1, 1), (3, 2, 2), (5, 0, 4), (5, 4, 0), (1001, 7, 3), (17, 16, 16)])
def test_reflect_pad_and_its_adjoint(lx, pl, pr):
    torch.manual_seed(3)
    x = torch.randn(3, lx, dtype=torch.float64)
    y = S.reflect_pad(x, pl, pr)
    assert torch.equal(y, torch.nn.functional.pad(x[None], (pl, pr), mode="reflect")[0])
    dy = torch.randn(3, lx + pl + pr, dtype=torch.float64)
    dx = S.reflect_pad_adjoint(dy, lx, pl, pr)
    # <pad(x), dy> == <x, pad^T(dy)>
    assert float((y * dy).sum()) == pytest.approx(float((x * dx).sum()), rel=1e-12, abs=1e-12)
    # every padded position lands somewhere, and an interior position of (3, 2, 2) collects three of them
    assert float(S.reflect_pad_adjoint(torch.ones(1, lx + pl + pr, dtype=torch.float64), lx, pl, pr).sum()) == lx + pl + pr
    if (lx, pl, pr) == (3, 2, 2):
        assert S.reflect_pad_adjoint(torch.ones(1, 7, dtype=torch.float64), lx, pl, pr).tolist() == [[2.0, 3.0, 2.0]]


def test_code_byte_of_the_bundle_planes():
    a = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, -1.0, -1.0])
    r = torch.tensor([0.5, 1.0, 2.0, -1.0, 0.0, 1.0, -2.0, -1.0, 0.0])
    #       sgn(a - r) + 1 | (sgn(a) + 1) << 2
    assert S.bl_fm_code(a, r).tolist() == [2 | 8, 1 | 8, 0 | 8, 2 | 4, 1 | 4, 0 | 4, 2 | 0, 1 | 0, 0 | 0]


# ---- (b) fp32 emulations of the kernels' structure: the right one passes, the wrong ones do not -------------------------------------
ADAM_BLOCK, ADAM_CHUNK, FM_PAIRS, FM_BLOCKS = 4096, 48, 32, 1024


def adam_elements_f32(p, m, v, g, step, lr, betas, eps, wd, gs, eps_inside=False):
    """adam_update of csrc/direct.hip operation by operation in fp32 (no contraction); eps_inside: (sqrt(v) + eps) / sqrt(bc2)."""
    b1, b2, lr, eps, wd, gs = F32(betas[0]), F32(betas[1]), F32(lr), F32(eps), F32(wd), F32(gs)
    bc1 = F32(1.0 - float(b1) ** step)
    bc2s = F32(math.sqrt(1.0 - float(b2) ** step))
    one = F32(1)
    g = g * gs
    if wd != 0:
        g = wd * p + g
    m = m + (g - m) * (one - b1)
    v = v * b2 + (one - b2) * g * g
    denom = (np.sqrt(v) + eps) / bc2s if eps_inside else np.sqrt(v) / bc2s + eps
    p = p - (lr / bc1) * (m / denom)
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v


def adam_table_f32(table, step, hyper, wd=0.0, gs=1.0, skip_tail=False, stale_chunk=False, eps_inside=False):
    """eben_adam_step over a table of (p, m, v, g) arrays: chunks of 48 tensors, blocks of 4096 elements.  skip_tail: a tensor's last
    partial block is not run; stale_chunk: a later chunk reads the table without its offset."""
    lr, betas, eps = hyper
    out = [[t[0].copy(), t[1].copy(), t[2].copy()] for t in table]
    for p0 in range(0, len(table), ADAM_CHUNK):
        for i in range(min(ADAM_CHUNK, len(table) - p0)):
            k = i if stale_chunk else p0 + i
            n = table[k][0].size
            for base in range(0, n, ADAM_BLOCK):
                end = min(base + ADAM_BLOCK, n)
                if skip_tail and end - base < ADAM_BLOCK and base > 0:
                    continue
                sl = slice(base, end)
                res = adam_elements_f32(out[k][0][sl], out[k][1][sl], out[k][2][sl], table[k][3][sl], step, lr, betas, eps, wd, gs, eps_inside)
                for dst, r in zip(out[k], res):
                    dst[sl] = r
    return out


def adam_table_violation(table, got, step, hyper, wd=0.0, gs=1.0):
    """Worst violation of the three Adam criteria over a table, exactly as the GPU test applies them."""
    lr, betas, eps = hyper
    worst = 0.0
    for (p, m, v, g), (p1, m1, v1) in zip(table, got):
        tp, tm, tv, tg = (torch.from_numpy(t) for t in (p, m, v, g))
        rp, rm, rv = S.adam_step(tp, tm, tv, tg, step, lr, betas, eps, wd, gs)
        bm, bv, bu = S.adam_bounds(tp, tm, tv, tg, step, lr, betas, eps, wd, gs)
        worst = max(worst, S.bound_violation(torch.from_numpy(m1), rm, 1, bm / S.U), S.bound_violation(torch.from_numpy(v1), rv, 1, bv / S.U),
                    S.bound_violation(torch.from_numpy(p1).double() - tp.double(), rp - tp.double(), 1, S.adam_update_bound(tp, rp, bu) / S.U))
    return worst


SIZES = (1, 3, 255, 256, 4095, 4096, 4097, 2 * 4096 + 5, 3 * 4096)


@pytest.mark.parametrize("gscale", [1e-2, 1e-8])
@pytest.mark.parametrize("step,wd,gs", [(1, 0.0, 1.0), (2, 0.01, 0.5), (1000, 0.0, 0.125)])
def test_adam_bounds_accept_an_fp32_step(gscale, step, wd, gs):
    table = [rng_state(n, 10 + i, gscale, psize=(1e-3 if i % 2 else 1.0)) for i, n in enumerate(SIZES)]
    got = adam_table_f32(table, step, HYPER, wd, gs)
    assert adam_table_violation(table, got, step, HYPER, wd, gs) <= 1.0


def test_adam_criteria_reject_eps_inside_the_bias_correction():
    """(sqrt(v) + eps) / sqrt(bc2): invisible at |g| ~ 1e-2 within any bound fp32 allows (the parameters of the old test move by 8e-7 of
    max|p|), a 35 % error of the update at |g| ~ 1e-8, where eps carries weight."""
    table = [rng_state(4097, 20, 1e-8, psize=1e-3)]
    assert adam_table_violation(table, adam_table_f32(table, 1, HYPER), 1, HYPER) <= 1.0
    wrong = adam_table_f32(table, 1, HYPER, eps_inside=True)
    assert adam_table_violation(table, wrong, 1, HYPER) > 1.0
    # the old criterion (max|p - ref| below 1e-6 of max|p|, |g| ~ 1e-2, |p| ~ 1) does not see it
    lr, betas, eps = HYPER
    old = rng_state(4097, 22, 1e-2)
    p, m, v, g = (torch.from_numpy(t) for t in old)
    rp = S.adam_step(p, m, v, g, 1, lr, betas, eps)[0]
    wrong_p = torch.from_numpy(adam_table_f32([old], 1, HYPER, eps_inside=True)[0][0]).double()
    assert float((wrong_p - rp).abs().max() / rp.abs().max()) < 1e-6


def test_adam_criteria_reject_a_skipped_tail_block():
    table = [rng_state(2 * 4096 + 5, 21, 1e-2)]
    assert adam_table_violation(table, adam_table_f32(table, 2, HYPER), 2, HYPER) <= 1.0
    assert adam_table_violation(table, adam_table_f32(table, 2, HYPER, skip_tail=True), 2, HYPER) > 1.0


def test_adam_criteria_reject_a_second_chunk_that_reads_the_first():
    table = [rng_state(SIZES[i % 5], 30 + i, 1e-2) for i in range(49)]
    assert adam_table_violation(table, adam_table_f32(table, 3, HYPER), 3, HYPER) <= 1.0
    assert adam_table_violation(table, adam_table_f32(table, 3, HYPER, stale_chunk=True), 3, HYPER) > 1.0


def fm_sums_f32(pairs, unoffset=False):
    """eben_fm_sums: launches of 32 pairs, 1024 slices per pair summed in fp32, then the fixed-order final sum into sums[2 (p0 + i)];
    unoffset: the final pass of a later launch writes at sums[2 i]."""
    sums = np.full(2 * len(pairs), np.nan, F32)
    for p0 in range(0, len(pairs), FM_PAIRS):
        for i, (a, b) in enumerate(pairs[p0:p0 + FM_PAIRS]):
            n = a.size
            per = ((n + FM_BLOCKS - 1) // FM_BLOCKS + 3) & ~3
            part = np.zeros((FM_BLOCKS, 2), F32)
            for blk in range(min(FM_BLOCKS, (n + per - 1) // per)):
                sl = slice(blk * per, min((blk + 1) * per, n))
                part[blk] = np.abs(a[sl] - b[sl]).sum(dtype=F32), np.abs(a[sl]).sum(dtype=F32)
            slot = i if unoffset else p0 + i
            sums[2 * slot:2 * slot + 2] = part.sum(0, dtype=F32)
    return sums


def fm_pairs(count, seed):
    r = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = (1, 3, 4, 1023, 4 * 1024 + 1)[i % 5]
        a, b = r.standard_normal(n).astype(F32), r.standard_normal(n).astype(F32)
        out.append((a, b))
    return out


def fm_sums_worst(pairs, sums):
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        s1, s2 = S.fm_sums(torch.from_numpy(a), torch.from_numpy(b))
        worst = max(worst, S.rel_sum_error(sums[2 * i], s1), S.rel_sum_error(sums[2 * i + 1], s2))
    return worst


def test_fm_sums_tolerance_rejects_the_unoffset_slot():
    pairs = fm_pairs(33, 40)
    assert fm_sums_worst(pairs, fm_sums_f32(pairs)) < 1e-5
    assert not fm_sums_worst(pairs, fm_sums_f32(pairs, unoffset=True)) < 1e-5


def fm_grad_f32(a, b, s1, s2, gout, inv_count, zero_is_positive=False):
    """fm_bwd_kernel's arithmetic in fp32; zero_is_positive: sgn(0) = +1."""
    s1, s2 = F32(s1), F32(s2)
    gs = F32(gout) * F32(inv_count)
    c1, c2 = gs / s2, gs * s1 / (s2 * s2)
    dv = a - b
    if zero_is_positive:
        sg1, sg2 = np.where(dv >= 0, F32(1), F32(-1)), np.where(a >= 0, F32(1), F32(-1))
    else:
        sg1, sg2 = np.sign(dv).astype(F32), np.sign(a).astype(F32)
    return c1 * sg1 - c2 * sg2


def test_fm_gradient_criteria_reject_a_positive_sign_of_zero():
    r = np.random.default_rng(41)
    a, b = r.standard_normal(4101).astype(F32), r.standard_normal(4101).astype(F32)
    b[100:140] = a[100:140]          # a == b
    a[200:230] = 0                   # a == 0
    a[300:310] = 0
    b[300:310] = 0                   # both
    s1, s2, gout, ic = float(F32(0.37 * a.size)), float(F32(0.81 * a.size)), float(F32(0.7)), float(F32(1 / 24))
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    ref, scale = S.fm_grad(ta, tb, s1, s2, gout, ic)
    codes = S.fm_codes(ta, tb).reshape(-1)
    assert len(set(codes.tolist())) == 9              # every combination of the two signs occurs
    good = torch.from_numpy(fm_grad_f32(a, b, s1, s2, gout, ic))
    assert S.pattern_mismatches(S.fm_decode(good, s1, s2, gout, ic), codes) == 0
    assert S.bound_violation(good, ref, S.FM_GRAD_K, scale) <= 1.0
    bad = torch.from_numpy(fm_grad_f32(a, b, s1, s2, gout, ic, zero_is_positive=True))
    assert S.pattern_mismatches(S.fm_decode(bad, s1, s2, gout, ic), codes) == 40 + 30 + 10
    assert S.bound_violation(bad, ref, S.FM_GRAD_K, scale) > 1.0


def hinge_seeds_f32(a, b, gout, scales, swapped=False):
    per = F32(a.size)
    g = [F32(gout) * F32(s) / per for s in scales]
    blocks = [np.zeros(a.size, F32), np.where(F32(1) - a > 0, -g[0], F32(0)), np.where(F32(1) + a > 0, g[1], F32(0)),
              np.where(F32(1) - b > 0, -g[2], F32(0))]
    if swapped:
        blocks[2], blocks[3] = blocks[3], blocks[2]
    return np.concatenate(blocks).astype(F32)


def test_seed_criteria_reject_swapped_blocks():
    r = np.random.default_rng(42)
    a, b = (r.standard_normal(257) * 2).astype(F32), (r.standard_normal(257) * 2).astype(F32)
    a[:3], b[:3] = (1.0, -1.0, 1.0), (-1.0, 1.0, 1.0)          # margins exactly zero
    gout, scales = float(F32(0.9)), tuple(float(F32(s)) for s in (0.25, 0.5, 0.75))
    ref = S.hinge_seeds(torch.from_numpy(a), torch.from_numpy(b), gout, scales)
    good = torch.from_numpy(hinge_seeds_f32(a, b, gout, scales))
    assert S.pattern_mismatches(S.sign_codes(good), S.sign_codes(ref)) == 0
    assert S.bound_violation(good, ref, S.HINGE_GRAD_K, ref.abs()) <= 1.0
    bad = torch.from_numpy(hinge_seeds_f32(a, b, gout, scales, swapped=True))
    assert S.pattern_mismatches(S.sign_codes(bad), S.sign_codes(ref)) > 0
    assert S.bound_violation(bad, ref, S.HINGE_GRAD_K, ref.abs()) > 1.0


def test_bound_violation_is_strict_about_shape_nan_and_zero_bounds():
    ref = torch.tensor([1.0, 0.0, -2.0], dtype=torch.float64)
    assert S.bound_violation(ref.float(), ref, 1, ref.abs()) == 0.0
    assert S.bound_violation(torch.tensor([1.0 + 2.0 ** -23, 0.0, -2.0]), ref, 1, ref.abs()) > 1.0      # two roundings against k = 1
    assert S.bound_violation(torch.tensor([1.0, 1e-30, -2.0]), ref, 1, ref.abs()) == math.inf            # scale 0: exact or nothing
    assert S.bound_violation(torch.tensor([1.0, float("nan"), -2.0]), ref, 1, ref.abs()) == math.inf
    assert S.bound_violation(torch.ones(2), ref, 1, 1.0) == math.inf
