"""GPU: the kernels at the end of every train step through the C ABI -- multi-tensor Adam, the feature-matching sums and gradient
(fp32 tensors and bundle planes), the hinge terms and the stacked backward seeds, the scalar loss totals, the element-wise ops and the
pads -- against the float64 restatements of tests/step_tail_oracle.py, at the sizes where each kernel changes route:

  adam_kernel            4096-element blocks: 16-byte route, tail block, misaligned pointers; tables past one and two 48-tensor chunks
  fm_partial_kernel      slices past 3075 elements (the four-loads-in-flight loop), misaligned (scalar) route, more than 32 pairs
  fm_bwd_kernel          second pass of the two-stride loop, the one-stride remainder, n % 4 tail, small pairs in a large pair's grid
  bl_fm_partial_kernel   more than 256 units per block (the two-unit loop) with and without code planes, more than 32 pairs
  grid-stride kernels    more than 4096 x 256 elements (second pass): hinge seeds, element-wise ops
  reflect_pad_bwd        both fold-back ranges on one element

Outputs live between sentinel margins that must come back untouched; inputs are compared bit for bit with a copy.  Bounds of the
element-wise comparisons are derived in step_tail_oracle.py (k roundings of 2^-24 on the magnitudes entering each operation); the
reductions keep the project's relative tolerances.  Every test prints the worst error it measured as a fraction of its bound.

Measured on an MI355X, worst over the cases, as a fraction of the derived bound (none was widened): Adam exp_avg 0.41, exp_avg_sq 0.47,
update 0.996 (the half ulp of the parameter's own rounding is part of the bound and is attained); FusedAdam over five steps 0.26 / 0.29 /
0.75; fm_bwd 0.31; hinge seeds 0.67; leaky-ReLU 0.99, add 1.0, axpby 0.97, tanh_bwd 0.73; pad adjoint 0.51.  Reductions relative to
float64: fm_sums 1.1e-7, bl_fm_sums 1.2e-7, hinge_fwd 9.9e-8, disc_losses 6.7e-8, stft_loss_total 7.1e-8, tanh_lift 8.9e-8, l2norm 5.8e-8.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import step_tail_oracle as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EINVAL = -1
MARGIN = 64                    # elements of sentinel on each side of an output
SENTINEL = 0x7FC0DEAD          # a quiet NaN with a payload no kernel produces
F32 = np.float32


def f32(x):
    """The fp32 value an entry point receives for a float argument, as a Python float."""
    return float(F32(x))


def stream():
    from vibravox_amd._lib import stream as s

    return s()


class Guarded:
    """`n` elements between two sentinel margins; `offset` more elements in front move the view off its 16-byte alignment."""

    def __init__(self, n, offset=0, dtype=torch.float32):
        self.n, self.lo = n, MARGIN + offset
        if dtype is torch.float32:
            self.full = torch.empty(n + 2 * MARGIN + offset, dtype=torch.int32, device=DEV).fill_(SENTINEL).view(torch.float32)
        else:
            assert dtype is torch.uint8
            self.full = torch.full((n + 2 * MARGIN + offset,), 0xA5, dtype=torch.uint8, device=DEV)
        self.view = self.full[self.lo:self.lo + n]
        self.pattern = self.full.view(torch.int32 if dtype is torch.float32 else torch.uint8)[0].item()

    def set(self, values):
        self.view.copy_(values.reshape(-1))
        return self

    def ptr(self):
        return self.view.data_ptr()

    def bits(self):
        return self.full.view(torch.int32) if self.full.dtype is torch.float32 else self.full

    def margins_intact(self):
        b = self.bits()
        return bool((b[:self.lo] == self.pattern).all()) and bool((b[self.lo + self.n:] == self.pattern).all())

    def untouched(self):
        return bool((self.bits() == self.pattern).all())


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(n, seed, scale=1.0):
    return torch.randn(n, generator=gen(seed), device=DEV) * scale


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def report(what, **figures):
    print(f"[step-tail] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))


# =====================================================================================================================================
# Adam
# =====================================================================================================================================
ADAM_SIZES = (1, 3, 255, 256, 4095, 4096, 4097, 2 * 4096 + 5, 3 * 4096)
CONFIGURED = dict(lr=f32(3e-4), betas=(0.5, f32(0.9)), eps=f32(1e-8))   # optimizer/adam.yaml, as the fp32 values the kernel receives


class AdamTensor:
    """One table entry: guarded p / m / v, a gradient, and copies of all four as they were.  |p| <= ~1e-3 for every second tensor (an
    ulp of p far below the update); a block of g = m = v = 0 in tensors of 255 elements and more."""

    def __init__(self, n, seed, gscale, small, offsets=(0, 0, 0, 0)):
        self.n = n
        p = randn(n, seed, 1e-3 if small else 1.0)
        g = randn(n, seed + 1, gscale)
        m = randn(n, seed + 2, gscale)
        v = randn(n, seed + 3, gscale).square()
        self.zeros = slice(0, 0)
        if n >= 255:
            self.zeros = slice(n // 3, n // 3 + 40)
            for t in (g, m, v):
                t[self.zeros] = 0
        self.p, self.g, self.m, self.v = (Guarded(n, o).set(t) for t, o in zip((p, g, m, v), offsets))
        self.p0, self.g0, self.m0, self.v0 = p, g, m, v

    def entry(self):
        from vibravox_amd._lib import EbenAdamTensor

        return EbenAdamTensor(self.p.ptr(), self.g.ptr(), self.m.ptr(), self.v.ptr(), self.n)

    def unchanged(self):
        return all(same_bits(b.view, t0) and b.margins_intact()
                   for b, t0 in ((self.p, self.p0), (self.g, self.g0), (self.m, self.m0), (self.v, self.v0)))


def adam_table(tensors):
    from vibravox_amd._lib import EbenAdamTensor

    return (EbenAdamTensor * max(1, len(tensors)))(*[t.entry() for t in tensors])


def adam_run_and_check(hip, tensors, step, wd=0.0, gs=1.0, what="adam"):
    lr, betas, eps = CONFIGURED["lr"], CONFIGURED["betas"], CONFIGURED["eps"]
    wd = f32(wd)
    rc = hip.eben_adam_step(adam_table(tensors), len(tensors), max(t.n for t in tensors), lr, betas[0], betas[1], eps, wd, step, gs, stream())
    assert rc == 0
    torch.cuda.synchronize()
    worst = dict(m=0.0, v=0.0, update=0.0)
    for t in tensors:
        assert t.p.margins_intact() and t.m.margins_intact() and t.v.margins_intact() and t.g.margins_intact()
        assert same_bits(t.g.view, t.g0), "the gradient was modified"
        rp, rm, rv = S.adam_step(t.p0, t.m0, t.v0, t.g0, step, lr, betas, eps, wd, gs)
        bm, bv, bu = S.adam_bounds(t.p0, t.m0, t.v0, t.g0, step, lr, betas, eps, wd, gs)
        worst["m"] = max(worst["m"], S.bound_violation(t.m.view, rm, 1, bm / S.U))
        worst["v"] = max(worst["v"], S.bound_violation(t.v.view, rv, 1, bv / S.U))
        # the update p_new - p_old, exact in float64; half an ulp of the parameter for its final rounding
        worst["update"] = max(worst["update"], S.bound_violation(t.p.view.double() - t.p0.double(), rp - t.p0.double(), 1,
                                                                 S.adam_update_bound(t.p0, rp, bu) / S.U))
        if t.zeros.stop > t.zeros.start and wd == 0.0:   # g = m = v = 0 (and no decay): nothing moves, nothing becomes NaN
            assert same_bits(t.p.view[t.zeros], t.p0[t.zeros])
            assert not bool(t.m.view[t.zeros].any()) and not bool(t.v.view[t.zeros].any())
    report(what, **worst)
    assert max(worst.values()) <= 1.0, worst
    return worst


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_single_tensor_sizes(hip, n):
    """One tensor per launch: below a block, exactly one, one and a tail, whole blocks and a tail (2 x 4096 + 5), whole blocks only."""
    adam_run_and_check(hip, [AdamTensor(n, 1000 + n, 1e-2, small=(n % 2 == 1))], step=2, what=f"adam n={n}")


@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq", "all_by_four"])
def test_adam_alignment_routes(hip, which):
    """2 x 4096 + 5 elements with one of the four pointers one float off 16 bytes: the scalar route for the whole blocks too.  All four
    moved by four floats stay aligned: the 16-byte route from an offset base."""
    offsets = dict(param=(1, 0, 0, 0), grad=(0, 1, 0, 0), exp_avg=(0, 0, 1, 0), exp_avg_sq=(0, 0, 0, 1), all_by_four=(4, 4, 4, 4))[which]
    t = AdamTensor(2 * 4096 + 5, 2000, 1e-2, small=True, offsets=offsets)
    for b, o in zip((t.p, t.g, t.m, t.v), offsets):
        assert (b.ptr() % 16 == 0) == (o % 4 == 0)
    adam_run_and_check(hip, [t], step=3, what=f"adam misaligned {which}")


@pytest.mark.parametrize("ntensors", [1, 48, 49, 97])
def test_adam_table_chunks(hip, ntensors):
    """Tables of one chunk, exactly 48, 48 + 1 and 2 x 48 + 1 tensors: the second and third launch read the table from their offset, the
    last chunk is a single tensor, and multi-block tensors sit in the middle of a chunk's block list."""
    tensors = [AdamTensor(ADAM_SIZES[i % len(ADAM_SIZES)], 3000 + 10 * i, 1e-2, small=(i % 2 == 0)) for i in range(ntensors)]
    adam_run_and_check(hip, tensors, step=2, wd=0.01, gs=0.5, what=f"adam table of {ntensors}")


@pytest.mark.parametrize("gscale", [1e-2, 1e-8])
@pytest.mark.parametrize("step,wd,gs", [(1, 0.0, 1.0), (2, 0.01, 1.0), (1000, 0.0, 0.5), (2, 0.01, 0.125), (1000, 0.01, 1.0)])
def test_adam_hyper_parameters(hip, step, wd, gs, gscale):
    """The configured optimiser, weight decay, grad_scale, early and late bias corrections; |g| ~ 1e-8 with v to match, where eps is a
    third of the denominator and its place relative to the bias correction is a 35 % matter."""
    tensors = [AdamTensor(n, 4000 + n, gscale, small=(i % 2 == 0)) for i, n in enumerate(ADAM_SIZES)]
    adam_run_and_check(hip, tensors, step, wd, gs, what=f"adam step={step} wd={wd} gs={gs} |g|~{gscale}")


def test_adam_rejects_bad_tables_before_any_launch(hip):
    """ntensors = 0, step = 0, and a null pointer or an empty tensor in entry 50 (the second chunk): EBEN_EINVAL and not one element
    of any tensor stepped -- the first chunk included."""
    tensors = [AdamTensor(ADAM_SIZES[i % 5], 5000 + 10 * i, 1e-2, small=False) for i in range(60)]
    lr, (b1, b2), eps = CONFIGURED["lr"], CONFIGURED["betas"], CONFIGURED["eps"]

    def call(table, n, step):
        rc = hip.eben_adam_step(table, n, 4097, lr, b1, b2, eps, 0.0, step, 1.0, stream())
        torch.cuda.synchronize()
        return rc

    assert call(adam_table(tensors), 0, 1) == EINVAL
    assert call(adam_table(tensors), 60, 0) == EINVAL
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        table = adam_table(tensors)
        setattr(table[50], field, None)
        assert call(table, 60, 1) == EINVAL
    table = adam_table(tensors)
    table[50].numel = 0
    assert call(table, 60, 1) == EINVAL
    assert all(t.unchanged() for t in tensors)
    assert call(adam_table(tensors), 60, 1) == 0          # and the same table, whole, steps
    assert not any(same_bits(t.p.view, t.p0) for t in tensors)


def fused_adam_shapes():
    shapes = [(n,) for n in ADAM_SIZES] + [(33, 5, 3), (64, 65), (1, 1, 1), (17, 241), (4096, 2), (3, 4097)]
    while len(shapes) < 60:
        shapes.append((7 + 13 * len(shapes),))
    return shapes


def test_fused_adam_follows_float64_adam_for_five_steps(hip):
    """FusedAdam against torch.optim.Adam in float64 (given the same fp32 hyper-parameters and the gradient already scaled): 60
    parameters, one a view one float into its storage, a fresh gradient every step, one of them not contiguous, one parameter without a
    gradient on step 2 (from then on the parameters are at two step counts: the by_step route), weight decay and grad_scale.  The moments
    and the accumulated update are held, element by element, to the per-step bounds of the oracle carried through the five steps."""
    from vibravox_amd.optim import FusedAdam

    lr, betas, eps, wd, gs = CONFIGURED["lr"], CONFIGURED["betas"], CONFIGURED["eps"], f32(0.01), 0.5
    shapes = fused_adam_shapes()
    params = []
    for i, s in enumerate(shapes):
        n = math.prod(s)
        init = randn(n, 6000 + i, 1e-3 if i % 2 else 1.0)
        if i == 7:   # 2 x 4096 + 5 elements one float into a larger buffer
            store = torch.zeros(n + 1, device=DEV)
            store[1:] = init
            p = store[1:].view(s).requires_grad_(True)
            assert p.data_ptr() % 16 == 4
        else:
            p = init.view(s).clone().requires_grad_(True)
        params.append(p)
    p_start = [p.detach().clone() for p in params]
    ref = [p.detach().double().clone().requires_grad_(True) for p in params]
    ours = FusedAdam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    theirs = torch.optim.Adam(ref, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    skipped, strided = 12, 10                                    # (17, 241) sits out step 2; (64, 65) gets a transposed gradient
    err = [dict(p=torch.zeros_like(r), m=torch.zeros_like(r), v=torch.zeros_like(r)) for r in ref]
    count = [0] * len(params)
    for step in range(1, 6):
        for i, (p, r) in enumerate(zip(params, ref)):
            if step == 2 and i == skipped:
                p.grad = r.grad = None
                continue
            if i == strided:
                g = randn(p.numel(), 7000 + 100 * step + i, 1e-2).view(p.shape[1], p.shape[0]).t()
                assert not g.is_contiguous()
            else:
                g = randn(p.numel(), 7000 + 100 * step + i, 1e-2).view(p.shape)
            p.grad, r.grad = g, g.double() * gs
            # the oracle's own step from the float64 state, and the bound this fp32 step adds to the errors carried so far
            count[i] += 1
            st = theirs.state[r] if r in theirs.state and len(theirs.state[r]) else None
            m = st["exp_avg"] if st else torch.zeros_like(r)
            v = st["exp_avg_sq"] if st else torch.zeros_like(r)
            bm, bv, bu = S.adam_bounds(r, m, v, g, count[i], lr, betas, eps, wd, gs, err[i]["p"], err[i]["m"], err[i]["v"])
            rp = S.adam_step(r, m, v, g, count[i], lr, betas, eps, wd, gs)[0]
            err[i]["rp"] = rp
            err[i]["m"], err[i]["v"] = bm, bv
            err[i]["p"] = err[i]["p"] + S.adam_update_bound(r, rp, bu)
        ours.step(grad_scale=gs)
        theirs.step()
        for i, r in enumerate(ref):   # the restatement and torch agree in float64
            if not (step == 2 and i == skipped):
                assert float((err[i]["rp"] - r.detach()).abs().max()) <= 1e-13 * float(r.detach().abs().max())
    assert int(ours.state[params[skipped]]["step"]) == 4 and int(ours.state[params[0]]["step"]) == 5
    worst = dict(m=0.0, v=0.0, update=0.0, update_rel=0.0)
    for i, (p, r) in enumerate(zip(params, ref)):
        so, st = ours.state[p], theirs.state[r]
        worst["m"] = max(worst["m"], S.bound_violation(so["exp_avg"], st["exp_avg"], 1, err[i]["m"] / S.U))
        worst["v"] = max(worst["v"], S.bound_violation(so["exp_avg_sq"], st["exp_avg_sq"], 1, err[i]["v"] / S.U))
        du_got, du_ref = p.detach().double() - p_start[i].double(), r.detach() - p_start[i].double()
        worst["update"] = max(worst["update"], S.bound_violation(du_got, du_ref, 1, err[i]["p"] / S.U))
        worst["update_rel"] = max(worst["update_rel"], float((du_got - du_ref).norm() / du_ref.norm()))
    report("FusedAdam, 5 steps", **worst)
    # (update_rel, the norm of the error over the norm of the update, is printed for the record: five roundings of |p| ~ 1 against an
    # update of a few lr; the assertion is the element-wise bound)
    assert max(worst["m"], worst["v"], worst["update"]) <= 1.0, worst


def test_fused_adam_state_dict_interchange(hip):
    """After two steps FusedAdam's state dict goes into a float32 torch.optim.Adam over copies of its parameters and the reverse; each
    pair then takes one more step from identical states.  Both sides of a pair are held to the one-step fp32 bound against the float64
    step from that state, so they differ by the roundings of one step and nothing else (a lost step count or a stale moment is O(1))."""
    import copy

    from vibravox_amd.optim import FusedAdam

    lr, betas, eps, wd = CONFIGURED["lr"], CONFIGURED["betas"], CONFIGURED["eps"], f32(0.01)
    shapes = [(4097,), (33, 5, 3), (2 * 4096 + 5,), (1,)]

    def grads(step):
        return [randn(math.prod(s), 8100 + 10 * step + i, 1e-2).view(s) for i, s in enumerate(shapes)]

    a = [randn(math.prod(s), 8000 + i, 1e-3 if i % 2 else 1.0).view(s).clone().requires_grad_(True) for i, s in enumerate(shapes)]
    b = [p.detach().clone().requires_grad_(True) for p in a]
    fused = FusedAdam(a, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    plain = torch.optim.Adam(b, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    for step in (1, 2):
        for p, q, g in zip(a, b, grads(step)):
            p.grad, q.grad = g.clone(), g.clone()
        fused.step()
        plain.step()
    a2 = [p.detach().clone().requires_grad_(True) for p in a]     # torch's Adam continues FusedAdam's run
    plain2 = torch.optim.Adam(a2, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    plain2.load_state_dict(copy.deepcopy(fused.state_dict()))
    b2 = [q.detach().clone().requires_grad_(True) for q in b]     # FusedAdam continues torch's run
    fused2 = FusedAdam(b2, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    fused2.load_state_dict(copy.deepcopy(plain.state_dict()))
    worst = dict(fused=0.0, plain=0.0, pair=0.0)
    for ours, theirs, po, pt in ((fused, plain2, a, a2), (fused2, plain, b2, b)):
        before = [(p.detach().clone(), ours.state[p]["exp_avg"].clone(), ours.state[p]["exp_avg_sq"].clone()) for p in po]
        for p, q, (p0, m0, v0) in zip(po, pt, before):   # identical states on both sides
            assert same_bits(q.detach(), p0) and same_bits(theirs.state[q]["exp_avg"], m0) and same_bits(theirs.state[q]["exp_avg_sq"], v0)
            assert int(ours.state[p]["step"]) == 2 and int(theirs.state[q]["step"]) == 2
        gl = grads(3)
        for p, q, g in zip(po, pt, gl):
            p.grad, q.grad = g.clone(), g.clone()
        ours.step()
        theirs.step()
        for p, q, g, (p0, m0, v0) in zip(po, pt, gl, before):
            rp, rm, rv = S.adam_step(p0, m0, v0, g, 3, lr, betas, eps, wd)
            bm, bv, bu = S.adam_bounds(p0, m0, v0, g, 3, lr, betas, eps, wd)
            bp = S.adam_update_bound(p0, rp, bu)
            for name, opt, x in (("fused", ours, p), ("plain", theirs, q)):
                worst[name] = max(worst[name], S.bound_violation(opt.state[x]["exp_avg"], rm, 1, bm / S.U),
                                  S.bound_violation(opt.state[x]["exp_avg_sq"], rv, 1, bv / S.U),
                                  S.bound_violation(x.detach().double() - p0.double(), rp - p0.double(), 1, bp / S.U))
            worst["pair"] = max(worst["pair"], S.bound_violation(p.detach(), q.detach().double(), 2, bp / S.U))
    report("Adam state dict interchange", **worst)
    assert max(worst.values()) <= 1.0, worst


# =====================================================================================================================================
# feature matching over bundle planes (ahead of the fp32 section: its large case and that section's pool are not live together)
# =====================================================================================================================================
def bl_planes(half, channels, length, seed):
    """Planes of a (2 half, C, L) embedding with runs of a == r, a == 0 and both; and the fp32 values hi + lo the kernels form."""
    from vibravox_amd.disc_engine_bl import Planes

    x = randn(2 * half * channels * length, seed).view(2 * half, channels, length)
    a, r = x[:half].reshape(-1), x[half:].reshape(-1)
    if a.numel() >= 255 * 8:
        plant(a, r)          # views of x: planted in place
    elif seed % 3 == 0:
        r[:3] = a[:3]
    elif seed % 3 == 1:
        a[2:5] = 0
    else:
        a[1:3] = 0
        r[1:3] = 0
    p = Planes.from_f32(x)
    val = (p.hi.float() + p.lo.float()).permute(0, 1, 3, 2).reshape(2 * half, channels, length)   # one exact-order fp32 add, as the kernel's
    return p, val


def bl_run(hip, planes, half, with_codes):
    k = len(planes)
    ptrs = (ctypes.c_void_p * (2 * k))(*[q for p in planes for q in (p.hi.data_ptr(), p.lo.data_ptr())])
    units = (ctypes.c_int64 * k)(*[half * (p.channels // 8) * p.length for p in planes])
    ws_bytes = hip.eben_bl_fm_sums_workspace(k)
    ws, sums = Guarded(ws_bytes // 4), Guarded(2 * k)
    codes = [Guarded(8 * units[i], dtype=torch.uint8) for i in range(k)] if with_codes else None
    if with_codes:
        cp = (ctypes.c_void_p * k)(*[c.ptr() for c in codes])
        rc = hip.eben_bl_fm_sums_codes(ptrs, units, cp, k, ws.ptr(), ws_bytes, sums.ptr(), stream())
    else:
        rc = hip.eben_bl_fm_sums(ptrs, units, k, ws.ptr(), ws_bytes, sums.ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert ws.margins_intact() and sums.margins_intact() and (not with_codes or all(c.margins_intact() for c in codes))
    return sums.view.clone(), codes


def bl_check(hip, shapes, half, what):
    made = [bl_planes(half, c, l, 9500 + 7 * i) for i, (c, l) in enumerate(shapes)]
    planes = [m[0] for m in made]
    copies = [(p.hi.clone(), p.lo.clone()) for p in planes]
    plain, _ = bl_run(hip, planes, half, False)
    coded, codes = bl_run(hip, planes, half, True)
    assert same_bits(plain, coded)                              # the code planes change nothing in the sums
    assert all(torch.equal(p.hi, h) and torch.equal(p.lo, l) for p, (h, l) in zip(planes, copies))
    worst, wrong, seen = 0.0, 0, set()
    got = coded.cpu().double()
    for i, (p, val) in enumerate(made):
        a, r = val[:half], val[half:]
        r1, r2 = S.fm_sums(a, r)
        worst = max(worst, S.rel_sum_error(got[2 * i], r1) if r1 else abs(float(got[2 * i])), S.rel_sum_error(got[2 * i + 1], r2) if r2 else abs(float(got[2 * i + 1])))
        want = S.bl_fm_code(a, r)                               # (half, C, L) -> the plane's (half, C / 8, L, 8)
        want = want.reshape(half, p.channels // 8, 8, p.length).permute(0, 1, 3, 2).reshape(-1)
        wrong += S.pattern_mismatches(codes[i].view, want)
        seen |= set(torch.unique(want).tolist())
    report(what, worst_relative=worst, code_mismatches=wrong)
    assert wrong == 0
    assert worst < 2e-5            # the project's tolerance (test_feature_matching_sums_over_planes)
    return seen


@pytest.mark.parametrize("half,channels,length", [(1, 8, 1), (1, 8, 255), (3, 40, 17), (1, 8, 257), (3, 768, 2134)])
def test_bl_fm_sums_and_codes(hip, half, channels, length):
    """1, 255, 255 (over three rows and five bundles), 257 and 614 592 units: at the last, 601 units per block -- every thread takes the
    two-unit loop, the first 89 of a block the one-unit loop after it, and the last block is ragged."""
    units = half * (channels // 8) * length
    if units > 1024 * 513:
        assert units % 1024 != 0
    seen = bl_check(hip, [(channels, length)], half, f"bl_fm_sums {units} units")
    if units >= 255:
        assert seen == {0, 1, 2, 4, 5, 6, 8, 9, 10}            # all nine codes, the planted zeros among them


def test_bl_fm_sums_33_pairs(hip):
    """33 small pairs: the second launch writes its partial sums and sums[] from its offset."""
    shapes = [((8, 16, 24, 40)[i % 4], (1, 31, 64, 101, 257)[i % 5]) for i in range(33)]
    bl_check(hip, shapes, 2, "bl_fm_sums 33 pairs")


# =====================================================================================================================================
# feature matching on fp32 tensors
# =====================================================================================================================================
FM_VEC2 = 1024 * 8192            # two full iterations of the four-loads-in-flight loop in every block
FM_RAGGED = 1024 * 4100 + 7      # one vector iteration for part of a block, then the scalar loop; ragged last slice; n % 4 = 3
FM_SMALL = (1, 3, 4, 1023, 4 * 1024 + 1)
CHUNK = 1 << 20


def plant(a, b):
    """Runs on the decision points, periodic over the tensor: a == b, a == 0, and both."""
    n = a.numel()
    idx = torch.arange(n, device=a.device)
    eq, za, both = (idx % 997) < 5, (idx % 1009 >= 20) & (idx % 1009 < 24), (idx % 2003 >= 40) & (idx % 2003 < 43)
    b[eq] = a[eq]
    a[za] = 0
    a[both] = 0
    b[both] = 0


@pytest.fixture(scope="module")
def fm_pool():
    """Two 33.5 MB embeddings every large pair is a slice of, their copies, and one guarded gradient buffer of that size."""
    n = FM_VEC2 + 16
    a, b = randn(n, 9000), randn(n, 9001)
    plant(a, b)
    # the same decision points for a pair whose a starts one float into the pool: b[i] == a[i + 1], and zeros at both
    idx = torch.arange(n - 1, device=DEV)
    eq, both = idx[(idx % 997 >= 500) & (idx % 997 < 505)], idx[(idx % 2003 >= 100) & (idx % 2003 < 103)]
    b[eq] = a[eq + 1]
    a[both + 1] = 0
    b[both] = 0
    pool = dict(a=a, b=b, a0=a.clone(), b0=b.clone(), da=Guarded(n))
    yield pool
    pool.clear()
    torch.cuda.empty_cache()


class FmPair:
    def __init__(self, a, b, da):
        self.a, self.b, self.da, self.n = a, b, da, a.numel()


def small_pair(i, n):
    a, b = randn(n, 9100 + 2 * i), randn(n, 9101 + 2 * i)
    if n >= 1023:
        plant(a, b)
    elif i % 3 == 0:
        b[0] = a[0]
    elif i % 3 == 1:
        a[0] = 0
    else:
        a[0] = b[0] = 0
    return FmPair(a, b, Guarded(n))


def big_pair(pool, n, a_offset=0):
    return FmPair(pool["a"][a_offset:a_offset + n], pool["b"][:n], pool["da"])


def fm_launch(pool, name):
    small = lambda i: small_pair(i, FM_SMALL[i % len(FM_SMALL)])
    if name == "1_pair_two_vector_iterations":
        return [big_pair(pool, FM_VEC2)]
    if name == "1_pair_misaligned":
        return [big_pair(pool, FM_RAGGED, a_offset=1)]
    if name == "32_pairs":               # exactly one full launch; the large pair's grid also serves 1-, 3-, 4-, 1023-element pairs
        return [big_pair(pool, FM_RAGGED) if i == 5 else small(i) for i in range(32)]
    if name == "33_pairs":               # the second launch is one misaligned pair
        av, bq = randn(4097, 9300), randn(4097, 9301)
        plant(av, bq)
        store = torch.empty(4098, device=DEV)
        store[1:] = av
        return [small(i) for i in range(32)] + [FmPair(store[1:], bq, Guarded(4097))]
    if name == "40_pairs":               # the large pair in the second launch (pairs 32 .. 39: 4, 1023, 4097, large, 3, 4, 1023, 4097)
        return [big_pair(pool, FM_RAGGED) if i == 35 else small(i) for i in range(40)]
    raise KeyError(name)


def fm_ref_sums(p):
    s1 = s2 = 0.0
    for i in range(0, p.n, CHUNK):
        c1, c2 = S.fm_sums(p.a[i:i + CHUNK], p.b[i:i + CHUNK])
        s1, s2 = s1 + c1, s2 + c2
    return s1, s2


FM_LAUNCHES = ["1_pair_two_vector_iterations", "1_pair_misaligned", "32_pairs", "33_pairs", "40_pairs"]


@pytest.mark.parametrize("name", FM_LAUNCHES)
def test_fm_sums(hip, fm_pool, name):
    pairs = fm_launch(fm_pool, name)
    k = len(pairs)
    if name == "1_pair_misaligned":
        assert pairs[0].a.data_ptr() % 16 == 4 and pairs[0].b.data_ptr() % 16 == 0
    if name == "33_pairs":
        assert pairs[32].a.data_ptr() % 16 == 4
    ptrs = (ctypes.c_void_p * (2 * k))(*[q for p in pairs for q in (p.a.data_ptr(), p.b.data_ptr())])
    numel = (ctypes.c_int64 * k)(*[p.n for p in pairs])
    ws_bytes = hip.eben_fm_sums_workspace(k)
    assert ws_bytes == 4 * 2 * 1024 * k
    ws, sums = Guarded(ws_bytes // 4), Guarded(2 * k)
    small_copies = [(p.a.clone(), p.b.clone()) for p in pairs if p.n <= 8192]
    assert hip.eben_fm_sums(ptrs, numel, k, ws.ptr(), ws_bytes, sums.ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert ws.margins_intact() and sums.margins_intact()
    assert same_bits(fm_pool["a"], fm_pool["a0"]) and same_bits(fm_pool["b"], fm_pool["b0"])
    assert all(same_bits(p.a, ca) and same_bits(p.b, cb) for p, (ca, cb) in zip([p for p in pairs if p.n <= 8192], small_copies))
    got = sums.view.cpu().double()
    worst = 0.0
    for i, p in enumerate(pairs):
        r1, r2 = fm_ref_sums(p)
        worst = max(worst, S.rel_sum_error(got[2 * i], r1) if r1 else abs(float(got[2 * i])), S.rel_sum_error(got[2 * i + 1], r2) if r2 else abs(float(got[2 * i + 1])))
    report(f"fm_sums {name}", worst_relative=worst)
    assert worst < 1e-5           # the project's tolerance for these sums (test_feature_and_hinge_losses)
    assert hip.eben_fm_sums(ptrs, numel, k, ws.ptr(), ws_bytes - 4, sums.ptr(), stream()) == -2   # EBEN_EWORKSPACE


@pytest.mark.parametrize("name", FM_LAUNCHES)
def test_fm_gradient(hip, fm_pool, name):
    """eben_fm_bwd with sums, gout and inv_count chosen here (different sums for every pair, so a launch that reads another pair's sums
    shows): the pattern of the two signs exact on every element, the values within five roundings of |c1| + |c2|."""
    fm_pool["da"].bits().fill_(SENTINEL)
    pairs = fm_launch(fm_pool, name)
    k = len(pairs)
    gout, inv_count = f32(0.7), f32(1.0 / 24)
    sums_host = np.array([[0.37 * p.n * (1 + 0.01 * i), 0.81 * p.n * (1 + 0.013 * i)] for i, p in enumerate(pairs)], F32)
    sums = torch.from_numpy(sums_host.reshape(-1)).to(DEV)
    gout_dev = torch.tensor([gout], device=DEV)
    ptrs = (ctypes.c_void_p * (2 * k))(*[q for p in pairs for q in (p.a.data_ptr(), p.b.data_ptr())])
    da = (ctypes.c_void_p * k)(*[p.da.ptr() for p in pairs])
    numel = (ctypes.c_int64 * k)(*[p.n for p in pairs])
    sums_copy = sums.clone()
    assert hip.eben_fm_bwd(ptrs, da, numel, k, sums.data_ptr(), gout_dev.data_ptr(), inv_count, stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(fm_pool["a"], fm_pool["a0"]) and same_bits(fm_pool["b"], fm_pool["b0"]) and same_bits(sums, sums_copy)
    worst, wrong, seen = 0.0, 0, set()
    for i, p in enumerate(pairs):
        s1, s2 = float(sums_host[i, 0]), float(sums_host[i, 1])
        b = p.da.bits()
        assert bool((b[:p.da.lo] == SENTINEL).all()) and bool((b[p.da.lo + p.n:] == SENTINEL).all())   # the shared buffer: all that follows
        for j in range(0, p.n, CHUNK):
            a_, b_, g_ = p.a[j:j + CHUNK], p.b[j:j + CHUNK], p.da.view[:p.n][j:j + CHUNK]
            ref, scale = S.fm_grad(a_, b_, s1, s2, gout, inv_count)
            codes = S.fm_codes(a_, b_)
            wrong += S.pattern_mismatches(S.fm_decode(g_, s1, s2, gout, inv_count), codes)
            worst = max(worst, S.bound_violation(g_, ref, S.FM_GRAD_K, scale))
            if p.n >= 1023:
                seen |= set(torch.unique(codes).tolist())
    report(f"fm_bwd {name}", worst_of_bound=worst, pattern_mismatches=wrong)
    assert wrong == 0 and worst <= 1.0
    assert len(seen) == 9                                      # every combination of sgn(a - b) and sgn(a) was exercised


def test_fm_rejects_an_empty_pair(hip):
    a, b, da = randn(8, 9400), randn(8, 9401), Guarded(8)
    ptrs = (ctypes.c_void_p * 4)(a.data_ptr(), b.data_ptr(), a.data_ptr(), None)
    numel = (ctypes.c_int64 * 2)(8, 8)
    ws, sums = Guarded(4096), Guarded(4)
    assert hip.eben_fm_sums(ptrs, numel, 2, ws.ptr(), 4 * 4096, sums.ptr(), stream()) == EINVAL
    dap = (ctypes.c_void_p * 2)(da.ptr(), da.ptr())
    s = torch.ones(4, device=DEV)
    assert hip.eben_fm_bwd(ptrs, dap, numel, 2, s.data_ptr(), s.data_ptr(), 1.0, stream()) == EINVAL
    torch.cuda.synchronize()
    assert sums.untouched() and da.untouched()


# =====================================================================================================================================
# hinge
# =====================================================================================================================================
def logits(n, seed):
    x = randn(n, seed, 1.5)
    for i, v in enumerate((1.0, -1.0, 1.0, -1.0)[:min(n, 4)]):      # margins exactly zero for one target or the other
        x[(i * 61) % n] = v
    if n == 1:
        x[0] = 1.0 if seed % 2 else -1.0
    return x


HINGE_FWD_N = (1, 255, 256, 257, 8001)


def test_hinge_forward_single_and_multi(hip):
    xs = [logits(n, 9600 + i) for i, n in enumerate(HINGE_FWD_N)]
    copies = [x.clone() for x in xs]
    terms = [(x, t) for x in xs for t in (1.0, -1.0)]
    single, worst = [], 0.0
    for x, t in terms:
        out = Guarded(1)
        assert hip.eben_hinge_fwd(x.data_ptr(), x.numel(), t, out.ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert out.margins_intact()
        ref = S.hinge_mean(x, t)
        worst = max(worst, S.rel_sum_error(out.view.item(), ref) if ref else abs(out.view.item()))
        single.append(out.view.clone())
    report("hinge_fwd", worst_relative=worst)
    assert worst < 1e-5            # the project's tolerance for the hinge terms (test_feature_and_hinge_losses)

    def multi(term_list, out):
        k = len(term_list)
        ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x, _ in term_list])
        numel = (ctypes.c_int64 * k)(*[x.numel() for x, _ in term_list])
        targets = (ctypes.c_float * k)(*[t for _, t in term_list])
        rc = hip.eben_hinge_fwd_multi(ptrs, numel, targets, k, out.ptr(), stream())
        torch.cuda.synchronize()
        return rc

    out = Guarded(len(terms))
    assert multi(terms, out) == 0 and out.margins_intact()
    assert same_bits(out.view, torch.cat(single))                # the single-term kernel's summation order
    full = (terms * 4)[:32]
    out = Guarded(32)
    assert multi(full, out) == 0 and out.margins_intact()
    assert same_bits(out.view, torch.cat((single * 4)[:32]))
    out = Guarded(33)
    assert multi((terms * 4)[:33], out) == EINVAL and out.untouched()
    assert all(same_bits(x, c) for x, c in zip(xs, copies))


def check_seeds(got, ref, what):
    wrong = S.pattern_mismatches(S.sign_codes(got), S.sign_codes(ref))
    worst = S.bound_violation(got, ref, S.HINGE_GRAD_K, ref.abs())
    report(what, worst_of_bound=worst, pattern_mismatches=wrong)
    assert wrong == 0 and worst <= 1.0


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 257])
def test_hinge_backward(hip, n):
    """Past 4096 x 256 elements the grid-stride loop takes a second pass (257 elements of it)."""
    x = logits(n, 9700)
    x0 = x.clone()
    gout, scale = f32(0.9), f32(1.3)
    g = torch.tensor([gout], device=DEV)
    for target in (1.0, -1.0):
        dx = Guarded(n)
        assert hip.eben_hinge_bwd(x.data_ptr(), n, target, g.data_ptr(), scale, dx.ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert dx.margins_intact() and same_bits(x, x0)
        check_seeds(dx.view, S.hinge_grad(x, target, gout, scale), f"hinge_bwd n={n} target={target:+.0f}")


@pytest.mark.parametrize("per", [1, 257, 262144 + 3])
def test_hinge_backward_stacked(hip, per):
    """[0 | hinge'(a, +1) s0 | hinge'(a, -1) s1 | hinge'(b, +1) s2]: bit for bit a zero block and three eben_hinge_bwd calls, and the
    float64 pattern; 4 x (262 144 + 3) elements is twelve past the grid cap."""
    a, b = logits(per, 9800), logits(per, 9801)
    a0, b0 = a.clone(), b.clone()
    gout, scales = f32(0.9), (f32(0.25), f32(0.5), f32(0.75))
    g = torch.tensor([gout], device=DEV)
    seeds = Guarded(4 * per)
    assert hip.eben_hinge_bwd_stacked(a.data_ptr(), b.data_ptr(), per, g.data_ptr(), *scales, seeds.ptr(), stream()) == 0
    parts = [torch.zeros(per, device=DEV)]
    for x, target, s in ((a, 1.0, scales[0]), (a, -1.0, scales[1]), (b, 1.0, scales[2])):
        dx = Guarded(per)
        assert hip.eben_hinge_bwd(x.data_ptr(), per, target, g.data_ptr(), s, dx.ptr(), stream()) == 0
        parts.append(dx.view)
    torch.cuda.synchronize()
    assert seeds.margins_intact() and same_bits(a, a0) and same_bits(b, b0)
    assert same_bits(seeds.view, torch.cat(parts))
    check_seeds(seeds.view, S.hinge_seeds(a, b, gout, scales), f"hinge_bwd_stacked per={per}")


# =====================================================================================================================================
# scalar totals
# =====================================================================================================================================
@pytest.mark.parametrize("nchains", [1, 4])
@pytest.mark.parametrize("npairs", [1, 28, 64, 65])
def test_disc_losses(hip, npairs, nchains):
    sums = torch.rand(2 * npairs, generator=gen(9900 + npairs), device=DEV) * 1e4 + 10.0
    hinge = torch.rand(3 * nchains, generator=gen(9901 + nchains), device=DEV) * 2
    inv_count = f32(1.0 / 24)
    out = Guarded(4)
    assert hip.eben_disc_losses(sums.data_ptr(), npairs, inv_count, hinge.data_ptr(), nchains, out.ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert out.margins_intact()
    ref = S.disc_losses(sums, inv_count, hinge)
    worst = float(((out.view.double() - ref).abs() / ref.abs()).max())
    report(f"disc_losses {npairs} pairs {nchains} chains", worst_relative=worst)
    assert worst < 1e-6


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [1, 3, 6])
def test_stft_loss_total(hip, n, rows):
    sums = [torch.rand(rows, 3, generator=gen(9950 + 10 * i + rows), device=DEV) * 100 + 1.0 for i in range(n)]
    inv_counts = [f32(1.0 / (rows * (257 << i) * (40 + i))) for i in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in sums])
    ic = (ctypes.c_float * n)(*inv_counts)
    out = Guarded(1)
    assert hip.eben_stft_loss_total(ptrs, ic, n, rows, out.ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert out.margins_intact()
    ref = S.stft_loss_total(sums, inv_counts)
    worst = S.rel_sum_error(out.view.item(), ref)
    report(f"stft_loss_total {n} resolutions {rows} rows", worst_relative=worst)
    assert worst < 1e-6


# =====================================================================================================================================
# element-wise ops and pads
# =====================================================================================================================================
EW_SIZES = (1, 257, 4096 * 256 + 3)       # the last: three elements in the second grid-stride pass
EDGES = (0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -126))


def with_edges(x, shift=0):
    """+-0, denormals and the smallest normal planted at a few places (a one-element tensor gets one of them)."""
    n = x.numel()
    for i, v in enumerate(EDGES):
        if n > 6:
            x[(37 * i + shift) % n] = v
            x[n - 1 - ((11 * i + shift) % 7)] = v
    if n == 1:
        x[0] = EDGES[shift % len(EDGES)]
    return x


def check_bound(got, ref, k, scale, what):
    worst = S.bound_violation(got, ref, k, scale, S.TINY)
    report(what, worst_of_bound=worst, worst_in_roundings=S.worst_error(got, ref, scale))
    assert worst <= 1.0


@pytest.mark.parametrize("n", EW_SIZES)
def test_leaky_relu_add_axpby_tanh_bwd(hip, n):
    x, y = with_edges(randn(n, 10000)), with_edges(randn(n, 10001), shift=1)
    if n == 1:
        x[0] = -0.0
    x0, y0 = x.clone(), y.clone()
    st = stream()
    for slope in (f32(0.01), f32(0.2)):
        out = Guarded(n)
        assert hip.eben_lrelu_fwd(x.data_ptr(), out.ptr(), n, slope, st) == 0
        ref = S.leaky_relu(x, slope)
        check_bound(out.view, ref, 1, ref, f"lrelu_fwd n={n} slope={slope:.2f}")          # one product
        assert out.margins_intact()
        out = Guarded(n)
        assert hip.eben_lrelu_bwd(y.data_ptr(), x.data_ptr(), out.ptr(), n, slope, st) == 0
        ref = S.leaky_relu_grad(y, x, slope)
        check_bound(out.view, ref, 1, ref, f"lrelu_bwd n={n} slope={slope:.2f}")          # one product; ref = +-0 takes the slope
        assert out.margins_intact()
    out = Guarded(n)
    assert hip.eben_add(x.data_ptr(), y.data_ptr(), out.ptr(), n, st) == 0
    ref = x.double() + y.double()
    check_bound(out.view, ref, 1, ref, f"add n={n}")                                     # one sum
    assert out.margins_intact()
    alpha, beta = f32(0.7), f32(-1.3)
    out = Guarded(n)
    assert hip.eben_axpby(x.data_ptr(), alpha, y.data_ptr(), beta, out.ptr(), n, st) == 0
    ref, scale = S.axpby(x, alpha, y, beta)
    check_bound(out.view, ref, 2, scale, f"axpby n={n}")                                 # two products and a sum, or a product and an fma
    assert out.margins_intact()
    o = torch.tanh(randn(n, 10002, 2.0))
    if n > 6:
        o[:4] = torch.tensor([1.0, -1.0, 0.0, 1.0 - 2.0 ** -24], device=DEV)            # saturated outputs: 1 - o^2 = 0 or one ulp
    o0 = o.clone()
    out = Guarded(n)
    assert hip.eben_tanh_bwd(y.data_ptr(), o.data_ptr(), out.ptr(), n, st) == 0
    ref, scale = S.tanh_grad(y, o)
    check_bound(out.view, ref, 1, scale, f"tanh_bwd n={n}")                              # o o, 1 - ., the product: the scale carries the chain
    assert out.margins_intact()
    assert same_bits(x, x0) and same_bits(y, y0) and same_bits(o, o0)


@pytest.mark.parametrize("length", [1, 1001])
@pytest.mark.parametrize("c_lift", [0, 1, 2, 4])
def test_tanh_lift(hip, c_lift, length):
    """c_lift = 0 is accepted with a null lift (include/eben_hip.h asks for a lift only when c_lift > 0): plain tanh."""
    batch, channels = 3, 4
    x = randn(batch * channels * length, 10100, 1.5).view(batch, channels, length)
    lift = randn(batch * max(c_lift, 1) * length, 10101).view(batch, max(c_lift, 1), length) if c_lift else None
    out = Guarded(x.numel())
    assert hip.eben_tanh_lift_fwd(x.data_ptr(), lift.data_ptr() if c_lift else None, out.ptr(), batch, channels, c_lift, length, stream()) == 0
    torch.cuda.synchronize()
    assert out.margins_intact()
    ref = S.tanh_lift(x, lift, c_lift).reshape(-1)
    worst = float((out.view.double() - ref).abs().max() / ref.abs().max())
    report(f"tanh_lift c_lift={c_lift} length={length}", worst_relative=worst)
    assert worst < 1e-5            # the project's tolerance (test_elementwise_and_pad)
    bad = Guarded(x.numel())
    assert hip.eben_tanh_lift_fwd(x.data_ptr(), None, bad.ptr(), batch, channels, channels + 1, length, stream()) == EINVAL
    if c_lift:
        assert hip.eben_tanh_lift_fwd(x.data_ptr(), None, bad.ptr(), batch, channels, c_lift, length, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bad.untouched()


@pytest.mark.parametrize("lx,pl,pr", [(2, 1, 1), (3, 2, 2), (5, 0, 4), (5, 4, 0), (1001, 7, 3), (17, 16, 16), (9, 8, 8)])
def test_reflect_pad_and_adjoint(hip, lx, pl, pr):
    """Pads up to lx - 1 on either side (the largest nn.ReflectionPad1d takes and the entry point accepts); in (3, 2, 2), (17, 16, 16)
    and (9, 8, 8) both fold-back ranges of the adjoint land on the same elements.  lx itself is refused."""
    rows, ly = 3, lx + pl + pr
    x = randn(rows * lx, 10200).view(rows, lx)
    x0 = x.clone()
    y = Guarded(rows * ly)
    assert hip.eben_reflect_pad_fwd(x.data_ptr(), y.ptr(), rows, lx, pl, pr, stream()) == 0
    torch.cuda.synchronize()
    assert y.margins_intact() and same_bits(x, x0)
    assert same_bits(y.view.view(rows, ly), S.reflect_pad(x, pl, pr))                   # a copy: exact
    dy = randn(rows * ly, 10201).view(rows, ly)
    dy0 = dy.clone()
    dx = Guarded(rows * lx)
    assert hip.eben_reflect_pad_bwd(dy.data_ptr(), dx.ptr(), rows, lx, pl, pr, stream()) == 0
    torch.cuda.synchronize()
    assert dx.margins_intact() and same_bits(dy, dy0)
    ref = S.reflect_pad_adjoint(dy, lx, pl, pr)
    scale = S.reflect_pad_adjoint(dy.abs(), lx, pl, pr)
    check_bound(dx.view.view(rows, lx), ref, 2, scale, f"reflect_pad_bwd ({lx}, {pl}, {pr})")   # at most three terms: two sums
    if pl == lx - 1 or pr == lx - 1:
        for bl, br in ((lx, pr), (pl, lx)):
            yb, db = Guarded(rows * (lx + bl + br)), Guarded(rows * lx)
            assert hip.eben_reflect_pad_fwd(x.data_ptr(), yb.ptr(), rows, lx, bl, br, stream()) == EINVAL
            assert hip.eben_reflect_pad_bwd(dy.data_ptr(), db.ptr(), rows, lx, bl, br, stream()) == EINVAL
            torch.cuda.synchronize()
            assert yb.untouched() and db.untouched()


@pytest.mark.parametrize("n", [1, 257, 256 * 256 + 5])
def test_l2norm(hip, n):
    """256 x 256 + 5 elements: 257 blocks' worth on a grid capped at 256 partial sums."""
    x = randn(n, 10300)
    x0 = x.clone()
    out = Guarded(257)
    assert hip.eben_l2norm(x.data_ptr(), n, out.ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert out.margins_intact() and same_bits(x, x0)
    worst = S.rel_sum_error(out.view[0].item(), S.l2norm(x))
    report(f"l2norm n={n}", worst_relative=worst)
    assert worst < 1e-6
