"""Float64 restatements of what runs at the end of every train step -- the feature-matching sums and gradient, the hinge terms and the
stacked backward seeds, the scalar loss totals, the element-wise ops and pads, the multi-tensor Adam -- written from the formulas in
include/eben_hip.h and the reference's modules, independent of the library (torch only; every function works on CPU and device tensors).

Error bounds.  U = 2^-24 is the unit roundoff of fp32 round-to-nearest: one correctly rounded operation (add, multiply, fma, and in this
build divide and square root) has a relative error of at most U of its exact result.  A kernel that does a fixed short chain of such
operations per element gets a bound  k * U * scale  where `scale` is built from the magnitudes ENTERING the operations (for c1 s1 - c2 s2
that is |c1| + |c2|, not the result) and k counts the roundings of the chain; each derivation is written at its function.  A fused
multiply-add in place of a multiply and an add drops one rounding, so the bounds hold whatever the compiler contracts.  `bound_violation`
and `pattern_mismatches` are the two comparisons of tests/test_gpu_step_tail.py; tests/test_step_tail_oracle.py shows on the CPU that they
separate an fp32 evaluation of the right formula from six wrong ones.
"""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
TINY = 2.0 ** -149      # the smallest fp32 denormal: the rounding quantum where a result leaves the normal range


def f64(t):
    return t.detach().to(torch.float64)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def bound_violation(got, ref, k, scale, floor=0.0):
    """Worst |got - ref| / (k 2^-24 scale + floor) over the elements (<= 1: inside the bound); an element whose bound is 0 must be exact.
    inf for a non-finite `got` or a shape mismatch."""
    got, ref = f64(got), f64(ref)
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return math.inf
    if got.numel() == 0:
        return 0.0
    scale = f64(scale) if torch.is_tensor(scale) else torch.full_like(ref, float(scale))
    bound = k * U * scale.abs() + floor
    err = (got - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
    return float(ratio.max())


def worst_error(got, ref, scale):
    """Measured worst |got - ref| / scale in units of 2^-24 (what a test prints beside its bound), over the elements whose scale is a
    normal fp32 number (below that the denormal quantum governs, not a relative rounding)."""
    got, ref, scale = f64(got), f64(ref), f64(scale).abs()
    keep = scale >= 2.0 ** -126 / U
    if not bool(keep.any()):
        return 0.0
    return float(((got - ref).abs()[keep] / scale[keep]).max()) / U


def pattern_mismatches(got, ref):
    """Exact match of two integer-coded patterns (signs, code bytes): the number of elements that differ (shape mismatch: all)."""
    if got.shape != ref.shape:
        return max(got.numel(), ref.numel(), 1)
    return int((got.to(torch.int64) != ref.to(torch.int64)).sum())


def rel_sum_error(got, ref):
    """|got - ref| / |ref| of a reduction (the project's relative tolerances for sums are stated in this form)."""
    got, ref = float(got), float(ref)
    if not math.isfinite(got):
        return math.inf
    return abs(got - ref) / max(abs(ref), 1e-300)


def sgn(t):
    return (t > 0).to(torch.float64) - (t < 0).to(torch.float64)


# ---- Adam (torch.optim.Adam, amsgrad off) ------------------------------------------------------------------------------------------
def adam_step(p, m, v, g, step, lr, betas, eps, wd=0.0, grad_scale=1.0):
    """One step from the state (p, m, v) with gradient g: (p_new, m_new, v_new) in float64."""
    p, m, v, g = f64(p), f64(m), f64(v), f64(g)
    b1, b2 = betas
    g = g * grad_scale
    if wd != 0.0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    p = p - lr / (1.0 - b1 ** step) * (m / denom)
    return p, m, v


def adam_bounds(p, m, v, g, step, lr, betas, eps, wd=0.0, grad_scale=1.0, err_p=0.0, err_m=0.0, err_v=0.0):
    """Absolute error bounds (bound_m, bound_v, bound_update) of one fp32 Adam step against `adam_step`, element by element.
    err_p / err_m / err_v: bounds of the errors the incoming fp32 state already carries (a run of several steps): they pass through the
    step's linear parts -- b1 err_m into m', b2 err_v into v', wd err_p into g' -- and on through the same chain.

    G = |g grad_scale| + |wd p| bounds the effective gradient g' = fma(wd, p, g grad_scale): two roundings, |dg'| <= 2 U G.
    exp_avg     m' = m + (g' - m)(1 - b1):  the subtraction, the constant 1 - b1, the product (3 U on (1 - b1)(G + |m|)), dg' passed on
                (2 U (1 - b1) G) and the final sum (U S_m):  6 U S_m,  S_m = |m| + (1 - b1)(G + |m|).                           k = 6
    exp_avg_sq  v' = v b2 + ((1 - b2) g') g':  the constant, two products and twice dg' on (1 - b2) G^2 (3 U + 4 U), one product on v b2
                (U; the two parts are disjoint, so 7 U covers both), the final sum (U S_v):  8 U S_v,  S_v = b2 v + (1 - b2) G^2.   k = 8
    update      -s q,  s = lr / fl(bc1) (2 U),  q = m' / d (U),  d = sqrt(v') / fl(sqrt(bc2)) + eps:  sqrt, the rounded constant and the
                division (3 U on r = sqrt(v') / sqrt(bc2)) plus the error of v' through the square root
                (dv / (sqrt(v') + sqrt(v' - dv)), exact mean-value form), the sum with eps (U d); then
                bound_q = bound_m / d_lo + |m'| bound_d / (d d_lo) + U |q|,   bound_update = s bound_q + 3 U |s q|   (s: 2 U, product: U).
    The parameter itself adds the rounding of p - s q: half an ulp of the result, <= U max(|p|, |p_new|) -- `adam_update_bound`."""
    p, m, v, g = f64(p), f64(m), f64(v), f64(g)
    b1, b2 = betas
    G = (g * grad_scale).abs() + (abs(wd) * p.abs() if wd != 0.0 else 0.0)
    p1, m1, v1 = adam_step(p, m, v, g, step, lr, betas, eps, wd, grad_scale)
    s_m = m.abs() + (1.0 - b1) * (G + m.abs())
    s_v = b2 * v.abs() + (1.0 - b2) * G * G
    dg = abs(wd) * err_p
    bound_m = 6 * U * s_m + TINY + b1 * err_m + (1.0 - b1) * dg
    bound_v = 8 * U * s_v + TINY + b2 * err_v + (1.0 - b2) * (2.0 * G * dg + dg * dg)
    bc2s = math.sqrt(1.0 - b2 ** step)
    s = lr / (1.0 - b1 ** step)
    root = v1.sqrt()
    low = (v1 - bound_v).clamp_min(0.0).sqrt()
    d_root = torch.where(root + low > 0, bound_v / (root + low).clamp_min(1e-300), bound_v.sqrt())
    d_root = torch.minimum(d_root, bound_v.sqrt())
    r = root / bc2s
    d = r + eps
    bound_d = 3 * U * r + d_root / bc2s + U * d
    d_lo = (d - bound_d).clamp_min(1e-300)
    q = m1 / d
    bound_q = bound_m / d_lo + m1.abs() * bound_d / (d * d_lo) + U * q.abs()
    bound_u = s * bound_q + 3 * U * (s * q).abs()
    return bound_m, bound_v, bound_u


def adam_update_bound(p, p_new, bound_u):
    """Bound of the observed update fl(p_new) - p: the chain's bound plus the final rounding of the parameter (half an ulp <= U |p|)."""
    return bound_u + U * torch.maximum(f64(p).abs(), f64(p_new).abs())


# ---- feature matching (feature_loss.py:37-50) --------------------------------------------------------------------------------------
def fm_sums(a, b):
    """(sum |a - b|, sum |a|) in float64."""
    a, b = f64(a), f64(b)
    return float((a - b).abs().sum()), float(a.abs().sum())


def fm_coefficients(s1, s2, gout, inv_count):
    gs = float(gout) * float(inv_count)
    return gs / float(s2), gs * float(s1) / (float(s2) * float(s2))


def fm_codes(a, b):
    """The pattern of the gradient: 3 (sgn(a - b) + 1) + (sgn(a) + 1), one of nine codes per element.  The fp32 difference a - b has
    the exact sign of the real one (rounding is monotonic and cannot reach zero from a non-zero difference of two floats)."""
    a, b = f64(a), f64(b)
    return (3 * (sgn(a - b) + 1) + (sgn(a) + 1)).to(torch.uint8)


def fm_grad(a, b, s1, s2, gout, inv_count):
    """d/da of gout inv_count sum|a - b| / sum|a| with the sums given: c1 sgn(a - b) - c2 sgn(a), and its bound's scale.

    fp32 chain: gs = gout inv_count (U), c1 = gs / s2 (U): 2 U |c1|;  c2 = (gs s1) / (s2 s2): 4 U |c2|;  the signs are exact and the one
    subtraction rounds the result, <= U (|c1| + |c2|):  at most 3 U |c1| + 5 U |c2| <= 5 U (|c1 sgn| + |c2 sgn|).                  k = 5"""
    c1, c2 = fm_coefficients(s1, s2, gout, inv_count)
    a, b = f64(a), f64(b)
    sd, sa = sgn(a - b), sgn(a)
    return c1 * sd - c2 * sa, abs(c1) * sd.abs() + abs(c2) * sa.abs()


FM_GRAD_K = 5


def fm_decode(grad, s1, s2, gout, inv_count):
    """The code (as `fm_codes`) whose value c1 sd - c2 sa lies nearest each element of a computed gradient."""
    c1, c2 = fm_coefficients(s1, s2, gout, inv_count)
    values = torch.tensor([c1 * sd - c2 * sa for sd in (-1, 0, 1) for sa in (-1, 0, 1)], dtype=torch.float64, device=grad.device)
    gaps = (values[:, None] - values[None, :]).abs() + torch.eye(9, dtype=torch.float64, device=grad.device)
    assert float(gaps.min()) > 1e-3 * max(abs(c1), abs(c2)), "choose sums whose nine gradient values are distinct"
    grad = f64(grad).reshape(-1)
    out = torch.empty(grad.numel(), dtype=torch.uint8, device=grad.device)
    for i in range(0, grad.numel(), 1 << 20):   # chunked: nine distances per element
        out[i:i + (1 << 20)] = (grad[i:i + (1 << 20), None] - values[None, :]).abs().argmin(1).to(torch.uint8)
    return out


def bl_fm_code(a, r):
    """The code byte of eben_bl_fm_sums_codes from the header: bits 0-1 = sgn(a - r) + 1, bits 2-3 = sgn(a) + 1; a, r = the fp32 sums
    hi + lo of the enhanced and the reference element."""
    a, r = f64(a), f64(r)
    return ((sgn(a - r) + 1).to(torch.uint8) | ((sgn(a) + 1).to(torch.uint8) << 2))


# ---- hinge (hinge_loss.py:35-43) ---------------------------------------------------------------------------------------------------
def hinge_mean(x, target):
    return float((1.0 - target * f64(x)).clamp_min(0.0).mean())


def hinge_grad(x, target, gout, scale):
    """d/dx of gout scale mean(relu(1 - target x)): -target g where 1 - target x > 0, else 0;  g = gout scale / n.
    fp32 chain: the product gout scale and the division by n (exact in fp32 below 2^24): 2 U |g|; -target g is exact for +-1.      k = 2
    The fp32 margin 1 - target x has the exact sign of the real one (target = +-1), so the pattern is unambiguous."""
    x = f64(x)
    g = float(gout) * float(scale) / x.numel()
    on = (1.0 - target * x) > 0
    return torch.where(on, torch.full_like(x, -target * g), torch.zeros_like(x))


HINGE_GRAD_K = 2


def hinge_seeds(a, b, gout, scales):
    """[0 | hinge'(a, +1) s0 | hinge'(a, -1) s1 | hinge'(b, +1) s2], `per` = a.numel() elements each."""
    a, b = f64(a).reshape(-1), f64(b).reshape(-1)
    assert a.numel() == b.numel()
    return torch.cat((torch.zeros_like(a), hinge_grad(a, 1.0, gout, scales[0]), hinge_grad(a, -1.0, gout, scales[1]),
                      hinge_grad(b, 1.0, gout, scales[2])))


def sign_codes(t):
    """-1 / 0 / +1 pattern of a sign-valued output, as integers."""
    return sgn(f64(t)).to(torch.int8)


# ---- scalar totals -----------------------------------------------------------------------------------------------------------------
def disc_losses(fm_sums_flat, inv_count, hinge):
    """out[0] = inv_count sum_p s1_p / s2_p over the (s1, s2) pairs; out[1 + k] = mean_i hinge[3 i + k] (adv, fake, real)."""
    s = f64(fm_sums_flat).reshape(-1, 2)
    h = f64(hinge).reshape(-1, 3)
    return torch.cat(((inv_count * (s[:, 0] / s[:, 1]).sum()).reshape(1), h.mean(0)))


def stft_loss_total(sums, inv_counts):
    """Header of eben_stft_loss_total: the mean over the resolutions of  mean_r sqrt(s0 / s1) + sum_r s2 inv_counts[i];
    sums[i] is (rows, 3)."""
    total = 0.0
    for s, ic in zip(sums, inv_counts):
        s = f64(s).reshape(-1, 3)
        total += float((s[:, 0] / s[:, 1]).sqrt().mean()) + float(s[:, 2].sum()) * float(ic)
    return total / len(sums)


# ---- element-wise ops and pads -----------------------------------------------------------------------------------------------------
def leaky_relu(x, slope):
    x = f64(x)
    return torch.where(x > 0, x, x * slope)


def leaky_relu_grad(dy, ref, slope):
    """dy where ref > 0, dy slope elsewhere (ref == +-0 included: torch's convention)."""
    dy, ref = f64(dy), f64(ref)
    return torch.where(ref > 0, dy, dy * slope)


def axpby(a, alpha, b, beta):
    """(alpha a + beta b, |alpha a| + |beta b|): two products and a sum, 2 U of the scale.                                          k = 2"""
    a, b = f64(a), f64(b)
    return alpha * a + beta * b, (alpha * a).abs() + (beta * b).abs()


def tanh_lift(x, lift, c_lift):
    """tanh(x + lift) on the first c_lift channels of (batch, channels, length), tanh(x) on the others; lift (batch, c_lift, length)."""
    x = f64(x).clone()
    if c_lift:
        x[:, :c_lift] += f64(lift)
    return torch.tanh(x)


def tanh_grad(dout, out):
    """(dout (1 - out^2), scale).  Three fp32 operations: out out (U out^2), 1 - . (U |w|, w = 1 - out^2), the product (U |dout w|):
    |error| <= U |dout| (out^2 + 2 |w|); a fused 1 - out out only drops the first.                                     k = 1 on that scale"""
    dout, out = f64(dout), f64(out)
    w = 1.0 - out * out
    return dout * w, dout.abs() * (out * out + 2.0 * w.abs())


def reflect_index(lx, pl, pr):
    """Source index of every position of the padded row (nn.ReflectionPad1d; pl, pr < lx)."""
    q = torch.arange(-pl, lx + pr)
    q = q.abs()
    return torch.where(q >= lx, 2 * (lx - 1) - q, q)


def reflect_pad(x, pl, pr):
    return x[..., reflect_index(x.shape[-1], pl, pr).to(x.device)]


def reflect_pad_adjoint(dy, lx, pl, pr):
    """Adjoint of reflect_pad by scattering: dx[q(j)] += dy[j] in float64.  A position receives at most three terms (itself and one
    fold from each side), i.e. two fp32 additions: 2 U of the same scatter of |dy|.                                                 k = 2"""
    dy = f64(dy)
    idx = reflect_index(lx, pl, pr).to(dy.device)
    dx = torch.zeros(dy.shape[:-1] + (lx,), dtype=torch.float64, device=dy.device)
    return dx.index_add_(dy.dim() - 1, idx, dy)


def l2norm(x):
    return float(f64(x).pow(2).sum().sqrt())
