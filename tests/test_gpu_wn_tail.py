"""GPU: the tail every weight gradient ends in -- the fixed-order sum over the split-K slabs and the weight-norm chain rule,
eben_wn_bwd (slab_reduce_kernel, wn_bwd_kernel) and eben_wn_bwd_multi (slab_reduce_multi_kernel, wn_bwd_multi_kernel) of conv_dw.hip
-- against a float64 sum over the slabs and, where weight norm is on, float64 autograd of g v / |v| applied to that sum.

Bounds: 1e-6 of max|ref| for the plain sum (dv without weight norm, dbias): at most 512 fp32 additions of formula values in [-1, 1].
2 * 3e-5 for the weight-norm outputs, the bound tests/test_gpu_ru_variants.py holds eben_wn_bwd to.  The multi form must equal the
single form bit for bit.  Slab counts: every remainder of the reduce loop's four-way unrolling, both sides of the 31 / 32 switch of
slab_reduce_multi_kernel between one thread per element and the four z-groups spread over the block's waves, and 512, the split-K
cap.  The memory between and behind the slabs, and every output, is NaN before the launch.
"""
import math

import pytest
import torch

from formula import formula_tensor
from tests.test_gpu_ops import rel_err

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-6
WN_TOL = 2 * 3e-5
NSLABS = (1, 2, 4, 5, 13, 16, 17, 29, 31, 32, 33, 48, 61, 512)
NAN = float("nan")


class Job:
    """One tensor's tail: slabs (nslab, rows, row_stride) in weight order, `pad` floats between slabs, optional bias column, optional
    weight norm; perm_k > 0: the slabs reach the device in bundle-major column order."""

    def __init__(self, tag, nslab, rows, cols, bias, wn, pad=0, perm_k=0):
        self.tag, self.nslab, self.rows, self.cols, self.bias, self.wn, self.pad, self.perm_k = tag, nslab, rows, cols, bias, wn, pad, perm_k
        self.rs = cols + (1 if bias else 0)
        self.slabs = formula_tensor(f"wn_tail/{tag}/slabs", (nslab, rows, self.rs))
        self.v = formula_tensor(f"wn_tail/{tag}/v", (rows, cols), 1 / math.sqrt(cols))
        self.g = self.v.norm(dim=1) * (1 + 0.3 * formula_tensor(f"wn_tail/{tag}/g", (rows,)))

    def reference(self):
        """(dv, dg or None, dbias or None) in float64."""
        s = self.slabs.double().sum(dim=0)
        dw, dbias = s[:, :self.cols], (s[:, self.cols] if self.bias else None)
        if not self.wn:
            return dw, None, dbias
        v, g = self.v.double().requires_grad_(True), self.g.double().requires_grad_(True)
        ((g / v.norm(dim=1)).unsqueeze(1) * v * dw).sum().backward()
        return v.grad, g.grad, dbias

    def device_slabs(self):
        """A fresh flat buffer: slab z at z * slab_stride, NaN in between."""
        u = self.slabs
        if self.perm_k:
            k = self.perm_k
            c, j = torch.arange(self.cols) // k, torch.arange(self.cols) % k
            s = ((c // 8) * k + j) * 8 + c % 8     # slab column of weight element c k + j
            p = u.clone()
            p[:, :, s] = u[:, :, :self.cols]
            u = p
        n = self.rows * self.rs
        buf = torch.full((self.nslab, n + self.pad), NAN)
        buf[:, :n] = u.reshape(self.nslab, n)
        return buf.reshape(-1).cuda()

    def slab_stride(self):
        return self.rows * self.rs + self.pad


class Run:
    """Device buffers of one launch of a job: inputs, NaN outputs."""

    def __init__(self, lib, job, norm=None):
        from vibravox_amd._lib import check, ptr, stream

        self.job = job
        self.slabs = job.device_slabs()
        self.v, self.g = job.v.cuda(), job.g.contiguous().cuda()
        self.dv = torch.full((job.rows, job.cols), NAN, device="cuda")
        self.dg = torch.full((job.rows,), NAN, device="cuda") if job.wn else None
        self.dbias = torch.full((job.rows,), NAN, device="cuda") if job.bias else None
        self.norm = norm
        if job.wn and norm is None:
            scale = torch.full((job.rows,), NAN, device="cuda")
            self.norm = torch.full((job.rows,), NAN, device="cuda")
            check(lib.eben_wn_scale(ptr(self.g), ptr(self.v), job.rows, job.cols, ptr(scale), ptr(self.norm), stream()), "wn_scale")

    def single(self, lib):
        from vibravox_amd._lib import check, ptr, stream

        j = self.job
        assert j.perm_k == 0
        wn = (ptr(self.g), ptr(self.v), ptr(self.norm), ptr(self.dg)) if j.wn else (None, None, None, None)
        check(lib.eben_wn_bwd(ptr(self.slabs), j.nslab, j.slab_stride(), j.rows, j.cols, j.rs, *wn, ptr(self.dv), ptr(self.dbias), stream()), "wn_bwd")
        return self

    def item(self):
        from vibravox_amd._lib import EbenWnBwdItem, ptr

        j = self.job
        g, v, norm, dg = (ptr(self.g), ptr(self.v), ptr(self.norm), ptr(self.dg)) if j.wn else (None, None, None, None)
        return EbenWnBwdItem(ptr(self.slabs), g, v, norm, dg, ptr(self.dv), ptr(self.dbias), j.slab_stride(), j.nslab, j.rows, j.cols, j.rs, j.perm_k, 0)

    def outputs(self):
        return {"dv": self.dv, "dg": self.dg, "dbias": self.dbias}


def multi(lib, runs):
    from vibravox_amd._lib import EbenWnBwdItem, check, stream

    check(lib.eben_wn_bwd_multi((EbenWnBwdItem * len(runs))(*[r.item() for r in runs]), len(runs), stream()), "wn_bwd_multi")
    return runs


def errors(run):
    """{output: rel_err against float64} of a finished run, each asserted against its bound."""
    j = run.job
    dv, dg, dbias = j.reference()
    errs = {"dv": rel_err(run.dv, dv)}
    assert errs["dv"] < (WN_TOL if j.wn else SUM_TOL), (j.tag, errs)
    if j.wn:
        errs["dg"] = rel_err(run.dg, dg)
        assert errs["dg"] < WN_TOL, (j.tag, errs)
    if j.bias:
        errs["dbias"] = rel_err(run.dbias, dbias)
        assert errs["dbias"] < SUM_TOL, (j.tag, errs)
    return errs


def same_bits(a, b):
    for key, t in a.outputs().items():
        assert t is None or (torch.isfinite(t).all() and torch.equal(t, b.outputs()[key])), (a.job.tag, key)


def check_both_forms(lib, jobs):
    """Each job through eben_wn_bwd, all of them through ONE eben_wn_bwd_multi: the float64 bounds, and the same bits."""
    singles = [Run(lib, j).single(lib) for j in jobs]
    multis = multi(lib, [Run(lib, j, norm=s.norm) for j, s in zip(jobs, singles)])
    torch.cuda.synchronize()
    worst = {}
    for s, m in zip(singles, multis):
        for k, e in errors(s).items():
            worst[k] = max(worst.get(k, 0.0), e)
        errors(m)
        same_bits(s, m)
    return worst


@pytest.mark.parametrize("nslab", NSLABS)
def test_slab_sum_and_weight_norm_at_every_slab_count(hip, nslab):
    """7 x 46 = 322 and 7 x 45 = 315 elements per slab: off a multiple of 64 (the LDS form's pass) and of 256 (the thread-sum form's);
    odd slab counts also with 37 floats of NaN between the slabs."""
    rows, cols = 7, 45
    assert (rows * cols) % 64 and (rows * (cols + 1)) % 64 and (rows * cols) % 256 and (rows * (cols + 1)) % 256
    pad = 37 if nslab % 2 else 0
    jobs = [Job(f"n{nslab}/b{int(bias)}w{int(wn)}", nslab, rows, cols, bias, wn, pad) for bias in (False, True) for wn in (False, True)]
    worst = check_both_forms(hip, jobs)
    print(f"[wn_tail] nslab {nslab}: " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()))


@pytest.mark.parametrize("nslab, rows, cols", [(3, 600, 899), (32, 150, 899)])
def test_grid_stride_past_the_block_cap(hip, nslab, rows, cols):
    """More elements than the multi form's 2048 blocks cover in one pass: 540000 > 2048 x 256 on the thread-sum form, 135000 >
    2048 x 64 on the LDS form."""
    n = rows * (cols + 1)
    assert n > 2048 * (256 if nslab < 32 else 64) and n % 256
    worst = check_both_forms(hip, [Job(f"cap{nslab}", nslab, rows, cols, True, True)])
    print(f"[wn_tail] {n} elements x {nslab} slabs: " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()))


@pytest.mark.parametrize("cols", (768, 769, 1030, 1795))
def test_rows_past_768_columns_are_the_same_bits_in_both_forms(hip, cols):
    """From four passes of the 256 threads over a row (cols > 768) the compiler unrolls wn_bwd_kernel's dv loop; its body was
    contracted into an FMA where the remainder loop and the multi form multiply and subtract, and 22 % of such a row's dv differed in
    the last bit between eben_wn_bwd and eben_wn_bwd_multi (wn_dv in conv_dw.hip pins one rounding per operation)."""
    worst = check_both_forms(hip, [Job(f"wide/{cols}", 3, 9, cols, True, True), Job(f"wide/{cols}/plain", 3, 9, cols, True, False)])
    print(f"[wn_tail] {cols} columns: " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()))


def seventy_jobs():
    """Two full tables of 32 items and a partial one; every third item has one slab (it owns no reduce block), slab counts on both
    sides of 32, with and without bias column, weight norm and slab padding."""
    counts = (1, 3, 40, 1, 17, 32, 2, 31, 64)
    jobs = []
    for i in range(70):
        nslab = counts[i % len(counts)]
        jobs.append(Job(f"seventy/{i}", nslab, 3 + (5 * i) % 37, 5 + (11 * i) % 126, i % 2 == 0, i % 3 != 1, pad=(i % 4) * 3 if nslab > 1 else 0))
    return jobs


def test_seventy_items_in_one_call(hip):
    jobs = seventy_jobs()
    assert len(jobs) == 70 > 2 * 32 and sum(j.nslab == 1 for j in jobs) >= 10
    assert jobs[31].nslab > 1 and jobs[32].nslab > 1 and any(j.nslab == 1 for j in jobs[64:])
    assert {(j.bias, j.wn) for j in jobs} == {(a, b) for a in (False, True) for b in (False, True)}
    worst = check_both_forms(hip, jobs)
    print("[wn_tail] 70 items: " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()))


def test_seventy_scales_in_one_call(hip):
    from vibravox_amd._lib import EbenWnScaleItem, check, ptr, stream

    jobs = seventy_jobs()
    keep, items = [], []
    for j in jobs:
        v, g = j.v.cuda(), j.g.contiguous().cuda()
        s1, n1, s2, n2 = (torch.full((j.rows,), NAN, device="cuda") for _ in range(4))
        check(hip.eben_wn_scale(ptr(g), ptr(v), j.rows, j.cols, ptr(s1), ptr(n1), stream()), "wn_scale")
        items.append(EbenWnScaleItem(ptr(g), ptr(v), ptr(s2), ptr(n2), j.rows, j.cols))
        keep.append((v, g, s1, n1, s2, n2))
    check(hip.eben_wn_scale_multi((EbenWnScaleItem * 70)(*items), 70, stream()), "wn_scale_multi")
    torch.cuda.synchronize()
    worst = 0.0
    for j, (v, g, s1, n1, s2, n2) in zip(jobs, keep):
        assert torch.equal(s1, s2) and torch.equal(n1, n2), j.tag
        norm = j.v.double().norm(dim=1)
        worst = max(worst, rel_err(n2, norm), rel_err(s2, j.g.double() / norm))
    print(f"[wn_tail] 70 scales: {worst:.3e}")
    assert worst < 1e-6   # a sum of at most 130 squares in fp32, a square root, a division


@pytest.mark.parametrize("k", (3, 5, 7, 41))
@pytest.mark.parametrize("n", (1, 3, 12))
def test_bundle_major_slab_columns(hip, k, n):
    """col_perm_k: the slabs hold column s = ((c / 8) k + j) 8 + c % 8 for weight element c k + j (bl_dw.hip's order), walked with
    carries; with the bias column, with weight norm and without, against float64 on the un-permuted order and against the
    col_perm_k = 0 launch on un-permuted slabs."""
    cols, rows, nslab = 8 * n * k, 5, 3
    for wn in (False, True):
        permuted = Job(f"perm/{k}/{n}/{int(wn)}", nslab, rows, cols, True, wn, perm_k=k)
        plain = Job(f"perm/{k}/{n}/{int(wn)}", nslab, rows, cols, True, wn)
        assert torch.equal(permuted.slabs, plain.slabs)
        a = Run(hip, permuted)
        b = Run(hip, plain, norm=a.norm)
        multi(hip, [a, b])
        torch.cuda.synchronize()
        ea, eb = errors(a), errors(b)
        assert torch.equal(a.dbias, b.dbias)
        if not wn:
            assert torch.equal(a.dv, b.dv)     # the same sums, element by element
        else:
            # the dot product's order differs: within the float64 bound of each other
            assert rel_err(a.dv, b.dv.double().cpu()) < WN_TOL and rel_err(a.dg, b.dg.double().cpu()) < WN_TOL
        print(f"[wn_tail] col_perm_k {k}, cols {cols}, weight norm {wn}: " + ", ".join(f"{key} {e:.3e} ({eb[key]:.3e} unpermuted)" for key, e in ea.items()))


def test_argument_checks_fail_cleanly(hip):
    """Both entry points: a negative return and a message, nothing launched."""
    from vibravox_amd._lib import EbenWnBwdItem, ptr, stream

    job = Job("args", 2, 4, 24, True, True)
    r = Run(hip, job)
    torch.cuda.synchronize()
    s, g, v, norm, dg, dv, db = (ptr(t) for t in (r.slabs, r.g, r.v, r.norm, r.dg, r.dv, r.dbias))
    rows, cols, rs, stride = job.rows, job.cols, job.rs, job.slab_stride()

    def single(cols=cols, rs=rs, g=g, norm=norm, db=db):
        return hip.eben_wn_bwd(s, 2, stride, rows, cols, rs, g, v, norm, dg, dv, db, stream())

    def multi_(cols=cols, rs=rs, g=g, norm=norm, db=db, perm=0):
        item = EbenWnBwdItem(s, g, v, norm, dg, dv, db, stride, 2, rows, cols, rs, perm, 0)
        return hip.eben_wn_bwd_multi((EbenWnBwdItem * 1)(item), 1, stream())

    bad = {
        "row_stride < cols": dict(rs=cols - 1),
        "a bias without a bias column": dict(rs=cols),
        "g without norm": dict(norm=None),
    }
    for what, kw in bad.items():
        for call in (single, multi_):
            rc = call(**kw)
            assert rc < 0 and hip.eben_last_error(), (what, call.__name__, rc)
    rc = multi_(perm=5)     # 24 columns are no multiple of 8 x 5
    assert rc < 0 and b"8 n k" in hip.eben_last_error(), rc
    assert multi_(perm=-1) < 0
    torch.cuda.synchronize()
    assert torch.isnan(r.dv).all() and torch.isnan(r.dbias).all()     # nothing ran
    assert multi_(perm=3) == 0 and single() == 0
    torch.cuda.synchronize()
