"""Values on both sides of every panel and chunk cut of the generic and panel routes (tests/seam_plan.py).

Every route that leaves the register-resident kernels cuts its work into panels by a fixed budget; the code that runs
only at a cut (`+ i0` / `+ j0` offsets, the accumulate flag of the NT GEMM from the second streamed chunk on, the
`i0 == 0` initialisation of the column sums, the per-launch offsets and splits of the fused projection, the per-panel
host sums of `mgp_kxx_grad`) is exercised here at the smallest shapes that cross each cut.

Every case runs on a fresh handle with NaN-filled outputs and then proves with `mgp_arena_bytes` that the LIBRARY cut
where the plan says: the named arena is exactly what `mgp_reserve` allocates for the plan's request (inside the window
[plan, 1.25 plan + 4096 + 256]), and that request is smaller than one panel over the whole shape.  If a budget changes
the proof fails; the test does not silently stop crossing anything.

Two checks per product:
 (a) few-hot multipliers (zero except on about 40 contraction indices: c - 1, c, c + 1 of every contraction cut, the
     first and last index, seeded random ones), against long double, for the output rows next to every owned-row cut.
     Zeros add exactly, so every checked element is held to
         |y^_i - y_i| <= sum_j (rho_ij + (nnz + s + 2) u) |k_ij w_j|
     with rho = `pair_reference.pair_bound`, u the unit roundoff, nnz the nonzero multipliers and s the partial results
     the route adds (streamed chunks or splits, plus at most 8 GEMM slices): any summation order of n terms meets
     (n - 1) u to first order.  Nothing is fitted.  One dropped or doubled term at a cut breaks it.
 (b) dense random multipliers, the whole output against an fp64 evaluation in torch (direct differences), at the
     normwise bar the route's existing test uses: a chunk that is misplaced, missing or stale anywhere.

Every case prints `seam <entry> ...: worst err / bound`; DESIGN section 4.8c records a run's figures.
"""

import contextlib
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pair_reference as pr
import seam_plan as sp
from lml_reference import kxx_grad_reference

pytestmark = pytest.mark.gpu

LD = np.longdouble
VAR = pr.VARIANCE
COLS, ROWS = 0, 1
GEMM_SLICES = 8  # gemm_nt_launch sums at most 8 slices of K (csrc/dense.hip:631)
TDT = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}


def dev():
    return torch.device("cuda:0")


def T(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev())


def nan_out(shape, dtype):
    dtype = dtype if isinstance(dtype, torch.dtype) else TDT[np.dtype(dtype)]
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def report(entry, what, worst):
    print(f"seam {entry} {what}: worst err / bound {worst:.3g}")


@contextlib.contextmanager
def fresh_handle(env=None):
    """A handle nothing else has touched (its arenas are this case's alone); `env` is read by mgp_create."""
    from cggp import _hip
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        hd = _hip.Handle(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    hd.sync_stream()
    try:
        yield hd
    finally:
        torch.cuda.synchronize()
        hd.lib.mgp_destroy(hd.h)
        hd.h = None


def arena_proof(hd, plan):
    """The cut was crossed in the library, not only in the plan."""
    name, need = plan.arena
    got = hd.lib.mgp_arena_bytes(hd.h, name.encode())
    lo, hi = sp.arena_window(plan)
    assert lo <= got <= hi, (name, got, lo, hi)
    # mgp_arena_bytes reports the allocation (a quarter above the request), so "smaller than one panel over the whole
    # shape" is asked of the request behind it -- which the allocation pins down exactly
    assert got == sp.reserved_bytes(need), (name, got, sp.reserved_bytes(need))
    assert sp.asked_bytes(got) < plan.whole, (name, got, plan.whole)


def spec_of(case):
    from cggp import ops
    return ops.KernelSpec(case.kind, VAR, list(pr.lengthscales(case.D)), case.D)


def kstruct(case):
    from cggp import _hip
    return spec_of(case).struct(_hip.F64 if case.dtype == np.float64 else _hip.F32)


def as_seen(a, dtype):
    """The values the device is given, as float64."""
    return np.asarray(a, dtype=dtype).astype(np.float64)


def few_hot(n, support, R, dtype, seed):
    rng = np.random.default_rng([seed, n, R])
    W = np.zeros((n, R))
    W[support] = rng.standard_normal((len(support), R))
    return as_seen(W, dtype)


def dense(n, R, dtype, seed):
    return as_seen(np.random.default_rng([seed, n, R, 7]).standard_normal((n, R)), dtype)


# ---------------------------------------------------------------- references
def k_torch(kind, ls, A, B):
    """k(A, B) in fp64 on the device, not libmgp: direct differences, one input dimension at a time; GPflow's floor
    r = sqrt(max(r2, 1e-36)) for the Matern family."""
    A, B = A.double(), B.double()
    r2 = torch.zeros((A.shape[0], B.shape[0]), dtype=torch.float64, device=A.device)
    for d in range(A.shape[1]):
        diff = (A[:, d, None] - B[None, :, d]) / float(ls[d])
        r2.addcmul_(diff, diff)
    del diff
    if kind == "se":
        return r2.mul_(-0.5).exp_().mul_(VAR)
    r = r2.clamp_min_(1e-36).sqrt_()
    if kind == "matern12":
        return r.neg_().exp_().mul_(VAR)
    c = math.sqrt(3.0) if kind == "matern32" else math.sqrt(5.0)
    a = r.mul_(c)
    poly = 1.0 + a if kind == "matern32" else 1.0 + a + a * a / 3.0
    return poly.mul_(a.neg_().exp_()).mul_(VAR)


def relmax(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


class FewHotReference:
    """Long-double y[rows] = k(P[rows], Q[J]) W[J] and its bound, for output rows `rows` and multiplier support `J`."""

    def __init__(self, case, P, Q, rows, J, partials):
        ls = pr.lengthscales(case.D)
        self.rows, self.J = rows, J
        self.pv = pr.pair_values(case.kind, VAR, ls, P[rows], Q, cols=J)
        floor = LD(VAR) * LD(2) ** pr.flush_floor_log2(case.dtype)
        assert self.pv.k.min() > floor  # every pair above the flush floor: the relative bound applies to all of them
        rho = pr.pair_bound(case.kind, VAR, self.pv.s, self.pv.q, pr.scaled(case.kind, ls, P[rows]),
                            pr.scaled(case.kind, ls, Q[J]), case.D, case.dtype)
        u = pr.unit_roundoff(case.dtype)
        self.weight = (rho + (len(J) + partials + 2) * u).astype(LD) * np.abs(self.pv.k)

    def product(self, W):
        """(y [rows, R], bound [rows, R]) for W [n, R]."""
        WJ = W[self.J].astype(LD)
        return self.pv.k @ WJ, self.weight @ np.abs(WJ)


def hold(label, got, want, bound):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.all(np.isfinite(got)), f"{label}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    err = np.abs(got.astype(LD) - want)
    ratio = (err / np.where(bound > 0, bound, LD(1))).astype(np.float64)
    ratio = np.where((bound > 0) | (err == 0), ratio, np.inf)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{label}: {int((ratio > 1).sum())} of {ratio.size} outside the bound; worst at {i}: got "
                             f"{float(got[i]):.17e}, want {float(want[i]):.17e}, err / bound {worst:.3g}")
    return worst


def rho_cap(case, P, Q):
    """An upper bound of `pair_bound` over ALL pairs from the largest scaled norms alone: S <= (max|a| + max|b|)^2,
    q <= max|a| + max|b|, min(ds / q, sqrt ds) <= sqrt ds."""
    ls = pr.lengthscales(case.D)
    top = (np.linalg.norm(pr.scaled(case.kind, ls, P), axis=1).max()
           + np.linalg.norm(pr.scaled(case.kind, ls, Q), axis=1).max())
    u = pr.unit_roundoff(case.dtype)
    ds = (case.D + 6) * u * top * top
    ln2 = math.log(2.0)
    if case.kind == "se":
        return ln2 * ds + pr.FUNCTION_BUDGET * u
    return ln2 * math.sqrt(ds) + 2.0 * u * ln2 * top + pr.FUNCTION_BUDGET * u


FP32_BAR = 2e-4  # tests/test_gpu_love.py::test_project_fp32_takes_the_generic_route: the same panel + NT GEMM in fp32


def dense_check(label, case, got, Kref, Wd, P, Q, partials, bar):
    """Check (b): the whole output, normwise (max |err| / max |ref|), at `bar` for fp64.  No existing test holds a
    generic fp32 product, so fp32 takes the bar of the fp32 projection, which is the same structure (explicit fp32
    panels, the NT GEMM of csrc/dense.hip, chunked by the same budget): 2e-4.  It is also what the format allows a dense
    random product: the terms' roundings are independent, so a sum of n = 16421 terms is off by about
    sqrt(n) u rms|k w| + rho rms|k w| sqrt(n), i.e. (u + rho) of the result's own scale sqrt(n) rms|k w|, with rho a few
    u for direct differences: 1e-6, two orders inside the bar, while a chunk that is misplaced, missing or doubled moves
    the result by 0.05 to O(1) of its scale.  On top, every fp32 element stays within the worst-case bound of check (a)
    with rho replaced by its cap over all pairs (which alone would let whole chunks pass: it is there for single
    elements far out).  Returns err / bar."""
    ref = Kref @ Wd.double()
    assert bool(torch.isfinite(got).all()), label
    e = relmax(got, ref)
    if case.dtype == np.float64:
        assert e < bar, (label, e)
        return e / bar
    assert e < FP32_BAR, (label, e)
    u = pr.unit_roundoff(case.dtype)
    bound = (rho_cap(case, P, Q) + (Kref.shape[1] + partials + 2) * u) * (Kref.abs() @ Wd.double().abs())
    ratio = float(((got.double() - ref).abs() / bound).max())
    assert ratio <= 1.0, (label, ratio)
    return e / FP32_BAR


# ---------------------------------------------------------------- knm_matvec / kmn_matvec / kxx_matvec
def matvec(hd, which, k, P, Q, V, R, layout):
    """k(P, Q) V with P owned and Q streamed, through mgp_knm_matvec(P, Q) or mgp_kmn_matvec(Q, P); -> [na, R]."""
    from cggp import _hip
    na, nb = P.shape[0], Q.shape[0]
    Vd = V if layout == COLS else V.t().contiguous()
    out = nan_out((na, R) if layout == COLS else (R, na), V.dtype)
    p = _hip.ptr
    if which == "knm":
        rc = hd.lib.mgp_knm_matvec(hd.h, ctypes.byref(k), p(P), na, p(Q), nb, p(Vd), R, layout, p(out), layout)
    else:
        rc = hd.lib.mgp_kmn_matvec(hd.h, ctypes.byref(k), p(Q), nb, p(P), na, p(Vd), R, layout, p(out), layout)
    hd.check(rc)
    return out if layout == COLS else out.t()


@pytest.mark.parametrize("case", sp.cases("sweep"), ids=repr)
def test_sweep_generic_seams(case):
    """sweep_generic_t (csrc/generic.hip) behind mgp_knm_matvec and mgp_kmn_matvec: R = 3 and 1, both layouts."""
    na, nb = case.shape
    X, Z, ls = pr.shifted_set(case.kind, case.D, na, nb)
    P, Q = as_seen(X, case.dtype), as_seen(Z, case.dtype)
    rows, J = case.rows("owned"), case.support("streamed")
    partials = len(case.plan.cuts("streamed")) + 1 + GEMM_SLICES
    ref = FewHotReference(case, P, Q, rows, J, partials)
    Pt, Qt = T(P, case.dtype), T(Q, case.dtype)
    Kref = k_torch(case.kind, ls, Pt, Qt)
    k = kstruct(case)
    rows_t = torch.from_numpy(rows).to(dev())
    worst_a = worst_b = 0.0
    with fresh_handle() as hd:
        for R in (3, 1):  # the widest first: the arena is then sized once, by the plan's R = 3
            W = few_hot(nb, J, R, case.dtype, seed=1)
            Wt, Wd = T(W, case.dtype), T(dense(nb, R, case.dtype, seed=2), case.dtype)
            want, bound = ref.product(W)
            for layout in (COLS, ROWS):
                for which in ("knm", "kmn"):
                    label = f"{case.id} {which} R={R} {'cols' if layout == COLS else 'rows'}"
                    got = matvec(hd, which, k, Pt, Qt, Wt, R, layout)
                    again = matvec(hd, which, k, Pt, Qt, Wt, R, layout)
                    assert torch.equal(got, again), label  # deterministic: bit-identical
                    worst_a = max(worst_a, hold(label + " few-hot", got[rows_t], want, bound))
                    gd = matvec(hd, which, k, Pt, Qt, Wd, R, layout)
                    assert torch.equal(gd, matvec(hd, which, k, Pt, Qt, Wd, R, layout)), label
                    # 1e-11: tests/test_gpu_parity.py::test_generic_dimension_path
                    worst_b = max(worst_b, dense_check(label + " dense", case, gd, Kref, Wd, P, Q, partials, 1e-11))
        arena_proof(hd, case.plan)
    report("sweep", f"{case.id} few-hot", worst_a)
    report("sweep", f"{case.id} dense", worst_b)


@pytest.mark.parametrize("case", sp.cases("kxx_matvec"), ids=repr)
def test_kxx_matvec_generic_seams(case):
    """mgp_kxx_matvec at D = 33: the sweep over (X, X) with the addend s2 V read, and the output written, at the
    `scatter_view` offsets of every row chunk.  out = K V + s2 V; the addend joins in one fma, whose rounding is u of
    the result: u |s2 v| on top of the product's bound (the rest of the result is inside its `+ 2`)."""
    from cggp import _hip
    N = case.shape[0]
    s2, R = 0.25, 3
    X, _, ls = pr.shifted_set(case.kind, case.D, N, 64)
    P = as_seen(X, case.dtype)
    rows, J = case.rows("owned"), case.support("streamed")
    partials = len(case.plan.cuts("streamed")) + 1 + GEMM_SLICES
    ref = FewHotReference(case, P, P, rows, J, partials)
    Pt = T(P)
    Kref = k_torch(case.kind, ls, Pt, Pt)
    k = kstruct(case)
    rows_t = torch.from_numpy(rows).to(dev())
    V = few_hot(N, J, R, case.dtype, seed=3)
    want, bound = ref.product(V)
    want = want + LD(s2) * V[rows].astype(LD)
    bound = bound + LD(pr.unit_roundoff(case.dtype) * s2) * np.abs(V[rows]).astype(LD)
    Vd = T(dense(N, R, case.dtype, seed=4))
    worst_a = worst_b = 0.0
    p = _hip.ptr

    def call(Vt, layout):
        Vin = Vt if layout == COLS else Vt.t().contiguous()
        out = nan_out(tuple(Vin.shape), np.float64)
        hd.check(hd.lib.mgp_kxx_matvec(hd.h, ctypes.byref(k), p(Pt), N, s2, p(Vin), R, layout, p(out), layout))
        return out if layout == COLS else out.t()

    with fresh_handle() as hd:
        for layout in (COLS, ROWS):
            label = f"{case.id} R={R} {'cols' if layout == COLS else 'rows'}"
            got, again = call(T(V), layout), call(T(V), layout)
            assert torch.equal(got, again), label
            worst_a = max(worst_a, hold(label + " few-hot", got[rows_t], want, bound))
            gd = call(Vd, layout)
            assert torch.equal(gd, call(Vd, layout)), label
            e = relmax(gd, Kref @ Vd + s2 * Vd)
            assert e < 1e-11, (label, e)  # tests/test_gpu_parity.py::test_generic_dimension_path
            worst_b = max(worst_b, e / 1e-11)
        arena_proof(hd, case.plan)
    report("kxx_matvec", f"{case.id} few-hot", worst_a)
    report("kxx_matvec", f"{case.id} dense", worst_b)


# ---------------------------------------------------------------- column sums
@pytest.mark.parametrize("case", sp.cases("sq_colsum"), ids=repr)
def test_sq_colsum_generic_seams(case):
    """sq_colsum_generic_t: out[m] = sum_i k(x_i, z_m)^2 over row chunks; the first chunk initialises, the others add."""
    from cggp import _hip
    N, M = case.shape
    X, Z, ls = pr.shifted_set(case.kind, case.D, N, M)
    Xt, Zt = T(X), T(Z)
    k = kstruct(case)
    p = _hip.ptr

    def call():
        out = nan_out((M,), np.float64)
        hd.check(hd.lib.mgp_kmn_sq_colsum(hd.h, ctypes.byref(k), p(Xt), N, p(Zt), M, p(out)))
        return out

    with fresh_handle() as hd:
        got, again = call(), call()
        arena_proof(hd, case.plan)
    assert torch.equal(got, again)
    assert bool(torch.isfinite(got).all())
    # (b) all M columns; 1e-12: tests/test_gpu_parity.py::test_generic_dimension_path
    Kref = k_torch(case.kind, ls, Xt, Zt)
    e = relmax(got, (Kref * Kref).sum(dim=0))
    assert e < 1e-12, (case.id, e)
    # 16 columns in long double over all N rows: (rho_max + (N + 2) u) sum_i k_im^2, rho_max over the column's pairs
    cols = sp.check_indices(M, [], 5, extra=14)
    pv = pr.pair_values(case.kind, VAR, ls, X, Z, cols=cols)
    rho = pr.pair_bound(case.kind, VAR, pv.s, pv.q, pr.scaled(case.kind, ls, X), pr.scaled(case.kind, ls, Z[cols]),
                        case.D, case.dtype)
    want = (pv.k * pv.k).sum(axis=0)
    bound = (rho.max(axis=0) + (N + 2) * pr.unit_roundoff(case.dtype)).astype(LD) * want
    worst = hold(f"{case.id} columns {cols.tolist()}", got[torch.from_numpy(cols).to(dev())], want, bound)
    report("sq_colsum", f"{case.id} 16 columns", worst)
    report("sq_colsum", f"{case.id} all columns", e / 1e-12)


# ---------------------------------------------------------------- the wide projection
def bar(kind):
    """tests/test_gpu_gpr.py::bar, the bar of tests/test_gpu_love.py::test_project_matches_longdouble."""
    return 1e-7 if kind == "matern12" else 1e-11


def project(hd, k, Xs, X, R, r, cols_layout, want_proj, dtype):
    from cggp import _hip
    B, N = Xs.shape[0], X.shape[0]
    Rd = R if cols_layout else R.t().contiguous()
    proj = nan_out((B, r), dtype) if want_proj else None
    sq = nan_out((B,), dtype)
    p = _hip.ptr
    hd.check(hd.lib.mgp_knm_project(hd.h, ctypes.byref(k), p(Xs), B, p(X), N, p(Rd), r, COLS if cols_layout else ROWS,
                                    p(proj), p(sq)))
    return proj, sq


def sqnorm_bound(want, bound, r, u):
    """|sum_c p^_c^2 - sum_c p_c^2| <= sum_c (2 |p_c| e_c + e_c^2) + (r + 2) u sum_c p_c^2 for |p^_c - p_c| <= e_c."""
    sq = (want * want).sum(axis=1)
    return sq, (2 * np.abs(want) * bound + bound * bound).sum(axis=1) + LD((r + 2) * u) * sq


def project_seams(case, partials, hd_env=None):
    B, N = case.shape
    r = case.opts["r"]
    cols_layout, want_proj = case.opts.get("cols_layout", True), case.opts.get("want_proj", True)
    Xs, X, ls = pr.shifted_set(case.kind, case.D, B, N)
    P, Q = as_seen(Xs, case.dtype), as_seen(X, case.dtype)
    rows, J = case.rows("owned"), case.support("streamed")
    ref = FewHotReference(case, P, Q, rows, J, partials)
    Pt, Qt = T(P, case.dtype), T(Q, case.dtype)
    k = kstruct(case)
    rows_t = torch.from_numpy(rows).to(dev())
    Rf = few_hot(N, J, r, case.dtype, seed=6)
    Rdn = T(dense(N, r, case.dtype, seed=7), case.dtype)
    u = pr.unit_roundoff(case.dtype)
    with fresh_handle(hd_env) as hd:
        proj, sq = project(hd, k, Pt, Qt, T(Rf, case.dtype), r, cols_layout, want_proj, case.dtype)
        proj2, sq2 = project(hd, k, Pt, Qt, T(Rf, case.dtype), r, cols_layout, want_proj, case.dtype)
        pd, sd = project(hd, k, Pt, Qt, Rdn, r, cols_layout, want_proj, case.dtype)
        pd2, sd2 = project(hd, k, Pt, Qt, Rdn, r, cols_layout, want_proj, case.dtype)
        arena_proof(hd, case.plan)
    assert bool(torch.isfinite(sq).all()) and (not want_proj or bool(torch.isfinite(proj).all())), \
        f"{case.id}: an output element was never written (the NaN it was pre-filled with is still there)"
    # deterministic: bit-identical
    assert torch.equal(sq, sq2) and (not want_proj or torch.equal(proj, proj2)), case.id
    assert torch.equal(sd, sd2) and (not want_proj or torch.equal(pd, pd2)), case.id
    # (a)
    want, bound = ref.product(Rf)
    worst_a = 0.0
    if want_proj:
        worst_a = hold(f"{case.id} proj few-hot", proj[rows_t], want, bound)
    sq_want, sq_bound = sqnorm_bound(want, bound, r, u)
    worst_a = max(worst_a, hold(f"{case.id} sqnorm few-hot", sq[rows_t], sq_want, sq_bound))
    # (b): bar(kind), tests/test_gpu_love.py::test_project_matches_longdouble; fp32: 2e-4,
    # tests/test_gpu_love.py::test_project_fp32_takes_the_generic_route
    tol = bar(case.kind) if case.dtype == np.float64 else 2e-4
    pref = k_torch(case.kind, ls, Pt, Qt) @ Rdn.double()
    assert bool(torch.isfinite(sd).all())
    worst_b = relmax(sd, (pref * pref).sum(dim=1)) / tol
    if want_proj:
        assert bool(torch.isfinite(pd).all())
        worst_b = max(worst_b, relmax(pd, pref) / tol)
    assert worst_b < 1.0, (case.id, worst_b * tol)
    return worst_a, worst_b


@pytest.mark.parametrize("case", sp.cases("project_generic"), ids=repr)
def test_project_generic_seams(case):
    """project_generic (csrc/project.hip): `proj + i0 * r`, `sqnorm + i0`, `Rrows + j0`, the accumulate flag, and the
    `pc` scratch that stands in for proj when only the norms are asked for."""
    worst_a, worst_b = project_seams(case, len(case.plan.cuts("streamed")) + 1 + GEMM_SLICES)
    report("project_generic", f"{case.id} few-hot", worst_a)
    report("project_generic", f"{case.id} dense", worst_b)


@pytest.mark.parametrize("case", sp.cases("project_fused"), ids=repr)
def test_project_fused_seams(case):
    """project_fused_dp: one launch per 2^16 test rows (`proj + c0 * r`, `sqnorm + c0`, `Xs + c0 * D`), the two
    launches splitting N differently over one shared arena of partials.  The plan is made for this chip's CU count.
    The few-hot rows of R include both sides of every split boundary of either launch."""
    B, N = case.shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = sp.project_fused(B, N, case.D, case.opts["r"], cus)
    assert plan.launches[0][2:] != plan.launches[1][2:], plan.launches  # the launches split N differently
    live = sp.Case(case.entry, case.id, case.kind, case.dtype, case.D, case.shape, plan, case.targeted, **case.opts)
    worst_a, worst_b = project_seams(live, max(ns for _, _, ns, _ in plan.launches))
    report("project_fused", f"{case.id} few-hot", worst_a)
    report("project_fused", f"{case.id} dense", worst_b)


# ---------------------------------------------------------------- mgp_kxx_grad, panel route
def kxx_grad_on(hd, k, D, X, U, V, R):
    from cggp import _hip
    dv = ctypes.c_double(float("nan"))
    dl = (ctypes.c_double * _hip.MGP_MAX_D)(*([float("nan")] * D))
    p = _hip.ptr
    hd.check(hd.lib.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), X.shape[0], p(U), p(V), R, COLS, ctypes.byref(dv), dl))
    return dv.value, [dl[d] for d in range(D)]


@pytest.mark.parametrize("case", sp.cases("kxx_grad"), ids=repr)
def test_kxx_grad_panel_seams(case):
    """kgrad_panel (csrc/kxx_grad.hip): row panels of G = U V^T through mgp_k_dense_vjp(X + i0 * D, ...), added on the
    host.  U is few-hot in its rows (both sides of the panel cut, the first and last row, random ones), so the long-double
    reference runs over those rows alone; bars of tests/test_gpu_gpr_lml.py::test_kxx_grad_routes_and_determinism."""
    N, D, R = case.shape[0], case.D, 3
    X, _, ls = pr.shifted_set(case.kind, D, N, 64)
    X = as_seen(X, case.dtype)
    rows = sp.few_hot_indices(N, case.plan.cuts("rows"), 8, target=24)
    U = few_hot(N, rows, R, case.dtype, seed=9)
    V = dense(N, R, case.dtype, seed=10)
    k = kstruct(case)
    Xt, Ut, Vt = T(X, case.dtype), T(U, case.dtype), T(V, case.dtype)
    env = {"MGP_KXX_GRAD": "panel"} if case.opts["forced"] else None
    with fresh_handle(env) as hd:
        a = kxx_grad_on(hd, k, D, Xt, Ut, Vt, R)
        b = kxx_grad_on(hd, k, D, Xt, Ut, Vt, R)
        if case.opts["forced"]:  # dense U and V on the panel route, to be compared with the fused route
            Ud = T(dense(N, R, case.dtype, seed=11))
            panel = kxx_grad_on(hd, k, D, Xt, Ud, Vt, R)
            assert panel == kxx_grad_on(hd, k, D, Xt, Ud, Vt, R), case.id
        arena_proof(hd, case.plan)
    assert a == b, case.id  # deterministic: bit-identical
    assert np.isfinite(a[0]) and all(np.isfinite(a[1]))
    rv, rl, sv, sl = kxx_grad_reference(case.kind, VAR, ls, X, U, V, rows=rows)
    tol = 1e-11 if case.dtype == np.float64 else 1e-5
    ratios = [abs(a[0] - float(rv)) / (tol * float(sv))]
    ratios += [abs(a[1][d] - float(rl[d])) / (tol * float(sl[d])) for d in range(D)]
    report("kxx_grad", f"{case.id} few-hot", max(ratios))
    assert max(ratios) <= 1.0, (case.id, ratios)
    if case.opts["forced"]:
        with fresh_handle({"MGP_KXX_GRAD": "fused"}) as hf:
            fused = kxx_grad_on(hf, k, D, Xt, Ud, Vt, R)
            assert hf.lib.mgp_arena_bytes(hf.h, b"kgrad") < case.plan.arena[1]  # the pair kernel: nothing N x rows
        worst = max([abs(fused[0] - panel[0]) / abs(panel[0])] + [abs(x - y) / abs(y) for x, y in zip(fused[1], panel[1])])
        report("kxx_grad", f"{case.id} dense, fused against panel (bar 1e-11)", worst / 1e-11)
        assert worst <= 1e-11, (case.id, worst)
