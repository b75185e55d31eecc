"""tests/assign_reference.py held honest on the CPU: a numpy emulation of both distance forms of csrc/cluster.hip and
csrc/generic.hip stays inside its bounds on every point set tests/test_gpu_assign.py uses, the undecided share of every
planned case is under the cap, and torch-CPU stand-ins that commit one fault each are rejected (the precedent of
tests/test_buffer_contract_host.py)."""

import numpy as np
import pytest
import torch

import assign_reference as ar
import pair_reference as pr

LD = np.longdouble
VAR = ar.VARIANCE
SHARE_ROWS = 1 << 16  # of the rows-per-thread cases (independent, identically drawn rows); the GPU test takes them all
EMULATED_ROWS = 64  # rows are independent: the first 64 of a case show its point set


def _fma(a, b, c, T):
    """One rounding: the long-double product of two values of T carries 2^-64 at most."""
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(T)


def emulate(route, dist_type, kind, ls, X, Z):
    """s [N, M] in the arithmetic of `nearest_kernel` ("fused") or `nearest_generic_kernel` ("generic"), operation by
    operation, in the inputs' dtype."""
    T = X.dtype.type
    D = X.shape[1]
    inv = np.ones(D) if dist_type <= 1 else float(pr.profile_scale(kind)) / np.asarray(ls, dtype=np.float64)
    a, b = X * inv.astype(T), Z * inv.astype(T)  # fl(x fl(c / l))
    shape = (X.shape[0], Z.shape[0])
    if dist_type == 1:
        s = np.zeros(shape, dtype=T)
        for d in range(D):
            df = a[:, None, d] - b[None, :, d]
            s = _fma(df, df, s, T)
        return s
    a2, b2 = np.zeros(X.shape[0], dtype=T), np.zeros(Z.shape[0], dtype=T)
    for d in range(D):
        a2, b2 = _fma(a[:, d], a[:, d], a2, T), _fma(b[:, d], b[:, d], b2, T)
    if route == "fused":
        s = b2[None, :] + a2[:, None]
        for d in range(D):
            s = _fma(np.broadcast_to(-a[:, None, d], shape), np.broadcast_to(b[None, :, d] + b[None, :, d], shape), s, T)
        return s
    acc = np.zeros(shape, dtype=T)
    for d in range(D):
        acc = _fma(np.broadcast_to(a[:, None, d], shape), np.broadcast_to(b[None, :, d], shape), acc, T)
    return _fma(np.full(shape, -2, dtype=T), acc, np.broadcast_to(b2[None, :], shape), T) + a2[:, None]


def _emulated_ratio(route, case):
    X, Z, ls = case.inputs()
    X = X[:EMULATED_ROWS]
    s, bound = ar.distances(case.dist_type, case.kind, ls, X, Z)
    err = np.abs(emulate(route, case.dist_type, case.kind, ls, X, Z).astype(LD) - s).astype(np.float64)
    assert np.all(err[bound == 0] == 0), case.id
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("route,cases", [("fused", ar.fused_cases()), ("generic", ar.generic_cases()),
                                         ("fused", ar.rpt_cases(ar.MI355X_CUS))], ids=["fused", "generic", "rpt"])
def test_emulated_kernels_stay_inside_the_bound(route, cases):
    worst = {}
    for case in cases:
        key = ("direct" if case.dist_type == 1 else "expansion", np.dtype(case.dtype).name)
        worst[key] = max(worst.get(key, 0.0), _emulated_ratio(route, case))
    print(f"{route}: worst emulated err / bound {worst}")
    assert len(worst) == 4 and max(worst.values()) < 1.0, worst


def test_emulated_tie_sets_give_equal_bits_for_equal_centres():
    """What rule 3 rests on: a copy's distance is the same bits as the original's, on both routes and both forms."""
    for route, D in (("fused", 3), ("generic", 40)):
        for dtype in (np.float64, np.float32):
            for pattern in ar.TIE_PATTERNS:
                X, Z = ar.tie_set(pattern, D, 64, dtype)
                first = ar.first_occurrence(Z)
                assert (first != np.arange(Z.shape[0])).sum() == (ar.TIE_M if pattern == "stack" else 20)
                for t in (0, 1, 2):
                    s = emulate(route, t, "matern52", pr.lengthscales(D), X, Z)
                    assert np.array_equal(s, s[:, first])


@pytest.mark.parametrize("family,cases", [("fused", ar.fused_cases()), ("generic", ar.generic_cases()),
                                          ("rpt", ar.rpt_cases(ar.MI355X_CUS))], ids=["fused", "generic", "rpt"])
def test_undecided_share_of_every_planned_case(family, cases):
    worst, total, rows = 0.0, 0, 0
    for case in cases:
        X, Z, ls = case.inputs()
        X = X[:SHARE_ROWS]
        rep = ar.check_assignment(case.id, case.dist_type, case.kind, VAR, ls, X, Z)  # asserts the cap
        worst = max(worst, rep.undecided_share)
        total, rows = total + int((~rep.decided).sum()), rows + X.shape[0]
    print(f"{family}: {len(cases)} cases, worst undecided share {worst:.2%}, {total} of {rows} rows in all")


def test_tables_cover_what_they_claim():
    for cases, Ds, Ns, Ms in ((ar.fused_cases(), ar.FUSED_DS, ar.FUSED_NS, ar.FUSED_MS),
                              (ar.generic_cases(), ar.GENERIC_DS, ar.GENERIC_NS, ar.GENERIC_MS)):
        assert {(c.N, c.M) for c in cases} == {(n, m) for n in Ns for m in Ms}
        assert {(c.D, np.dtype(c.dtype).name, c.dist_type) for c in cases} == \
            {(D, t, k) for D in Ds for t in ("float64", "float32") for k in range(4)}
        for D in Ds:
            assert {c.kind for c in cases if c.D == D and c.dist_type >= 2} == set(pr.KINDS)
            assert len({c.kind for c in cases if c.D == D and c.dist_type <= 1}) >= 2
        assert {c.points for c in cases} == set(ar.SETS) and {c.want_best for c in cases} == {True, False}
    rpt = ar.rpt_cases(ar.MI355X_CUS)
    assert {(c.rpt, c.D <= 8) for c in rpt} == {(4, True), (2, True), (2, False), (1, True), (1, False)}
    assert ar.rows_per_thread(100_000, 8, ar.MI355X_CUS) == 1 and ar.rows_per_thread(1 << 20, 8, ar.MI355X_CUS) == 4


# ---------------------------------------------------------------- stand-ins that commit one fault each
def standin_nearest(X, Z, dist_type, kind, variance, ls, fault=None):
    """argmin and best distance by torch on the CPU (expansion form, direct for type 1), with one fault on request."""
    Xt, Zt = torch.from_numpy(X), torch.from_numpy(Z)
    if dist_type >= 2:
        inv = torch.from_numpy((float(pr.profile_scale(kind)) / np.asarray(ls)).astype(X.dtype))
        Xt, Zt = Xt * inv, Zt * inv
    if dist_type == 1:
        d = ((Xt[:, None, :] - Zt[None, :, :]) ** 2).sum(-1)
    else:
        d = (Xt * Xt).sum(1)[:, None] + (Zt * Zt).sum(1)[None, :] - 2.0 * Xt @ Zt.T
    N, M = d.shape
    if fault == "last_centre_never_visited":
        d[:, M - 1] = float("inf")
    elif fault == "first_column_of_second_tile_skipped":
        d[:, 128] = float("inf")
    if fault == "last_index_on_ties":
        idx = M - 1 - torch.argmin(d.flip(1), dim=1)
    else:
        idx = torch.argmin(d, dim=1)  # first index on ties
    s = d.gather(1, idx[:, None])[:, 0]
    if fault == "best_from_the_runner_up":
        s = d.topk(2, dim=1, largest=False).values[:, 1]
    if fault == "last_block_unassigned":
        idx[N - N % 256:] = -1  # what an output buffer filled with a sentinel keeps
    elif fault == "last_block_left_at_zero":
        idx[N - N % 256:] = 0
    if dist_type == 0:
        best = s
    elif dist_type == 1:
        best = s.clamp(min=0).sqrt()
    else:
        r2 = (s / float(pr.profile_scale(kind) ** 2)).clamp(min=1e-36).double().numpy()
        rho = torch.from_numpy(pr.k_over_variance(kind, r2.astype(LD), np.zeros_like(r2, dtype=LD)).astype(X.dtype))
        best = 2.0 * variance * (1.0 - rho) if dist_type == 2 else 1.0 - rho
    return idx.numpy(), best.numpy().astype(X.dtype)


FAULTS = ["last_index_on_ties", "last_centre_never_visited", "first_column_of_second_tile_skipped",
          "last_block_unassigned", "last_block_left_at_zero", "best_from_the_runner_up"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("dist_type", range(4), ids=ar.TYPES)
def test_a_correct_standin_passes_and_every_fault_is_rejected(dist_type, dtype):
    D, N, kind = 3, 1200, "matern32"  # a last block of 176 rows
    ls = pr.lengthscales(D)
    X, Z = ar.tie_set("+150", D, N, dtype)
    idx, best = standin_nearest(X, Z, dist_type, kind, VAR, ls)
    rep = ar.check_assignment("correct", dist_type, kind, VAR, ls, X, Z, idx, best)
    assert rep.best_ratio < 1.0 and np.array_equal(idx[rep.decided], rep.ref_idx[rep.decided])
    for fault in FAULTS:
        fidx, fbest = standin_nearest(X, Z, dist_type, kind, VAR, ls, fault)
        assert not (np.array_equal(fidx, idx) and np.array_equal(fbest, best)), fault
        with pytest.raises(AssertionError, match="rule [123]|best"):
            ar.check_assignment(fault, dist_type, kind, VAR, ls, X, Z, fidx, fbest)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_one_row_dropped_from_a_cluster_sum_is_rejected(dtype):
    rng = np.random.default_rng(3)
    N, M, C = 5000, 70, 3
    idx = rng.integers(0, M - 1, N)  # the last cluster stays empty
    Y = rng.standard_normal((N, C)).astype(dtype)
    Yt, it = torch.from_numpy(Y), torch.from_numpy(idx)
    sums = torch.zeros((M, C), dtype=Yt.dtype).index_add_(0, it, Yt).numpy()
    counts = torch.bincount(it, minlength=M).to(Yt.dtype).numpy()
    assert ar.check_cluster_sums("correct", idx, Y, M, sums, counts) < 1.0
    row = int(np.flatnonzero(np.abs(Y[:, 1]) < 0.05)[0])  # a small term, still 100 times the float32 bound of its cluster
    dropped = sums.copy()
    dropped[idx[row], 1] -= Y[row, 1]
    with pytest.raises(AssertionError, match="sums outside"):
        ar.check_cluster_sums("dropped row", idx, Y, M, dropped, counts)
    miscounted = counts.copy()
    miscounted[idx[row]] -= 1
    with pytest.raises(AssertionError, match="counts differ"):
        ar.check_cluster_sums("dropped count", idx, Y, M, sums, miscounted)
