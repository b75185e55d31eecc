"""Row F1 on the MI355X, every kernel form: `mgp_nearest_center` (`nearest_kernel` of csrc/cluster.hip at every padded
dimension, rows per thread, direct and expansion form; `nearest_generic_kernel` of csrc/generic.hip above D = 32) and the
cluster sums (`mgp_cluster_stats`, `mgp_segment_sums`) against the references of tests/assign_reference.py.  Every row
of every case is held to the rule of that module: the index is in range, no correct evaluation can prefer another
centre (which pins it exactly on decided rows, at least 97 % of every case), a bitwise copy of a lower-indexed centre
is never named, and `best` is within the derived bound of the long-double value at the chosen pair."""

import numpy as np
import pytest
import torch

import assign_reference as ar
import pair_reference as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VAR = ar.VARIANCE
WORST = {}  # route -> [worst err / bound of `best`, worst undecided share, cases]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nearest(case, X, Z, ls, want_best=True):
    from cggp import ops
    spec = ops.KernelSpec(case.kind, VAR, list(ls), case.D)
    out = ops.nearest_center(spec, T(X), T(Z), distance_type=ar.TYPES[case.dist_type], return_distance=want_best)
    idx, best = out if want_best else (out, None)
    return idx.cpu().numpy(), None if best is None else best.cpu().numpy()


def _run(route, case):
    X, Z, ls = case.inputs()
    idx, best = _nearest(case, X, Z, ls, case.want_best)
    rep = ar.check_assignment(case.id, case.dist_type, case.kind, VAR, ls, X, Z, idx, best)
    w = WORST.setdefault(route, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], rep.best_ratio or 0.0), max(w[1], rep.undecided_share), w[2] + 1
    print(f"{case.id}: undecided {rep.undecided_share:.2%}, best err / bound {rep.best_ratio}")
    return rep


@pytest.mark.parametrize("case", ar.fused_cases(), ids=lambda c: c.id)
def test_fused_route(case):
    _run("fused", case)


@pytest.mark.parametrize("case", ar.generic_cases(), ids=lambda c: c.id)
def test_generic_route(case):
    _run("generic", case)


def _rpt_id(i):
    c = ar.rpt_cases(ar.MI355X_CUS)[i]  # the table's order does not depend on the CU count, its N do: not in the id
    return f"rpt{c.rpt}-{ar.TYPES[c.dist_type]}-{c.kind}-D{c.D}-M{c.M}-{np.dtype(c.dtype).name}-{i}"


@pytest.mark.parametrize("i", range(len(ar.rpt_cases(ar.MI355X_CUS))), ids=_rpt_id)
def test_fused_route_rows_per_thread(i):
    """`nearest_t` (csrc/cluster.hip) takes rpt = D <= 8 ? 4 : 2 rows per thread and halves it while
    ceil(N / (256 rpt)) < 2 CUs: `assign_reference.rows_per_thread` mirrors that rule, and `rpt_cases` sizes N from the
    device's CU count so that every instantiation with 4 and with 2 rows per thread runs, with a last block whose strided
    rows run past N, and one block of rows under each threshold."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = ar.rpt_cases(cus)[i]
    assert ar.rows_per_thread(case.N, case.D, cus) == case.rpt
    _run(f"fused, {case.rpt} rows per thread", case)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("route,D", [("fused", 3), ("generic", 40)])
@pytest.mark.parametrize("pattern", ar.TIE_PATTERNS)
def test_first_index_on_ties(pattern, route, D, dtype):
    """Rule 3 on every duplicate pattern, all four distance types; 600 rows are several workgroups of either kernel."""
    N, ls = 600, pr.lengthscales(D)
    X, Z = ar.tie_set(pattern, D, N, dtype)
    first = ar.first_occurrence(Z)
    for t in range(4):
        case = ar.Case(dist_type=t, kind=pr.KINDS[t], D=D, N=N, M=Z.shape[0], dtype=dtype, points=pattern, want_best=True)
        idx, best = _nearest(case, X, Z, ls)
        ar.check_assignment(case.id, t, case.kind, VAR, ls, X, Z, idx, best)
        assert np.array_equal(first[idx], idx)
        if t == 1:  # the first 40 rows sit on copied centres
            assert np.all(best[:40] == 0)
        if pattern == "stack":
            alone, _ = _nearest(case, X, Z[:ar.TIE_M], ls, want_best=False)
            assert np.array_equal(idx, alone)


def _cluster_indices(pattern, N, M, rng):
    if pattern == "one":  # all rows in one cluster, the last
        return np.full(N, M - 1, dtype=np.int64)
    return (2 * rng.integers(0, max(1, M // 2), N)) % M  # every odd cluster stays empty


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("N", [1, 1023, 1025, 70001])
def test_cluster_sums(N, M, dtype):
    from cggp import ops
    rng = np.random.default_rng([N, M])
    worst = 0.0
    for C in (1, 3):
        Y = rng.standard_normal((N, C)).astype(dtype)
        for pattern in ("empty", "one"):
            idx = _cluster_indices(pattern, N, M, rng)
            y, it = T(Y if C > 1 else Y[:, 0]), T(idx)
            got = {}
            for method in ("sweep", "sorted"):
                sums, counts = ops.cluster_stats(it, y, M, method=method)
                again = ops.cluster_stats(it, y, M, method=method)
                assert torch.equal(sums, again[0]) and torch.equal(counts, again[1]), (method, C, pattern)
                assert sums.shape == ((M, C) if C > 1 else (M,)) and counts.shape == (M,) and sums.dtype == y.dtype
                got[method] = counts
                worst = max(worst, ar.check_cluster_sums(f"{method} C={C} {pattern}", idx, Y, M, sums.cpu().numpy(),
                                                         counts.cpu().numpy()))
            assert torch.equal(got["sweep"], got["sorted"])
    w = WORST.setdefault("cluster sums", [0.0, 0.0, 0])
    w[0], w[2] = max(w[0], worst), w[2] + 1
    print(f"N={N} M={M} {np.dtype(dtype).name}: worst err / bound {worst:.3f}")


def test_report_the_worst_ratios():
    """Informative: the worst err / bound of `best` (of the sums for the cluster sums) and the worst
    undecided share per route, over the cases of this run."""
    for route, (ratio, share, n) in WORST.items():
        print(f"{route}: {n} cases, worst err / bound {ratio:.3f}, worst undecided share {share:.2%}")
        assert ratio < 1.0
