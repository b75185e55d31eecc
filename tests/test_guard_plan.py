"""The guard plan on the CPU (tests/guard_plan.py; the values are checked by tests/test_gpu_cg_guards.py): its cases
can fail.  No case rests on a coin toss, every guard regime occurs in every family of kernels, a recurrence with one
guard or the stopping rule mutated fails at least one case of every family, and the cases reach every kernel site."""

import functools

import numpy as np
import pytest

import cg_route_plan as rp
import guard_plan as gp
from oracle import cg as ocg

F64 = [c for c in gp.CASES if c.dtype == "f64"]


@functools.lru_cache(maxsize=4)
def _matrix(n, system, jacobi):
    return gp.operator_matrix(next(c for c in gp.CASES if (c.n, c.system, c.pre == "jacobi") == (n, system, jacobi)))


def matrix(case):
    return _matrix(case.n, case.system, case.pre == "jacobi")


def by_system(cases):
    return sorted(cases, key=lambda c: (c.n, c.system, c.pre == "jacobi", c.id))


def test_ids_are_unique_and_the_systems_are_what_the_plan_says():
    assert len({c.id for c in gp.CASES}) == len(gp.CASES)
    n = 257
    A, U = gp.matrix(n), gp.basis(n)
    assert np.array_equal(A, A.T) and np.array_equal(A, gp.matrix(n))
    assert np.allclose(U.T @ U, np.eye(gp.Q), atol=1e-14)
    lam = np.linalg.eigvalsh(A)
    assert np.allclose(lam[:n - gp.Q], 2.0, atol=1e-13) and np.allclose(lam[n - gp.Q:], 2.0 + np.arange(1, gp.Q + 1), atol=1e-13)
    assert np.allclose(A @ gp.column("d", n), 3.0 * gp.column("d", n), atol=1e-13)  # an eigenvector
    assert not np.any(gp.column("b", n)) and abs(np.sum(gp.column("c", n) ** 2) - 9e-20) < 1e-32
    P = gp.dense_pinv(n)
    assert np.array_equal(P, P.T) and np.allclose(P @ A, A @ P, atol=1e-13) and np.linalg.eigvalsh(P)[0] > 0.49
    # the Jacobi cases: a similarity transform of the same system by a diagonal that varies
    case = next(c for c in gp.CASES if c.id == "fused-250-jacobi")
    D = gp.jacobi_diagonal(250)
    assert D.min() >= 1.0 and D.max() <= 3.0 and D.max() / D.min() > 2.5
    assert np.allclose(gp.operator_matrix(case) / np.sqrt(np.outer(D, D)), gp.matrix(250), atol=1e-14)
    for c in gp.CASES:
        assert gp.rhs(c).shape == (c.Bt, c.n) == gp.start(c).shape
        assert bool(np.any(gp.start(c))) == (c.start == "v0")


@pytest.mark.parametrize("case", [c for c in by_system(gp.CASES) if c.n <= 2200], ids=repr)
def test_the_unmutated_recurrence_is_the_oracle(case):
    A = matrix(case)
    dt = np.float64 if case.dtype == "f64" else np.float32
    pre = gp.host_preconditioner(case, A)
    for k in case.ks + ((None,) if case.thr else ()):
        v, steps, err, _, coef, _ = gp.run(case, k, dtype=dt, A=A)
        cap = k if k is not None else case.cap
        o_v, (o_steps, o_err) = ocg.conjugate_gradient(
            A.astype(dt), gp.rhs(case).astype(dt), gp.start(case).astype(dt), 0.0 if k is not None else case.thr, pre,
            max_iterations=cap, max_steps_cycle=case.cycle if case.cycle is not None else cap + 1,
            min_float=case.min_float)
        assert steps == o_steps and (k is None or steps == k)
        assert np.array_equal(v, o_v, equal_nan=True) and np.array_equal(err, o_err, equal_nan=True)
        assert coef.shape == (steps, case.Bt, 3)


@pytest.mark.parametrize("case", by_system(F64), ids=repr)
def test_no_case_rests_on_a_coin_toss(case):
    """Every rz_old and p.Ap of every step and column is at least a factor 10 away from min_float, every 0.5 ||r||^2 of
    the stopping run from the threshold.  Exact zeros (the zero column) are computed exactly in any order."""
    worst = gp.determinate(case, matrix(case))
    print(f"{case.id}: closest approach a factor {worst:.3g}")
    assert worst >= gp.FACTOR


def test_the_stopping_runs_end_where_the_construction_says():
    for case in by_system(c for c in F64 if c.thr and c.n <= 2200):
        steps = gp.run(case, None, A=matrix(case))[1]
        if case.system == "unit" and case.cycle is None and case.pre != "block":
            # q + 1 steps whenever a column that lives that long is in the batch; column e alone: three
            # q + 1 steps whenever a column that lives that long is in the batch; column e alone: three.  Under
            # min_float = 1e-6 column j is frozen ABOVE the threshold and holds the loop to the cap
            assert steps == (case.cap if "j" in case.cols else gp.Q + 1 if set(case.cols) & set("afghi") else 3), case.id
        else:
            assert steps == case.cap, case.id  # matrix-free: the cap, with a column under the threshold from the start


def test_every_regime_occurs_in_every_family():
    for fam in gp.FAMILIES[:-1]:  # matfree: columns a, b, c on kernel matrices -- frozen from step 0 beside a live one
        seen = set()
        for case in by_system(c for c in F64 if c.family == fam and c.n <= 5000):
            reg = gp.regimes(case, matrix(case))
            last_live = max([max(r["live"] + r["gamma_only"] + r["beta_only"], default=-1) for r in reg])
            for r in reg:
                if r["frozen_from"] == 0:
                    seen.add("frozen from step 0")
                elif r["frozen_from"] is not None and r["frozen_from"] <= last_live:
                    seen.add("frozen after converging beside a live column")
                if r["gamma_only"]:
                    seen.add("gamma zeroed, beta kept")
                if r["beta_only"]:
                    seen.add("beta dropped, gamma taken")
        assert len(seen) == 4, (fam, seen)
    for case in (c for c in F64 if c.family == "matfree"):
        reg = gp.regimes(case, matrix(case))
        assert any(r["frozen_from"] == 0 for r in reg) and any(len(r["live"]) == max(case.ks) for r in reg), case.id


def test_every_mutation_fails_a_case_of_every_family():
    """A recurrence without the gamma guard, without the beta guard, with both guards or the stopping rule read from
    column 0, with < for <=, or with the floor fixed at 1e-16: per family, the first case that notices and how."""
    with np.errstate(all="ignore"):
        for fam in gp.FAMILIES:
            cases = by_system(c for c in F64 if c.family == fam and c.n <= 5000)
            for mutation in gp.MUTATIONS:
                hit = next(((c.id, why) for c in cases for why in [gp.killed_by(c, mutation, matrix(c))] if why), None)
                print(f"{fam:8s} {mutation:22s} {hit}")
                assert hit is not None, (fam, mutation)


def test_fp32_notes_are_the_oracles_own_distance():
    f32 = [c for c in gp.CASES if c.dtype == "f32"]
    assert {c.family for c in f32} == set(gp.FAMILIES[:5])
    for case in f32:
        assert max(case.ks) == 3 and set("bcf") <= set(case.cols) and not set("de") & set(case.cols)
        own = gp.f32_distance(case, matrix(case))
        print(f"{case.id}: measured {own[0]:.2e} {own[1]:.2e}, note {case.note}")
        assert all(abs(m - r) <= 0.06 * r for m, r in zip(own, case.note)), (case.id, own)  # two digits are recorded


def test_the_cases_reach_every_site():
    by = {f: [c for c in gp.CASES if c.family == f] for f in gp.FAMILIES}
    # fused update: both thread counts, EPT 1, 2 (x2) and 4, Eye and Jacobi; nine columns keep the tile scheme away
    fused = [c for c in by["fused"] if c.system == "unit" and c.min_float == gp.FLOOR]
    for pre in ("eye", "jacobi"):
        tiers = {rp.fused_tier(c.n) for c in fused if c.pre == pre}
        assert tiers == {(1, 256), (1, 1024), (4, 1024), (8, 1024)}, (pre, tiers)  # n = 250, 513, 2049, 4097
    assert all(c.route.fused and gp.dense1_form(c) is None and (c.Bt == 9 or c.n < 1024) for c in by["fused"])
    # generic update: all six modes, both block sizes, none on the tile scheme
    modes = set()
    for c in by["generic"]:
        modes |= c.route.modes
        assert gp.dense1_form(c) is None
    assert modes == {0, 1, 2, 3, 4, 5}
    assert {rp.update_threads(c.n) for c in by["generic"]} == {256, 1024}
    assert any(c.route.modes == {0} and not c.route.fused for c in by["generic"])  # mode 0 alone: block, n > 8192
    # the three forms of cg_dense1.hip by their size rules
    for fam in ("tile", "full", "blk"):
        assert all(gp.dense1_form(c) == fam for c in by[fam]), fam
    assert {c.Bt for c in by["tile"] if c.system == "unit"} >= {1, 3, 6, 8}
    assert {c.pre for c in by["tile"]} == {c.pre for c in by["full"]} == {"eye", "jacobi"}
    assert {c.Bt for c in by["full"]} >= {1, 6} and {c.Bt for c in by["blk"]} >= {1, 6}
    assert any(c.n % 64 and -(-c.n // 64) % 3 for c in by["blk"])
    # the recording solve takes the fused kernel, not the tile scheme; the matrix-free cases: both operators, low rank
    assert all(c.record and c.pre == "eye" and gp.dense1_form(c) is None for c in by["record"])
    assert {(c.system, c.pre) for c in by["matfree"]} == {("kxx", "eye"), ("kxx", "lowrank"), ("kmm", "eye")}
    # every family but the matrix-free one meets the other floors and both scaled systems
    for fam in gp.FAMILIES[:-1]:
        assert {c.min_float for c in by[fam]} >= {gp.FLOOR, 1e-6, 1e-300, 0.0}, fam
        assert {c.system for c in by[fam]} == {"unit", "small", "large"}, fam
        assert {c.Bt for c in by[fam] if c.system != "unit"} == {1, 3}, fam
