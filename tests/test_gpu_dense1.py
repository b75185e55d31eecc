"""The reference's literal CG loop -- ONE right-hand side on a dense matrix, `p @ A` of
`cggp/conjugate_gradient.py:65` with `A = Kmm + Lambda` (`cggp/models.py:301-303,337-339`) -- at the sizes where
libmgp runs it as the two-launch iteration of `csrc/cg_dense1.hip` (n >= 1024: tile kernel with the direction formed
on the fly + chunk-local update kernel).  The small-n tests of tests/test_gpu_parity.py never reach that path.

Against `oracle/cg.py` (line-for-line restatement of `conjugate_gradient.py:44-122`): iterate and error statistic
after exactly k steps, step counts and stopping quantity of converged solves, the iteration cap, the guard floor,
Jacobi preconditioning, an initial solution, ragged n (n % 64 != 0), fp32, and -- the path change must not be
visible -- agreement with the several-right-hand-side path (a different set of kernels) on the same system.
One kernel family carries 1 .. 8 columns on the two-launch form: a column's iterate is the same bits alone and in
company (test_a_column_does_not_depend_on_its_company).
"""

import functools

import numpy as np
import pytest
import torch

from oracle import cg as ocg
from oracle import kernels as ok
from oracle import models as om

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def relerr(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref)))


def problem(n, seed=0, noise=0.1, d=3):
    """K_SE(Z, Z) + Lambda with cluster-count-like diagonal (models.py:226-228: sigma^2 / counts)."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, d))
    kern = ok.Kernel("se", 1.3, rng.random(d) ** 2 + 0.5)
    counts = rng.integers(1, 40, n).astype(np.float64)
    A = om.add_diagonal(kern.K(Z), noise / counts)
    rhs = rng.standard_normal((n, 1))
    return A, rhs


@pytest.mark.parametrize("n", [1024, 1025, 2048, 3000, 4096])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_fixed_steps_match_oracle(n, k):
    from cggp.conjugate_gradient import conjugate_gradient
    A, rhs = problem(n, seed=n)
    z = torch.zeros((1, n), dtype=torch.float64, device=dev())
    sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), z, 0.0, max_iterations=k, max_steps_cycle=k + 1)
    o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs.T, np.zeros((1, n)), 0.0, max_iterations=k,
                                                     max_steps_cycle=k + 1)
    assert int(steps) == k == o_steps
    assert relerr(sol, o_sol) < 1e-9
    assert abs(float(err) - float(o_err[0, 0])) / float(o_err[0, 0]) < 1e-6


def test_thirty_steps_well_conditioned():
    from cggp.conjugate_gradient import conjugate_gradient
    n = 1536
    Q = np.random.default_rng(9).standard_normal((n, n))
    A = Q @ Q.T / n + 2.0 * np.eye(n)
    rhs = np.random.default_rng(10).standard_normal((n, 1))
    sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), None, 0.0, max_iterations=30, max_steps_cycle=31)
    o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs.T, np.zeros((1, n)), 0.0, max_iterations=30,
                                                     max_steps_cycle=31)
    assert int(steps) == 30 == o_steps and relerr(sol, o_sol) < 1e-9
    assert abs(float(err) - float(o_err[0, 0])) / float(o_err[0, 0]) < 1e-6


@pytest.mark.parametrize("n", [1024, 2500, 4096, 8192])
@pytest.mark.parametrize("thr", [1e-6, 1e-12])
def test_converged_solve_facade(n, thr):
    """`ConjugateGradient.__call__` defaults (`conjugate_gradient.py:190-196`: cap n, no refresh): where the loop
    stops, the stopping quantity on the TRUE residual, and the distance to the exact solution."""
    from cggp.conjugate_gradient import ConjugateGradient
    A, rhs = problem(n, seed=n + 1, noise=0.3)
    cg = ConjugateGradient(thr)
    sol, (steps, err) = cg.solve_with_stats(T(A), T(rhs))
    o_sol, (o_steps, o_err) = ocg.ConjugateGradient(thr).solve_with_stats(A, rhs)
    assert sol.shape == (n, 1) and err.shape == (1, 1)
    # where the loop stops depends on rounding once orthogonality is lost: over hundreds of steps two correct
    # implementations (the oracle against itself under a permutation of the system; the
    # two-launch path / round-2 kernels (MGP_CG_DENSE1=0) / oracle: 553 / 551 / 542 steps at n = 2500, 1039 / 1029 / 1061 at 8192) cross the threshold a few
    # per cent apart.  What is pinned is the stopping quantity and the distance to the exact solution.
    print(f"\nn={n} thr={thr}: steps HIP {int(steps)} oracle {o_steps}")
    assert abs(int(steps) - o_steps) <= max(4, 0.05 * o_steps) and int(steps) < n
    s = sol.cpu().numpy()
    r = rhs - A @ s
    assert 0.5 * float(np.sum(r * r)) <= thr * (1 + 1e-6) + 1e-20
    assert float(err) <= thr
    exact = np.linalg.solve(A, rhs)
    scale = np.linalg.norm(exact)
    # both are as far from the exact solution as the threshold leaves them
    e_hip, e_or = np.linalg.norm(s - exact) / scale, np.linalg.norm(o_sol - exact) / scale
    assert e_hip <= 4 * e_or + 1e-12, (e_hip, e_or)
    if thr <= 1e-12:
        assert relerr(sol, o_sol) < 1e-6


def test_iteration_cap_zero_rhs_and_zero_cap():
    from cggp.conjugate_gradient import conjugate_gradient
    n = 1300
    A, rhs = problem(n, seed=3)
    _, (steps, _) = conjugate_gradient(T(A), T(rhs.T), None, 0.0, max_iterations=7, max_steps_cycle=8)
    assert int(steps) == 7
    z = torch.zeros((1, n), dtype=torch.float64, device=dev())
    sol, (steps, err) = conjugate_gradient(T(A), z, z.clone(), 1e-6, max_iterations=n, max_steps_cycle=n + 1)
    assert int(steps) == 0 and float(sol.abs().max()) == 0.0 and float(err.abs().max()) == 0.0
    sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), None, 1e-6, max_iterations=0, max_steps_cycle=1)
    assert int(steps) == 0 and float(sol.abs().max()) == 0.0
    assert abs(float(err) - 0.5 * float(np.sum(rhs * rhs))) / float(np.sum(rhs * rhs)) < 1e-12


def test_check_every_does_not_change_the_result():
    """Iterations enqueued past convergence are no-ops: step count and iterate do not depend on the poll period."""
    from cggp.conjugate_gradient import conjugate_gradient
    n = 2048
    A, rhs = problem(n, seed=5, noise=0.5)
    out = []
    for ce in (1, 7, 64):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), None, 1e-8, max_iterations=n, max_steps_cycle=n + 1,
                                               check_every=ce)
        out.append((int(steps), sol.clone(), float(err)))
    assert out[0][0] == out[1][0] == out[2][0] and out[0][0] < n
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][1], out[2][1])
    assert out[0][2] == out[1][2] == out[2][2]


def test_guard_floor():
    from cggp.conjugate_gradient import ConjugateGradient
    n = 1100
    A, rhs = problem(n, seed=6, noise=1.0)
    cap = 400
    sol, (steps, err) = ConjugateGradient(1e-30, max_iterations=cap).solve_with_stats(T(A), T(rhs))
    o_sol, (o_steps, o_err) = ocg.ConjugateGradient(1e-30, max_iterations=cap).solve_with_stats(A, rhs)
    assert int(steps) == cap == o_steps
    assert relerr(sol, o_sol) < 1e-8 and float(err) < 1e-15 and torch.isfinite(sol).all()


@pytest.mark.parametrize("n", [1024, 3001])
def test_jacobi_preconditioner(n):
    from cggp.conjugate_gradient import ConjugateGradient, JacobiPreconditioner, conjugate_gradient
    A, rhs = problem(n, seed=7)
    A = A * np.outer(np.linspace(1, 3, n), np.linspace(1, 3, n))  # a diagonal worth scaling by
    pre, o_pre = JacobiPreconditioner(), ocg.JacobiPreconditioner()
    for k in (1, 4, 8):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), None, 0.0, pre, max_iterations=k, max_steps_cycle=k + 1)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs.T, np.zeros((1, n)), 0.0, o_pre, max_iterations=k,
                                                         max_steps_cycle=k + 1)
        assert int(steps) == k == o_steps and relerr(sol, o_sol) < 1e-9
        assert abs(float(err) - float(o_err[0, 0])) / abs(float(o_err[0, 0])) < 1e-6
    sol, (steps, _) = ConjugateGradient(1e-10, pre).solve_with_stats(T(A), T(rhs))
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-10, o_pre).solve_with_stats(A, rhs)
    assert abs(int(steps) - o_steps) <= max(4, 0.05 * o_steps)  # see test_converged_solve_facade
    r = rhs - A @ sol.cpu().numpy()
    assert 0.5 * float(np.sum(r * r)) <= 1e-10 * (1 + 1e-6)


def test_initial_solution():
    from cggp.conjugate_gradient import ConjugateGradient
    n = 1500
    A, rhs = problem(n, seed=8, noise=0.4)
    ref = np.linalg.solve(A, rhs)
    _, (steps, _) = ConjugateGradient(1e-10).solve_with_stats(T(A), T(rhs), initial_solution=T(ref))
    assert int(steps) == 0
    v0 = ref + 1e-3 * np.random.default_rng(1).standard_normal(ref.shape)
    sol, (steps, err) = ConjugateGradient(1e-14, max_iterations=300).solve_with_stats(T(A), T(rhs), initial_solution=T(v0))
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-14, max_iterations=300).solve_with_stats(A, rhs, initial_solution=v0)
    assert abs(int(steps) - o_steps) <= max(3, 0.05 * o_steps) and relerr(sol, o_sol) < 1e-7


def test_one_column_agrees_with_the_several_column_path():
    """Bt = 1 runs cg_dense1.hip; Bt = 2 with the same column twice runs the skinny product + fused update.  Two
    sets of kernels, one recurrence: fixed steps agree to rounding, converged solves to the threshold's bound."""
    from cggp.conjugate_gradient import conjugate_gradient
    n = 2048
    A, rhs = problem(n, seed=11)
    b1 = T(rhs.T)
    b2 = T(np.concatenate([rhs.T, rhs.T], 0))
    for k in (3, 8):
        s1, (k1, e1) = conjugate_gradient(T(A), b1, None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        s2, (k2, e2) = conjugate_gradient(T(A), b2, None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        assert int(k1) == int(k2) == k
        assert float((s1[0] - s2[0]).abs().max() / s2[0].abs().max()) < 1e-10
        assert abs(float(e1[0]) - float(e2[0])) / float(e2[0]) < 1e-8
    # run-to-run: bit-identical
    s1b, _ = conjugate_gradient(T(A), b1, None, 0.0, max_iterations=8, max_steps_cycle=9)
    assert torch.equal(s1, s1b)


@pytest.mark.parametrize("n", [1024, 2050, 4096, 8000])
@pytest.mark.parametrize("Bt", [2, 5, 8])
def test_several_columns_on_the_tile_scheme(n, Bt):
    """2 .. 8 right-hand sides (the reference's default num_probes = 5, cggp/models.py:286): the two-launch tile scheme
    with BT columns (csrc/cg_dense1.hip, d1_tile_kernel<BT> + d1_update_kernel) where it is the faster route (Bt <= 4 at n <= 4096, <= 6 above; every
    BT up to 8 is forced through it in test_every_form_...), the skinny product + fused update otherwise -- either
    way: k steps against the oracle, column by column; the `any`
    stopping rule (:59-62) -- all columns iterate until the slowest one is under the threshold; run-to-run identity;
    and the same columns one at a time through the one-column forms."""
    from cggp.conjugate_gradient import JacobiPreconditioner, conjugate_gradient
    A, _ = problem(n, seed=n + Bt)
    rng = np.random.default_rng(Bt)
    rhs = rng.standard_normal((Bt, n)) * (10.0 ** rng.integers(-3, 3, (Bt, 1)))  # columns of very different size
    for k in (1, 4, 7):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, max_iterations=k,
                                                         max_steps_cycle=k + 1)
        assert int(steps) == k == o_steps and sol.shape == (Bt, n) and err.shape == (Bt, 1)
        for b in range(Bt):
            assert relerr(sol[b], o_sol[b]) < 1e-9, (k, b)
            assert abs(float(err[b]) - float(o_err[b, 0])) / float(o_err[b, 0]) < 1e-8
    again, _ = conjugate_gradient(T(A), T(rhs), None, 0.0, max_iterations=7, max_steps_cycle=8, check_every=3)
    assert torch.equal(sol, again)
    # a converged solve: the step count is that of the slowest column, every column meets the rule on its TRUE residual
    thr = 1e-8
    s, (ks, es) = conjugate_gradient(T(A), T(rhs), None, thr, max_iterations=n, max_steps_cycle=n + 1, check_every=16)
    assert int(ks) < n
    if n <= 4096:  # (the oracle's converged several-column solve at n = 8000 is 40 s of numpy per case)
        o_s, (o_ks, _) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), thr, max_iterations=n, max_steps_cycle=n + 1)
        assert abs(int(ks) - o_ks) <= max(3, o_ks // 20)
    res = rhs - s.cpu().numpy() @ A
    assert np.all(0.5 * np.sum(res * res, axis=1) <= thr * (1 + 1e-6) + 1e-16)
    # Jacobi + an initial solution, three steps
    if n <= 4096:
        v0 = 0.01 * rng.standard_normal((Bt, n))
        sj, (kj, ej) = conjugate_gradient(T(A), T(rhs), T(v0), 0.0, JacobiPreconditioner(), max_iterations=3,
                                          max_steps_cycle=4)
        o_sj, _ = ocg.conjugate_gradient(A, rhs, v0, 0.0, ocg.JacobiPreconditioner(), max_iterations=3, max_steps_cycle=4)
        assert relerr(sj, o_sj) < 1e-9


@functools.lru_cache(maxsize=1)  # the cases come grouped by system; the oracle runs once per (system, Jacobi)
def company_system(n, dtype, cols):
    """fp64: `problem` with a diagonal worth scaling by (test_jacobi_preconditioner); fp32: the system of test_fp32,
    rounded to float32.  `cols` right-hand sides; with the k = 5 oracle iterates, Jacobi off and on."""
    A, _ = problem(n, seed=n, noise=0.1 if dtype == "f64" else 1.0)
    if dtype == "f64":
        A = A * np.outer(np.linspace(1, 3, n), np.linspace(1, 3, n))
    rhs = np.random.default_rng(n + cols).standard_normal((cols, n))
    if dtype == "f32":
        A, rhs = A.astype(np.float32).astype(np.float64), rhs.astype(np.float32).astype(np.float64)
    oracle = {}
    for jac in (False, True):
        pre = ocg.JacobiPreconditioner() if jac else None
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((cols, n)), 0.0, pre, max_iterations=5,
                                                         max_steps_cycle=6)
        assert o_steps == 5
        oracle[jac] = (o_sol, o_err)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    return T(A, tdt), T(rhs, tdt), oracle


# n: the smallest sizes, all with a ragged last tile, that reach each instantiation of the update kernel --
# nt = 17 <256, 8, 3>, nt = 34 <256, 16, 9>, nt = 66 <512, 16, 17>
@pytest.mark.parametrize("n,dtype,cols,jac", [(1025, "f64", 3, False), (1025, "f64", 3, True), (1025, "f64", 8, False),
                                              (1025, "f32", 3, False), (2113, "f64", 3, False),
                                              (2113, "f64", 3, True), (4161, "f64", 3, False),
                                              (4161, "f64", 3, True)])
def test_a_column_does_not_depend_on_its_company(n, dtype, cols, jac, monkeypatch):
    """Two launches per iteration (MGP_CG_DENSE1=1; MGP_CG_DENSE1_COLS=8 so that eight columns at n = 1025 take them
    too, csrc/cg.hip `d1_cols`): the k = 5 iterate and error statistic of a column are the same bits whether it is
    solved alone or with the others -- one kernel family, column = blockIdx.y, the same additions in the same order.
    The joint solve against oracle/cg.py at the bars of test_fixed_steps_match_oracle (fp32: of test_fp32); every
    call twice with the same bits."""
    import switch_forms
    from cggp.conjugate_gradient import JacobiPreconditioner, conjugate_gradient
    k = 5
    A, rhs, oracle = company_system(n, dtype, cols)
    o_sol, o_err = oracle[jac]

    def solve(b):
        runs = []
        for _ in range(2):
            sol, (steps, err) = conjugate_gradient(A, b, None, 0.0, JacobiPreconditioner() if jac else None,
                                                   max_iterations=k, max_steps_cycle=k + 1)
            assert int(steps) == k
            runs.append((sol.clone(), err.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        return runs[0]

    with switch_forms.switched(monkeypatch, {"MGP_CG_DENSE1": "1", "MGP_CG_DENSE1_COLS": "8"}):
        V, err = solve(rhs)
        assert V.shape == (cols, n) and err.shape == (cols, 1)
        bar_v, bar_e = (1e-9, 1e-6) if dtype == "f64" else (5e-4, 5e-3)
        for c in range(cols):
            d_v = relerr(V[c], o_sol[c])
            d_e = abs(float(err[c]) - float(o_err[c, 0])) / float(o_err[c, 0])
            print(f"n={n} {dtype} jac={jac} column {c} of {cols}: iterate {d_v:.2e} (bar {bar_v:g}) err {d_e:.2e} (bar {bar_e:g})")
            assert d_v < bar_v and d_e < bar_e, (c, d_v, d_e)
        for c in range(cols):
            v1, e1 = solve(rhs[c:c + 1].contiguous())
            assert torch.equal(v1[0], V[c]) and torch.equal(e1[0], err[c]), c


@pytest.mark.parametrize("n,Bt", [(2049, 1), (2500, 4), (3000, 6), (3520, 2), (4001, 3), (4095, 5), (4096, 6), (4001, 7), (3000, 8)])
def test_super_block_form(n, Bt):
    """2048 < n <= 4096, 1..8 columns: the whole solve in one launch with the upper triangle on the chip in 3 x 3
    super-blocks of tiles (csrc/cg_dense1.hip, d1_persist_blk_kernel): whole and ragged sizes (n % 64, nt % 3 != 0),
    columns of very different size, fp64 and fp32, Jacobi with an initial solution -- k steps against the oracle --
    and a converged solve on the true residual."""
    from cggp.conjugate_gradient import JacobiPreconditioner, conjugate_gradient
    A, _ = problem(n, seed=3 * n + Bt)
    rng = np.random.default_rng(n + Bt)
    rhs = rng.standard_normal((Bt, n)) * (10.0 ** rng.integers(-2, 3, (Bt, 1)))
    for k in (1, 2, 9):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, max_iterations=k,
                                                         max_steps_cycle=k + 1)
        assert int(steps) == k == o_steps
        for b in range(Bt):
            assert relerr(sol[b], o_sol[b]) < 1e-9, (k, b)
            assert abs(float(err[b]) - float(o_err[b, 0])) / float(o_err[b, 0]) < 1e-8
    again, _ = conjugate_gradient(T(A), T(rhs), None, 0.0, max_iterations=9, max_steps_cycle=10, check_every=4)
    assert torch.equal(sol, again)
    v0 = 0.01 * rng.standard_normal((Bt, n))
    sj, (kj, ej) = conjugate_gradient(T(A), T(rhs), T(v0), 0.0, JacobiPreconditioner(), max_iterations=4, max_steps_cycle=5)
    o_sj, _ = ocg.conjugate_gradient(A, rhs, v0, 0.0, ocg.JacobiPreconditioner(), max_iterations=4, max_steps_cycle=5)
    assert relerr(sj, o_sj) < 1e-9
    s32, (k32, _) = conjugate_gradient(T(A, torch.float32), T(rhs, torch.float32), None, 0.0, max_iterations=3,
                                       max_steps_cycle=4)
    o32, _ = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, max_iterations=3, max_steps_cycle=4)
    assert int(k32) == 3 and relerr(s32, o32) < 5e-3
    thr = 1e-9
    s, (ks, es) = conjugate_gradient(T(A), T(rhs), None, thr, max_iterations=n, max_steps_cycle=n + 1, check_every=16)
    res = rhs - s.cpu().numpy() @ A
    assert int(ks) < n and np.all(0.5 * np.sum(res * res, axis=1) <= thr * (1 + 1e-6) + 1e-16)


def test_every_form_of_the_dense_cg_gives_the_oracle_steps():
    """The forms are chosen when the handle is made (MGP_CG_DENSE1 = 3: register-resident for n <= 4096 -- the full
    matrix for n <= 2048, super-blocks of the triangle above; 4: super-blocks wherever they fit; 1: two launches
    per iteration; MGP_CG_DENSE1_COLS = 1: several columns through the skinny product as in round 3): the stress
    script -- random n, steps, Jacobi, initial solutions, fp32, each case against the several-column kernels -- and a
    k-step comparison with the oracle, once per form, each in a process of its own."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, numpy as np, torch; sys.path[:0] = [%r, %r]\n"
        "from oracle import cg as ocg\n"
        "from cggp.conjugate_gradient import conjugate_gradient\n"
        "rng = np.random.default_rng(5)\n"
        "for n, Bt in ((1500, 1), (4096, 1), (2048, 3), (6000, 1), (1500, 8), (4096, 5)):\n"
        "    Q = rng.standard_normal((n, 16)); A = Q @ Q.T / 16 + np.diag(0.5 + rng.random(n)); b = rng.standard_normal((Bt, n))\n"
        "    s, (k, e) = conjugate_gradient(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), None, 0.0, max_iterations=6, max_steps_cycle=7)\n"
        "    o, _ = ocg.conjugate_gradient(A, b, np.zeros((Bt, n)), 0.0, max_iterations=6, max_steps_cycle=7)\n"
        "    assert int(k) == 6 and np.max(np.abs(s.cpu().numpy() - o)) / np.max(np.abs(o)) < 1e-9, (n, Bt)\n"
        "print('FORM_OK')\n" % (root, os.path.join(root, "conjugate-gradient-sparse-gp_amd")))
    for env in ({"MGP_CG_DENSE1": "1"}, {"MGP_CG_DENSE1": "3"}, {"MGP_CG_DENSE1": "4"}, {"MGP_CG_DENSE1_COLS": "1"},
                {"MGP_CG_DENSE1_COLS": "8"}, {"MGP_CG_DENSE1": "0"},
                {"MGP_CG_PIPELINE_POLLS": "0", "MGP_CG_DENSE1": "1"}):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0 and "FORM_OK" in out.stdout, (env, out.stderr[-1500:])
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_dense1.py"), "40", "7"],
                         env=dict(os.environ, MGP_CG_DENSE1_COLS="1"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "cases ok" in out.stdout, out.stderr[-1500:]
    # ... and 1..8 columns on the register-resident forms, random sizes, against the oracle
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_dense_cols.py"), "40", "3"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "cases ok" in out.stdout, out.stderr[-1500:]


@pytest.mark.parametrize("n,Bt,absent", [(4096, 1, 3), (3000, 5, 0), (2048, 1, 17), (1536, 4, 2)])
def test_a_missing_workgroup_makes_the_register_resident_solve_fail_over_not_hang(n, Bt, absent):
    """The register-resident forms need every workgroup on the chip at once.  MGP_D1_INJECT_ABSENT=<w> makes workgroup
    w leave at launch -- what a shared GPU would look like: every wait of the others is bounded, the launch ends with
    its error word set, libmgp says so on stderr and runs the solve again with two launches per iteration; the result
    is the oracle's.  (An owner, a workgroup without a chunk, both forms, one and several columns.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, time, numpy as np, torch; sys.path[:0] = [%r, %r]\n"
        "from oracle import cg as ocg\n"
        "from cggp.conjugate_gradient import conjugate_gradient\n"
        "n, Bt = %d, %d\n"
        "rng = np.random.default_rng(9)\n"
        "Q = rng.standard_normal((n, 16)); A = Q @ Q.T / 16 + np.diag(0.5 + rng.random(n)); b = rng.standard_normal((Bt, n))\n"
        "t0 = time.time()\n"
        "s, (k, e) = conjugate_gradient(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), None, 0.0, max_iterations=6, max_steps_cycle=7)\n"
        "torch.cuda.synchronize(); dt = time.time() - t0\n"
        "o, _ = ocg.conjugate_gradient(A, b, np.zeros((Bt, n)), 0.0, max_iterations=6, max_steps_cycle=7)\n"
        "assert int(k) == 6 and np.max(np.abs(s.cpu().numpy() - o)) / np.max(np.abs(o)) < 1e-9\n"
        "assert dt < 30.0, dt\n"
        "print('FAILOVER_OK %%.2f s' %% dt)\n" % (root, os.path.join(root, "conjugate-gradient-sparse-gp_amd"), n, Bt))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MGP_D1_INJECT_ABSENT=str(absent)),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILOVER_OK" in out.stdout, out.stderr[-1500:]
    assert "hand-off between resident workgroups timed out" in out.stderr, out.stderr[-1500:]


def test_register_resident_solve_beside_a_busy_stream():
    """The register-resident forms want a whole CU per workgroup.  With another stream keeping the chip busy (large
    fp64 GEMMs queued on it for ~0.5 s) the solve must still come back with the oracle's steps, by whichever road:
    its workgroups get their CUs late, or a bounded wait runs out and the solve fails over to two launches per
    iteration -- never a hang, never a wrong iterate."""
    import time
    from cggp.conjugate_gradient import conjugate_gradient
    n, Bt = 4096, 3
    A, _ = problem(n, seed=77)
    rng = np.random.default_rng(5)
    rhs = rng.standard_normal((Bt, n))
    o_sol, _ = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, max_iterations=6, max_steps_cycle=7)
    At, bt = T(A), T(rhs)
    big = torch.randn(6144, 6144, dtype=torch.float64, device=dev())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.cuda.stream(side):
        for _ in range(60):
            big2 = big @ big
    for _ in range(3):  # several solves while the side stream works
        sol, (steps, err) = conjugate_gradient(At, bt, None, 0.0, max_iterations=6, max_steps_cycle=7)
        assert int(steps) == 6 and relerr(sol, o_sol) < 1e-9
    torch.cuda.synchronize()
    assert time.time() - t0 < 60.0
    del big2


def test_fp32():
    from cggp.conjugate_gradient import conjugate_gradient
    n = 2048
    A, rhs = problem(n, seed=12, noise=1.0)
    A32, rhs32 = A.astype(np.float32), rhs.astype(np.float32)
    for k in (2, 6):
        sol, (steps, err) = conjugate_gradient(T(A32), T(rhs32.T), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A32.astype(np.float64), rhs32.T.astype(np.float64),
                                                         np.zeros((1, n)), 0.0, max_iterations=k, max_steps_cycle=k + 1)
        assert sol.dtype == torch.float32 and int(steps) == k == o_steps
        assert relerr(sol, o_sol) < 5e-4
        assert abs(float(err) - float(o_err[0, 0])) / float(o_err[0, 0]) < 5e-3


def test_cdgp_predict_mean_through_the_dense_path():
    """`CGGP.predict_f`'s `a = CG(Kmm + Lambda, pseudo_u)` (`models.py:339`) at M = 2048 is this path; the mean
    against the oracle's CGGP with the same inputs."""
    from cggp import kernels, synthetic
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP
    from oracle import cluster as oc
    N, D, M = 20000, 4, 2048
    syn = synthetic.make_inputs(N, D, M)
    idx = oc.nearest_centre_sqdist(syn.Z, syn.X)
    u, counts = oc.cluster_stats(idx, syn.y, M)
    kern = kernels.SquaredExponential(1.0, [1.0] * D)
    m = CGGP(kern, 0.1, T(syn.Z), ConjugateGradient(1e-14, max_iterations=4 * M), num_probes=None, pseudo_u=T(u),
             cluster_counts=T(counts))
    mu, var = m.predict_f(T(syn.X[:64]))
    ref = om.CGGP(ok.Kernel("se", 1.0, np.ones(D)), 0.1, syn.Z, ocg.ConjugateGradient(1e-14, max_iterations=4 * M),
                  num_probes=None, pseudo_u=u, cluster_counts=counts)
    mu0, var0 = ref.predict_f(syn.X[:64])
    assert relerr(mu, mu0) < 1e-6 and float(np.max(np.abs(var.cpu().numpy() - var0))) < 1e-6


@pytest.mark.parametrize("Bt", [1, 3])
def test_beyond_the_fused_sizes(Bt):
    """n > 8192: neither the two-launch path nor the register-resident fused update applies; the generic update
    kernel (1024 threads per right-hand side there) runs the same recurrence, with and without Jacobi."""
    from cggp.conjugate_gradient import JacobiPreconditioner, conjugate_gradient
    n = 9001
    rng = np.random.default_rng(31)
    Q = rng.standard_normal((n, 40))
    A = Q @ Q.T / 40 + np.diag(1.0 + rng.random(n))
    rhs = rng.standard_normal((Bt, n))
    for pre, o_pre in ((None, None), (JacobiPreconditioner(), ocg.JacobiPreconditioner())):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs), None, 0.0, pre, max_iterations=6, max_steps_cycle=7)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, o_pre, max_iterations=6,
                                                         max_steps_cycle=7)
        assert int(steps) == 6 == o_steps and relerr(sol, o_sol) < 1e-9
        assert np.max(np.abs(err.cpu().numpy() - o_err) / np.abs(o_err)) < 1e-6


@pytest.mark.parametrize("M,G,dtype", [(2048, 8, torch.float64), (1500, 3, torch.float64), (1024, 4, torch.float32)])
def test_rank_slabs_of_the_sgpr_operator_sum_to_the_whole(M, G, dtype):
    """Multi-GPU decomposition of S.p at sizes where a rank's slab of s2 Kmm.p runs the column-split
    slab kernel (M >= 1024): the partial operators of G ranks -- row shard of X, row slab of Kmm -- add up to the
    whole operator, which the oracle checks."""
    from cggp import kernels, parallel
    from cggp.conjugate_gradient import SgprNormalOperator
    N, D = 6000, 3
    rng = np.random.default_rng(M + G)
    X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    kern = kernels.Matern52(1.2, [0.9, 1.1, 1.3])
    Xt, Zt = T(X, dtype), T(Z, dtype)
    P = T(rng.standard_normal((1, M)), dtype)
    whole = SgprNormalOperator(kern, Xt, Zt, 0.1, jitter=1e-6).rmatmul(P)
    acc = torch.zeros_like(whole, dtype=torch.float64)

    class _OneRank:  # the exchange of a one-rank group: the partial is its own sum (slabs are honoured only with one)
        comm, world_size = None, 1

        def __call__(self, t):
            pass

    for g in range(G):
        lo, hi = parallel.shard_bounds(N, G, g)
        part = SgprNormalOperator(kern, Xt[lo:hi].contiguous(), Zt, 0.1, jitter=1e-6, allreduce=_OneRank(),
                                  kmm_rows=parallel.kmm_slab(M, G, g)).rmatmul(P)
        acc += part.double()
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert float((acc - whole.double()).abs().max() / whole.double().abs().max()) < tol
    if dtype == torch.float64:
        ko = ok.Kernel("matern52", 1.2, np.array([0.9, 1.1, 1.3]))
        ref = om.SgprNormalOperator(X, Z, ko, 0.1, jitter=1e-6).rmatmul(P.cpu().numpy())
        assert relerr(whole, ref) < 1e-11
