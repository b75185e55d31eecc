"""Every launch form the CG solve driver can choose (csrc/cg.hip: fused update tiers, deferred and reduced skinny
products, both block sizes and all six modes of the generic update kernel, the recording solve), on the cases of
tests/cg_route_plan.py: the k-step iterate and 0.5 rz against oracle/cg.py at the bars of
tests/test_gpu_parity.py::test_cg_fixed_iterations_match_oracle (1e-9 relative on the iterate, 1e-6 relative on
0.5 rz), each solve twice with the same bits.

fp32 has no fixed-step bar elsewhere: a case's bar is four times the distance of the oracle on float32 copies from its
own float64 run on that case (cg_route_plan.py).

No breakdown guard fires on these cases (every column is live at every step, asserted below).  The guards, columns of
different lifetimes in one batch and the stopping rule are held to the oracle on every one of these kernel sites by
tests/test_gpu_cg_guards.py, on the cases of tests/guard_plan.py."""

import functools

import numpy as np
import pytest
import torch

import cg_route_plan as rp
from oracle import cg as ocg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=2)  # the cases come sorted by n: 540 MB at the largest, built and uploaded once
def system(n):
    A = rp.matrix(n)
    return A, T(A)


def preconditioners(case, A):
    from cggp import conjugate_gradient as cg
    if case.pre == "jacobi":
        return cg.JacobiPreconditioner(), ocg.JacobiPreconditioner()
    if case.pre == "block":
        idx = rp.block_indices(case.n)
        return cg.BlockPreconditioner(idx), ocg.BlockPreconditioner(idx)
    if case.pre == "dense":
        P = rp.dense_pinv(case.n)
        return cg.DensePreconditioner(T(P)), ocg.DensePreconditioner(P)
    return cg.EyePreconditioner(), ocg.EyePreconditioner()


def oracle(case, A, np_dtype, pre):
    b, v0 = rp.rhs(case).astype(np_dtype), rp.start(case).astype(np_dtype)
    sol, (steps, err) = ocg.conjugate_gradient(np.asarray(A, dtype=np_dtype), b, v0, 0.0, pre, max_iterations=case.k,
                                               max_steps_cycle=case.max_steps_cycle)
    assert steps == case.k
    return sol.astype(np.float64), err.astype(np.float64)


def distance(sol, err, o_sol, o_err):
    return (float(np.max(np.abs(sol - o_sol)) / np.max(np.abs(o_sol))), float(np.max(np.abs(err - o_err) / o_err)))


def device_solve(case, At, pre):
    from cggp.conjugate_gradient import conjugate_gradient
    dt = torch.float64 if case.dtype == "f64" else torch.float32
    A = At if dt == torch.float64 else At.to(dt)
    v0 = None if case.start == "zero" else T(rp.start(case), dt)
    runs = []
    for _ in range(2):
        sol, (steps, err) = conjugate_gradient(A, T(rp.rhs(case), dt), v0, 0.0, pre, max_iterations=case.k,
                                               max_steps_cycle=case.max_steps_cycle)
        assert int(steps) == case.k
        runs.append((sol, err))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # same bits
    return runs[0][0].double().cpu().numpy(), runs[0][1].double().cpu().numpy()


@pytest.mark.parametrize("case", sorted((c for c in rp.CASES if not c.record), key=lambda c: (c.n, c.id)), ids=repr)
def test_cg_route_matches_oracle(case):
    A, At = system(case.n)
    pre, o_pre = preconditioners(case, A)
    o_sol, o_err = oracle(case, A, np.float64, o_pre)
    assert o_err.min() > 1e-16  # no breakdown guard fires
    if case.dtype == "f64":
        bar = (1e-9, 1e-6)
    else:
        own = distance(*oracle(case, A, np.float32, o_pre), o_sol, o_err)
        bar = (4 * own[0], 4 * own[1])
    got = distance(*device_solve(case, At, pre), o_sol, o_err)
    print(f"{case.id}: ks {case.slices} iterate {got[0]:.3e} (bar {bar[0]:.3e}) err {got[1]:.3e} (bar {bar[1]:.3e})")
    assert got[0] < bar[0] and got[1] < bar[1], (case.id, got, bar)


@pytest.mark.parametrize("case", [c for c in rp.CASES if c.record], ids=repr)
def test_recording_route_matches_plain_solve_and_oracle_steps(case):
    from cggp import ops
    from cggp.conjugate_gradient import DenseOperator
    A, At = system(case.n)
    b = rp.rhs(case)
    plain_sol, plain_err = device_solve(case, At, None)
    sol, err, st, coef = ops.pcg_solve_record(DenseOperator(At), T(b), 0.0, case.k)
    assert st.iterations == case.k and coef.shape == (case.k, case.Bt, 3)
    assert np.array_equal(sol.cpu().numpy(), plain_sol) and np.array_equal(err.cpu().numpy(), plain_err)
    o_sol, o_err = oracle(case, A, np.float64, None)
    got = distance(plain_sol, plain_err, o_sol, o_err)
    assert got[0] < 1e-9 and got[1] < 1e-6, got
    # (gamma, beta, 0.5 rz) of every step against a plain numpy CG, column by column
    c = coef.cpu().numpy()
    for col in range(case.Bt):
        r = b[col].copy()
        pdir = r.copy()
        rz = r @ r
        for k in range(case.k):
            Ap = A @ pdir
            g = rz / (pdir @ Ap)
            r -= g * Ap
            rzn = r @ r
            beta = rzn / rz
            pdir = r + beta * pdir
            ref = np.array([g, beta, 0.5 * rzn])
            assert np.all(np.abs(c[k, col] - ref) <= 1e-9 * np.abs(ref)), (col, k, c[k, col], ref)
            rz = rzn
