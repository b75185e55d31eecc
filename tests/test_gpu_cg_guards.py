"""CG's breakdown guards and the any-over-columns stopping rule at every kernel site that repeats them, on the cases
of tests/guard_plan.py (tests/test_guard_plan.py shows on the CPU that a wrong guard fails them), against oracle/cg.py.

Per column, never over the batch: max |v_b - o_b| / max |o_b| under the k-step bar (1e-9 in fp64, four times the oracle's
own float32 distance in fp32), a column the oracle leaves at exactly zero exactly zero; 0.5 rz to a relative 1e-6 where
the oracle's value is above the floor, finite and under the floor where it is not (rounding noise, not compared), the
oracle's 0.5 rz_0 to 1e-12 for the column frozen from step 0 and exactly 0.0 for the zero column.  A column that both
guards hold from step j on has the same bits at every step count >= j.  The stopping run takes exactly the oracle's
steps, with the same bits for check_every 1, 3 and 16.  Every solve runs twice with the same bits."""

import contextlib
import functools

import numpy as np
import pytest
import torch

import guard_plan as gp
import switch_forms
from oracle import cg as ocg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def by_system(cases):
    return sorted(cases, key=lambda c: (c.n, c.system, c.pre == "jacobi", c.id))


@functools.lru_cache(maxsize=1)  # the cases come sorted by system: built and uploaded once (540 MB at n = 8193)
def _system(n, system, jacobi):
    A = gp.operator_matrix(next(c for c in gp.CASES if (c.n, c.system, c.pre == "jacobi") == (n, system, jacobi)))
    return A, T(A)


def system(case):
    return _system(case.n, case.system, case.pre == "jacobi")


def handle(case, monkeypatch):
    return switch_forms.switched(monkeypatch, case.env) if case.env else contextlib.nullcontext()


def torch_dtype(case):
    return torch.float64 if case.dtype == "f64" else torch.float32


def device_preconditioner(case):
    from cggp import conjugate_gradient as cg
    dt = torch_dtype(case)
    if case.pre == "jacobi":
        return cg.JacobiPreconditioner(T(gp.jacobi_diagonal(case.n), dt))
    if case.pre == "block":
        from cg_route_plan import block_indices
        return cg.BlockPreconditioner(block_indices(case.n))
    if case.pre == "dense":
        return cg.DensePreconditioner(T(gp.dense_pinv(case.n), dt))
    return cg.EyePreconditioner()


def oracle(case, A, k):
    """oracle/cg.py on the case in float64 (also for the fp32 cases: their bar is the distance of its float32 run from
    this one): k fixed steps, or the stopping run."""
    b, v0 = gp.rhs(case), gp.start(case)
    cap = k if k is not None else case.cap
    sol, (steps, err) = ocg.conjugate_gradient(
        A, b, v0, 0.0 if k is not None else case.thr, gp.host_preconditioner(case, A), max_iterations=cap,
        max_steps_cycle=case.cycle if case.cycle is not None else cap + 1,
        min_float=case.min_float if case.dtype == "f64" else float(np.float32(case.min_float)))
    return sol, steps, err


def twice(solve):
    """The solve run twice: the same bits; (solution [Bt, n], err [Bt, 1], steps) of the first."""
    runs = [solve() for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    return runs[0]


def fixed_steps(case, op, pre, k):
    from cggp.conjugate_gradient import conjugate_gradient
    dt = torch_dtype(case)
    v0 = T(gp.start(case), dt) if case.start == "v0" else None

    def solve():
        sol, (steps, err) = conjugate_gradient(op, T(gp.rhs(case), dt), v0, 0.0, pre, max_iterations=k,
                                               max_steps_cycle=case.cycle if case.cycle is not None else k + 1,
                                               min_float=case.min_float)
        return sol.clone(), err.clone(), int(steps)

    return twice(solve)


def stopping_run(case, op, pre, check_every):
    from cggp.conjugate_gradient import ConjugateGradient
    cg = ConjugateGradient(case.thr, pre, max_iterations=case.cap, min_float=case.min_float, check_every=check_every)

    def solve():
        sol, (steps, err) = cg.solve_with_stats(op, T(gp.rhs(case).T, torch_dtype(case)))
        return sol.t().contiguous(), err.clone(), int(steps)

    return twice(solve)


def hold_to_oracle(case, label, sol, err, o_sol, o_err):
    """The per-column assertions of the module docstring; prints every distance next to its bar."""
    assert bool(torch.isfinite(sol).all()) and bool(torch.isfinite(err).all()), (case.id, label)
    v, e = sol.double().cpu().numpy(), err.double().cpu().numpy()
    dv, de = gp.column_distances(v, e, o_sol, o_err)
    floor = case.min_float if case.dtype == "f64" else float(np.float32(case.min_float))
    bar_v, bar_e = case.bar
    failures = []
    for j, name in enumerate(case.cols):
        oe, ge = float(o_err[j, 0]), float(e[j, 0])
        if not np.any(o_sol[j]):
            how_v, ok_v = "exactly zero", not np.any(v[j])
        else:
            how_v, ok_v = f"{dv[j]:.2e} (bar {bar_v:.1e})", dv[j] < bar_v
        if oe == 0.0:
            how_e, ok_e = f"{ge:.3e}, exactly 0", ge == 0.0
        elif name == "c" and not np.any(o_sol[j]):  # frozen from step 0: 0.5 rz_0
            bar_c = 1e-12 if case.dtype == "f64" else bar_e
            how_e, ok_e = f"{de[j]:.2e} of 0.5 rz_0 (bar {bar_c:.1e})", de[j] < bar_c and ge <= floor
        elif oe > floor:
            how_e, ok_e = f"{de[j]:.2e} (bar {bar_e:.1e})", de[j] < bar_e
        else:
            how_e, ok_e = f"{ge:.3e} under the floor {floor:.1e} (oracle {oe:.3e})", ge <= floor
        print(f"{case.id} {label} column {name}: iterate {how_v}, err {how_e}")
        if not (ok_v and ok_e):
            failures.append((name, how_v, how_e))
    assert not failures, (case.id, label, failures)


def frozen_columns_keep_their_bits(case, A, runs):
    """runs: {k: (sol, err, steps)}.  A column under both guards from step j on: the same bits at every k >= j."""
    for j, reg in enumerate(gp.regimes(case, A)):
        if reg["frozen_from"] is None or case.dtype != "f64":
            continue
        ks = [k for k in sorted(runs) if k >= reg["frozen_from"]]
        for k in ks[1:]:
            assert torch.equal(runs[ks[0]][0][j], runs[k][0][j]) and torch.equal(runs[ks[0]][1][j], runs[k][1][j]), \
                (case.id, case.cols[j], ks[0], k)
        if len(ks) > 1:
            print(f"{case.id} column {case.cols[j]}: frozen from step {reg['frozen_from']}, the same bits at k = {ks}")


def whole_case(case, A, op, pre):
    runs = {}
    for k in case.ks:
        sol, err, steps = runs[k] = fixed_steps(case, op, pre, k)
        o_sol, o_steps, o_err = oracle(case, A, k)
        assert steps == k == o_steps
        hold_to_oracle(case, f"k={k}", sol, err, o_sol, o_err)
    frozen_columns_keep_their_bits(case, A, runs)
    if case.thr:
        o_sol, o_steps, o_err = oracle(case, A, None)
        first = None
        for check_every in (1, 3, 16):
            sol, err, steps = stopping_run(case, op, pre, check_every)
            print(f"{case.id} thr={case.thr:g} check_every={check_every}: {steps} steps (oracle {o_steps})")
            assert steps == o_steps, (case.id, check_every, steps, o_steps)
            if first is None:
                first = (sol, err)
                hold_to_oracle(case, f"thr={case.thr:g}", sol, err, o_sol, o_err)
            assert torch.equal(sol, first[0]) and torch.equal(err, first[1]), (case.id, check_every)


DENSE = [c for c in gp.CASES if c.family not in ("record", "matfree")]


@pytest.mark.parametrize("case", by_system(DENSE), ids=repr)
def test_guards_match_oracle_column_by_column(case, monkeypatch):
    A, At = system(case)
    with handle(case, monkeypatch):
        whole_case(case, A, At if case.dtype == "f64" else At.float(), device_preconditioner(case))


@pytest.mark.parametrize("case", by_system(c for c in gp.CASES if c.family == "record"), ids=repr)
def test_recorded_coefficients_under_the_guards(case):
    """mgp_pcg_solve_record: (gamma, beta, 0.5 rz) of every step.  A column under both guards: gamma and beta exactly 0
    and the third entry its 0.5 rz (for the columns frozen from step 0: 0.5 rz_0); gamma zeroed alone: exactly 0 beside
    the host recurrence's beta; beta dropped alone: exactly 0 beside its gamma; live: both to 1e-9."""
    from cggp import ops
    from cggp.conjugate_gradient import DenseOperator
    A, At = system(case)
    k = max(case.ks)
    sol, err, st, coef = ops.pcg_solve_record(DenseOperator(At), T(gp.rhs(case)), 0.0, k, min_float=case.min_float)
    assert st.iterations == k and coef.shape == (k, case.Bt, 3) and bool(torch.isfinite(coef).all())
    plain = fixed_steps(case, At, None, k)
    assert torch.equal(sol, plain[0]) and torch.equal(err, plain[1])
    o_sol, o_steps, o_err = oracle(case, A, k)
    hold_to_oracle(case, f"record k={k}", sol, err, o_sol, o_err)
    ref = gp.run(case, k, A=A)[4]
    c = coef.cpu().numpy()
    for j, (name, reg) in enumerate(zip(case.cols, gp.regimes(case, A))):
        worst = 0.0
        for i in range(k):
            g, b, h = c[i, j]
            rg, rb, rh = ref[i, j]
            close = lambda x, y: abs(x - y) <= 1e-9 * abs(y)
            if reg["frozen_from"] is not None and i >= reg["frozen_from"]:
                assert g == 0.0 and b == 0.0, (case.id, name, i, g, b)
                if reg["frozen_from"] == 0:
                    assert h == 0.0 if rh == 0.0 else abs(h - rh) <= 1e-12 * rh, (case.id, name, i, h, rh)
                else:
                    assert np.isfinite(h) and h <= case.min_float, (case.id, name, i, h)
            elif i in reg["gamma_only"]:
                assert g == 0.0 and close(b, rb) and close(h, rh), (case.id, name, i, c[i, j], ref[i, j])
            elif i in reg["beta_only"]:
                assert b == 0.0 and close(g, rg) and close(h, rh), (case.id, name, i, c[i, j], ref[i, j])
            else:
                # the step on which a column converges leaves rounding noise as rz: only gamma is compared there
                last = rh <= case.min_float
                assert close(g, rg) and (last or (close(b, rb) and close(h, rh))), (case.id, name, i, c[i, j], ref[i, j])
                worst = max(worst, abs(g - rg) / abs(rg))
        print(f"{case.id} column {name}: {reg}, largest distance of a live gamma {worst:.2e} (bar 1e-09)")


@pytest.mark.parametrize("case", [c for c in gp.CASES if c.family == "matfree"], ids=repr)
def test_guards_on_matrix_free_operators(case):
    """KxxNoise, KxxNoise under MGP_PRE_LOWRANK (a rank-8 factor made on the host; reference: pivchol_reference.pcg,
    column by column) and Kmm + Lambda: columns c (frozen from step 0), a (live), b (zeros)."""
    from cggp import kernels
    from cggp.conjugate_gradient import (EyePreconditioner, KmmLambdaOperator, KxxNoiseOperator,
                                         PivotedCholeskyPreconditioner)
    A = gp.operator_matrix(case)
    kern = kernels.SquaredExponential(1.0, [1.0, 1.0, 1.0])
    X = T(gp.points(case.n))
    op = KxxNoiseOperator(kern, X, gp.NOISE) if case.system == "kxx" else KmmLambdaOperator(kern, X, T(gp.lam(case.n)))
    if case.pre != "lowrank":
        whole_case(case, A, op, EyePreconditioner())
        return
    import pivchol_reference as pr
    L, dinv, B = gp.lowrank_factor(case, A)
    pre = PivotedCholeskyPreconditioner(rank=L.shape[0]).set_factor(T(L), gp.NOISE)
    b = gp.rhs(case)
    runs = {}
    for k in case.ks:
        sol, err, steps = runs[k] = fixed_steps(case, op, pre, k)
        assert steps == k
        o_sol, o_err = np.zeros_like(b), np.zeros((case.Bt, 1))
        for j in range(case.Bt):
            x, st, coef = pr.pcg(lambda v: A @ v, b[j], dinv=dinv, B=B, threshold=0.0, max_iterations=k,
                                 min_float=case.min_float)
            assert st == (k if np.any(b[j]) else 0)
            o_sol[j], o_err[j, 0] = x, coef[-1, 2] if st else 0.0
        hold_to_oracle(case, f"k={k} (pivchol_reference.pcg)", sol, err, o_sol, o_err)
    frozen_columns_keep_their_bits(case, A, runs)
