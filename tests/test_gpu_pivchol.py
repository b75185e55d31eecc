"""The pivoted-Cholesky preconditioner on the MI355X: the matrix-free factor `mgp_kxx_pivchol` against a long-double
factor with the device's pivot order forced, `mgp_lowrank_apply` against numpy, `MGP_PRE_LOWRANK` inside the device CG
(fixed-step iterates, the recorded coefficients, the refresh path, iteration counts) against the numpy PCG of
pivchol_reference.py, and `GPR` / `TrainableGPR` with `PivotedCholeskyPreconditioner` against the Cholesky model."""

import ctypes
import math

import numpy as np
import pytest
import torch

from pivchol_reference import (LD, forced_pivoted_cholesky, greedy_pivoted_cholesky, kernel_matrix, kernel_rows, pcg,
                               table_inputs)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MGP_E_BADARG, MGP_E_SHAPE, MGP_E_DTYPE, MGP_E_NOMEM = -1, -2, -3, -6  # include/mgp.h
KINDS = ["se", "matern12", "matern32", "matern52"]
# Ranks per input dimension: the greedy check is relative (1e-10 of the residual maximum), and the device's residual
# diagonal carries the rounding of up to 200 fp64 updates, <= 200 * 2.2e-16 * variance = 5e-14 variance, so it is
# meaningful while the reference maximum stays above ~1e-3 variance.  On these inputs (U(-3, 3)^D, lengthscales
# linspace(0.8, 1.6) sqrt(D), N >= 1000) the float64 reference keeps that for D = 1 up to rank 12 (SE: 3e-3) and for
# D = 3 up to rank 100 (SE: 7e-3); D = 8 and 40 keep it at 200.
RANKS = {1: 12, 3: 100, 8: 200, 40: 200}
DUP = 40


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _factor_inputs(D, N, seed=None):
    rng = np.random.default_rng(D if seed is None else seed)
    X = rng.uniform(-3.0, 3.0, (N, D))
    X[-DUP:] = X[:DUP]  # duplicated rows
    return X, np.linspace(0.8, 1.6, D) * np.sqrt(D)


@pytest.mark.parametrize("N", [1000, 5000])
@pytest.mark.parametrize("D", [1, 3, 8, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_factor_against_long_double_with_forced_pivots(kind, D, N):
    from cggp import ops
    var = 1.3
    X, ls = _factor_inputs(D, N)
    spec = ops.KernelSpec(kind, var, list(ls), D)
    L, piv, diag = ops.kxx_pivchol(spec, T(X), RANKS[D])
    k = RANKS[D]
    assert L.shape == (k, N) and piv.shape == (k,) and diag.shape == (N,)
    piv = piv.cpu().numpy()
    assert len(set(piv.tolist())) == k and piv.min() >= 0 and piv.max() < N  # distinct pivots
    assert piv[0] == 0  # step 0 is an N-way tie (d = variance everywhere): the lowest index
    rows = kernel_rows(kind, var, ls, X, piv)
    Lr, before, dr = forced_pivoted_cholesky(lambda p: rows[list(piv).index(p)], np.full(N, LD(var)), list(piv))
    Ld = L.cpu().numpy()
    err = float(np.max(np.abs(Ld.astype(LD) - Lr)))
    print(f"{kind} D={D} N={N}: max |L - L_ref| = {err:.3e}, min pivot residual = {float(before[-1].max()):.3e}")
    assert err <= 1e-10 * math.sqrt(var)
    # greedy: the chosen pivot's reference residual is the reference maximum (up to near-ties)
    for i, p in enumerate(piv):
        assert before[i][p] >= (1 - 1e-10) * before[i].max(), (i, p, float(before[i][p]), float(before[i].max()))
    # the residual diagonal; the reference's variance - sum_i L[i]^2
    ref_diag = LD(var) - (Lr * Lr).sum(axis=0)
    assert np.max(np.abs(diag.cpu().numpy().astype(LD) - ref_diag)) <= 1e-10
    assert float(diag.min()) >= 0.0 and np.all(diag.cpu().numpy()[piv] == 0.0)
    for i in range(k):  # exact zeros at the earlier pivots, sqrt(d_p) on the pivot
        assert np.all(Ld[i, piv[:i]] == 0.0) and Ld[i, piv[i]] > 0.0
    # duplicated rows: the copy of a pivot has residual 0 and is never chosen (positive residuals exist throughout)
    chosen = set(piv.tolist())
    dd = diag.cpu().numpy()
    for a in range(DUP):
        b = N - DUP + a
        assert not (a in chosen and b in chosen)
        assert b not in chosen  # equal rows have equal residuals, bit for bit, until one is taken: the lower index first
        if a in chosen or b in chosen:
            assert dd[a] <= 1e-10 and dd[b] <= 1e-10


def test_rel_tol_stop_matches_the_reference_and_two_calls_are_bit_identical():
    from cggp import ops
    N, var = 5000, 1.3
    X, ls = _factor_inputs(1, N)
    spec = ops.KernelSpec("se", var, list(ls), 1)
    K = kernel_matrix("se", var, ls, X, dtype=np.float64)
    for rel_tol in (1e-2, 1e-4):
        Lr, pr = greedy_pivoted_cholesky(K, 64, rel_tol)
        L, piv, diag = ops.kxx_pivchol(spec, T(X), 64, rel_tol)
        assert 0 < len(pr) < 64 and L.shape[0] == len(pr), (rel_tol, L.shape, len(pr))
        assert float(diag.sum()) <= rel_tol * N * var
    # determinism: same bits for L, piv and diag, on a larger case whose every step has many workgroups
    X8, ls8 = _factor_inputs(8, 70001, seed=3)
    spec8 = ops.KernelSpec("matern32", 0.7, list(ls8), 8)
    a = ops.kxx_pivchol(spec8, T(X8), 96)
    b = ops.kxx_pivchol(spec8, T(X8), 96)
    assert a[0].shape == (96, 70001)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(a[1][0]) == 0  # the N-way tie of step 0 across many workgroups: the lowest index
    # max_rank > N is clamped; N = 0 gives rank 0
    Ls, ps, _ = ops.kxx_pivchol(ops.KernelSpec("matern12", 1.0, [1.0, 1.0], 2), T(np.random.default_rng(0).random((5, 2))), 9)
    assert Ls.shape == (5, 5) and sorted(ps.tolist()) == [0, 1, 2, 3, 4]
    L0, p0, d0 = ops.kxx_pivchol(ops.KernelSpec("se", 1.0, [1.0, 1.0], 2), torch.zeros((0, 2), dtype=torch.float64, device=DEV), 4)
    assert L0.shape == (0, 0) and p0.shape == (0,) and d0.shape == (0,)


def test_bad_arguments_fixed_pool_and_workspace_bound():
    from cggp import _hip
    lib = _hip.load_library()
    hd = _hip.get_handle(DEV)
    N, k = 20000, 16
    X = T(np.random.default_rng(0).uniform(-1, 1, (N, 2)))
    L = torch.empty((k, N), dtype=torch.float64, device=DEV)
    piv = torch.empty((k,), dtype=torch.int64, device=DEV)
    rank = ctypes.c_int32(0)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    k64 = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    k32 = _hip.make_kernel_struct("se", _hip.F32, 2, 1.0, [1.0, 1.0])
    call = lambda h, kk, x, n, mr, tol, l, pv, rk: lib.mgp_kxx_pivchol(h, ctypes.byref(kk), x, n, mr, tol, l, pv, None, rk)
    assert call(hd.h, k32, p(X), N, k, 0.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_DTYPE
    assert call(hd.h, k64, p(X), N, 0, 0.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), N, 1025, 0.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), N, k, -1.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), -1, k, 0.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_SHAPE
    assert call(hd.h, k64, None, N, k, 0.0, p(L), p(piv), ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), N, k, 0.0, None, p(piv), ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), N, k, 0.0, p(L), None, ctypes.byref(rank)) == MGP_E_BADARG
    assert call(hd.h, k64, p(X), N, k, 0.0, p(L), p(piv), None) == MGP_E_BADARG
    one = torch.ones((N,), dtype=torch.float64, device=DEV)
    assert lib.mgp_lowrank_apply(hd.h, 7, p(one), p(L), k, N, p(one), 1, p(one)) == MGP_E_DTYPE
    assert lib.mgp_lowrank_apply(hd.h, _hip.F64, p(one), p(L), 0, N, p(one), 1, p(L)) == MGP_E_SHAPE
    assert lib.mgp_lowrank_apply(hd.h, _hip.F64, None, p(L), k, N, p(one), 1, p(L)) == MGP_E_BADARG
    assert lib.mgp_lowrank_apply(hd.h, _hip.F64, p(one), p(L), k, N, p(one), 1, p(one)) == MGP_E_BADARG  # in place
    # a fresh growing handle: the factor's scratch is within the stated bound (8 N + 32 KiB, an arena grows by a quarter)
    idx = DEV.index or 0
    fresh = _hip.Handle(idx)
    fresh.sync_stream()
    w0 = lib.mgp_workspace_bytes(fresh.h)
    assert call(fresh.h, k64, p(X), N, k, 0.0, p(L), p(piv), ctypes.byref(rank)) == 0 and rank.value == k
    used = lib.mgp_workspace_bytes(fresh.h) - w0
    bound = 8 * N + (32 << 10)
    assert 0 < used <= bound + bound // 4 + 4096 + 256, (used, bound)
    # a fixed pool that is too small: MGP_E_NOMEM, and one that fits works
    for pool, want in ((64 << 10, MGP_E_NOMEM), (16 << 20, 0)):
        h = ctypes.c_void_p()
        assert lib.mgp_create_ex(ctypes.byref(h), idx, pool) == 0
        try:
            lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream))
            assert call(h, k64, p(X), N, k, 0.0, p(L), p(piv), ctypes.byref(rank)) == want
            if want == 0:
                assert lib.mgp_workspace_bytes(h) <= 16 << 20
        finally:
            lib.mgp_destroy(h)


@pytest.mark.parametrize("n", [1000, 70000])
@pytest.mark.parametrize("k", [1, 33, 128])
@pytest.mark.parametrize("Bt", [1, 5, 16, 40])
def test_lowrank_apply_against_numpy(Bt, k, n):
    from cggp import ops
    rng = np.random.default_rng(Bt * 1000 + k + n)
    B = rng.standard_normal((k, n)) / math.sqrt(n)
    dinv = 0.5 + rng.random(n)
    R = rng.standard_normal((Bt, n))
    ref = dinv[None, :] * R - (R @ B.T) @ B
    scale = np.abs(dinv[None, :] * R) + (np.abs(R) @ np.abs(B).T) @ np.abs(B)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        args = [T(a).to(dtype) for a in (dinv, B, R)]
        z1 = ops.lowrank_apply(*args)
        z2 = ops.lowrank_apply(*args)
        assert torch.equal(z1, z2)
        err = float(np.max(np.abs(z1.cpu().numpy().astype(np.float64) - ref) / scale))
        print(f"Bt={Bt} k={k} n={n} {dtype}: {err:.3e}")
        assert err <= tol


def _kxx(N, D, s2, ls, seed=0, name="se"):
    from cggp import kernels
    from cggp.conjugate_gradient import KxxNoiseOperator
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    kern = cls(1.0, list(np.broadcast_to(np.asarray(ls, dtype=np.float64), (D,))))
    X = T(np.random.default_rng(seed).uniform(-1.5, 1.5, (N, D)))
    return KxxNoiseOperator(kern, X, s2), kern, X


def _dense(op):
    from cggp import ops
    return ops.k_dense(op.spec, op.X, op.X, jitter=op.noise_variance).cpu().numpy()


def test_fixed_step_iterates_and_recorded_coefficients_against_numpy_pcg():
    from cggp import ops
    from cggp.conjugate_gradient import PivotedCholeskyPreconditioner, _solve_device
    # well conditioned, as the recording test of the identity path: two correct CGs then agree to ~1e-13 per step
    N = 2000
    op, kern, X = _kxx(N, 3, 1.0, 0.3, seed=1)
    pre = PivotedCholeskyPreconditioner(rank=24, rel_tol=0.0)
    rhs = T(np.random.default_rng(2).standard_normal((3, N)))
    sol, st, err = _solve_device(op, rhs, None, 0.0, pre, 5, 6, 1e-16, 10)
    assert st.iterations == 5 and pre.rank_ == 24
    A = _dense(op)
    dinv, B = pre.diag_inv.cpu().numpy(), pre.B.cpu().numpy()
    sol_r, err_r, st_r, coef = ops.pcg_solve_record(op, rhs, 0.0, 5, preconditioner=pre)
    assert torch.equal(sol_r, sol) and torch.equal(err_r, err) and coef.shape == (5, 3, 3)
    c = coef.cpu().numpy()
    for col in range(3):
        x, it, cr = pcg(lambda v: A @ v, rhs[col].cpu().numpy(), dinv=dinv, B=B, threshold=0.0, max_iterations=5)
        assert it == 5
        e = np.max(np.abs(sol[col].cpu().numpy() - x)) / np.max(np.abs(x))
        print(f"column {col}: iterate {e:.3e}, coefficients {np.max(np.abs(c[:, col] - cr) / np.abs(cr)):.3e}")
        assert e <= 1e-9
        assert np.all(np.abs(c[:, col] - cr) <= 1e-9 * np.abs(cr)), (c[:, col], cr)
        assert abs(float(err[col, 0]) - cr[-1, 2]) <= 1e-9 * cr[-1, 2]
    # a longer recorded solve: the record is the run of the plain preconditioned solve
    s1, st1, e1 = _solve_device(op, rhs, None, 1e-12, pre, 200, 201, 1e-16, 10)
    s2_, e2, st2, coef2 = ops.pcg_solve_record(op, rhs, 1e-12, 200, preconditioner=pre)
    assert st1.iterations == st2.iterations == coef2.shape[0] and torch.equal(s1, s2_) and st2.converged


def test_refresh_path_reaches_the_numpy_solution():
    from cggp.conjugate_gradient import PivotedCholeskyPreconditioner, _solve_device
    N = 3000
    op, kern, X = _kxx(N, 2, 0.1, 1.0, seed=4)
    pre = PivotedCholeskyPreconditioner(rank=16, rel_tol=0.0)  # a low rank: tens of steps are left
    rhs = T(np.random.default_rng(5).standard_normal((2, N)))
    sol, st, _ = _solve_device(op, rhs, None, 1e-14, pre, 400, 7, 1e-16, 10)  # refresh every 7th step
    assert st.converged and st.iterations > 14
    A = _dense(op)
    dinv, B = pre.diag_inv.cpu().numpy(), pre.B.cpu().numpy()
    for col in range(2):
        b = rhs[col].cpu().numpy()
        x, it, _ = pcg(lambda v: A @ v, b, dinv=dinv, B=B, threshold=1e-14, max_iterations=400, max_steps_cycle=7)
        e = np.max(np.abs(sol[col].cpu().numpy() - x)) / np.max(np.abs(x))
        print(f"column {col}: device {st.iterations} steps, numpy {it}, difference {e:.3e}")
        assert e <= 1e-8


@pytest.mark.parametrize("D,ls,rank,cap", [(2, 1.5, 64, 5), (8, 3.0, 256, 2)])
def test_iteration_counts_on_the_table_inputs(D, ls, rank, cap):
    from cggp import kernels
    from cggp.conjugate_gradient import (EyePreconditioner, KxxNoiseOperator, PivotedCholeskyPreconditioner,
                                         _solve_device)
    N, s2, thr = 8192, 0.1, 1e-8
    Xn, yn = table_inputs(N, D)
    X, y = T(Xn), T(yn[None, :])
    op = KxxNoiseOperator(kernels.SquaredExponential(1.0, [ls] * D), X, s2)
    pre = PivotedCholeskyPreconditioner(rank=rank, rel_tol=0.0)
    x_id, st_id, _ = _solve_device(op, y, None, thr, EyePreconditioner(), N, N + 1, 1e-16, 10)
    x_pc, st_pc, _ = _solve_device(op, y, None, thr, pre, N, N + 1, 1e-16, 10)
    A = _dense(op)
    _, it_np, _ = pcg(lambda v: A @ v, yn, dinv=pre.diag_inv.cpu().numpy(), B=pre.B.cpu().numpy(), threshold=thr)
    res = lambda x: float(np.linalg.norm(A @ x[0].cpu().numpy() - yn))
    print(f"D={D} ls={ls} rank={pre.rank_}: identity {st_id.iterations} steps (|r| {res(x_id):.3e}), "
          f"preconditioned {st_pc.iterations} (|r| {res(x_pc):.3e}), numpy PCG {it_np}")
    assert st_id.converged and st_pc.converged
    assert abs(st_pc.iterations - it_np) <= 2
    assert st_pc.iterations * cap <= st_id.iterations
    assert res(x_pc) <= 10 * res(x_id)


def test_gpr_with_the_preconditioner_against_the_cholesky_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient, PivotedCholeskyPreconditioner
    N, D, s2 = 3000, 2, 0.1
    rng = np.random.default_rng(2)
    Xn = rng.uniform(-3, 3, (N, D))
    Yn = np.sin(Xn.sum(axis=1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    Xs = T(rng.uniform(-3, 3, (200, D)))
    kern = kernels.SquaredExponential(1.0, [0.9, 1.2])
    data = (T(Xn), T(Yn))
    chol = models.GPR(data, kern, noise_variance=s2, solver="cholesky")
    pre = PivotedCholeskyPreconditioner(rank=128)
    cg = models.GPR(data, kern, noise_variance=s2, solver="cg",
                    conjugate_gradient=ConjugateGradient(1e-12, preconditioner=pre, max_iterations=4000))
    m0, v0 = chol.predict_f(Xs)
    m1, v1 = cg.predict_f(Xs)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print(f"mean {rel(m1, m0):.3e} variance {rel(v1, v0):.3e} rank {pre.rank_}")
    assert rel(m1, m0) < 1e-6 and rel(v1, v0) < 1e-6  # the tolerance of test_gpr_cg_against_cholesky
    # the factor follows the kernel parameters and the noise
    L_a = pre.L
    kern.lengthscales = [0.5, 0.6]
    cg.predict_f(Xs[:4])
    assert pre.L is not L_a
    L_b = pre.L
    cg.predict_f(Xs[:4])
    assert pre.L is L_b
    cg.likelihood.variance = 0.3
    cg.predict_f(Xs[:4])
    assert pre.L is not L_b and float(pre.D[0]) == 0.3


def _lml_inputs(N, D, seed, name="se", ls=(0.5, 1.0)):
    """The inputs of tests/test_gpu_gpr_lml.py (`_kxx_op`): X ~ U(-1.5, 1.5), lengthscales linspace(ls)."""
    from cggp import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    kern = cls(1.0, list(np.linspace(ls[0], ls[1], D)))
    X = T(np.random.default_rng(seed).uniform(-1.5, 1.5, (N, D)))
    return kern, X


def test_lml_estimate_with_sampled_probes_against_slogdet():
    from cggp import models, ops
    from cggp.conjugate_gradient import ConjugateGradient, PivotedCholeskyPreconditioner
    N = 4096
    kern, X = _lml_inputs(N, 3, 7)
    Y = torch.sin(X.sum(dim=1, keepdim=True))
    pre = PivotedCholeskyPreconditioner(rank=128)
    mp = models.GPR((X, Y), kern, noise_variance=0.1, conjugate_gradient=ConjugateGradient(1e-14, preconditioner=pre))
    mi = models.GPR((X, Y), kern, noise_variance=0.1, conjugate_gradient=ConjugateGradient(1e-14))
    Khat = ops.k_dense(kern.spec(3), X, X, jitter=0.1)
    sld = float(torch.linalg.slogdet(Khat)[1])
    ep = mp.log_marginal_likelihood_estimate(num_probes=64, seed=1)
    ei = mi.log_marginal_likelihood_estimate(num_probes=64, seed=1)
    msg = (f"preconditioned: log_det {ep.log_det:.6f} std_error {ep.std_error:.4f} steps {ep.iterations}; identity: "
           f"log_det {ei.log_det:.6f} std_error {ei.std_error:.4f} steps {ei.iterations}; slogdet {sld:.6f}")
    print(msg)
    assert ep.converged and abs(ep.log_det - sld) <= 4 * ep.std_error, msg
    exact = mi.log_marginal_likelihood()
    assert abs((ep.value + 0.5 * ep.log_det) - (exact + 0.5 * sld)) <= 1e-8 * abs(exact), msg
    assert mp.log_marginal_likelihood_estimate(num_probes=64, seed=1) == ep  # the same seed, the same estimate


@pytest.mark.parametrize("name", ["se", "matern32"])
def test_exact_probes_give_the_cholesky_value_and_gradient(name):
    from cggp import kernels, ops, training
    from cggp.conjugate_gradient import ConjugateGradient, KxxNoiseOperator, PivotedCholeskyPreconditioner
    N = 512
    _, X = _lml_inputs(N, 3, 11, name=name)
    Y = torch.cos(2 * X[:, :1]) + 0.1 * T(np.random.default_rng(0).standard_normal((N, 1)))
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    k0 = cls(1.3, [0.6, 0.8, 1.1])
    pre = PivotedCholeskyPreconditioner(rank=40, rel_tol=0.0)
    chol = training.TrainableGPR(k0, 0.15, X, Y)
    est = training.TrainableGPR(k0, 0.15, X, Y, num_probes=N, conjugate_gradient=ConjugateGradient(1e-20, preconditioner=pre))
    # the exact probe set Z = sqrt(N) P^(1/2): Z Z^T / N = P
    pre._prepare(KxxNoiseOperator(est.kernel.frozen(), X, est.likelihood_variance.value))
    assert pre.rank_ == 40
    P = pre.L.t() @ pre.L + torch.diag(pre.D)
    lam, Q = torch.linalg.eigh(P)
    est.probes = math.sqrt(N) * (Q * torch.sqrt(lam)) @ Q.t()
    l0 = chol.log_marginal_likelihood()
    l1 = est.log_marginal_likelihood()
    frozen = est.frozen_model()
    parts = frozen.log_marginal_likelihood_estimate(probes=est.probes)
    Khat = ops.k_dense(frozen._spec(), X, X, jitter=frozen.likelihood.variance)
    sld = float(torch.linalg.slogdet(Khat)[1])
    print(f"{name}: log_det {parts.log_det:.10f} slogdet {sld:.10f} value {l1.item():.10f} cholesky {l0.item():.10f} "
          f"steps {parts.iterations}")
    assert abs(parts.log_det - sld) <= 1e-8 * abs(sld)
    assert abs(l1.item() - l0.item()) <= 1e-8 * abs(l0.item())
    g0 = torch.autograd.grad(l0, chol.parameters())
    g1 = torch.autograd.grad(l1, est.parameters())
    for a, b in zip(g0, g1):
        assert torch.allclose(b, a, rtol=1e-7, atol=1e-7 * float(a.abs().max())), (a, b)


def test_adam_training_with_the_preconditioner_tracks_cholesky_training():
    from cggp import kernels, models, training
    from cggp.conjugate_gradient import ConjugateGradient, PivotedCholeskyPreconditioner
    N, D = 8192, 3
    rng = np.random.default_rng(21)
    Xn = rng.uniform(-2, 2, (N, D))
    Yn = np.sin(1.5 * Xn[:, :1]) * np.cos(Xn[:, 1:2]) + 0.3 * Xn[:, 2:3] + np.sqrt(0.1) * rng.standard_normal((N, 1))
    X, Y = T(Xn), T(Yn)
    k0 = kernels.SquaredExponential(0.3, [3.0, 3.0, 3.0])
    exact = lambda m: models.GPR((X, Y), m.kernel.frozen(), noise_variance=m.likelihood_variance.value,
                                 solver="cholesky").log_marginal_likelihood()
    mc = training.TrainableGPR(k0, 1.0, X, Y)
    pre = PivotedCholeskyPreconditioner(rank=128)
    me = training.TrainableGPR(k0, 1.0, X, Y, num_probes=15,
                               conjugate_gradient=ConjugateGradient(1e-10, preconditioner=pre))
    a, b = me.log_marginal_likelihood().item(), me.log_marginal_likelihood().item()
    assert a == b  # repeated evaluations at one theta agree
    start = exact(me)
    training.train_using_adam_and_update((X, Y), mc, 40, N, 0.05)
    training.train_using_adam_and_update((X, Y), me, 40, N, 0.05)
    lc, le = exact(mc), exact(me)
    print(f"start {start:.3f} cholesky-trained {lc:.3f} estimate-trained {le:.3f}")
    assert le > start
    assert abs(le - lc) <= 0.01 * abs(lc), (start, lc, le)


def test_estimate_and_gradient_at_2_17_rows_within_the_memory_bound():
    from cggp import _hip, kernels, training
    from cggp.conjugate_gradient import ConjugateGradient, PivotedCholeskyPreconditioner
    N, D, k = 1 << 17, 2, 128
    Xn, yn = table_inputs(N, D)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    X, Y = T(Xn), T(yn[:, None])
    idx = DEV.index or 0
    shared = _hip._handles.get(idx)
    _hip._handles[idx] = _hip.Handle(idx)  # a fresh handle: its workspace is this evaluation's alone
    try:
        pre = PivotedCholeskyPreconditioner(rank=k)
        m = training.TrainableGPR(kernels.SquaredExponential(1.0, [1.5] * D), 0.1, X, Y, num_probes=15,
                                  conjugate_gradient=ConjugateGradient(1e-8, preconditioner=pre))
        loss = m.training_loss()
        grads = torch.autograd.grad(loss, m.parameters())
        torch.cuda.synchronize()
        ws = _hip.load_library().mgp_workspace_bytes(_hip._handles[idx].h)
    finally:
        if shared is None:
            del _hip._handles[idx]
        else:
            _hip._handles[idx] = shared
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"loss {loss.item():.3f} rank {pre.rank_} peak torch {peak / 2**20:.0f} MiB workspace {ws / 2**20:.0f} MiB")
    assert math.isfinite(loss.item()) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert peak + ws < 1.5 * 2**30 + 8 * k * N * 2  # L and B; nothing N x N (8 N^2 = 128 GiB)
