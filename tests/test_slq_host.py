"""Stochastic Lanczos quadrature from CG coefficients (cggp.slq), host only: a numpy CG on random SPD matrices, the
tridiagonal against an explicit Lanczos, the quadrature against eigh, truncation; and the argument checks of the two
new entry points that need no device."""

import ctypes

import numpy as np
import pytest

from cggp import slq


def _spd(n, seed, cond=50.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.geomspace(1.0, cond, n)
    return (Q * lam) @ Q.T


def _cg_record(A, b, steps, min_float=1e-16):
    """The recurrence of csrc/cg.hip (identity preconditioner, x0 = 0): (gamma, beta, 0.5 rz after) per step."""
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rz = r @ r
    out = []
    for _ in range(steps):
        Ap = A @ p
        d = p @ Ap
        gamma = 0.0 if d <= min_float else rz / d
        x += gamma * p
        r -= gamma * Ap
        rz_new = r @ r
        beta = 0.0 if rz <= min_float else rz_new / rz
        p = r + beta * p if rz > min_float else r.copy()
        out.append((gamma, beta, 0.5 * rz_new))
        rz = rz_new
    return np.array(out)


def _lanczos(A, q0, m):
    """Explicit Lanczos with full reorthogonalisation: Q [n, m], T = Q^T A Q."""
    n = A.shape[0]
    Q = np.zeros((n, m))
    Q[:, 0] = q0 / np.linalg.norm(q0)
    for k in range(1, m):
        w = A @ Q[:, k - 1]
        w -= Q[:, :k] @ (Q[:, :k].T @ w)
        w -= Q[:, :k] @ (Q[:, :k].T @ w)
        Q[:, k] = w / np.linalg.norm(w)
    return Q, Q.T @ A @ Q


def test_tridiagonal_from_cg_matches_explicit_lanczos():
    A = _spd(60, 0)
    z = np.random.default_rng(1).choice([-1.0, 1.0], 60)
    m = 12
    rec = _cg_record(A, z, m)
    T = slq.lanczos_tridiagonal(rec[:, 0], rec[:, 1])
    _, T0 = _lanczos(A, z, m)
    # Lanczos vectors are the normalised residuals up to sign: the off-diagonal signs may differ
    assert np.max(np.abs(np.diag(T) - np.diag(T0))) < 1e-10
    assert np.max(np.abs(np.abs(np.diag(T, 1)) - np.abs(np.diag(T0, 1)))) < 1e-10


def test_quadrature_converges_to_the_log_quadratic_form():
    n = 40
    A = _spd(n, 2, cond=20.0)
    z = np.random.default_rng(3).choice([-1.0, 1.0], n)
    lam, Q = np.linalg.eigh(A)
    exact = float(z @ (Q * np.log(lam)) @ Q.T @ z)
    rec = _cg_record(A, z / np.linalg.norm(z), n)
    vals, used = slq.slq_log_quadratic(rec[:, None, :], [z @ z], threshold=1e-28)
    assert used[0] >= 10
    assert abs(vals[0] - exact) < 1e-8 * max(1.0, abs(exact))


def test_truncation_at_breakdown_convergence_and_end():
    g = np.array([0.5, 0.4, 0.0, 0.3])
    b = np.array([0.2, 0.1, 0.1, 0.1])
    hr = np.array([1.0, 0.5, 0.2, 0.1])
    assert slq.usable_steps(g, b, hr) == 2  # gamma = 0 at step 2
    assert slq.usable_steps(g[:2], b[:2], hr[:2]) == 2  # the record's end
    assert slq.usable_steps([0.5, 0.4, 0.3], [0.2, 0.1, 0.1], [1.0, 1e-12, 1e-13], threshold=1e-10) == 2  # converged
    assert slq.usable_steps([0.5, 0.4, 0.3], [0.0, 0.1, 0.1], [1e-20, 1.0, 1.0], min_float=1e-16) == 1  # rz <= min_float
    # a truncated column gives the quadrature of its leading block; an empty one gives 0
    rec = np.zeros((3, 2, 3))
    rec[:, 0] = np.stack([[0.5, 0.4, 0.0], [0.2, 0.1, 0.1], [1.0, 0.5, 0.2]], axis=1)
    vals, used = slq.slq_log_quadratic(rec, [4.0, 4.0])
    assert list(used) == [2, 0] and vals[1] == 0.0
    T = slq.lanczos_tridiagonal([0.5, 0.4], [0.2])
    assert np.isfinite(vals[0]) and abs(vals[0] - slq.quadratic_log(T, 4.0)) == 0.0
    with pytest.raises(ValueError):
        slq.slq_log_quadratic(np.zeros((3, 2)), [1.0, 1.0])


def test_new_entry_points_reject_bad_arguments():
    from cggp import _hip
    lib = _hip.load_library()
    k = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    dv = ctypes.c_double(0.0)
    dl = (ctypes.c_double * _hip.MGP_MAX_D)()
    BAD = -1  # MGP_E_BADARG
    assert lib.mgp_kxx_grad(None, ctypes.byref(k), None, 4, None, None, 1, 0, ctypes.byref(dv), dl) == BAD
    assert lib.mgp_pcg_solve_record(None, None, None, None, None, 1, 1e-6, 10, 11, 1e-16, 10, None, None, None,
                                    None, 10) == BAD
    # a handle without a GPU cannot be created here; the checks behind it are covered on the device
    assert _hip.SIGNATURES["mgp_kxx_grad"][1][6] is ctypes.c_int32
    assert _hip.SIGNATURES["mgp_pcg_solve_record"][1][-1] is ctypes.c_int64


def test_gpr_estimate_and_trainable_modes_are_exposed():
    import torch
    from cggp import kernels, models, ops, training
    assert callable(ops.kxx_grad) and callable(ops.pcg_solve_record)
    assert models.LMLEstimate._fields == ("value", "log_det", "data_fit", "std_error", "iterations", "converged")
    X, Y = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64)
    m = training.TrainableGPR(kernels.SquaredExponential(1.0, [1.0, 1.0]), 0.1, X, Y, num_probes=3, probe_seed=5)
    assert m.probes.shape == (4, 3) and set(m.probes.unique().tolist()) <= {-1.0, 1.0}
    p0 = m.probes.clone()
    m.resample_probes(5)
    assert torch.equal(p0, m.probes)
    assert training.TrainableGPR(kernels.SquaredExponential(1.0, [1.0, 1.0]), 0.1, X, Y).num_probes is None
