"""Host-side checks of the pivoted-Cholesky preconditioner: the exported entry points and the ABI mirror, the torch
form of `PivotedCholeskyPreconditioner` (Woodbury inverse, log-determinant, sampling) against numpy, and the
preconditioned stochastic-Lanczos identity log|Khat| = log|P| + E[z^T P^-1 z e1^T log(T) e1] through `cggp.slq`."""

import ctypes

import numpy as np
import pytest
import torch

from cggp import _hip, slq
from cggp.conjugate_gradient import PivotedCholeskyPreconditioner
from pivchol_reference import greedy_pivoted_cholesky, kernel_matrix, pcg, woodbury_factor


def test_entry_points_are_exported_and_refuse_a_null_handle():
    lib = _hip.load_library()
    assert hasattr(lib, "mgp_kxx_pivchol") and hasattr(lib, "mgp_lowrank_apply")
    k = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    rank = ctypes.c_int32(7)
    assert lib.mgp_kxx_pivchol(None, ctypes.byref(k), None, 0, 4, 0.0, None, None, None, ctypes.byref(rank)) == -1
    assert lib.mgp_lowrank_apply(None, _hip.F64, None, None, 1, 0, None, 0, None) == -1
    assert _hip.PRE_LOWRANK == 5
    assert ctypes.sizeof(_hip.MgpPrecond) == 80


def _hand_made(n=300, k=7, seed=0):
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((k, n))
    D = 0.05 + rng.random(n) * 2.0  # general positive diagonal
    return L, D, rng


def test_call_is_the_inverse_and_log_det_is_slogdet():
    L, D, rng = _hand_made()
    P = np.diag(D) + L.T @ L
    pre = PivotedCholeskyPreconditioner(rank=7).set_factor(torch.from_numpy(L), torch.from_numpy(D))
    assert pre.rank_ == 7
    R = rng.standard_normal((4, 300))
    z, rz = pre(torch.from_numpy(R), None)
    ref = np.linalg.solve(P, R.T).T
    assert np.max(np.abs(z.numpy() - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.allclose(rz.numpy()[:, 0], (ref * R).sum(axis=1), rtol=1e-11)
    assert np.max(np.abs(pre.solve(torch.from_numpy(R)).numpy() - ref)) <= 1e-12 * np.max(np.abs(ref))
    sld = np.linalg.slogdet(P)[1]
    assert abs(pre.log_det() - sld) <= 1e-12 * abs(sld)
    # a scalar D (the exact-GP system, D = s2 I)
    pre.set_factor(torch.from_numpy(L), 0.1)
    sld = np.linalg.slogdet(0.1 * np.eye(300) + L.T @ L)[1]
    assert abs(pre.log_det() - sld) <= 1e-12 * abs(sld)
    # the helper's factor is the same map
    B, ld = woodbury_factor(L, 0.1)
    assert np.allclose(pre.B.numpy(), B, rtol=1e-10, atol=1e-13) and abs(ld - sld) <= 1e-12 * abs(sld)


def test_samples_have_covariance_p_and_follow_the_seed():
    L, D, _ = _hand_made(n=40, k=3, seed=1)
    pre = PivotedCholeskyPreconditioner(rank=3).set_factor(torch.from_numpy(L), torch.from_numpy(D))
    Z = pre.sample(200000, seed=5)
    assert Z.shape == (40, 200000)
    P = np.diag(D) + L.T @ L
    emp = (Z @ Z.t()).numpy() / Z.shape[1]
    # entries of the empirical covariance have standard error <= sqrt(2) max(P) / sqrt(t)
    assert np.max(np.abs(emp - P)) <= 6 * np.sqrt(2.0) * P.max() / np.sqrt(Z.shape[1])
    assert torch.equal(pre.sample(16, seed=5), pre.sample(16, seed=5))
    assert not torch.equal(pre.sample(16, seed=5), pre.sample(16, seed=6))
    g = torch.Generator().manual_seed(3)
    assert pre.sample(4, generator=g).shape == (40, 4)


def test_needs_a_kxx_operator_or_a_given_factor():
    pre = PivotedCholeskyPreconditioner()
    with pytest.raises(RuntimeError, match="set_factor"):
        pre.log_det()
    with pytest.raises(ValueError):
        PivotedCholeskyPreconditioner(rank=0)

    class Other:
        shape = (4, 4)
        dtype = torch.float64

    with pytest.raises(TypeError, match="KxxNoiseOperator"):
        pre._native(Other())


def test_preconditioned_lanczos_quadrature_gives_slogdet():
    """K + 0.1 I, N = 400, D = 3, SE, lengthscale 1.0, with its exact rank-20 factor; the N probe columns
    Z = sqrt(N) P^(1/2) have Z Z^T / N = P exactly and every weight z^T P^-1 z = N, so log|P| plus the mean of the
    quadratures is log|Khat| up to the quadrature's own error (1e-8 relative; 7e-16 was measured when this was
    specified)."""
    N, s2 = 400, 0.1
    rng = np.random.default_rng(0)
    X = rng.uniform(-3.0, 3.0, (N, 3))
    K = kernel_matrix("se", 1.0, [1.0] * 3, X, dtype=np.float64)
    Khat = K + s2 * np.eye(N)
    L, piv = greedy_pivoted_cholesky(K, 20)
    assert L.shape == (20, N) and len(set(piv)) == 20
    pre = PivotedCholeskyPreconditioner(rank=20).set_factor(torch.from_numpy(L), s2)
    P = s2 * np.eye(N) + L.T @ L
    lam, Q = np.linalg.eigh(P)
    Z = np.sqrt(N) * (Q * np.sqrt(lam)) @ Q.T
    assert np.allclose(Z @ Z.T / N, P, rtol=1e-12, atol=1e-13)
    B = pre.B.numpy()
    dinv = pre.diag_inv.numpy()
    weights = (Z * pre.solve(torch.from_numpy(Z.T.copy())).numpy().T).sum(axis=0)
    assert np.allclose(weights, N, rtol=1e-10)
    quads, steps = [], []
    for c in range(N):
        _, it, coef = pcg(lambda v: Khat @ v, Z[:, c], dinv=dinv, B=B, threshold=1e-26, max_iterations=N,
                          min_float=1e-300)
        q, used = slq.slq_log_quadratic(coef[:, None, :], [weights[c]], 1e-26, 1e-300)
        quads.append(q[0])
        steps.append(it)
    est = pre.log_det() + float(np.mean(quads))
    sld = np.linalg.slogdet(Khat)[1]
    assert max(steps) < N
    assert abs(est - sld) <= 1e-8 * abs(sld), (est, sld)
