"""tests/kvjp_reference.py is what the any-dimension SGPR VJP is held to on the GPU, so it is itself checked here on the
CPU: against central finite differences of the oracle's K_mn K_nm and K_mn y contracted with random Gq, Gb (step
1e-5, relative 1e-6), at a dimension below and one above the fused kernels' 32, and at the Matern floor."""

import numpy as np
import pytest

from kvjp_reference import LD, kvjp_reference
from oracle import kernels as ok

KERNELS = ["se", "matern12", "matern32", "matern52"]
N, M, STEP, REL = 23, 7, 1e-5, 1e-6


def _problem(D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (N, D))
    Z = rng.uniform(-1.5, 1.5, (M, D))
    ls = np.sqrt(D) * np.linspace(0.7, 1.3, D)  # unequal; r2 = O(1) at either D
    # Matern-1/2 is not differentiable at r = 0: every pair at least 0.1 apart (in scaled units too)
    gap = np.sqrt((((X[:, None, :] - Z[None, :, :]) / ls) ** 2).sum(axis=2)).min()
    assert gap >= 0.1, gap
    return X, Z, ls, rng.standard_normal((M, M)), rng.standard_normal((N, 2)), rng.standard_normal((M, 2))


def _objective(name, var, ls, X, Z, Gq, Y, Gb):
    """sum(Gq o K_mn K_nm) + sum(Gb o K_mn Y) on the oracle's kernel"""
    K = ok.Kernel(name, var, ls).K(X, Z)
    return float(np.sum(Gq * (K.T @ K)) + np.sum(Gb * (K.T @ Y)))


@pytest.mark.parametrize("D", [5, 37])
@pytest.mark.parametrize("name", KERNELS)
def test_reference_agrees_with_central_differences(name, D):
    X, Z, ls, Gq, Y, Gb = _problem(D, 100 + D)
    var = 1.4
    ref = kvjp_reference(name, var, ls, X, Z, Gq, Y, Gb)
    L = lambda v, l, z: _objective(name, v, l, X, z, Gq, Y, Gb)
    fd_v = (L(var + STEP, ls, Z) - L(var - STEP, ls, Z)) / (2 * STEP)
    assert abs(fd_v - float(ref.dv)) <= REL * abs(float(ref.dv))
    fd_l, fd_z = np.zeros(D), np.zeros((M, D))
    for d in range(D):
        e = np.zeros(D)
        e[d] = STEP
        fd_l[d] = (L(var, ls + e, Z) - L(var, ls - e, Z)) / (2 * STEP)
        for m in range(M):
            Ez = np.zeros((M, D))
            Ez[m, d] = STEP
            fd_z[m, d] = (L(var, ls, Z + Ez) - L(var, ls, Z - Ez)) / (2 * STEP)
    dl, dZ = ref.dl.astype(np.float64), ref.dZ.astype(np.float64)
    assert np.max(np.abs(fd_l - dl)) <= REL * np.max(np.abs(dl))
    assert np.max(np.abs(fd_z - dZ)) <= REL * np.max(np.abs(dZ))
    # the companions dominate the values, and W's companion dominates W
    assert float(ref.sv) >= abs(float(ref.dv)) and np.all(ref.sl >= np.abs(ref.dl)) and np.all(ref.sz >= np.abs(ref.dZ))
    assert np.all(ref.Wa >= np.abs(ref.W))


def test_w_and_its_companion_are_the_stated_sums():
    X, Z, ls, Gq, Y, Gb = _problem(5, 3)
    ref = kvjp_reference("matern32", 0.9, ls, X, Z, Gq, Y, Gb)
    K = ok.Kernel("matern32", 0.9, ls).K(X, Z)
    G2 = Gq + Gq.T
    assert np.max(np.abs(ref.W.astype(np.float64) - (K @ G2 + Y @ Gb.T))) <= 1e-12
    assert np.max(np.abs(ref.Wa.astype(np.float64) - (np.abs(K) @ np.abs(G2) + np.abs(Y) @ np.abs(Gb).T))) <= 1e-12
    rank = kvjp_reference("matern32", 0.9, ls, X, Z, None, Y, Gb)  # Gq = None: W = Y Gb^T alone
    assert np.max(np.abs(rank.W.astype(np.float64) - Y @ Gb.T)) <= 1e-14


def test_matern12_pair_at_the_floor_adds_exactly_zero():
    X, Z, ls, Gq, Y, Gb = _problem(5, 11)
    X2 = X.copy()
    X2[4] = Z[2]  # r = 0 for the pair (4, 2)
    full = kvjp_reference("matern12", 1.4, ls, X2, Z, Gq, Y, Gb)
    # the same problem with that pair's W removed from the lengthscale and dZ sums: identical, bit for bit
    diff = (X2[4] - Z[2]) / ls
    assert np.all(diff == 0.0)
    rest = kvjp_reference("matern12", 1.4, ls, np.delete(X2, 4, axis=0), Z, Gq, np.delete(Y, 4, axis=0), Gb)
    assert np.all(np.isfinite(full.dl.astype(np.float64))) and np.all(np.isfinite(full.dZ.astype(np.float64)))
    # row 4 reaches dZ[2] only through the pair at the floor (f' = 0 there) and through its other columns
    one = kvjp_reference("matern12", 1.4, ls, X2[4:5], Z, Gq, Y[4:5], Gb)
    assert np.all(one.dZ[2] == 0) and np.all(one.sz[2] == 0)
    assert np.all(np.abs(rest.dZ[2] - full.dZ[2]) <= 64 * np.finfo(LD).eps * full.sz[2])  # summation order only
