"""Random Fourier features on the host (no GPU): the spectral draws of `cggp.rff`, the reference's own kernel check
of the feature map, and the two noise conventions of the pathwise update (`cggp.models.pathwise_epsilon`)."""

import numpy as np
import pytest
import torch
from scipy import stats

from cggp import kernels, models, rff
from oracle import kernels as ok

KINDS = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
         "matern52": kernels.Matern52}
NU = {"matern12": 1, "matern32": 3, "matern52": 5}


def test_draws_reproducible_from_seed():
    k = kernels.Matern32(variance=1.3, lengthscales=[0.5, 2.0, 1.0])
    a = rff.basis_theta_parameter(k, 64, seed=7)
    b = rff.basis_theta_parameter(k, 64, seed=7)
    c = rff.basis_theta_parameter(k, 64, seed=8)
    assert a.shape == (64, 3) and a.dtype == torch.float64
    assert torch.equal(a, b) and not torch.equal(a, c)
    X = torch.randn(10, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    s1 = rff.rff_sample(X, k, 64, 4, seed=3)
    s2 = rff.rff_sample(X, k, 64, 4, seed=3)
    assert s1.shape == (4, 10) and torch.equal(s1, s2)
    # the documented stream: theta first, then W, from one PCG64 generator
    rng = np.random.default_rng(3)
    th = rff.basis_theta_parameter(k, 64, rng)
    W = torch.from_numpy(rng.standard_normal((4, 128)))
    np.testing.assert_array_equal(s1.numpy(), rff.rff_sample(X, k, 64, theta=th, weights=W).numpy())


def test_isotropic_lengthscale_needs_dim():
    k = kernels.SquaredExponential(lengthscales=0.7)
    th = rff.basis_theta_parameter(k, 5, seed=0, dim=4)
    assert th.shape == (5, 4)
    X = torch.zeros(3, 4, dtype=torch.float64)
    assert rff.rff_sample(X, k, 5, 2, seed=0).shape == (2, 3)


@pytest.mark.parametrize("kind", ["se", "matern12", "matern32", "matern52"])
def test_theta_law(kind):
    """theta * lengthscale: N(0, I) for SE, a multivariate Student-t with nu = 1, 3, 5 degrees of freedom (one
    chi-square factor per basis, shared by the coordinates) for Matern-nu/2 (reference rff.py:20-45,82-91)."""
    n, ls = 200_000, np.array([0.3, 1.0, 4.0])
    th = rff.basis_theta_parameter(KINDS[kind](lengthscales=ls), n, seed=11).numpy() * ls[None, :]
    law = stats.norm() if kind == "se" else stats.t(NU[kind])
    ps = np.array([0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
    q = law.ppf(ps)
    # standard error of an empirical p-quantile: sqrt(p (1-p) / n) / density(q); 5 of them
    tol = 5 * np.sqrt(ps * (1 - ps) / n) / law.pdf(q)
    for d in range(3):
        np.testing.assert_array_less(np.abs(np.quantile(th[:, d], ps) - q), tol)
        assert stats.kstest(th[:, d], law.cdf).pvalue > 1e-4
    if kind == "se":
        np.testing.assert_array_less(np.abs(th.mean(0)), 5 / np.sqrt(n))
        np.testing.assert_array_less(np.abs(th.var(0) - 1), 5 * np.sqrt(2 / n))
        r = np.corrcoef(np.abs(th[:, 0]), np.abs(th[:, 1]))[0, 1]
        assert abs(r) < 5 / np.sqrt(n)  # independent coordinates
    else:
        if kind == "matern52":  # nu = 5: finite fourth moment, var = nu / (nu - 2)
            np.testing.assert_allclose(th.var(0), 5 / 3, rtol=0.05)
        r = np.corrcoef(np.abs(th[:, 0]), np.abs(th[:, 1]))[0, 1]
        assert r > 0.05  # the shared chi-square factor couples the magnitudes


@pytest.mark.parametrize("kind", ["se", "matern32", "matern52"])
def test_features_approximate_kernel(kind):
    """The reference's own check (rff_test.py:9-30): sigma^2 / L Phi Phi^T -> K with L = 1e5 bases, atol 1e-2."""
    rng = np.random.default_rng(5)
    inputs = rng.standard_normal((4, 2))
    ls = rng.random(2) ** 2 + 0.5
    variance = 1.3
    k = KINDS[kind](variance=variance, lengthscales=ls)
    L = 100_000
    theta = rff.basis_theta_parameter(k, L, seed=6)
    phi = rff.basis_vectors(torch.from_numpy(inputs), theta).numpy()
    assert phi.shape == (4, 2 * L)
    approx = variance / L * phi @ phi.T
    kxx = ok.Kernel(kind, variance, ls).K(inputs)
    np.testing.assert_allclose(approx, kxx, rtol=1e-3, atol=1e-2)


def test_basis_vectors_cos_block_first():
    X = torch.tensor([[0.25, -1.0]], dtype=torch.float64)
    th = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, 1.0]], dtype=torch.float64)
    phi = rff.basis_vectors(X, th)
    xt = (X @ th.t())[0]
    np.testing.assert_allclose(phi[0, :3].numpy(), np.cos(xt.numpy()), rtol=0, atol=1e-15)
    np.testing.assert_allclose(phi[0, 3:].numpy(), np.sin(xt.numpy()), rtol=0, atol=1e-15)


def test_epsilon_conventions():
    lam = torch.tensor([0.04, 0.25, 1.0, 9.0], dtype=torch.float64)
    xi = torch.from_numpy(np.random.default_rng(2).standard_normal((3, 4)))
    ref = models.pathwise_epsilon(lam, 3, "reference", xi=xi)
    mat = models.pathwise_epsilon(lam, 3, "matheron", xi=xi)
    np.testing.assert_array_equal(ref.numpy(), (lam[None, :] * xi).numpy())  # scale_diag = lambda (models.py:404-408)
    np.testing.assert_allclose(mat.numpy(), (np.sqrt(lam.numpy())[None, :] * xi.numpy()), rtol=1e-15)
    # drawn from a seed: the same normals under both conventions, covariance lambda^2 vs lambda
    big_r = models.pathwise_epsilon(lam, 100_000, "reference", seed=9)
    big_m = models.pathwise_epsilon(lam, 100_000, "matheron", seed=9)
    np.testing.assert_allclose((big_r / lam).numpy(), (big_m / torch.sqrt(lam)).numpy(), rtol=1e-14)
    np.testing.assert_allclose(big_r.var(0).numpy(), (lam ** 2).numpy(), rtol=0.02)
    np.testing.assert_allclose(big_m.var(0).numpy(), lam.numpy(), rtol=0.02)
    with pytest.raises(ValueError):
        models.pathwise_epsilon(lam, 1, "other", xi=xi[:1])
