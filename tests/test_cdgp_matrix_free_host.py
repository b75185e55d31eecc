"""The reference of the matrix-free CDGP training test, held honest on the CPU: the three backward formulas of
tests/cdgp_mf_reference.py (closed-form kernel derivatives, dense solves) against torch autograd through dense
algebra at M = 40, to 1e-10 of the largest entry of each gradient."""

import numpy as np
import pytest
import torch

import cdgp_mf_reference as ref

M, D, R = 40, 3, 4
BAR = 1e-10


def setup(kind, seed=0):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    Z = t(rng.uniform(-1.5, 1.5, (M, D)))
    Z[1] = Z[0]  # a coincident pair: the 1e-36 floor of the Matern profiles off the diagonal too
    variance = t(1.7).requires_grad_(True)
    ls = t(rng.uniform(0.6, 1.4, D)).requires_grad_(True)
    lam = t(rng.uniform(0.3, 1.2, M)).requires_grad_(True)
    V = t(rng.standard_normal((M, R))).requires_grad_(True)
    G = t(rng.standard_normal((M, R)))
    return Z, variance, ls, lam, V, G


def close(name, got, want):
    got, want = torch.as_tensor(got).detach(), torch.as_tensor(want).detach()
    dist = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    print(f"{name}: {dist:.2e} (bar {BAR:.0e})")
    assert dist <= BAR, (name, dist)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_kzz_times_backward_is_the_gradient_of_the_dense_product(kind):
    Z, variance, ls, lam, V, G = setup(kind)
    out = ref.kzz(kind, variance, ls, Z) @ V
    want = torch.autograd.grad((out * G).sum(), [V, variance, ls])
    with torch.no_grad():
        got = ref.kzz_times_backward(kind, variance, ls, Z, V, G)
    for name, g, w in zip(("dV", "dvariance", "dls"), got, want):
        close(f"{kind} {name}", g, w)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_solve_backward_is_the_gradient_of_the_dense_solve(kind):
    Z, variance, ls, lam, rhs, G = setup(kind, 1)
    X = torch.linalg.solve(ref.kzz(kind, variance, ls, Z) + torch.diag(lam), rhs)
    want = torch.autograd.grad((X * G).sum(), [rhs, variance, ls, lam])
    with torch.no_grad():
        got = ref.solve_backward(kind, variance, ls, lam, Z, rhs, G)
    for name, g, w in zip(("drhs", "dvariance", "dls", "dlam"), got, want):
        close(f"{kind} {name}", g, w)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_logdet_backward_is_the_gradient_of_its_surrogate_and_exact_with_scaled_unit_probes(kind):
    Z, variance, ls, lam, _, _ = setup(kind, 2)
    A = ref.kzz(kind, variance, ls, Z) + torch.diag(lam)
    # any probes: the gradient of sum(S.detach() * (A probes)) / P, which is what the node's dense twin sends back
    probes = torch.from_numpy(2.0 * np.random.default_rng(3).integers(0, 2, (M, 5)) - 1.0)
    S = torch.linalg.solve(A, probes).detach()
    want = torch.autograd.grad(0.7 * (S * (A @ probes)).sum() / 5, [variance, ls, lam], retain_graph=True)
    with torch.no_grad():
        got = ref.logdet_backward(kind, variance, ls, lam, Z, S, probes, df=0.7)
    for name, g, w in zip(("dvariance", "dls", "dlam"), got, want):
        close(f"{kind} surrogate {name}", g, w)
    # probes = sqrt(M) I: sum_r z_r z_r^T / P = I, the estimate is the exact gradient of log|A|
    unit = np.sqrt(M) * torch.eye(M, dtype=torch.float64)
    want = torch.autograd.grad(torch.logdet(A), [variance, ls, lam])
    with torch.no_grad():
        got = ref.logdet_backward(kind, variance, ls, lam, Z, torch.linalg.solve(A, unit), unit)
    for name, g, w in zip(("dvariance", "dls", "dlam"), got, want):
        close(f"{kind} exact {name}", g, w)
