"""CDGP with trainable inducing inputs, the parts that need no GPU: the reference of the device test
(tests/cdgp_tip_reference.py) held to finite differences of its own value, to the exact log-determinant and to the
closed forms of tests/cdgp_mf_reference.py; `training.k_grad_points` against autograd; the symmetrisation identity
behind the matrix-free nodes (one rank-2R `mgp_kmn_knm_vjp` call on (Z, Z) gives dZ and twice the hyper-parameter
forms) on the long-double reference; and what the constructor of `TrainableCGGP(trainable_inducing=True)` promises."""

import numpy as np
import pytest
import torch

import cdgp_mf_reference as mf
import cdgp_tip_reference as tip
from cggp import training
from sgpr_grad_reference import kernel_torch, kmn_knm_vjp_reference

KINDS = mf.KINDS


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def small_problem(kind, M=12, D=2, B=7, P=4, seed=0):
    rng = np.random.default_rng(seed)
    Z, x = t(rng.uniform(-1.5, 1.5, (M, D))), t(rng.uniform(-1.5, 1.5, (B, D)))
    y, u = t(rng.standard_normal((B, 1))), t(rng.standard_normal((M, 1)))
    counts = t(rng.integers(1, 6, (M, 1)))
    probes = t(2.0 * rng.integers(0, 2, (M, P)) - 1.0)
    return dict(kind=kind, variance=t(1.3), ls=t(rng.uniform(0.7, 1.2, D)), s2=t(0.4), Z=Z, x=x, y=y, pseudo_u=u,
                counts=counts, probes=probes, num_data=50)


def dist(got, want):
    got, want = (torch.as_tensor(v, dtype=torch.float64).detach().reshape(-1) for v in (got, want))
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("kind", KINDS)
def test_reference_gradient_in_z_matches_central_differences_of_its_value(kind):
    """With the exact log-determinant every term of the value depends on Z, so central differences see all of them.
    h = 1e-5 on a value of order 10: truncation ~h^2 and rounding ~1e-15 / h are both far below the bar of 1e-6 of the
    largest entry."""
    p = small_problem(kind)
    _, grads = tip.loss_and_grads(**p, logdet="exact")
    gZ = grads[3]
    h, fd = 1e-5, torch.zeros_like(p["Z"])
    with torch.no_grad():
        for i in range(p["Z"].shape[0]):
            for d in range(p["Z"].shape[1]):
                vals = []
                for sgn in (1.0, -1.0):
                    q = dict(p)
                    q["Z"] = p["Z"].clone()
                    q["Z"][i, d] += sgn * h
                    vals.append(-float(tip.elbo(**q, logdet="exact")))
                fd[i, d] = (vals[0] - vals[1]) / (2.0 * h)
    print(f"{kind}: dZ against central differences {dist(gZ, fd):.2e} (bar 1e-6)")
    assert bool(torch.isfinite(gZ).all()) and float(gZ.abs().max()) > 0.0
    assert dist(gZ, fd) <= 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_surrogate_gradient_is_exact_with_scaled_unit_probes(kind):
    """probes = sqrt(M) I: sum_r z_r z_r^T / P = I, so the estimator's gradient is that of log|A| -- in Z too."""
    p = small_problem(kind, seed=1)
    M = p["Z"].shape[0]
    p["probes"] = np.sqrt(M) * torch.eye(M, dtype=torch.float64)
    l_m, g_m = tip.loss_and_grads(**p, logdet="model")
    l_e, g_e = tip.loss_and_grads(**p, logdet="exact")
    for name, a, b in zip(("dvariance", "dls", "ds2", "dZ"), g_m, g_e):
        print(f"{kind} {name}: {dist(a, b):.2e} (bar 1e-10)")
        assert dist(a, b) <= 1e-10
    # the model's log-determinant has the value 0.0: the two losses differ by log|A| / 2 exactly
    A = tip.kzz(kind, p["variance"], p["ls"], p["Z"]) + torch.diag(p["s2"] / p["counts"].reshape(-1))
    assert abs((l_e - l_m) - 0.5 * float(torch.logdet(A))) <= 1e-10 * abs(l_e)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_kernel_agrees_with_the_closed_forms_in_the_hyper_parameters(kind):
    rng = np.random.default_rng(2)
    M, D, R = 40, 3, 4
    Z, U, V = t(rng.uniform(-1.5, 1.5, (M, D))), t(rng.standard_normal((M, R))), t(rng.standard_normal((M, R)))
    Z[1] = Z[0]
    variance, ls = t(1.7).requires_grad_(True), t(rng.uniform(0.6, 1.4, D)).requires_grad_(True)
    K = tip.kzz(kind, variance, ls, Z)
    assert dist(K, mf.kzz(kind, variance, ls, Z)) <= 1e-14
    got = torch.autograd.grad((U * (K @ V)).sum(), [variance, ls])
    with torch.no_grad():
        want = mf.bilinear_grads(kind, variance, ls, Z, U, V)
    assert dist(got[0], want[0]) <= 1e-10 and dist(got[1], want[1]) <= 1e-10


# ---------------------------------------------------------------- k_grad_points
@pytest.mark.parametrize("D", [1, 3, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_k_grad_points_against_autograd(kind, D):
    rng = np.random.default_rng(D)
    na, nb = 23, 17
    A, B = t(rng.uniform(-1.5, 1.5, (na, D))), t(rng.uniform(-1.5, 1.5, (nb, D)))
    G = t(rng.standard_normal((na, nb)))
    ls = t(rng.uniform(0.7, 1.3, D) * np.sqrt(D))
    Al, Bl = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
    want = torch.autograd.grad((G * kernel_torch(kind, t(1.4), ls, Al, Bl)).sum(), [Al, Bl])
    for chunk in (1 << 24, nb * D * 5):  # one chunk, and chunks of 5 rows with a short last one
        dA, dB = training.k_grad_points(kind, 1.4, ls.tolist(), A, B, G, max_elems=chunk)
        assert dA.shape == A.shape and dB.shape == B.shape
        assert dist(dA, want[0]) <= 1e-12 and dist(dB, want[1]) <= 1e-12


@pytest.mark.parametrize("kind", ["matern12", "matern32", "matern52"])
def test_k_grad_points_is_exactly_zero_at_coincident_points(kind):
    rng = np.random.default_rng(5)
    A = t(rng.uniform(-1.0, 1.0, (6, 3)))
    G = t(rng.standard_normal((6, 6)))
    # every pair coincident: A against copies of one of its rows
    B = A[2:3].repeat(6, 1)
    dA, dB = training.k_grad_points(kind, 1.1, [0.9, 1.0, 1.2], B, B.clone(), G)
    assert float(dA.abs().max()) == 0.0 and float(dB.abs().max()) == 0.0
    # the diagonal of k(A, A) adds nothing and no NaN
    dA, dB = training.k_grad_points(kind, 1.1, [0.9, 1.0, 1.2], A, A, torch.diag(torch.diagonal(G)))
    assert float(dA.abs().max()) == 0.0 and float(dB.abs().max()) == 0.0
    dA, dB = training.k_grad_points(kind, 1.1, [0.9, 1.0, 1.2], A, A, G)
    assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dB).all())


@pytest.mark.parametrize("kind", KINDS)
def test_k_grad_points_adds_up_to_kmm_grad_z(kind):
    rng = np.random.default_rng(6)
    Z, G = t(rng.uniform(-1.5, 1.5, (31, 3))), t(rng.standard_normal((31, 31)))
    ls = [0.8, 1.0, 1.3]
    dA, dB = training.k_grad_points(kind, 1.2, ls, Z, Z, G)
    assert dist(dA + dB, training.kmm_grad_z(kind, 1.2, ls, Z, G)) <= 1e-13


# ---------------------------------------------------------------- the symmetrisation identity
@pytest.mark.parametrize("kind", KINDS)
def test_rank_2r_cotangent_on_z_z_gives_dz_and_twice_the_bilinear_forms(kind):
    """Y = [U | V], Gb = [V | U], Gq = 0 on (Z, Z): W = U V^T + V U^T."""
    rng = np.random.default_rng(7)
    M, D, R = 40, 3, 5
    Z, U, V = rng.uniform(-1.5, 1.5, (M, D)), rng.standard_normal((M, R)), rng.standard_normal((M, R))
    ls, variance = rng.uniform(0.6, 1.4, D), 1.7
    dv, dl, dZ, _, _, _ = kmn_knm_vjp_reference(kind, variance, ls, Z, Z, np.zeros((M, M)), np.hstack([U, V]),
                                                np.hstack([V, U]))
    with torch.no_grad():
        bv, bl = mf.bilinear_grads(kind, t(variance), t(ls), t(Z), t(U), t(V))
    assert dist(float(dv), 2.0 * bv) <= 1e-12
    assert dist(dl.astype(np.float64), 2.0 * bl) <= 1e-12
    Zl = t(Z).requires_grad_(True)
    want, = torch.autograd.grad((t(U) * (tip.kzz(kind, t(variance), t(ls), Zl) @ t(V))).sum(), [Zl])
    print(f"{kind}: dZ {dist(dZ.astype(np.float64), want):.2e} (bar 1e-12)")
    assert dist(dZ.astype(np.float64), want) <= 1e-12


# ---------------------------------------------------------------- the constructor
def make_model(D=3, **kw):
    from cggp import kernels
    rng = np.random.default_rng(8)
    M = 10
    Z = t(rng.uniform(-1.0, 1.0, (M, D)))
    kern = kernels.Matern32(variance=1.1, lengthscales=[1.0] * D)
    m = training.TrainableCGGP(kern, 0.3, Z, pseudo_u=t(rng.standard_normal((M, 1))), cluster_counts=t(np.ones((M, 1))),
                               **kw)
    return m, Z


@pytest.mark.parametrize("matrix_free", [False, True])
def test_parameters_gain_exactly_z_and_z_is_a_clone(matrix_free):
    plain, Z = make_model(matrix_free=matrix_free)
    assert plain.Z is Z and not plain.Z.requires_grad and len(plain.parameters()) == 3  # the default: as before
    m, Z = make_model(matrix_free=matrix_free, trainable_inducing=True)
    ps = m.parameters()
    assert len(ps) == 4 and ps[3] is m.Z and all(a.shape == b.shape for a, b in zip(ps[:3], plain.parameters()))
    assert m.Z.requires_grad and m.Z.is_leaf and m.Z.is_contiguous()
    assert torch.equal(m.Z.detach(), Z) and m.Z.data_ptr() != Z.data_ptr() and not Z.requires_grad
    assert not m.pseudo_u.requires_grad and not m.cluster_counts.requires_grad


def test_matrix_free_refuses_more_than_32_dimensions_only_when_z_is_trainable():
    with pytest.raises(ValueError, match="D <= 32"):
        make_model(D=33, matrix_free=True, trainable_inducing=True)
    assert make_model(D=33, matrix_free=True)[0].matrix_free
    assert make_model(D=33, trainable_inducing=True)[0].Z.requires_grad  # the dense model takes any D
    assert make_model(D=32, matrix_free=True, trainable_inducing=True)[0].Z.requires_grad
