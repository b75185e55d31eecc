"""The trace form of the CDGP data term, the parts that need no GPU: the reference of the device test
(tests/cdgp_full_reference.py) held to the batch form's reference (tests/cdgp_tip_reference.py) where the two must agree
-- with probes = sqrt(M) I the estimator is exact -- and its Rademacher estimate held to the exact trace; and what the
constructors of `TrainableCGGP(data_term=...)` and `CGGP(data_term=...)` promise."""

import inspect

import numpy as np
import pytest
import torch

import cdgp_full_reference as full
import cdgp_mf_reference as mf
import cdgp_tip_reference as tip
from cggp import models, training
from test_cdgp_tip_host import dist, small_problem, t

KINDS = mf.KINDS


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("num_data", [None, 50])
@pytest.mark.parametrize("kind", KINDS)
def test_with_scaled_unit_probes_the_trace_form_is_the_batch_form(kind, num_data):
    """probes = sqrt(M) I: sum_p z_p z_p^T / P = I, so (1/P) sum_p (K_nm A^-1 z_p) . (K_nm z_p) = tr(A^-1 K_mn K_nm)
    = sum_n k_n^T A^-1 k_n, the batch form's sum, as an identity in every parameter."""
    p = small_problem(kind, seed=3)
    M = p["Z"].shape[0]
    p["probes"] = np.sqrt(M) * torch.eye(M, dtype=torch.float64)
    p["num_data"] = num_data
    p["x"][:2] = p["Z"][:2]  # data rows on inducing points: the floor of the Matern slopes
    l_f, g_f = full.loss_and_grads(**p)
    l_b, g_b = tip.loss_and_grads(**p)
    print(f"{kind}: loss {abs(l_f - l_b) / abs(l_b):.2e} (bar 1e-12)")
    assert abs(l_f - l_b) <= 1e-12 * abs(l_b)
    for name, a, b in zip(("dvariance", "dls", "ds2", "dZ"), g_f, g_b):
        print(f"{kind} {name}: {dist(a, b):.2e} (bar 1e-12)")
        assert dist(a, b) <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_the_exact_form_is_the_batch_form_and_the_scaled_unit_probes(kind):
    p = small_problem(kind, seed=4)
    M = p["Z"].shape[0]
    eye = dict(p, probes=np.sqrt(M) * torch.eye(M, dtype=torch.float64))
    l_e, g_e = full.loss_and_grads(**dict(p, probes=None))
    l_p, g_p = full.loss_and_grads(**eye)
    assert abs(l_e - l_p) <= 1e-12 * abs(l_p)
    for a, b in zip(g_e, g_p):
        assert dist(a, b) <= 1e-10  # the surrogate's gradient against torch.logdet's


SEEDS = tuple(range(100, 1124))  # 1024 draws of P = 5 probes each


@pytest.mark.parametrize("kind", KINDS)
def test_the_rademacher_estimate_is_unbiased(kind):
    """The mean over the draws lies within 4 standard errors of the exact value.  The list of seeds is fixed, so the
    test is deterministic.  On this small, badly conditioned problem one draw of 5 probes has a standard deviation of
    several times the exact value; the first 64, 256, 1024 and 2048 seeds of this stream gave z = -2.3, -2.2, -0.3 and
    -0.1 for the squared exponential (the four kernels share their probes and move together), so 1024 draws it is:
    the running mean has settled and |z| stays under 1."""
    p = small_problem(kind, M=30, B=40, seed=5)
    args = (kind, p["variance"], p["ls"], p["s2"], p["Z"], p["x"], p["counts"])
    with torch.no_grad():
        exact = float(full.variance_sum(*args))
        batch = p["x"].shape[0] * float(p["variance"]) - float(
            (tip.kernel_torch(kind, p["variance"], p["ls"], p["Z"], p["x"])
             * torch.linalg.solve(tip.kzz(kind, p["variance"], p["ls"], p["Z"])
                                  + torch.diag(p["s2"] / p["counts"].reshape(-1)),
                                  tip.kernel_torch(kind, p["variance"], p["ls"], p["Z"], p["x"]))).sum())
        assert abs(exact - batch) <= 1e-12 * abs(batch)  # the trace IS the batch form's sum of variances
        draws = []
        for seed in SEEDS:
            probes = t(2.0 * np.random.default_rng(seed).integers(0, 2, (30, 5)) - 1.0)
            draws.append(float(full.variance_sum(*args, probes=probes)))
    draws = np.array(draws)
    se = draws.std(ddof=1) / np.sqrt(len(draws))
    z = (draws.mean() - exact) / se
    print(f"{kind}: exact {exact:.6f}, mean of {len(draws)} draws {draws.mean():.6f}, standard error {se:.2e}, z {z:+.2f}")
    assert se > 0.0 and abs(z) <= 4.0


def test_a_batch_without_rows_gives_minus_kl():
    p = small_problem("matern32", seed=6)
    q = dict(p, x=p["x"][:0], y=p["y"][:0])
    with torch.no_grad():
        e0 = float(full.elbo(**q))
        # the KL of the batch form: its elbo minus its data term, at any batch
        Kmn = tip.kernel_torch("matern32", p["variance"], p["ls"], p["Z"], p["x"])
        A = tip.kzz("matern32", p["variance"], p["ls"], p["Z"]) + torch.diag(p["s2"] / p["counts"].reshape(-1))
        fvar = p["variance"] - (Kmn * torch.linalg.solve(A, Kmn)).sum(dim=0)[:, None]
        fmu = Kmn.t() @ torch.linalg.solve(A, p["pseudo_u"])
        ve = -0.5 * np.log(2.0 * np.pi) - 0.5 * torch.log(p["s2"]) - 0.5 * ((p["y"] - fmu) ** 2 + fvar) / p["s2"]
        scale = p["num_data"] / p["x"].shape[0]
        minus_kl = float(tip.elbo(**p)) - scale * float(ve.sum())
    assert np.isfinite(e0) and abs(e0 - minus_kl) <= 1e-12 * abs(minus_kl)


# ---------------------------------------------------------------- the constructors
def make_trainable(D=3, dtype=torch.float64, **kw):
    from cggp import kernels
    rng = np.random.default_rng(8)
    M = 10
    Z = t(rng.uniform(-1.0, 1.0, (M, D))).to(dtype)
    kern = kernels.Matern32(variance=1.1, lengthscales=[1.0] * D)
    return training.TrainableCGGP(kern, 0.3, Z, pseudo_u=t(rng.standard_normal((M, 1))).to(dtype),
                                  cluster_counts=t(np.ones((M, 1))).to(dtype), **kw)


def make_frozen(D=3, dtype=torch.float64, **kw):
    from cggp import kernels
    from cggp.conjugate_gradient import ConjugateGradient
    rng = np.random.default_rng(8)
    M = 10
    Z = t(rng.uniform(-1.0, 1.0, (M, D))).to(dtype)
    kern = kernels.Matern32(variance=1.1, lengthscales=[1.0] * D)
    return models.CGGP(kern, 0.3, Z, ConjugateGradient(1e-6), pseudo_u=t(rng.standard_normal((M, 1))).to(dtype),
                       cluster_counts=t(np.ones((M, 1))).to(dtype), **kw)


def test_batch_stays_the_default():
    assert make_trainable().data_term == "batch" and make_trainable(matrix_free=True).data_term == "batch"
    assert make_frozen().data_term == "batch"
    assert inspect.signature(training.TrainableCGGP.__init__).parameters["data_term"].default == "batch"
    assert inspect.signature(models.CGGP.__init__).parameters["data_term"].default == "batch"
    assert make_trainable(dtype=torch.float32).data_term == "batch"  # fp32 is refused for "trace" only


@pytest.mark.parametrize("matrix_free", [False, True])
def test_the_keyword_is_kept_and_handed_on(matrix_free):
    m = make_trainable(matrix_free=matrix_free, data_term="trace")
    assert m.data_term == "trace" and len(m.parameters()) == 3
    frozen = m.frozen_model()
    assert frozen.data_term == "trace" and frozen.matrix_free == matrix_free
    assert make_trainable(matrix_free=matrix_free).frozen_model().data_term == "batch"
    assert make_frozen(matrix_free=matrix_free, data_term="trace").data_term == "trace"
    from cggp import kernels
    Z = t(np.random.default_rng(1).uniform(-1.0, 1.0, (6, 2)))
    assert models.cdgp_class(kernels.SquaredExponential(1.0, [1.0, 1.0]), 0.3, Z, matrix_free=matrix_free,
                             data_term="trace").data_term == "trace"


def test_what_the_trace_form_refuses():
    for make in (make_trainable, make_frozen):
        with pytest.raises(ValueError, match="data_term must be one of"):
            make(data_term="hutchinson")
        with pytest.raises(ValueError, match="fp64 only"):
            make(dtype=torch.float32, data_term="trace")
        with pytest.raises(ValueError, match="fp64 only"):
            make(dtype=torch.float32, data_term="trace", matrix_free=True)
    for matrix_free in (False, True):
        with pytest.raises(ValueError, match="D <= 32"):
            make_trainable(D=33, data_term="trace", trainable_inducing=True, matrix_free=matrix_free)
        assert make_trainable(D=33, data_term="trace", matrix_free=matrix_free).data_term == "trace"  # theta alone: fine
        assert make_trainable(D=32, data_term="trace", trainable_inducing=True, matrix_free=matrix_free).Z.requires_grad
    assert make_trainable(D=33, trainable_inducing=True).Z.requires_grad  # "batch", dense: any D, as before
    # the exact trace solves M right-hand sides: the matrix-free models refuse it before any device work
    data = (torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="num_probes"):
        make_trainable(matrix_free=True, data_term="trace", num_probes=None).elbo(data)
    with pytest.raises(ValueError, match="num_probes"):
        make_frozen(matrix_free=True, data_term="trace", num_probes=None).elbo(data)
