"""tests/cdgp_pathwise_reference.py held to account on the CPU, and the constructors' checks of
`data_term="pathwise"`:
 - its samples are those of the numpy restatement of the reference's `pathwise_samples` (tests/test_gpu_rff.py, which
   holds `PathwiseClusterGP` to it on the device) on the same draws;
 - over 1024 fixed seeds its data term averages to the batch form's `-(1/2) [(|y - mu|^2 + sum_n var_n) / s2 + B log(2
   pi s2)]` of tests/cdgp_full_reference.py, within 4 standard errors (`epsilon="matheron"`);
 - every `ValueError` fires and "batch" is still the default."""

import inspect

import numpy as np
import pytest
import torch

import cdgp_full_reference as full
import cdgp_pathwise_reference as pw
from cggp import models, training
from test_cdgp_tip_host import dist, small_problem, t
from test_gpu_rff import numpy_pathwise


def draw_of(kind, D, M, L, S, seed):
    return models.draw_pathwise(kind, D, M, L, S, seed)


@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_reference_samples_are_the_restated_pathwise_samples(kind):
    p = small_problem(kind, M=12, D=2, B=7)
    E, W, xi = draw_of(kind, 2, 12, 16, 3, seed=4)
    got = pw.samples(kind, p["variance"], p["ls"], p["s2"], p["Z"], p["x"], p["pseudo_u"], p["counts"], (E, W, xi),
                     epsilon="reference")
    lam = (p["s2"] / p["counts"].reshape(-1)).numpy()
    theta = (E / p["ls"][None, :]).numpy()
    want, _ = numpy_pathwise(p["x"].numpy(), p["Z"].numpy(), p["pseudo_u"].numpy()[:, 0], lam, float(p["variance"]),
                             p["ls"].numpy(), theta, W.numpy(), xi.numpy(), kind=kind)
    assert got.shape == (3, 7) and dist(got, want) <= 1e-12


def test_draws_follow_the_documented_stream():
    """bases, then weights, then noise, from one PCG64 stream; the Matern factor sqrt(nu / chi2) is inside E"""
    from cggp import kernels, rff
    E, W, xi = draw_of("matern32", 3, 5, 8, 2, seed=9)
    rng = np.random.default_rng(9)
    E0 = rff.basis_theta_parameter(kernels.Matern32(lengthscales=[1.0] * 3), 8, rng)
    assert torch.equal(E, E0) and torch.equal(W, rff.rff_weights(2, 8, rng))
    assert np.array_equal(xi.numpy(), rng.standard_normal((2, 5)))
    assert E.shape == (8, 3) and W.shape == (2, 16) and xi.shape == (2, 5) and E.dtype == torch.float64


def test_mean_data_term_is_the_batch_data_term():
    """M = 40, B = 150, S = 5, L = 32, 1024 seeds (0 .. 1023).  Given E the samples are linear in (W, xi) and
    E_E[phi phi^T] / L is the kernel exactly, so with eps of covariance Lambda the expectation of sum_n (y_n - f_sn)^2 is
    |y - mu|^2 + sum_n var_n: no truncation bias.  4 standard errors of the mean of the 1024 values."""
    kind, M, D, B, S, L = "matern32", 40, 3, 150, 5, 32
    p = small_problem(kind, M=M, D=D, B=B, seed=2)
    args = [p[k] for k in ("variance", "ls", "s2", "Z", "x", "y", "pseudo_u", "counts")]
    with torch.no_grad():
        exact = float(full.elbo(kind, *args, None) - full.elbo(kind, *args[:4], p["x"][:0], p["y"][:0], *args[6:], None))
        vals = np.array([float(pw.data_term(kind, *args, draw_of(kind, D, M, L, S, seed))) for seed in range(1024)])
    se = vals.std(ddof=1) / np.sqrt(len(vals))
    print(f"batch data term {exact:.6f}; pathwise mean {vals.mean():.6f} +- {se:.6f} "
          f"({(vals.mean() - exact) / se:+.2f} standard errors); spread of one draw {vals.std(ddof=1):.4f}")
    assert abs(vals.mean() - exact) <= 4.0 * se
    assert np.all(vals <= -0.5 * B * np.log(2.0 * np.pi * float(p["s2"])))  # the quadratic part is >= 0 on every draw


def test_reference_elbo_without_rows_is_minus_kl_and_scales():
    kind = "se"
    p = small_problem(kind)
    draw = draw_of(kind, 2, 12, 8, 2, seed=1)
    args = [p[k] for k in ("variance", "ls", "s2", "Z")]
    tail = [p["pseudo_u"], p["counts"], p["probes"]]
    none = pw.elbo(kind, *args, p["x"][:0], p["y"][:0], *tail, draw, num_data=50)
    kl = -full.elbo(kind, *args, p["x"][:0], p["y"][:0], *tail)
    assert float(none) == float(-kl)
    a = pw.elbo(kind, *args, p["x"], p["y"], *tail, draw, num_data=None)
    b = pw.elbo(kind, *args, p["x"], p["y"], *tail, draw, num_data=70)
    assert abs(float(b + kl) - 10.0 * float(a + kl)) <= 1e-12 * abs(float(b))
    loss, grads = pw.loss_and_grads(kind, *args, p["x"], p["y"], *tail, draw, num_data=50)
    assert np.isfinite(loss) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


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


def test_batch_stays_the_default_and_pathwise_is_listed():
    assert models.DATA_TERMS == ("batch", "trace", "pathwise")
    assert make_trainable().data_term == "batch" and make_frozen().data_term == "batch"
    for cls in (training.TrainableCGGP, models.CGGP):
        par = inspect.signature(cls.__init__).parameters
        assert par["data_term"].default == "batch"
        assert (par["num_bases"].default, par["num_samples"].default, par["epsilon"].default) == (1024, 5, "matheron")
    assert inspect.signature(models.PathwiseClusterGP.__init__).parameters["epsilon"].default == "reference"
    par = inspect.signature(training.TrainableCGGP.elbo).parameters
    assert list(par)[1:] == ["data", "probes", "pathwise"] and par["pathwise"].default is None


@pytest.mark.parametrize("matrix_free", [False, True])
def test_the_keywords_are_kept_and_handed_on(matrix_free):
    kw = dict(data_term="pathwise", num_bases=64, num_samples=3, epsilon="reference")
    m = make_trainable(matrix_free=matrix_free, **kw)
    assert (m.data_term, m.num_bases, m.num_samples, m.epsilon, m.pathwise_seed) == ("pathwise", 64, 3, "reference", 0)
    frozen = m.frozen_model()
    assert (frozen.data_term, frozen.num_bases, frozen.num_samples, frozen.epsilon) == ("pathwise", 64, 3, "reference")
    assert frozen.matrix_free == matrix_free
    assert make_frozen(matrix_free=matrix_free, **kw).num_samples == 3
    from cggp import kernels
    Z = t(np.random.default_rng(1).uniform(-1.0, 1.0, (6, 2)))
    c = models.cdgp_class(kernels.SquaredExponential(1.0, [1.0, 1.0]), 0.3, Z, matrix_free=matrix_free, **kw)
    assert (c.data_term, c.num_bases, c.epsilon) == ("pathwise", 64, "reference")
    E, W, xi = m.draw_pathwise(5)
    assert E.shape == (64, 3) and W.shape == (3, 128) and xi.shape == (3, 10)


def test_what_the_pathwise_form_refuses():
    for make in (make_trainable, make_frozen):
        with pytest.raises(ValueError, match="data_term must be one of"):
            make(data_term="samples")
        with pytest.raises(ValueError, match="fp64 only"):
            make(dtype=torch.float32, data_term="pathwise")
        with pytest.raises(ValueError, match="fp64 only"):
            make(dtype=torch.float32, data_term="pathwise", matrix_free=True)
        with pytest.raises(ValueError, match="num_bases"):
            make(data_term="pathwise", num_bases=0)
        with pytest.raises(ValueError, match="num_samples"):
            make(data_term="pathwise", num_samples=0)
        with pytest.raises(ValueError, match="epsilon"):
            make(data_term="pathwise", epsilon="lambda")
    for matrix_free in (False, True):
        with pytest.raises(ValueError, match="D <= 32"):
            make_trainable(D=33, data_term="pathwise", trainable_inducing=True, matrix_free=matrix_free)
        assert make_trainable(D=33, data_term="pathwise", matrix_free=matrix_free).data_term == "pathwise"
        assert make_trainable(D=32, data_term="pathwise", trainable_inducing=True, matrix_free=matrix_free).Z.requires_grad
    data = (torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64))
    # the exact KL trace solves M right-hand sides: the matrix-free models refuse it before any device work
    with pytest.raises(ValueError, match="num_probes"):
        make_trainable(matrix_free=True, data_term="pathwise", num_probes=None).elbo(data)
    with pytest.raises(ValueError, match="num_probes"):
        make_frozen(matrix_free=True, data_term="pathwise", num_probes=None).elbo(data)
    # an injected draw of the wrong shape
    m = make_trainable(data_term="pathwise", num_bases=8, num_samples=2)
    E, W, xi = m.draw_pathwise(0)
    with pytest.raises(ValueError, match="pathwise="):
        m.elbo(data, pathwise=(E, W[:, :-1], xi))
    with pytest.raises(ValueError, match="pathwise="):
        m.elbo(data, pathwise=(E, W, xi[:, :-1]))
