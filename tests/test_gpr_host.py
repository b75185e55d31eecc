"""Exact GP regression, host side: the numpy restatement the GPU tests measure against (checked here against
scikit-learn), and the argument checks of the new product / operator that need no device."""

import ctypes

import numpy as np
import pytest
import torch

from gpr_reference import gpr_posterior, kxx_product
from oracle import kernels as ok


@pytest.mark.parametrize("kind,nu", [("se", None), ("matern12", 0.5), ("matern32", 1.5), ("matern52", 2.5)])
def test_numpy_gpr_against_sklearn(kind, nu):
    gp = pytest.importorskip("sklearn.gaussian_process")
    kr = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(0)
    X = rng.uniform(-2, 2, (300, 2))
    Y = np.sin(X.sum(axis=1, keepdims=True)) + 0.1 * rng.standard_normal((300, 1))
    Xs = rng.uniform(-2, 2, (40, 2))
    ls, var, s2 = np.array([0.7, 1.3]), 1.4, 0.05
    base = kr.RBF(ls) if nu is None else kr.Matern(ls, nu=nu)
    sk = gp.GaussianProcessRegressor(kr.ConstantKernel(var) * base, alpha=s2, optimizer=None).fit(X, Y)
    mu0, cov0 = sk.predict(Xs, return_cov=True)
    mean, v, cov, lml = gpr_posterior(kind, var, ls, X, Y, s2, Xs)
    # scikit-learn forms distances directly (scipy cdist), GPflow by the expansion |a|^2 + |b|^2 - 2 a.b: the two
    # differ by ~1e-16 |x|^2 / r in r, which the Matern-1/2 profile passes on at short range
    assert np.max(np.abs(mean[:, 0] - np.ravel(mu0))) < 1e-7 * np.max(np.abs(mu0))
    assert np.max(np.abs(cov - np.squeeze(cov0))) < 1e-7 * np.max(np.abs(cov0))
    assert np.max(np.abs(v[:, 0] - np.diag(cov))) < 1e-7  # k(x, x) through sqrt(max(r2, 1e-36)) for Matern-1/2
    assert abs(lml - sk.log_marginal_likelihood_value_) < 1e-7 * abs(lml)


def test_kxx_product_restatement():
    rng = np.random.default_rng(1)
    X, V = rng.standard_normal((50, 3)), rng.standard_normal((50, 2))
    ls = np.array([0.5, 1.0, 2.0])
    K = ok.Kernel("matern32", 1.1, ls).K(X)
    ref = K @ V + 0.3 * V
    assert np.max(np.abs(np.asarray(kxx_product("matern32", 1.1, ls, X, 0.3, V), dtype=np.float64) - ref)) < 1e-12


def test_kxx_entry_point_is_bound():
    from cggp import _hip, ops
    from cggp.conjugate_gradient import KxxNoiseOperator
    assert _hip.SIGNATURES["mgp_kxx_matvec"][1][4] is ctypes.c_double  # s2 is a double, after N
    assert _hip.OP_KXX_NOISE == 3
    assert callable(ops.kxx_matvec) and issubclass(KxxNoiseOperator, object)


def test_kxx_null_handle_is_an_error():
    from cggp import _hip
    lib = _hip.load_library()
    k = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    assert lib.mgp_kxx_matvec(None, ctypes.byref(k), None, 4, 0.1, None, 1, 0, None, 0) == -1  # MGP_E_BADARG


def test_kxx_operator_and_product_need_device_tensors():
    from cggp import kernels, ops
    from cggp.conjugate_gradient import KxxNoiseOperator
    k = kernels.SquaredExponential(1.0, [1.0, 1.0])
    X = torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU|CPU fallback"):
        KxxNoiseOperator(k, X, 0.1)
    with pytest.raises(RuntimeError, match="GPU|CPU fallback"):
        ops.kxx_matvec(k.spec(2), X, 0.1, torch.zeros((4, 1), dtype=torch.float64))


def test_gpr_model_argument_checks():
    from cggp import kernels, models
    X, Y = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64)
    k = kernels.SquaredExponential(1.0, [1.0, 1.0])
    with pytest.raises(ValueError, match="solver"):
        models.GPR((X, Y), k, solver="lu")
    with pytest.raises(ValueError, match="data"):
        models.GPR((X, Y[:3]), k)
    m = models.GPR((X, Y), k, noise_variance=0.2, cholesky_max_n=2)
    assert not m.uses_cholesky() and m.likelihood.variance == 0.2
    with pytest.raises(NotImplementedError, match="log"):
        m.log_marginal_likelihood()
    from cggp import cli_utils
    assert cli_utils.gpr_class is models.gpr_class and cli_utils.create_gpr_model is models.create_gpr_model
