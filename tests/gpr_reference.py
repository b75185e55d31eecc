"""numpy restatement of exact GP regression (GPflow `GPR`: Cholesky of K + s2 I), the yardstick of the GPR tests.

Kernel values come from `oracle.kernels.Kernel` (GPflow's expansion-form square distance).  Kept under tests/, not
oracle/: it is test support for the `cggp.models.GPR` model, not a restatement of a reference file.
"""

import numpy as np

from oracle import kernels as ok


def kxx_product(name, variance, lengthscales, X, s2, V, dtype=np.longdouble):
    """(k(X, X) + s2 I) V evaluated in `dtype` (longdouble by default)."""
    kern = ok.Kernel(name, variance, lengthscales, dtype=dtype)
    X = np.asarray(X, dtype=dtype)
    V = np.asarray(V, dtype=dtype)
    return kern.K(X) @ V + dtype(s2) * V


def gpr_posterior(name, variance, lengthscales, X, Y, s2, Xs):
    """mean [B, 1], variance [B, 1], covariance [B, B] and log marginal likelihood, all fp64."""
    kern = ok.Kernel(name, variance, lengthscales)
    K = kern.K(X) + s2 * np.eye(X.shape[0])
    L = np.linalg.cholesky(K)
    Kxs = kern.K(X, Xs)
    A = np.linalg.solve(L, Kxs)
    v = np.linalg.solve(L, Y)
    mean = A.T @ v
    cov = kern.K(Xs) - A.T @ A
    var = np.full(Xs.shape[0], float(variance)) - np.sum(A * A, axis=0)
    N = X.shape[0]
    lml = -0.5 * N * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(L))) - 0.5 * float(np.sum(v * v))
    return mean, var[:, None], cov, lml
