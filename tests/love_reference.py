"""numpy restatement of the Lanczos variance cache (Pleiss et al. 2018), the yardstick of the `love` tests.

Kernel matrices as in `tests/gpr_reference.py` (`oracle.kernels.Kernel`, GPflow's expansion-form distance), Lanczos
with full re-orthogonalisation, and the Galerkin variance k** - p^T T^-1 p with p = Q k_X*.  Everything takes a
`dtype`, longdouble included, so the fp64 implementations can be measured against a more precise run of the same
recurrence.  Test support, not a restatement of a reference file.
"""

import numpy as np

from oracle import kernels as ok


def lanczos(A, start, steps, breakdown=1e-10, dtype=np.float64):
    """(Q [k, n], alpha [k], beta [k - 1]): k <= steps Lanczos steps on the symmetric matrix A from `start`, every new
    vector orthogonalised against all earlier ones (classical Gram-Schmidt, twice); stops early when the residual
    norm falls to breakdown * |alpha_0|."""
    A = np.asarray(A, dtype=dtype)
    v = np.asarray(start, dtype=dtype).reshape(-1)
    n = v.shape[0]
    steps = min(int(steps), n)
    Q = np.zeros((steps, n), dtype=dtype)
    alpha = np.zeros(steps, dtype=dtype)
    beta = np.zeros(steps, dtype=dtype)
    Q[0] = v / np.sqrt(v @ v)
    k = steps
    for j in range(steps):
        q = Q[j]
        w = A @ q
        alpha[j] = q @ w
        if j + 1 == steps:
            break
        w = w - alpha[j] * q
        if j > 0:
            w = w - beta[j - 1] * Q[j - 1]
        for _ in range(2):
            w = w - Q[:j + 1].T @ (Q[:j + 1] @ w)
        beta[j] = np.sqrt(w @ w)
        if beta[j] <= breakdown * abs(alpha[0]):
            k = j + 1
            break
        Q[j + 1] = w / beta[j]
    return Q[:k], alpha[:k], beta[:k - 1]


def tridiagonal(alpha, beta):
    return np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)


def cholesky(T):
    """Lower Cholesky factor in T's dtype (numpy.linalg has no longdouble)."""
    n = T.shape[0]
    C = np.zeros_like(T)
    for j in range(n):
        d = T[j, j] - C[j, :j] @ C[j, :j]
        C[j, j] = np.sqrt(d)
        C[j + 1:, j] = (T[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    return C


def forward_solve(C, B):
    """C^-1 B for lower-triangular C, in C's dtype."""
    X = np.array(B, dtype=C.dtype, copy=True)
    for i in range(C.shape[0]):
        X[i] = (X[i] - C[i, :i] @ X[:i]) / C[i, i]
    return X


def projector(Q, alpha, beta):
    """R = Q^T C^-T [n, k] with tridiag(beta, alpha, beta) = C C^T."""
    C = cholesky(tridiagonal(alpha, beta))
    return forward_solve(C, Q).T


def galerkin(kind, variance, lengthscales, X, Xs, R, dtype=np.float64):
    """(variance [B], covariance [B, B]) of the cache: k** - |k(x*, X) R|^2 and k(X*, X*) - proj proj^T."""
    kern = ok.Kernel(kind, variance, lengthscales, dtype=dtype)
    proj = kern.K(np.asarray(Xs, dtype=dtype), np.asarray(X, dtype=dtype)) @ np.asarray(R, dtype=dtype)
    var = kern.K_diag(Xs) - np.sum(proj * proj, axis=1)
    cov = kern.K(np.asarray(Xs, dtype=dtype)) - proj @ proj.T
    return var, cov


def knm_project(kind, variance, lengthscales, Xs, X, R, dtype=np.longdouble):
    """(proj [B, r], sqnorm [B]) = (k(Xs, X) R, row square sums), evaluated in `dtype`."""
    kern = ok.Kernel(kind, variance, lengthscales, dtype=dtype)
    proj = kern.K(np.asarray(Xs, dtype=dtype), np.asarray(X, dtype=dtype)) @ np.asarray(R, dtype=dtype)
    return proj, np.sum(proj * proj, axis=1)


def exact_variance(kind, variance, lengthscales, X, s2, Xs, dtype=np.float64):
    """(variance [B], covariance [B, B], cond(K + s2 I)) by Cholesky, in `dtype`."""
    kern = ok.Kernel(kind, variance, lengthscales, dtype=dtype)
    X = np.asarray(X, dtype=dtype)
    Xs = np.asarray(Xs, dtype=dtype)
    Khat = kern.K(X) + dtype(s2) * np.eye(X.shape[0], dtype=dtype)
    L = cholesky(Khat) if dtype is np.longdouble else np.linalg.cholesky(Khat)
    A = forward_solve(L, kern.K(X, Xs)) if dtype is np.longdouble else np.linalg.solve(L, kern.K(X, Xs))
    ev = np.linalg.eigvalsh(Khat.astype(np.float64))
    return kern.K_diag(Xs) - np.sum(A * A, axis=0), kern.K(Xs) - A.T @ A, float(ev[-1] / ev[0])
