"""Long-double restatement of the hyper-parameter bilinear forms of k(X, X) (`mgp_kxx_grad`), in the style of
gpr_reference.py: every ordered pair of rows, direct differences, GPflow's kernel profiles."""

import numpy as np

LD = np.longdouble


def _profile(name, r2):
    """f = k / variance and df/dr2 at the scaled squared distance (Matern-1/2: 0 below GPflow's 1e-36 floor)."""
    if name == "se":
        f = np.exp(LD(-0.5) * r2)
        return f, LD(-0.5) * f
    floor = ~(r2 > LD(1e-36))
    r = np.sqrt(np.where(floor, LD(1e-36), r2))
    if name == "matern12":
        f = np.exp(-r)
        return f, np.where(floor, LD(0), -f / (LD(2) * r))
    if name == "matern32":
        s3 = np.sqrt(LD(3))
        e = np.exp(-s3 * r)
        return (LD(1) + s3 * r) * e, np.where(floor, LD(0), LD(-1.5) * e)
    s5 = np.sqrt(LD(5))
    e = np.exp(-s5 * r)
    return (LD(1) + s5 * r + LD(5) / LD(3) * r2) * e, np.where(floor, LD(0), LD(-5) / LD(6) * (LD(1) + s5 * r) * e)


def kxx_grad_reference(name, variance, lengthscales, X, U, V, block=64, rows=None):
    """(dvariance, dlengthscales [D]) = sum_r u_r^T dK/dtheta v_r in long double, and the same sums of |terms| (the
    scale the tests measure rounding against).  U, V [N, R].  rows: the rows of U that are not all zero, when the
    caller knows them -- only their pairs (i, all j) are visited (the others contribute exact zeros)."""
    X = np.asarray(X, dtype=LD)
    U, V = np.asarray(U, dtype=LD), np.asarray(V, dtype=LD)
    ls = np.asarray(lengthscales, dtype=LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, X.shape[1])
    Xs = X / ls
    var = LD(variance)
    D = X.shape[1]
    dv, dl = LD(0), np.zeros(D, dtype=LD)
    sv, sl = LD(0), np.zeros(D, dtype=LD)
    if rows is None:
        rows = np.arange(X.shape[0])
    rows = np.asarray(rows, dtype=np.int64)
    outside = np.ones(X.shape[0], dtype=bool)
    outside[rows] = False
    assert not np.any(U[outside]), "rows must contain every nonzero row of U"
    for b0 in range(0, rows.shape[0], block):
        sel = rows[b0:b0 + block]
        diff = Xs[sel, None, :] - Xs[None, :, :]
        d2 = diff * diff
        r2 = d2.sum(axis=2)
        f, fp = _profile(name, r2)
        G = U[sel] @ V.T
        dv += np.sum(G * f)
        sv += np.sum(np.abs(G * f))
        w = (G * fp)[:, :, None] * d2 * (var * LD(-2) / ls)
        dl += w.sum(axis=(0, 1))
        sl += np.abs(w).sum(axis=(0, 1))
    return dv, dl, sv, sl
