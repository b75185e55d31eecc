"""Numpy / long-double restatements behind the pivoted-Cholesky preconditioner (`mgp_kxx_pivchol`, `MGP_PRE_LOWRANK`),
in the style of lml_reference.py: the kernel matrix from direct differences and GPflow's profiles, a dense pivoted
Cholesky with a FORCED pivot order, a numpy PCG with this project's recurrence and stopping rule that also returns
(gamma, beta, 1/2 rz) per step, and the experiment behind the iteration-count table of DESIGN 4.13."""

import numpy as np

from lml_reference import _profile

LD = np.longdouble


def kernel_matrix(name, variance, lengthscales, X, dtype=LD, block=256):
    """K = k(X, X) [N, N] in `dtype`."""
    X = np.asarray(X, dtype=dtype)
    ls = np.asarray(lengthscales, dtype=dtype).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, X.shape[1])
    Xs = X / ls
    N = X.shape[0]
    K = np.empty((N, N), dtype=dtype)
    for i0 in range(0, N, block):
        diff = Xs[i0:i0 + block, None, :] - Xs[None, :, :]
        r2 = (diff * diff).sum(axis=2)
        K[i0:i0 + block] = dtype(variance) * _profile(name, r2.astype(LD))[0].astype(dtype)
    return K


def kernel_rows(name, variance, lengthscales, X, rows, dtype=LD):
    """k(X[rows], X) [len(rows), N] in `dtype` (what a forced-pivot factor needs of K at large N)."""
    X = np.asarray(X, dtype=dtype)
    ls = np.asarray(lengthscales, dtype=dtype).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, X.shape[1])
    Xs = X / ls
    diff = Xs[np.asarray(rows), None, :] - Xs[None, :, :]
    r2 = (diff * diff).sum(axis=2)
    return dtype(variance) * _profile(name, r2.astype(LD))[0].astype(dtype)


def forced_pivoted_cholesky(row_of, diag0, pivots):
    """Partial Cholesky with the given pivot order.  `row_of(p)` returns row p of K (any float dtype), `diag0` its
    diagonal.  Returns (L [k, N], residual diagonals BEFORE each step [k, N], final residual diagonal [N]); entries of
    L at earlier pivots and the pivot's own residual are set to exactly 0, as the device does."""
    d = np.array(diag0, copy=True)
    N = d.shape[0]
    k = len(pivots)
    L = np.zeros((k, N), dtype=d.dtype)
    before = np.zeros((k, N), dtype=d.dtype)
    for i, p in enumerate(pivots):
        before[i] = d
        row = np.array(row_of(p), dtype=d.dtype)
        row = row - L[:i, p] @ L[:i]
        L[i] = row / np.sqrt(d[p])
        L[i, list(pivots[:i])] = 0
        L[i, p] = np.sqrt(d[p])
        d = d - L[i] * L[i]
        d[p] = 0
    return L, before, d


def greedy_pivoted_cholesky(K, max_rank, rel_tol=0.0):
    """The algorithm itself on a dense K (float64 or long double): argmax pivots (lowest index on ties), stop when the
    trace of the residual is <= rel_tol * N * K[0, 0] or no positive pivot is left.  Returns (L [rank, N], pivots)."""
    K = np.asarray(K)
    N = K.shape[0]
    d = np.array(np.diag(K), copy=True)
    var = d[0] if N else 0
    L = np.zeros((min(max_rank, N), N), dtype=K.dtype)
    piv = []
    for i in range(L.shape[0]):
        p = int(np.argmax(d))
        if d.sum() <= rel_tol * N * var or d[p] <= 0:
            break
        row = K[p] - L[:i, p] @ L[:i]
        L[i] = row / np.sqrt(d[p])
        L[i, piv] = 0
        L[i, p] = np.sqrt(d[p])
        d = np.maximum(d - L[i] * L[i], 0)
        d[p] = 0
        piv.append(p)
    return L[:len(piv)], piv


def woodbury_factor(L, D):
    """B [k, n] and log|P| for P = diag(D) + L^T L: P^-1 = diag(1/D) - B^T B, B = C^-1 L D^-1, C C^T = I + L D^-1 L^T."""
    L = np.asarray(L, dtype=np.float64)
    D = np.broadcast_to(np.asarray(D, dtype=np.float64), (L.shape[1],))
    LD_ = L / D[None, :]
    C = np.linalg.cholesky(np.eye(L.shape[0]) + LD_ @ L.T)
    B = np.linalg.solve(C, LD_)
    return B, 2.0 * np.log(np.diag(C)).sum() + np.log(D).sum()


def pcg(matvec, b, dinv=None, B=None, threshold=1e-8, max_iterations=None, min_float=1e-16, max_steps_cycle=None):
    """This project's CG (csrc/cg.hip, the reference's cggp/conjugate_gradient.py:59-98) for one right-hand side from
    x0 = 0 with z = dinv * r - B^T (B r) (identity when both are None): stop when 1/2 |r|^2 <= threshold or after
    max_iterations; gamma = 0 where p.Ap <= min_float; the beta term is dropped where rz <= min_float; residual refresh
    and direction restart at step i when i % max_steps_cycle == max_steps_cycle - 1.
    Returns (x, steps, coef [steps, 3] = (gamma, beta, 1/2 rz after the step))."""
    n = b.shape[0]
    max_iterations = n if max_iterations is None else max_iterations
    cycle = max_iterations + 1 if max_steps_cycle is None else max_steps_cycle

    def pre(r):
        if dinv is None and B is None:
            return r
        z = r * dinv if dinv is not None else r.copy()
        return z - B.T @ (B @ r) if B is not None else z

    x = np.zeros(n)
    r = b.astype(np.float64).copy()
    z = pre(r)
    p = z.copy()
    rz = r @ z
    coef = []
    i = 0
    while 0.5 * (r @ r) > threshold and i < max_iterations:
        Ap = matvec(p)
        den = p @ Ap
        gamma = 0.0 if den <= min_float else rz / den
        x = x + gamma * p
        reset = i % cycle == cycle - 1
        r = b - matvec(x) if reset else r - gamma * Ap
        z = pre(r)
        rz_new = r @ z
        if reset:
            beta = 0.0
            p = z.copy()
        elif rz <= min_float:
            beta = 0.0
            p = z.copy()
        else:
            beta = rz_new / rz
            p = z + beta * p
        coef.append((gamma, beta, 0.5 * rz_new))
        rz = rz_new
        i += 1
    return x, i, np.array(coef).reshape(-1, 3)


def table_inputs(N, D, seed=0):
    """Inputs of the iteration-count table: X ~ U(-3, 3)^(N x D), y = sin(sum x) + 0.1 eps."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (N, D))
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    return X, y


def iteration_table(N=8192, s2=0.1, threshold=1e-8, cases=((2, 1.5, (32, 64, 128)), (8, 3.0, (64, 128, 256)),
                                                            (8, 1.5, (32, 64, 128, 256)))):
    """CG steps of the identity and of rank-k pivoted-Cholesky preconditioners on K + s2 I (SE kernel, float64):
    {(D, lengthscale): {"identity": steps, rank: steps, ...}}."""
    out = {}
    for D, ls, ranks in cases:
        X, y = table_inputs(N, D)
        K = kernel_matrix("se", 1.0, [ls] * D, X, dtype=np.float64)
        A = K + s2 * np.eye(N)
        mv = lambda v: A @ v
        row = {"identity": pcg(mv, y, threshold=threshold)[1]}
        Lfull, _ = greedy_pivoted_cholesky(K, max(ranks))
        for k in ranks:
            Bk, _ = woodbury_factor(Lfull[:k], s2)
            row[k] = pcg(mv, y, dinv=np.full(N, 1.0 / s2), B=Bk, threshold=threshold)[1]
        out[(D, ls)] = row
    return out


if __name__ == "__main__":
    for key, row in iteration_table().items():
        print(key, row)
