"""The quadratic form of mgp_knm_quadform (include/mgp_predict.h) in long double, the bound a device result is held
to, and the SGPR variance matrix of `cggp.models.SGPR.variance_matrix` in numpy (tests/test_quadform_reference.py on the
CPU, tests/test_gpu_quadform.py and tests/test_gpu_predict_batched.py on the GPU).

    q[b] = sum_i C_ii k_bi^2 + 2 sum_{i<j} C_ij k_bi k_bj,   k_bi = k(xs_b, z_i)  (`pair_reference.pair_values`)

`prefix_forms` returns q for EVERY leading M' x M' block of C at once: with W[b, j] = sum_{i<j} C_ij k_bi (the strict
upper triangle, one long-double product), q_M'[b] = sum_{j<M'} (2 W[b, j] + C_jj k_bj) k_bj, and W[b, j] does not
depend on M' > j.  The same for the magnitude |k|^T |C_upper form| |k| the bound is relative to.

The bound.  Let k~ = k (1 + d), |d_bi| <= eps_b (the per-pair bound of `pair_reference.pair_bound` for the expansion-form
distance and the base-2 profiles, maximised over the row's pairs) be the values a kernel works with, and
mag_b = sum_i |C_ii| k_bi^2 + 2 sum_{i<j} |C_ij| k_bi k_bj.
  Values.  Every term holds two kernel values: |k~_i k~_j - k_i k_j| <= 2 eps_b k_i k_j to first order, 2 eps_b mag_b in all.
  Sum.  The fused kernel adds term (i, j) into the accumulator of column j at walk step i (one fused multiply-add: the
  product is not rounded on its own), so it is rounded once per later step of that column, at most j - i <= M - 1
  times; the doubling is exact; C_jj k_j joins by one fma and the product with k_j by another; the generic route is a
  GEMM (any order over M terms, M - 1 roundings) and a row dot of M terms.  The first-order bound of a sum whose terms
  pass through at most n roundings is n u times the sum of their magnitudes; with n = M + 4 -- the M - 1 of the longest
  chain, the two fmas, the variance (the scale variance^2 on the fused route) and two to spare --
        |q - q*| <= (2 eps_b + (M + 4) u) mag_b.
  What n = M + 4 leaves out, stated plainly: the fused kernel adds the finished 16-column tiles of a row into one
  number over up to 4 tiles per wave, 4 shuffle steps, the two column waves and the nJ = ceil(M / 128) blocks, so the
  terms with j - i > M - (8 + nJ) -- a corner of the triangle -- pass through up to M + 10 + nJ roundings; a first-order
  worst case that charges every term its own count exceeds the bound by at most (6 + nJ) u on those terms alone.  The
  bound is applied as stated; every test prints the worst err / bound it saw.
"""

import numpy as np

import pair_reference as pr

LD = np.longdouble


def upper_form(C):
    """(diagonal, strict upper triangle) of C in long double: all that defines the form."""
    C = np.asarray(C).astype(LD)
    return np.diag(C).copy(), np.triu(C, 1)


def prefix_forms(k, C):
    """(Q, MAG) [B, M]: Q[b, m] = the form of the leading (m + 1) x (m + 1) block of C on the first m + 1 kernel values
    of row b, MAG the same with absolute values.  k [B, M] long double (signed values allowed)."""
    k = np.asarray(k).astype(LD)
    d, U = upper_form(C)
    W = k @ U
    Q = np.cumsum((LD(2) * W + d[None, :] * k) * k, axis=1)
    ka = np.abs(k)
    Wa = ka @ np.abs(U)
    MAG = np.cumsum((LD(2) * Wa + np.abs(d)[None, :] * ka) * ka, axis=1)
    return Q, MAG


def form(k, C):
    """(q, mag) [B] for the whole of C."""
    Q, MAG = prefix_forms(k, C)
    if Q.shape[1] == 0:
        return np.zeros(Q.shape[0], dtype=LD), np.zeros(Q.shape[0], dtype=LD)
    return Q[:, -1], MAG[:, -1]


def symmetric_form(k, C):
    """k^T sym(C) k with sym(C) the symmetric matrix of the upper triangle, written out independently of `form`."""
    C = np.asarray(C).astype(LD)
    S = np.triu(C) + np.triu(C, 1).T
    k = np.asarray(k).astype(LD)
    return np.einsum("bi,bi->b", k @ S, k)


def row_eps(name, variance, ls, Xs, Z, pv, dtype):
    """eps_b [B]: `pair_bound` maximised over the pairs of a row."""
    D = np.asarray(Xs).shape[1]
    rel = pr.pair_bound(name, variance, pv.s, pv.q, pr.scaled(name, ls, Xs), pr.scaled(name, ls, Z), D, dtype)
    return np.maximum.accumulate(np.asarray(rel, dtype=np.float64), axis=1)  # [B, M]: the maximum over the first m + 1 pairs


def bound(eps, M, mag, dtype):
    """(2 eps + (M + 4) u) mag."""
    return (2.0 * np.asarray(eps, dtype=np.float64) + (M + 4) * pr.unit_roundoff(dtype)) * np.asarray(mag, dtype=np.float64)


# ---------------------------------------------------------------- the SGPR variance matrix
def sgpr_variance_matrix(X, Z, kernel, noise_variance, jitter):
    """C = (Kmm + jitter I)^-1 - s2 S^-1 with S = s2 (Kmm + jitter I) + K_mn K_nm, by the route of
    `cggp.models.SGPR.variance_matrix` (no subtraction): C = L^-T (B^-1 AAT) L^-1.  kernel: `oracle.kernels.Kernel`."""
    from scipy.linalg import cho_solve, solve_triangular
    from oracle.kernels import Kuf, Kuu
    Kmn = Kuf(Z, kernel, X)
    KK = Kmn @ Kmn.T
    L = np.linalg.cholesky(Kuu(Z, kernel, jitter=jitter))
    # the statements of the model, one for one (triangular solves, not LU)
    T1 = solve_triangular(L, KK, lower=True)
    AAT = solve_triangular(L, T1.T, lower=True) / noise_variance
    AAT = 0.5 * (AAT + AAT.T)
    B = AAT + np.eye(AAT.shape[0])
    G = cho_solve((np.linalg.cholesky(B), True), AAT)
    G = 0.5 * (G + G.T)
    T2 = solve_triangular(L.T, G, lower=False)
    C = solve_triangular(L.T, T2.T, lower=False)
    return 0.5 * (C + C.T)


def sgpr_variance_matrix_subtractive(X, Z, kernel, noise_variance, jitter):
    """The same matrix as the difference of two inverses: what `sgpr_variance_matrix` avoids."""
    from oracle.kernels import Kuf, Kuu
    Kmn = Kuf(Z, kernel, X)
    Kmm = Kuu(Z, kernel, jitter=jitter)
    S = noise_variance * Kmm + Kmn @ Kmn.T
    return np.linalg.inv(Kmm) - noise_variance * np.linalg.inv(S)
