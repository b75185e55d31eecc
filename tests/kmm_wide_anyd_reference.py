"""Long-double reference of out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda) and the bound include/mgp_sweep_anyd.h
states for MGP_OP_KMM_LAMBDA_WIDE_ANYD (checked on the CPU by tests/test_kmm_wide_anyd_plan.py, applied on the GPU by
tests/test_gpu_kmm_wide_anyd.py):

    |out[b, j] - exact| <= sum_i |P[b, i]| pairbound(i, j) + u (terms + nsplit + 3) sum_i |P[b, i] K[i, j]|
                           + 2 u |lambda_j P[b, j]|

pairbound(i, j) = K*[i, j] `pair_reference.pair_bound` (the bound of the expansion-form distance through the profile:
the chain of csrc/kmm_wide_anyd.hip is that of csrc/sweep_anyd.hip, `sweep_anyd_plan.emulate_neg_s`); terms = the
streamed rows of one split (one product per row accumulated on the matrix cores, padding rows included); nsplit for
the sum of the splits' tiles; 3 = the product with the variance, the product lambda_j P[b, j] and the last sum.  No
constant is fitted."""

import numpy as np

import kmm_wide_anyd_plan as wp
import pair_reference as pr

LD = np.longdouble
F64 = np.float64
U = 2.0 ** -53
VARIANCE = pr.VARIANCE


def inputs(D, M, seed=0):
    """(Z [M, D], lengthscales [D], lambda [M] in [0.5, 1.5)): a standard normal cloud, the lengthscales stretched by
    sqrt(D) so that r^2 is about 2 at every D (kernel values of order 1/e, |a|^2 of order D/D = 1 per unit of c^2)."""
    rng = np.random.default_rng([seed, D, 17])
    Z = rng.standard_normal((M, D))
    return Z, pr.lengthscales(D) * np.sqrt(D), 0.5 + np.random.default_rng([seed, D, 18]).random(M)


def kernel_columns(name, ls, Z, cols=None):
    """(K* [M, C] in long double, pairbound [M, C] absolute) for the columns `cols` of k(Z, Z) (all when None)."""
    D = Z.shape[1]
    Zc = Z if cols is None else Z[np.asarray(cols, dtype=np.int64)]
    pv = pr.pair_values(name, VARIANCE, ls, Z, Zc, block=32)
    a = pr.scaled(name, ls, Z)
    rel = pr.pair_bound(name, VARIANCE, pv.s, pv.q, a, pr.scaled(name, ls, Zc), D, F64)
    return pv, rel


def product(K, lam, P):
    """P (K + diag lam) in long double; K [M, M] long double."""
    Pl = np.asarray(P, dtype=F64).astype(LD)
    return Pl @ K + Pl * np.asarray(lam, dtype=F64).astype(LD)


def product_bound(K, pairbound, lam, P, M, num_cus):
    """The header's bound for every element of out [Bt, M]."""
    _, nsplit, rows = wp.split_plan(M, num_cus)
    Pa = np.abs(np.asarray(P, dtype=F64)).astype(LD)
    chain = U * (rows + nsplit + 3)
    return Pa @ pairbound.astype(LD) + chain * (Pa @ np.abs(K)) + 2 * U * Pa * np.abs(np.asarray(lam, dtype=F64))


def operator_eps(name, ls, Z, num_cus):
    """A relative bound of one product, for the oracle's perturbed-operator check: the largest pair bound plus the chain."""
    _, rel = kernel_columns(name, ls, Z)
    _, nsplit, rows = wp.split_plan(Z.shape[0], num_cus)
    return float(rel.max()) + U * (rows + nsplit + 3)


def cg_trace(A, rhs, steps, min_float=1e-16):
    """(denominators, rz) [steps, Bt] of oracle/cg.py's recurrence on the float64 matrix A from a zero start, identity
    preconditioner, no residual refresh: what its two breakdown guards compare with `min_float`."""
    b = np.asarray(rhs, dtype=F64)
    v, r = np.zeros_like(b), b.copy()
    rz = np.sum(r * r, axis=-1, keepdims=True)
    p = r
    den, rzs = [], []
    for _ in range(steps):
        pA = p @ A
        d = np.sum(p * pA, axis=-1, keepdims=True)
        den.append(d[:, 0].copy())
        rzs.append(rz[:, 0].copy())
        with np.errstate(divide="ignore", invalid="ignore"):
            gamma = np.where(d <= min_float, 0.0, rz / d)
        v = v + gamma * p
        r = r - gamma * pA
        new_rz = np.sum(r * r, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = r + np.where(rz <= min_float, 0.0, p * new_rz / rz)
        rz = new_rz
    return np.array(den), np.array(rzs)
