"""Numpy restatements behind the pivoted-Cholesky preconditioner of matrix-free CDGP (`PivotedCholeskyPreconditioner`
on a `KmmLambdaOperator`, `MGP_PRE_LOWRANK_WIDE`): the CDGP-shaped system K_mm + Lambda with Lambda = s2 / cluster size,
P = L^T L + Lambda from the greedy factor of pivchol_reference.py, the step counts of its PCG, the scratch plan of the
many-column application (include/mgp.h) and one preconditioner application with its error scale."""

import numpy as np

from pivchol_reference import greedy_pivoted_cholesky, kernel_matrix, pcg, woodbury_factor

S2 = 0.1  # likelihood variance of the table inputs


def cdgp_inputs(M=2048, D=2, seed=0):
    """Z ~ U(-3, 3)^(M x D), cluster sizes uniform on 1 ... 64, lambda = 0.1 / size, b = sin(sum z) + 0.1 eps."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-3.0, 3.0, (M, D))
    counts = rng.integers(1, 65, M)
    lam = S2 / counts
    b = np.sin(Z.sum(axis=1)) + 0.1 * rng.standard_normal(M)
    return Z, lam, b


def system(kind, D, ls, M=2048):
    """(K_mm, lambda, b) of one row of the table."""
    Z, lam, b = cdgp_inputs(M, D)
    return kernel_matrix(kind, 1.0, [ls] * D, Z, dtype=np.float64), lam, b


def preconditioner(K, lam, rank):
    """(dinv, B, log|P|) of P = L^T L + diag(lam), L the greedy rank-`rank` factor of K."""
    L, _ = greedy_pivoted_cholesky(K, rank)
    B, log_det = woodbury_factor(L, lam)
    return 1.0 / lam, B, log_det


def steps(K, lam, b, rank=None, jacobi=False, threshold=1e-8):
    """CG steps on K + diag(lam): the identity, Jacobi, or the rank-`rank` preconditioner."""
    A = K + np.diag(lam)
    mv = lambda v: A @ v
    if rank is not None:
        dinv, B, _ = preconditioner(K, lam, rank)
        return pcg(mv, b, dinv=dinv, B=B, threshold=threshold)[1]
    if jacobi:
        return pcg(mv, b, dinv=1.0 / np.diag(A), threshold=threshold)[1]
    return pcg(mv, b, threshold=threshold)[1]


TABLE_CASES = (("se", 2, 1.5, (32, 64, 128)), ("se", 2, 0.5, (64, 128, 256)), ("matern32", 2, 1.5, (64, 128)),
               ("se", 8, 3.0, (64, 128, 256)))


def iteration_table(cases=TABLE_CASES, M=2048, threshold=1e-8):
    """{(kind, D, lengthscale): {"identity": steps, "jacobi": steps, rank: steps, ...}} on the inputs above."""
    out = {}
    for kind, D, ls, ranks in cases:
        K, lam, b = system(kind, D, ls, M)
        A = K + np.diag(lam)
        mv = lambda v: A @ v
        row = {"identity": pcg(mv, b, threshold=threshold)[1],
               "jacobi": pcg(mv, b, dinv=1.0 / np.diag(A), threshold=threshold)[1]}
        Lfull, _ = greedy_pivoted_cholesky(K, max(ranks))
        for k in ranks:
            Bk, _ = woodbury_factor(Lfull[:k], lam)
            row[k] = pcg(mv, b, dinv=1.0 / lam, B=Bk, threshold=threshold)[1]
        out[(kind, D, ls)] = row
    return out


def apply_reference(dinv, B, R):
    """(z, scale): z = dinv o R - (R B^T) B and the magnitude |dinv o R| + |R| |B^T| |B| its rounding error is relative
    to (the bar of tests/test_gpu_pivchol.py::test_lowrank_apply_against_numpy)."""
    z = dinv[None, :] * R - (R @ B.T) @ B
    return z, np.abs(dinv[None, :] * R) + (np.abs(R) @ np.abs(B).T) @ np.abs(B)


def narrow_arena_bytes(Bt, k, n):
    """Scratch of MGP_PRE_LOWRANK for one 16-column group (include/mgp.h, mgp_lowrank_apply)."""
    b = min(Bt, 16)
    bp = 1 if b == 1 else 2 if b == 2 else 4 if b <= 4 else 8 if b <= 8 else 16
    c = 2048 // bp
    return (-(-n // c) + 1) * b * k * 8


def wide_arena_bytes(Bt, k, n, cus):
    """Scratch of MGP_PRE_LOWRANK_WIDE (include/mgp.h): 8 (s + 1) b' k' bytes for the widest group."""
    need = 0
    for b in (min(Bt, 256), Bt % 256 if Bt > 256 else 0):
        if b <= 0:
            continue
        t = 32 if b <= 32 else 64 if b <= 64 else 128
        bp, kp = -(-b // t) * t, -(-k // 64) * 64
        tiles = (bp // t) * (kp // 64)
        s = max(1, min(-(-4 * cus // tiles), -(-n // 256)))
        cols = -(-(-(-n // s)) // 16) * 16
        s = -(-n // cols)
        need = max(need, 8 * (s + 1) * bp * kp)
    return need


if __name__ == "__main__":
    for key, row in iteration_table().items():
        print(key, row)
