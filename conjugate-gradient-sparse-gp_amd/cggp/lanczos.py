"""Lanczos tridiagonalisation with full re-orthogonalisation.

`k` steps on a symmetric operator A from a start vector give an orthonormal Q [k, n] and a tridiagonal
T = Q A Q^T (diagonal `alpha`, off-diagonal `beta`): the Galerkin basis of a `models.LanczosVarianceCache`
(Pleiss et al. 2018).  One operator application per step (`mgp_operator_apply` for a `LinearOperator`); the new vector
is orthogonalised against every earlier one by two classical Gram-Schmidt passes (two torch GEMVs each, 2 j n elements
per pass -- small beside the operator), which keeps |Q Q^T - I| at rounding level where the three-term recurrence alone
loses it after a few dozen steps.
"""

import torch

from .conjugate_gradient import LinearOperator


def _apply(operator, q):
    """A q for q [n]: a `LinearOperator`, a symmetric matrix, or a callable q -> A q."""
    if isinstance(operator, LinearOperator):
        return operator.rmatmul(q[None, :])[0]
    if isinstance(operator, torch.Tensor):
        return operator @ q
    return operator(q)


def lanczos(operator, start, steps, breakdown=1e-10):
    """(Q [k, n], alpha [k], beta [k - 1]) with k <= steps, Q Q^T = I_k and Q A Q^T = tridiag(beta, alpha, beta).

    `operator`: a `conjugate_gradient.LinearOperator` (GPU), a symmetric torch matrix, or a callable v [n] -> A v (any
    device, so the recurrence can be checked on the CPU).  `start` [n] need not be normalised.  The recurrence stops
    early, with k < steps rows, when the norm beta_j of the re-orthogonalised residual falls to `breakdown * |alpha_0|`
    or below: the Krylov space is then invariant to that accuracy and a further vector would be rounding noise."""
    start = start.reshape(-1)
    n = start.shape[0]
    steps = min(int(steps), n)
    if steps < 1:
        raise ValueError("lanczos needs steps >= 1 and a non-empty start vector")
    norm = torch.linalg.vector_norm(start)
    if not float(norm) > 0.0:
        raise ValueError("the start vector is zero")
    Q = torch.zeros((steps, n), dtype=start.dtype, device=start.device)
    alpha = torch.zeros((steps,), dtype=start.dtype, device=start.device)
    beta = torch.zeros((steps,), dtype=start.dtype, device=start.device)
    Q[0] = start / norm
    k = steps
    for j in range(steps):
        q = Q[j]
        w = _apply(operator, q).reshape(-1)
        a = torch.dot(q, w)
        alpha[j] = a
        if j + 1 == steps:
            break
        w = w - a * q
        if j > 0:
            w = w - beta[j - 1] * Q[j - 1]
        basis = Q[:j + 1]
        for _ in range(2):  # classical Gram-Schmidt, twice
            w = w - basis.t() @ (basis @ w)
        b = torch.linalg.vector_norm(w)
        beta[j] = b
        if float(b) <= breakdown * abs(float(alpha[0])):
            k = j + 1
            break
        Q[j + 1] = w / b
    return Q[:k], alpha[:k], beta[:k - 1]
