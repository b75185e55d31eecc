"""Stochastic Lanczos quadrature from recorded CG coefficients (host only: numpy, no GPU).

CG from x0 = 0 on an SPD matrix A with right-hand side z is the Lanczos process started at z / |z|: with the step
lengths gamma_k and direction ratios beta_k = rz_{k+1} / rz_k of the solve (what `ops.pcg_solve_record` records), the
Lanczos tridiagonal of the first m steps is (Golub & Van Loan 10.2; the mBCG scheme of Gardner et al. 2018)

    T[0, 0]   = 1 / gamma_0
    T[k, k]   = 1 / gamma_k + beta_{k-1} / gamma_{k-1}
    T[k-1, k] = sqrt(beta_{k-1}) / gamma_{k-1}

and Gauss quadrature gives  z^T f(A) z  ~=  |z|^2 e1^T f(T) e1.  With Rademacher probes (E[z z^T] = I) the mean over
probes of z^T log(A) z estimates log|A|.  T does not depend on the scale of z, so the solve may run on normalised
columns and |z|^2 taken from the original probe.

Preconditioned CG (preconditioner P, `MGP_PRE_LOWRANK`) is the same process on P^-1/2 A P^-1/2 started at P^-1/2 z:
with gamma_k and beta_k = (r.z)_{k+1} / (r.z)_k of that solve the formulas above hold unchanged, the quadrature is
z^T P^-1/2 f(P^-1/2 A P^-1/2) P^-1/2 z  ~=  (z^T P^-1 z) e1^T f(T) e1, and with probes drawn so that E[z z^T] = P the
mean of the log-quadratures estimates log|A| - log|P|.  `norms2` is then the weight z^T P^-1 z of each column.
"""

import numpy as np


def usable_steps(gamma, beta, half_rz, threshold=0.0, min_float=1e-16):
    """Steps of one column that enter T: up to and including the step at which the column itself converged
    (0.5 rz <= threshold), or the step whose beta-term was dropped (rz <= min_float); a step with gamma = 0 (p.Ap
    <= min_float, breakdown) and everything after it is left out, as is anything past the record's end."""
    gamma, beta, half_rz = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (gamma, beta, half_rz))
    m = 0
    for k in range(gamma.shape[0]):
        if not (gamma[k] > 0.0) or not np.isfinite(gamma[k]):
            break
        m = k + 1
        if half_rz[k] <= threshold or 2.0 * half_rz[k] <= min_float or not (beta[k] > 0.0):
            break
    return m


def lanczos_tridiagonal(gamma, beta):
    """T [m, m] from m step lengths and (at least) m - 1 direction ratios."""
    gamma = np.asarray(gamma, dtype=np.float64).reshape(-1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    m = gamma.shape[0]
    T = np.zeros((m, m))
    if m == 0:
        return T
    T[0, 0] = 1.0 / gamma[0]
    for k in range(1, m):
        T[k, k] = 1.0 / gamma[k] + beta[k - 1] / gamma[k - 1]
        T[k - 1, k] = T[k, k - 1] = np.sqrt(beta[k - 1]) / gamma[k - 1]
    return T


def quadratic_log(T, norm2):
    """|z|^2 e1^T log(T) e1 through the eigen-decomposition of T (Gauss quadrature nodes and weights)."""
    if T.shape[0] == 0:
        return 0.0
    lam, Q = np.linalg.eigh(T)
    return float(norm2) * float(np.sum(Q[0, :] ** 2 * np.log(lam)))


def slq_log_quadratic(coef, norms2, threshold=0.0, min_float=1e-16):
    """Per column b of a recorded solve: |z_b|^2 e1^T log(T_b) e1 ~= z_b^T log(A) z_b.

    coef [steps, B, 3] = (gamma, beta, 0.5 rz after the step) as `ops.pcg_solve_record` returns it (any array-like);
    norms2 [B] = |z_b|^2 of the original columns; `threshold` the per-column 0.5 rz at which a column counts as
    converged (in the units of the solve's columns).  Returns (values [B], steps used [B])."""
    c = np.asarray(coef, dtype=np.float64)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError(f"coef must be [steps, B, 3], got {c.shape}")
    norms2 = np.asarray(norms2, dtype=np.float64).reshape(-1)
    if norms2.shape[0] != c.shape[1]:
        raise ValueError(f"{norms2.shape[0]} norms for {c.shape[1]} columns")
    vals = np.zeros(c.shape[1])
    used = np.zeros(c.shape[1], dtype=np.int64)
    for b in range(c.shape[1]):
        g, bt, hr = c[:, b, 0], c[:, b, 1], c[:, b, 2]
        m = usable_steps(g, bt, hr, threshold, min_float)
        used[b] = m
        vals[b] = quadratic_log(lanczos_tridiagonal(g[:m], bt[:max(m - 1, 0)]), norms2[b])
    return vals, used
