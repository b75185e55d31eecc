"""The contract of the fused any-D random-Fourier-feature kernels (MGP_RFF_ANYD, include/mgp_pathwise.h,
csrc/rff_anyd.hip) as Python: the split plan, the scratch formula and the error bounds that header states.  The
long-double `forward` / `vjp` are those of tests/rff_vjp_reference.py.  tests/test_rff_anyd_reference.py holds this file
honest: the plan against the expressions in csrc/rff_anyd.hip, the phase term of the bound against an fp64 emulation of
the k-step sums in several orders.
"""

import numpy as np

from rff_vjp_reference import LD, U, forward, vjp  # noqa: F401  (re-exported: the reference of the GPU tests)

GROUP = 256  # most output dimensions of one group of the backward pass
NT_LADDER = (3, 4, 5, 6, 8, 10, 12, 16)


def ceil_div(a, b):
    return -(-a // b)


def a256(b):
    return (b + 255) // 256 * 256


def ks_of(D):
    return ceil_div(D, 4)


def groups_of(D):
    return ceil_div(D, GROUP)


def nt_of(D):
    """Output tiles a wave holds: the 16-wide tiles of D shared among the groups, rounded up the ladder."""
    per = ceil_div(ceil_div(D, 16), groups_of(D))
    return next(nt for nt in NT_LADDER if per <= nt)


def split_plan(owned, streamed, groups, num_cus):
    """(nsplit, tps) of include/mgp_pathwise.h: `nsplit` runs of `tps` streamed tiles of 16 points."""
    wg = ceil_div(owned, 64) * groups
    stiles = ceil_div(streamed, 16)
    ns = 1
    if wg < 2 * num_cus:
        ns = max(1, min(ceil_div(2 * num_cus, wg), ceil_div(stiles, 16), 256))
    tps = ceil_div(stiles, ns)
    return ceil_div(stiles, tps), tps


def cuts(owned, streamed, groups, num_cus):
    """First streamed point of every split but the first."""
    ns, tps = split_plan(owned, streamed, groups, num_cus)
    return [16 * tps * z for z in range(1, ns)]


def scratch_bytes(N, L, D, num_cus, op):
    """Bytes of the "gen" arena one call takes: op in "forward", "dtheta", "dX", "both"."""
    KS = ks_of(D)
    if op == "both":
        return max(scratch_bytes(N, L, D, num_cus, "dtheta"), scratch_bytes(N, L, D, num_cus, "dX"))
    owned, streamed = (L, N) if op == "dtheta" else (N, L)
    To, Ts = ceil_div(owned, 16), ceil_div(streamed, 16)
    ns, _ = split_plan(owned, streamed, 1 if op == "forward" else groups_of(D), num_cus)
    b = a256(512 * KS * To) + a256(512 * KS * Ts)
    if op == "forward":
        return b + a256(4096 * Ts) + (a256(64 * ns * N) if ns > 1 else 0)
    DT = 16 * ceil_div(D, 16)
    return b + a256(2048 * To) + a256(2048 * Ts) + (a256(8 * ns * owned * DT) if ns > 1 else 0)


def phase_factor(D, pmax):
    """8 + (K + 2) P: the per-feature bound in units of u, K = 4 ceil(D / 4)."""
    return 8 + (4 * ks_of(D) + 2) * pmax


def _pmax(X, theta):
    return float(np.max(np.abs(X) @ np.abs(theta).T)) if X.shape[0] and theta.shape[0] else 0.0


def forward_bound(X, theta, W, scale, num_cus):
    """Bound on |out - exact| [S, N]: u (8 + (K + 2) P + 2 len + nsplit + 2) |scale| sum_l (|Wc| + |Ws|)."""
    X, theta, W = (np.asarray(a, dtype=np.float64) for a in (X, theta, W))
    (N, D), L = X.shape, theta.shape[0]
    ns, tps = split_plan(N, L, 1, num_cus) if L else (0, 0)
    absw = abs(scale) * (np.abs(W[:, :L]) + np.abs(W[:, L:])).sum(axis=1)  # [S]
    fac = phase_factor(D, _pmax(X, theta)) + 2 * 16 * tps + ns + 2
    return U * fac * np.repeat(absw[:, None], N, axis=1)


def vjp_bounds(X, theta, W, scale, G, num_cus):
    """(bound on |dtheta - exact| [L, D], bound on |dX - exact| [N, D]):
        u (8 + (K + 2) P + S + len + nsplit + 4) times the sums of absolute terms of the plain call's bound."""
    Xa, ta, Wa, Ga = (np.abs(np.asarray(a, dtype=np.float64)) for a in (X, theta, W, G))
    (N, D), L, S = Xa.shape, ta.shape[0], Wa.shape[0]
    A = abs(scale) * (Ga.T @ (Wa[:, :L] + Wa[:, L:]))  # [N, L]
    base = phase_factor(D, _pmax(Xa, ta)) + S + 4
    out = []
    for streamed, owned, absterms in ((N, L, A.T @ Xa), (L, N, A @ ta)):
        ns, tps = split_plan(owned, streamed, groups_of(D), num_cus) if streamed and owned else (0, 0)
        out.append(U * (base + 16 * tps + ns) * absterms)
    return out[0], out[1]
