"""Long-double reference of the backward pass of the random-Fourier-feature prior sample (`mgp_rff_sample_vjp`,
include/mgp_pathwise.h), the error bound that header states, and the chunking rule it documents.

    out(s, n)    = scale sum_l (W[s, l] cos phi_nl + W[s, L + l] sin phi_nl),   phi_nl = theta_l . x_n
    q(n, l)      = scale sum_s G(s, n) (W[s, L + l] cos phi_nl - W[s, l] sin phi_nl)
    dtheta[l, d] = sum_n q(n, l) x_n[d]
    dX[n, d]     = sum_l q(n, l) theta_l[d]

Everything is numpy in np.longdouble from float64 inputs; G is [S, N].  tests/test_rff_vjp_reference.py holds this
file honest against central differences of `forward`.
"""

import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def forward(X, theta, W, scale):
    """out [S, N] in long double."""
    X, theta, W = (np.asarray(a, dtype=LD) for a in (X, theta, W))
    L = theta.shape[0]
    ph = X @ theta.T
    return LD(scale) * (W[:, :L] @ np.cos(ph).T + W[:, L:] @ np.sin(ph).T)


def vjp(X, theta, W, scale, G):
    """(dtheta [L, D], dX [N, D]) in long double."""
    X, theta, W, G = (np.asarray(a, dtype=LD) for a in (X, theta, W, G))
    L = theta.shape[0]
    ph = X @ theta.T  # [N, L]
    Q = LD(scale) * ((G.T @ W[:, L:]) * np.cos(ph) - (G.T @ W[:, :L]) * np.sin(ph))
    return Q.T @ X, Q @ theta


def chunk_plan(streamed, owned, D, num_cus):
    """(len, chunks) of the streamed side as include/mgp_pathwise.h documents them."""
    owners = 256 * (2 if D <= 8 else 1)
    blocks = -(-owned // owners)
    want = 4 * num_cus
    chunks = 1
    if blocks < want:
        chunks = max(1, min(-(-want // blocks), -(-streamed // 32), 256))
    length = -(-streamed // chunks)
    return length, -(-streamed // length)


def bounds(X, theta, W, scale, G, num_cus):
    """(bound on |dtheta - exact| [L, D], bound on |dX - exact| [N, D]) of include/mgp_pathwise.h:
        u (8 (1 + max_nl sum_d |x_nd theta_ld|) + 2 S + D + len + chunks + 4) times the sum of the absolute terms
    |scale| sum_n sum_s |G(s, n)| (|W[s, l]| + |W[s, L + l]|) |x_n[d]| (dtheta; dX: |theta_l[d]|, summed over l)."""
    X, theta, W, G = (np.abs(np.asarray(a, dtype=np.float64)) for a in (X, theta, W, G))
    N, D = X.shape
    L, S = theta.shape[0], W.shape[0]
    pmax = float(np.max(X @ theta.T)) if N and L else 0.0
    A = abs(scale) * (G.T @ (W[:, :L] + W[:, L:]))  # [N, L]: sum_s |G| (|Wc| + |Ws|)
    out = []
    for streamed, owned, absterms in ((N, L, A.T @ X), (L, N, A @ theta)):
        length, chunks = chunk_plan(streamed, owned, D, num_cus) if streamed else (0, 0)
        out.append(U * (8 * (1 + pmax) + 2 * S + D + length + chunks + 4) * absterms)
    return out[0], out[1]
