"""References for the SGPR gradient (`mgp_kmn_knm_vjp`, `training.TrainableSGPR`): a long-double restatement of the VJP
of (Q, B) = (K_mn K_nm, K_mn Y) with every (row, column) pair evaluated, the same for the VJP of a dense kernel block
(`mgp_k_dense_vjp`), and a torch fp64 restatement of GPflow's
`SGPR.elbo` on an explicit K_nm, differentiable in every parameter including Z."""

import math

import numpy as np
import torch

from lml_reference import _profile

LD = np.longdouble


def kmn_knm_vjp_reference(name, variance, lengthscales, X, Z, Gq, Y=None, Gb=None, block=256):
    """(dvariance, dl [D], dZ [M, D]) in long double, with W = K (Gq + Gq^T) + Y Gb^T, and the same sums over
    |terms| where a term's W is replaced by |K| |Gq + Gq^T| + |Y| |Gb|^T (so the GEMM's rounding is inside the scale)."""
    X, Z = np.asarray(X, dtype=LD), np.asarray(Z, dtype=LD)
    Gq = np.asarray(Gq, dtype=LD)
    ls = np.asarray(lengthscales, dtype=LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, X.shape[1])
    var = LD(variance)
    Xs, Zs = X / ls, Z / ls
    G2 = Gq + Gq.T
    aG2 = np.abs(G2)
    M, D = Z.shape
    coef = var * LD(-2) / ls
    dv, dl, dZ = LD(0), np.zeros(D, dtype=LD), np.zeros((M, D), dtype=LD)
    sv, sl, sz = LD(0), np.zeros(D, dtype=LD), np.zeros((M, D), dtype=LD)
    for i0 in range(0, X.shape[0], block):
        diff = Xs[i0:i0 + block, None, :] - Zs[None, :, :]
        r2 = (diff * diff).sum(axis=2)
        f, fp = _profile(name, r2)
        K = var * f
        W = K @ G2
        Wa = np.abs(K) @ aG2
        if Y is not None:
            Yb, Gbl = np.asarray(Y[i0:i0 + block], dtype=LD), np.asarray(Gb, dtype=LD)
            W = W + Yb @ Gbl.T
            Wa = Wa + np.abs(Yb) @ np.abs(Gbl).T
        dv += np.sum(W * f)
        sv += np.sum(Wa * np.abs(f))
        g, ga = (W * fp)[:, :, None], (Wa * np.abs(fp))[:, :, None]
        dl += (g * diff * diff).sum(axis=(0, 1)) * coef
        sl += (ga * diff * diff).sum(axis=(0, 1)) * np.abs(coef)
        dZ += (g * diff).sum(axis=0) * coef
        sz += (ga * np.abs(diff)).sum(axis=0) * np.abs(coef)
    return dv, dl, dZ, sv, sl, sz


def k_dense_vjp_reference(name, variance, lengthscales, A, B, G, block=256):
    """(dvariance, dl [D]) = sum_ij G_ij dk(a_i, b_j) / d(variance, l_d) in long double (`mgp_k_dense_vjp`), every pair,
    direct differences, and the same sums over |terms| (the scale the tests measure rounding against)."""
    A, B, G = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD), np.asarray(G, dtype=LD)
    ls = np.asarray(lengthscales, dtype=LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, A.shape[1])
    As, Bs = A / ls, B / ls
    coef = LD(variance) * LD(-2) / ls
    D = A.shape[1]
    dv, dl, sv, sl = LD(0), np.zeros(D, dtype=LD), LD(0), np.zeros(D, dtype=LD)
    for i0 in range(0, A.shape[0], block):
        diff = As[i0:i0 + block, None, :] - Bs[None, :, :]
        d2 = diff * diff
        f, fp = _profile(name, d2.sum(axis=2))
        Gb = G[i0:i0 + block]
        dv += np.sum(Gb * f)
        sv += np.sum(np.abs(Gb * f))
        w = (Gb * fp)[:, :, None] * d2 * coef
        dl += w.sum(axis=(0, 1))
        sl += np.abs(w).sum(axis=(0, 1))
    return dv, dl, sv, sl


def kernel_torch(name, variance, lengthscales, A, B):
    """GPflow's stationary kernels on explicit pairs, direct differences, r = sqrt(max(r2, 1e-36))."""
    diff = A[:, None, :] / lengthscales - B[None, :, :] / lengthscales
    r2 = (diff * diff).sum(dim=2)
    if name == "se":
        return variance * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-36))
    if name == "matern12":
        return variance * torch.exp(-r)
    if name == "matern32":
        s3 = math.sqrt(3.0)
        return variance * (1.0 + s3 * r) * torch.exp(-s3 * r)
    s5 = math.sqrt(5.0)
    return variance * (1.0 + s5 * r + 5.0 / 3.0 * r2) * torch.exp(-s5 * r)


def sgpr_elbo_explicit(name, variance, lengthscales, s2, X, Y, Z, jitter=1e-6):
    """GPflow `SGPR.elbo` (const + logdet + quad + trace) with K_nm formed explicitly; torch tensors throughout, so
    autograd gives the gradient in variance, lengthscales, s2 and Z."""
    N, M = X.shape[0], Z.shape[0]
    Knm = kernel_torch(name, variance, lengthscales, X, Z)
    Kmm = kernel_torch(name, variance, lengthscales, Z, Z) + jitter * torch.eye(M, dtype=X.dtype, device=X.device)
    L = torch.linalg.cholesky(Kmm)
    A = torch.linalg.solve_triangular(L, Knm.t(), upper=False) / torch.sqrt(s2)
    AAT = A @ A.t()
    LB = torch.linalg.cholesky(AAT + torch.eye(M, dtype=X.dtype, device=X.device))
    c = torch.linalg.solve_triangular(LB, A @ Y, upper=False) / torch.sqrt(s2)
    const = -0.5 * N * math.log(2.0 * math.pi)
    logdet = -torch.log(LB.diagonal()).sum() - 0.5 * N * torch.log(s2)
    quad = -0.5 * (Y * Y).sum() / s2 + 0.5 * (c * c).sum()
    trace = -0.5 * N * variance / s2 + 0.5 * AAT.diagonal().sum()
    return const + logdet + quad + trace
