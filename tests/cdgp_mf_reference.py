"""The three backward formulas of the matrix-free CDGP training path (cggp/training.py: _KzzTimes, _KzzLambdaSolve,
_KzzLambdaLogdet), restated in torch float64 on the CPU with dense algebra and closed-form kernel derivatives -- no
autograd in here.  tests/test_cdgp_matrix_free_host.py holds them to autograd through dense torch algebra;
tests/test_gpu_cdgp_matrix_free.py holds the device nodes to them.

K = variance f(r2), r2_ij = sum_d ((z_id - z_jd) / l_d)^2 (direct differences); A = K + diag(lam).  Every function takes
and returns column batches [M, R].
"""

import math

import torch

KINDS = ("se", "matern12", "matern32", "matern52")


def scaled_r2(Z, ls):
    a = Z / ls
    d = a[:, None, :] - a[None, :, :]
    return (d * d).sum(dim=2)


def profile(kind, r2):
    """f = k / variance (GPflow: r = sqrt(max(r2, 1e-36)) for the Matern kernels)."""
    if kind == "se":
        return torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-36))
    if kind == "matern12":
        return torch.exp(-r)
    if kind == "matern32":
        s = math.sqrt(3.0)
        return (1.0 + s * r) * torch.exp(-s * r)
    s = math.sqrt(5.0)
    return (1.0 + s * r + (5.0 / 3.0) * r * r) * torch.exp(-s * r)


def profile_slope(kind, r2):
    """df / dr2 in closed form; under the 1e-36 floor the Matern profiles do not depend on r2."""
    if kind == "se":
        return -0.5 * torch.exp(-0.5 * r2)
    live = r2 > 1e-36
    r = torch.sqrt(torch.where(live, r2, torch.full_like(r2, 1.0)))
    if kind == "matern12":
        g = -torch.exp(-r) / (2.0 * r)
    elif kind == "matern32":
        g = -1.5 * torch.exp(-math.sqrt(3.0) * r)
    else:
        s = math.sqrt(5.0)
        g = (-5.0 / 6.0) * (1.0 + s * r) * torch.exp(-s * r)
    return torch.where(live, g, torch.zeros_like(r2))


def kzz(kind, variance, ls, Z):
    return variance * profile(kind, scaled_r2(Z, ls))


def bilinear_grads(kind, variance, ls, Z, U, V):
    """(sum_r u_r^T (dK/dvariance) v_r, [sum_r u_r^T (dK/dl_d) v_r]): what `mgp_kxx_grad` returns."""
    G = U @ V.t()
    r2 = scaled_r2(Z, ls)
    dvar = (G * profile(kind, r2)).sum()
    W = variance * G * profile_slope(kind, r2)
    diff2 = (Z[:, None, :] - Z[None, :, :]) ** 2  # d r2 / d l_d = -2 diff2_d / l_d^3
    dls = -2.0 * (W[:, :, None] * diff2).sum(dim=(0, 1)) / ls ** 3
    return dvar, dls


def kzz_times_backward(kind, variance, ls, Z, V, G):
    """Out = K V, cotangent G: (dV, dvariance, dls)."""
    dvar, dls = bilinear_grads(kind, variance, ls, Z, G, V)
    return kzz(kind, variance, ls, Z) @ G, dvar, dls


def solve_backward(kind, variance, ls, lam, Z, rhs, G):
    """X = A^-1 rhs, cotangent G: (d rhs, dvariance, dls, dlam) with Gb = A^-1 G."""
    A = kzz(kind, variance, ls, Z) + torch.diag(lam)
    X = torch.linalg.solve(A, rhs)
    Gb = torch.linalg.solve(A, G)
    dvar, dls = bilinear_grads(kind, variance, ls, Z, Gb, X)
    return Gb, -dvar, -dls, -(Gb * X).sum(dim=1)


def logdet_backward(kind, variance, ls, lam, Z, S, probes, df=1.0):
    """The probe estimate of d log|A| with S = A^-1 probes handed in: (dvariance, dls, dlam)."""
    P = probes.shape[1]
    dvar, dls = bilinear_grads(kind, variance, ls, Z, S, probes)
    return df * dvar / P, df * dls / P, df * (S * probes).sum(dim=1) / P
