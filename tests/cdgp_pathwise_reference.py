"""Reference for the pathwise form of the CDGP data term (`training.TrainableCGGP(data_term="pathwise")`,
`models.CGGP(data_term="pathwise")`): a dense torch-fp64 CPU restatement on explicit kernel matrices and explicit
[cos | sin] feature matrices, with Cholesky solves and autograd in the variance, the lengthscales, the noise variance
and Z.  `elbo` takes the arguments of `cdgp_full_reference.elbo` plus the draw (E, W, xi) and the noise convention.

    theta = E / ls,  phi(p) = [cos(p theta^T) | sin(p theta^T)],  prior(p) = sqrt(variance / L) W phi(p)^T      [S, .]
    A = K_mm + diag(lam),  lam = s2 / counts,  eps = sqrt(lam) xi ("matheron") or lam xi ("reference")
    f = prior(x) + (K_nm A^-1 (u - prior(Z) - eps)^T)^T                                                        [S, B]
    elbo = -(1/2) [sum_sn (y_n - f_sn)^2 / (S s2) + B log(2 pi s2)] scale - KL

with KL what `cdgp_full_reference.elbo` gives on a batch without rows.  tests/test_cdgp_pathwise_host.py holds the
samples to the numpy restatement of the reference's `pathwise_samples` and the expectation to the batch form.
"""

import math

import torch

import cdgp_full_reference as full
import cdgp_tip_reference as tip
from sgpr_grad_reference import kernel_torch


def prior(variance, ls, points, E, W):
    """[S, n] prior function samples on the reparameterised frequencies E / ls."""
    L = E.shape[0]
    ph = points @ (E / ls.reshape(1, -1)).t()
    return torch.sqrt(variance / L) * (W @ torch.cat([torch.cos(ph), torch.sin(ph)], dim=1).t())


def samples(kind, variance, ls, s2, Z, x, pseudo_u, counts, draw, epsilon="matheron"):
    """[S, B] pathwise posterior samples at x."""
    E, W, xi = draw
    B = x.shape[0]
    lam = s2 / counts.reshape(-1)
    p = prior(variance, ls, torch.cat([x, Z], dim=0), E, W)
    eps = (torch.sqrt(lam) if epsilon == "matheron" else lam)[None, :] * xi
    A = tip.kzz(kind, variance, ls, Z) + torch.diag(lam)
    w = torch.cholesky_solve((pseudo_u.reshape(1, -1) - p[:, B:] - eps).t(), torch.linalg.cholesky(A))  # [M, S]
    return p[:, :B] + (kernel_torch(kind, variance, ls, x, Z) @ w).t()


def data_term(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, draw, epsilon="matheron"):
    """-(1/2) [sum_sn (y_n - f_sn)^2 / (S s2) + B log(2 pi s2)], unscaled."""
    B = x.shape[0]
    f = samples(kind, variance, ls, s2, Z, x, pseudo_u, counts, draw, epsilon)
    sq = ((y.reshape(1, -1) - f) ** 2).sum()
    return -0.5 * (sq / (f.shape[0] * s2) + B * (math.log(2.0 * math.pi) + torch.log(s2)))


def elbo(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, draw, epsilon="matheron", num_data=None,
         logdet_probes=None, logdet="model"):
    """`TrainableCGGP(data_term="pathwise").elbo((x, y), probes, pathwise=draw)`.  A batch without rows gives -KL."""
    minus_kl = full.elbo(kind, variance, ls, s2, Z, x[:0], y[:0], pseudo_u, counts, probes, logdet_probes=logdet_probes,
                         logdet=logdet)
    B = x.shape[0]
    if B == 0:
        return minus_kl
    scale = 1.0 if num_data is None else float(num_data) / float(B)
    return data_term(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, draw, epsilon) * scale + minus_kl


def loss_and_grads(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, draw, **kw):
    """(-elbo, [d/dvariance, d/dls, d/ds2, d/dZ]) at plain tensors."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (variance, ls, s2, Z)]
    loss = -elbo(kind, *leaves, x, y, pseudo_u, counts, probes, draw, **kw)
    return float(loss.detach()), list(torch.autograd.grad(loss, leaves))
