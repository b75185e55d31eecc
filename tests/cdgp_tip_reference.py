"""Reference for CDGP training with trainable inducing inputs (`training.TrainableCGGP(trainable_inducing=True)`): a
dense torch-fp64 restatement of `TrainableCGGP.elbo` on explicit kernel matrices and `torch.linalg.solve`,
differentiable by autograd in the variance, the lengthscales, the noise variance and Z.  tests/test_cdgp_tip_host.py
holds it to finite differences, to the exact log-determinant and to the closed forms of tests/cdgp_mf_reference.py;
tests/test_gpu_cdgp_tip.py holds the device models to it.

The log-determinant enters as the model's does: value 0.0 (`models.eval_logdet`) and the gradient of the surrogate
sum(S.detach() * (A probes)) / P with S = A^-1 probes, which is the probe estimator of d log|A|.
"""

import math

import torch

from sgpr_grad_reference import kernel_torch


def kzz(kind, variance, ls, Z):
    """k(Z, Z), differentiable in Z (direct differences; the Matern floor keeps the diagonal's gradient at 0)."""
    return kernel_torch(kind, variance, ls, Z, Z)


def logdet_surrogate(A, probes):
    """sum(S.detach() * (A probes)) / P: its gradient in A is S probes^T / P, the estimator's."""
    S = torch.linalg.solve(A, probes).detach()
    return (S * (A @ probes)).sum() / probes.shape[1]


def elbo(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, num_data=None, logdet_probes=None, logdet="model"):
    """`TrainableCGGP.elbo((x, y), probes)` with Hutchinson probes [M, P].  `logdet_probes`: the estimator's own draw
    (`independent_logdet_probes=True`), else `probes`.  `logdet`: "model" (value 0.0, the surrogate's gradient),
    "surrogate" (the surrogate's value too) or "exact" (`torch.logdet`)."""
    Kmm = kzz(kind, variance, ls, Z)
    lam = s2 / counts.reshape(-1)
    A = Kmm + torch.diag(lam)
    Kmn = kernel_torch(kind, variance, ls, Z, x)
    a = torch.linalg.solve(A, pseudo_u.reshape(-1, 1))
    W = torch.linalg.solve(A, Kmn)
    S = torch.linalg.solve(A, probes)
    fvar = (variance - (Kmn * W).sum(dim=0))[:, None]
    fmu = Kmn.t() @ a
    var_exp = -0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(s2) - 0.5 * ((y - fmu) ** 2 + fvar) / s2
    trace = (S * (Kmm @ probes)).sum() / probes.shape[1]
    quad = ((Kmm @ a) * a).sum()
    if logdet == "exact":
        ld = torch.logdet(A)
    else:
        ld = logdet_surrogate(A, probes if logdet_probes is None else logdet_probes)
        if logdet == "model":
            ld = ld - ld.detach()
    kl = 0.5 * (quad - trace + ld - torch.log(lam).sum())
    scale = 1.0 if num_data is None else float(num_data) / float(x.shape[0])
    return var_exp.sum() * scale - kl


def loss_and_grads(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, **kw):
    """(-elbo, [d/dvariance, d/dls, d/ds2, d/dZ]) at plain tensors."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (variance, ls, s2, Z)]
    loss = -elbo(kind, *leaves, x, y, pseudo_u, counts, probes, **kw)
    return float(loss.detach()), list(torch.autograd.grad(loss, leaves))
