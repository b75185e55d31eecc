"""Reference for the trace form of the CDGP data term (`training.TrainableCGGP(data_term="trace")`,
`models.CGGP(data_term="trace")`): a dense torch-fp64 CPU restatement on explicit kernel matrices, with Cholesky solves
and autograd in the variance, the lengthscales, the noise variance and Z.  `elbo` takes the arguments of
`cdgp_tip_reference.elbo`, the reference of the batch form.  tests/test_cdgp_full_host.py holds it to that reference
(with probes = sqrt(M) I the two agree) and the Rademacher estimate to the exact trace; tests/test_gpu_cdgp_full.py
holds the device models to it.

    A = K_mm + diag(s2 / counts),  a = A^-1 u,  S = A^-1 Zp,  mu = K_nm a,  U = K_nm S,  V = K_nm Zp
    sum_n var_exp_n = -(B/2) log(2 pi s2) - (|y - mu|^2 + B variance - (1/P) sum_p U_p . V_p) / (2 s2)
    elbo = scale sum_n var_exp_n - KL          (KL as `cdgp_tip_reference.elbo` forms it)

`probes=None` is the exact form: tr(A^-1 K_mm) and tr(A^-1 K_mn K_nm) from the inverse, the log-determinant's gradient
exact as well (`eval_logdet` without probes); its value stays 0.0 under logdet="model".
"""

import math

import torch

import cdgp_tip_reference as tip
from sgpr_grad_reference import kernel_torch


def _solver(A):
    L = torch.linalg.cholesky(A)
    return lambda R: torch.cholesky_solve(R, L)


def variance_sum(kind, variance, ls, s2, Z, x, counts, probes=None):
    """sum_n fvar_n over the rows of x as the trace form has it: B variance - tr(A^-1 K_mn K_nm), the trace estimated
    by (1/P) sum_p (K_nm s_p) . (K_nm z_p) with the probes [M, P], or exact with `probes=None`."""
    solve = _solver(tip.kzz(kind, variance, ls, Z) + torch.diag(s2 / counts.reshape(-1)))
    Knm = kernel_torch(kind, variance, ls, x, Z)
    if probes is None:
        tr = torch.diagonal(solve(Knm.t() @ Knm)).sum()
    else:
        tr = ((Knm @ solve(probes)) * (Knm @ probes)).sum() / probes.shape[1]
    return x.shape[0] * variance - tr


def elbo(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, num_data=None, logdet_probes=None, logdet="model"):
    """`TrainableCGGP(data_term="trace").elbo((x, y), probes)`; the keywords are those of `cdgp_tip_reference.elbo`.  A
    batch without rows gives -KL."""
    Kmm = tip.kzz(kind, variance, ls, Z)
    lam = s2 / counts.reshape(-1)
    A = Kmm + torch.diag(lam)
    solve = _solver(A)
    a = solve(pseudo_u.reshape(-1, 1))
    B = x.shape[0]
    Knm = kernel_torch(kind, variance, ls, x, Z)
    if probes is None:
        inv = solve(torch.eye(A.shape[0], dtype=A.dtype))
        trace = (inv * Kmm).sum()
        data_trace = (inv * (Knm.t() @ Knm)).sum()
    else:
        S = solve(probes)
        trace = (S * (Kmm @ probes)).sum() / probes.shape[1]
        data_trace = ((Knm @ S) * (Knm @ probes)).sum() / probes.shape[1]
    resid = y - Knm @ a
    data_sum = -0.5 * B * (math.log(2.0 * math.pi) + torch.log(s2)) \
        - 0.5 * ((resid * resid).sum() + B * variance - data_trace) / s2
    quad = ((Kmm @ a) * a).sum()
    if logdet == "exact" or (probes is None and logdet_probes is None):
        ld = torch.logdet(A)
        if logdet != "exact":  # eval_logdet without probes: the exact gradient, the value 0.0
            ld = ld - ld.detach()
    else:
        ld = tip.logdet_surrogate(A, probes if logdet_probes is None else logdet_probes)
        if logdet == "model":
            ld = ld - ld.detach()
    kl = 0.5 * (quad - trace + ld - torch.log(lam).sum())
    scale = 1.0 if num_data is None or B == 0 else float(num_data) / float(B)
    return data_sum * scale - kl


def loss_and_grads(kind, variance, ls, s2, Z, x, y, pseudo_u, counts, probes, **kw):
    """(-elbo, [d/dvariance, d/dls, d/ds2, d/dZ]) at plain tensors."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (variance, ls, s2, Z)]
    loss = -elbo(kind, *leaves, x, y, pseudo_u, counts, probes, **kw)
    return float(loss.detach()), list(torch.autograd.grad(loss, leaves))
