"""Random Fourier features of the stationary kernels -- host mirror of the reference's `cggp/rff.py`.

Names and argument order follow the reference (`basis_theta_parameter`, `basis_vectors`, `rff_sample`).  The
spectral draws come from the project's documented stream (numpy PCG64 from `seed`, as `models.rademacher`):
first the [L, D] standard normals, then (Matern) the L chi-square variates, then the [S, 2L] weights.  The
reference draws them with TensorFlow Probability, whose stream cannot be reproduced outside it, so tests inject
`theta=` / `weights=`.

On device tensors the features and the samples are computed by libmgp (`mgp_rff_features`, `mgp_rff_sample`,
csrc/rff.hip); for CPU tensors `basis_vectors` and `rff_sample` are the reference's dense torch expression.
"""

import math

import numpy as np
import torch

from . import ops

# smoothness index nu of the Matern kernels (reference rff.py:13-17); SE has no entry
_SMOOTHNESS = {"matern12": 1, "matern32": 3, "matern52": 5}


def _rng(seed):
    # an int / None seeds a fresh PCG64 stream; a Generator continues the caller's
    return np.random.default_rng(seed)


def basis_theta_parameter(kernel, num_bases, seed=None, *, dim=None):
    """theta [L, D] float64 (CPU tensor) drawn from the kernel's spectral density (reference `rff.py:20-45,82-91`).

    SE: N(0, diag(1/lengthscale)^2).  Matern-nu/2: the same normal times sqrt(nu / chi2_nu), one chi-square variate
    per basis (a multivariate Student-t with nu degrees of freedom).  `dim` gives D for an isotropic kernel whose
    lengthscale is a single number; otherwise D = len(kernel.lengthscales)."""
    ls = np.asarray(kernel.lengthscales, dtype=np.float64)
    D = int(dim) if dim is not None else ls.size
    if ls.size == 1:
        ls = np.full(D, ls[0])
    if ls.size != D:
        raise ValueError(f"kernel has {ls.size} lengthscales, dim={D}")
    rng = _rng(seed)
    theta = rng.standard_normal((int(num_bases), D)) / ls[None, :]
    name = getattr(kernel, "name", None)
    if name == "se":
        pass
    elif name in _SMOOTHNESS:
        nu = _SMOOTHNESS[name]
        chi2 = rng.chisquare(nu, size=int(num_bases))
        theta = theta * np.sqrt(nu / chi2)[:, None]
    else:
        raise ValueError(f"Not supported kernel class {kernel.__class__}")
    return torch.from_numpy(theta)


def basis_vectors(inputs, theta):
    """[N, 2L] = [cos(inputs theta^T) | sin(inputs theta^T)] (reference `rff.py:48-57`), cos block first."""
    theta = torch.as_tensor(theta).to(device=inputs.device, dtype=inputs.dtype)
    if inputs.is_cuda:
        return ops.rff_features(inputs, theta)
    xt = inputs @ theta.t()
    return torch.cat([torch.cos(xt), torch.sin(xt)], dim=-1)


def rff_weights(num_samples, num_bases, seed=None):
    """W [S, 2L] float64 standard normals (reference `rff.py:68-69`), the next draws of the stream."""
    return torch.from_numpy(_rng(seed).standard_normal((int(num_samples), 2 * int(num_bases))))


def rff_sample(inputs, kernel, num_bases, num_samples=1, *, seed=None, theta=None, weights=None):
    """[S, N] prior function samples sqrt(variance / L) * W Phi(inputs)^T (reference `rff.py:60-73`).

    One stream: theta first (unless injected), then the weights (unless injected).  On the device the samples are
    formed by `mgp_rff_sample` without the [N, 2L] feature panel where D <= 32 and S <= 8."""
    D = inputs.shape[-1]
    rng = _rng(seed)
    if theta is None:
        theta = basis_theta_parameter(kernel, num_bases, rng, dim=D)
    if weights is None:
        weights = rff_weights(num_samples, num_bases, rng)
    theta = torch.as_tensor(theta).to(device=inputs.device, dtype=inputs.dtype).contiguous()
    weights = torch.as_tensor(weights).to(device=inputs.device, dtype=inputs.dtype).contiguous()
    L = theta.shape[0]
    if weights.shape != (weights.shape[0], 2 * L):
        raise ValueError(f"weights must be [S, 2L={2 * L}], got {tuple(weights.shape)}")
    scale = math.sqrt(kernel.variance / L) if L > 0 else 0.0
    if inputs.is_cuda:
        return ops.rff_sample(inputs.contiguous(), theta, weights, scale, ops.ROWS)
    return scale * (weights @ basis_vectors(inputs, theta).t())
