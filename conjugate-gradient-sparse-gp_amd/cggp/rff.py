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


# `rff_anyd="auto"` takes the fused any-D kernels (MGP_RFF_ANYD, include/mgp_pathwise.h) in a region (op, S,
# D <= max_d, N L >= min_nl) only where they took at most 0.9 of the parent route's time (feature panels and a GEMM
# forward, `training._rff_vjp_panels` backward) at EVERY measured point of that region; `tools/run_rff_anyd.py
# --derive` computes the table from profiles/rff_anyd_times.json and tests/test_rff_anyd_abi.py pins it to that file.
# Measured: D in {33, 48, 77, 90, 128, 256, 257, 512}, S in {1, 5, 8}, L in {256, 1024, 4096}, N in {2^14, 2^17, 2^20}
# (DESIGN 4.24).  Forward: 0.10 - 0.65 everywhere.  dtheta and dX: 0.02 - 0.82 up to D = 257; at D = 512, where the
# output dimensions go in two groups and the phases are formed twice, 0.35 - 0.93 at L <= 1024 and 1.10 - 1.43 at
# L = 4096, so D = 512 is left out.  2^22 = 2^14 * 256 is the smallest N L measured.
# {(op, S): (max_d, min_nl)}; a sample count or an operation that was not measured is not taken.
RFF_ANYD_AUTO_MIN_D = 33
RFF_ANYD_AUTO = {(op, S): (max_d, 1 << 22)
                 for op, max_d in (("forward", 512), ("dtheta", 257), ("dX", 257)) for S in (1, 5, 8)}
RFF_ANYD_MAX_S = 8  # above it libmgp's flagged calls are the plain ones


def check_rff_anyd(rff_anyd, name="rff_anyd"):
    """`rff_anyd` as given, or `ValueError`: False, True or "auto"."""
    if isinstance(rff_anyd, bool) or (isinstance(rff_anyd, str) and rff_anyd == "auto"):
        return rff_anyd
    raise ValueError(f"{name} must be False, True or 'auto', got {rff_anyd!r}")


def rff_anyd_auto(dtype, D, S, N, L, op="forward"):
    """The rule behind `rff_anyd="auto"` for `op` ("forward", "dtheta" or "dX"): fp64, a measured sample count, and
    RFF_ANYD_AUTO_MIN_D <= D <= max_d, N L >= min_nl of RFF_ANYD_AUTO[(op, S)]."""
    region = RFF_ANYD_AUTO.get((op, int(S)))
    return (dtype == torch.float64 and region is not None and RFF_ANYD_AUTO_MIN_D <= int(D) <= region[0]
            and int(N) * int(L) >= region[1])


def use_rff_anyd(rff_anyd, dtype, D, S, N, L, op="forward"):
    """Whether a call with this setting ORs the flag in.  True: wherever libmgp serves it (fp64, D > 32, S <= 8; the
    flag changes nothing elsewhere, but the backward pass must not be sent where the plain call refuses)."""
    if rff_anyd == "auto":
        return rff_anyd_auto(dtype, D, S, N, L, op)
    return bool(rff_anyd) and dtype == torch.float64 and int(D) > 32 and 1 <= int(S) <= RFF_ANYD_MAX_S


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


def rff_sample(inputs, kernel, num_bases, num_samples=1, *, seed=None, theta=None, weights=None, rff_anyd=False):
    """[S, N] prior function samples sqrt(variance / L) * W Phi(inputs)^T (reference `rff.py:60-73`).

    One stream: theta first (unless injected), then the weights (unless injected).  On the device the samples are
    formed by `mgp_rff_sample` without the [N, 2L] feature panel where D <= 32 and S <= 8 -- and, with `rff_anyd`
    (False, True or "auto": `rff_anyd_auto`), at 32 < D <= 512 in fp64 too (csrc/rff_anyd.hip)."""
    check_rff_anyd(rff_anyd)
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
        anyd = use_rff_anyd(rff_anyd, inputs.dtype, D, weights.shape[0], inputs.shape[0], L)
        return ops.rff_sample(inputs.contiguous(), theta, weights, scale, ops.ROWS, anyd=anyd)
    return scale * (weights @ basis_vectors(inputs, theta).t())
