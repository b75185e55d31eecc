"""tests/kvjp_points_reference.py held honest on the CPU: its four outputs against torch fp64 autograd of `kernel_torch`
(sgpr_grad_reference.py) for all four kernels, against `k_dense_vjp_reference` for the scalars, and against the
project's torch route `training.k_grad_points` / `kmm_grad_z` (no GPU needed)."""

import numpy as np
import pytest
import torch

from kvjp_points_reference import excess, k_dense_vjp_points_reference
from sgpr_grad_reference import k_dense_vjp_reference, kernel_torch

KERNELS = ["se", "matern12", "matern32", "matern52"]
# torch evaluates the same sums in fp64: a few hundred terms of rounding 2^-53 each stay far below 1e-10 of the sum of
# |terms|; the bar is the GPU tests' (kvjp_points_reference.VJP_BAR)


def _problem(D, na=23, nb=17, seed=0, same=False):
    rng = np.random.default_rng(seed + D)
    A = rng.uniform(-2.0, 2.0, (na, D))
    B = A.copy() if same else rng.uniform(-2.0, 2.0, (nb, D))
    return A, B, rng.standard_normal((A.shape[0], B.shape[0])), rng.uniform(0.6, 1.4, D) * np.sqrt(D), 1.3


@pytest.mark.parametrize("D", [1, 3, 8])
@pytest.mark.parametrize("name", KERNELS)
def test_against_autograd_of_kernel_torch(name, D):
    A, B, G, ls, var = _problem(D)
    ref = k_dense_vjp_points_reference(name, var, ls, A, B, G)
    v = torch.tensor(var, dtype=torch.float64, requires_grad=True)
    l = torch.tensor(ls, requires_grad=True)
    At, Bt = torch.tensor(A, requires_grad=True), torch.tensor(B, requires_grad=True)
    (kernel_torch(name, v, l, At, Bt) * torch.tensor(G)).sum().backward()
    for key, got in (("dv", v.grad), ("dl", l.grad), ("dA", At.grad), ("dB", Bt.grad)):
        e = excess(got.numpy(), ref[key], ref["s" + key[1:]])
        print(f"{name} D={D} {key}: {e:.2e}")
        assert e <= 1.0
    dv, dl, sv, sl = k_dense_vjp_reference(name, var, ls, A, B, G)
    assert excess(ref["dv"], dv, sv, 1e-17) <= 1.0 and excess(ref["dl"], dl, sl, 1e-17) <= 1.0
    assert excess(ref["sv"], sv, sv, 1e-17) <= 1.0 and excess(ref["sl"], sl, sl, 1e-17) <= 1.0


@pytest.mark.parametrize("name", KERNELS)
def test_against_the_torch_route_of_training(name):
    from cggp import training
    D = 3
    A, B, G, ls, var = _problem(D, seed=5)
    ref = k_dense_vjp_points_reference(name, var, ls, A, B, G)
    dA, dB = training.k_grad_points(name, var, list(ls), torch.tensor(A), torch.tensor(B), torch.tensor(G))
    assert excess(dA.numpy(), ref["dA"], ref["sA"]) <= 1.0 and excess(dB.numpy(), ref["dB"], ref["sB"]) <= 1.0
    Z, _, G, ls, var = _problem(D, seed=6, same=True)
    ref = k_dense_vjp_points_reference(name, var, ls, Z, Z, G)
    dZ = training.kmm_grad_z(name, var, list(ls), torch.tensor(Z), torch.tensor(G))
    assert excess(dZ.numpy(), ref["dA"] + ref["dB"], ref["sA"] + ref["sB"]) <= 1.0


def test_coincident_points_add_exactly_nothing():
    A, B, G, ls, var = _problem(3, na=9, nb=9, seed=7)
    B[:4] = A[:4]
    Gd = np.zeros_like(G)
    Gd[np.arange(4), np.arange(4)] = 1.0
    for name in ("matern12", "matern52"):
        ref = k_dense_vjp_points_reference(name, var, ls, A, B, Gd)
        assert float(ref["dv"]) == 4.0 and not ref["dl"].any() and not ref["dA"].any() and not ref["dB"].any()
