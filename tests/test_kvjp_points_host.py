"""The `fused_point_grads` keyword on the host (no GPU needed): its `ValueError`s, what the default calls (exactly what
it called before the keyword existed), the fall-back of fp32 and host tensors to the torch route under True, and the
constants of "auto" against profiles/kvjp_points_times.json."""

import json
import os
import types

import numpy as np
import pytest
import torch

from sgpr_grad_reference import kernel_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_setting_is_checked_everywhere():
    from cggp import conjugate_gradient as cgm, kernels, training
    for ok in (False, True, "auto"):
        assert cgm.check_fused_point_grads(ok) == ok
    Z = torch.zeros((4, 2), dtype=torch.float64)
    kern = kernels.SquaredExponential(variance=1.0, lengthscales=[1.0, 1.0])
    for bad in (None, 1, 0, "yes", "Auto"):
        with pytest.raises(ValueError, match="fused_point_grads"):
            cgm.check_fused_point_grads(bad)
        with pytest.raises(ValueError, match="fused_point_grads"):
            training.TrainableKernel(kern).K(Z, fused_point_grads=bad)
        with pytest.raises(ValueError, match="fused_point_grads"):
            training.TrainableCGGP(kern, 0.1, Z, pseudo_u=torch.zeros(4, dtype=torch.float64),
                                   cluster_counts=torch.ones(4, dtype=torch.float64), fused_point_grads=bad)
        with pytest.raises(ValueError, match="fused_point_grads"):
            training.TrainableSGPR(kern, 0.1, torch.zeros((6, 2), dtype=torch.float64),
                                   torch.zeros((6, 1), dtype=torch.float64), Z, fused_point_grads=bad)
    m = training.TrainableSGPR(kern, 0.1, torch.zeros((6, 2), dtype=torch.float64),
                               torch.zeros((6, 1), dtype=torch.float64), Z, fused_point_grads="auto")
    assert m.fused_point_grads == "auto"


def _spied(monkeypatch):
    """libmgp's three calls of a `_KBlock` replaced by torch on the host, each recording its name"""
    from cggp import ops, training
    calls = []

    def k_dense(spec, A, B, jitter=0.0, diag_add=None):
        calls.append("k_dense")
        ls = torch.tensor(spec.lengthscales, dtype=A.dtype)
        K = kernel_torch(spec.kind, spec.variance, ls, A.detach(), B.detach())
        return K + jitter * torch.eye(K.shape[0], dtype=K.dtype) if jitter else K

    def k_dense_vjp(spec, A, B, G):
        calls.append("k_dense_vjp")
        return 0.5, [0.25] * spec.D

    def k_dense_vjp_points(*a, **k):
        calls.append("k_dense_vjp_points")
        raise AssertionError("the fused entry point was called on the host")

    orig = training.k_grad_points

    def k_grad_points(*a, **k):
        calls.append("k_grad_points")
        return orig(*a, **k)

    monkeypatch.setattr(ops, "k_dense", k_dense)
    monkeypatch.setattr(ops, "k_dense_vjp", k_dense_vjp)
    monkeypatch.setattr(ops, "k_dense_vjp_points", k_dense_vjp_points)
    monkeypatch.setattr(training, "k_grad_points", k_grad_points)
    return calls


@pytest.mark.parametrize("setting", [False, True, "auto"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_host_tensors_take_the_calls_of_the_default(monkeypatch, setting, dtype):
    """False calls `ops.k_dense_vjp` then `k_grad_points`, as before the keyword; so do host tensors and fp32 tensors
    under True and "auto"; the gradients are those of the default, bit for bit."""
    from cggp import kernels, training
    rng = np.random.default_rng(0)
    A0, B0 = torch.tensor(rng.standard_normal((7, 3)), dtype=dtype), torch.tensor(rng.standard_normal((5, 3)), dtype=dtype)
    G = torch.tensor(rng.standard_normal((7, 5)), dtype=dtype)
    kern = training.TrainableKernel(kernels.Matern32(variance=1.2, lengthscales=[0.9, 1.0, 1.1]))
    grads = {}
    for which, s in (("default", False), ("setting", setting)):
        calls = _spied(monkeypatch)
        A, B = A0.clone().requires_grad_(True), B0.clone().requires_grad_(True)
        kw = {} if which == "default" else dict(fused_point_grads=s)
        kern.K(A, B, **kw).backward(G)
        assert calls == ["k_dense", "k_dense_vjp", "k_grad_points"]
        grads[which] = (A.grad.clone(), B.grad.clone())
        monkeypatch.undo()
    assert torch.equal(grads["setting"][0], grads["default"][0]) and torch.equal(grads["setting"][1], grads["default"][1])
    # without a point gradient nothing but mgp_k_dense_vjp runs, whatever the setting
    calls = _spied(monkeypatch)
    kern.K(A0, B0, fused_point_grads=setting).backward(G)
    assert calls == ["k_dense", "k_dense_vjp"]


def test_the_rule_of_use_fused_point_grads():
    from cggp import conjugate_gradient as cgm
    t = lambda dtype, cuda, n=4096, D=8: types.SimpleNamespace(dtype=dtype, is_cuda=cuda, shape=(n, D))
    dev64, dev32, host64 = t(torch.float64, True), t(torch.float32, True), t(torch.float64, False)
    assert cgm.use_fused_point_grads(True, dev64, dev64)
    for s in (True, "auto"):
        assert not cgm.use_fused_point_grads(s, dev32, dev32)
        assert not cgm.use_fused_point_grads(s, host64, host64) and not cgm.use_fused_point_grads(s, dev64, host64)
    assert not cgm.use_fused_point_grads(False, dev64, dev64)
    small = t(torch.float64, True, n=8)
    assert cgm.use_fused_point_grads(True, small, small)
    assert cgm.use_fused_point_grads("auto", dev64, dev64) == cgm.fused_point_grads_auto(torch.float64, 8, 4096, 4096)
    assert cgm.use_fused_point_grads("auto", small, small) == cgm.fused_point_grads_auto(torch.float64, 8, 8, 8)


def test_auto_follows_the_profile():
    from cggp import conjugate_gradient as cgm
    prof = json.load(open(os.path.join(ROOT, "profiles", "kvjp_points_times.json")))
    auto = prof["auto"]
    assert cgm.FUSED_POINT_GRADS_AUTO_MIN_PAIRS == auto["min_pairs"]
    assert cgm.FUSED_POINT_GRADS_AUTO_MAX_D == auto["max_d"]
    ops_rows = prof["op"]
    assert ops_rows and all(r["ratio"] == pytest.approx(r["fused_ms"] / r["torch_ms"], rel=1e-3) for r in ops_rows)
    inside = [r for r in ops_rows if cgm.fused_point_grads_auto(torch.float64, r["D"], r["na"], r["nb"])]
    # every measured point the rule takes is at or below 0.9 of the torch route, and the rule's corner points are measured
    assert all(r["ratio"] <= 0.9 for r in inside)
    if auto["min_pairs"] is None:
        assert not inside
    else:
        assert min(r["na"] * r["nb"] for r in inside) == auto["min_pairs"]
        assert max(r["D"] for r in inside) == auto["max_d"]
        assert not cgm.fused_point_grads_auto(torch.float32, 8, 4096, 4096)
        assert not cgm.fused_point_grads_auto(torch.float64, auto["max_d"] + 1, 4096, 4096)
        assert not cgm.fused_point_grads_auto(torch.float64, 8, 1, auto["min_pairs"] - 1)
