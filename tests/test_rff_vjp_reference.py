"""The long-double VJP reference of tests/rff_vjp_reference.py against central differences of its own forward pass,
and the torch panel expression of `training._rff_vjp_panels` (the route of `_RffSample` beyond D = 32 or S = 8) against
that reference.  CPU only."""

import numpy as np
import pytest
import torch

import rff_vjp_reference as rr

LD = np.longdouble


def problem(N, L, D, S, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    theta = spread * rng.standard_normal((L, D))
    W = rng.standard_normal((S, 2 * L))
    G = rng.standard_normal((S, N))
    return X, theta, W, 0.37, G


def test_reference_against_central_differences():
    """6 rows x 5 bases x 3 dimensions, 4 samples.  Step h = 2^-20 in long double (u = 2^-64): truncation
    h^2 / 6 |f'''| ~ 1e-13 |f'| for phases of order 1, rounding u |f| / h ~ 6e-14; 1e-10 of the largest derivative is held."""
    X, theta, W, scale, G = problem(6, 5, 3, 4, seed=1)
    dtheta, dX = rr.vjp(X, theta, W, scale, G)
    h = LD(2.0) ** -20
    Gl = G.astype(LD)
    loss = lambda Xv, tv: np.sum(Gl * rr.forward(Xv, tv, W, scale))
    for arr, grad, which in ((theta, dtheta, 1), (X, dX, 0)):
        fd = np.zeros(arr.shape, dtype=LD)
        for i in range(arr.shape[0]):
            for d in range(arr.shape[1]):
                up, dn = arr.astype(LD), arr.astype(LD)
                up[i, d] += h
                dn[i, d] -= h
                args_up = (X, up) if which else (up, theta)
                args_dn = (X, dn) if which else (dn, theta)
                fd[i, d] = (loss(*args_up) - loss(*args_dn)) / (2 * h)
        assert np.max(np.abs(fd - grad)) <= 1e-10 * np.max(np.abs(grad))


def test_reference_zero_cotangent_and_empty_sides():
    X, theta, W, scale, G = problem(7, 4, 2, 3, seed=2)
    dtheta, dX = rr.vjp(X, theta, W, scale, np.zeros_like(G))
    assert not dtheta.any() and not dX.any()
    dtheta, dX = rr.vjp(X[:0], theta, W, scale, G[:, :0])
    assert dtheta.shape == (4, 2) and not dtheta.any() and dX.shape == (0, 2)


def test_chunk_plan():
    # 1024 bases at D = 32 own four workgroups: 2^20 streamed rows go in 256 chunks of 4096 on 256 CUs
    assert rr.chunk_plan(1 << 20, 1024, 32, 256) == (4096, 256)
    assert rr.chunk_plan(1, 257, 8, 256) == (1, 1)
    assert rr.chunk_plan(33, 257, 8, 256) == (17, 2)
    assert rr.chunk_plan(70, 1, 3, 256) == (24, 3)  # 24 + 24 + 22: a ragged last chunk
    assert rr.chunk_plan(1024, 1 << 20, 8, 256) == (1024, 1)  # 2048 owner blocks: no split


@pytest.mark.parametrize("shape", [(6, 5, 3, 4), (300, 33, 40, 9), (257, 64, 33, 13), (1, 1, 1, 1)],
                         ids=lambda s: "N%d_L%d_D%d_S%d" % s)
def test_panel_expression_against_reference(shape, monkeypatch):
    """`_rff_vjp_panels` on host tensors (torch cos / sin, fp64) against long double.  Bound: the one of
    `rr.bounds` with libm's features (1 u each, inside the 8 u (1 + phase) allowance) and chains of at most N or L
    additions in the matrix products, i.e. u (8 (1 + pmax) + 4 S + 2 D + max(N, L) + 8) times the absolute terms."""
    from cggp import training
    N, L, D, S = shape
    X, theta, W, scale, G = problem(N, L, D, S, seed=sum(shape))
    monkeypatch.setattr(training, "PANEL_BYTES", 16 * L * 100)  # 100 rows per chunk: N = 300, 257 walk three chunks
    t = torch.from_numpy
    dtheta, dX = training._rff_vjp_panels(t(X), t(theta), t(W), scale, t(G), want_dX=True)
    rt, rx = rr.vjp(X, theta, W, scale, G)
    pmax = float(np.max(np.abs(X) @ np.abs(theta).T))
    A = abs(scale) * (np.abs(G).T @ (np.abs(W[:, :L]) + np.abs(W[:, L:])))
    fac = rr.U * (8 * (1 + pmax) + 4 * S + 2 * D + max(N, L) + 8)
    assert np.all(np.abs(dtheta.numpy() - rt.astype(np.float64)) <= fac * (A.T @ np.abs(X)))
    assert np.all(np.abs(dX.numpy() - rx.astype(np.float64)) <= fac * (A @ np.abs(theta)))
    only, none = training._rff_vjp_panels(t(X), t(theta), t(W), scale, t(G))
    assert none is None and torch.equal(only, dtheta)
