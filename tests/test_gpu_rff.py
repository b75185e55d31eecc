"""Random Fourier features and pathwise posterior samples on the GPU (csrc/rff.hip, cggp.rff,
cggp.models.PathwiseClusterGP).

Accuracy contract of the feature map (include/mgp.h): per feature |err| <= 8 u (1 + sum_d |x_d theta_d|), u the unit
roundoff of the dtype.  A sample sums 2L weighted features, so its bound is that contract summed over l with the
weights, plus the rounding of the 2L-term sum itself (statistically u sqrt(2L) times the sum of magnitudes; 4x that
is allowed) and of the final scaling.  Exact values are computed in np.longdouble from the same inputs.
"""

import math

import numpy as np
import pytest
import torch

from oracle import kernels as ok

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}


def dev():
    return torch.device("cuda:0")


def T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev())


def exact_parts(X, th, rows):
    """(cos, sin, sum_d |x_d theta_d|) in long double for the chosen rows: [r, L] each."""
    Xr = X[rows].astype(LD)
    thl = th.astype(LD)
    P = Xr @ thl.T
    Pabs = np.abs(Xr) @ np.abs(thl).T
    return np.cos(P), np.sin(P), Pabs


def spot_rows(N, rng, k=200, panel_rows=None):
    """The first and last row, k random ones and, for every multiple c of the panel route's row count inside N
    (`sample_panel_t` starts a new panel there: `out + i0`, `X + i0 * D`), the rows c - 1, c and c + 1."""
    if N <= k:
        return np.arange(N)
    seams = [] if not panel_rows else [i for c in range(panel_rows, N, panel_rows) for i in (c - 1, c, c + 1) if i < N]
    return np.unique(np.concatenate([[0, N - 1], rng.choice(N, k, replace=False), seams]).astype(np.int64))


def check_case(D, S, L, N, dtype, layout, route, monkeypatch, theta_kind="se", lscale=1.0, seed=0, twice=False,
               report=None, all_rows=False):
    """`twice`: both entry points are called a second time and must return the same bits.  `report`: a dict that
    receives the worst error / bound of the features and of the samples.  `all_rows`: every row of both results is
    compared with long double, not the rows of `spot_rows` (the default, for the large N of the cases below)."""
    from cggp import kernels, ops, rff

    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    if theta_kind == "se":
        th = rng.standard_normal((L, D)) / lscale
    else:  # Matern-1/2 law: Cauchy-tailed frequencies
        th = rff.basis_theta_parameter(kernels.Matern12(lengthscales=[lscale] * D), L, rng).numpy()
    W = rng.standard_normal((S, 2 * L))
    scale = math.sqrt(1.7 / max(L, 1))
    # the values the device sees
    X = X.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    th = th.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    W = W.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    if route is not None:
        monkeypatch.setenv("MGP_RFF_ROUTE", route)
    else:
        monkeypatch.delenv("MGP_RFF_ROUTE", raising=False)
    Xd, thd, Wd = T(X, dtype), T(th, dtype), T(W, dtype)
    out = ops.rff_sample(Xd, thd, Wd, scale, layout)
    phi = ops.rff_features(Xd, thd)
    torch.cuda.synchronize()
    assert out.shape == ((S, N) if layout == ops.ROWS else (N, S))
    assert phi.shape == (N, 2 * L)
    if twice:
        assert torch.equal(ops.rff_sample(Xd, thd, Wd, scale, layout), out)
        assert torch.equal(ops.rff_features(Xd, thd), phi)
    if N == 0:
        return None
    u = U[dtype]
    # rows of Phi per panel: 2^28 / (2 L elem) (csrc/rff.hip, sample_panel_t): 16384 at fp64 and 32768 at fp32 for L = 1024
    rows = spot_rows(N, rng, panel_rows=(1 << 28) // (2 * L * (4 if dtype == torch.float32 else 8)) if L else None)
    if all_rows:
        rows = np.arange(N, dtype=np.int64)
    cos, sin, Pabs = exact_parts(X, th, rows)
    # features
    feat_bound = 8 * u * (1 + Pabs)
    ph = phi[torch.from_numpy(rows).to(dev())].double().cpu().numpy()
    assert np.all(np.abs(ph[:, :L] - cos) <= feat_bound), float(np.max(np.abs(ph[:, :L] - cos) / feat_bound))
    assert np.all(np.abs(ph[:, L:] - sin) <= feat_bound), float(np.max(np.abs(ph[:, L:] - sin) / feat_bound))
    # samples [S, rows]
    Wc, Ws = W[:, :L].astype(LD), W[:, L:].astype(LD)
    ref = LD(scale) * (Wc @ cos.T + Ws @ sin.T)
    absw = np.abs(W[:, :L]) + np.abs(W[:, L:])  # [S, L]
    bound = scale * (absw @ (8 * u * (1 + Pabs)).T) + scale * u * (4 * math.sqrt(2 * L) + 2) * absw.sum(1)[:, None]
    got = out.double().cpu().numpy()
    got = got[:, rows] if layout == ops.ROWS else got[rows].T
    err = np.abs(got - ref.astype(np.float64))
    if report is not None:
        report["features"] = float(np.max(np.maximum(np.abs(ph[:, :L] - cos), np.abs(ph[:, L:] - sin)) / feat_bound))
        report["samples"] = float(np.max(err / bound))
    assert np.all(err <= bound), (D, S, L, N, str(dtype), route, float(np.max(err / bound)))
    return float(np.max(Pabs))


# (D, S, L, N): every D in {1, 8, 32, 77}, S in {1, 5, 8, 13}, L in {1, 100, 1024}, N in {0, 1, 257, 100 003}; the
# fused route (D <= 32, S <= 8; split over the bases when N is small), the panel route (S > 8 or D > 32, or forced)
CASES = [
    (1, 1, 1, 1, None),
    (8, 5, 1024, 257, None),        # fused, bases split over blockIdx.y
    (8, 5, 1024, 100_003, None),    # fused
    (32, 8, 100, 257, None),        # fused, D = 32
    (1, 8, 1024, 100_003, None),    # fused, D = 1
    (77, 5, 100, 257, None),        # panel (D > 32)
    (8, 13, 1024, 100_003, None),   # panel (S > 8)
    (77, 1, 1024, 1, None),         # panel, one row
    (32, 13, 1, 0, None),           # empty
    (8, 5, 100, 1, "panel"),        # panel forced where fused is eligible
    (32, 8, 1024, 257, "panel"),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=[f"D{c[0]}_S{c[1]}_L{c[2]}_N{c[3]}_{c[4] or 'auto'}" for c in CASES])
def test_rff_parity(case, dtype, monkeypatch):
    from cggp import ops
    D, S, L, N, route = case
    layout = ops.ROWS if (D + S + L) % 2 else ops.COLS
    check_case(D, S, L, N, dtype, layout, route, monkeypatch, seed=D * 131 + S * 17 + L)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route", [None, "panel"], ids=["fused", "panel"])
def test_rff_matern12_large_phases(dtype, route, monkeypatch):
    """Cauchy frequencies with lengthscale 1e-3: phases well above 1e5 rad, reduced exactly in revolutions."""
    from cggp import ops
    pmax = check_case(8, 5, 1024, 257, dtype, ops.ROWS, route, monkeypatch, theta_kind="matern12", lscale=1e-3,
                      seed=21)
    assert pmax > 1e5


def test_rff_deterministic(monkeypatch):
    from cggp import ops
    rng = np.random.default_rng(4)
    for N, S, route in ((257, 5, None), (100_003, 8, None), (3000, 13, None), (3000, 5, "panel")):
        if route:
            monkeypatch.setenv("MGP_RFF_ROUTE", route)
        else:
            monkeypatch.delenv("MGP_RFF_ROUTE", raising=False)
        X = T(rng.standard_normal((N, 8)), torch.float64)
        th = T(rng.standard_normal((1024, 8)), torch.float64)
        W = T(rng.standard_normal((S, 2048)), torch.float64)
        a = ops.rff_sample(X, th, W, 0.03)
        b = ops.rff_sample(X, th, W, 0.03)
        assert torch.equal(a, b)
        assert torch.equal(ops.rff_features(X, th), ops.rff_features(X, th))


def test_rff_edge_shapes_and_errors():
    from cggp import _hip, ops
    X = T(np.ones((5, 3)), torch.float64)
    th0 = torch.empty((0, 3), dtype=torch.float64, device=dev())
    W0 = torch.empty((2, 0), dtype=torch.float64, device=dev())
    z = ops.rff_sample(X, th0, W0, 1.0)  # L = 0: zeros
    assert z.shape == (2, 5) and torch.count_nonzero(z) == 0
    assert ops.rff_features(X, th0).shape == (5, 0)
    hd = _hip.get_handle(dev())
    th = T(np.ones((4, 3)), torch.float64)
    W = T(np.ones((2, 8)), torch.float64)
    out = torch.empty((2, 5), dtype=torch.float64, device=dev())
    p = _hip.ptr
    lib = hd.lib
    assert lib.mgp_rff_sample(hd.h, _hip.F64, p(X), 5, 3, p(th), 4, p(W), 0, 1.0, p(out), _hip.ROWS) == -2
    assert lib.mgp_rff_sample(hd.h, _hip.F64, p(X), 5, 0, p(th), 4, p(W), 2, 1.0, p(out), _hip.ROWS) == -2
    assert lib.mgp_rff_sample(hd.h, _hip.F64, p(X), -1, 3, p(th), 4, p(W), 2, 1.0, p(out), _hip.ROWS) == -2
    assert lib.mgp_rff_sample(hd.h, _hip.F64, p(X), 5, 3, p(th), 4, p(W), 2, 1.0, p(out), 7) == -1
    assert lib.mgp_rff_sample(hd.h, _hip.F64, p(X), 5, 3, p(th), 4, p(W), 2, float("nan"), p(out), _hip.ROWS) == -1
    assert lib.mgp_rff_sample(hd.h, 5, p(X), 5, 3, p(th), 4, p(W), 2, 1.0, p(out), _hip.ROWS) == -3
    assert lib.mgp_rff_features(hd.h, _hip.F64, p(X), 5, 3, p(th), 4, p(out), 7) == -2  # ld < 2L
    with pytest.raises(ValueError):
        ops.rff_sample(X, th, W[:, :7], 1.0)


# ---- PathwiseClusterGP

def numpy_pathwise(X, Z, u, lam, variance, ls, theta, W, xi, kind="se"):
    """Restatement of the reference's pathwise_samples (cggp/models.py:391-420) in numpy, [S, N]."""
    L = theta.shape[0]
    P = np.concatenate([X, Z], 0)
    ph = P @ theta.T
    prior = math.sqrt(variance / L) * W @ np.concatenate([np.cos(ph), np.sin(ph)], 1).T
    n = X.shape[0]
    fx, fz = prior[:, :n], prior[:, n:]
    eps = lam[None, :] * xi
    k = ok.Kernel(kind, variance, ls)
    A = k.K(Z) + np.diag(lam)
    w = np.linalg.solve(A, (u[None, :] - fz - eps).T)
    return fx + (k.K(X, Z) @ w).T, A


def make_model(Z, u, counts, noise, kern, **kw):
    from cggp import models
    return models.PathwiseClusterGP(kern, noise, T(Z, torch.float64), pseudo_u=T(u[:, None], torch.float64),
                                    cluster_counts=T(counts[:, None], torch.float64), **kw)


def test_pathwise_samples_against_numpy():
    from cggp import kernels
    from cggp.conjugate_gradient import ConjugateGradient
    rng = np.random.default_rng(12)
    N, M, D, L, S = 1000, 200, 4, 256, 5
    X = rng.standard_normal((N, D))
    Z = rng.standard_normal((M, D))
    u = np.sin(Z).sum(1)
    counts = rng.integers(1, 4, size=M).astype(np.float64)
    noise, variance, ls = 0.3, 1.0, np.array([1.0, 1.5, 0.8, 1.2])
    lam = noise / counts
    theta = rng.standard_normal((L, D)) / ls
    W = rng.standard_normal((S, 2 * L))
    xi = rng.standard_normal((S, M))
    ref, A = numpy_pathwise(X, Z, u, lam, variance, ls, theta, W, xi)
    ev = np.linalg.eigvalsh(A)
    assert ev[-1] / ev[0] <= 1e4  # cond(K_zz + Lambda)
    kern = kernels.SquaredExponential(variance=variance, lengthscales=ls)
    inj = dict(theta=torch.from_numpy(theta), weights=torch.from_numpy(W), xi=torch.from_numpy(xi))
    Xd = T(X, torch.float64)
    chol = make_model(Z, u, counts, noise, kern).pathwise_samples(Xd, L, S, **inj)
    assert chol.shape == (S, N, 1)
    scale = np.max(np.abs(ref))
    assert np.max(np.abs(chol[..., 0].cpu().numpy() - ref)) <= 1e-8 * scale
    kxz = ok.Kernel("se", variance, ls).K(X, Z)
    for thr in (1e-12, 1e-16):
        cg = make_model(Z, u, counts, noise, kern, conjugate_gradient=ConjugateGradient(thr, max_iterations=4 * M))
        got = cg.pathwise_samples(Xd, L, S, **inj)[..., 0].cpu().numpy()
        # CG stops at 0.5 ||r||^2 <= thr per column: its weights are off by at most ||A^-1|| sqrt(2 thr), which
        # reaches a sample through a row of K_xz.  At thr = 1e-12 that bound is ~2e-5 of the samples' scale (the
        # error measured on this problem: ~6e-8), at thr = 1e-16 it is ~2e-7 (measured: ~4e-10) and 1e-8 is held.
        cg_bound = np.linalg.norm(kxz, axis=1).max() * math.sqrt(2 * thr) / ev[0]
        err = np.max(np.abs(got - ref))
        assert err <= (cg_bound if thr > 1e-16 else 1e-8 * scale), (thr, err / scale, cg_bound / scale)


def test_pathwise_moments_match_predict_f():
    """epsilon="matheron": given theta the samples are Gaussian with mean exactly predict_f's mean (E W = 0, E eps = 0)
    and variance Var_theta = predict_f's variance + the random-feature error of k.  Tolerances (5 standard errors):
      mean:     5 sqrt(v_hat / S)                                     (Monte Carlo)
      variance: 5 v_hat sqrt(2 / (S - 1))                              (Monte Carlo, Gaussian sample variance)
              + 5 std_l(h_l) / sqrt(L)                                 (random features: Var_theta - var is the mean
                over the L bases of h_l = s2 (c_l^2 + s_l^2 - 2 (cos(theta_l x) c_l + sin(theta_l x) s_l)) minus its
                expectation, c_l = sum_m a_m cos(theta_l z_m), s_l likewise, a = (K_zz + Lambda)^-1 k_zx; this is
                the O(s2 sqrt(2 / L)) term, with its constant measured on the drawn bases)"""
    from cggp import kernels, rff
    rng = np.random.default_rng(31)
    D, M, n, L, S = 2, 32, 64, 4096, 2048
    g = np.linspace(-1.5, 1.5, 6)
    Z = np.array([[a, b] for a in g for b in g])[:M]
    X = rng.uniform(-2, 2, size=(n, D))
    u = np.sin(2 * Z[:, 0]) * np.cos(Z[:, 1])
    counts = np.full(M, 4.0)
    noise, variance, ls = 0.2, 1.0, np.array([0.7, 0.9])
    kern = kernels.SquaredExponential(variance=variance, lengthscales=ls)
    model = make_model(Z, u, counts, noise, kern, epsilon="matheron")
    Xd = T(X, torch.float64)
    theta = rff.basis_theta_parameter(kern, L, seed=5).numpy()
    samples = model.pathwise_samples(Xd, L, S, seed=6, theta=torch.from_numpy(theta))[..., 0].cpu().numpy()
    mu, var = model.predict_f(Xd)
    mu, var = mu[:, 0].cpu().numpy(), var[:, 0].cpu().numpy()
    m_hat, v_hat = samples.mean(0), samples.var(0, ddof=1)
    assert np.all(np.abs(m_hat - mu) <= 5 * np.sqrt(v_hat / S)), np.max(np.abs(m_hat - mu) / np.sqrt(v_hat / S))
    k = ok.Kernel("se", variance, ls)
    lam = noise / counts
    a = np.linalg.solve(k.K(Z) + np.diag(lam), k.K(Z, X))  # [M, n]
    cz, sz = np.cos(theta @ Z.T), np.sin(theta @ Z.T)  # [L, M]
    cx, sx = np.cos(theta @ X.T), np.sin(theta @ X.T)  # [L, n]
    c, s = cz @ a, sz @ a  # [L, n]
    h = variance * (c ** 2 + s ** 2 - 2 * (cx * c + sx * s))
    tol_v = 5 * v_hat * np.sqrt(2 / (S - 1)) + 5 * h.std(0) / np.sqrt(L)
    assert np.all(np.abs(v_hat - var) <= tol_v), np.max(np.abs(v_hat - var) / tol_v)


def test_pathwise_elbo_matches_its_samples():
    from cggp import kernels
    rng = np.random.default_rng(8)
    N, M, D = 300, 40, 3
    X = rng.standard_normal((N, D))
    y = np.sin(X).sum(1, keepdims=True)
    Z = X[:M]
    kern = kernels.Matern32(variance=1.2, lengthscales=[1.0, 0.7, 1.3])
    model = make_model(Z, np.zeros(M), np.ones(M), 0.1, kern, num_data=3 * N)
    Xd, yd = T(X, torch.float64), T(y, torch.float64)
    e1 = model.elbo((Xd, yd), num_bases=64, num_samples=3, seed=1)
    e2 = model.elbo((Xd, yd), num_bases=64, num_samples=3, seed=1)
    assert e1 == e2 and math.isfinite(e1)
    f = model.pathwise_samples(Xd, 64, 3, seed=1)
    lik = -0.5 * (((yd[None] - f) ** 2).sum().item() / 0.1 / 3 + N * math.log(2 * math.pi * 0.1))
    assert abs(e1 - (lik * 3 - model.prior_kl())) <= 1e-9 * abs(e1)


def test_pathwise_c3_size():
    """One call at C3 size: 2^20 rows, M = 4096, S = 5, L = 1024 (D = 8, fp64); finite, 1000 rows against numpy, peak
    extra device memory (torch allocations + libmgp workspace growth) below 1 GB."""
    from cggp import _hip, kernels
    N, M, D, L, S = 1 << 20, 4096, 8, 1024, 5
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, D))
    Z = X[rng.choice(N, M, replace=False)]
    u = np.sin(Z).sum(1) / math.sqrt(D)
    counts = rng.integers(50, 400, size=M).astype(np.float64)
    noise, ls = 0.1 * 256, np.ones(D)  # lambda = noise / counts in [0.064, 0.51]
    kern = kernels.SquaredExponential(variance=1.0, lengthscales=ls)
    model = make_model(Z, u, counts, noise, kern)
    theta = rng.standard_normal((L, D))
    W = rng.standard_normal((S, 2 * L))
    xi = rng.standard_normal((S, M))
    Xd = T(X, torch.float64)
    hd = _hip.get_handle(dev())
    torch.cuda.synchronize()
    ws0 = hd.lib.mgp_workspace_bytes(hd.h)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f = model.pathwise_samples(Xd, L, S, theta=torch.from_numpy(theta), weights=torch.from_numpy(W),
                               xi=torch.from_numpy(xi))
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base + (hd.lib.mgp_workspace_bytes(hd.h) - ws0)
    assert extra < 1 << 30, extra
    f = f[..., 0]
    assert f.shape == (S, N) and bool(torch.isfinite(f).all())
    rows = np.sort(rng.choice(N, 1000, replace=False))
    lam = noise / counts
    ref, _ = numpy_pathwise(X[rows], Z, u, lam, 1.0, ls, theta, W, xi)
    got = f[:, torch.from_numpy(rows).to(dev())].cpu().numpy()
    assert np.max(np.abs(got - ref)) <= 1e-8 * np.max(np.abs(ref))
