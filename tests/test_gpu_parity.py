"""GPU parity: every libmgp entry point, through the C ABI, against the CPU oracle.

Tolerance: the north star asks for 1e-6 fp64 relative error on CG residual and predictive
mean/variance; single kernel products are held to 1e-11 (fp64) / 2e-4 (fp32) relative to the
largest entry, CG-level results to 1e-6 or tighter as written at each assert.
"""

import numpy as np
import pytest
import torch

import assign_reference
from oracle import cg as ocg, cluster as oc, distance as od, kernels as ok, models as om

pytestmark = pytest.mark.gpu

KINDS = ["se", "matern12", "matern32", "matern52"]


def dev():
    return torch.device("cuda:0")


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def relerr(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    scale = np.max(np.abs(ref)) if ref.size else 1.0
    return float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))) / max(scale, 1e-300)) if ref.size else 0.0


def make_kernel(name, D, variance=1.3, seed=0):
    from cggp import kernels
    rng = np.random.default_rng(seed)
    ls = rng.random(D) ** 2 + 0.5
    cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
           "matern52": kernels.Matern52}[name]
    return cls(variance=variance, lengthscales=ls), ok.Kernel(name, variance, ls)


def points(N, M, D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, D)), rng.standard_normal((M, D))


# ------------------------------------------------------------------ library sanity
def test_library_loaded_and_arch():
    from cggp import _hip
    lib = _hip.load_library()
    assert lib.mgp_version() == _hip.MGP_VERSION and lib.mgp_build_arch() == b"gfx950"
    hd = _hip.get_handle(dev())
    assert hd.h


# ------------------------------------------------------------------ sweeps
@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("D", [1, 2, 3, 8, 17, 32])
def test_knm_kmn_matvec_fp64(name, D):
    from cggp import ops
    N, M, R = 1000, 77, 3
    k, ko = make_kernel(name, D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(2)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    spec = k.spec(D)
    # Matern12 = exp(-sqrt(r2)) has a cusp at 0: in 1-D some of the 77000 pairs are nearly
    # coincident and the rounding of GPflow's r2 expansion shows through the sqrt (reference too)
    tol = 1e-11 if name != "matern12" else 1e-9
    out = ops.knm_matvec(spec, T(X), T(Z), T(V))
    assert out.shape == (N, R) and relerr(out, K @ V) < tol
    out_t = ops.kmn_matvec(spec, T(X), T(Z), T(W))
    assert out_t.shape == (M, R) and relerr(out_t, K.T @ W) < tol


@pytest.mark.parametrize("R", [1, 2, 4, 5, 8, 13])
@pytest.mark.parametrize("layout", ["cols", "rows"])
def test_sweep_rhs_counts_and_layouts(R, layout):
    from cggp import ops
    N, M, D = 777, 300, 8
    k, ko = make_kernel("se", D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(3)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    spec = k.spec(D)
    if layout == "cols":
        a = ops.knm_matvec(spec, T(X), T(Z), T(V), ops.COLS)
        b = ops.kmn_matvec(spec, T(X), T(Z), T(W), ops.COLS)
        assert relerr(a, K @ V) < 1e-11 and relerr(b, K.T @ W) < 1e-11
    else:
        a = ops.knm_matvec(spec, T(X), T(Z), T(V.T), ops.ROWS)
        b = ops.kmn_matvec(spec, T(X), T(Z), T(W.T), ops.ROWS)
        assert a.shape == (R, N) and b.shape == (R, M)
        assert relerr(a, (K @ V).T) < 1e-11 and relerr(b, (K.T @ W).T) < 1e-11


@pytest.mark.parametrize("N,M", [(1, 1), (5, 1), (1, 5), (255, 257), (4097, 513), (20000, 64)])
def test_sweep_ragged_shapes(N, M):
    from cggp import ops
    D = 4
    k, ko = make_kernel("matern32", D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(4)
    V, W = rng.standard_normal((M, 1)), rng.standard_normal((N, 1))
    K = ko.K(X, Z)
    assert relerr(ops.knm_matvec(k.spec(D), T(X), T(Z), T(V)), K @ V) < 1e-11
    assert relerr(ops.kmn_matvec(k.spec(D), T(X), T(Z), T(W)), K.T @ W) < 1e-11


@pytest.mark.parametrize("N,M", [(1, 1), (5, 1), (1, 5), (255, 257), (4097, 513)])
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("name,D", [("se", 8), ("matern52", 16), ("matern32", 32)])
def test_sweep_ragged_shapes_several_right_hand_sides(N, M, R, name, D):
    """The multi-right-hand-side fast sweeps stream an even count (pad row with zero weights) and read the
    weights from a transposed copy: odd / tiny streamed sets in both directions, every RC instantiation."""
    from cggp import ops
    k, ko = make_kernel(name, D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(N + M + R)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    assert relerr(ops.knm_matvec(k.spec(D), T(X), T(Z), T(V)), K @ V) < 1e-11
    assert relerr(ops.kmn_matvec(k.spec(D), T(X), T(Z), T(W)), K.T @ W) < 1e-11


def test_sweep_empty_inputs():
    from cggp import ops
    D = 3
    k, _ = make_kernel("se", D)
    X, Z = points(10, 4, D)
    e = ops.knm_matvec(k.spec(D), T(X[:0]), T(Z), T(np.zeros((4, 2))))
    assert e.shape == (0, 2)
    z = ops.kmn_matvec(k.spec(D), T(X[:0]), T(Z), T(np.zeros((0, 2))))
    assert z.shape == (4, 2) and float(z.abs().max()) == 0.0
    z = ops.knm_matvec(k.spec(D), T(X), T(Z[:0]), T(np.zeros((0, 2))))
    assert z.shape == (10, 2) and float(z.abs().max()) == 0.0


@pytest.mark.parametrize("name", KINDS)
def test_sweep_fp32(name):
    from cggp import ops
    N, M, D, R = 3000, 200, 2, 2
    k, ko = make_kernel(name, D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(5)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    a = ops.knm_matvec(k.spec(D), T(X, torch.float32), T(Z, torch.float32), T(V, torch.float32))
    b = ops.kmn_matvec(k.spec(D), T(X, torch.float32), T(Z, torch.float32), T(W, torch.float32))
    assert a.dtype == torch.float32
    assert relerr(a, K @ V) < 2e-4 and relerr(b, K.T @ W) < 2e-4


@pytest.mark.parametrize("D,R", [(2, 1), (2, 3), (5, 2), (8, 1)])
def test_sweep_fp32_se_scaled_sums(D, R):
    """fp32 SE keeps the sums scaled by 2^|a|^2 while every owned point of a workgroup has |a|^2 < 64: workgroups
    that qualify, workgroups that do not (a block of owned points far from the origin), far streamed points (the
    general loop inside a scaled workgroup), and coincident points -- rows compared one by one so that a wrong
    scale on a few rows cannot hide in a norm."""
    from cggp import kernels, ops
    N, M = 5000, 700
    k = kernels.SquaredExponential(variance=1.3, lengthscales=[0.7] * D)
    ko = ok.Kernel("se", 1.3, np.full(D, 0.7))
    X, Z = points(N, M, D)
    X[1024:2048] += 9.0      # |a|^2 ~ D * 120 in log2 units: these row blocks do not scale their sums
    X[3000:3010] = 400.0     # far streamed points for the K_mn direction: the distance bound of their tile fails
    X[:50] = Z[:50]          # coincident points
    Z[600:] += 9.0
    rng = np.random.default_rng(11)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    f = torch.float32
    a = ops.knm_matvec(k.spec(D), T(X, f), T(Z, f), T(V, f)).double().cpu().numpy()
    b = ops.kmn_matvec(k.spec(D), T(X, f), T(Z, f), T(W, f)).double().cpu().numpy()
    ra, rb = K @ V, K.T @ W
    assert np.isfinite(a).all() and np.isfinite(b).all()
    # Row-wise bound of the fp32 expansion form itself (GPflow's in fp32 just as much): the exponent of pair (i,j)
    # is formed from terms of size |a_i|^2 + |b_j|^2 (log2 units), so term j of row i is off by about
    # eps32 * (1 + |a_i|^2 + |b_j|^2) * |w_j| k_ij.  A wrong scale factor on a row would miss this bound by orders.
    eps = float(np.finfo(np.float32).eps)
    c2 = 0.5 * np.log2(np.e) / 0.7 ** 2
    na2, nb2 = c2 * (X * X).sum(1), c2 * (Z * Z).sum(1)
    G = K * (1.0 + na2[:, None] + nb2[None, :])
    bound_a = 8 * eps * (G @ np.abs(V)) + 1e-30
    bound_b = 8 * eps * (G.T @ np.abs(W)) + 1e-30
    assert np.max(np.abs(a - ra) / bound_a) < 1.0
    assert np.max(np.abs(b - rb) / bound_b) < 1.0


def test_sweep_coincident_points_and_far_points():
    from cggp import ops
    D = 8
    k, ko = make_kernel("se", D)
    X, Z = points(300, 40, D)
    X[:40] = Z  # r = 0 exactly -> k = variance
    X[100:110] *= 50.0  # far away: exp underflows towards 0, no NaN
    V = np.ones((40, 1))
    out = ops.knm_matvec(k.spec(D), T(X), T(Z), T(V))
    assert torch.isfinite(out).all()
    assert relerr(out, ko.K(X, Z) @ V) < 1e-11


def test_sweep_tiny_lengthscale_takes_the_clamped_path():
    """Scaled distances beyond 2^19 switch the tile to the clamped exp2 loop (no int32 wrap of the
    table index): everything underflows to 0 except coincident points, which give the variance."""
    from cggp import kernels, ops
    D = 8
    k = kernels.SquaredExponential(variance=1.3, lengthscales=[1e-3] * D)
    ko = ok.Kernel("se", 1.3, np.full(D, 1e-3))
    X, Z = points(600, 300, D)
    X[:300] = Z
    V = np.random.default_rng(0).standard_normal((300, 2))
    out = ops.knm_matvec(k.spec(D), T(X), T(Z), T(V))
    assert torch.isfinite(out).all()
    # |a|^2 ~ 1e7 in scaled units: the expansion's rounding (eps * |a|^2 ~ 1e-9) is what is left
    # of r2 = 0 at the coincident points, in the reference's formula as much as here
    assert relerr(out, ko.K(X, Z) @ V) < 1e-7
    assert float(out[300:].abs().max()) == 0.0
    # mixed tile: a few far rows next to ordinary ones
    k2, ko2 = make_kernel("se", D)
    X2, Z2 = points(700, 260, D)
    X2[5] *= 1e4
    Z2[7] *= 1e4
    out2 = ops.kmn_matvec(k2.spec(D), T(X2), T(Z2), T(np.ones((700, 1))))
    assert relerr(out2, ko2.K(X2, Z2).T @ np.ones((700, 1))) < 1e-11


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("D", [33, 40, 90])
def test_generic_dimension_path(name, D):
    """D > 32 leaves the fused register-resident sweeps: explicit panels + NT GEMM, same results."""
    from cggp import kernels as gk, ops
    from cggp.conjugate_gradient import ConjugateGradient, SgprNormalOperator
    N, M, R = 700, 90, 3
    k, ko = make_kernel(name, D)
    # keep scaled distances O(1) in high dimension so the kernel values are not all ~0
    for d in range(D):
        k.lengthscales[d] *= np.sqrt(D)
    ko.lengthscales = ko.lengthscales * np.sqrt(D)
    X, Z = points(N, M, D)
    rng = np.random.default_rng(2)
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    K = ko.K(X, Z)
    assert np.max(np.abs(K)) > 1e-3
    spec = k.spec(D)
    assert relerr(k.K(T(X), T(Z)), K) < 1e-12
    # (Matern12 diagonal: the oracle's expansion leaves ~1e-8 noise at coincident points, the
    # generic path uses direct differences and returns the variance exactly)
    dtol = 1e-12 if name != "matern12" else 3e-7
    assert relerr(gk.Kuu(T(Z), k, jitter=1e-3, diag_add=T(np.ones(M))), ko.K(Z) + (1 + 1e-3) * np.eye(M)) < dtol
    assert relerr(ops.knm_matvec(spec, T(X), T(Z), T(V)), K @ V) < 1e-11
    assert relerr(ops.kmn_matvec(spec, T(X), T(Z), T(W)), K.T @ W) < 1e-11
    assert relerr(ops.knm_matvec(spec, T(X), T(Z), T(V.T), ops.ROWS), (K @ V).T) < 1e-11
    assert relerr(ops.kmn_knm(spec, T(X), T(Z)), K.T @ K) < 1e-11
    op = SgprNormalOperator(k, T(X), T(Z), 0.1, jitter=1e-6)
    S = om.SgprNormalOperator(X, Z, ko, 0.1, jitter=1e-6).dense()
    assert relerr(op.dense(), S) < 1e-9  # matern12 again (Z are not rows of X here, but near-ties exist)
    rhs = rng.standard_normal((M, 2))
    sol = ConjugateGradient(1e-14, max_iterations=3000)(op, T(rhs))
    assert relerr(sol, np.linalg.solve(S, rhs)) < 1e-6
    # the k^2 column sum (diag of K_mn K_nm) above the fused limit: explicit panels, ordered partial sums
    assert relerr(ops.kmn_sq_colsum(spec, T(X), T(Z)), np.sum(K * K, axis=0)) < 1e-12
    assert relerr(op.diag(), np.diag(S)) < 1e-9


# ------------------------------------------------------------------ dense K
@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_k_dense(name, dtype):
    from cggp import kernels as gk
    D = 5
    k, ko = make_kernel(name, D)
    X, Z = points(333, 70, D)
    tol = 1e-12 if dtype == torch.float64 else 3e-5
    Kd = k.K(T(X, dtype), T(Z, dtype))
    assert Kd.shape == (333, 70) and relerr(Kd, ko.K(X, Z)) < tol
    lam = np.random.default_rng(0).random(70) + 0.1
    Kuu = gk.Kuu(T(Z, dtype), k, jitter=1e-3, diag_add=T(lam, dtype))
    ref = ok.Kuu(Z, ko, 1e-3) + np.diag(lam)
    # Matern12 is exp(-sqrt(r2)): at coincident points GPflow's expansion leaves r2 ~ eps*|a|^2
    # instead of 0 and the sqrt turns that into ~1e-8 (fp64) / ~3e-4 (fp32) of k -- in the
    # reference as much as here, so the diagonal only agrees to that level.
    dtol = tol if name != "matern12" else (3e-7 if dtype == torch.float64 else 3e-3)
    assert relerr(Kuu, ref) < dtol
    off = ~np.eye(70, dtype=bool)
    assert relerr(Kuu.cpu().numpy()[off], ref[off]) < tol
    assert relerr(gk.Kuf(T(Z, dtype), k, T(X, dtype)), ok.Kuf(Z, ko, X)) < tol
    assert float((k.K_diag(T(X, dtype)) - k.variance).abs().max()) == 0.0
    if dtype == torch.float64:
        # symmetry, and variance on the diagonal up to the rounding of GPflow's expansion
        # |a|^2 + |b|^2 - 2 a.b at a == b (a few ulp of |a|^2, not exactly 0)
        Kzz = k.K(T(Z))
        assert float((Kzz - Kzz.t()).abs().max()) < 1e-15
        assert float((Kzz.diagonal() - k.variance).abs().max()) < (1e-13 if name != "matern12" else 3e-7)


def test_add_diagonal():
    from cggp.utils import add_diagonal
    A = T(np.arange(9.0).reshape(3, 3))
    out = add_diagonal(A, T(np.array([1.0, 2.0, 3.0])))
    assert np.array_equal(out.cpu().numpy(), np.arange(9.0).reshape(3, 3) + np.diag([1.0, 2.0, 3.0]))
    assert np.array_equal(A.cpu().numpy(), np.arange(9.0).reshape(3, 3))


# ------------------------------------------------------------------ symmetric product
@pytest.mark.parametrize("n", [1, 7, 64, 129, 512, 1001])
@pytest.mark.parametrize("Bt", [1, 2, 3, 5, 8, 9, 64, 130, 300])
def test_symm_matmul_fp64(n, Bt):
    from cggp import ops
    rng = np.random.default_rng(6)
    A = rng.standard_normal((n, n))
    A = A + A.T
    P = rng.standard_normal((Bt, n))
    out = ops.symm_matmul(T(A), T(P))
    assert out.shape == (Bt, n) and relerr(out, P @ A) < 1e-12


@pytest.mark.parametrize("n", [64, 128, 256, 257, 300, 1000, 1280, 2047, 2048, 3072, 4001, 4608])
@pytest.mark.parametrize("Bt", [17, 32, 33, 48, 64, 65, 100, 128])
def test_symm_matmul_pipelined_form(n, Bt, monkeypatch):
    """n >= 256 and 16 < Bt <= 128 take the software-pipelined kernel (64-wide k steps up to Bt = 64, 32-wide
    beyond; step counts per slice covering every
    remainder of its loop unrolled by three; Bt not a multiple of 16 exercises the clamped panel rows; n not a
    multiple of 64 / of 4 the element-wise partial step and the element-aligned vector loads).
    Checked against numpy and, bit for bit, against the round-1 form run on a second handle."""
    import ctypes
    from cggp import _hip, ops
    rng = np.random.default_rng(n + Bt)
    A = rng.standard_normal((n, n))
    A = A + A.T
    P = rng.standard_normal((Bt, n))
    At, Pt = T(A), T(P)
    out = ops.symm_matmul(At, Pt)
    assert relerr(out, P @ A) < 1e-12
    monkeypatch.setenv("MGP_SKINNY_PIPE", "0")
    hd = _hip.Handle(At.device.index or 0)
    hd.sync_stream()
    ref = torch.empty_like(Pt)
    hd.check(hd.lib.mgp_symm_matmul(hd.h, _hip.dtype_code(At), _hip.ptr(At), n, _hip.ptr(Pt), Bt, _hip.ptr(ref)))
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@pytest.mark.parametrize("n,Bt", [(4001, 2100), (1001, 700), (4001, 300), (530, 129), (999, 1000)])
def test_symm_matmul_ragged_gemm_regime(n, Bt):
    """Bt > 128 with n not a multiple of 16 (or of 2): the GEMM's element-aligned vector loads and its element-wise
    partial last step -- full-grid form (4001 x 2100), sliced forms, and a last slice shorter than the others."""
    from cggp import ops
    rng = np.random.default_rng(n * 7 + Bt)
    A = rng.standard_normal((n, n))
    A = A + A.T
    P = rng.standard_normal((Bt, n))
    out = ops.symm_matmul(T(A), T(P))
    assert relerr(out, P @ A) < 1e-12
    out32 = ops.symm_matmul(T(A, torch.float32), T(P, torch.float32))
    assert relerr(out32, P @ A) < 2e-4


@pytest.mark.parametrize("Bt", [1, 8, 33, 200])
def test_symm_matmul_fp32(Bt):
    from cggp import ops
    rng = np.random.default_rng(7)
    n = 300
    A = rng.standard_normal((n, n))
    A = A + A.T
    P = rng.standard_normal((Bt, n))
    out = ops.symm_matmul(T(A, torch.float32), T(P, torch.float32))
    assert relerr(out, P @ A) < 1e-4


@pytest.mark.parametrize("n", [1024, 1030, 1091, 2048, 4096])
@pytest.mark.parametrize("dt,tol", [(torch.float64, 1e-13), (torch.float32, 2e-5)])
def test_symm_gemv_upper_triangle_path(n, dt, tol):
    """One RHS, n >= 1024: the product reads only the upper-triangular 64x64 tiles and the last
    workgroup per chunk sums the contributions.  Repeated launches check that the arrival
    counters are reset, bit-equal outputs that the summation order is fixed; the strictly lower
    triangle is poisoned to show it is never read."""
    from cggp import ops
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    A = A + A.T
    P = rng.standard_normal((1, n))
    ref = P @ A
    At = T(A, dt)
    out1 = ops.symm_matmul(At, T(P, dt))
    out2 = ops.symm_matmul(At, T(P, dt))
    assert relerr(out1, ref) < tol
    assert torch.equal(out1, out2)
    Ap = A.copy()
    il = np.tril_indices(n, -64)  # everything below the diagonal tiles
    Ap[il] = np.nan
    out3 = ops.symm_matmul(T(Ap, dt), T(P, dt))
    assert torch.equal(out1, out3)
    P2 = rng.standard_normal((1, n))
    assert relerr(ops.symm_matmul(At, T(P2, dt)), P2 @ A) < tol


def test_symm_matmul_asymmetric_b_layout_check():
    """A = I with an asymmetric P catches a swapped C/D map in the MFMA epilogue."""
    from cggp import ops
    n, Bt = 160, 140
    P = np.arange(Bt * n, dtype=np.float64).reshape(Bt, n)
    out = ops.symm_matmul(T(np.eye(n)), T(P))
    assert np.array_equal(out.cpu().numpy(), P)


@pytest.mark.parametrize("name,D,R", [("se", 8, 1), ("matern32", 2, 5), ("matern52", 3, 70)])
def test_kmm_lambda_matvec(name, D, R):
    from cggp import ops
    k, ko = make_kernel(name, D)
    rng = np.random.default_rng(21)
    Z = rng.standard_normal((300, D))
    lam = rng.uniform(0.01, 0.5, 300)
    V = rng.standard_normal((R, 300))
    out = ops.kmm_lambda_matvec(k.spec(D), T(Z), T(lam), T(V))
    assert relerr(out, V @ (ko.K(Z) + np.diag(lam))) < 1e-11


# ------------------------------------------------------------------ contraction
@pytest.mark.parametrize("name,D", [("se", 8), ("matern32", 32), ("matern12", 3)])
def test_kmn_knm(name, D):
    from cggp import ops
    N, M = 5000, 200
    k, ko = make_kernel(name, D)
    X, Z = points(N, M, D)
    K = ko.K(X, Z)
    out = ops.kmn_knm(k.spec(D), T(X), T(Z))
    assert out.shape == (M, M) and relerr(out, K.T @ K) < 1e-11
    assert float((out - out.t()).abs().max()) == 0.0


def test_kmn_knm_fp32_and_ragged():
    from cggp import ops
    N, M, D = 3001, 130, 2
    k, ko = make_kernel("se", D)
    X, Z = points(N, M, D)
    K = ko.K(X, Z)
    out = ops.kmn_knm(k.spec(D), T(X, torch.float32), T(Z, torch.float32))
    assert relerr(out, K.T @ K) < 2e-4


# ------------------------------------------------------------------ reductions
def test_colwise_dot_and_dot_all():
    from cggp import ops
    rng = np.random.default_rng(8)
    A, B = rng.standard_normal((300, 77)), rng.standard_normal((300, 77))
    assert relerr(ops.colwise_dot(T(A), T(B)), np.sum(A * B, axis=0)) < 1e-13
    assert abs(ops.dot_all(T(A), T(B)) - np.sum(A * B)) < 1e-10


# ------------------------------------------------------------------ CG (row CG1, CG3-CG5)
def cg_problem(n=100, d=2, nsys=5, seed=0, noise=0.1 ** 2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    ls = rng.random(d) ** 2 + 0.5
    kern = ok.Kernel("se", 1.3, ls)
    A = om.add_diagonal(kern.K(X), noise * np.ones(n))
    rhs = rng.standard_normal((n, nsys))
    return A, rhs


def test_cg_reference_test_config():
    """cggp/cg_test.py:12-46: CG vs direct solve at the reference's own size and tolerance."""
    from cggp.conjugate_gradient import ConjugateGradient
    A, rhs = cg_problem()
    cg = ConjugateGradient(1e-12)
    sol, (steps, err) = cg.solve_with_stats(T(A), T(rhs))
    ref = np.linalg.solve(A, rhs)
    np.testing.assert_allclose(sol.cpu().numpy(), ref, rtol=1e-3, atol=1e-4)  # cg_test.py:43
    o_sol, (o_steps, o_err) = ocg.ConjugateGradient(1e-12).solve_with_stats(A, rhs)
    assert abs(int(steps) - o_steps) <= 2
    assert relerr(sol, o_sol) < 1e-6
    assert err.shape == (5, 1)


@pytest.mark.parametrize("Bt", [1, 4, 9, 40])
@pytest.mark.parametrize("k,kind", [(1, "se"), (3, "se"), (5, "se"), (8, "se"), (30, "wellcond")])
def test_cg_fixed_iterations_match_oracle(Bt, k, kind):
    """Line-by-line equivalence: after exactly k steps (thr = 0, cap = k) the iterate and the
    CG residual statistic 0.5*rz agree with the oracle far below the 1e-6 north-star bar.

    CG trajectories on SE kernel matrices are chaotic in floating point: the oracle run against
    ITSELF on a symmetrically permuted copy of the same system (only the summation order changes)
    differs by 5e-7 after 15 steps and 5e-4 after 30 (measured on this very problem).  So the
    step-for-step comparison uses few steps on the SE system and 30 steps on a well-conditioned
    SPD matrix, where rounding differences stay small."""
    from cggp.conjugate_gradient import conjugate_gradient
    A, rhs = cg_problem(n=200, nsys=Bt, noise=0.1)
    if kind == "wellcond":
        Q = np.random.default_rng(9).standard_normal((200, 200))
        A = Q @ Q.T / 200 + 2.0 * np.eye(200)
    z = torch.zeros((Bt, 200), dtype=torch.float64, device=dev())
    sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), z, 0.0, max_iterations=k)
    o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs.T, np.zeros((Bt, 200)), 0.0, max_iterations=k)
    assert int(steps) == k == o_steps
    assert relerr(sol, o_sol) < 1e-9
    assert np.max(np.abs(err.cpu().numpy() - o_err) / o_err) < 1e-6  # CG residual, 1e-6 relative


@pytest.mark.parametrize("thr", [1e-6, 1e-10, 1e-14])
@pytest.mark.parametrize("Bt", [1, 4, 9, 40])
def test_cg_matches_oracle(thr, Bt):
    """Converged solves.  Where the loop stops depends on rounding (finite-precision CG loses
    orthogonality, so two correct implementations cross the threshold a step or two apart); what
    is pinned is the stopping quantity itself and the distance to the exact solution that the
    threshold implies: ||v - A^-1 b|| <= ||A^-1|| * sqrt(2 thr) for both."""
    from cggp.conjugate_gradient import conjugate_gradient
    A, rhs = cg_problem(n=200, nsys=Bt, noise=0.1)
    sol, (steps, err) = conjugate_gradient(T(A), T(rhs.T), torch.zeros((Bt, 200), dtype=torch.float64, device=dev()),
                                           thr, max_iterations=200)
    o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs.T, np.zeros((Bt, 200)), thr, max_iterations=200)
    assert sol.shape == (Bt, 200) and err.shape == (Bt, 1)
    assert abs(int(steps) - o_steps) <= 4 and int(steps) < 200
    r = rhs.T - sol.cpu().numpy() @ A
    assert np.all(0.5 * np.sum(r * r, -1) <= thr * (1 + 1e-6) + 1e-20)
    exact = np.linalg.solve(A, rhs).T
    bound = np.linalg.norm(np.linalg.inv(A), 2) * np.sqrt(2 * thr) * 1.001 + 1e-9
    assert np.max(np.linalg.norm(sol.cpu().numpy() - exact, axis=1)) <= bound
    assert np.max(np.linalg.norm(o_sol - exact, axis=1)) <= bound
    if thr <= 1e-14:
        assert relerr(sol, o_sol) < 1e-6


def test_cg_cap_any_zero_rhs_initial_solution():
    from cggp.conjugate_gradient import ConjugateGradient, conjugate_gradient
    A, rhs = cg_problem(n=60, nsys=3)
    z = torch.zeros((3, 60), dtype=torch.float64, device=dev())
    # iteration cap
    _, (steps, _) = conjugate_gradient(T(A), T(rhs.T), z, 0.0, max_iterations=7)
    assert int(steps) == 7
    # zero rhs: no step, zero solution, zero error
    sol, (steps, err) = conjugate_gradient(T(A), z, z.clone(), 1e-6)
    assert int(steps) == 0 and float(sol.abs().max()) == 0.0 and float(err.abs().max()) == 0.0
    # a zero RHS beside live ones stays exactly zero (gamma guard, conjugate_gradient.py:68)
    b = rhs.T.copy()
    b[0] = 0.0
    sol, _ = conjugate_gradient(T(A), T(b), z.clone(), 1e-16, max_iterations=300)
    assert float(sol[0].abs().max()) == 0.0 and torch.isfinite(sol).all()
    # exact initial solution: zero steps
    ref = np.linalg.solve(A, rhs)
    _, (steps, _) = ConjugateGradient(1e-10).solve_with_stats(T(A), T(rhs), initial_solution=T(ref))
    assert int(steps) == 0
    # near initial solution + refresh cycle: same answer as the oracle with the same settings
    cg = ConjugateGradient(1e-14, max_iterations=400, max_steps_cycle=5)
    sol, (steps, _) = cg.solve_with_stats(T(A), T(rhs), initial_solution=T(ref + 1e-3))
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-14, max_iterations=400, max_steps_cycle=5).solve_with_stats(
        A, rhs, initial_solution=ref + 1e-3)
    assert abs(int(steps) - o_steps) <= 2 and relerr(sol, o_sol) < 1e-7


def test_cg_guard_floor_matches_oracle():
    """Below the reference's guard floor CG stalls; the device loop must stall the same way."""
    from cggp.conjugate_gradient import ConjugateGradient
    A, rhs = cg_problem(n=100, noise=1.0)
    sol, (steps, err) = ConjugateGradient(1e-26, max_iterations=150).solve_with_stats(T(A), T(rhs))
    o_sol, (o_steps, o_err) = ocg.ConjugateGradient(1e-26, max_iterations=150).solve_with_stats(A, rhs)
    assert int(steps) == 150 == o_steps
    assert relerr(sol, o_sol) < 1e-8
    assert float(err.max()) < 1e-15


@pytest.mark.parametrize("pre", ["jacobi", "block", "dense"])
def test_cg_preconditioners(pre):
    from cggp.conjugate_gradient import (BlockPreconditioner, ConjugateGradient, DensePreconditioner,
                                         JacobiPreconditioner)
    A, rhs = cg_problem(n=64, noise=0.1)
    if pre == "jacobi":
        P, Po = JacobiPreconditioner(), ocg.JacobiPreconditioner()
    elif pre == "dense":
        E = np.random.default_rng(5).standard_normal((64, 8))
        Pinv = np.linalg.inv(A + 0.05 * E @ E.T)
        Pinv = 0.5 * (Pinv + Pinv.T)
        P, Po = DensePreconditioner(T(Pinv)), ocg.DensePreconditioner(Pinv)
    else:
        blocks = np.arange(64).reshape(8, 8)
        P, Po = BlockPreconditioner(blocks), ocg.BlockPreconditioner(blocks)
    sol, (steps, _) = ConjugateGradient(1e-14, preconditioner=P, max_iterations=300).solve_with_stats(T(A), T(rhs))
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-14, preconditioner=Po, max_iterations=300).solve_with_stats(A, rhs)
    assert abs(int(steps) - o_steps) <= 2 and relerr(sol, o_sol) < 1e-7
    assert relerr(sol, np.linalg.solve(A, rhs)) < 1e-5
    z, rz = P(T(rhs.T), T(A))
    zo, rzo = Po(rhs.T, A)
    assert relerr(z, zo) < 1e-10 and relerr(rz, rzo) < 1e-10


@pytest.mark.parametrize("n,bt,cycle", [(64, 1, 100), (200, 5, 7), (333, 130, 100)])
def test_cg_dense_preconditioner_steps(n, bt, cycle):
    """Fixed-iteration parity of the dense-preconditioned loop (start-up, step and refresh paths,
    GEMV / skinny / GEMM regimes of the z = r @ Pinv product)."""
    from cggp.conjugate_gradient import DensePreconditioner, conjugate_gradient
    rng = np.random.default_rng(n)
    A, _ = cg_problem(n=n, noise=0.1)
    rhs = rng.standard_normal((bt, n))
    E = rng.standard_normal((n, n // 4))
    Pinv = np.linalg.inv(A + 0.2 * E @ E.T / n)
    Pinv = 0.5 * (Pinv + Pinv.T)
    v0 = 0.1 * rng.standard_normal((bt, n))
    for k in (1, 3, 9):
        sol, (steps, err) = conjugate_gradient(T(A), T(rhs), T(v0), 0.0, DensePreconditioner(T(Pinv)),
                                               max_iterations=k, max_steps_cycle=cycle)
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, v0, 0.0, ocg.DensePreconditioner(Pinv),
                                                         max_iterations=k, max_steps_cycle=cycle)
        assert int(steps) == o_steps == k
        assert relerr(sol, o_sol) < 1e-9, (k, relerr(sol, o_sol))
        assert relerr(err, o_err) < 1e-6


def test_sgpr_subsampled_preconditioner():
    """PCG on the SGPR normal system: same solution as the closed form, far fewer steps than Eye."""
    from cggp.conjugate_gradient import ConjugateGradient, SgprNormalOperator, SubsampledNormalPreconditioner
    from cggp import kernels as ck
    rng = np.random.default_rng(11)
    N, M, D = 6000, 128, 3
    X = rng.uniform(-2, 2, (N, D))
    Z = X[rng.choice(N, M, replace=False)].copy()
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    kern = ck.SquaredExponential(variance=1.3, lengthscales=[0.9, 1.1, 0.8])
    okern = ok.Kernel("se", 1.3, np.array([0.9, 1.1, 0.8]))
    s2 = 0.05
    op = SgprNormalOperator(kern, T(X), T(Z), s2, jitter=1e-6)
    Kmn = okern.K(Z, X)
    S = s2 * (okern.K(Z, Z) + 1e-6 * np.eye(M)) + Kmn @ Kmn.T
    b = Kmn @ y
    ref = np.linalg.solve(S, b)
    P = SubsampledNormalPreconditioner(op, rows_per_inducing=16, seed=0)
    assert P.sample_rows == 16 * M
    sol, (steps, err) = ConjugateGradient(1e-10, preconditioner=P, max_iterations=400).solve_with_stats(op, T(b))
    _, (steps_eye, err_eye) = ConjugateGradient(1e-10, max_iterations=400).solve_with_stats(op, T(b))
    assert float(err.max()) <= 1e-10 * 10 and int(steps) < 60
    assert int(steps) * 3 < int(steps_eye)
    # residual-level agreement with the closed form (S is ill conditioned: compare S sol with b)
    assert np.max(np.abs(S @ sol.cpu().numpy() - b)) < 1e-3 * np.max(np.abs(b)) * 1e-2
    # and against the oracle's PCG with the very same P^-1
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-10, preconditioner=ocg.DensePreconditioner(
        P.inverse.cpu().numpy()), max_iterations=400).solve_with_stats(S, b)
    assert abs(int(steps) - o_steps) <= 3
    assert np.max(np.abs(S @ (sol.cpu().numpy() - o_sol))) < 1e-4 * np.max(np.abs(b)) * 1e-2


def test_sgpr_subsampled_preconditioner_fp32():
    """fp32 operator: P is factorised in fp64 and applied in fp32; the solve reaches the fp32 floor
    of the system in a few steps where the identity-preconditioned one stalls far above it."""
    from cggp.conjugate_gradient import ConjugateGradient, SgprNormalOperator, SubsampledNormalPreconditioner
    from cggp import kernels as ck
    rng = np.random.default_rng(12)
    N, M, D = 20000, 256, 2
    X = rng.uniform(-3, 3, (N, D))
    Z = X[rng.choice(N, M, replace=False)].copy()
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    kern = ck.SquaredExponential(variance=1.0, lengthscales=[1.0, 1.0])
    okern = ok.Kernel("se", 1.0, np.ones(2))
    op = SgprNormalOperator(kern, T(X, torch.float32), T(Z, torch.float32), 0.1, jitter=1e-4)
    Kmn = okern.K(Z, X)
    S = 0.1 * (okern.K(Z, Z) + 1e-4 * np.eye(M)) + Kmn @ Kmn.T
    b = Kmn @ y
    P = SubsampledNormalPreconditioner(op, rows_per_inducing=32)
    assert P.inverse.dtype == torch.float32
    bt = T(b, torch.float32)
    sol, (steps, _) = ConjugateGradient(0.0, preconditioner=P, max_iterations=30).solve_with_stats(op, bt)
    sol_eye, _ = ConjugateGradient(0.0, max_iterations=30).solve_with_stats(op, bt)
    res = np.linalg.norm(S @ sol.double().cpu().numpy() - b) / np.linalg.norm(b)
    res_eye = np.linalg.norm(S @ sol_eye.double().cpu().numpy() - b) / np.linalg.norm(b)
    assert res < 5e-4 and res < 0.1 * res_eye, (res, res_eye)


def test_pcg_abi_rejects_incomplete_preconditioners():
    """Error convention of the C ABI: a preconditioner struct without its payload is MGP_E_BADARG
    with a message, the Python shim raises; a mismatched dense inverse is refused before the call."""
    from cggp import _hip
    from cggp.conjugate_gradient import (CGPreconditioner, ConjugateGradient, DenseOperator, DensePreconditioner,
                                         as_operator)
    A, rhs = cg_problem(n=32, noise=0.1)

    class Broken(CGPreconditioner):
        def __init__(self, kind):
            self.kind = kind

        def _native(self, op):
            st = _hip.MgpPrecond()
            st.kind = self.kind
            return st, ()

    for kind in (_hip.PRE_DENSE, _hip.PRE_JACOBI, _hip.PRE_BLOCK, 17):
        with pytest.raises(RuntimeError, match="preconditioner"):
            ConjugateGradient(1e-6, preconditioner=Broken(kind))(T(A), T(rhs))
    with pytest.raises(ValueError):
        ConjugateGradient(1e-6, preconditioner=DensePreconditioner(T(np.eye(31))))(T(A), T(rhs))
    with pytest.raises(ValueError):
        DensePreconditioner(T(np.ones((4, 5))))
    assert isinstance(as_operator(T(A)), DenseOperator)


def test_cg_fp32():
    from cggp.conjugate_gradient import ConjugateGradient
    A, rhs = cg_problem(n=80, noise=0.5)
    sol = ConjugateGradient(1e-6)(T(A, torch.float32), T(rhs, torch.float32))
    assert relerr(sol, np.linalg.solve(A, rhs)) < 5e-3


def test_cg_custom_gradient():
    """conjugate_gradient.py:100-118: db = CG(A, dx), dA = -solution^T db (cg_test.py:34-46)."""
    from cggp.conjugate_gradient import conjugate_gradient
    A, rhs = cg_problem(n=40, noise=0.1)
    At = T(A).requires_grad_(True)
    bt = T(rhs.T).requires_grad_(True)
    sol, _ = conjugate_gradient(At, bt, None, 1e-15, max_iterations=400)
    sol.sum().backward()
    Ainv1 = np.linalg.solve(A, np.ones((40, 5)))
    assert relerr(bt.grad, Ainv1.T) < 1e-6
    assert relerr(At.grad, -np.linalg.solve(A, rhs) @ Ainv1.T) < 1e-6


def test_cg_custom_gradient_proportional_shortcut():
    """loss = c * sum(rhs * CG(A, rhs)): the incoming dx is c * rhs, so c * solution solves the backward
    system with residual c * r.  It is returned as is only while c^2 * err still meets the reference's
    absolute rule (conjugate_gradient.py:59-62); for a large scale (the ELBO's num_data/batch factor) it
    becomes the warm start of the second solve.  Gradients equal the closed form
    d/dB = 2c A^-1 B, d/dA = -c (A^-1 B)(A^-1 B)^T either way."""
    from cggp.conjugate_gradient import conjugate_gradient
    A, rhs = cg_problem(n=40, noise=0.1)
    X = np.linalg.solve(A, rhs)
    for c, thr in ((1.0, 1e-15), (3.0, 1e-14), (1e4, 1e-14)):
        At = T(A).requires_grad_(True)
        bt = T(rhs.T).requires_grad_(True)
        b0, w0 = conjugate_gradient.backward_shortcuts, conjugate_gradient.backward_warm_starts
        sol, (_, err) = conjugate_gradient(At, bt, None, thr, max_iterations=400)
        (c * (sol * bt.detach()).sum()).backward()
        took_short = conjugate_gradient.backward_shortcuts - b0
        took_warm = conjugate_gradient.backward_warm_starts - w0
        assert took_short + took_warm == 1
        # the rule itself: shortcut iff c^2 * err_b <= thr for every row
        assert bool(took_short) == bool((c * c * err <= thr).all().item())
        if c >= 1e4:
            assert took_warm == 1  # 1e8 * err cannot meet 1e-14: the reference would have re-solved
        assert relerr(bt.grad, c * X.T) < 1e-6
        assert relerr(At.grad, -c * X @ X.T) < 1e-6
    # a loss that is not of that form takes the full second solve
    At = T(A).requires_grad_(True)
    b0, w0 = conjugate_gradient.backward_shortcuts, conjugate_gradient.backward_warm_starts
    sol, _ = conjugate_gradient(At, T(rhs.T), None, 1e-15, max_iterations=400)
    (sol ** 2).sum().backward()
    assert (conjugate_gradient.backward_shortcuts, conjugate_gradient.backward_warm_starts) == (b0, w0)
    assert relerr(At.grad, -2.0 * X @ np.linalg.solve(A, X).T) < 1e-6


def test_nan_inputs_propagate():
    """GPflow's tf.exp / tf.maximum keep a NaN distance NaN (the reference's check_numerics relies on a
    non-finite ELBO to stop a diverged run, optimize.py:359-360): a NaN row of X gives NaN in K and in
    the fused products, for every kernel, and does not leak into other rows."""
    from cggp import kernels, ops
    rng = np.random.default_rng(2)
    X = rng.standard_normal((300, 3))
    Z = rng.standard_normal((20, 3))
    X[7, 1] = np.nan
    v = rng.standard_normal((20, 2))
    for cls in (kernels.SquaredExponential, kernels.Matern12, kernels.Matern32, kernels.Matern52):
        for dt in (torch.float64, torch.float32):
            k = cls(1.3, [0.7, 1.0, 1.4])
            K = k.K(T(X, dt), T(Z, dt))
            assert torch.isnan(K[7]).all() and torch.isfinite(K[:7]).all() and torch.isfinite(K[8:]).all()
            u = ops.knm_matvec(k.spec(3), T(X, dt), T(Z, dt), T(v, dt))
            assert torch.isnan(u[7]).all() and torch.isfinite(u[:7]).all() and torch.isfinite(u[8:]).all()
            t = ops.kmn_matvec(k.spec(3), T(X, dt), T(Z, dt), T(rng.standard_normal((300, 1)), dt))
            assert torch.isnan(t).all()  # every column sum contains the NaN row


def test_eval_logdet():
    """cggp/cg_test.py:49-77: forward 0, backward = d logdet."""
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import eval_logdet, eval_logdet_grad
    A, _ = cg_problem(n=50, noise=0.1)
    cg = ConjugateGradient(1e-15, max_iterations=500)
    At = T(A).requires_grad_(True)
    val = eval_logdet(At, cg)
    assert float(val) == 0.0
    (2.0 * val).backward()
    assert relerr(At.grad, 2.0 * np.linalg.inv(A)) < 1e-6
    probes = om.rademacher(50, 6, seed=4)
    G = eval_logdet_grad(T(A), cg, 1.0, probes=T(probes))
    Go = om.eval_logdet_grad(A, ocg.ConjugateGradient(1e-15, max_iterations=500), 1.0, probes=probes)
    assert relerr(G, Go) < 1e-6


# ------------------------------------------------------------------ operators
def test_kmm_lambda_operator():
    from cggp.conjugate_gradient import ConjugateGradient, KmmLambdaOperator
    D, M = 3, 90
    k, ko = make_kernel("matern52", D)
    _, Z = points(1, M, D)
    lam = np.random.default_rng(0).random(M) + 0.05
    op = KmmLambdaOperator(k, T(Z), T(lam))
    Aref = ko.K(Z) + np.diag(lam)
    assert relerr(op.dense(), Aref) < 1e-12
    rhs = np.random.default_rng(1).standard_normal((M, 2))
    sol = ConjugateGradient(1e-14, max_iterations=600)(op, T(rhs))
    assert relerr(sol, np.linalg.solve(Aref, rhs)) < 1e-6


@pytest.mark.parametrize("name", ["se", "matern32"])
def test_sgpr_operator_and_cg(name):
    from cggp.conjugate_gradient import ConjugateGradient, SgprNormalOperator
    N, M, D = 2000, 48, 4
    k, ko = make_kernel(name, D)
    X, Z = points(N, M, D)
    op = SgprNormalOperator(k, T(X), T(Z), 0.1, jitter=1e-6)
    oop = om.SgprNormalOperator(X, Z, ko, 0.1, jitter=1e-6)
    S = oop.dense()
    assert relerr(op.dense(), S) < 1e-11
    V = np.random.default_rng(2).standard_normal((M, 3))
    assert relerr(op.matmul(T(V)), S @ V) < 1e-11
    rhs = ko.K(Z, X) @ np.sin(X[:, :1])
    sol, (steps, _) = ConjugateGradient(1e-14, max_iterations=2000).solve_with_stats(op, T(rhs))
    o_sol, (o_steps, _) = ocg.ConjugateGradient(1e-14, max_iterations=2000).solve_with_stats(oop, rhs)
    assert relerr(sol, o_sol) < 1e-6
    r = rhs - S @ sol.cpu().numpy()
    assert 0.5 * float(np.sum(r * r)) <= 1e-14 * 1.01 + 1e-16 or int(steps) == 2000
    # fixed number of steps: same iterate
    sol5, _ = ConjugateGradient(0.0, max_iterations=8).solve_with_stats(op, T(rhs))
    o_sol5, _ = ocg.ConjugateGradient(0.0, max_iterations=8).solve_with_stats(oop, rhs)
    assert relerr(sol5, o_sol5) < 1e-9


def test_sgpr_kmm_product_beside_the_sweep_at_small_sizes():
    """For slabs of Kmm of 48 MB and more the SGPR operator runs its s2*Kmm.p product on a stream of its own beside the
    K_nm sweep and takes it as the addend of the K_mn sweep (csrc/cg.hip; C3: the whole 134 MB).  MGP_SGPR_KMM_ASIDE=2
    forces that route at every size: the operator / CG tests above and the rank-sharded solve (row slabs of Kmm, the
    agreement word written by the slab product) must hold on it unchanged."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(root, "tests", "test_gpu_parity.py"),
                          os.path.join(root, "tests", "test_distributed.py"), "-k",
                          "sgpr_operator_and_cg or sgpr_cg_model or sgpr_solve_paths or sharded_sgpr_cg_on_one_gpu"],
                         env=dict(os.environ, MGP_SGPR_KMM_ASIDE="2"), capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]


# ------------------------------------------------------------------ models
def model_problem(name="se", N=600, D=2, M=40, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    y = np.sin(X).sum(1, keepdims=True) + 0.3 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)]
    k, ko = make_kernel(name, D, variance=1.1)
    idx = oc.nearest_centre_sqdist(Z, X)
    u, counts = oc.cluster_stats(idx, y, M)
    return X, y, Z, k, ko, u, counts


@pytest.mark.parametrize("name", KINDS)
def test_cggp_predict_f(name):
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP, ClusterGP
    X, y, Z, k, ko, u, counts = model_problem(name)
    # CG threshold 1e-15 (near the reference's guard floor): where the loop stops no longer
    # matters and the 1e-6 north-star bar on mean/variance is meaningful
    # (and enough iterations to get there: the default cap of n steps does not converge these)
    m = CGGP(k, 0.1, T(Z), ConjugateGradient(1e-15, max_iterations=3000), num_probes=None, pseudo_u=T(u),
             cluster_counts=T(counts))
    ref = om.CGGP(ko, 0.1, Z, ocg.ConjugateGradient(1e-15, max_iterations=3000), num_probes=None, pseudo_u=u,
                  cluster_counts=counts)
    Xs = X[:257]
    mu, var = m.predict_f(T(Xs))
    mu0, var0 = ref.predict_f(Xs)
    assert mu.shape == (257, 1) and var.shape == (257, 1)
    assert relerr(mu, mu0) < 1e-6 and relerr(var, var0) < 1e-6  # north-star tolerance
    c = m.predict_f(T(Xs[:9]), full_cov=True)[1]
    assert c.shape == (1, 9, 9) and relerr(c, ref.predict_f(Xs[:9], full_cov=True)[1]) < 1e-6
    # Cholesky twin (models.py:250-276) on the device agrees with the oracle twin
    tw = ClusterGP(k, 0.1, T(Z), pseudo_u=T(u), cluster_counts=T(counts))
    tw0 = om.ClusterGP(ko, 0.1, Z, pseudo_u=u, cluster_counts=counts)
    tmu, tvar = tw.predict_f(T(Xs))
    tmu0, tvar0 = tw0.predict_f(Xs)
    assert relerr(tmu, tmu0) < 1e-7 and relerr(tvar, tvar0) < 1e-7
    # batched prediction == one shot
    bmu, bvar = m.predict_f_batched(T(Xs), 100)
    # (the "any" stopping rule makes the step count depend on which rows share a batch)
    assert relerr(bmu, mu.cpu().numpy()) < 1e-9 and relerr(bvar, var.cpu().numpy()) < 1e-6
    # one CG against the identity shared by all batches == per-batch CG (and the Cholesky twin)
    smu, svar = m.predict_f_batched(T(Xs), 100, shared_inverse=True)
    assert relerr(smu, mu.cpu().numpy()) < 1e-9 and relerr(svar, var.cpu().numpy()) < 1e-6
    assert relerr(svar, tvar0) < 1e-6
    assert relerr(m.q_moments()[0], ref.q_moments()[0]) < 1e-6
    assert relerr(m.diag_variance, ref.diag_variance) < 1e-15
    # the reference's default threshold (cdgp_class, cli_utils.py:439: 1e-6 on 0.5||r||^2): both
    # implementations sit within the error that threshold allows around the Cholesky twin
    md = CGGP(k, 0.1, T(Z), ConjugateGradient(1e-6), num_probes=None, pseudo_u=T(u), cluster_counts=T(counts))
    rd = om.CGGP(ko, 0.1, Z, ocg.ConjugateGradient(1e-6), num_probes=None, pseudo_u=u, cluster_counts=counts)
    dmu, dvar = md.predict_f(T(Xs))
    dmu0, dvar0 = rd.predict_f(Xs)
    e_ref = max(relerr(dmu0, tmu0), relerr(dvar0, tvar0))
    assert relerr(dmu, tmu0) < 3 * e_ref + 1e-4 and relerr(dvar, tvar0) < 3 * e_ref + 1e-4


def test_cggp_prior_kl_and_elbo():
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP, ClusterGP, rmse_nlpd
    X, y, Z, k, ko, u, counts = model_problem("se")
    cg, cgo = ConjugateGradient(1e-12, max_iterations=2000), ocg.ConjugateGradient(1e-12, max_iterations=2000)
    m = CGGP(k, 0.1, T(Z), cg, num_probes=None, pseudo_u=T(u), cluster_counts=T(counts), num_data=600)
    ref = om.CGGP(ko, 0.1, Z, cgo, num_probes=None, pseudo_u=u, cluster_counts=counts, num_data=600)
    assert abs(m.prior_kl() - ref.prior_kl()) / abs(ref.prior_kl()) < 1e-6
    e, e0 = m.elbo((T(X[:100]), T(y[:100]))), ref.elbo((X[:100], y[:100]))
    assert abs(e - e0) / abs(e0) < 1e-6
    # Hutchinson branch with injected probes (models.py:308-314)
    probes = om.rademacher(40, 5, seed=4)
    m.num_probes = ref.num_probes = 5
    kl, kl0 = m.prior_kl(probes=T(probes)), ref.prior_kl(probes=probes)
    assert abs(kl - kl0) / abs(kl0) < 1e-6
    # the documented default stream reproduces numpy's PCG64
    from cggp.models import rademacher
    assert np.array_equal(rademacher((40, 5), torch.float64, dev(), 4).cpu().numpy(), probes)
    # twin: value differs from CGGP's exactly by the omitted 0.5 log|Kmm+Lambda|
    tw = ClusterGP(k, 0.1, T(Z), pseudo_u=T(u), cluster_counts=T(counts))
    tw0 = om.ClusterGP(ko, 0.1, Z, pseudo_u=u, cluster_counts=counts)
    assert abs(tw.prior_kl() - tw0.prior_kl()) / abs(tw0.prior_kl()) < 1e-8
    # metrics
    m.num_probes = None
    rmse, nlpd = rmse_nlpd(m, (T(X[:200]), T(y[:200])), batch_size=64)
    mu0, var0 = ref.predict_f(X[:200])
    r0, n0 = om.rmse_nlpd(mu0, var0, y[:200], 0.1)
    assert abs(rmse - r0) / r0 < 1e-6 and abs(nlpd - n0) / abs(n0) < 1e-6


def test_sgpr_cg_model():
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import SGPR
    X, y, Z, k, ko, u, counts = model_problem("se", N=1500, M=30)
    m = SGPR((T(X), T(y)), k, T(Z), 0.1, ConjugateGradient(1e-12, max_iterations=5000), jitter=1e-6)
    ref = om.SGPR((X, y), ko, Z, 0.1, jitter=1e-6)
    Xs = X[:100] + 0.1
    mu, var = m.predict_f(T(Xs))
    mu0, var0 = ref.predict_f(Xs)
    # north star: 1e-6 on predictive mean AND variance.  With the model's default ("auto") preconditioner CG
    # on S acts as iterative refinement of a factorised solve and meets it with room (measured at C1 against
    # the longdouble oracle: 7e-11 matrix-free, 2e-8 through the explicit S; tools/dbg/sgpr_var.py)
    assert relerr(mu, mu0) < 1e-6 and relerr(var, var0) < 1e-6
    e, e0 = m.elbo(), ref.elbo()
    assert abs(e - e0) / abs(e0) < 1e-8
    _, cov = m.predict_f(T(Xs[:20]), full_cov=True)
    _, cov0 = ref.predict_f(Xs[:20], full_cov=True)
    assert cov.shape == (1, 20, 20) and relerr(cov, cov0) < 1e-6


@pytest.mark.parametrize("pre,explicit,kmm", [(None, 0, "cg"), ("auto", 0, "cholesky"), (None, 8, "cholesky"),
                                              ("auto", 8, "cg")])
def test_sgpr_solve_paths(pre, explicit, kmm):
    """Matrix-free / explicit-S solves, with and without the subsampled preconditioner: the same
    predictions as the two-Cholesky closed form."""
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import SGPR
    X, y, Z, k, ko, u, counts = model_problem("matern32", N=4000, M=40)
    m = SGPR((T(X), T(y)), k, T(Z), 0.1, ConjugateGradient(1e-13, max_iterations=5000), jitter=1e-6,
             preconditioner=pre, explicit_rhs=explicit, kmm_solver=kmm)
    ref = om.SGPR((X, y), ko, Z, 0.1, jitter=1e-6)
    Xs = X[:50] + 0.05
    mu, var = m.predict_f(T(Xs))
    mu0, var0 = ref.predict_f(Xs)
    # the un-preconditioned recurrence on S (cond ~ cond(Kmm)^2) stalls at the reference's guard floor
    #  before the variance reaches 1e-6: that is the reference algorithm's own limit, kept
    # as a selectable path; the default path is held to the north star's 1e-6
    assert relerr(mu, mu0) < 1e-6 and relerr(var, var0) < (1e-6 if pre == "auto" else 1e-5)
    assert (m._S is not None) == (explicit > 0)
    steps = int(m.solver().last_stats[0])
    if pre == "auto":
        assert steps < 40, steps  # the identity-preconditioned solve takes hundreds here


@pytest.mark.parametrize("N,M,C", [(5000, 37, 1), (5000, 37, 4), (100, 300, 3), (70000, 512, 2)])
def test_cluster_stats_sorted_and_sweep_agree(N, M, C):
    """The two forms of the per-cluster sums (fused N x M sweep, and stable sort + segmented sums)
    against the oracle: counts exact, sums to rounding, both deterministic run to run."""
    from cggp import ops
    rng = np.random.default_rng(N + M)
    idx = rng.integers(0, M, N)
    idx[idx == 3] = 4  # an empty cluster
    Y = rng.standard_normal((N, C))
    ref = np.zeros((M, C))
    np.add.at(ref, idx, Y)
    cnt = np.bincount(idx, minlength=M).astype(np.float64)
    it = torch.from_numpy(idx).to("cuda:0")
    for method in ("sweep", "sorted", "auto"):
        sums, counts = ops.cluster_stats(it, T(Y if C > 1 else Y[:, 0]), M, method=method)
        assert sums.shape == ((M, C) if C > 1 else (M,))
        assert np.array_equal(counts.cpu().numpy(), cnt)
        assert relerr(sums.reshape(M, C), ref) < 1e-12
        again, _ = ops.cluster_stats(it, T(Y if C > 1 else Y[:, 0]), M, method=method)
        assert torch.equal(sums, again)
    with pytest.raises(ValueError):
        ops.cluster_stats(it + M, T(Y), M, method="sorted")


# ------------------------------------------------------------------ F1: assignment + stats
@pytest.mark.parametrize("dist", ["sqeuclidean", "euclidean", "covariance", "correlation"])
def test_nearest_center(dist):
    from cggp import ops
    N, M, D = 3000, 70, 3
    k, ko = make_kernel("matern32", D)
    X, Z = points(N, M, D)
    idx, best = ops.nearest_center(k.spec(D), T(X), T(Z), distance_type=dist)
    idx = idx.cpu().numpy()
    if dist == "sqeuclidean":
        d_all = ok.square_distance(Z, X).T
    else:
        fn = od.create_distance_fn(ko, dist)
        d_all = fn((Z[None, :, :], X[:, None, :]))
    chosen = d_all[np.arange(N), idx]
    # every row: no correct evaluation can prefer another centre (tests/assign_reference.py), which pins the index
    # exactly wherever the long-double distances decide it; the chosen distance is always the minimum
    rep = assign_reference.check_assignment(f"nearest_center {dist}", ops.DIST_TYPES[dist], "matern32", 1.3,
                                            ko.lengthscales, X, Z, idx, best.cpu().numpy())
    assert np.array_equal(idx[rep.decided], rep.ref_idx[rep.decided]) and rep.decided.mean() >= 0.97
    assert np.max(np.abs(chosen - d_all.min(1))) < 1e-10
    assert relerr(best, chosen) < 1e-9


@pytest.mark.parametrize("dist", ["sqeuclidean", "euclidean", "covariance", "correlation"])
@pytest.mark.parametrize("D", [33, 77, 90])
def test_nearest_center_any_dimension(dist, D):
    """Row F1 above the fused limit (the reference's `buzz` has D = 77, `song` D = 90, cli_utils.py:72-86; its
    assignment is dimension-free, optimize.py:41-98): the index sequence is the oracle's, exactly."""
    from cggp import ops
    N, M = 3001, 70  # neither a multiple of the 64-wide tiles
    k, ko = make_kernel("matern32", D)
    for d in range(D):
        k.lengthscales[d] *= np.sqrt(D)
    ko.lengthscales = ko.lengthscales * np.sqrt(D)
    X, Z = points(N, M, D)
    Z[:5] = X[:5]  # coincident points: distance exactly 0 for `euclidean` (norm of differences)
    idx, best = ops.nearest_center(k.spec(D), T(X), T(Z), distance_type=dist)
    idx = idx.cpu().numpy()
    if dist == "sqeuclidean":
        d_all = ok.square_distance(Z, X).T
    else:
        fn = od.create_distance_fn(ko, dist)
        d_all = fn((Z[None, :, :], X[:, None, :]))
    assert np.array_equal(idx, np.argmin(d_all, axis=1))
    chosen = d_all[np.arange(N), idx]
    assert np.max(np.abs(best.cpu().numpy() - chosen)) < 1e-9 * max(1.0, np.max(np.abs(chosen)))
    if dist == "euclidean":
        assert np.all(best.cpu().numpy()[:5] == 0.0)
    # ties: duplicated centres -> the FIRST index wins (argmin semantics)
    Zd = np.vstack([Z, Z])
    idx2 = ops.nearest_center(k.spec(D), T(X), T(Zd), distance_type=dist, return_distance=False).cpu().numpy()
    assert np.array_equal(idx2, idx)


def test_nearest_center_any_dimension_fp32_and_the_update_functions():
    from cggp import kernels, ops
    from cggp.models import ClusterGP
    from cggp.optimize import kmeans_update_inducing_parameters, oips_update_inducing_parameters
    D, N, M = 77, 5000, 100
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, D))
    Z = X[rng.choice(N, M, replace=False)]
    y = np.sin(X[:, :3]).sum(1, keepdims=True)
    k = kernels.SquaredExponential(1.0, [np.sqrt(D)] * D)
    ref_idx = oc.nearest_centre_sqdist(Z, X)
    i32 = ops.nearest_center(k.spec(D), T(X, torch.float32), T(Z, torch.float32), return_distance=False).cpu().numpy()
    assert np.mean(i32 == ref_idx) > 0.995  # fp32 rounding moves only numerical near-ties
    u, counts = oc.cluster_stats(ref_idx, y, M)
    m = ClusterGP(k, 0.1, T(Z))
    _, means, c = oips_update_inducing_parameters(m, (T(X), T(y)), T(Z))
    assert relerr(means, u) < 1e-12 and relerr(c, counts) == 0.0
    _, means_k, c_k = kmeans_update_inducing_parameters(m, (T(X), T(y)), "euclidean", T(Z))
    assert relerr(c_k, counts) == 0.0 and relerr(means_k, u) < 1e-12


def test_cluster_stats_and_update():
    from cggp import kernels, ops
    from cggp.models import ClusterGP
    from cggp.optimize import kmeans_update_inducing_parameters, oips_update_inducing_parameters
    X, y, Z, k, ko, u, counts = model_problem("se", N=5000, M=64)
    idx = ops.nearest_center(k.spec(2), T(X), T(Z), return_distance=False)
    sums, cnt = ops.cluster_stats(idx, T(y), 64)
    ref_idx = oc.nearest_centre_sqdist(Z, X)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    assert relerr(cnt, np.bincount(ref_idx, minlength=64)) == 0.0
    assert relerr(sums, np.bincount(ref_idx, weights=y[:, 0], minlength=64)) < 1e-13
    m = ClusterGP(k, 0.1, T(Z))
    iv, means, c = oips_update_inducing_parameters(m, (T(X), T(y)), T(Z))
    assert relerr(means, u) < 1e-12 and relerr(c, counts) == 0.0
    # an empty cluster: count -> 1 (optimize.py:70), mean NaN (reduce_mean of nothing)
    Z2 = np.vstack([Z, [[100.0, 100.0]]])
    _, means2, c2 = oips_update_inducing_parameters(m, (T(X), T(y)), T(Z2))
    assert float(c2[-1]) == 1.0 and bool(torch.isnan(means2[-1]))
    _, means3, c3 = kmeans_update_inducing_parameters(m, (T(X), T(y)), "euclidean", T(Z2))
    assert float(c3[-1]) == 0.0


def test_distance_functions():
    from cggp.distance import create_distance_fn, euclid_distance
    rng = np.random.default_rng(0)
    x, yv = rng.standard_normal((5, 3)), rng.standard_normal((5, 3))
    for name in KINDS:
        k, ko = make_kernel(name, 3)
        for dt in ("euclidean", "covariance", "correlation"):
            got = create_distance_fn(k, dt)((T(x), T(yv)))
            assert relerr(got, od.create_distance_fn(ko, dt)((x, yv))) < 1e-12
    assert create_distance_fn(k, "euclidean") is euclid_distance


# ------------------------------------------------------------------ error behaviour
def test_errors_are_loud():
    from cggp import ops
    from cggp._hip import MgpError
    k, _ = make_kernel("se", 3)
    X, Z = points(10, 4, 3)
    with pytest.raises(RuntimeError):
        ops.knm_matvec(k.spec(3), torch.from_numpy(X), T(Z), T(np.zeros((4, 1))))  # CPU tensor
    with pytest.raises(ValueError):
        ops.knm_matvec(k.spec(3), T(X), T(Z), T(np.zeros((5, 1))))  # wrong M
    with pytest.raises(TypeError):
        ops.knm_matvec(k.spec(3), T(X), T(Z, torch.float32), T(np.zeros((4, 1))))
    with pytest.raises(ValueError):
        k.spec(600).struct(1)  # D > MGP_MAX_D
    assert issubclass(MgpError, RuntimeError)


# ------------------------------------------------------------------ row F4: parameter I/O, reports
def test_parameter_io_and_condition_report(tmp_path):
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP
    from cggp.utils import covariance_properties, load_params, multiple_assign, parameter_dict, store_params
    X, y, Z, k, ko, u, counts = model_problem("matern32")
    m = CGGP(k, 0.1, T(Z), ConjugateGradient(1e-10), num_probes=None, pseudo_u=T(u), cluster_counts=T(counts))
    p = parameter_dict(m)
    assert set(p) == {".kernel.variance", ".kernel.lengthscales", ".likelihood.variance", ".inducing_variable.Z",
                      ".pseudo_u", ".cluster_counts"}
    store_params(tmp_path / "params.npz", p)
    q = load_params(tmp_path / "params.npz")
    k2, _ = make_kernel("matern32", 2, variance=9.0, seed=5)
    m2 = CGGP(k2, 0.7, T(Z * 0), ConjugateGradient(1e-10), num_probes=None)
    multiple_assign(m2, q)
    a, b = m.predict_f(T(X[:40])), m2.predict_f(T(X[:40]))
    assert relerr(b[0], a[0].cpu().numpy()) < 1e-12 and relerr(b[1], a[1].cpu().numpy()) < 1e-12
    rep = covariance_properties(m, jitter=1e-6)
    ev = np.linalg.eigvalsh(ok.Kuu(Z, ko, 1e-6))
    assert abs(rep["condition_number"] - ev.max() / ev.min()) / (ev.max() / ev.min()) < 1e-6
    rep2 = covariance_properties(m, with_lambda=True)
    ev2 = np.linalg.eigvalsh(ok.Kuu(Z, ko) + np.diag(0.1 / counts[:, 0]))
    assert abs(rep2["eig_min"] - ev2.min()) < 1e-9 and abs(rep2["eig_max"] - ev2.max()) < 1e-8


def test_lpsvgp_base_class():
    """`cggp/models.py:51-173`: the base of the reference's class tree (free nu and diag_variance)."""
    from cggp.models import LpSVGP
    X, y, Z, k, ko, u, counts = model_problem("matern52")
    rng = np.random.default_rng(0)
    nu, dv = rng.standard_normal((40, 1)), rng.random((40, 1)) + 0.05
    m = LpSVGP(k, 0.2, T(Z), nu=T(nu), diag_variance=T(dv), num_data=600)
    r = om.LpSVGP(ko, 0.2, Z, nu=nu, diag_variance=dv, num_data=600)
    mu, var = m.predict_f(T(X[:77]))
    mu0, var0 = r.predict_f(X[:77])
    assert relerr(mu, mu0) < 1e-10 and relerr(var, var0) < 1e-9
    assert relerr(m.predict_f(T(X[:5]), full_cov=True)[1], r.predict_f(X[:5], full_cov=True)[1]) < 1e-9
    assert abs(m.prior_kl() - r.prior_kl()) / abs(r.prior_kl()) < 1e-9
    e, e0 = m.elbo((T(X[:100]), T(y[:100]))), r.elbo((X[:100], y[:100]))
    assert abs(e - e0) / abs(e0) < 1e-9
    d = LpSVGP(k, 0.2, T(Z))  # defaults: nu = 0, diag_variance = 1e-4 (:93-94)
    assert float(d.nu.abs().max()) == 0.0 and float((d.diag_variance - 1e-4).abs().max()) == 0.0


def test_cg_start_up_ignores_stale_arena_contents():
    """The CG state arena is reused between solves: a dense-preconditioned solve must not read what an
    earlier solve (here: one on a NaN matrix, in the other dtype) left in it.  Found by
    tests/test_gpu_configs.py: p = 0 * stale + z turned stale Inf/NaN bit patterns into NaN."""
    from cggp.conjugate_gradient import DensePreconditioner, conjugate_gradient
    rng = np.random.default_rng(31)
    n = 96
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T + n * np.eye(n)
    b = rng.standard_normal((3, n))
    Pinv = np.linalg.inv(A + np.diag(rng.uniform(0, 1, n)))
    Pinv = 0.5 * (Pinv + Pinv.T)
    bad = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev())
    conjugate_gradient(bad, torch.from_numpy(b).to(dev()), None, 1e-12, max_iterations=3)  # poisons r, p, Ap
    A32, b32 = torch.from_numpy(A.astype(np.float32)).to(dev()), torch.from_numpy(b.astype(np.float32)).to(dev())
    pre = DensePreconditioner(torch.from_numpy(Pinv.astype(np.float32)).to(dev()))
    sol, (k, err) = conjugate_gradient(A32, b32, None, 1e-10, pre, max_iterations=20, max_steps_cycle=4)
    assert torch.isfinite(sol).all() and int(k) >= 2
    ref = np.linalg.solve(A, b.T).T
    assert np.max(np.abs(sol.cpu().numpy() - ref)) / np.max(np.abs(ref)) < 1e-4


def test_sgpr_caches_follow_parameter_updates():
    """`update_fn` / `multiple_assign` / `assign_inducing_parameters` change Z and the hyper-parameters
    from outside the model (cggp/cli_utils.py:394-411, paper_cli_uci.py:123-124): predictions and the
    bound afterwards must be those of a freshly built SGPR, not a mix of new Z and cached alpha / Kmm /
    K_mn K_nm."""
    from cggp import kernels
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import SGPR
    from cggp.optimize import assign_inducing_parameters
    from cggp.utils import multiple_assign
    rng = np.random.default_rng(17)
    N, D, M = 700, 2, 24
    X, y = rng.standard_normal((N, D)), rng.standard_normal((N, 1))
    Z0, Z1 = X[:M].copy(), X[M:2 * M + 5].copy()  # the update also changes M
    Xs = T(X[::7])

    def fresh(Z, var, ls, s2):
        return SGPR((T(X), T(y)), kernels.Matern32(var, ls), T(Z), s2, ConjugateGradient(1e-14, max_iterations=4000),
                    jitter=1e-6)

    m = fresh(Z0, 1.0, [1.0, 1.0], 0.1)
    mu0, var0 = m.predict_f(Xs)
    e0 = m.elbo()
    # 1. new inducing points (and a new M) through the reference's update path
    assign_inducing_parameters(m, T(Z1), None, None)
    ref = fresh(Z1, 1.0, [1.0, 1.0], 0.1)
    mu, var = m.predict_f(Xs)
    rmu, rvar = ref.predict_f(Xs)
    assert relerr(mu, rmu.cpu().numpy()) < 1e-9 and relerr(var, rvar.cpu().numpy()) < 1e-9
    assert abs(m.elbo() - ref.elbo()) < 1e-9 * abs(ref.elbo())
    assert relerr(mu, mu0.cpu().numpy()) > 1e-6  # and they did change
    # 2. new hyper-parameters in place
    multiple_assign(m, {".kernel.variance": 1.7, ".kernel.lengthscales": np.array([0.6, 1.4]),
                        ".likelihood.variance": 0.05})
    ref = fresh(Z1, 1.7, [0.6, 1.4], 0.05)
    mu, var = m.predict_f(Xs)
    rmu, rvar = ref.predict_f(Xs)
    assert relerr(mu, rmu.cpu().numpy()) < 1e-9 and relerr(var, rvar.cpu().numpy()) < 1e-9
    assert abs(m.elbo() - ref.elbo()) < 1e-9 * abs(ref.elbo())
    # 3. Z edited in place (same tensor object): the version counter is part of the fingerprint
    m.inducing_variable.Z.mul_(0.9)
    ref = fresh(0.9 * Z1, 1.7, [0.6, 1.4], 0.05)
    assert relerr(m.predict_f(Xs)[0], ref.predict_f(Xs)[0].cpu().numpy()) < 1e-9
    assert e0 != m.elbo()


def test_reference_callable_protocols():
    """Call-compatibility with the reference's callables (missing 3): `distance_fn` produced by
    `create_distance_fn` is accepted positionally by the selection functions (`cggp/selection.py:14-18,35-41`)
    and runs the SAME distance fused; a user-written `CGPreconditioner.__call__(vec, mat)`
    (`cggp/conjugate_gradient.py:125-128`) runs inside the device-resident loop through libmgp's callback."""
    from cggp import selection
    from cggp.conjugate_gradient import CGPreconditioner, conjugate_gradient
    from cggp.distance import create_distance_fn, euclid_distance
    from cggp.optimize import kmeans_update_inducing_parameters
    N, M, D = 2000, 30, 3
    k, ko = make_kernel("matern32", D)
    X, Z = points(N, M, D)
    for name in ("euclidean", "covariance", "correlation"):
        fn = create_distance_fn(k, name)
        idx, dist = selection.kmeans_indices_and_distances(T(Z), T(X), fn)  # positional, as the reference calls it
        ref_fn = od.create_distance_fn(ko, name)
        d_all = ref_fn((Z[None, :, :], X[:, None, :]))
        chosen = d_all[np.arange(N), idx.cpu().numpy()]
        assert np.max(np.abs(chosen - d_all.min(1))) < 1e-9 and relerr(dist, chosen) < 1e-7
        # the eager function and the fused search are the same distance
        eager = fn((T(Z)[idx], T(X)))
        assert relerr(dist, eager.cpu().numpy()) < 1e-7
    i0, _ = selection.kmeans_indices_and_distances(T(Z), T(X))
    i1, _ = selection.kmeans_indices_and_distances(T(Z), T(X), euclid_distance)
    assert torch.equal(i0, i1)
    C, _ = selection.kmeans_lloyd(T(X), 5, 1e-6, T(X[:5].copy()), create_distance_fn(k, "covariance"))
    assert C.shape == (5, D)
    with pytest.raises(TypeError, match="fused"):
        selection.kmeans_indices_and_distances(T(Z), T(X), lambda a: (a[0] - a[1]).abs().sum(-1))

    class M:  # stand-in for a model: kmeans_update_inducing_parameters only reads .kernel
        kernel = k
    y = np.sin(X).sum(1, keepdims=True)
    Zo, u, c = kmeans_update_inducing_parameters(M, (T(X), T(y)), create_distance_fn(k, "correlation"), T(Z))
    Zs, us, cs = kmeans_update_inducing_parameters(M, (T(X), T(y)), "correlation", T(Z))
    assert torch.equal(c, cs) and float(c.sum()) == N

    # a preconditioner the library has never heard of: damped Jacobi written with torch ops
    class MyPreconditioner(CGPreconditioner):
        calls = 0

        def __call__(self, vec, mat):
            MyPreconditioner.calls += 1
            z = vec / (mat.diagonal()[None, :] + 0.25)
            return z, (z * vec).sum(dim=-1, keepdim=True)

    class OraclePre:
        def __call__(self, vec, mat):
            z = vec / (np.diagonal(mat)[None, :] + 0.25)
            return z, np.sum(z * vec, axis=-1, keepdims=True)

    A, rhs = cg_problem(n=60, noise=0.3)
    A = A * np.linspace(0.5, 3.0, 60)[:, None] * np.linspace(0.5, 3.0, 60)[None, :]  # a diagonal worth scaling by
    for steps in (1, 4, 7):
        sol, (kk, err) = conjugate_gradient(T(A), T(rhs.T), None, 0.0, MyPreconditioner(), max_iterations=steps,
                                            max_steps_cycle=3, check_every=2)
        sol_o, (ko_, err_o) = ocg.conjugate_gradient(A, rhs.T, np.zeros_like(rhs.T), 0.0, OraclePre(),
                                                     max_iterations=steps, max_steps_cycle=3)
        assert int(kk) == steps == ko_
        assert relerr(sol, sol_o) < 1e-9 and relerr(err, err_o) < 1e-8
    assert MyPreconditioner.calls >= 1 + 1 + 4 + 7
    # and it converges like its native twin
    sol, (kk, _) = conjugate_gradient(T(A), T(rhs.T), None, 1e-12, MyPreconditioner(), max_iterations=500)
    assert relerr(sol, np.linalg.solve(A, rhs).T) < 1e-6 and int(kk) < 500
