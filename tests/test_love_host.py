"""Host-side checks of the Lanczos variance cache: the exported entry point, `cggp.lanczos.lanczos` against the numpy
restatement, and the torch half of `LanczosVarianceCache` against the theorems a Galerkin projection obeys -- it never
under-states the variance, it decreases monotonically with the rank, it is capped by the prior, and rank N is exact."""

import ctypes

import numpy as np
import pytest
import torch

import love_reference as lr
from cggp import _hip, kernels, models
from cggp.lanczos import lanczos
from oracle import kernels as ok
from test_gpu_gpr import gpr_data

KINDS = ["se", "matern12", "matern32", "matern52"]
KCLS = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
        "matern52": kernels.Matern52}
EPS = float(np.finfo(np.float64).eps)
N, D, S2, VAR, LS = 256, 3, 0.1, 1.2, [0.8, 1.1, 0.6]

# |Q Q^T - I|_max and |Q A Q^T - T|_max / |A|_2 of the two fp64 implementations (numpy restatement, cggp.lanczos) on
# the four N = 256 kernel matrices below at 16, 64, 128 and 256 steps, measured beside the longdouble restatement
# (4.3e-19 ... 9.8e-19 and 1.9e-18 ... 5.7e-18 there): orthogonality at most 1.22e-15 (numpy) / 1.33e-15 (torch), the
# tridiagonal at most 4.58e-16 (numpy) / 5.17e-16 (torch).  The bounds are the larger figure times 10.
ORTH_TOL = 1.4e-14
TRI_TOL = 6e-15


def test_entry_point_is_exported_and_refuses_a_null_handle():
    lib = _hip.load_library()
    assert hasattr(lib, "mgp_knm_project")
    k = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    assert lib.mgp_knm_project(None, ctypes.byref(k), None, 0, None, 0, None, 0, 0, None, None) == -1
    assert lib.mgp_version() == 210 == _hip.MGP_VERSION


def khat(kind):
    X, Y, Xs = gpr_data(N, D)
    return ok.Kernel(kind, VAR, LS).K(X) + S2 * np.eye(N), X, Y, Xs


def lanczos_errors(A, Q, alpha, beta):
    k = Q.shape[0]
    A = A.astype(Q.dtype)
    orth = np.max(np.abs(Q @ Q.T - np.eye(k)))
    tri = np.max(np.abs(Q @ A @ Q.T - lr.tridiagonal(alpha, beta))) / np.linalg.norm(A.astype(np.float64), 2)
    return float(orth), float(tri)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("steps", [16, 64, 128, 256])
def test_lanczos_is_orthonormal_and_tridiagonalises(kind, steps):
    A, _, Y, _ = khat(kind)
    start = Y[:, 0]
    Qt, at, bt = lanczos(torch.from_numpy(A), torch.from_numpy(start), steps)
    assert Qt.shape == (steps, N) and at.shape == (steps,) and bt.shape == (steps - 1,)
    runs = {"torch": (Qt.numpy(), at.numpy(), bt.numpy()), "numpy": lr.lanczos(A, start, steps),
            "longdouble": lr.lanczos(A, start, steps, dtype=np.longdouble)}
    for name, (Q, a, b) in runs.items():
        orth, tri = lanczos_errors(A, Q, a, b)
        print(f"{kind} steps={steps} {name}: |QQ^T-I|={orth:.3e} |QAQ^T-T|/|A|={tri:.3e}")
        assert orth < ORTH_TOL and tri < TRI_TOL
    # the first steps of the recurrence are well determined: the three runs give the same tridiagonal there
    m = min(steps, 8)
    ref = runs["longdouble"]
    assert np.allclose(at.numpy()[:m], ref[1][:m].astype(np.float64), rtol=1e-9)
    assert np.allclose(bt.numpy()[:m - 1], ref[2][:m - 1].astype(np.float64), rtol=1e-9)


def test_lanczos_takes_a_callable_and_stops_on_an_invariant_space():
    A, _, Y, _ = khat("matern32")
    At = torch.from_numpy(A)
    v = torch.from_numpy(Y[:, 0])
    Q0, a0, b0 = lanczos(At, v, 12)
    Q1, a1, b1 = lanczos(lambda q: At @ q, v, 12)
    assert torch.equal(Q0, Q1) and torch.equal(a0, a1) and torch.equal(b0, b1)
    # an eigenvector spans a Krylov space of dimension one
    w, V = np.linalg.eigh(A)
    Q, a, b = lanczos(At, torch.from_numpy(np.ascontiguousarray(V[:, -3])), 10)
    assert Q.shape == (1, N) and a.shape == (1,) and b.shape == (0,)
    assert abs(float(a[0]) - w[-3]) < 1e-12 * w[-1]
    # and so does the restatement
    assert lr.lanczos(A, V[:, -3], 10)[0].shape == (1, N)
    # steps are clamped to n; a zero start is refused
    assert lanczos(At[:5, :5], v[:5], 9)[0].shape[0] <= 5
    with pytest.raises(ValueError):
        lanczos(At, torch.zeros(N, dtype=torch.float64), 4)


@pytest.mark.parametrize("kind", KINDS)
def test_cache_bounds_hold_to_rounding(kind):
    """var_k >= var_exact, var_k <= var_k' for k > k', var_k <= K_diag; tol is rounding only: the error of
    p^T T^-1 p is about cond(T) eps p^T T^-1 p with cond(T) <= cond(Khat) and p^T T^-1 p <= k**."""
    A, X, Y, Xs = khat(kind)
    v_exact, _, cond = lr.exact_variance(kind, VAR, LS, X, S2, Xs)
    tol = 100.0 * cond * EPS * VAR
    kern = KCLS[kind](VAR, LS)
    At, Xt, Xst = torch.from_numpy(A), torch.from_numpy(X), torch.from_numpy(Xs)
    prev = None
    for rank in [16, 64, 128, N]:
        Q, a, b = lanczos(At, torch.from_numpy(Y[:, 0]), rank)
        cache = models.LanczosVarianceCache(rank=rank).from_tridiagonal(Q, a, b, Xt)
        var = cache.variance(kern, Xst).numpy()
        # the restatement shows the same figures
        var_np, _ = lr.galerkin(kind, VAR, LS, X, Xs, lr.projector(*lr.lanczos(A, Y[:, 0], rank)))
        print(f"{kind} rank={cache.rank_}: min(var-exact)={np.min(var - v_exact):.3e} "
              f"max(var-exact)={np.max(var - v_exact):.3e} numpy min={np.min(var_np - v_exact):.3e} tol={tol:.2e}")
        assert np.all(var >= v_exact - tol) and np.all(var_np >= v_exact - tol)
        assert np.all(var <= VAR + tol)
        if prev is not None:
            assert np.all(var <= prev + tol)
        prev = var
    # rank N: the Krylov space is everything and the cache equals the Cholesky variance.  For the SE kernel the
    # recurrence was expected to break down before N steps; at this N, D and noise (cond(Khat) = 275) it does not --
    # torch and the restatement both reach rank N = 256 -- and the variance is exact to rounding like the others
    # (measured: |var - exact| <= 5.3e-15 for every kernel, tol = 2.8e-12 ... 7.4e-12)
    assert cache.rank_ == N
    assert np.max(np.abs(var - v_exact)) <= tol
    # the covariance at rank N too, and it dominates the exact one below
    _, c_exact, _ = lr.exact_variance(kind, VAR, LS, X, S2, Xs[:20])
    cov = cache.covariance(kern, Xst[:20]).numpy()
    assert np.max(np.abs(cov - c_exact)) <= tol
    Q, a, b = lanczos(At, torch.from_numpy(Y[:, 0]), 64)
    cov64 = models.LanczosVarianceCache(64).from_tridiagonal(Q, a, b, Xt).covariance(kern, Xst[:20]).numpy()
    d = cov64 - c_exact
    assert np.linalg.eigvalsh(0.5 * (d + d.T))[0] >= -tol


def test_cache_and_model_argument_checks():
    X, Y, Xs = gpr_data(40, 2)
    kern = kernels.Matern32(1.0, [1.0, 1.0])
    with pytest.raises(ValueError):
        models.LanczosVarianceCache(rank=0)
    with pytest.raises(ValueError):
        models.LanczosVarianceCache(start="x")
    with pytest.raises(RuntimeError):
        models.LanczosVarianceCache().variance(kern, torch.from_numpy(Xs))
    Q = torch.eye(3, 40, dtype=torch.float64)
    with pytest.raises(ValueError):
        models.LanczosVarianceCache().from_tridiagonal(Q, torch.ones(3, dtype=torch.float64),
                                                       torch.zeros(3, dtype=torch.float64))
    data = (torch.from_numpy(X), torch.from_numpy(Y))
    with pytest.raises(ValueError, match="variance"):
        models.GPR(data, kern, variance="exact")
    m = models.GPR(data, kern)
    assert m.variance == "solve" and m.variance_rank == 128 and m._variance_cache is None
    m = models.GPR(data, kern, variance="lanczos", variance_rank=32)
    assert m.variance == "lanczos" and m.variance_rank == 32 and m._variance_cache is None
