"""The Lanczos variance cache on the GPU: the wide projection `mgp_knm_project` (csrc/project.hip) against a longdouble
restatement, its determinism and memory contract, `cggp.lanczos` on the matrix-free operator, and
`GPR(variance="lanczos")` against the Cholesky model."""

import ctypes
import math

import numpy as np
import pytest
import torch

import love_reference as lr
from cggp import _hip, kernels, models, ops, training
from cggp.conjugate_gradient import ConjugateGradient
from cggp.lanczos import lanczos
from test_gpu_gpr import KCLS, KINDS, T, bar, dev, gpr_data, inputs, relmax, relnorm, spec_of

pytestmark = pytest.mark.gpu

MGP_E_BADARG, MGP_E_SHAPE, MGP_E_NOMEM = -1, -2, -6  # include/mgp.h
EPS = float(np.finfo(np.float64).eps)

# ---- 1. the projection against a longdouble restatement -----------------------------------------------------------
# every r (1, 15, 16, 17 around the 16-column tiles; 128, 256 the widths of a cache; 257 the generic route) against
# every kind, with N (tile edges of the 16-row steps and the split over N), D (every register-resident width, and 33
# for the generic route), B (around the 64-row tile), the layout of R and the set of outputs cycling
_NS, _DS, _BS = [1, 63, 64, 65, 1000, 4097], [1, 3, 8, 17, 32, 33], [1, 15, 16, 17, 300]
_PARITY = []
for ki, kind in enumerate(KINDS):
    for ri, r in enumerate([1, 15, 16, 17, 128, 256, 257]):
        _PARITY.append((kind, _DS[(ri + 2 * ki) % 6], _NS[(ri + ki) % 6], _BS[(ri + ki) % 5], r, (ri + ki) % 2,
                        (ri + ki) % 3))
_PARITY += [("se", 8, 4097, 300, 256, ops.COLS, 0), ("matern52", 32, 4097, 300, 128, ops.ROWS, 0),
            ("matern32", 33, 1000, 17, 257, ops.COLS, 0), ("matern12", 3, 4097, 300, 17, ops.ROWS, 0),
            ("se", 17, 1000, 300, 256, ops.ROWS, 0)]


def project_on(lib, h, spec, Xs, X, R, layout, want_proj=True, want_sq=True):
    """mgp_knm_project on a raw handle (null stream, synchronised around the call) -> (rc, proj, sqnorm)."""
    B, N = Xs.shape[0], X.shape[0]
    r = R.shape[1] if layout == ops.COLS else R.shape[0]
    proj = torch.full((B, r), float("nan"), dtype=Xs.dtype, device=Xs.device) if want_proj else None
    sq = torch.full((B,), float("nan"), dtype=Xs.dtype, device=Xs.device) if want_sq else None
    k = spec.struct(_hip.dtype_code(Xs))
    torch.cuda.synchronize()
    rc = lib.mgp_knm_project(h, ctypes.byref(k), _hip.ptr(Xs), B, _hip.ptr(X), N, _hip.ptr(R), r, layout,
                             _hip.ptr(proj), _hip.ptr(sq))
    torch.cuda.synchronize()
    return rc, proj, sq


def default_handle():
    hd = _hip.get_handle(dev())
    return hd.lib, hd.h


def project_case(kind, D, N, B, r, seed=0):
    X, ls = inputs(N, D, seed=N + D)
    rng = np.random.default_rng(seed + 1)
    Xs = rng.standard_normal((B, D))
    R = rng.standard_normal((N, r))
    return X, ls, Xs, R


@pytest.mark.parametrize("kind,D,N,B,r,layout,outs", _PARITY)
def test_project_matches_longdouble(kind, D, N, B, r, layout, outs):
    X, ls, Xs, R = project_case(kind, D, N, B, r)
    var = 1.3
    ref_p, ref_s = lr.knm_project(kind, var, ls, Xs, X, R)
    spec = spec_of(kind, var, ls, D)
    Rd = T(R) if layout == ops.COLS else T(R.T)
    lib, h = default_handle()
    want_proj, want_sq = outs in (0, 1), outs in (0, 2)  # both, proj alone, sqnorm alone
    rc, proj, sq = project_on(lib, h, spec, T(Xs), T(X), Rd, layout, want_proj, want_sq)
    assert rc == 0, lib.mgp_last_error(h)
    if want_proj:
        e = relmax(proj, ref_p)
        print(f"proj {kind} D={D} N={N} B={B} r={r}: {e:.3e}")
        assert e < bar(kind)
    if want_sq:
        e = relmax(sq, ref_s)
        print(f"sqnorm {kind} D={D} N={N} B={B} r={r}: {e:.3e}")
        assert e < bar(kind)
    # the wrapper gives the same numbers
    s2, p2 = ops.knm_project(spec, T(Xs), T(X), Rd, want_proj=True, r_layout=layout)
    assert relmax(p2, ref_p) < bar(kind) and relmax(s2, ref_s) < bar(kind)


@pytest.mark.parametrize("kind", ["se", "matern32"])
@pytest.mark.parametrize("r", [64, 257])
def test_project_fp32_takes_the_generic_route(kind, r):
    N, D, B = 1500, 5, 200
    X, ls, Xs, R = project_case(kind, D, N, B, r, seed=7)
    f = np.float32
    ref_p, ref_s = lr.knm_project(kind, 1.0, ls, Xs.astype(f), X.astype(f), R.astype(f))
    sq, proj = ops.knm_project(spec_of(kind, 1.0, ls, D), T(Xs, torch.float32), T(X, torch.float32),
                               T(R, torch.float32), want_proj=True)
    assert proj.dtype == torch.float32 and sq.dtype == torch.float32
    assert relmax(proj, ref_p) < 2e-4 and relmax(sq, ref_s) < 2e-4


def test_project_generic_and_fused_agree():
    """r = 256 (fused) and the same columns inside r = 257 (generic): the same results to rounding."""
    N, D, B = 4097, 8, 300
    X, ls, Xs, R = project_case("matern52", D, N, B, 257, seed=3)
    spec = spec_of("matern52", 0.9, ls, D)
    _, fused = ops.knm_project(spec, T(Xs), T(X), T(R[:, :256]), want_proj=True)
    _, gen = ops.knm_project(spec, T(Xs), T(X), T(R), want_proj=True)
    assert relmax(fused, gen[:, :256].cpu().numpy()) < 1e-12


def test_project_small_b_at_size_splits_n():
    """B = 8 test rows against N = 2^17: the split over N and the fixed-order reduction; against the sweep."""
    N, D, B, r = 1 << 17, 8, 8, 128
    X, ls = inputs(N, D, seed=11, spread=2.0)
    rng = np.random.default_rng(4)
    Xs = rng.standard_normal((B, D)) * 2.0
    R = rng.standard_normal((N, r))
    spec = spec_of("se", 1.0, ls, D)
    Xd, Xsd, Rd = T(X), T(Xs), T(R)
    sq, proj = ops.knm_project(spec, Xsd, Xd, Rd, want_proj=True)
    ref = torch.cat([ops.knm_matvec(spec, Xsd, Xd, Rd[:, c:c + 8].contiguous()) for c in range(0, r, 8)], dim=1)
    assert relnorm(proj, ref) < 1e-12
    assert relnorm(sq, (ref * ref).sum(dim=1)) < 1e-12
    sq2, proj2 = ops.knm_project(spec, Xsd, Xd, Rd, want_proj=True)
    assert torch.equal(proj, proj2) and torch.equal(sq, sq2)  # deterministic: bit-identical
    sq3, _ = ops.knm_project(spec, Xsd, Xd, Rd.t().contiguous(), r_layout=ops.ROWS)
    assert relnorm(sq3, sq) < 1e-12


# ---- 2. determinism, empty inputs, arguments, memory -----------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "generic", "generic_fp32"])
def test_project_twice_is_bit_identical(route):
    D, r, dt = {"fused": (8, 128, torch.float64), "generic": (33, 257, torch.float64),
                "generic_fp32": (5, 64, torch.float32)}[route]
    X, ls, Xs, R = project_case("matern32", D, 4097, 300, r, seed=9)
    spec = spec_of("matern32", 1.1, ls, D)
    a = ops.knm_project(spec, T(Xs, dt), T(X, dt), T(R, dt), want_proj=True)
    b = ops.knm_project(spec, T(Xs, dt), T(X, dt), T(R, dt), want_proj=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_project_empty_and_args():
    spec = spec_of("se", 1.0, [1.0, 1.0], 2)
    lib, h = default_handle()
    k = spec.struct(_hip.F64)
    kp = ctypes.byref(k)
    X, Xs, R = T(np.zeros((5, 2))), T(np.ones((3, 2))), T(np.ones((5, 4)))
    proj = torch.full((3, 4), 7.0, dtype=torch.float64, device=dev())
    sq = torch.full((3,), 7.0, dtype=torch.float64, device=dev())
    call = lib.mgp_knm_project
    # B = 0: nothing written, not an error
    assert call(h, kp, None, 0, _hip.ptr(X), 5, _hip.ptr(R), 4, 0, _hip.ptr(proj), _hip.ptr(sq)) == 0
    torch.cuda.synchronize()
    assert bool((proj == 7.0).all()) and bool((sq == 7.0).all())
    # N = 0: zeros
    assert call(h, kp, _hip.ptr(Xs), 3, None, 0, None, 4, 0, _hip.ptr(proj), _hip.ptr(sq)) == 0
    torch.cuda.synchronize()
    assert bool((proj == 0.0).all()) and bool((sq == 0.0).all())
    # r = 0: the norms are zeros
    sq.fill_(7.0)
    assert call(h, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, None, 0, 0, None, _hip.ptr(sq)) == 0
    torch.cuda.synchronize()
    assert bool((sq == 0.0).all())
    s, p = ops.knm_project(spec, Xs[:0], X, R, want_proj=True)
    assert s.shape == (0,) and p.shape == (0, 4)
    # both outputs NULL, a bad layout, a NULL input, a negative size
    assert call(h, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, _hip.ptr(R), 4, 0, None, None) == MGP_E_BADARG
    assert call(h, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, _hip.ptr(R), 4, 2, _hip.ptr(proj), None) == MGP_E_BADARG
    assert call(h, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, None, 4, 0, _hip.ptr(proj), None) == MGP_E_BADARG
    assert call(h, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, _hip.ptr(R), -1, 0, _hip.ptr(proj), None) == MGP_E_SHAPE
    assert call(None, kp, _hip.ptr(Xs), 3, _hip.ptr(X), 5, _hip.ptr(R), 4, 0, _hip.ptr(proj), None) == MGP_E_BADARG
    with pytest.raises(ValueError):
        ops.knm_project(spec, Xs, X, R.t().contiguous())


def test_project_fixed_pool_too_small_is_nomem():
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, 1 << 16) == 0
    try:
        X, ls, Xs, R = project_case("se", 4, 4097, 300, 128)
        rc, _, _ = project_on(lib, h, spec_of("se", 1.0, ls, 4), T(Xs), T(X), T(R), ops.COLS)
        assert rc == MGP_E_NOMEM
        assert b"fixed workspace exhausted" in lib.mgp_last_error(h)
    finally:
        lib.mgp_destroy(h)


@pytest.mark.parametrize("route", ["fused", "generic"])
def test_project_workspace_within_stated_bound(route):
    N, B = 20000, 3000
    D, r = (8, 256) if route == "fused" else (33, 257)
    X, ls, Xs, R = project_case("se", D, N, B, r)
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, 0) == 0
    try:
        base = lib.mgp_workspace_bytes(h)
        rc, _, sq = project_on(lib, h, spec_of("se", 1.0, ls, D), T(Xs), T(X), T(R), ops.COLS, want_proj=False)
        assert rc == 0, lib.mgp_last_error(h)
        used = lib.mgp_workspace_bytes(h) - base
        if route == "fused":  # mgp.h, mgp_knm_project: 8 t r' (min(B', 2^16) / t + s) + 8 N (D' + 1) + 256, t = 64 here
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            bound = 512 * 256 * ((B + 63) // 64 + 4 * cus + 1) + 8 * N * (8 + 1) + 256
        else:  # elem (r N + c min(N, 16384) + c r) + 256, c = min(B, max(64, 2^28 / (elem min(N, 16384))))
            sc = min(N, 16384)
            c = min(B, max(64, (1 << 28) // (8 * sc)))
            bound = 8 * (r * N + c * sc + c * r) + 256
            bound += 8 * 8 * c * r  # the NT GEMM's own slices of its [c, r] output (at most 8) in the shared arena
        # a growing handle rounds each arena up by a quarter (+ 4 KiB) and counts 256 bytes of slack per arena
        assert 0 < used <= 1.25 * bound + 2 * (4096 + 256)
        # the norms themselves, against torch in fp64 (direct differences); on the generic route the call crossed a
        # test-row and a streamed cut (tests/test_gpu_seams.py checks both sides of each in long double)
        Xd, Xsd = T(X), T(Xs)
        r2 = torch.zeros((B, N), dtype=torch.float64, device=dev())
        for d in range(D):
            diff = (Xsd[:, d, None] - Xd[None, :, d]) / float(ls[d])
            r2.addcmul_(diff, diff)
        ref = torch.exp(-0.5 * r2) @ T(R)
        assert relmax(sq, (ref * ref).sum(dim=1).cpu().numpy()) < bar("se")
    finally:
        lib.mgp_destroy(h)


# ---- 3. Lanczos on the matrix-free operator ---------------------------------------------------------------------------
def test_lanczos_on_the_operator_matches_the_dense_matrix():
    N, D = 2000, 3
    X, Y, _ = gpr_data(N, D, seed=6)
    m = models.GPR((T(X), T(Y)), kernels.Matern32(1.0, [0.9, 1.2, 0.7]), noise_variance=0.1, solver="cg")
    Q, a, b = lanczos(m.operator(), T(Y[:, 0]), 48)
    assert Q.shape == (48, N) and Q.is_cuda
    A = m.operator().dense()
    Qc, ac, bc = lanczos(A.cpu(), torch.from_numpy(Y[:, 0]), 48)
    eye = torch.eye(48, dtype=torch.float64, device=dev())
    assert float((Q @ Q.t() - eye).abs().max()) < 1.4e-14  # the bound of tests/test_love_host.py
    Tm = torch.diag(a) + torch.diag(b, 1) + torch.diag(b, -1)
    assert float((Q @ A @ Q.t() - Tm).abs().max() / torch.linalg.matrix_norm(A, 2)) < 6e-15
    assert np.allclose(a.cpu().numpy()[:8], ac.numpy()[:8], rtol=1e-9)


# ---- 4. the model -----------------------------------------------------------------------------------------------------
def love_models(N, kind, rank, seed=2):
    X, Y, Xs = gpr_data(N, 3, seed=seed)
    kern = KCLS[kind](1.0, [0.9, 1.2, 0.7])
    data = (T(X), T(Y))
    chol = models.GPR(data, kern, noise_variance=0.1, solver="cholesky")
    cg = ConjugateGradient(1e-12, max_iterations=4000)
    love = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg", variance="lanczos",
                      variance_rank=rank)
    return chol, love, cg, data, kern, T(Xs)


@pytest.mark.parametrize("kind", ["matern32", "matern52"])
def test_gpr_lanczos_full_rank_equals_cholesky(kind):
    """N = 256, rank 256: the Krylov space is everything.  Measured against the Cholesky model, relative to the largest
    entry: variance 1.7e-15 (Matern-3/2) and 1.5e-15 (Matern-5/2), covariance 2.3e-15 and 2.0e-15 -- nine orders inside
    the 1e-6 of test_gpr_cg_against_cholesky; the mean, which comes from the CG solve, 1.3e-7."""
    chol, love, _, _, _, Xs = love_models(256, kind, 256)
    m0, v0 = chol.predict_f(Xs)
    m1, v1 = love.predict_f(Xs)
    assert love.variance_cache().rank_ == 256
    ev, em = relmax(v1, v0.cpu().numpy()), relmax(m1, m0.cpu().numpy())
    _, c0 = chol.predict_f(Xs[:20], full_cov=True)
    _, c1 = love.predict_f(Xs[:20], full_cov=True)
    ec = relmax(c1, c0.cpu().numpy())
    print(f"{kind}: variance {ev:.3e} covariance {ec:.3e} mean {em:.3e}")
    assert v1.shape == (97, 1) and c1.shape == (1, 20, 20)
    assert em < 1e-6 and ev < 1e-6 and ec < 1e-6


@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_gpr_lanczos_bounds_at_8192(kind):
    """The data and kernels of test_gpr_cg_against_cholesky: upper bound, monotonicity and the prior cap, to the
    rounding tolerance 100 cond(Khat) eps variance of tests/test_love_host.py."""
    chol, _, cg, data, kern, Xs = love_models(8192, kind, 16)
    _, v0 = chol.predict_f(Xs)
    _, c0 = chol.predict_f(Xs[:20], full_cov=True)
    Khat = ops.k_dense(kern.spec(3), data[0], data[0], jitter=0.1)
    ev = torch.linalg.eigvalsh(Khat)
    cond = float(ev[-1] / ev[0])
    tol = 100.0 * cond * EPS * kern.variance
    solve = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg")
    mean_solve = ops.knm_matvec(kern.spec(3), Xs, data[0], solve.alpha())
    prev = None
    for rank in [16, 64, 256]:
        love = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg", variance="lanczos",
                          variance_rank=rank)
        mean, var = love.predict_f(Xs)
        d = (var - v0)[:, 0]
        print(f"{kind} rank={love.variance_cache().rank_}: excess min {float(d.min()):.3e} max {float(d.max()):.3e} "
              f"tol {tol:.2e} cond {cond:.3e}")
        assert torch.equal(mean, mean_solve)  # the mean does not go through the cache
        assert float(d.min()) >= -tol
        assert float(var.max()) <= kern.variance + tol
        if prev is not None:
            assert float((var - prev).max()) <= tol
        prev = var
        _, c1 = love.predict_f(Xs[:20], full_cov=True)
        diff = c1[0] - c0[0]
        assert float(torch.linalg.eigvalsh(0.5 * (diff + diff.t()))[0]) >= -tol


def test_gpr_default_is_untouched_and_cache_follows_parameters(monkeypatch):
    X, Y, Xs = gpr_data(3000, 2, seed=3)
    kern = kernels.Matern32(1.0, [1.0, 1.0])
    data = (T(X), T(Y))
    cg = ConjugateGradient(1e-10, max_iterations=2000)
    a = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg")
    b = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg", variance="solve")
    Xq = T(Xs[:12])
    (ma, va), (mb, vb) = a.predict_f(Xq), b.predict_f(Xq)
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    (_, ca), (_, cb) = a.predict_f(Xq, full_cov=True), b.predict_f(Xq, full_cov=True)
    assert torch.equal(ca, cb)
    assert a._variance_cache is None and b._variance_cache is None
    # the Cholesky path ignores the option
    c = models.GPR(data, kern, noise_variance=0.1, solver="cholesky", variance="lanczos")
    d = models.GPR(data, kern, noise_variance=0.1, solver="cholesky")
    assert torch.equal(c.predict_f(Xq)[1], d.predict_f(Xq)[1]) and c._variance_cache is None

    builds = []
    real = models.LanczosVarianceCache.build
    monkeypatch.setattr(models.LanczosVarianceCache, "build", lambda self, gpr: (builds.append(1), real(self, gpr))[1])
    m = models.GPR(data, kern, noise_variance=0.1, conjugate_gradient=cg, solver="cg", variance="lanczos",
                   variance_rank=32)
    _, v1 = m.predict_f(Xq)
    _, v1b = m.predict_f(T(Xs))
    m.predict_f(Xq, full_cov=True)
    assert len(builds) == 1 and torch.equal(v1b[:12], v1)  # built once, reused
    kern.lengthscales = [0.5, 0.5]
    _, v2 = m.predict_f(Xq)
    assert len(builds) == 2 and not torch.equal(v1, v2)
    m.likelihood.variance = 0.3
    _, v3 = m.predict_f(Xq)
    assert len(builds) == 3 and not torch.equal(v2, v3)
    data[0].mul_(1.01)  # X changes in place
    _, v4 = m.predict_f(Xq)
    assert len(builds) == 4 and not torch.equal(v3, v4)
    m.predict_f(Xq)
    assert len(builds) == 4
    m.variance_rank = 48
    m.predict_f(Xq)
    assert len(builds) == 5 and m.variance_cache().rank_ == 48


def test_rmse_nlpd_and_frozen_model_through_the_cache():
    X, Y, Xs = gpr_data(3000, 2, seed=4)
    Ys = np.sin(Xs.sum(axis=1, keepdims=True) * 1.3)
    kern = kernels.Matern52(1.0, [1.0, 1.0])
    data = (T(X), T(Y))
    cg = ConjugateGradient(1e-10, max_iterations=2000)
    solve = models.GPR(data, kern, noise_variance=0.2, conjugate_gradient=cg, solver="cg")
    love = models.GPR(data, kern, noise_variance=0.2, conjugate_gradient=cg, solver="cg", variance="lanczos",
                      variance_rank=64)
    r0, n0 = models.rmse_nlpd(solve, (T(Xs), T(Ys)), batch_size=40)
    r1, n1 = models.rmse_nlpd(love, (T(Xs), T(Ys)), batch_size=40)
    print(f"rmse {r1:.6f} nlpd solve {n0:.6f} lanczos(64) {n1:.6f}")
    assert r1 == r0 and math.isfinite(n1)
    my, vy = love.predict_y(T(Xs))
    assert torch.equal(vy, love.predict_f(T(Xs))[1] + 0.2)

    model = training.TrainableGPR(kernels.Matern52(0.7, [0.5, 1.5]), 0.3, T(X[:300]), T(Y[:300]))
    f0 = model.frozen_model()
    assert f0.variance == "solve" and f0.variance_rank == 128
    f1 = model.frozen_model(variance="lanczos", variance_rank=64)
    assert f1.variance == "lanczos" and f1.variance_rank == 64 and f1.solver == f0.solver
    with pytest.raises(TypeError):
        model.frozen_model(solver="cg")
