"""Exact GP regression on the GPU: the symmetric self-kernel product `mgp_kxx_matvec` (csrc/kxx.hip), the
`MGP_OP_KXX_NOISE` operator inside the device CG, `KxxNoiseOperator`, `cggp.models.GPR` and `TrainableGPR`."""

import ctypes

import numpy as np
import pytest
import torch

from cggp import _hip, kernels, models, ops, training
from cggp.conjugate_gradient import (ConjugateGradient, KmmLambdaOperator, KxxNoiseOperator, conjugate_gradient)
from gpr_reference import gpr_posterior, kxx_product
from oracle import cg as ocg
from oracle import kernels as ok

pytestmark = pytest.mark.gpu

MGP_E_BADARG, MGP_E_NOMEM = -1, -6  # include/mgp.h
KINDS = ["se", "matern12", "matern32", "matern52"]
KCLS = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
        "matern52": kernels.Matern52}


def dev():
    return torch.device("cuda:0")


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev())


def relmax(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def relnorm(a, b):
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def inputs(N, D, seed=0, spread=1.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * spread
    ls = 0.6 + rng.random(D) * float(np.sqrt(D))
    return X, ls


def spec_of(kind, var, ls, D):
    return ops.KernelSpec(kind, var, list(ls), D)


@pytest.fixture(scope="module")
def sym_handle():
    """A handle with MGP_KXX=sym: the symmetric kernel at every N (the default routes N < 2^16 to the plain sweep)."""
    import os
    lib = _hip.load_library()
    old = os.environ.get("MGP_KXX")
    os.environ["MGP_KXX"] = "sym"
    h = ctypes.c_void_p()
    try:
        assert lib.mgp_create_ex(ctypes.byref(h), 0, 0) == 0
    finally:
        if old is None:
            del os.environ["MGP_KXX"]
        else:
            os.environ["MGP_KXX"] = old
    yield lib, h
    lib.mgp_destroy(h)


def kxx_on(handle, spec, X, s2, V, layout=ops.COLS):
    """mgp_kxx_matvec on `handle` (null stream, synchronised around the call)."""
    lib, h = handle
    N = X.shape[0]
    R = V.shape[1] if layout == ops.COLS else V.shape[0]
    out = torch.empty_like(V)
    k = spec.struct(_hip.dtype_code(X))
    torch.cuda.synchronize()
    rc = lib.mgp_kxx_matvec(h, ctypes.byref(k), _hip.ptr(X), N, float(s2), _hip.ptr(V), R, layout, _hip.ptr(out),
                            layout)
    assert rc == 0, lib.mgp_last_error(h)
    torch.cuda.synchronize()
    return out


# GPflow's expansion-form distance leaves r2 ~ 1e-16 |x|^2 instead of 0 on the diagonal; Matern-1/2 takes
# r = sqrt(max(r2, 1e-36)) into exp(-r), so k(x, x) is 1 - O(1e-8) there (the plain sweep does the same: the two agree
# to rounding).  Against a longdouble restatement that bar is the kernel's, not the product's.
def bar(kind):
    return 1e-7 if kind == "matern12" else 1e-11


# ---- 1. product parity against a longdouble restatement ------------------------------------------------------------
# every N against every kind (D cycling) and every R / layout (cycling), so the tile edges (N = 63, 64, 65, 1000, 4097
# around 256 / 512 / 1024-row blocks) and the diagonal tile meet each kernel instantiation family
_PARITY = []
for ki, kind in enumerate(KINDS):
    for ni, N in enumerate([1, 63, 64, 65, 1000, 4097]):
        D = [1, 3, 8, 17, 32, 33][(ni + ki) % 6]
        R = [1, 2, 5, 8, 11][(ni + 2 * ki) % 5]
        layout = (ni + ki) % 2
        _PARITY.append((kind, D, N, R, layout))


@pytest.mark.parametrize("kind,D,N,R,layout", _PARITY)
def test_kxx_matches_longdouble(sym_handle, kind, D, N, R, layout):
    X, ls = inputs(N, D, seed=N + D)
    rng = np.random.default_rng(1)
    V = rng.standard_normal((N, R))
    s2, var = 0.37, 1.3
    ref = kxx_product(kind, var, ls, X, s2, V)
    Vin = T(V) if layout == ops.COLS else T(V.T)
    spec = spec_of(kind, var, ls, D)
    out = kxx_on(sym_handle, spec, T(X), s2, Vin, layout)
    got = out if layout == ops.COLS else out.t()
    assert relmax(got, ref) < bar(kind)
    plain = ops.knm_matvec(spec, T(X), T(X), T(V)) + s2 * T(V)
    assert relmax(got, plain.cpu().numpy()) < 1e-11
    default = ops.kxx_matvec(spec, T(X), s2, Vin, v_layout=layout)  # the default route (the sweep below 2^16 rows)
    assert relmax(default if layout == ops.COLS else default.t(), ref) < bar(kind)


@pytest.mark.parametrize("R", [1, 2, 4, 8, 11])
@pytest.mark.parametrize("D", [3, 8, 17])
def test_kxx_all_column_groups_se(sym_handle, D, R):
    N = 2100  # three 1024-row blocks with a ragged last one; 512 / 256-row blocks for the wider forms
    X, ls = inputs(N, D, seed=3)
    V = np.random.default_rng(2).standard_normal((N, R))
    ref = kxx_product("se", 0.8, ls, X, 0.05, V)
    got = kxx_on(sym_handle, spec_of("se", 0.8, ls, D), T(X), 0.05, T(V))
    assert relmax(got, ref) < 1e-11


@pytest.mark.parametrize("kind", KINDS)
def test_kxx_duplicate_rows(sym_handle, kind):
    """Distance exactly 0 off the diagonal: repeated rows, in one block and across blocks."""
    rng = np.random.default_rng(5)
    base = rng.standard_normal((700, 4))
    X = np.concatenate([base, base[::-1], base[:300]])  # 1700 rows, every one repeated
    V = rng.standard_normal((X.shape[0], 2))
    ls = np.array([0.7, 1.1, 0.9, 1.4])
    ref = kxx_product(kind, 1.0, ls, X, 0.1, V)
    spec = spec_of(kind, 1.0, ls, 4)
    got = kxx_on(sym_handle, spec, T(X), 0.1, T(V))
    assert relmax(got, ref) < bar(kind)
    plain = ops.knm_matvec(spec, T(X), T(X), T(V)) + 0.1 * T(V)
    assert relmax(got, plain.cpu().numpy()) < 1e-11


@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_kxx_fp32(kind):
    N, D, R = 1500, 5, 3
    X, ls = inputs(N, D, seed=7)
    V = np.random.default_rng(3).standard_normal((N, R))
    ref = kxx_product(kind, 1.0, ls, X.astype(np.float32), 0.2, V.astype(np.float32))
    got = ops.kxx_matvec(spec_of(kind, 1.0, ls, D), T(X, torch.float32), 0.2, T(V, torch.float32))
    assert relmax(got, ref) < 2e-4


def test_kxx_empty_and_args():
    spec = spec_of("se", 1.0, [1.0, 1.0], 2)
    X = torch.zeros((0, 2), dtype=torch.float64, device=dev())
    out = ops.kxx_matvec(spec, X, 0.1, torch.zeros((0, 3), dtype=torch.float64, device=dev()))
    assert out.shape == (0, 3)
    hd = _hip.get_handle(dev())
    k = spec.struct(_hip.F64)
    # N = 0: nothing written, not an error
    assert hd.lib.mgp_kxx_matvec(hd.h, ctypes.byref(k), None, 0, 0.1, None, 3, 0, None, 0) == 0
    X = T(np.zeros((4, 2)))
    V = T(np.ones((4, 1)))
    o = torch.empty_like(V)
    assert hd.lib.mgp_kxx_matvec(hd.h, ctypes.byref(k), _hip.ptr(X), 4, -1.0, _hip.ptr(V), 1, 0, _hip.ptr(o), 0) \
        == MGP_E_BADARG


# ---- 2. against the plain sweep at size ------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 8])
def test_kxx_against_sweep_at_size(sym_handle, R):
    N, D, s2 = 1 << 17, 8, 0.1
    X, ls = inputs(N, D, seed=11, spread=2.0)
    rng = np.random.default_rng(4)
    V = rng.standard_normal((N, R))
    spec = spec_of("se", 1.0, ls, D)
    Xd, Vd = T(X), T(V)
    got = kxx_on(sym_handle, spec, Xd, s2, Vd)  # the symmetric kernel (the default takes it for R = 1 only)
    plain = ops.knm_matvec(spec, Xd, Xd, Vd) + s2 * Vd
    assert relnorm(got, plain) < 1e-12
    again = kxx_on(sym_handle, spec, Xd, s2, Vd)
    assert torch.equal(got, again)  # deterministic: bit-identical
    default = ops.kxx_matvec(spec, Xd, s2, Vd)
    assert relnorm(default, plain) < 1e-12
    if R == 1:
        assert torch.equal(default, got)
    rows = np.sort(rng.choice(N, 512, replace=False))
    kern = ok.Kernel("se", 1.0, ls)
    ref = np.concatenate([kern.K(X[rows[c:c + 64]], X) @ V for c in range(0, 512, 64)]) + s2 * V[rows]
    assert relmax(got[torch.as_tensor(rows, device=dev())], ref) < 1e-11


# ---- 3. CG through MGP_OP_KXX_NOISE -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_cg_fixed_steps_against_oracle_dense(sym_handle, kind):
    # 10 steps: finite-precision CG trajectories of this system part by 1e-3 after 25 steps for ANY two roundings of
    # the same matrix (oracle against oracle with a 1e-16 perturbation), by 5e-11 after 10
    N, D, s2, k = 2000, 3, 0.1, 10
    X, ls = inputs(N, D, seed=21)
    rhs = np.random.default_rng(6).standard_normal((1, N))
    A = ok.Kernel(kind, 1.0, ls).K(X) + s2 * np.eye(N)
    ref, (steps_ref, err_ref) = ocg.conjugate_gradient(A, rhs, np.zeros_like(rhs), 0.0, max_iterations=k)
    op = KxxNoiseOperator(KCLS[kind](1.0, list(ls)), T(X), s2)
    sol, (steps, err) = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k)  # default route: the sweep
    assert int(steps) == int(steps_ref) == k
    assert relmax(sol, ref) < 1e-9
    # the same solve on the symmetric kernel
    lib, h = sym_handle
    st, keep = op._struct()
    pre = _hip.MgpPrecond()
    stats = _hip.MgpCgStats()
    B = T(rhs)
    Vout, e = torch.empty_like(B), torch.empty((1,), dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    assert lib.mgp_pcg_solve(h, ctypes.byref(st), ctypes.byref(pre), _hip.ptr(B), None, 1, 0.0, k, 100, 1e-16, 10,
                             _hip.ptr(Vout), _hip.ptr(e), ctypes.byref(stats)) == 0
    torch.cuda.synchronize()
    assert stats.iterations == k
    assert relmax(Vout, ref) < 1e-9
    del keep


def test_cg_fixed_steps_against_kmm_lambda_at_size():
    N, D, s2, k = 1 << 17, 8, 0.1, 6
    X, ls = inputs(N, D, seed=22, spread=2.0)
    rhs = T(np.random.default_rng(7).standard_normal((1, N)))
    kern = kernels.SquaredExponential(1.0, list(ls))
    Xd = T(X)
    a, _ = conjugate_gradient(KxxNoiseOperator(kern, Xd, s2), rhs, None, 0.0, max_iterations=k)
    lam = torch.full((N,), s2, dtype=torch.float64, device=dev())
    b, _ = conjugate_gradient(KmmLambdaOperator(kern, Xd, lam), rhs, None, 0.0, max_iterations=k)
    assert relmax(a, b.cpu().numpy()) < 1e-9


def test_cg_converged_true_residual():
    N, D, s2, thr = 1 << 16, 4, 0.5, 1e-10  # 2^16: the default route takes the symmetric kernel
    X, ls = inputs(N, D, seed=23, spread=3.0)
    y = T(np.random.default_rng(8).standard_normal((N, 1)))
    kern = kernels.Matern52(1.0, list(ls))
    Xd = T(X)
    cg = ConjugateGradient(thr, max_iterations=2000)
    sol, stats = cg.solve_with_stats(KxxNoiseOperator(kern, Xd, s2), y)
    steps = int(stats[0])
    assert 0 < steps < 2000
    spec = kern.spec(D)
    r = y - (ops.knm_matvec(spec, Xd, Xd, sol) + s2 * sol)
    # the stop rule bounds the recurrence's 0.5 |r|^2; the true residual drifts from it by rounding only
    assert 0.5 * float((r * r).sum()) < 10 * thr


def test_kxx_operator_is_single_rank():
    X = T(np.random.default_rng(9).standard_normal((100, 2)))
    op = KxxNoiseOperator(kernels.SquaredExponential(1.0, [1.0, 1.0]), X, 0.1)
    hd = _hip.get_handle(dev())
    P = T(np.ones((1, 100)))
    out = torch.empty_like(P)
    st, keep = op._struct()
    assert hd.lib.mgp_operator_apply(hd.h, ctypes.byref(st), _hip.ptr(P), 1, _hip.ptr(out)) == 0
    st.comm = ctypes.c_void_p(1)
    assert hd.lib.mgp_operator_apply(hd.h, ctypes.byref(st), _hip.ptr(P), 1, _hip.ptr(out)) == MGP_E_BADARG
    st.comm = None
    st.allreduce = _hip.ALLREDUCE_FN(lambda *a: 0)
    st.world_size = 1
    assert hd.lib.mgp_operator_apply(hd.h, ctypes.byref(st), _hip.ptr(P), 1, _hip.ptr(out)) == MGP_E_BADARG
    del keep


# ---- 4. memory -----------------------------------------------------------------------------------------------------------
def test_fixed_pool_too_small_is_nomem():
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, 1 << 16) == 0
    try:
        N, D = 20000, 4
        X, ls = inputs(N, D)
        Xd, V = T(X), T(np.ones((N, 1)))
        out = torch.empty_like(V)
        torch.cuda.synchronize()
        k = spec_of("se", 1.0, ls, D).struct(_hip.F64)
        rc = lib.mgp_kxx_matvec(h, ctypes.byref(k), _hip.ptr(Xd), N, 0.1, _hip.ptr(V), 1, 0, _hip.ptr(out), 0)
        assert rc == MGP_E_NOMEM
        assert b"fixed workspace exhausted" in lib.mgp_last_error(h)
    finally:
        lib.mgp_destroy(h)


def test_workspace_after_solve_within_stated_bound():
    N, D = 1 << 17, 8
    X, ls = inputs(N, D, seed=31)
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, 0) == 0
    try:
        Xd = T(X)
        B = T(np.random.default_rng(10).standard_normal((1, N)))
        Vout, err = torch.empty_like(B), torch.empty((1,), dtype=torch.float64, device=dev())
        op = KxxNoiseOperator(kernels.SquaredExponential(1.0, list(ls)), Xd, 0.1)
        st, keep = op._struct()
        pre = _hip.MgpPrecond()
        stats = _hip.MgpCgStats()
        torch.cuda.synchronize()
        rc = lib.mgp_pcg_solve(h, ctypes.byref(st), ctypes.byref(pre), _hip.ptr(B), None, 1, 0.0, 3, 100, 1e-16, 10,
                               _hip.ptr(Vout), _hip.ptr(err), ctypes.byref(stats))
        assert rc == 0 and stats.iterations == 3
        used = lib.mgp_workspace_bytes(h)
        Np, Dp = (N + 1023) // 1024 * 1024, 8
        bound = max(1 << 29, 128 * Np) + 8 * Np * (Dp + 17) + 256  # mgp.h, mgp_kxx_matvec
        # the growing handle rounds each arena up by a quarter; CG state is a few [Bt, N] vectors
        assert used <= 1.25 * bound + 64 * 8 * N + (1 << 20)
        assert used < N * N * 8 / 100
        del keep
    finally:
        lib.mgp_destroy(h)


# ---- 5. the GPR model ----------------------------------------------------------------------------------------------------
def gpr_data(N, D, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    Y = np.sin(X.sum(axis=1, keepdims=True) * 1.3) + 0.1 * rng.standard_normal((N, 1))
    Xs = rng.uniform(-2.2, 2.2, (97, D))
    return X, Y, Xs


@pytest.mark.parametrize("kind", KINDS)
def test_gpr_cholesky_against_numpy(kind):
    N, D, s2, var = 2000, 3, 0.1, 1.2
    X, Y, Xs = gpr_data(N, D)
    ls = [0.8, 1.1, 0.6]
    mean0, var0, cov0, lml0 = gpr_posterior(kind, var, ls, X, Y, s2, Xs)
    m = models.GPR((T(X), T(Y)), KCLS[kind](var, ls), noise_variance=s2, solver="cholesky")
    mean, v = m.predict_f(T(Xs))
    tol = 1e-9 if kind != "matern12" else 1e-6  # Matern-1/2 at r2 ~ 0: see bar()
    assert mean.shape == (97, 1) and v.shape == (97, 1)
    assert relmax(mean, mean0) < tol and relmax(v, var0) < tol
    _, cov = m.predict_f(T(Xs), full_cov=True)
    assert cov.shape == (1, 97, 97) and relmax(cov[0], cov0) < tol
    assert abs(m.log_marginal_likelihood() - lml0) < tol * abs(lml0)
    assert m.training_loss() == -m.maximum_log_likelihood_objective()
    my, vy = m.predict_y(T(Xs))
    assert relmax(vy, var0 + s2) < tol


@pytest.mark.parametrize("kind", KINDS)
def test_gpr_cholesky_against_sklearn(kind):
    gp = pytest.importorskip("sklearn.gaussian_process")
    kr = pytest.importorskip("sklearn.gaussian_process.kernels")
    N, D, s2, var = 2000, 3, 0.1, 1.2
    X, Y, Xs = gpr_data(N, D, seed=1)
    ls = np.array([0.8, 1.1, 0.6])
    base = kr.RBF(ls) if kind == "se" else kr.Matern(ls, nu={"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind])
    sk = gp.GaussianProcessRegressor(kr.ConstantKernel(var) * base, alpha=s2, optimizer=None).fit(X, Y)
    mu0, cov0 = sk.predict(Xs, return_cov=True)
    m = models.GPR((T(X), T(Y)), KCLS[kind](var, list(ls)), noise_variance=s2, solver="cholesky")
    mean, cov = m.predict_f(T(Xs), full_cov=True)
    # direct (scikit-learn) against expansion-form (GPflow) distances: see tests/test_gpr_host.py
    assert relmax(mean[:, 0], np.ravel(mu0)) < 1e-6
    assert relmax(cov[0], np.squeeze(cov0)) < 1e-6
    assert abs(m.log_marginal_likelihood() - sk.log_marginal_likelihood_value_) < 1e-7 * abs(
        sk.log_marginal_likelihood_value_)


@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_gpr_cg_against_cholesky(kind):
    N, D, s2 = 8192, 3, 0.1
    X, Y, Xs = gpr_data(N, D, seed=2)
    kern = KCLS[kind](1.0, [0.9, 1.2, 0.7])
    data = (T(X), T(Y))
    chol = models.GPR(data, kern, noise_variance=s2, solver="cholesky")
    cg = models.GPR(data, kern, noise_variance=s2, conjugate_gradient=ConjugateGradient(1e-12, max_iterations=4000),
                    solver="cg")
    m0, v0 = chol.predict_f(T(Xs))
    m1, v1 = cg.predict_f(T(Xs))
    assert relmax(m1, m0.cpu().numpy()) < 1e-6 and relmax(v1, v0.cpu().numpy()) < 1e-6
    _, c0 = chol.predict_f(T(Xs[:20]), full_cov=True)
    _, c1 = cg.predict_f(T(Xs[:20]), full_cov=True)
    assert relmax(c1, c0.cpu().numpy()) < 1e-6
    with pytest.raises(NotImplementedError, match="log"):
        cg.log_marginal_likelihood()
    auto = models.GPR(data, kern, noise_variance=s2, cholesky_max_n=4096)
    assert not auto.uses_cholesky()


@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_gpr_cg_variance_chunks(kind):
    """`variance_chunk_bytes = 8 N 8` makes predict_f solve its B = 37 test columns in chunks of 8: five, the last of 5
    (`var[c0:c0 + step]`, `cov[:, c0:c0 + step]`).  The chunked run must equal the single-chunk run.  The device CG
    iterates a batch until its slowest column is under the threshold (csrc/cg.hip: `while any_b(0.5 |r_b|^2 > thr)`),
    so a column may take more steps beside 36 others than beside 7 and bit-equality is not promised; the runs are
    held to 1e-12 absolute instead, the rounding level of these entries (at most the prior variance 1, each a
    difference of two 300-term sums: about 300 u = 3e-14 apiece), not a bar made from the CG threshold.  Both must
    meet the Cholesky model at the bar of test_gpr_cg_against_cholesky."""
    N, D, s2, B, thr = 300, 3, 0.1, 37, 1e-18
    X, Y, Xs = gpr_data(N, D, seed=5)
    Xs = Xs[:B]
    kern = KCLS[kind](1.0, [0.9, 1.2, 0.7])
    data = (T(X), T(Y))
    cg = lambda **kw: models.GPR(data, kern, noise_variance=s2, solver="cg",
                                 conjugate_gradient=ConjugateGradient(thr, max_iterations=1200), **kw)
    one, chunked = cg(), cg(variance_chunk_bytes=8 * N * 8)
    assert chunked.variance_chunk_bytes // (N * 8) == 8 and -(-B // 8) == 5 and B % 8 == 5
    chol = models.GPR(data, kern, noise_variance=s2, solver="cholesky")
    for full_cov in (False, True):
        m0, v0 = chol.predict_f(T(Xs), full_cov=full_cov)
        m1, v1 = one.predict_f(T(Xs), full_cov=full_cov)
        m2, v2 = chunked.predict_f(T(Xs), full_cov=full_cov)
        assert v2.shape == v0.shape == ((1, B, B) if full_cov else (B, 1))
        assert torch.equal(m1, m2)  # the mean does not go through the chunks
        gap = float((v1 - v2).abs().max())
        print(f"gpr variance chunks {kind} full_cov={full_cov}: chunked - single {gap:.2e} (bar 1e-12)")
        assert float(v0.abs().max()) <= 1.0 + 1e-9 and gap <= 1e-12
        for v in (v1, v2):
            assert relmax(v, v0.cpu().numpy()) < 1e-6 and relmax(m2, m0.cpu().numpy()) < 1e-6


def test_gpr_caches_follow_parameters():
    X, Y, Xs = gpr_data(500, 2, seed=3)
    kern = kernels.SquaredExponential(1.0, [1.0, 1.0])
    m = models.GPR((T(X), T(Y)), kern, noise_variance=0.1, solver="cholesky")
    mu_a, _ = m.predict_f(T(Xs))
    L_a = m.cholesky()
    kern.lengthscales = [0.5, 0.5]
    mu_b, _ = m.predict_f(T(Xs))
    assert m.cholesky() is not L_a
    assert relmax(mu_b, gpr_posterior("se", 1.0, [0.5, 0.5], X, Y, 0.1, Xs)[0]) < 1e-9
    L_b = m.cholesky()
    m.likelihood.variance = 0.3
    assert m.cholesky() is not L_b
    ref = gpr_posterior("se", 1.0, [0.5, 0.5], X, Y, 0.3, Xs)
    assert abs(m.log_marginal_likelihood() - ref[3]) < 1e-9 * abs(ref[3])
    assert relmax(m.predict_f(T(Xs))[0], ref[0]) < 1e-9
    assert not torch.equal(mu_a, mu_b)


def test_gpr_factories_and_metrics():
    from cggp import cli_utils
    from cggp.likelihoods import Gaussian

    X, Y, Xs = gpr_data(600, 2, seed=4)
    data = (T(X), T(Y))
    m = cli_utils.gpr_class(data, kernels.Matern32(1.0, [1.0, 1.0]), Gaussian(0.2))
    assert isinstance(m, models.GPR) and m.likelihood.variance == 0.2
    g = cli_utils.create_gpr_model(data, None)
    assert g.likelihood.variance == 0.1 and g.kernel.name == "matern32"
    Ys = np.sin(Xs.sum(axis=1, keepdims=True) * 1.3)
    rmse, nlpd = models.rmse_nlpd(m, (T(Xs), T(Ys)), batch_size=40)
    mu, var, _, _ = gpr_posterior("matern32", 1.0, [1.0, 1.0], X, Y, 0.2, Xs)
    v = var + 0.2
    rmse0 = float(np.sqrt(np.mean((Ys - mu) ** 2)))
    nlpd0 = float(np.mean(0.5 * (np.log(2 * np.pi) + np.log(v) + (Ys - mu) ** 2 / v)))
    assert abs(rmse - rmse0) < 1e-9 and abs(nlpd - nlpd0) < 1e-9


# ---- 6. training ---------------------------------------------------------------------------------------------------------
def test_trainable_gpr_gradients_and_lbfgs():
    X, Y, Xs = gpr_data(400, 2, seed=5)
    model = training.TrainableGPR(kernels.Matern52(0.7, [0.5, 1.5]), 0.3, T(X), T(Y))
    params = model.parameters()
    loss = model.training_loss((model.X, model.Y))
    loss.backward()
    grads = [p.grad.clone() for p in params]
    h = 1e-6
    for p, g in zip(params, grads):
        for i in range(p.numel()):
            with torch.no_grad():
                p.view(-1)[i] += h
            lp = float(model.training_loss())
            with torch.no_grad():
                p.view(-1)[i] -= 2 * h
            lm = float(model.training_loss())
            with torch.no_grad():
                p.view(-1)[i] += h
            fd = (lp - lm) / (2 * h)
            assert abs(fd - float(g.view(-1)[i])) < 1e-5 * max(1.0, abs(fd))
    before = -float(model.training_loss())
    training.train_vanilla_using_lbfgs((model.X, model.Y), model, None, 15)
    after = -float(model.training_loss())
    assert after > before
    frozen = model.frozen_model()
    ls = model.kernel.lengthscales_p.value
    mu0, var0, _, lml0 = gpr_posterior("matern52", model.kernel.variance_p.value, ls, X, Y,
                                       model.likelihood_variance.value, Xs)
    mu, var = frozen.predict_f(T(Xs))
    assert relmax(mu, mu0) < 1e-8 and relmax(var, var0) < 1e-8
    assert abs(frozen.log_marginal_likelihood() - after) < 1e-8 * abs(after)
