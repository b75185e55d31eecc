"""The kernel forms behind libmgp's environment switches, against a plain high-precision reference.

One test per row of tests/switch_forms.py: a handle is made with the row's environment and installed as the
device's handle, so `ops.*`, the operators and `conjugate_gradient` all run on it.  fp64 products are checked
against a long-double restatement (`oracle.kernels.Kernel(..., dtype=np.longdouble)`), fp32 against fp64, k-step CG
iterates against `oracle/cg.py`; rows that change only timing or launch boundaries must also equal the default
handle's result bit for bit.  Last, the fused k^2 column sum (default handle), which feeds the SGPR Jacobi
preconditioner, against the long-double sum.
"""

import ctypes
import types

import numpy as np
import pytest
import torch

import switch_forms as sf
from gpr_reference import kxx_product
from oracle import cg as ocg
from oracle import kernels as ok
from oracle import models as om

pytestmark = pytest.mark.gpu

LD = np.longdouble


def dev():
    return torch.device("cuda:0")


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def relerr(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    if ref.size == 0:
        return 0.0
    scale = max(float(np.max(np.abs(ref))), 1e-300)
    return float(np.max(np.abs(got.astype(LD) - ref.astype(LD))) / scale)


def make_kernel(name, D, variance=1.3, seed=0, ls=None):
    from cggp import kernels
    if ls is None:
        ls = np.random.default_rng(seed).random(D) ** 2 + 0.5
    cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
           "matern52": kernels.Matern52}[name]
    return cls(variance=variance, lengthscales=ls), ls


def product_bar(name):
    # tests/test_gpu_parity.py::test_knm_kmn_matvec_fp64: 1e-11; Matern-1/2 1e-9 (cusp at r = 0)
    return 1e-9 if name == "matern12" else 1e-11


switched = sf.switched  # the context manager lives beside the table: tests/test_gpu_pair_accuracy.py runs its probes under the same rows


def rows_of(kind):
    return [r for r in sf.FORMS if r["entry"] == kind]


def row_params(kind):
    return [pytest.param(r, id=r["id"]) for r in rows_of(kind)]


# ---------------------------------------------------------------- sweeps
def _sweep_run(case, X, Z, V, W, ls):
    from cggp import ops
    from cggp.conjugate_gradient import SgprNormalOperator
    name, D, N, M, R, layout, sgpr = case
    k, _ = make_kernel(name, D, ls=ls)
    spec = k.spec(D)
    if layout == "cols":
        out = [ops.knm_matvec(spec, T(X), T(Z), T(V), ops.COLS), ops.kmn_matvec(spec, T(X), T(Z), T(W), ops.COLS)]
    else:
        out = [ops.knm_matvec(spec, T(X), T(Z), T(V.T), ops.ROWS).t(),
               ops.kmn_matvec(spec, T(X), T(Z), T(W.T), ops.ROWS).t()]
    if sgpr:  # the K_mn sweep with s2 K_mm p as its addend (mgp_operator_apply, MGP_OP_SGPR)
        out.append(SgprNormalOperator(k, T(X), T(Z), 0.1, jitter=1e-6).matmul(T(V)))
    torch.cuda.synchronize()
    return out


def _check_sweep(row, case, monkeypatch):
    name, D, N, M, R, layout, sgpr = case
    rng = np.random.default_rng(N * 31 + M * 7 + R + D)
    ls = rng.random(D) ** 2 + 0.5
    X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    V, W = rng.standard_normal((M, R)), rng.standard_normal((N, R))
    ko = ok.Kernel(name, 1.3, ls, dtype=LD)
    K = ko.K(X, Z)
    refs = [K @ V.astype(LD), K.T @ W.astype(LD)]
    if sgpr:
        Kmm = ok.Kuu(Z, ko, 1e-6)
        refs.append(LD(0.1) * (Kmm @ V.astype(LD)) + K.T @ (K @ V.astype(LD)))
    default = _sweep_run(case, X, Z, V, W, ls) if row.get("same_as_default") else None
    with switched(monkeypatch, row["env"]):
        got = _sweep_run(case, X, Z, V, W, ls)
    for i, (g, r) in enumerate(zip(got, refs)):
        assert g.shape == r.shape
        assert relerr(g, r) < product_bar(name), (case, i, relerr(g, r))  # test_knm_kmn_matvec_fp64's bar
        if default is not None:
            assert torch.equal(g, default[i]), (case, i)


def _check_extreme(row, case, monkeypatch):
    """tests/test_properties.py::test_gpu_fused_products_at_extreme_scales, its reference and its bar."""
    from cggp import ops
    name, D, N, M, ls_scale, x_scale, seed = case
    rng = np.random.default_rng(seed)
    ls = rng.uniform(0.5, 2.0, D) * ls_scale
    X = rng.standard_normal((N, D)) * x_scale
    Z = np.concatenate([X[: min(N, M // 2 + 1)], rng.standard_normal((M, D)) * x_scale])[:M]
    k, _ = make_kernel(name, D, variance=0.7, ls=ls)
    K = ok.Kernel(name, 0.7, ls).K(X, Z)
    V, W = rng.standard_normal((M, 2)), rng.standard_normal((N, 2))
    r2max = 2.0 * float(np.max(np.sum((X / ls) ** 2, axis=1)) + np.max(np.sum((Z / ls) ** 2, axis=1)))
    tol = max(1e-11, 4e-16 * r2max) * (10.0 if name != "matern12" else 3e4)
    if name == "matern12":
        tol = max(tol, 2.0 * np.sqrt(4e-16 * r2max))
    with switched(monkeypatch, row["env"]):
        u = ops.knm_matvec(k.spec(D), T(X), T(Z), T(V)).cpu().numpy()
        t = ops.kmn_matvec(k.spec(D), T(X), T(Z), T(W)).cpu().numpy()
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(t))
    assert np.max(np.abs(u - K @ V)) <= tol * 0.7 * (1 + np.abs(V).sum(0).max()), case
    assert np.max(np.abs(t - K.T @ W)) <= tol * 0.7 * (1 + np.abs(W).sum(0).max()), case


@pytest.mark.parametrize("row", row_params("sweep"))
def test_sweep_form(row, monkeypatch):
    for case in row["cases"]:
        if len(case) == 7 and isinstance(case[5], str):
            _check_sweep(row, case, monkeypatch)
        else:
            _check_extreme(row, case, monkeypatch)


@pytest.mark.parametrize("case", sf.CHUNK_CASES, ids=lambda c: f"{c[1]}_D{c[2]}_M{c[4]}_R{c[5]}_{c[6]}")
def test_sweep_chunk_decodes(case, monkeypatch):
    """Each block decode of sweep_fast_kernel, one and several right-hand sides (the branch each case takes is
    checked on the CPU, tests/test_switch_inventory.py)."""
    from cggp import ops
    env, name, D, N, M, R, _ = case
    rng = np.random.default_rng(M + R)
    ls = rng.random(D) ** 2 + 0.5
    X, Z, V = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((M, R))
    k, _ = make_kernel(name, D, ls=ls)
    ref = ok.Kernel(name, 1.3, ls, dtype=LD).K(X, Z) @ V.astype(LD)
    with switched(monkeypatch, env):
        out = ops.knm_matvec(k.spec(D), T(X), T(Z), T(V))
    assert relerr(out, ref) < product_bar(name)


@pytest.mark.parametrize("row", row_params("sweep32"))
def test_sweep_fp32_form(row, monkeypatch):
    from cggp import ops
    for name, D, N, M, R in row["cases"]:
        rng = np.random.default_rng(N + M)
        ls = rng.random(D) ** 2 + 0.5
        X, Z, V = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((M, R))
        k, _ = make_kernel(name, D, ls=ls)
        ko = ok.Kernel(name, 1.3, ls)
        ref = np.concatenate([ko.K(X[i:i + 32768], Z) @ V for i in range(0, N, 32768)])
        with switched(monkeypatch, row["env"]):
            out = ops.knm_matvec(k.spec(D), T(X, torch.float32), T(Z, torch.float32), T(V, torch.float32))
        assert relerr(out, ref) < 2e-4  # fp32 against fp64, test_sweep_fp32's bar


@pytest.mark.parametrize("row", row_params("kxx"))
def test_kxx_form(row, monkeypatch):
    from cggp import ops
    for name, D, N in row["cases"]:
        rng = np.random.default_rng(N + D)
        ls = rng.random(D) ** 2 + 0.5
        X, V = rng.standard_normal((N, D)), rng.standard_normal((N, 1))
        k, _ = make_kernel(name, D, ls=ls)
        ref = kxx_product(name, 1.3, ls, X, 0.1, V)
        with switched(monkeypatch, {"MGP_KXX": "sym"}):
            sym = ops.kxx_matvec(k.spec(D), T(X), 0.1, T(V))
        with switched(monkeypatch, row["env"]):
            got = ops.kxx_matvec(k.spec(D), T(X), 0.1, T(V))
        assert relerr(got, ref) < 1e-11  # tests/test_gpu_gpr.py::test_kxx_matches_longdouble
        assert torch.equal(got, sym)


# ---------------------------------------------------------------- dense
def _sym_problem(n, Bt, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A = A + A.T
    return A, rng.standard_normal((Bt, n))


@pytest.mark.parametrize("row", row_params("symm1"))
def test_symm_gemv_form(row, monkeypatch):
    """The upper-triangle one-RHS product from n = 64 on: lower triangle poisoned below the diagonal tiles."""
    from cggp import ops
    for n in row["cases"]:
        A, P = _sym_problem(n, 1, n)
        ref = P.astype(LD) @ A.astype(LD)
        Ap = A.copy()
        Ap[np.tril_indices(n, -64)] = np.nan
        with switched(monkeypatch, row["env"]):
            for dt, bar in ((torch.float64, 1e-13), (torch.float32, 2e-5)):  # test_symm_gemv_upper_triangle_path
                out = ops.symm_matmul(T(A, dt), T(P, dt))
                assert relerr(out, ref) < bar, (n, dt)
                assert torch.equal(out, ops.symm_matmul(T(Ap, dt), T(P, dt))), (n, dt)


@pytest.mark.parametrize("row", row_params("symm"))
def test_symm_matmul_form(row, monkeypatch):
    from cggp import ops
    for n, Bt in row["cases"]:
        A, P = _sym_problem(n, Bt, n * 7 + Bt)
        # long double where it is cheap; the GEMM shapes keep test_symm_matmul_ragged_gemm_regime's fp64 numpy reference
        ref = P.astype(LD) @ A.astype(LD) if Bt * n * n <= 4e7 else P @ A
        default = ops.symm_matmul(T(A), T(P)) if row.get("same_as_default") else None
        with switched(monkeypatch, row["env"]):
            out = ops.symm_matmul(T(A), T(P))
            out2 = ops.symm_matmul(T(A), T(P))
        assert relerr(out, ref) < 1e-12, (n, Bt)  # test_symm_matmul_fp64
        assert torch.equal(out, out2)
        if default is not None:
            assert torch.equal(out, default), (n, Bt)


@pytest.mark.parametrize("row", row_params("k_dense"))
def test_k_dense_form(row, monkeypatch):
    from cggp import ops
    for name, D, NA, NB in row["cases"]:
        rng = np.random.default_rng(NA * 3 + D)
        ls = rng.random(D) ** 2 + 0.5
        A, B = rng.standard_normal((NA, D)), rng.standard_normal((NB, D))
        k, _ = make_kernel(name, D, ls=ls)
        ref = ok.Kernel(name, 1.3, ls, dtype=LD).K(A, B)
        with switched(monkeypatch, row["env"]):
            for dt, bar in ((torch.float64, 1e-12), (torch.float32, 3e-5)):  # tests/test_gpu_parity.py::test_k_dense
                out = ops.k_dense(k.spec(D), T(A, dt), T(B, dt))
                assert out.shape == (NA, NB) and relerr(out, ref) < bar, (name, D, NA, dt)


# ---------------------------------------------------------------- CG on a dense matrix
def _cg_problem(n, Bt):
    """K_SE(Z, Z) + Lambda with a cluster-count-like diagonal, as tests/test_gpu_dense1.py."""
    rng = np.random.default_rng(n * 11 + Bt)
    Z = rng.standard_normal((n, 3))
    kern = ok.Kernel("se", 1.3, rng.random(3) ** 2 + 0.5)
    A = om.add_diagonal(kern.K(Z), 0.1 / rng.integers(1, 40, n).astype(np.float64))
    return A, rng.standard_normal((Bt, n))


@pytest.mark.parametrize("row", row_params("cg"))
def test_dense_cg_form(row, monkeypatch):
    from cggp.conjugate_gradient import conjugate_gradient
    for n, Bt in row["cases"]:
        A, rhs = _cg_problem(n, Bt)
        for k in (1, 6):
            run = lambda: conjugate_gradient(T(A), T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
            default = run()[0] if row.get("same_as_default") else None
            with switched(monkeypatch, row["env"]):
                sol, (steps, err) = run()
            o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, n)), 0.0, max_iterations=k,
                                                             max_steps_cycle=k + 1)
            assert int(steps) == k == o_steps
            for b in range(Bt):
                assert relerr(sol[b], o_sol[b]) < 1e-9, (n, Bt, k, b)  # test_cg_fixed_iterations_match_oracle
            if default is not None:
                assert torch.equal(sol, default), (n, Bt, k)


# ---------------------------------------------------------------- contraction
def _panel_n(env, M, es):
    nz = int(env.get("MGP_CONTRACT_NZ", 16))
    rows = (int(env.get("MGP_CONTRACT_PANEL_MB", 2048)) << 20) // (M * es)
    rows = max(rows // (16 * nz) * (16 * nz), 16 * nz)
    return 2 * rows + 37  # two full panels and a ragged tail (contract.hip, kmn_knm_two_stage)


@pytest.mark.parametrize("row", row_params("contract"))
def test_contraction_form(row, monkeypatch):
    from cggp import ops
    for name, D, N, M, dtn in row["cases"]:
        dt, es = (torch.float64, 8) if dtn == "f64" else (torch.float32, 4)
        if N is None:
            N = _panel_n(row["env"], M, es)
        rng = np.random.default_rng(N + M)
        ls = rng.random(D) ** 2 + 0.5
        X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
        k, _ = make_kernel(name, D, ls=ls)
        K = ok.Kernel(name, 1.3, ls, dtype=LD).K(X, Z)
        # K^T K from the long-double K, split into two fp64 parts: the fp64 sums of positive terms (N eps <= 6e-11
        # relative at N = 2.6e5, M = 1; <= 5e-13 at the other sizes) stay under the bar
        hi = K.astype(np.float64)
        lo = (K - hi).astype(np.float64)
        ref = hi.T @ hi + (hi.T @ lo + lo.T @ hi)
        with switched(monkeypatch, row["env"]):
            KK = ops.kmn_knm(k.spec(D), T(X, dt), T(Z, dt))
        bar = 1e-11 if dt == torch.float64 else 2e-4  # tests/test_gpu_parity.py::test_kmn_knm / _fp32_and_ragged
        assert KK.shape == (M, M) and relerr(KK, ref) < bar, (name, N, M, dtn, relerr(KK, ref))
        assert torch.equal(KK, KK.t())  # the upper triangle is mirrored


# ---------------------------------------------------------------- one-rank communicator, unfused agreement
@pytest.mark.parametrize("row", row_params("comm"))
def test_fuse_agree_form(row, monkeypatch):
    """The native-collective SGPR solve of tests/test_gpu_rccl.py on a one-rank communicator (mgp_comm_init_all):
    the agreement launches of their own give the same bits as the fused form and the no-collective solve."""
    from cggp import _hip, kernels
    from cggp.conjugate_gradient import ConjugateGradient, SgprNormalOperator
    lib = _hip.load_library()
    comms = (ctypes.c_void_p * 1)()
    devs = (ctypes.c_int * 1)(0)
    assert lib.mgp_comm_init_all(1, devs, comms) == 0, lib.mgp_comm_last_error()
    comm = types.SimpleNamespace(ptr=ctypes.c_void_p(comms[0]))
    ar = types.SimpleNamespace(comm=comm, world_size=1)
    try:
        rng = np.random.default_rng(0)
        N, D, M = 6000, 3, 64
        X = rng.standard_normal((N, D))
        Z = X[rng.choice(N, M, replace=False)]
        rhs = rng.standard_normal((M, 2))
        for (dtn,) in row["cases"]:
            dt = torch.float64 if dtn == "f64" else torch.float32
            Xt, Zt, bt = T(X, dt), T(Z, dt), T(rhs, dt)
            kern = kernels.Matern32(1.2, [0.8, 1.0, 1.3])
            thr = 1e-12 if dt == torch.float64 else 1e-3
            cg = ConjugateGradient(thr, max_iterations=500, check_every=7)

            def solve(collective):
                op = SgprNormalOperator(kern, Xt, Zt, 0.1, jitter=1e-6, allreduce=ar if collective else None,
                                        kmm_rows=(0, M) if collective else None)
                if collective:
                    st, _ = op._struct()
                    assert st.comm and not st.allreduce
                s, (k, e) = cg.solve_with_stats(op, bt)
                torch.cuda.synchronize()
                return s, int(k), e

            s0, k0, e0 = solve(False)
            sf_, kf, ef = solve(True)
            with switched(monkeypatch, row["env"]):
                su, ku, eu = solve(True)
            assert 1 < k0 < 500 and k0 == kf == ku
            assert torch.equal(su, sf_) and torch.equal(su, s0) and torch.equal(eu, e0) and torch.equal(ef, e0)
    finally:
        torch.cuda.synchronize()
        lib.mgp_comm_destroy(comm.ptr)


# ---------------------------------------------------------------- fused k^2 column sum (default handle)
SQ_SHAPES = [(0, 5), (1, 1), (63, 65), (257, 63), (700, 257), (65, 1), (1030, 17), (4097, 3), (300, 300), (2, 130)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sf.KINDS)
def test_kmn_sq_colsum(name, dtype):
    """diag(K_mn K_nm) = sum_i k(x_i, z_m)^2 through sweep_kernel<T, DP, KIND, 1, SQ = true> at every DP tier."""
    from cggp import ops
    for D, (N, M) in zip([1, 2, 3, 4, 5, 8, 9, 16, 17, 32], SQ_SHAPES):
        rng = np.random.default_rng(D * 13 + N)
        ls = rng.random(D) ** 2 + 0.5
        X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
        k, _ = make_kernel(name, D, ls=ls)
        out = ops.kmn_sq_colsum(k.spec(D), T(X, dtype), T(Z, dtype))
        if N == 0:
            assert float(out.abs().max()) == 0.0
            continue
        if dtype == torch.float64:
            K = ok.Kernel(name, 1.3, ls, dtype=LD).K(X, Z)
            bar = product_bar(name)
        else:
            K = ok.Kernel(name, 1.3, ls).K(X, Z)
            bar = 2e-4
        ref = np.sum(K * K, axis=0)
        assert out.shape == (M,) and relerr(out, ref) < bar, (D, N, M, relerr(out, ref))


@pytest.mark.parametrize("name,D", [("se", 3), ("matern52", 17), ("matern32", 32), ("matern12", 8)])
def test_sgpr_operator_diag(name, D):
    """SgprNormalOperator.diag() -- the SGPR Jacobi preconditioner -- against diag(S) = s2 diag(K_mm) + sum_i k^2,
    the sum in long double.  diag(K_mm) is the operator's own: at coincident points the expansion's rounding of r2
    leaves ~1e-7 of k for Matern-1/2 (tests/test_gpu_parity.py::test_k_dense checks it), and is not what is tested."""
    from cggp.conjugate_gradient import SgprNormalOperator
    rng = np.random.default_rng(D)
    ls = rng.random(D) ** 2 + 0.5
    X, Z = rng.standard_normal((1500, D)), rng.standard_normal((90, D))
    k, _ = make_kernel(name, D, ls=ls)
    K = ok.Kernel(name, 1.3, ls, dtype=LD).K(X, Z)
    op = SgprNormalOperator(k, T(X), T(Z), 0.1, jitter=1e-6)
    ref = LD(0.1) * op.Kmm.diagonal().cpu().numpy().astype(LD) + np.sum(K * K, axis=0)
    assert relerr(op.diag(), ref) < product_bar(name)
