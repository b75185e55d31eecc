"""The many-column form of the matrix-free (K_mm + Lambda) operator above 32 dimensions, `MGP_OP_KMM_LAMBDA_WIDE_ANYD`
(csrc/kmm_wide_anyd.hip under csrc/cg.hip's `apply_operator`), at the smallest shapes at which each of its parts can go
wrong.

Every output is held to the bound include/mgp_sweep_anyd.h states (tests/kmm_wide_anyd_reference.py: the per-pair
bound of the expansion-form distance, the chain of one split, the sum of the splits, no fitted constant) against long
double: single kernel values through one-hot right-hand sides at every K-slice and tile seam, dense right-hand sides at
every group seam.  Then the routes (which kind `kind_for` hands out, agreement with `MGP_OP_KMM_LAMBDA`, the bits of
the kinds it falls back to), memory and reproducibility, the argument checks, the kind under `mgp_pcg_solve` and
`mgp_pcg_solve_record` against oracle/cg.py, and `wide_anyd` on `CGGP` and `TrainableCGGP`.

Without the feature kind 8 is MGP_E_BADARG ("unknown operator kind 8") and `wide_anyd=` a TypeError: every test of this
file but the fallback-bits ones fails on the parent."""

import ctypes

import numpy as np
import pytest
import torch

import kmm_wide_anyd_plan as wp
import kmm_wide_anyd_reference as wr
import pair_reference as pr
from buffer_contract import Guarded
from cggp import _hip, ops
from test_gpu_kmm_wide import T, apply, apply_rc, fresh_handle, prj_bytes, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VAR = wr.VARIANCE
LD = np.longdouble
F64 = np.float64
KIND_SWEEP, KIND_WIDE, KIND_ANYD, KIND = 2, 4, 6, wp.KIND
MGP_E_BADARG, MGP_E_SHAPE, MGP_E_DTYPE, MGP_E_NOMEM = -1, -2, -3, -6  # include/mgp.h


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def handle():
    lib, h = fresh_handle()
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


def spec_of(name, ls, D):
    return ops.KernelSpec(name, VAR, list(ls), D)


def worst_ratio(got, want, bound):
    err = np.abs(np.asarray(got).astype(LD) - want)
    assert np.all(np.isfinite(np.asarray(got)))
    return float((err / bound).max())


# ---------------------------------------------------------------- single kernel values
_PAIR_REF = {}


def pair_reference(name, D):
    """One cloud of max(PAIR_SIZES) points per (kind, D); the first M of them are the Z of size M.  The reference
    columns are the union of the probed ones: computed once, shared by every size."""
    if (name, D) not in _PAIR_REF:
        Z, ls, _ = wr.inputs(D, max(wp.PAIR_SIZES))
        cols = sorted({c for M in wp.PAIR_SIZES for c in wp.probed(M)})
        pv, rel = wr.kernel_columns(name, ls, Z, cols)
        _PAIR_REF[(name, D)] = (Z, ls, cols, pv.k, rel)
    return _PAIR_REF[(name, D)]


@pytest.mark.parametrize("D", wp.PAIR_DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_single_kernel_values(handle, name, D):
    """One-hot right-hand sides return single kernel values (the other terms are k * 0 = 0, lambda = 0): every probed
    column of k(Z, Z) against long double within the header's bound."""
    Z, ls, cols, K, rel = pair_reference(name, D)
    spec = spec_of(name, ls, D)
    worst = 0.0
    for M in wp.PAIR_SIZES:
        mine = wp.probed(M)
        at = [cols.index(c) for c in mine]
        P = np.zeros((len(mine), M))
        P[np.arange(len(mine)), mine] = 1.0
        got = apply(handle, KIND, spec, T(Z[:M]), T(np.zeros(M)), T(P)).cpu().numpy()  # [C, M] = k(Z[mine], Z)
        want = K[:M, at].T
        _, nsplit, rows = wp.split_plan(M, cus())
        bound = (rel[:M, at].T + (rows + nsplit + 3) * wr.U) * want  # the header's bound at a one-hot P, lambda = 0
        ratio = worst_ratio(got, want, bound)
        assert ratio <= 1.0, (name, D, M, ratio)
        worst = max(worst, ratio)
    assert wp.split_plan(391, cus())[1] == 2 and wp.split_plan(129, cus())[1] == 1  # a split and an unsplit streamed side
    print(f"kmm-wide-anyd pairs {name} D={D}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------- dense right-hand sides
_DENSE_REF = {}


def dense_reference(name, D, M):
    if (name, D, M) not in _DENSE_REF:
        Z, ls, lam = wr.inputs(D, M, seed=1)
        pv, rel = wr.kernel_columns(name, ls, Z)
        _DENSE_REF[(name, D, M)] = (Z, ls, lam, pv.k, rel * pv.k)
    return _DENSE_REF[(name, D, M)]


DENSE_CASES = [(pr.KINDS[i % 4], wp.DENSE_D, wp.DENSE_M, Bt) for i, Bt in enumerate(wp.WIDTHS)] + [
    ("matern52", 34, 129, 17), ("se", 512, 70, 40), ("matern12", 33, 391, 300)]


@pytest.mark.parametrize("name,D,M,Bt", DENSE_CASES)
def test_dense_right_hand_sides(handle, name, D, M, Bt):
    """Random P, random positive lambda, against the long-double product within the header's bound; a second call
    gives the same bits."""
    Z, ls, lam, K, pairb = dense_reference(name, D, M)
    P = np.random.default_rng([3, Bt, M]).standard_normal((Bt, M))
    spec = spec_of(name, ls, D)
    Zt, lt, Pt = T(Z), T(lam), T(P)
    got = apply(handle, KIND, spec, Zt, lt, Pt)
    ratio = worst_ratio(got.cpu().numpy(), wr.product(K, lam, P), wr.product_bound(K, pairb, lam, P, M, cus()))
    print(f"kmm-wide-anyd dense {name} D={D} M={M} columns={Bt}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert same_bits(got, apply(handle, KIND, spec, Zt, lt, Pt))


# ---------------------------------------------------------------- routes
def test_kind_for_hands_out_the_kind_only_where_it_serves():
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator
    mk = lambda D, dtype, **kw: KmmLambdaOperator(kernels.SquaredExponential(VAR, [1.5] * D), T(np.zeros((40, D)), dtype),
                                                  T(np.ones(40), dtype), **kw)
    f64, f32 = torch.float64, torch.float32
    for cols in (1, 48, 300):
        assert mk(33, f64, wide_anyd=True).kind_for(cols) == 8 == _hip.OP_KMM_LAMBDA_WIDE_ANYD
        assert mk(33, f64, wide_anyd=True, wide=True, fused_anyd=True).kind_for(cols) == 8  # asked first
        assert mk(33, f64).kind_for(cols) == 2 and mk(33, f64, wide_anyd=False, fused_anyd=True).kind_for(cols) == 6
        assert mk(32, f64, wide_anyd=True).kind_for(cols) == 2 and mk(32, f64, wide_anyd=True, wide=True).kind_for(cols) == 4
        assert mk(40, f32, wide_anyd=True).kind_for(cols) == 2 and mk(40, f32, wide_anyd=True, fused_anyd=True).kind_for(cols) == 6
    from cggp import conjugate_gradient as cgm
    auto = mk(33, f64, wide_anyd="auto")
    assert auto.kind_for(256) == (8 if cgm.wide_anyd_auto(f64, 33, 256, 40) else 2)
    with pytest.raises(ValueError):
        mk(33, f64, wide_anyd="yes")


@pytest.mark.parametrize("name,D", [("se", 33), ("matern32", 77)])
def test_agrees_with_the_plain_kind(handle, name, D):
    """Kind 8 against MGP_OP_KMM_LAMBDA (kernel panels, direct differences) on the same inputs, within the sum of the
    two bounds: the plain kind is granted the same bound (its distance is the better one, its sums are as long)."""
    M = wp.DENSE_M
    Z, ls, lam, K, pairb = dense_reference(name, D, M)
    spec = spec_of(name, ls, D)
    for Bt in (20, 257):
        P = np.random.default_rng([4, Bt]).standard_normal((Bt, M))
        wide = apply(handle, KIND, spec, T(Z), T(lam), T(P)).cpu().numpy()
        plain = apply(handle, KIND_SWEEP, spec, T(Z), T(lam), T(P)).cpu().numpy()
        bound = 2 * wr.product_bound(K, pairb, lam, P, M, cus())
        ratio = float((np.abs(wide.astype(LD) - plain.astype(LD)) / bound).max())
        print(f"kmm-wide-anyd against the plain kind {name} D={D} columns={Bt}: worst difference / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("D,dtype,other", [(8, torch.float64, KIND_WIDE), (32, torch.float64, KIND_WIDE),
                                           (40, torch.float32, KIND_SWEEP)], ids=["D8", "D32", "fp32-D40"])
def test_fallback_bits(D, dtype, other):
    """fp64 at D <= 32 runs the code of MGP_OP_KMM_LAMBDA_WIDE, fp32 that of MGP_OP_KMM_LAMBDA: their bits."""
    hd = fresh_handle()
    try:
        M = 300
        Z, ls, lam = wr.inputs(D, M, seed=2)
        spec = spec_of("matern32", ls, D)
        for Bt in (1, 70, 257):
            Pt = T(np.random.default_rng([5, Bt]).standard_normal((Bt, M)), dtype)
            a = apply(hd, KIND, spec, T(Z, dtype), T(lam, dtype), Pt)
            b = apply(hd, other, spec, T(Z, dtype), T(lam, dtype), Pt)
            assert same_bits(a, b), (D, Bt)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- memory and reproducibility
CONTRACT = dict(name="matern32", D=62, M=391, Bt=70)  # two splits, a ragged group, a ragged last tile, two whole K slices


def _contract_inputs():
    c = CONTRACT
    Z, ls, lam = wr.inputs(c["D"], c["M"], seed=3)
    return spec_of(c["name"], ls, c["D"]), Z, lam, np.random.default_rng(6).standard_normal((c["Bt"], c["M"]))


def test_guard_bands_inputs_and_repeats():
    """Guard bands around out untouched; P, Z, lambda unchanged; buffers one element off a 16-byte boundary and a
    repeated call give the same bits."""
    spec, Z, lam, P = _contract_inputs()
    M, Bt = CONTRACT["M"], CONTRACT["Bt"]
    vals = dict(Z=Z, lam=lam, P=P)
    hd = fresh_handle()
    try:
        ref = None
        for offsets in ({}, {}, {"P": 1, "out": 1}, {"Z": 1, "lam": 1, "P": 1, "out": 1}):
            g = {k: Guarded(v.shape, torch.float64, offsets.get(k, 0), DEV) for k, v in vals.items()}
            g["out"] = Guarded((Bt, M), torch.float64, offsets.get("out", 0), DEV)
            for k, v in vals.items():
                g[k].upload(torch.from_numpy(v))
            torch.cuda.synchronize()
            rc = apply_rc(hd, KIND, spec, g["Z"].ptr, g["lam"].ptr, g["P"].ptr, g["out"].ptr, M, Bt)
            assert rc == 0, (rc, hd[0].mgp_last_error(hd[1]))
            torch.cuda.synchronize()
            g["out"].check_output(None, name="kmm-wide-anyd out")
            for k in vals:
                g[k].check_input(name=f"kmm-wide-anyd {k}")
            if ref is None:
                ref = g["out"].payload.clone()
                assert prj_bytes(hd) >= wp.arena_bytes(M, CONTRACT["D"], Bt, cus())  # this route ran
            assert same_bits(g["out"].payload, ref), offsets
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


@pytest.mark.parametrize("earlier", ["knm_project", "wide-D8"])
def test_stale_arena_does_not_reach_the_result(handle, earlier):
    """Another user of the prj arena leaves NaN there (its pack, its split tiles); the call that follows gives the bits
    of a fresh handle."""
    spec, Z, lam, P = _contract_inputs()
    clean = apply(handle, KIND, spec, T(Z), T(lam), T(P))
    hd = fresh_handle()
    try:
        lib, h = hd
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        D8 = 8
        spec8 = spec_of("se", np.ones(D8), D8)
        if earlier == "knm_project":
            B, N, r = 2048, 2048, 128
            Xs, X, R = nan(B, D8), nan(N, D8), nan(N, r)
            proj = torch.empty((B, r), dtype=torch.float64, device=DEV)
            k = spec8.struct(_hip.F64)
            assert lib.mgp_knm_project(h, ctypes.byref(k), _hip.ptr(Xs), B, _hip.ptr(X), N, _hip.ptr(R), r, ops.COLS,
                                       _hip.ptr(proj), None) == 0
            torch.cuda.synchronize()
            assert bool(torch.isnan(proj).all())
        else:
            M8 = 2048
            out8 = apply(hd, KIND_WIDE, spec8, nan(M8, D8), nan(M8), nan(256, M8))
            assert bool(torch.isnan(out8).all())
        before = prj_bytes(hd)
        assert before >= wp.arena_bytes(CONTRACT["M"], CONTRACT["D"], CONTRACT["Bt"], cus())  # reused, not grown
        got = apply(hd, KIND, spec, T(Z), T(lam), T(P))
        assert prj_bytes(hd) == before and same_bits(got, clean)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


def test_fixed_pool_of_the_documented_bytes():
    """A fixed pool of exactly the header's formula serves the call; one of 256 bytes less is MGP_E_NOMEM."""
    spec, Z, lam, P = _contract_inputs()
    M, D, Bt = CONTRACT["M"], CONTRACT["D"], CONTRACT["Bt"]
    Zt, lt, Pt = T(Z), T(lam), T(P)
    grow = fresh_handle()
    try:
        ref = apply(grow, KIND, spec, Zt, lt, Pt)
    finally:
        grow[0].mgp_destroy(grow[1])
    need = wp.arena_bytes(M, D, Bt, cus())
    for pool, want in ((need, 0), (need - 256, MGP_E_NOMEM)):
        hd = fresh_handle(pool)
        try:
            out = torch.empty_like(Pt)
            rc = apply_rc(hd, KIND, spec, Zt, lt, Pt, out, M, Bt)
            torch.cuda.synchronize()
            assert rc == want, (pool, rc, hd[0].mgp_last_error(hd[1]))
            if want:
                assert b"fixed workspace exhausted" in hd[0].mgp_last_error(hd[1])
            else:
                assert same_bits(out, ref) and int(hd[0].mgp_workspace_bytes(hd[1])) == need
        finally:
            torch.cuda.synchronize()
            hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- argument checks
def test_argument_checks(handle):
    """The checks of MGP_OP_KMM_LAMBDA, as return codes of one-shot calls."""
    lib, h = handle
    spec, Z, lam, P = _contract_inputs()
    M, Bt = CONTRACT["M"], CONTRACT["Bt"]
    Zt, lt, Pt = T(Z), T(lam), T(P)
    out = torch.empty_like(Pt)

    def call(n=M, m=M, lam_ptr=lt.data_ptr(), dtype=None, bt=Bt):
        k = spec.struct(_hip.F64)
        st = _hip.MgpOperator()
        st.kind, st.dtype = KIND, k.dtype if dtype is None else dtype
        st.kernel = ctypes.pointer(k)
        st.Z, st.lam, st.n, st.M = Zt.data_ptr(), lam_ptr, n, m
        return lib.mgp_operator_apply(h, ctypes.byref(st), ctypes.c_void_p(Pt.data_ptr()), bt, ctypes.c_void_p(out.data_ptr()))

    assert call() == 0
    assert call(m=M - 1) == MGP_E_SHAPE
    assert call(lam_ptr=0) == MGP_E_BADARG
    assert call(dtype=7) == MGP_E_DTYPE
    assert call(dtype=_hip.F32) == MGP_E_DTYPE  # operator / kernel dtype mismatch
    assert call(bt=0) == 0 and call(bt=-1) == MGP_E_SHAPE
    torch.cuda.synchronize()


# ---------------------------------------------------------------- inside mgp_pcg_solve
def cg_problem(D, M=300, seed=41, latent=8, ell=1.2):
    """Points in a `latent`-dimensional subspace of R^D (a spread spectrum, as tests/test_gpu_sweep_anyd.py's
    `cg_points`), lambda in [0.1, 0.5) * variance ... so that the condition number is about 60."""
    rng = np.random.default_rng([seed, D, M])
    Q, _ = np.linalg.qr(rng.standard_normal((D, latent)))
    Z = rng.standard_normal((M, latent)) @ Q.T
    lam = 0.1 * VAR + 0.4 * rng.random(M)
    return Z, np.full(D, ell), lam


# decades by which the right-hand sides are scaled down, cycled over the columns: unscaled columns, and columns whose
# 0.5-free |r|^2 or p.Ap falls through min_float = 1e-16 at different steps (or stands below it from the start)
CG_DECADES = (0.0, 0.0, 7.0, 8.45, 8.6, 8.75, 8.9, 9.5)
_CG_REF = {}


def cg_reference(D):
    if D not in _CG_REF:
        Z, ls, lam = cg_problem(D)
        pv, rel = wr.kernel_columns("se", ls, Z)
        A = (pv.k + np.diag(lam.astype(LD))).astype(F64)
        eps = float(rel.max()) + wr.U * (sum(wp.split_plan(Z.shape[0], cus())[1:]) + 3)
        _CG_REF[D] = (Z, ls, lam, A, eps)
    return _CG_REF[D]


def cg_rhs(A, Bt, steps):
    """Standard normal right-hand sides scaled down by CG_DECADES; a column one of whose guard operands (p.Ap, |r|^2 on
    the host recurrence) comes within a factor 1.25 of min_float is scaled by 0.8 until none does."""
    dec = np.array([CG_DECADES[b % len(CG_DECADES)] for b in range(Bt)])
    rhs = np.random.default_rng([7, Bt]).standard_normal((Bt, A.shape[0])) * 10.0 ** -dec[:, None]
    for _ in range(20):
        both = np.concatenate(wr.cg_trace(A, rhs, steps))
        close = np.any((both > 1e-16 / 1.25) & (both < 1e-16 * 1.25), axis=0)
        if not close.any():
            return rhs
        rhs[close] *= 0.8
    raise AssertionError("no margin around min_float")


class PerturbedMatrix:
    """A for oracle/cg.py with every product off by `eps` of its sum of magnitudes, at random."""

    def __init__(self, A, eps, seed):
        self.A, self.eps, self.rng, self.shape = A, eps, np.random.default_rng(seed), A.shape

    def rmatmul(self, p):
        out = p @ self.A
        return out + self.eps * self.rng.standard_normal(out.shape) * (np.abs(p) @ np.abs(self.A))


def column_distance(got, want):
    top = np.max(np.abs(want), axis=1)
    assert not np.any(got[top == 0]), "a column the oracle leaves at zero is not exactly zero"
    return float((np.max(np.abs(got - want), axis=1) / np.where(top > 0, top, 1.0)).max())


@pytest.mark.parametrize("Bt", [20, 260])
@pytest.mark.parametrize("D", [33, 77])
def test_pcg_solve_fixed_steps_against_the_oracle(D, Bt):
    """mgp_pcg_solve and mgp_pcg_solve_record on kind 8 after 5 steps (threshold 0) against oracle/cg.py on the
    float64 dense matrix, every column within 1e-9 of the oracle's (relative to the column's largest entry).

    Conditioning, checked on the CPU before these inputs were fixed and asserted here: lambda >= 0.1 variance keeps
    the condition number near 60, and the oracle on `PerturbedMatrix` with eps = the bound of one product of the kind
    (3e-13) stays within 1e-10 of the oracle on A after 5 steps, so the recurrence does not carry the kernel's rounding
    past 1e-9.  The gate: the right-hand sides are scaled by CG_DECADES, so columns freeze (p.Ap or |r|^2 at or below
    min_float = 1e-16) at different steps; no guard's operand lies within 5 % of min_float on the host recurrence, so
    the device, 1e-12 away, takes every guard the way the oracle does."""
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator, conjugate_gradient
    from oracle import cg as ocg
    Z, ls, lam, A, eps = cg_reference(D)
    M, k = Z.shape[0], 5
    rhs = cg_rhs(A, Bt, k)
    den, rz = wr.cg_trace(A, rhs, k)
    both = np.concatenate([den, rz])
    assert not np.any((both > 1e-16 / 1.05) & (both < 1e-16 * 1.05))
    hit = [int(np.argmax((den[:, b] <= 1e-16) | (rz[:, b] <= 1e-16))) if np.any((den[:, b] <= 1e-16) | (rz[:, b] <= 1e-16))
           else -1 for b in range(Bt)]
    assert len(set(hit)) >= 3 and -1 in hit and 0 in hit, sorted(set(hit))  # never, from the start, and in between
    zero = np.zeros((Bt, M))
    o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, zero, 0.0, max_iterations=k, max_steps_cycle=k + 1)
    exact = np.linalg.solve(A, rhs[0])
    assert np.linalg.norm(o_sol[0] - exact) > 1e-4 * np.linalg.norm(exact)  # an iterate, not a limit
    p_sol, _ = ocg.conjugate_gradient(PerturbedMatrix(A, eps, 0), rhs, zero, 0.0, max_iterations=k, max_steps_cycle=k + 1)
    assert column_distance(p_sol, o_sol) < 1e-10, eps
    op = KmmLambdaOperator(kernels.SquaredExponential(VAR, list(ls)), T(Z), T(lam), wide_anyd=True)
    assert op.kind_for(Bt) == 8
    sol, (steps, err) = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
    torch.cuda.synchronize()
    d = column_distance(sol.cpu().numpy(), o_sol)
    print(f"kmm-wide-anyd pcg D={D} columns={Bt}: column distance to the oracle {d:.2e} (bar 1e-09), eps {eps:.1e}")
    assert int(steps) == k == o_steps and d < 1e-9
    r_sol, r_err, r_st, coef = ops.pcg_solve_record(op, T(rhs), 0.0, k)
    torch.cuda.synchronize()
    assert r_st.iterations == k and coef.shape == (k, Bt, 3)
    assert column_distance(r_sol.cpu().numpy(), o_sol) < 1e-9
    again, _ = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
    assert same_bits(again, sol)


def test_converged_solve_against_numpy():
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator, conjugate_gradient
    Z, ls, lam, A, _ = cg_reference(77)
    M = Z.shape[0]
    rhs = np.random.default_rng(8).standard_normal((70, M))
    op = KmmLambdaOperator(kernels.SquaredExponential(VAR, list(ls)), T(Z), T(lam), wide_anyd=True)
    sol, (steps, err) = conjugate_gradient(op, T(rhs), None, 1e-12, max_iterations=400, max_steps_cycle=401)
    want = np.linalg.solve(A, rhs.T).T
    d = float(np.abs(sol.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"kmm-wide-anyd converged solve: {int(steps)} steps, distance to numpy.linalg.solve {d:.2e} (bar 1e-06)")
    assert int(steps) < 400 and d < 1e-6


# ---------------------------------------------------------------- models
def model_data(D=33, N=400, M=96, seed=61):
    rng = np.random.default_rng([seed, D])
    ls = pr.lengthscales(D) * np.sqrt(D / 2.0)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ (rng.standard_normal(D) / np.sqrt(D)))[:, None] + 0.1 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)] + 0.01 * rng.standard_normal((M, D))
    u = rng.standard_normal((M, 1))
    counts = rng.integers(5, 15, size=(M, 1)).astype(F64)
    return X, Y, Z, rng.standard_normal((40, D)), ls, u, counts


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_cggp_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, Z, Xs, ls, u, counts = model_data()
    make = lambda **kw: models.CGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z),
                                    ConjugateGradient(1e-12, max_iterations=2000), num_probes=5, pseudo_u=T(u),
                                    cluster_counts=T(counts), num_data=400, **kw)
    on, off = make(matrix_free=True, wide_anyd=True), make(matrix_free=True)
    assert on._system()[1].kind_for(40) == 8 and off._system()[1].kind_for(40) == 2
    (m1, v1), (m0, v0) = on.predict_f(T(Xs)), off.predict_f(T(Xs))  # W = CG(K_mm + Lambda, K_mn): 40 columns
    print(f"kmm-wide-anyd CGGP.predict_f: mean {relerr(m1, m0):.2e}, variance {relerr(v1, v0):.2e} (bar 1e-06)")
    assert relerr(m1, m0) < 1e-6 and relerr(v1, v0) < 1e-6
    with pytest.raises(ValueError):
        make(wide_anyd=True)  # without matrix_free there is no operator to widen
    with pytest.raises(ValueError):
        make(matrix_free=True, wide_anyd="on")
    assert models.cdgp_class(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z), matrix_free=True, wide_anyd="auto",
                             pseudo_u=T(u), cluster_counts=T(counts), num_data=400).wide_anyd == "auto"


def test_trainable_cggp():
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, Z, _, ls, u, counts = model_data()
    probes = T(np.random.default_rng(91).choice([-1.0, 1.0], size=(Z.shape[0], 5)))
    data = (T(X[:40]), T(Y[:40]))
    make = lambda w: training.TrainableCGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z),
                                            ConjugateGradient(1e-12, max_iterations=2000), num_probes=5, pseudo_u=T(u),
                                            cluster_counts=T(counts), num_data=400, matrix_free=True, wide_anyd=w)

    def run(m):
        loss = m.training_loss(data, probes=probes)
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters()]).numpy()

    (l1, g1), (l0, g0) = run(make(True)), run(make(False))
    dl, dg = abs(l1 - l0) / abs(l0), np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))
    print(f"kmm-wide-anyd TrainableCGGP: loss {dl:.2e}, gradient {dg:.2e} (bar 1e-06)")
    assert np.all(np.isfinite(g1)) and dl <= 1e-6 and dg <= 1e-6
    assert make(True).frozen_model().wide_anyd is True and make("auto").frozen_model().wide_anyd == "auto"
    with pytest.raises(ValueError):
        training.TrainableCGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z), ConjugateGradient(1e-8),
                               pseudo_u=T(u), cluster_counts=T(counts), wide_anyd=True)  # no matrix_free
