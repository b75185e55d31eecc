"""The symmetric self-kernel operator above 32 dimensions, `MGP_OP_KXX_NOISE_SYM_ANYD` (csrc/kxx_sym_anyd.hip under
csrc/cg.hip's `apply_operator`), through the C ABI at the smallest shapes at which each of its parts can go wrong.

Every output is held to the bound include/mgp.h states -- sum_j |P[b, j]| pairbound(i, j) + u (terms + slots + 3)
sum_j |P[b, j] K[i, j]| + 2 u |s2 P[b, i]|, pairbound from tests/pair_reference.py, terms and slots from
tests/kxx_sym_anyd_plan.py, no fitted constant -- against long double: single kernel values through one-hot right-hand
sides on the point sets of tests/test_gpu_sweep_anyd.py (coincident rows, far pairs), with the rows of every block
probed so that both contractions of a tile are held separately; dense right-hand sides on both sides of the group seam.
Then reproducibility, the bits of the kind it falls back to, the buffer contract, the workspace, the kind under
`mgp_pcg_solve` and `mgp_pcg_solve_record`, and `sym_anyd` on `GPR` and `TrainableGPR`.

Without the feature kind 9 is MGP_E_BADARG ("unknown operator kind 9") and `sym_anyd=` a TypeError: every test of this
file fails on the parent."""

import ctypes

import numpy as np
import pytest
import torch

import kxx_sym_anyd_plan as sp
import pair_reference as pr
from buffer_contract import Guarded
from cggp import _hip, ops
from test_gpu_kmm_wide import T, fresh_handle, same_bits
from test_gpu_sweep_anyd import PerturbedMatrix, cg_points, k64, model_data, relerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VAR = pr.VARIANCE
LD = np.longdouble
F64 = np.float64
U = 2.0 ** -53
KIND_PLAIN, KIND_ANYD, KIND = 3, 7, sp.KIND
MGP_E_NOMEM = -6  # include/mgp.h
S2 = 0.5


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def handle():
    lib, h = fresh_handle()
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


def kxx_bytes(hd):
    return int(hd[0].mgp_arena_bytes(hd[1], b"kxx"))


def apply_rc(hd, op_kind, spec, X, s2, P, out, N, Bt, dtype=_hip.F64):
    """mgp_operator_apply on device tensors or raw addresses (guard-banded buffers)."""
    lib, h = hd
    lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    addr = lambda t: t if isinstance(t, int) else t.data_ptr()
    k = spec.struct(dtype)
    st = _hip.MgpOperator()
    st.kind, st.dtype = op_kind, k.dtype
    st.kernel = ctypes.pointer(k)
    st.X, st.N, st.n, st.s2 = addr(X), N, N, s2
    return lib.mgp_operator_apply(h, ctypes.byref(st), ctypes.c_void_p(addr(P)), Bt, ctypes.c_void_p(addr(out)))


def apply(hd, op_kind, spec, X, s2, P):
    out = torch.empty_like(P)
    rc = apply_rc(hd, op_kind, spec, X, s2, P, out, X.shape[0], P.shape[0],
                  _hip.F64 if X.dtype == torch.float64 else _hip.F32)
    assert rc == 0, (rc, hd[0].mgp_last_error(hd[1]))
    torch.cuda.synchronize()
    return out


def spec_of(name, ls, D):
    return ops.KernelSpec(name, VAR, list(ls), D)


# ---------------------------------------------------------------- single kernel values
_SETS = {}


def point_sets(name, D):
    """The shifted clouds (exact duplicates, |a|^2 ~ 170 - 200) and the edge set (the clamp, t through -1000 and the
    flush floor) of tests/test_gpu_sweep_anyd.py, as one pool of filler rows and the special rows of a probe: a
    coincident pair, the far point of the edge set and three of the rows opposite it."""
    if (name, D) not in _SETS:
        X, Z, ls = pr.shifted_set(name, D, 300, 63)
        eX, eZ, _, far = pr.edge_set(name, D, 2200, 300)
        i, j = np.argwhere((X[:, None, :] == Z[None, :, :]).all(-1))[0]
        special = np.stack([X[i], Z[j], eZ[0], eX[far[-1]], eX[far[-33]], eX[far[0]]])
        filler = np.concatenate([X, Z, eZ[1:], eX[:200]])
        _SETS[(name, D)] = (special, filler, ls)
    return _SETS[(name, D)]


def cloud(name, D, N):
    """(X [N, D], lengthscales, probed columns): filler rows with the special rows at 1 and N - 2 (coincident), N//2 + 1
    (the far point) and N//3 + 1, 5, N - 6 (far rows)."""
    special, filler, ls = point_sets(name, D)
    X = np.array(filler[np.arange(N) % filler.shape[0]])
    at = [1, N - 2, N // 2 + 1, N // 3 + 1, 5, N - 6]
    X[at] = special
    cols = sorted(set(sp.probed(N)) | set(at[:4]))
    assert len(cols) <= sp.COLS
    return X, ls, cols


def one_hot_check(hd, name, D, N, label):
    X, ls, cols = cloud(name, D, N)
    pv = pr.pair_values(name, VAR, ls, X, X[cols])
    a = pr.scaled(name, ls, X)
    rel = pr.pair_bound(name, VAR, pv.s, pv.q, a, a[cols], D, F64)
    P = np.zeros((len(cols), N))
    P[np.arange(len(cols)), cols] = 1.0
    got = apply(hd, KIND, spec_of(name, ls, D), T(X), S2, T(P)).cpu().numpy().T.copy()  # [N, C] = k(X, X[cols]) + s2 on the diagonal
    chain = sp.chain(N, len(cols), cus()) * U
    for r, j in enumerate(cols):  # P = e_j: variance + s2 on the diagonal, once; then handed on as its reference value
        want = pv.k[j, r] + LD(S2)
        assert abs(got[j, r] - want) <= (rel[j, r] + chain) * pv.k[j, r] + 2 * U * S2, (label, j, float(got[j, r]))
        got[j, r] = float(pv.k[j, r])
    nb = sp.ceil_div(N, sp.TB)
    paths = {sp.path(nb, bi, c // sp.TB) for bi in range(nb) for c in cols}
    assert paths == ({"diag"} if nb == 1 else {"diag", "kept", "streamed"}), (label, paths)
    return pr.check_pairs(label, got, pv, rel, VAR, F64, extra_rel=chain, col_ids=cols)


@pytest.mark.parametrize("D", sp.PAIR_DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_single_kernel_values(handle, name, D):
    """One-hot right-hand sides return single kernel values: every row of X against the probed columns -- both sides
    of every block seam, the coincident pair, the far point -- within the header's bound.  A probed column j in block
    B reaches the rows of block A through the kept-side contraction where A is the block its workgroup keeps and
    through the transposed tile where A is streamed; K[i, j] and K[j, i] of two probed columns come by different
    paths, and both are held."""
    worst = 0.0
    for N in sp.PAIR_SIZES:
        worst = max(worst, one_hot_check(handle, name, D, N, f"kxx-sym-anyd pairs {name} D={D} N={N}"))
    print(f"kxx-sym-anyd pairs {name} D={D}: worst err / bound {worst:.3f}")


def test_single_kernel_values_where_a_workgroup_chains_several_d(handle):
    """N large enough that a workgroup keeps its block over more than one d (DC > 1): the kept-side accumulator lives
    across block pairs and one slot per chunk is written."""
    N = sp.chained_size(cus())
    _, _, nd, dc, S = sp.plan(N, sp.COLS, cus())
    assert dc > 1 and S == nd
    worst = one_hot_check(handle, "matern32", 33, N, f"kxx-sym-anyd chained N={N}")
    print(f"kxx-sym-anyd pairs, DC = {dc} at N = {N}: worst err / bound {worst:.3f}")


def test_single_kernel_values_over_several_launches(handle):
    """N = 2^15 with 16 columns: the slots of all d exceed the 2^29-byte budget, so the d go in two launches and the
    finish kernel carries the running sum from one to the next."""
    N = 1 << 15
    _, _, nd, dc, S = sp.plan(N, sp.COLS, cus())
    assert S < nd and len(sp.launches(N, sp.COLS, cus())) >= 2
    worst = one_hot_check(handle, "se", 33, N, f"kxx-sym-anyd launches N={N}")
    print(f"kxx-sym-anyd pairs, {len(sp.launches(N, sp.COLS, cus()))} launches at N = {N}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------- dense right-hand sides
_DENSE = {}


def dense_reference(name, D=sp.DENSE_D, N=sp.DENSE_N):
    """(X, ls, K* [N, N] long double, pairbound [N, N] absolute): a standard normal cloud, the lengthscales stretched by
    sqrt(D) so that the sums are of kernel values of order 1/e."""
    if (name, D, N) not in _DENSE:
        X = np.random.default_rng([1, D, N]).standard_normal((N, D))
        ls = pr.lengthscales(D) * np.sqrt(D)
        pv = pr.pair_values(name, VAR, ls, X, X)
        a = pr.scaled(name, ls, X)
        rel = pr.pair_bound(name, VAR, pv.s, pv.q, a, a, D, F64)
        _DENSE[(name, D, N)] = (X, ls, pv.k, rel * pv.k)
    return _DENSE[(name, D, N)]


def product(K, s2, P):
    Pl = np.asarray(P, dtype=F64).astype(LD)
    return Pl @ K + LD(s2) * Pl


def product_bound(K, pairb, s2, P, N):
    """The header's bound for every element of out [Bt, N]."""
    Pa = np.abs(np.asarray(P, dtype=F64)).astype(LD)
    return Pa @ pairb.astype(LD) + U * sp.chain(N, P.shape[0], cus()) * (Pa @ np.abs(K)) + 2 * U * s2 * Pa


@pytest.mark.parametrize("Bt", sp.WIDTHS)
def test_dense_right_hand_sides(handle, Bt):
    """Random P against the long-double product, element by element inside the header's bound; a second call gives
    the same bits."""
    name = pr.KINDS[sp.WIDTHS.index(Bt) % 4]
    X, ls, K, pairb = dense_reference(name)
    N = X.shape[0]
    P = np.random.default_rng([3, Bt, N]).standard_normal((Bt, N))
    spec = spec_of(name, ls, sp.DENSE_D)
    Xt, Pt = T(X), T(P)
    got = apply(handle, KIND, spec, Xt, S2, Pt)
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g))
    ratio = float((np.abs(g.astype(LD) - product(K, S2, P)) / product_bound(K, pairb, S2, P, N)).max())
    print(f"kxx-sym-anyd dense {name} D={sp.DENSE_D} N={N} columns={Bt}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert same_bits(got, apply(handle, KIND, spec, Xt, S2, Pt))


# ---------------------------------------------------------------- reproducibility
CONTRACT = dict(name="matern32", D=62, N=391, Bt=21)  # nb = 4 (even), a ragged last block and tile, a ragged group


def _contract_inputs():
    c = CONTRACT
    X = np.random.default_rng([2, c["D"], c["N"]]).standard_normal((c["N"], c["D"]))
    ls = pr.lengthscales(c["D"]) * np.sqrt(c["D"])
    return spec_of(c["name"], ls, c["D"]), X, np.random.default_rng(6).standard_normal((c["Bt"], c["N"]))


def test_same_bits_from_a_fresh_handle_a_stale_arena_and_a_changed_x(handle):
    """Two calls, a fresh handle and a handle whose kxx arena a larger call filled with NaN all give the same bits; after
    X is changed in place the next call follows the new X (outside a solve every call packs for itself)."""
    spec, X, P = _contract_inputs()
    N, D, Bt = CONTRACT["N"], CONTRACT["D"], CONTRACT["Bt"]
    Xt, Pt = T(X), T(P)
    first = apply(handle, KIND, spec, Xt, S2, Pt)
    assert same_bits(first, apply(handle, KIND, spec, Xt, S2, Pt))
    hd = fresh_handle()
    try:
        assert same_bits(first, apply(hd, KIND, spec, Xt, S2, Pt))
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])
    hd = fresh_handle()
    try:
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        big = apply(hd, KIND, spec, nan(4 * N, D), S2, nan(32, 4 * N))
        assert bool(torch.isnan(big).all())
        before = kxx_bytes(hd)
        assert before >= sp.arena_bytes(4 * N, D, 32, cus()) > sp.arena_bytes(N, D, Bt, cus())
        got = apply(hd, KIND, spec, Xt, S2, Pt)
        assert kxx_bytes(hd) == before and same_bits(got, first)  # reused, not grown; nothing stale is read
        X2 = X[::-1].copy()
        want = apply(hd, KIND, spec, T(X2), S2, Pt)
        Xt2 = Xt.clone()
        assert same_bits(apply(hd, KIND, spec, Xt2, S2, Pt), first)
        Xt2.copy_(T(X2))  # in place: the same address, other points
        assert same_bits(apply(hd, KIND, spec, Xt2, S2, Pt), want) and not same_bits(want, first)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("D,dtype", [(8, torch.float64), (32, torch.float64), (40, torch.float32)],
                         ids=["D8", "D32", "fp32-D40"])
def test_fallback_bits(D, dtype):
    """fp64 at D <= 32 and fp32 run exactly the code of MGP_OP_KXX_NOISE: its bits."""
    hd = fresh_handle()
    try:
        N = 300
        X = np.random.default_rng([4, D]).standard_normal((N, D))
        spec = spec_of("matern32", pr.lengthscales(D) * np.sqrt(D), D)
        for Bt in (1, 5, 17):
            Pt = T(np.random.default_rng([5, Bt]).standard_normal((Bt, N)), dtype)
            a = apply(hd, KIND, spec, T(X, dtype), S2, Pt)
            b = apply(hd, KIND_PLAIN, spec, T(X, dtype), S2, Pt)
            assert same_bits(a, b), (D, Bt)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- buffer contract and workspace
def test_guard_bands_inputs_and_empty_inputs():
    """Guard bands around out untouched; P and X unchanged; buffers one element off a 16-byte boundary give the same
    bits; Bt = 0 writes nothing."""
    spec, X, P = _contract_inputs()
    N, Bt = CONTRACT["N"], CONTRACT["Bt"]
    vals = dict(X=X, P=P)
    hd = fresh_handle()
    try:
        ref = None
        for offsets in ({}, {"P": 1, "out": 1}, {"X": 1, "P": 1, "out": 1}):
            g = {k: Guarded(v.shape, torch.float64, offsets.get(k, 0), DEV) for k, v in vals.items()}
            g["out"] = Guarded((Bt, N), torch.float64, offsets.get("out", 0), DEV)
            for k, v in vals.items():
                g[k].upload(torch.from_numpy(v))
            torch.cuda.synchronize()
            rc = apply_rc(hd, KIND, spec, g["X"].ptr, S2, g["P"].ptr, g["out"].ptr, N, Bt)
            assert rc == 0, (rc, hd[0].mgp_last_error(hd[1]))
            torch.cuda.synchronize()
            g["out"].check_output(None, name="kxx-sym-anyd out")
            for k in vals:
                g[k].check_input(name=f"kxx-sym-anyd {k}")
            if ref is None:
                ref = g["out"].payload.clone()
                assert kxx_bytes(hd) >= sp.arena_bytes(N, CONTRACT["D"], Bt, cus())  # this route ran
            assert same_bits(g["out"].payload, ref), offsets
        out = torch.full((Bt, N), 7.0, dtype=torch.float64, device=DEV)
        assert apply_rc(hd, KIND, spec, T(X), S2, T(P), out, N, 0) == 0
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


def test_a_closed_gate_leaves_the_solution_untouched():
    """A stopping solve polled every 16 steps: the gate closes at the step the threshold is crossed with the rest of
    the batch of 16 queued behind it; a cap at that step and one past it give the same bits in every column."""
    from cggp import kernels
    from cggp.conjugate_gradient import ConjugateGradient, KxxNoiseOperator
    Xn, _, ls = cg_points(40, 260, 1, 41, 4, 1.5)
    op = KxxNoiseOperator(kernels.SquaredExponential(VAR, list(ls)), T(Xn), S2, sym_anyd=True)
    rhs = T(np.random.default_rng(43).standard_normal((260, 3)))

    def run(cap):
        cg = ConjugateGradient(1e-6, None, max_iterations=cap, check_every=16)
        sol, (steps, err) = cg.solve_with_stats(op, rhs)
        torch.cuda.synchronize()
        return sol.clone(), int(steps)

    first, steps = run(200)
    assert 1 < steps < 100 and steps % 16 != 0
    for cap in (steps, steps + 1):
        sol, s = run(cap)
        assert s == steps and same_bits(sol, first)


def test_fixed_pool_of_the_documented_bytes():
    """A fixed pool of exactly the header's formula serves the call and mgp_workspace_bytes reports it; one byte less
    is MGP_E_NOMEM."""
    spec, X, P = _contract_inputs()
    N, D, Bt = CONTRACT["N"], CONTRACT["D"], CONTRACT["Bt"]
    Xt, Pt = T(X), T(P)
    grow = fresh_handle()
    try:
        ref = apply(grow, KIND, spec, Xt, S2, Pt)
    finally:
        grow[0].mgp_destroy(grow[1])
    need = sp.arena_bytes(N, D, Bt, cus())
    for pool, want in ((need, 0), (need - 1, MGP_E_NOMEM)):
        hd = fresh_handle(pool)
        try:
            out = torch.empty_like(Pt)
            rc = apply_rc(hd, KIND, spec, Xt, S2, Pt, out, N, Bt)
            torch.cuda.synchronize()
            assert rc == want, (pool, rc, hd[0].mgp_last_error(hd[1]))
            if want:
                assert b"fixed workspace exhausted" in hd[0].mgp_last_error(hd[1])
            else:
                assert same_bits(out, ref) and int(hd[0].mgp_workspace_bytes(hd[1])) == need
        finally:
            torch.cuda.synchronize()
            hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- inside mgp_pcg_solve
@pytest.mark.parametrize("Bt", [1, 5])
def test_pcg_solve_fixed_steps_against_the_oracle(Bt):
    """mgp_pcg_solve on kind 9 after 3 and 5 steps against oracle/cg.py on the fp64 matrix at 1e-9, with the inputs and
    the conditioning check of the kind-7 test of tests/test_gpu_sweep_anyd.py (N = 260, D = 40)."""
    from cggp import kernels
    from cggp.conjugate_gradient import KxxNoiseOperator, conjugate_gradient
    from oracle import cg as ocg
    D, N = 40, 260
    Xn, _, ls = cg_points(D, N, 1, 41, 4, 1.5)
    kern = kernels.SquaredExponential(VAR, list(ls))
    a2 = (pr.scaled("se", ls, Xn) ** 2).sum(1).max()
    rel = np.log(2.0) * (D + 6) * U * 4 * a2 + 8 * U
    A = (k64("se", ls, Xn, Xn) + LD(S2) * np.eye(N, dtype=LD)).astype(F64)
    op = KxxNoiseOperator(kern, T(Xn), S2, sym_anyd=True)
    assert op.kind_for(Bt) == KIND == _hip.OP_KXX_NOISE_SYM_ANYD
    eps = rel + sp.chain(N, Bt, cus()) * U
    rhs = np.random.default_rng(42).standard_normal((Bt, N))
    exact = np.linalg.solve(A, rhs.T).T
    for k in (3, 5):
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((Bt, N)), 0.0, max_iterations=k,
                                                         max_steps_cycle=k + 1)
        assert np.linalg.norm(o_sol - exact) > 1e-4 * np.linalg.norm(exact)  # not converged: an iterate, not a limit
        for seed in range(3):
            p_sol, _ = ocg.conjugate_gradient(PerturbedMatrix(A, eps, seed), rhs, np.zeros((Bt, N)), 0.0,
                                              max_iterations=k, max_steps_cycle=k + 1)
            assert np.linalg.norm(p_sol - o_sol) < 1e-10 * np.linalg.norm(o_sol), (k, eps)
        sol, (steps, err) = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        rel_diff = np.linalg.norm(sol.cpu().numpy() - o_sol) / np.linalg.norm(o_sol)
        print(f"kxx-sym-anyd pcg columns={Bt} k={k}: eps {eps:.2e}, relative difference {rel_diff:.3e} (bar 1e-09)")
        assert int(steps) == k == o_steps and rel_diff < 1e-9
        again, _ = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        assert same_bits(again, sol)


def test_recording_solve_with_the_lowrank_preconditioner():
    """mgp_pcg_solve_record with MGP_PRE_LOWRANK on kind 9: the recorded coefficients of every step agree with those
    recorded on kind 7 at 1e-6."""
    from cggp import kernels
    from cggp.conjugate_gradient import KxxNoiseOperator, PivotedCholeskyPreconditioner
    X, Y, _, _, ls = model_data(N=400)
    kern = kernels.SquaredExponential(VAR, list(ls))
    rhs = T(np.random.default_rng(44).standard_normal((3, 400)))
    out = {}
    for key, kw in (("sym", dict(sym_anyd=True)), ("anyd", dict(fused_anyd=True))):
        op = KxxNoiseOperator(kern, T(X), 0.2, **kw)
        assert op.kind_for(3) == (KIND if key == "sym" else KIND_ANYD)
        out[key] = ops.pcg_solve_record(op, rhs, 0.0, 6, preconditioner=PivotedCholeskyPreconditioner(rank=20, rel_tol=0.0))
    torch.cuda.synchronize()
    (a_sol, _, a_st, a_coef), (b_sol, _, b_st, b_coef) = out["sym"], out["anyd"]
    assert a_st.iterations == b_st.iterations == 6 and a_coef.shape == b_coef.shape == (6, 3, 3)
    d = float(((a_coef - b_coef).abs() / b_coef.abs().clamp_min(1e-300)).max())
    print(f"kxx-sym-anyd record with MGP_PRE_LOWRANK: coefficients against kind 7 {d:.2e}, "
          f"solution {relerr(a_sol, b_sol):.2e} (bar 1e-06)")
    assert d < 1e-6 and relerr(a_sol, b_sol) < 1e-6


# ---------------------------------------------------------------- models
def test_gpr_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, _, Xs, ls = model_data(N=500)
    make = lambda **kw: models.GPR((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), noise_variance=0.2,
                                   conjugate_gradient=ConjugateGradient(1e-12, max_iterations=2000), solver="cg", **kw)
    on, off = make(sym_anyd=True), make()
    assert on.operator().kind_for(1) == KIND and off.operator().kind_for(1) == KIND_PLAIN
    assert make(sym_anyd=True, fused_anyd=True).operator().kind_for(3) == KIND  # asked first
    rhs = T(np.random.default_rng(81).standard_normal((500, 2)))
    assert relerr(on.solve(rhs), off.solve(rhs)) < 1e-6
    (m1, v1), (m0, v0) = on.predict_f(T(Xs)), off.predict_f(T(Xs))
    print(f"kxx-sym-anyd GPR.predict_f: mean {relerr(m1, m0):.2e}, variance {relerr(v1, v0):.2e} (bar 1e-06)")
    assert relerr(m1, m0) < 1e-6 and relerr(v1, v0) < 1e-6
    assert models.gpr_class((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), models.Gaussian(0.2),
                            sym_anyd=True).sym_anyd is True
    assert models.create_gpr_model((T(X), T(Y)), lambda dim: kernels.SquaredExponential(VAR, list(ls)),
                                   sym_anyd="auto").sym_anyd == "auto"
    with pytest.raises(ValueError):
        make(sym_anyd=None)


def test_trainable_gpr():
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, _, _, ls = model_data(N=400)
    gpr = lambda **kw: training.TrainableGPR(kernels.SquaredExponential(VAR, list(ls)), 0.2, T(X), T(Y), num_probes=4,
                                             conjugate_gradient=ConjugateGradient(1e-13, max_iterations=2000), **kw)

    def run(m):
        loss = m.training_loss()
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters()]).numpy()

    (l1, g1), (l0, g0) = run(gpr(sym_anyd=True)), run(gpr(fused_anyd=True))
    dl, dg = abs(l1 - l0) / abs(l0), np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))
    print(f"kxx-sym-anyd TrainableGPR: loss {dl:.2e}, gradient {dg:.2e} (bar 1e-06)")
    assert np.isfinite(l1) and np.all(np.isfinite(g1)) and dl <= 1e-6 and dg <= 1e-6
    assert gpr(sym_anyd=True).frozen_model().sym_anyd is True and gpr(sym_anyd="auto").frozen_model().sym_anyd == "auto"
    with pytest.raises(ValueError):
        gpr(sym_anyd="no")
