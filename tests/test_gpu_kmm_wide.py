"""The many-column form of the matrix-free (K_mm + Lambda) operator, `MGP_OP_KMM_LAMBDA_WIDE` (csrc/project.hip under
csrc/cg.hip's `apply_operator`), at the smallest shapes at which each of its parts can go wrong.

Products against the long-double restatement of tests/kmm_wide_reference.py on the cases of its cut plan (bar: `bar(kind)`
of tests/test_gpu_gpr.py on `relmax`, the one the sweep form and `mgp_knm_project` meet); single kernel values through
one-hot right-hand sides under the derived bound of tests/pair_reference.py; agreement with the sweep form
(`MGP_OP_KMM_LAMBDA`) inside twice the bar, and its very bits where the kind falls back to it (fp32, D = 33); two calls
with the same bits; the buffer contract; the kind under `mgp_pcg_solve` and `mgp_pcg_solve_record` on the K_mm + Lambda
case of tests/guard_plan.py; `wide_solves` on `CGGP` and `TrainableCGGP`, and which form `"auto"` picks.

Without the feature every kind-4 call is MGP_E_BADARG ("unknown operator kind 4") and `KmmLambdaOperator(..., wide=)`
a TypeError: every test of this file fails on the parent."""

import ctypes

import numpy as np
import pytest
import torch

import guard_plan as gp
import kmm_wide_reference as kr
import pair_reference as pr
import switch_forms
from buffer_contract import Guarded
from cggp import _hip, ops
from test_gpu_cdgp_matrix_free import loss_and_grads, probes_of, problem, rel, tight_cg, trainable
from test_gpu_gpr import bar, relmax

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VAR = kr.VARIANCE
KIND_SWEEP, KIND_WIDE = 2, 4
MGP_E_NOMEM = -6  # include/mgp.h
F64 = np.float64


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def fresh_handle(pool=0):
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
    return lib, h


@pytest.fixture(scope="module")
def handle():
    lib, h = fresh_handle()
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


def prj_bytes(hd):
    lib, h = hd
    return int(lib.mgp_arena_bytes(h, b"prj"))


def operator(op_kind, spec, Z, lam):
    """(MgpOperator, keepalive) on device tensors or raw addresses (guard-banded buffers)."""
    addr = lambda t: t if isinstance(t, int) else t.data_ptr()
    k = spec.struct(_hip.F64 if isinstance(Z, int) else _hip.dtype_code(Z))
    st = _hip.MgpOperator()
    st.kind, st.dtype = op_kind, k.dtype
    st.kernel = ctypes.pointer(k)
    st.Z, st.lam = addr(Z), addr(lam)
    return st, k


def apply_rc(hd, op_kind, spec, Z, lam, P, out, M, Bt, stream=None):
    lib, h = hd
    stream = torch.cuda.current_stream(DEV) if stream is None else stream
    lib.mgp_set_stream(h, ctypes.c_void_p(stream.cuda_stream))
    st, keep = operator(op_kind, spec, Z, lam)
    st.n = st.M = M
    addr = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    rc = lib.mgp_operator_apply(h, ctypes.byref(st), addr(P), Bt, addr(out))
    del keep
    return rc


def apply(hd, op_kind, spec, Z, lam, P):
    out = torch.empty_like(P)
    rc = apply_rc(hd, op_kind, spec, Z, lam, P, out, Z.shape[0], P.shape[0])
    assert rc == 0, (rc, hd[0].mgp_last_error(hd[1]))
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    iv = torch.int64 if a.element_size() == 8 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def right_hand_sides(Bt, M, seed=0):
    return np.random.default_rng([seed, Bt, M]).standard_normal((Bt, M))


# ---------------------------------------------------------------- products, agreement, determinism
@pytest.mark.parametrize("kind,D,M,cols", kr.product_cases(), ids=lambda v: str(v) if not isinstance(v, tuple) else "c")
def test_products_against_long_double(handle, kind, D, M, cols):
    """Every right-hand side named by `probed_columns` against long double under bar(kind); the whole batch against the
    sweep form under twice that bar; a second call with the same bits."""
    Z, ls, lam = kr.inputs(M, D)
    K = kr.kmm_matrix(kind, VAR, ls, Z)
    spec = ops.KernelSpec(kind, VAR, list(ls), D)
    Zt, lt = T(Z), T(lam)
    worst, worst_pair = 0.0, 0.0
    for Bt in cols:
        P = right_hand_sides(Bt, M)
        Pt = T(P)
        got = apply(handle, KIND_WIDE, spec, Zt, lt, Pt)
        assert bool(torch.isfinite(got).all())
        probed = kr.probed_columns(M, Bt)
        dist = relmax(got[probed], kr.product(K, lam, P, probed))
        sweep = apply(handle, KIND_SWEEP, spec, Zt, lt, Pt)
        pair = relmax(got, sweep.cpu().numpy())
        print(f"kmm-wide {kind} D={D} M={M} columns={Bt}: long double {dist:.2e} (bar {bar(kind):.0e}, ratio "
              f"{dist / bar(kind):.3f}), sweep form {pair:.2e} (bar {2 * bar(kind):.0e})")
        worst, worst_pair = max(worst, dist / bar(kind)), max(worst_pair, pair / (2 * bar(kind)))
        assert dist < bar(kind), (kind, D, M, Bt, dist)
        assert pair < 2 * bar(kind), (kind, D, M, Bt, pair)
        assert same_bits(got, apply(handle, KIND_WIDE, spec, Zt, lt, Pt)), (kind, D, M, Bt)
    print(f"kmm-wide {kind} D={D} M={M}: worst ratio to the bar {worst:.3f} (long double), {worst_pair:.3f} (sweep form)")


@pytest.mark.parametrize("kind", ["se", "matern32"])
@pytest.mark.parametrize("dtype,D", [(torch.float32, 5), (torch.float64, 33)], ids=["fp32", "D33"])
def test_fallbacks_give_the_sweep_forms_bits(kind, dtype, D):
    """fp32 and D > 32 take the code of MGP_OP_KMM_LAMBDA: the same bits, and the route's arena is never reserved."""
    hd = fresh_handle()
    try:
        M = 300
        Z, ls, lam = kr.inputs(M, D)
        spec = ops.KernelSpec(kind, VAR, list(ls), D)
        for Bt in (1, 70, 257):
            Pt = T(right_hand_sides(Bt, M), dtype)
            wide = apply(hd, KIND_WIDE, spec, T(Z, dtype), T(lam, dtype), Pt)
            sweep = apply(hd, KIND_SWEEP, spec, T(Z, dtype), T(lam, dtype), Pt)
            assert same_bits(wide, sweep), (kind, D, Bt)
        assert prj_bytes(hd) == 0
    finally:
        hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- single kernel values
def _one_hot_values(hd, name, D, S, cols, width):
    """k(S, S[cols]) [n, len(cols)] from a product with `width` right-hand sides, the one-hot ones spread over them
    (the others zero), lambda = 0 (0 * 1 added by an fma: exact)."""
    n = S.shape[0]
    where = np.linspace(0, width - 1, len(cols)).astype(np.int64)
    P = np.zeros((width, n))
    P[where, cols] = 1.0
    spec = ops.KernelSpec(name, VAR, list(pr.lengthscales(D)), D)
    out = apply(hd, KIND_WIDE, spec, T(S), T(np.zeros(n)), T(P))
    return out[torch.from_numpy(where).to(DEV)].t().cpu().numpy()


@pytest.mark.parametrize("name", pr.KINDS)
def test_single_kernel_values(handle, name):
    """The method of tests/test_gpu_pair_accuracy.py: one-hot right-hand sides return single kernel values, held by
    `pair_reference.check_pairs` to the derived bound of the expansion-form routes (`pair_bound`), on the range set
    (every table entry of the exponential) and the edge set (the largest norms, the flush floor), 8 and 257 columns."""
    for D in (1, 3, 8, 17, 32):
        ls = pr.lengthscales(D)
        X, _, _, near = pr.range_set(name, D, 1 << 13)
        n = X.shape[0]
        sets = [("range", X, [0, near // 2, near - 1, n - 1, n - 2, n // 4, n // 4 + 1, (3 * n) // 7])]
        Xe, Ze, _, far = pr.edge_set(name, D, 4200, 300)
        far = [300 + f for f in far]
        sets.append(("edge", np.concatenate([Ze, Xe]), [0, 1, 299, far[-1], far[-20], far[-40], far[0], far[7]]))
        worst = 0.0
        for label, S, cols in sets:
            pv = pr.pair_values(name, VAR, ls, S, S, cols)
            a = pr.scaled(name, ls, S)
            bound = pr.pair_bound(name, VAR, pv.s, pv.q, a, a[cols], D, F64)
            for width in (8, 257):
                got = _one_hot_values(handle, name, D, S, cols, width)
                worst = max(worst, pr.check_pairs(f"kmm-wide {name} D={D} {label} columns={width}", got, pv, bound, VAR,
                                                  F64, col_ids=cols))
        print(f"pair-accuracy kmm-wide {name} D={D}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------- buffer contract
CONTRACT = dict(kind="matern32", D=3, M=1040, Bt=70)  # two splits, a ragged 16-column tile, 9 row tiles of 128


def _contract_inputs():
    c = CONTRACT
    Z, ls, lam = kr.inputs(c["M"], c["D"])
    return ops.KernelSpec(c["kind"], VAR, list(ls), c["D"]), Z, lam, right_hand_sides(c["Bt"], c["M"], seed=5)


def _guarded_call(hd, spec, vals, offsets, stream=None, staged=None):
    """kind 4 on guard-banded buffers; offsets: name -> 0 | 1 element off a 16-byte boundary.  Returns the Guarded
    buffers; with `staged` the inputs are copied in on `stream` just before the call."""
    M, Bt = CONTRACT["M"], CONTRACT["Bt"]
    g = {k: Guarded(v.shape, torch.float64, offsets.get(k, 0), DEV) for k, v in vals.items()}
    g["out"] = Guarded((Bt, M), torch.float64, offsets.get("out", 0), DEV)
    for k, v in vals.items():
        if staged is None:
            g[k].upload(torch.from_numpy(v))
        else:
            g[k].expect(staged[k])
            g[k].payload.copy_(staged[k], non_blocking=True)
    if staged is None:
        torch.cuda.synchronize()
    rc = apply_rc(hd, KIND_WIDE, spec, g["Z"].ptr, g["lam"].ptr, g["P"].ptr, g["out"].ptr, M, Bt, stream)
    assert rc == 0, (rc, hd[0].mgp_last_error(hd[1]))
    return g


def _check_contract(g):
    g["out"].check_output(None, name="kmm-wide out")
    for k in ("Z", "lam", "P"):
        g[k].check_input(name=f"kmm-wide {k}")


def test_buffer_contract_guards_alignment_and_arena():
    spec, Z, lam, P = _contract_inputs()
    vals = dict(Z=Z, lam=lam, P=P)
    M, D, Bt = CONTRACT["M"], CONTRACT["D"], CONTRACT["Bt"]
    hd = fresh_handle()
    try:
        assert prj_bytes(hd) == 0
        sweep = apply(hd, KIND_SWEEP, spec, T(Z), T(lam), T(P))
        assert prj_bytes(hd) == 0  # the sweep form never reaches the arena ...
        aligned = _guarded_call(hd, spec, vals, {})
        torch.cuda.synchronize()
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        held = prj_bytes(hd)
        print(f"prj arena after kind 4: {held} bytes (plan: {kr.arena_bytes(M, D, Bt, cus)})")
        assert held >= kr.arena_bytes(M, D, Bt, cus) > 0  # ... and the many-column form does: this route ran
        _check_contract(aligned)
        ref = aligned["out"].payload.clone()
        assert relmax(ref, sweep.cpu().numpy()) < 2 * bar(CONTRACT["kind"])
        for offsets in ({"P": 1, "out": 1}, {"P": 1}, {"out": 1}, {"Z": 1, "lam": 1, "P": 1, "out": 1}):
            off = _guarded_call(hd, spec, vals, offsets)
            torch.cuda.synchronize()
            _check_contract(off)
            assert same_bits(off["out"].payload, ref), offsets
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


def test_stale_arena_does_not_reach_the_result(handle):
    """A larger mgp_knm_project call on NaN inputs leaves the arena full of NaN tiles and a NaN pack; the many-column
    product that follows reuses that arena (it does not grow) and gives the bits of a clean handle."""
    spec, Z, lam, P = _contract_inputs()
    M, D, Bt = CONTRACT["M"], CONTRACT["D"], CONTRACT["Bt"]
    clean = apply(handle, KIND_WIDE, spec, T(Z), T(lam), T(P))
    hd = fresh_handle()
    try:
        lib, h = hd
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        B, N, r = 4096, 2048, 128
        Xs, X, R = nan(B, D), nan(N, D), nan(N, r)
        proj = torch.empty((B, r), dtype=torch.float64, device=DEV)
        k = spec.struct(_hip.F64)
        lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert lib.mgp_knm_project(h, ctypes.byref(k), _hip.ptr(Xs), B, _hip.ptr(X), N, _hip.ptr(R), r, ops.COLS,
                                   _hip.ptr(proj), None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(proj).all())
        before = prj_bytes(hd)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert before >= kr.arena_bytes(M, D, Bt, cus)
        got = apply(hd, KIND_WIDE, spec, T(Z), T(lam), T(P))
        assert prj_bytes(hd) == before
        assert same_bits(got, clean)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


def test_call_enqueued_behind_an_unfinished_producer(handle):
    """Inputs copied and the product enqueued on a side stream behind ~20 large matmuls; one synchronisation at the end."""
    spec, Z, lam, P = _contract_inputs()
    vals = dict(Z=Z, lam=lam, P=P)
    clean = apply(handle, KIND_WIDE, spec, T(Z), T(lam), T(P))
    staged = {k: torch.from_numpy(v).to(DEV) for k, v in vals.items()}
    a = (torch.randn((4096, 4096), generator=torch.Generator().manual_seed(0)) / 64.0).to(DEV)
    b = torch.empty_like(a)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = a
        for _ in range(10):
            torch.matmul(x, a, out=b)
            x = torch.matmul(b, a)
        e1.record()
        g = _guarded_call(handle, spec, vals, {"P": 1, "out": 1}, stream=side, staged=staged)
        got = g["out"].payload.clone()
    torch.cuda.synchronize()  # the one synchronisation
    print(f"the producers ran for {e0.elapsed_time(e1):.1f} ms")
    _check_contract(g)
    assert same_bits(got, clean)
    handle[0].mgp_set_stream(handle[1], ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def test_fixed_pool_too_small_is_nomem():
    spec, Z, lam, P = _contract_inputs()
    M, Bt = CONTRACT["M"], CONTRACT["Bt"]
    Zt, lt, Pt = T(Z), T(lam), T(P)
    out = torch.empty_like(Pt)
    grow = fresh_handle()
    try:
        ref = apply(grow, KIND_WIDE, spec, Zt, lt, Pt)
        fits = int(grow[0].mgp_workspace_bytes(grow[1]))
    finally:
        grow[0].mgp_destroy(grow[1])
    for pool, want in ((1 << 16, MGP_E_NOMEM), (fits + (1 << 20), 0)):
        hd = fresh_handle(pool)
        try:
            rc = apply_rc(hd, KIND_WIDE, spec, Zt, lt, Pt, out, M, Bt)
            torch.cuda.synchronize()
            assert rc == want, (pool, rc, hd[0].mgp_last_error(hd[1]))
            if want:
                assert b"fixed workspace exhausted" in hd[0].mgp_last_error(hd[1])
            else:
                assert same_bits(out, ref)
        finally:
            torch.cuda.synchronize()
            hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- under CG
KMM_CASES = [c for c in gp.CASES if c.family == "matfree" and c.system == "kmm"]
STOP_STEP, STOP_CAP = 6, 50  # the case has no stopping run of its own (thr None): see `_stop_threshold`


def _stop_threshold(case):
    """A threshold the case's batch crosses at step STOP_STEP exactly: the geometric mean of the largest 0.5 |r|^2 over
    the columns before that step and the smallest such maximum before any earlier step, from the host recurrence of
    tests/guard_plan.py (for this case 10.9 and 28: a factor 1.6 either way, against distances of 1e-15).  Six steps:
    the length at which the 1e-9 column bar of the fixed-step runs is meant."""
    trace = gp.run(case, STOP_STEP + 1)[3]
    worst = [float(np.max(t[2])) for t in trace]
    lo, hi = worst[STOP_STEP], min(worst[:STOP_STEP])
    assert 1.5 * 1.5 * lo < hi, (lo, hi)
    return float(np.sqrt(lo * hi))


def _cg_operators(case):
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator
    kern = kernels.SquaredExponential(1.0, [1.0, 1.0, 1.0])
    X, lam = T(gp.points(case.n)), T(gp.lam(case.n))
    return {w: KmmLambdaOperator(kern, X, lam, wide=w) for w in (False, True)}


def _widened(case, copies):
    """The case's right-hand sides `copies` times, copy q scaled by 2^-q: columns that freeze at different steps in
    every 16-column tile of a batch wide enough for the 64-row-tile instantiation."""
    b = gp.rhs(case)
    return np.concatenate([b * 2.0 ** -q for q in range(copies)])


def _fixed(op, rhs, k, min_float):
    from cggp.conjugate_gradient import conjugate_gradient
    sol, (steps, err) = conjugate_gradient(op, rhs, None, 0.0, None, max_iterations=k, max_steps_cycle=k + 1,
                                           min_float=min_float)
    torch.cuda.synchronize()
    return sol.clone(), err.clone(), int(steps)


def _stopping(op, rhs, thr, cap, check_every, min_float):
    from cggp.conjugate_gradient import ConjugateGradient
    cg = ConjugateGradient(thr, None, max_iterations=cap, min_float=min_float, check_every=check_every)
    sol, (steps, err) = cg.solve_with_stats(op, rhs.t().contiguous())
    torch.cuda.synchronize()
    return sol.t().contiguous(), err.clone(), int(steps)


def _column_distance(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    top = np.max(np.abs(b), axis=1)
    d = np.max(np.abs(a - b), axis=1) / np.where(top > 0, top, 1.0)
    assert not np.any(a[top == 0]), "a column the sweep form leaves at zero is not exactly zero"
    return float(d.max())


@pytest.mark.parametrize("copies", [1, 43], ids=["as-is", "129-columns"])
@pytest.mark.parametrize("case", KMM_CASES, ids=repr)
def test_solves_match_the_sweep_form(case, copies):
    """mgp_pcg_solve with kind 4 against kind 2: k fixed steps and the stopping run at check_every 1, 3 and 16 take the
    same steps and stay inside the 1e-9 column bar of tests/test_gpu_cg_guards.py; a frozen column keeps its bits
    across step counts; a cap one larger than the steps taken changes nothing (no write behind a closed gate)."""
    ops_ = _cg_operators(case)
    rhs = T(_widened(case, copies))
    frozen = [j for j, reg in enumerate(gp.regimes(case)) if reg["frozen_from"] == 0]
    assert frozen, "the case has columns frozen from step 0"
    frozen = [j + 3 * q for q in range(copies) for j in frozen] if copies > 1 else frozen
    runs = {}
    for k in case.ks:
        wide, sweep = _fixed(ops_[True], rhs, k, case.min_float), _fixed(ops_[False], rhs, k, case.min_float)
        assert wide[2] == sweep[2] == k
        d = _column_distance(wide[0], sweep[0])
        print(f"{case.id} x{copies} k={k}: column distance to the sweep form {d:.2e} (bar 1e-09)")
        assert d < 1e-9
        again = _fixed(ops_[True], rhs, k, case.min_float)
        assert same_bits(wide[0], again[0]) and same_bits(wide[1], again[1])
        runs[k] = wide
    ks = sorted(runs)
    for k in ks[1:]:
        assert same_bits(runs[ks[0]][0][frozen], runs[k][0][frozen]) and same_bits(runs[ks[0]][1][frozen], runs[k][1][frozen])
    first, thr = None, _stop_threshold(case)
    for check_every in (1, 3, 16):
        wide = _stopping(ops_[True], rhs, thr, STOP_CAP, check_every, case.min_float)
        sweep = _stopping(ops_[False], rhs, thr, STOP_CAP, check_every, case.min_float)
        print(f"{case.id} x{copies} thr={thr:g} check_every={check_every}: {wide[2]} steps (sweep form {sweep[2]})")
        assert wide[2] == sweep[2] == STOP_STEP
        assert _column_distance(wide[0], sweep[0]) < 1e-9
        if first is None:
            first = wide
        assert same_bits(wide[0], first[0]) and same_bits(wide[1], first[1])
    # the gate closed at first[2] steps with the other 10 steps of the batch of 16 queued behind it: a cap at that step
    # and one step past it, the same bits in every column
    for cap in (first[2], first[2] + 1):
        capped = _stopping(ops_[True], rhs, thr, cap, 16, case.min_float)
        assert capped[2] == first[2] and same_bits(capped[0], first[0]) and same_bits(capped[1], first[1])


@pytest.mark.parametrize("case", KMM_CASES, ids=repr)
def test_recording_solve_matches_the_sweep_form(case):
    ops_ = _cg_operators(case)
    rhs = T(_widened(case, 22))  # 66 columns
    k = max(case.ks)
    out = {w: ops.pcg_solve_record(ops_[w], rhs, 0.0, k, min_float=case.min_float) for w in (False, True)}
    torch.cuda.synchronize()
    (s_sol, s_err, s_st, s_coef), (w_sol, w_err, w_st, w_coef) = out[False], out[True]
    assert w_st.iterations == s_st.iterations == k and w_coef.shape == s_coef.shape == (k, rhs.shape[0], 3)
    assert _column_distance(w_sol, s_sol) < 1e-9
    live = s_coef[..., :2].abs() > 0
    assert torch.equal(live, w_coef[..., :2].abs() > 0)  # the same guards hold on the same steps
    dist = float(((w_coef[..., :2] - s_coef[..., :2]).abs()[live] / s_coef[..., :2].abs()[live]).max())
    print(f"{case.id} record k={k}: largest distance of a live (gamma, beta) {dist:.2e} (bar 1e-09)")
    assert dist < 1e-9
    again = ops.pcg_solve_record(ops_[True], rhs, 0.0, k, min_float=case.min_float)
    assert same_bits(again[0], w_sol) and same_bits(again[3], w_coef)


# ---------------------------------------------------------------- models
@pytest.mark.parametrize("kind,D", [("se", 3), ("matern32", 32)])
def test_model_with_wide_solves_matches_the_sweep_form(kind, D):
    """CGGP(matrix_free=True, wide_solves=True) against wide_solves=False inside the bars
    tests/test_gpu_cdgp_matrix_free.py holds its matrix-free model to against the dense one."""
    from cggp.models import CGGP, cdgp_class
    M, N, s2 = 300, 1500, 0.4
    X, y, Z, kern, u, counts = problem(kind, D, M, N)
    make = lambda w: CGGP(kern, s2, Z, tight_cg(M), num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=N,
                          matrix_free=True, wide_solves=w)
    sweep, wide = make(False), make(True)
    assert wide.wide_solves is True and sweep.wide_solves is False
    assert cdgp_class(kern, s2, Z, matrix_free=True, wide_solves="auto", pseudo_u=u, cluster_counts=counts,
                      num_data=N).wide_solves == "auto"
    for P in (5, 70):
        pr_ = probes_of(M, P, P)
        a, b = wide.prior_kl(pr_), sweep.prior_kl(pr_)
        print(f"{kind} D={D}: prior_kl P={P} {rel(a, b):.2e} (bar 1e-9)")
        assert rel(a, b) <= 1e-9
    for rows in (70, 257):
        xs = X[100:100 + rows]
        mu_s, var_s = sweep.predict_f(xs)
        mu_w, var_w = wide.predict_f(xs)
        dm, dv = float((mu_w - mu_s).abs().max()), float((var_w - var_s).abs().max())
        print(f"{kind} D={D}: predict_f rows={rows} mean {dm:.2e} variance {dv:.2e} (bar 1e-8)")
        assert mu_w.shape == (rows, 1) and var_w.shape == (rows, 1) and dm <= 1e-8 and dv <= 1e-8
        _, cov_w = wide.predict_f(xs, full_cov=True)
        _, cov_s = sweep.predict_f(xs, full_cov=True)
        assert cov_w.shape == (1, rows, rows) and float((cov_w - cov_s).abs().max()) <= 1e-8
    xs = X[:327]
    mu_b, var_b = wide.predict_f_batched(xs, 257)  # batches of 257 and 70 rows
    mu_s, var_s = sweep.predict_f_batched(xs, 257)
    assert float((mu_b - mu_s).abs().max()) <= 1e-8 and float((var_b - var_s).abs().max()) <= 1e-8
    pr_ = probes_of(M, 5, 7)
    for rows in (70, 257):
        data = (X[:rows], y[:rows])
        e_w, e_s = wide.elbo(data, probes=pr_), sweep.elbo(data, probes=pr_)
        print(f"{kind} D={D}: elbo rows={rows} {rel(e_w, e_s):.2e} (bar 1e-8)")
        assert rel(e_w, e_s) <= 1e-8


@pytest.mark.parametrize("kind,D", [("se", 3), ("matern32", 32)])
def test_training_with_wide_solves_matches_the_sweep_form(kind, D):
    M = 300
    pr_ = probes_of(M, 5, 11)
    for B in (70, 257):
        out = {}
        for w in (False, True):
            m, data = trainable(kind, D, M, B, True, wide_solves=w)
            out[w] = loss_and_grads(m, data, pr_)
            assert m.frozen_model().wide_solves is w
        (l_s, g_s), (l_w, g_w) = out[False], out[True]
        dist = np.max(np.abs(g_w - g_s)) / np.max(np.abs(g_s))
        print(f"{kind} D={D} batch={B}: loss {rel(l_w, l_s):.2e} (bar 1e-8), gradient {dist:.2e} (bar 1e-7)")
        assert g_w.shape == (D + 2,) and np.all(np.isfinite(g_w))
        assert rel(l_w, l_s) <= 1e-8 and dist <= 1e-7


def test_auto_picks_the_form_by_width_and_size(monkeypatch):
    """`wide="auto"` through the arena: nothing reserved below either threshold, reserved at both."""
    from cggp import conjugate_gradient as cg
    from cggp import kernels
    C, Mmin, D = cg.WIDE_MIN_COLUMNS, cg.WIDE_MIN_M, 3
    kern = kernels.SquaredExponential(1.0, [1.5] * D)
    rng = np.random.default_rng(0)
    Z = T(rng.standard_normal((Mmin, D)))
    lam = T(0.5 + rng.random(Mmin))
    with switch_forms.switched(monkeypatch, {}) as hd:
        held = lambda: int(hd.lib.mgp_arena_bytes(hd.h, b"prj"))
        below_m = cg.KmmLambdaOperator(kern, Z[:Mmin - 1].contiguous(), lam[:Mmin - 1].contiguous(), wide="auto")
        at_m = cg.KmmLambdaOperator(kern, Z, lam, wide="auto")
        assert below_m.kind_for(4 * C) == _hip.OP_KMM_LAMBDA and at_m.kind_for(C - 1) == _hip.OP_KMM_LAMBDA
        assert at_m.kind_for(C) == _hip.OP_KMM_LAMBDA_WIDE
        P = T(rng.standard_normal((C, Mmin)))
        below_m.rmatmul(P[:, :Mmin - 1].contiguous())
        narrow = at_m.rmatmul(P[:C - 1].contiguous())
        torch.cuda.synchronize()
        assert held() == 0
        full = at_m.rmatmul(P)
        torch.cuda.synchronize()
        assert held() > 0
        assert relmax(full[:C - 1], narrow.cpu().numpy()) < 2 * bar("se")
        sol, (steps, err) = cg.conjugate_gradient(at_m, P, None, 1e-6, max_iterations=3)
        assert int(steps) == 3 and bool(torch.isfinite(sol).all())
