"""The pivoted-Cholesky preconditioner of matrix-free CDGP on the MI355X: the many-column application
`MGP_PRE_LOWRANK_WIDE` element by element through one CG step (against numpy, beside `MGP_PRE_LOWRANK`), inside the
device loop (fixed-step iterates against the numpy PCG, kinds 5 and 6 side by side, mixed lifetimes, the refresh path),
the iteration counts on the CDGP-shaped system of tests/cdgp_precond_reference.py, `CGGP` / `TrainableCGGP` with
`matrix_free=True` and the preconditioner against the same models without it, and the buffer contract of the route."""

import ctypes
import math

import numpy as np
import pytest
import torch

import cdgp_precond_reference as cr
import guard_plan as gp
from pivchol_reference import pcg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MGP_E_BADARG, MGP_E_NOMEM = -1, -6  # include/mgp.h
KIND_NARROW, KIND_WIDE = 5, 6


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def same_bits(a, b):
    iv = torch.int64 if a.element_size() == 8 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def fresh_handle(pool=0):
    from cggp import _hip
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
    return lib, h


def pch_bytes(hd):
    return int(hd[0].mgp_arena_bytes(hd[1], b"pch"))


class Hand:
    """A hand-made preconditioner (dinv [n], B [k, n]) in the protocol `_solve_device` asks for, of a given kind."""

    def __init__(self, dinv, B, kind):
        self.dinv, self.B, self.kind = dinv, B, kind

    def struct(self):
        from cggp import _hip
        st = _hip.MgpPrecond()
        st.kind = self.kind
        st.diag_inv = self.dinv.data_ptr()
        st.dense_inv = self.B.data_ptr()
        st.num_blocks = self.B.shape[0]
        return st

    def _native_for(self, op, Bt):
        return self.struct(), (self.dinv, self.B)


def raw_solve(hd, A, pre, rhs, steps, out=None):
    """mgp_pcg_solve on a handle of the test's own: dense A, threshold 0, `steps` steps.  Returns (rc, solution)."""
    from cggp import _hip
    lib, h = hd
    lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    st = _hip.MgpOperator()
    st.kind, st.dtype, st.n, st.A = _hip.OP_DENSE, _hip.dtype_code(A), A.shape[0], A.data_ptr()
    ps = pre.struct()
    sol = torch.empty_like(rhs) if out is None else out
    err = torch.empty((rhs.shape[0], 1), dtype=rhs.dtype, device=DEV)
    stats = _hip.MgpCgStats()
    rc = lib.mgp_pcg_solve(h, ctypes.byref(st), ctypes.byref(ps), _hip.ptr(rhs), None, rhs.shape[0], 0.0, steps,
                           steps + 1, 1e-16, 10, _hip.ptr(sol), _hip.ptr(err), ctypes.byref(stats))
    torch.cuda.synchronize()
    return rc, sol


def solve(op, rhs, pre, thr, cap, cycle=None, check_every=10, min_float=1e-16):
    from cggp.conjugate_gradient import _solve_device
    sol, st, err = _solve_device(op, rhs, None, thr, pre, cap, cap + 1 if cycle is None else cycle, min_float,
                                 check_every)
    torch.cuda.synchronize()
    return sol, st, err


def column_distance(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    top = np.max(np.abs(b), axis=1)
    assert not np.any(a[top == 0]), "a column that stays at zero on one form is not exactly zero on the other"
    return float((np.max(np.abs(a - b), axis=1) / np.where(top > 0, top, 1.0)).max())


# ---------------------------------------------------------------- 1. the wide kernels, element by element
def hand_made(Bt, k, n, seed):
    """dinv on [0.5, 1.5] and a B with |B|_2 <= 0.3, so that P^-1 = diag(dinv) - B^T B is positive definite; the
    low-rank part of z is ~1e-2 of the diagonal part, 1e10 times the bar."""
    rng = np.random.default_rng([seed, Bt, k, n])
    B = 0.3 * rng.standard_normal((k, n)) / (math.sqrt(n) + math.sqrt(k))
    return 0.5 + rng.random(n), B, rng.standard_normal((Bt, n)), rng


def one_step_reference(dinv, B, R, times_a):
    """x_1 = gamma z of one CG step from zero, z = P^-1 r and gamma = r.z / z.Az from the reference z, and the bar's
    scale |gamma| (|dinv o R| + |R| |B^T| |B|)."""
    z, scale = cr.apply_reference(dinv, B, R)
    gamma = (R * z).sum(axis=1) / (z * times_a(z)).sum(axis=1)
    return gamma[:, None] * z, np.abs(gamma)[:, None] * scale


# every Bt, k and n of the plan once: the 64- and 128-row tiles (48, 49), the group seam (255, 256, 257), two groups
# with a ragged second (300); k below the MFMA depth (1, 3), ragged (33, 130), whole tiles (128); n of one column, under
# one tile (63), several splits (1000) and a ragged last tile (4097)
DENSE_SHAPES = [(48, 1, 1), (49, 3, 63), (255, 33, 1000), (256, 128, 4097), (257, 130, 1000), (300, 128, 63)]


@pytest.mark.parametrize("Bt,k,n", DENSE_SHAPES)
def test_one_step_shows_every_entry_of_the_application(Bt, k, n):
    from cggp.conjugate_gradient import DenseOperator
    dinv, B, R, rng = hand_made(Bt, k, n, 1)
    u = rng.standard_normal(n) / math.sqrt(n)
    d = 1.0 + rng.random(n)
    A = np.diag(d) + np.outer(u, u)
    ref, scale = one_step_reference(dinv, B, R, lambda z: z @ A)
    op, rhs = DenseOperator(T(A)), T(R)
    got = {}
    for kind in (KIND_NARROW, KIND_WIDE):
        pre = Hand(T(dinv), T(B), kind)
        x, st, _ = solve(op, rhs, pre, 0.0, 1)
        assert st.iterations == 1
        err = float(np.max(np.abs(x.cpu().numpy() - ref) / scale))
        print(f"Bt={Bt} k={k} n={n} kind {kind}: {err:.3e} (bar 1e-12)")
        assert err <= 1e-12
        again, _, _ = solve(op, rhs, pre, 0.0, 1)
        assert same_bits(x, again)
        got[kind] = x
    assert column_distance(got[KIND_WIDE], got[KIND_NARROW]) <= 1e-12


def test_one_step_on_the_matrix_free_operator_at_70001():
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator
    Bt, k, n = 49, 33, 70001
    dinv, B, R, rng = hand_made(Bt, k, n, 2)
    Z, lam = T(rng.uniform(-3.0, 3.0, (n, 2))), T(0.1 / rng.integers(1, 65, n))
    op = KmmLambdaOperator(kernels.SquaredExponential(1.0, [1.5, 1.5]), Z, lam)
    ref, scale = one_step_reference(dinv, B, R, lambda z: op.rmatmul(T(z)).cpu().numpy())
    rhs = T(R)
    for kind in (KIND_NARROW, KIND_WIDE):
        pre = Hand(T(dinv), T(B), kind)
        x, st, _ = solve(op, rhs, pre, 0.0, 1)
        err = float(np.max(np.abs(x.cpu().numpy() - ref) / scale))
        print(f"Bt={Bt} k={k} n={n} kind {kind}: {err:.3e} (bar 1e-12)")
        assert st.iterations == 1 and err <= 1e-12
    again, _, _ = solve(op, rhs, pre, 0.0, 1)
    assert same_bits(x, again)


def test_fp32_under_the_wide_kind_gives_the_narrow_kinds_bits():
    from cggp.conjugate_gradient import DenseOperator
    Bt, k, n = 49, 3, 63
    dinv, B, R, rng = hand_made(Bt, k, n, 3)
    A = np.diag(1.0 + rng.random(n))
    f32 = torch.float32
    op, rhs = DenseOperator(T(A, f32)), T(R, f32)
    x = {kind: solve(op, rhs, Hand(T(dinv, f32), T(B, f32), kind), 0.0, 3)[0] for kind in (KIND_NARROW, KIND_WIDE)}
    assert bool(torch.isfinite(x[KIND_WIDE]).all()) and float(x[KIND_WIDE].abs().max()) > 0
    assert same_bits(x[KIND_WIDE], x[KIND_NARROW])


def test_the_recording_solve_refuses_the_wide_kind():
    from cggp import _hip
    hd = fresh_handle()
    try:
        lib, h = hd
        n = 64
        A, rhs = T(np.eye(n)), T(np.ones((2, n)))
        pre = Hand(T(np.ones(n)), T(np.zeros((1, n))), KIND_WIDE)
        st = _hip.MgpOperator()
        st.kind, st.dtype, st.n, st.A = _hip.OP_DENSE, _hip.F64, n, A.data_ptr()
        ps, stats = pre.struct(), _hip.MgpCgStats()
        sol, err = torch.empty_like(rhs), torch.empty((2, 1), dtype=torch.float64, device=DEV)
        coef = torch.zeros((4, 2, 3), dtype=torch.float64, device=DEV)
        rc = lib.mgp_pcg_solve_record(h, ctypes.byref(st), ctypes.byref(ps), _hip.ptr(rhs), None, 2, 0.0, 4, 5, 1e-16, 10,
                                      _hip.ptr(sol), _hip.ptr(err), ctypes.byref(stats), _hip.ptr(coef), 4)
        assert rc == MGP_E_BADARG
        ps.kind = KIND_NARROW
        rc = lib.mgp_pcg_solve_record(h, ctypes.byref(st), ctypes.byref(ps), _hip.ptr(rhs), None, 2, 0.0, 4, 5, 1e-16, 10,
                                      _hip.ptr(sol), _hip.ptr(err), ctypes.byref(stats), _hip.ptr(coef), 4)
        assert rc == 0
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


# ---------------------------------------------------------------- 2. inside the loop
LOOP_M = 2000


@pytest.fixture(scope="module")
def loop_system():
    """K_mm + Lambda at M = 2000 on the points of tests/guard_plan.py (SE, D = 3, lambda on [0.5, 1.5]): its explicit
    matrix, the two operators' preconditioners built by the device from one rank-24 factor, and their (dinv, B)."""
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator, PivotedCholeskyPreconditioner
    case = gp._case("precond-kmm-2000", "matfree", LOOP_M, 3, ks=(3, 6), thr=None, system="kmm")
    A = gp.operator_matrix(case)
    op = KmmLambdaOperator(kernels.SquaredExponential(1.0, [1.0, 1.0, 1.0]), T(gp.points(LOOP_M)), T(gp.lam(LOOP_M)))
    pres = {w: PivotedCholeskyPreconditioner(rank=24, rel_tol=0.0, wide=w) for w in (False, True)}
    for p in pres.values():
        p._prepare(op)
        assert p.rank_ == 24
    assert same_bits(pres[True].B, pres[False].B)
    return case, A, op, pres, pres[True].diag_inv.cpu().numpy(), pres[True].B.cpu().numpy()


def test_fixed_step_iterates_at_64_columns_against_numpy_pcg(loop_system):
    case, A, op, pres, dinv, B = loop_system
    rhs = T(np.random.default_rng(2).standard_normal((64, LOOP_M)))
    x = {w: solve(op, rhs, pres[w], 0.0, 5) for w in (False, True)}
    assert x[True][1].iterations == x[False][1].iterations == 5
    worst = 0.0
    for col in range(64):
        ref, it, coef = pcg(lambda v: A @ v, rhs[col].cpu().numpy(), dinv=dinv, B=B, threshold=0.0, max_iterations=5)
        assert it == 5
        e = np.max(np.abs(x[True][0][col].cpu().numpy() - ref)) / np.max(np.abs(ref))
        worst = max(worst, e)
        assert e <= 1e-9, (col, e)
        assert abs(float(x[True][2][col, 0]) - coef[-1, 2]) <= 1e-9 * coef[-1, 2]
    d = column_distance(x[True][0], x[False][0])
    print(f"64 columns, 5 steps: to the numpy PCG {worst:.3e} (bar 1e-9), kind 6 to kind 5 {d:.3e} (bar 1e-12)")
    assert d <= 1e-12


def mixed_batch(case):
    """The three columns of the case (c: under the floor from the start, a: generic, b: zero) 22 times, copy q scaled by
    2^-q, the first 64: columns that freeze at different steps in every tile."""
    b = gp.rhs(case)
    return np.concatenate([b * 2.0 ** -q for q in range(22)])[:64]


def test_kinds_5_and_6_take_the_same_steps_and_frozen_columns_keep_their_bits(loop_system):
    case, A, op, pres, dinv, B = loop_system
    b = mixed_batch(case)
    rhs = T(b)
    host = gp.LowRankPreconditioner(dinv, B)
    trace = gp.recurrence(A, b, np.zeros_like(b), 0.0, host, 10, 11, case.min_float)[3]
    frozen = [j for j in range(64) if all(t[0][j] <= case.min_float and t[1][j] <= case.min_float for t in trace)]
    live = [j for j in range(64) if all(t[0][j] > case.min_float for t in trace[:3])]
    assert len(frozen) >= 22 and len(live) >= 10, (len(frozen), len(live))  # the zero columns at least; mixed lifetimes
    # fixed steps: the same steps, 1e-12 apart; what is frozen from the start keeps its bits whatever the step count
    runs = {}
    for k in (3, 6):
        w, nrw = solve(op, rhs, pres[True], 0.0, k, min_float=case.min_float), solve(op, rhs, pres[False], 0.0, k, min_float=case.min_float)
        assert w[1].iterations == nrw[1].iterations == k
        d = column_distance(w[0], nrw[0])
        print(f"mixed lifetimes k={k}: kind 6 to kind 5 {d:.3e} (bar 1e-12)")
        assert d <= 1e-12
        runs[k] = w
    assert same_bits(runs[3][0][frozen], runs[6][0][frozen]) and same_bits(runs[3][2][frozen], runs[6][2][frozen])
    # a threshold the batch crosses at one step exactly (the construction of tests/test_gpu_kmm_wide.py): the first
    # step from the fourth on before which the host recurrence's largest 0.5 |r|^2 is a factor 1.5^2 under every
    # earlier one; the threshold is the geometric mean, a factor 1.5 from either, against distances of 1e-12
    worst = [float(np.max(t[2])) for t in trace]
    stop = next(s_ for s_ in range(4, len(worst)) if 1.5 * 1.5 * worst[s_] < min(worst[:s_]))
    thr = math.sqrt(worst[stop] * min(worst[:stop]))
    first = None
    for check_every in (1, 3, 16):
        w = solve(op, rhs, pres[True], thr, 50, check_every=check_every, min_float=case.min_float)
        nrw = solve(op, rhs, pres[False], thr, 50, check_every=check_every, min_float=case.min_float)
        print(f"thr={thr:g} check_every={check_every}: kind 6 {w[1].iterations} steps, kind 5 {nrw[1].iterations}")
        assert w[1].iterations == nrw[1].iterations == stop
        assert column_distance(w[0], nrw[0]) <= 1e-12
        first = w if first is None else first
        assert same_bits(w[0], first[0]) and same_bits(w[2], first[2])
    # the gate closed at that step with the rest of the batch of 16 queued behind it: a cap at that step and one past it
    # give the same bits in every column (no write behind a closed gate)
    for cap in (stop, stop + 1):
        capped = solve(op, rhs, pres[True], thr, cap, check_every=16, min_float=case.min_float)
        assert capped[1].iterations == stop and same_bits(capped[0], first[0]) and same_bits(capped[2], first[2])


def test_refresh_path_under_the_wide_kind(loop_system):
    case, A, op, pres, dinv, B = loop_system
    rhs = T(np.random.default_rng(5).standard_normal((64, LOOP_M)))
    w = solve(op, rhs, pres[True], 1e-14, 400, cycle=7)
    nrw = solve(op, rhs, pres[False], 1e-14, 400, cycle=7)
    assert w[1].converged and w[1].iterations > 7 and w[1].iterations == nrw[1].iterations
    # two correct CGs run to convergence over several refreshes: the project's column bar (tests/guard_plan.py BAR_F64)
    d = column_distance(w[0], nrw[0])
    print(f"refresh every 7th step, {w[1].iterations} steps: kind 6 to kind 5 {d:.3e} (bar 1e-9)")
    assert d <= 1e-9
    for col in (0, 31, 63):
        ref, it, _ = pcg(lambda v: A @ v, rhs[col].cpu().numpy(), dinv=dinv, B=B, threshold=1e-14, max_iterations=400,
                         max_steps_cycle=7)
        e = np.max(np.abs(w[0][col].cpu().numpy() - ref)) / np.max(np.abs(ref))
        print(f"column {col}: device {w[1].iterations} steps, numpy {it}, difference {e:.3e} (bar 1e-8)")
        assert e <= 1e-8


# ---------------------------------------------------------------- 3. it helps
def test_iteration_counts_on_the_cdgp_table_inputs():
    from cggp import kernels
    from cggp.conjugate_gradient import EyePreconditioner, KmmLambdaOperator, PivotedCholeskyPreconditioner
    M, thr = 2048, 1e-8
    Zn, lamn, bn = cr.cdgp_inputs(M, 2)
    A = cr.kernel_matrix("se", 1.0, [1.5, 1.5], Zn, dtype=np.float64) + np.diag(lamn)
    op = KmmLambdaOperator(kernels.SquaredExponential(1.0, [1.5, 1.5]), T(Zn), T(lamn))
    y = T(bn[None, :])
    res = lambda x: float(np.linalg.norm(A @ x[0].cpu().numpy() - bn))
    x_id, st_id, _ = solve(op, y, EyePreconditioner(), thr, M)
    assert st_id.converged
    for wide in (False, True):
        pre = PivotedCholeskyPreconditioner(rank=64, rel_tol=0.0, wide=wide)
        x_pc, st_pc, _ = solve(op, y, pre, thr, M)
        _, it_np, _ = pcg(lambda v: A @ v, bn, dinv=pre.diag_inv.cpu().numpy(), B=pre.B.cpu().numpy(), threshold=thr)
        print(f"wide={wide} rank {pre.rank_}: identity {st_id.iterations} steps (|r| {res(x_id):.3e}), preconditioned "
              f"{st_pc.iterations} (|r| {res(x_pc):.3e}), numpy PCG on the device's factor {it_np}")
        assert st_pc.converged and pre.rank_ == 64
        assert abs(st_pc.iterations - it_np) <= 2
        assert 10 * st_pc.iterations <= st_id.iterations
        assert res(x_pc) <= 10 * res(x_id)


# ---------------------------------------------------------------- 4. the models
def device_kernel(kind, variance, ls):
    from cggp import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[kind]
    return cls(variance=variance, lengthscales=[float(v) for v in ls])


def tight_cg(M, pre=None, thr=1e-15):
    from cggp.conjugate_gradient import ConjugateGradient
    return ConjugateGradient(thr, preconditioner=pre, max_iterations=4 * M, min_float=1e-30)


def problem(kind, D, M, N, seed=0):
    """The inputs of tests/test_gpu_cdgp_matrix_free.py: [-2, 2]^D, Z a subset, pseudo_u and counts from the
    nearest-centre pass."""
    from cggp.optimize import nearest_centre_statistics
    rng = np.random.default_rng(seed + D)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = np.sin(X[:, :3]).sum(axis=1, keepdims=True) + 0.3 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)]
    ls = rng.uniform(0.5, 0.9, D) * np.sqrt(D)
    kern = device_kernel(kind, 1.2, ls)
    _, sums, counts = nearest_centre_statistics(kern, T(Z), (T(X), T(y)))
    assert float(counts.min()) >= 1.0
    return T(X), T(y), T(Z), kern, (sums / counts)[:, None].contiguous(), counts[:, None].contiguous()


def rel(a, b):
    return abs(a - b) / abs(b)


def probes_of(M, P, seed):
    return T(2.0 * np.random.default_rng(seed).integers(0, 2, (M, P)) - 1.0)


def make_pre(wide):
    from cggp.conjugate_gradient import PivotedCholeskyPreconditioner
    return None if wide is None else PivotedCholeskyPreconditioner(rank=48, wide=wide)


@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_cggp_with_the_preconditioner_matches_the_model_without(kind):
    """Bars of tests/test_gpu_cdgp_matrix_free.py: prior_kl 1e-9, predict_f 1e-8 absolute, elbo 1e-8."""
    from cggp.models import CGGP
    M, N, s2, D = 300, 1500, 0.4, 3
    X, y, Z, kern, u, counts = problem(kind, D, M, N)
    make = lambda wide: CGGP(kern, s2, Z, tight_cg(M, make_pre(wide)), num_probes=5, pseudo_u=u, cluster_counts=counts,
                             num_data=N, matrix_free=True)
    plain = make(None)
    pr, xs, data = probes_of(M, 5, 5), X[100:164], (X[:64], y[:64])
    kl0, (mu0, var0), (_, cov0) = plain.prior_kl(pr), plain.predict_f(xs), plain.predict_f(xs, full_cov=True)
    (mub0, varb0), e0 = plain.predict_f_batched(X[:101], 37), plain.elbo(data, probes=pr)
    eb0 = plain.elbo_over_batches((X[:128], y[:128]), 64, shared_inverse=False, probes=pr)
    for wide in (False, True):
        m = make(wide)  # TypeError on the first solve without the feature
        kl = m.prior_kl(pr)
        mu, var = m.predict_f(xs)
        _, cov = m.predict_f(xs, full_cov=True)
        mub, varb = m.predict_f_batched(X[:101], 37)
        e = m.elbo(data, probes=pr)
        eb = m.elbo_over_batches((X[:128], y[:128]), 64, shared_inverse=False, probes=pr)
        dm, dv, dc = float((mu - mu0).abs().max()), float((var - var0).abs().max()), float((cov - cov0).abs().max())
        db = max(float((mub - mub0).abs().max()), float((varb - varb0).abs().max()))
        print(f"{kind} wide={wide}: prior_kl {rel(kl, kl0):.2e} (1e-9) mean {dm:.2e} variance {dv:.2e} cov {dc:.2e} "
              f"batched {db:.2e} (1e-8) elbo {rel(e, e0):.2e} over batches {rel(eb, eb0):.2e} (1e-8)")
        assert m.conjugate_gradient.preconditioner.rank_ == 48
        assert rel(kl, kl0) <= 1e-9
        assert dm <= 1e-8 and dv <= 1e-8 and dc <= 1e-8 and db <= 1e-8
        assert rel(e, e0) <= 1e-8 and rel(eb, eb0) <= 1e-8


def test_dense_cggp_is_refused_with_a_pointer_to_matrix_free():
    from cggp.models import CGGP, cdgp_class
    X, y, Z, kern, u, counts = problem("se", 3, 60, 300)
    kw = dict(pseudo_u=u, cluster_counts=counts, num_data=300)
    with pytest.raises(TypeError, match="matrix_free=True"):
        CGGP(kern, 0.4, Z, tight_cg(60, make_pre(False)), **kw).predict_f(X[:8])
    pre = make_pre(True)
    m = cdgp_class(kern, 0.4, Z, 1e-10, preconditioner=pre, matrix_free=True, **kw)
    assert m.conjugate_gradient.preconditioner is pre
    mu, var = m.predict_f(X[:8])
    assert bool(torch.isfinite(mu).all()) and bool((var > 0).all()) and pre.rank_ == 48  # the solves went through it


def loss_and_grads(m, data, probes):
    for p in m.parameters():
        p.grad = None
    loss = m.training_loss(data, probes=probes)
    loss.backward()
    return float(loss.detach()), torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters()]).numpy()


@pytest.mark.parametrize("tip", [False, True], ids=["fixed-Z", "trainable-Z"])
def test_training_loss_and_gradients_with_the_preconditioner(tip):
    """Bars of tests/test_gpu_cdgp_matrix_free.py: loss 1e-8, gradient 1e-7 of its largest entry."""
    from cggp.training import TrainableCGGP
    kind, D, M, B = "se", 4, 200, 50
    X, y, Z, kern, u, counts = problem(kind, D, M, 1000, seed=3)
    data, pr = (X[:B], y[:B]), probes_of(M, 5, 11)

    def make(wide, **kw):
        return TrainableCGGP(kern, 0.3, Z, tight_cg(M, make_pre(wide)), num_probes=5, pseudo_u=u, cluster_counts=counts,
                             num_data=1000, matrix_free=True, trainable_inducing=tip, **kw)

    configs = ({}, {"fused_solves": True}, {"independent_logdet_probes": True}, {"wide_solves": True})
    plain = [loss_and_grads(make(None, **kw), data, pr) for kw in configs]  # the same model without the preconditioner
    assert plain[0][1].shape == (D + 2 + (M * D if tip else 0),)
    for wide in (False, True):
        for kw, (l0, g0) in list(zip(configs, plain))[:4 if wide else 1]:
            m = make(wide, **kw)
            l1, g1 = loss_and_grads(m, data, pr)
            dist = np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))
            print(f"trainable_inducing={tip} wide={wide} {kw}: loss {rel(l1, l0):.2e} (1e-8) gradient {dist:.2e} (1e-7)")
            assert np.all(np.isfinite(g1)) and rel(l1, l0) <= 1e-8 and dist <= 1e-7
    # the factor is a constant of the solve, built from detached values: frozen_model carries the preconditioner on
    frozen = m.frozen_model()
    assert frozen.conjugate_gradient is m.conjugate_gradient and frozen.matrix_free
    mu, var = frozen.predict_f(X[:16])
    assert bool(torch.isfinite(mu).all()) and bool((var > 0).all())


def test_the_factor_is_built_once_and_follows_z_theta_and_lambda(monkeypatch):
    from cggp import ops
    from cggp.models import CGGP
    M, N = 300, 1500
    X, y, Z, kern, u, counts = problem("se", 3, M, N)
    pre = make_pre(True)
    m = CGGP(kern, 0.4, Z, tight_cg(M, pre, 1e-10), num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=N,
             matrix_free=True)
    calls = []
    inner = ops.kxx_pivchol
    monkeypatch.setattr(ops, "kxx_pivchol", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    m.predict_f_batched(X[:200], 37)  # six batches and the solve against pseudo_u
    assert len(calls) == 1
    L, B = pre.L, pre.B
    m.prior_kl(probes_of(M, 5, 1))
    assert len(calls) == 1 and pre.L is L and pre.B is B  # a new lambda tensor with the same values: nothing re-formed
    m.likelihood.variance = 0.2  # lambda changes: B is re-formed, L stays
    m.predict_f(X[:8])
    assert len(calls) == 1 and pre.L is L and pre.B is not B
    assert float((pre.D - 0.2 / counts[:, 0]).abs().max()) == 0.0
    B = pre.B
    kern.lengthscales = [0.7, 0.8, 0.9]  # theta changes: L is rebuilt
    m.predict_f(X[:8])
    assert len(calls) == 2 and pre.L is not L
    L = pre.L
    m.inducing_variable.Z.add_(1e-3)  # Z changes in place (an optimiser step): rebuilt
    m.predict_f(X[:8])
    assert len(calls) == 3 and pre.L is not L
    assert not pre.B.requires_grad and not pre.L.requires_grad
    # refusals: fp32 and a non-positive lambda, as for exact GPR
    from cggp.conjugate_gradient import KmmLambdaOperator
    Zm = m.inducing_variable.Z
    with pytest.raises(TypeError, match="fp64"):
        pre._native(KmmLambdaOperator(kern, Zm.float(), (0.4 / counts[:, 0]).float()))
    lam0 = (0.4 / counts[:, 0]).clone()
    lam0[3] = 0.0
    with pytest.raises(ValueError, match="lambda > 0"):
        make_pre(False)._native(KmmLambdaOperator(kern, Zm, lam0))


# ---------------------------------------------------------------- 5. the buffer contract of the route
CONTRACT = dict(Bt=70, k=33, n=1040)  # one 128 x 64 tile, five splits of 208 columns, a ragged last tile of pass 2


def contract_inputs(k=None):
    c = CONTRACT
    dinv, B, R, rng = hand_made(c["Bt"], c["k"] if k is None else k, c["n"], 4)
    A = np.diag(1.0 + rng.random(c["n"]))
    return T(A), T(dinv), T(B), T(R)


def test_the_pch_arena_shows_which_route_ran_and_a_stale_arena_does_not_reach_the_result():
    from cggp import _hip
    c = CONTRACT
    A, dinv, B, R = contract_inputs()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan_w, plan_n = cr.wide_arena_bytes(c["Bt"], c["k"], c["n"], cus), cr.narrow_arena_bytes(c["Bt"], c["k"], c["n"])
    assert plan_w > 2 * plan_n  # a growing handle rounds an arena up by a quarter: the two plans stay apart
    hd = fresh_handle()
    try:
        assert pch_bytes(hd) == 0
        rc, narrow = raw_solve(hd, A, Hand(dinv, B, KIND_NARROW), R, 3)
        held = pch_bytes(hd)
        assert rc == 0 and plan_n <= held < plan_w  # kind 5 reserved its own plan, not the many-column one ...
        rc, clean = raw_solve(hd, A, Hand(dinv, B, KIND_WIDE), R, 3)
        print(f"pch arena: {held} bytes after kind 5 (plan {plan_n}), {pch_bytes(hd)} after kind 6 (plan {plan_w})")
        assert rc == 0 and pch_bytes(hd) >= plan_w  # ... and kind 6 did: the wide route ran
        assert column_distance(clean, narrow) <= 1e-12
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])
    hd = fresh_handle()
    try:
        lib, h = hd
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        n2, k2 = 70000, 128
        z = torch.empty((16, n2), dtype=torch.float64, device=DEV)
        lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert lib.mgp_lowrank_apply(h, _hip.F64, _hip.ptr(nan(n2)), _hip.ptr(nan(k2, n2)), k2, n2, _hip.ptr(nan(16, n2)),
                                     16, _hip.ptr(z)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(z).all())
        before = pch_bytes(hd)
        assert before >= plan_w  # the arena is full of NaN partials and large enough: it will not grow
        rc, got = raw_solve(hd, A, Hand(dinv, B, KIND_WIDE), R, 3)
        assert rc == 0 and pch_bytes(hd) == before
        assert same_bits(got, clean)
    finally:
        torch.cuda.synchronize()
        hd[0].mgp_destroy(hd[1])


def test_fixed_pool_too_small_is_nomem_naming_the_many_column_plan():
    """k = 1024: the many-column plan (6 x 128 x 1024 doubles, 6 MiB) is larger than the quarter by which a growing
    handle rounds up everything a kind-5 solve reserves, so a fixed pool of the size that handle reports takes the
    kind-5 solve and then refuses exactly the many-column request."""
    c = CONTRACT
    k = 1024
    A, dinv, B, R = contract_inputs(k)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan_w = cr.wide_arena_bytes(c["Bt"], k, c["n"], cus)
    grow = fresh_handle()
    try:
        rc, _ = raw_solve(grow, A, Hand(dinv, B, KIND_NARROW), R, 3)
        fits5 = int(grow[0].mgp_workspace_bytes(grow[1]))
        rc6, ref = raw_solve(grow, A, Hand(dinv, B, KIND_WIDE), R, 3)
        fits = int(grow[0].mgp_workspace_bytes(grow[1]))
        assert rc == 0 and rc6 == 0
    finally:
        grow[0].mgp_destroy(grow[1])
    print(f"workspace after kind 5: {fits5} bytes, after kind 6: {fits}; the many-column plan: {plan_w}")
    assert plan_w > fits5 // 5  # the slack of the growing handle (a quarter of each arena) cannot hold it
    for pool, want in ((fits5, MGP_E_NOMEM), (fits + plan_w + (1 << 20), 0)):
        hd = fresh_handle(pool)
        try:
            rc5, _ = raw_solve(hd, A, Hand(dinv, B, KIND_NARROW), R, 3)
            assert rc5 == 0, hd[0].mgp_last_error(hd[1])
            rc, out = raw_solve(hd, A, Hand(dinv, B, KIND_WIDE), R, 3)
            assert rc == want, (pool, rc, hd[0].mgp_last_error(hd[1]))
            if want:
                msg = hd[0].mgp_last_error(hd[1])
                assert b"fixed workspace exhausted" in msg and f"{plan_w} bytes requested".encode() in msg, msg
            else:
                assert same_bits(out, ref)
        finally:
            torch.cuda.synchronize()
            hd[0].mgp_destroy(hd[1])
