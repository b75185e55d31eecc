"""The fused any-D sweeps (include/mgp_sweep_anyd.h, csrc/sweep_anyd.hip) on the GPU: per-pair values through one-hot
multipliers and dense products against long double, the buffer contract, the arena proof that no kernel panel is
written, fallback bits, determinism, the three operator kinds inside `mgp_operator_apply` and `mgp_pcg_solve`, and the
`fused_anyd` keyword of the models.

Bounds.  Per pair: `pair_reference.pair_bound(..., D, F64)`, (D + 6) u S on the distance, with no extra constant: the
chain of this kernel is the one that docstring derives (two fma chains for the squared norms, then D + 2 fused steps of
one accumulator, K ascending through the slices), and tests/test_sweep_anyd_plan.py shows an fp64 emulation of it inside
the same bound on the same point sets.  Dense multipliers: sum_j rel_ij k*_ij |w_j| + (nb + 2) u sum_j k*_ij |w_j|, the
second term the first-order bound of any summation order of nb terms (plus, where s2 v is added, u times the result).
"""

import contextlib
import ctypes

import numpy as np
import pytest
import torch

import buffer_contract as bc
import pair_reference as pr
import sweep_anyd_plan as ap

pytestmark = pytest.mark.gpu

LD = np.longdouble
VAR = pr.VARIANCE
F64 = np.float64
U = 2.0 ** -53
COLS, ROWS = 0, 1


def dev():
    return torch.device("cuda:0")


def T(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev())


def spec_of(name, D, ls=None, variance=VAR):
    from cggp import ops
    return ops.KernelSpec(name, variance, list(pr.lengthscales(D) if ls is None else ls), D)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def report(what, worst):
    print(f"sweep-anyd {what}: worst err / bound {worst:.3f}")


@contextlib.contextmanager
def fresh_handle(pool=0):
    """A handle nothing else has touched; pool > 0: a fixed workspace of that many bytes."""
    from cggp import _hip
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
    lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    try:
        yield lib, h
    finally:
        torch.cuda.synchronize()
        lib.mgp_destroy(h)


def call(lib, h, entry, k, X, Z, V, R, v_layout, out, out_layout, s2=0.0):
    """The raw entry point (plain or _anyd) on device pointers; X [N, D], Z [M, D] (unused for kxx)."""
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    if entry.startswith("mgp_kxx"):
        return getattr(lib, entry)(h, ctypes.byref(k), p(X[0]), X[1], s2, p(V), R, v_layout, p(out), out_layout)
    return getattr(lib, entry)(h, ctypes.byref(k), p(X[0]), X[1], p(Z[0]), Z[1], p(V), R, v_layout, p(out), out_layout)


# ---------------------------------------------------------------- per-pair values
_PAIRS = {}


def pair_orientations(name, D):
    if (name, D) not in _PAIRS:
        ls = pr.lengthscales(D)
        out = []
        for label, P, Q, cols in ap.pair_sets(name, D):
            Qc = Q[cols]
            pv = pr.pair_values(name, VAR, ls, P, Qc)
            rel = pr.pair_bound(name, VAR, pv.s, pv.q, pr.scaled(name, ls, P), pr.scaled(name, ls, Qc), D, F64)
            out.append((label, P, Q, cols, pv, rel))
        _PAIRS[(name, D)] = out
    return _PAIRS[(name, D)]


def one_hot(n, cols, R):
    V = np.zeros((n, R))
    V[cols[:R], np.arange(R)] = 1.0
    return V


@pytest.mark.parametrize("D", ap.PAIR_DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_pair_values(name, D):
    """knm_matvec_anyd(P, Q, one-hot) and kmn_matvec_anyd(Q, P, one-hot), both layouts, 1 and 8 columns: k(P, Q[cols])
    with P owned and Q streamed, every pair held to its bound or, below the flush floor, to the floor rule."""
    from cggp import ops
    spec = spec_of(name, D)
    worst = 0.0
    for label, P, Q, cols, pv, rel in pair_orientations(name, D):
        Pt, Qt = T(P), T(Q)
        for R in (1, 8):
            V = one_hot(Q.shape[0], cols, R)
            got = {"knm cols": ops.knm_matvec_anyd(spec, Pt, Qt, T(V), COLS),
                   "knm rows": ops.knm_matvec_anyd(spec, Pt, Qt, T(V.T), ROWS).t(),
                   "kmn cols": ops.kmn_matvec_anyd(spec, Qt, Pt, T(V), COLS),
                   "kmn rows": ops.kmn_matvec_anyd(spec, Qt, Pt, T(V.T), ROWS).t()}
            torch.cuda.synchronize()
            for what, g in got.items():
                worst = max(worst, pr.check_pairs(f"{what} {name} D={D} {label} R={R}", g.cpu().numpy(), pv.columns(R),
                                                  rel[:, :R], VAR, F64, col_ids=cols))
    report(f"pairs {name} D={D}", worst)


@pytest.mark.parametrize("name", pr.KINDS)
def test_pair_values_kxx_with_noise(name):
    """(k(X, X) + s2 I) e_j: off the diagonal the single kernel value, on it fl(s2 + variance k) -- one more rounding
    of the sum, checked as such."""
    from cggp import ops
    D, s2 = 77, 0.5
    spec = spec_of(name, D)
    ls = pr.lengthscales(D)
    worst = 0.0
    for label, P, _, _, _, _ in pair_orientations(name, D):
        if P.shape[0] > 400:
            P = P[-400:]  # the last run of the edge set: the far rows
        n = P.shape[0]
        cols = [0, n - 1, n - 2, n // 2, n // 2 + 1, n // 4, (3 * n) // 4, n // 3]
        pv = pr.pair_values(name, VAR, ls, P, P[cols])
        a = pr.scaled(name, ls, P)
        rel = pr.pair_bound(name, VAR, pv.s, pv.q, a, a[cols], D, F64)
        got = ops.kxx_matvec_anyd(spec, T(P), s2, T(one_hot(n, cols, 8)), COLS).cpu().numpy()
        for r, j in enumerate(cols):  # the diagonal entries, then handed to check_pairs as their reference value
            want = pv.k[j, r] + LD(s2)
            assert abs(got[j, r] - want) <= rel[j, r] * pv.k[j, r] + U * want, (name, label, j)
            got[j, r] = float(pv.k[j, r])
        worst = max(worst, pr.check_pairs(f"kxx {name} D={D} {label}", got, pv, rel, VAR, F64, col_ids=cols))
    report(f"pairs kxx {name} D={D}", worst)


# ---------------------------------------------------------------- dense multipliers
def dense_reference(case):
    """(A, B, ls, W, want [na, R] long double, tol [na, R])."""
    A, B, ls = ap.points(case)
    W = np.random.default_rng([7, case.na, case.nb, case.R]).standard_normal((case.nb, max(case.R, 0)))
    pv = pr.pair_values(case.kind, VAR, ls, A, B)
    rel = pr.pair_bound(case.kind, VAR, pv.s, pv.q, pr.scaled(case.kind, ls, A), pr.scaled(case.kind, ls, B), case.D, F64)
    Wl = W.astype(LD)
    want = pv.k @ Wl
    mag = pv.k @ np.abs(Wl)
    tol = (rel.astype(LD) * pv.k) @ np.abs(Wl) + (case.nb + 2) * U * mag
    if case.entry == "kxx":
        want = want + LD(case.s2) * Wl
        tol = tol + U * (np.abs(want) + LD(case.s2) * np.abs(Wl))  # the fma with s2 v: one rounding of the result
    return A, B, ls, W, want, tol


def run_dense(case, A, B, ls, W):
    from cggp import ops
    spec = spec_of(case.kind, case.D, ls)
    Wt = T(W if case.w_layout == COLS else W.T)
    if case.entry == "knm":
        out = ops.knm_matvec_anyd(spec, T(A), T(B), Wt, case.w_layout, case.out_layout)
    elif case.entry == "kmn":  # owned = Z (A), streamed = X (B)
        out = ops.kmn_matvec_anyd(spec, T(B), T(A), Wt, case.w_layout, case.out_layout)
    else:
        out = ops.kxx_matvec_anyd(spec, T(A), case.s2, Wt, case.w_layout, case.out_layout)
    torch.cuda.synchronize()
    assert tuple(out.shape) == ((case.na, case.R) if case.out_layout == COLS else (case.R, case.na))
    return (out if case.out_layout == COLS else out.t()).cpu().numpy()


@pytest.mark.parametrize("case", ap.dense_cases(), ids=lambda c: c.id)
def test_dense_multipliers(case):
    A, B, ls, W, want, tol = dense_reference(case)
    got = run_dense(case, A, B, ls, W)
    if case.R == 0:
        assert got.shape == (case.na, 0)
        return
    assert np.all(np.isfinite(got))
    ratio = np.abs(got.astype(LD) - want) / tol
    report(f"dense {case.id}", float(ratio.max()))
    assert ratio.max() <= 1.0, (case.id, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))


def test_unsplit_streamed_set():
    """So many owned blocks that the streamed set is one chunk: a workgroup walks three tiles; a sample of rows is held
    to the long-double product (the first and last blocks, block seams, random rows)."""
    case = ap.unsplit_case(cus())
    assert ap.chunk_plan(case.na, case.nb, cus())[1] == 1
    A, B, ls = ap.points(case)
    W = np.random.default_rng(11).standard_normal((case.nb, 1))
    got = run_dense(case, A, B, ls, W)
    rows = np.unique(np.concatenate([np.arange(0, 130), np.arange(case.na - 130, case.na),
                                     np.random.default_rng(12).integers(0, case.na, 140)]))
    pv = pr.pair_values(case.kind, VAR, ls, A[rows], B)
    rel = pr.pair_bound(case.kind, VAR, pv.s, pv.q, pr.scaled(case.kind, ls, A[rows]), pr.scaled(case.kind, ls, B),
                        case.D, F64)
    Wl = W.astype(LD)
    tol = (rel.astype(LD) * pv.k) @ np.abs(Wl) + (case.nb + 2) * U * (pv.k @ np.abs(Wl))
    ratio = np.abs(got[rows].astype(LD) - pv.k @ Wl) / tol
    report(f"dense {case.id}", float(ratio.max()))
    assert np.all(np.isfinite(got)) and ratio.max() <= 1.0


def test_empty_inputs():
    """nb = 0: zeros (kxx cannot have it); na = 0 and R = 0: nothing is written; as the plain names."""
    from cggp import ops
    D = 40
    spec = spec_of("se", D)
    X, Z0 = T(np.random.default_rng(1).standard_normal((70, D))), T(np.zeros((0, D)))
    assert torch.equal(ops.knm_matvec_anyd(spec, X, Z0, T(np.zeros((0, 3)))), torch.zeros((70, 3), dtype=torch.float64,
                                                                                           device=dev()))
    assert torch.equal(ops.kmn_matvec_anyd(spec, Z0, X, T(np.zeros((0, 2)))), torch.zeros((70, 2), dtype=torch.float64,
                                                                                           device=dev()))
    assert tuple(ops.knm_matvec_anyd(spec, Z0, X, T(np.zeros((70, 3)))).shape) == (0, 3)
    assert tuple(ops.kxx_matvec_anyd(spec, X, 0.1, T(np.zeros((70, 0)))).shape) == (70, 0)


# ---------------------------------------------------------------- memory
@pytest.mark.parametrize("entry", ["knm", "kmn", "kxx"])
def test_buffer_contract(entry):
    """Guard bands round out, inputs bit-identical afterwards, NaN-filled memory directly behind W, X and Z (the guards
    are quiet NaNs), element-aligned bases one double past a 16-byte boundary; the result is still the right one."""
    from cggp import _hip
    D, N, M, R = 77, 131, 70, 3
    case = ap.Case(entry, "matern52", D, N if entry != "kmn" else M, M if entry == "knm" else N, R, s2=0.25)
    A, B, ls, W, want, tol = dense_reference(case)
    k = spec_of(case.kind, D, ls).struct(_hip.F64)
    gA = bc.guarded(A.shape, torch.float64, 1, dev())[1].upload(torch.from_numpy(A))
    gB = gA if entry == "kxx" else bc.guarded(B.shape, torch.float64, 1, dev())[1].upload(torch.from_numpy(B))
    gW = bc.guarded(W.shape, torch.float64, 1, dev())[1].upload(torch.from_numpy(W))
    gO = bc.guarded((case.na, R), torch.float64, 1, dev())[1]
    hd = _hip.get_handle(dev())
    X, Z = ((gA, gB) if entry == "knm" else (gB, gA))  # kmn: owned = Z
    rc = call(hd.lib, hd.h, f"mgp_{entry}_matvec_anyd", k, (X.ptr, X.shape[0]), (Z.ptr, Z.shape[0]), gW.ptr, R, COLS,
              gO.ptr, COLS, s2=case.s2)
    hd.check(rc)
    torch.cuda.synchronize()
    for g, name in ((gA, "owned"), (gB, "streamed"), (gW, "W")):
        g.check_input(name)
    gO.check_output(np.ones((case.na, R), dtype=bool), "out")
    got = gO.payload.cpu().numpy()
    assert (np.abs(got.astype(LD) - want) / tol).max() <= 1.0


# ---------------------------------------------------------------- the route: ws alone, never gen
@pytest.mark.parametrize("entry,N,M,R", [("knm", 391, 150, 5), ("kmn", 1000, 129, 8), ("kxx", 300, 300, 1)])
def test_route_proof(entry, N, M, R):
    from cggp import _hip
    D = 77
    rng = np.random.default_rng([3, N, M])
    X, Z = T(rng.standard_normal((N, D))), T(rng.standard_normal((M, D)))
    na, nb = {"knm": (N, M), "kmn": (M, N), "kxx": (N, N)}[entry]
    V = T(rng.standard_normal((nb, R)))
    k = spec_of("se", D, pr.lengthscales(D) * np.sqrt(D)).struct(_hip.F64)
    need = ap.ws_bytes(na, nb, R, cus())
    outs = {}
    for name in (f"mgp_{entry}_matvec_anyd", f"mgp_{entry}_matvec"):
        with fresh_handle() as (lib, h):
            out = torch.full((na, R), float("nan"), dtype=torch.float64, device=dev())
            assert call(lib, h, name, k, (X, N), (Z, M), V, R, COLS, out, COLS, s2=0.3) == 0, lib.mgp_last_error(h)
            torch.cuda.synchronize()
            gen, ws = lib.mgp_arena_bytes(h, b"gen"), lib.mgp_arena_bytes(h, b"ws")
            if name.endswith("_anyd"):
                assert gen == 0, gen
                assert ws == need + (need >> 2) + 4096, (ws, need)  # mgp_reserve's allocation for exactly the plan's request
                total = lib.mgp_workspace_bytes(h)
            else:
                assert gen > 0  # the probe sees the panel route's arena
            outs[name] = out
    assert torch.allclose(*outs.values(), rtol=1e-11, atol=1e-12)  # the panel route, direct differences
    # a fixed pool of the size a growing handle reports serves the same call; one that cannot hold ws is refused
    with fresh_handle(pool=total) as (lib, h):
        out = torch.full((na, R), float("nan"), dtype=torch.float64, device=dev())
        assert call(lib, h, f"mgp_{entry}_matvec_anyd", k, (X, N), (Z, M), V, R, COLS, out, COLS, s2=0.3) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, outs[f"mgp_{entry}_matvec_anyd"])
        assert lib.mgp_arena_bytes(h, b"gen") == 0
    with fresh_handle(pool=need // 2) as (lib, h):
        out = torch.zeros((na, R), dtype=torch.float64, device=dev())
        assert call(lib, h, f"mgp_{entry}_matvec_anyd", k, (X, N), (Z, M), V, R, COLS, out, COLS, s2=0.3) == -6  # MGP_E_NOMEM


# ---------------------------------------------------------------- fallbacks give the plain bits
@pytest.mark.parametrize("D,dtype", [(8, torch.float64), (32, torch.float64), (40, torch.float32)])
def test_fallback_bits(D, dtype):
    from cggp import kernels, ops
    from cggp.conjugate_gradient import KmmLambdaOperator, KxxNoiseOperator, SgprNormalOperator
    rng = np.random.default_rng([5, D])
    N, M, R = 300, 70, 3
    X = torch.from_numpy(rng.standard_normal((N, D))).to(dtype).to(dev())
    Z = torch.from_numpy(rng.standard_normal((M, D))).to(dtype).to(dev())
    V = torch.from_numpy(rng.standard_normal((M, R))).to(dtype).to(dev())
    Wn = torch.from_numpy(rng.standard_normal((N, R))).to(dtype).to(dev())
    spec = spec_of("matern32", D, pr.lengthscales(D) * np.sqrt(D))
    assert torch.equal(ops.knm_matvec_anyd(spec, X, Z, V), ops.knm_matvec(spec, X, Z, V))
    assert torch.equal(ops.kmn_matvec_anyd(spec, X, Z, Wn), ops.kmn_matvec(spec, X, Z, Wn))
    assert torch.equal(ops.kxx_matvec_anyd(spec, X, 0.2, Wn), ops.kxx_matvec(spec, X, 0.2, Wn))
    kern = kernels.Matern32(VAR, list(pr.lengthscales(D) * np.sqrt(D)))
    lam = torch.from_numpy(rng.random(M) + 0.5).to(dtype).to(dev())
    P = V.t().contiguous()
    for make in (lambda f: SgprNormalOperator(kern, X, Z, 0.3, jitter=1e-6, fused_anyd=f),
                 lambda f: KmmLambdaOperator(kern, Z, lam, fused_anyd=f)):
        assert torch.equal(make(True).rmatmul(P), make(False).rmatmul(P))
    Pn = Wn.t().contiguous()
    assert torch.equal(KxxNoiseOperator(kern, X, 0.2, fused_anyd=True).rmatmul(Pn),
                       KxxNoiseOperator(kern, X, 0.2).rmatmul(Pn))


# ---------------------------------------------------------------- determinism
def test_bit_reproducible_and_shards_add_up():
    from cggp import ops
    D, N, M, R = 90, 1000, 129, 3
    rng = np.random.default_rng(21)
    ls = pr.lengthscales(D) * np.sqrt(D)
    Xn, Zn, Wn = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((N, R))
    X, Z, W = T(Xn), T(Zn), T(Wn)
    spec = spec_of("se", D, ls)
    a, b = ops.kmn_matvec_anyd(spec, X, Z, W), ops.kmn_matvec_anyd(spec, X, Z, W)
    assert torch.equal(a, b)
    assert torch.equal(ops.knm_matvec_anyd(spec, X, Z, a), ops.knm_matvec_anyd(spec, X, Z, a))
    cut = 437  # no multiple of the tile: the chunk seams of the shards fall elsewhere than those of the whole
    parts = ops.kmn_matvec_anyd(spec, X[:cut], Z, W[:cut]) + ops.kmn_matvec_anyd(spec, X[cut:], Z, W[cut:])
    pv = pr.pair_values("se", VAR, ls, Zn, Xn)
    terms = (pv.k.astype(F64) @ np.abs(Wn))  # sum of |terms| per output entry
    ratio = (parts - a).abs().cpu().numpy() / (2 * U * terms)
    report("shards against the whole (2 u sum|terms|)", float(ratio.max()))
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------- operators and CG
def cg_points(D, N, M, seed, latent=8, ell=1.2):
    """Standard normal clouds in a `latent`-dimensional subspace of R^D (a random orthonormal embedding), lengthscale
    `ell` in every dimension.  Independent clouds in all D dimensions have nearly equal distances -- a kernel matrix of
    one large eigenvalue and a cluster, which CG solves in three steps and then only rounds; these have a spread
    spectrum and a moderate condition number, so the iterates of the first dozen steps are well defined."""
    rng = np.random.default_rng([seed, D, N, M])
    Q, _ = np.linalg.qr(rng.standard_normal((D, latent)))
    return rng.standard_normal((N, latent)) @ Q.T, rng.standard_normal((M, latent)) @ Q.T, np.full(D, ell)


def k64(name, ls, A, B):
    return pr.pair_values(name, VAR, ls, A, B).k


def test_operator_apply_against_long_double():
    """Kinds 5, 6 and 7 through mgp_operator_apply against the long-double product, within the bound of its sums."""
    from cggp import kernels
    from cggp.conjugate_gradient import KmmLambdaOperator, KxxNoiseOperator, SgprNormalOperator
    from cggp import _hip
    D, N, M, Bt = 77, 300, 130, 3
    Xn, Zn, ls = cg_points(D, N, M, 31)
    kern = kernels.SquaredExponential(VAR, list(ls))
    X, Z = T(Xn), T(Zn)
    Knm, Kmm, Kxx = k64("se", ls, Xn, Zn), k64("se", ls, Zn, Zn), k64("se", ls, Xn, Xn)
    rng = np.random.default_rng(32)
    P = rng.standard_normal((Bt, M))
    lam = rng.random(M) + 0.5
    s2 = 0.3
    # per-term rounding of a kernel value at these points: (D + 6) u S ln2 + 8u, S <= 4 max|a|^2
    a2 = max((pr.scaled("se", ls, Xn) ** 2).sum(1).max(), (pr.scaled("se", ls, Zn) ** 2).sum(1).max())
    rel = np.log(2.0) * (D + 6) * U * 4 * a2 + 8 * U

    op = SgprNormalOperator(kern, X, Z, s2, jitter=0.0, fused_anyd=True)
    assert op._struct()[0].kind == _hip.OP_SGPR_ANYD == 5
    got = op.rmatmul(T(P)).cpu().numpy()
    Pl = P.astype(LD)
    want = (Pl @ Knm.T) @ Knm + LD(s2) * (Pl @ Kmm)
    mag = (np.abs(Pl) @ Knm.T) @ Knm + LD(s2) * (np.abs(Pl) @ Kmm)
    tol = (2 * rel + (N + M + 6) * U) * mag
    worst = float((np.abs(got - want) / tol).max())
    report("operator_apply kind 5", worst)
    assert worst <= 1.0

    op = KmmLambdaOperator(kern, Z, T(lam), fused_anyd=True)
    assert op._struct_for(Bt)[0].kind == _hip.OP_KMM_LAMBDA_ANYD == 6
    got = op.rmatmul(T(P)).cpu().numpy()
    want = Pl @ Kmm + Pl * lam.astype(LD)
    tol = (rel + (M + 4) * U) * (np.abs(Pl) @ Kmm + np.abs(Pl) * lam)
    worst = float((np.abs(got - want) / tol).max())
    report("operator_apply kind 6", worst)
    assert worst <= 1.0

    op = KxxNoiseOperator(kern, X, s2, fused_anyd=True)
    assert op._struct()[0].kind == _hip.OP_KXX_NOISE_ANYD == 7
    Pn = rng.standard_normal((Bt, N))
    got = op.rmatmul(T(Pn)).cpu().numpy()
    Pnl = Pn.astype(LD)
    want = Pnl @ Kxx + LD(s2) * Pnl
    tol = (rel + (N + 4) * U) * (np.abs(Pnl) @ Kxx + s2 * np.abs(Pnl))
    worst = float((np.abs(got - want) / tol).max())
    report("operator_apply kind 7", worst)
    assert worst <= 1.0


class PerturbedMatrix:
    """A for oracle/cg.py with every product off by `eps` of its sum of magnitudes, at random: an operator that is
    correct within a relative bound `eps`, as the fused sweeps are."""

    def __init__(self, A, eps, seed):
        self.A, self.eps, self.rng, self.shape = A, eps, np.random.default_rng(seed), A.shape

    def rmatmul(self, p):
        out = p @ self.A
        return out + self.eps * self.rng.standard_normal(out.shape) * (np.abs(p) @ np.abs(self.A))


@pytest.mark.parametrize("kind,D,N,M", [(5, 77, 300, 130), (7, 40, 260, 0)])
def test_pcg_solve_fixed_steps_against_the_oracle(kind, D, N, M):
    """mgp_pcg_solve on kinds 5 and 7 after 3 and 5 steps against oracle/cg.py on the fp64 matrix, at the suite's 1e-9
    (tests/test_gpu_dense1.py).  This is the comparison against the oracle, not the fallback against the plain kind.

    The iterates depend on the operator within its bound, and CG amplifies a perturbation of the operator from the step
    at which its first Ritz value has converged (a kernel matrix has a separated top eigenvalue: oracle/cg.py itself,
    given products off by 1e-15, is 1e-14 from its own 5-step iterate, 1e-10 from the 8-step and 1e-4 from the 12-step
    one).  So "conditioned for 1e-9" is checked as what it has to mean: the oracle on `PerturbedMatrix` with eps = the
    bound of the fused operator's product stays within 1e-10 of the oracle on A at every compared step, and the solve
    is still under way there (iterates are compared, not the rounding of a converged solve)."""
    from cggp import kernels
    from cggp.conjugate_gradient import KxxNoiseOperator, SgprNormalOperator, conjugate_gradient
    from oracle import cg as ocg
    Xn, Zn, ls = cg_points(D, N, max(M, 1), 41, *((8, 1.2) if kind == 5 else (4, 1.5)))
    kern = kernels.SquaredExponential(VAR, list(ls))
    s2 = 0.5
    # a kernel value: ln2 (D + 6) u S + 8u with S <= 4 max|a|^2; a sweep's sum: (n + 2) u
    a2 = max((pr.scaled("se", ls, Xn) ** 2).sum(1).max(), (pr.scaled("se", ls, Zn) ** 2).sum(1).max())
    rel = np.log(2.0) * (D + 6) * U * 4 * a2 + 8 * U
    if kind == 5:
        Knm, Kmm = k64("se", ls, Xn, Zn), k64("se", ls, Zn, Zn)
        A = (Knm.T @ Knm + LD(s2) * Kmm).astype(F64)
        op = SgprNormalOperator(kern, T(Xn), T(Zn), s2, jitter=0.0, fused_anyd=True)
        eps = 2 * rel + (N + M + 6) * U  # two sweeps
    else:
        A = (k64("se", ls, Xn, Xn) + LD(s2) * np.eye(N, dtype=LD)).astype(F64)
        op = KxxNoiseOperator(kern, T(Xn), s2, fused_anyd=True)
        eps = rel + (N + 4) * U
    n = A.shape[0]
    rhs = np.random.default_rng(42).standard_normal((2, n))
    exact = np.linalg.solve(A, rhs.T).T
    for k in (3, 5):
        o_sol, (o_steps, o_err) = ocg.conjugate_gradient(A, rhs, np.zeros((2, n)), 0.0, max_iterations=k,
                                                         max_steps_cycle=k + 1)
        assert np.linalg.norm(o_sol - exact) > 1e-4 * np.linalg.norm(exact)  # not converged: an iterate, not a limit
        for seed in range(3):  # conditioned for the comparison
            p_sol, _ = ocg.conjugate_gradient(PerturbedMatrix(A, eps, seed), rhs, np.zeros((2, n)), 0.0,
                                              max_iterations=k, max_steps_cycle=k + 1)
            assert np.linalg.norm(p_sol - o_sol) < 1e-10 * np.linalg.norm(o_sol), (k, eps)
        sol, (steps, err) = conjugate_gradient(op, T(rhs), None, 0.0, max_iterations=k, max_steps_cycle=k + 1)
        rel_diff = np.linalg.norm(sol.cpu().numpy() - o_sol) / np.linalg.norm(o_sol)
        print(f"sweep-anyd pcg kind {kind} k={k}: cond {np.linalg.cond(A):.3g}, eps {eps:.2e}, relative difference {rel_diff:.3e}")
        assert int(steps) == k == o_steps and rel_diff < 1e-9


def test_sgpr_anyd_with_the_allreduce_hook_on_one_rank():
    """Kind 5 with the `allreduce` hook set and world_size = 1 equals the call with no hook."""
    from cggp import kernels
    from cggp.conjugate_gradient import SgprNormalOperator
    D, N, M = 77, 300, 130
    Xn, Zn, ls = cg_points(D, N, M, 51)
    kern = kernels.SquaredExponential(VAR, list(ls))

    class OneRank:
        world_size = 1
        calls = 0

        def __call__(self, t):
            OneRank.calls += 1

    P = T(np.random.default_rng(52).standard_normal((1, M)))
    plain = SgprNormalOperator(kern, T(Xn), T(Zn), 0.3, fused_anyd=True).rmatmul(P)
    hooked = SgprNormalOperator(kern, T(Xn), T(Zn), 0.3, allreduce=OneRank(), kmm_rows=(0, M), fused_anyd=True)
    assert hooked._struct()[0].kind == 5
    got = hooked.rmatmul(P)
    assert OneRank.calls == 1 and torch.equal(got, plain)


# ---------------------------------------------------------------- models
def model_data(D=77, N=600, M=40, seed=61):
    rng = np.random.default_rng([seed, D])
    ls = pr.lengthscales(D) * np.sqrt(D / 2.0)
    X = rng.standard_normal((N, D))
    w = rng.standard_normal(D) / np.sqrt(D)
    Y = np.sin(X @ w)[:, None] + 0.1 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)] + 0.01 * rng.standard_normal((M, D))
    Xs = rng.standard_normal((50, D))
    return X, Y, Z, Xs, ls


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_sgpr_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, Z, Xs, ls = model_data()
    make = lambda f: models.SGPR((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), T(Z), 0.2,
                                 ConjugateGradient(1e-12, max_iterations=2000), explicit_rhs=0, fused_anyd=f)
    on, off = make(True), make(False)
    assert on.operator()._struct()[0].kind == 5 and off.operator()._struct()[0].kind == 1
    (m1, v1), (m0, v0) = on.predict_f(T(Xs)), off.predict_f(T(Xs))
    assert relerr(m1, m0) < 1e-6 and relerr(v1, v0) < 1e-6
    assert abs(float(on.elbo()) - float(off.elbo())) <= 1e-6 * abs(float(off.elbo()))
    assert models.sgpr_class((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), models.Gaussian(0.2), T(Z),
                             fused_anyd="auto").fused_anyd == "auto"
    with pytest.raises(ValueError):
        make("yes")


def test_trainable_sgpr_takes_an_adam_step():
    from cggp import kernels, training
    X, Y, Z, _, ls = model_data(N=400, M=30)
    m = training.TrainableSGPR(kernels.SquaredExponential(VAR, list(ls)), 0.2, T(X), T(Y), T(Z), fused_anyd=True)
    params = m.parameters()
    opt = torch.optim.Adam(params, lr=1e-2)
    opt.zero_grad()
    loss = m.training_loss()
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    opt.step()
    assert np.isfinite(float(m.training_loss().detach()))
    assert m.frozen_model().fused_anyd is True
    with pytest.raises(ValueError):
        training.TrainableSGPR(kernels.SquaredExponential(VAR, list(ls)), 0.2, T(X), T(Y), T(Z), fused_anyd=2)


def test_cggp_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, Z, Xs, ls = model_data(M=60)
    rng = np.random.default_rng(71)
    u = T(rng.standard_normal((60, 1)))
    counts = T(rng.integers(5, 15, size=(60, 1)).astype(F64))
    make = lambda **kw: models.CGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z),
                                    ConjugateGradient(1e-12, max_iterations=2000), num_probes=5, pseudo_u=u,
                                    cluster_counts=counts, num_data=600, **kw)
    on, off = make(matrix_free=True, fused_anyd=True), make(matrix_free=True)
    assert on._system()[1].kind_for(1) == 6 and off._system()[1].kind_for(1) == 2
    (m1, v1), (m0, v0) = on.predict_f(T(Xs)), off.predict_f(T(Xs))
    assert relerr(m1, m0) < 1e-6 and relerr(v1, v0) < 1e-6
    with pytest.raises(ValueError):
        make(fused_anyd=True)  # without matrix_free there is no sweep to fuse
    with pytest.raises(ValueError):
        make(matrix_free=True, fused_anyd="on")
    assert models.cdgp_class(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z), matrix_free=True, fused_anyd=True,
                             pseudo_u=u, cluster_counts=counts, num_data=600).fused_anyd is True


def test_gpr_model():
    from cggp import kernels, models
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, _, Xs, ls = model_data(N=500)
    make = lambda f: models.GPR((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), noise_variance=0.2,
                                conjugate_gradient=ConjugateGradient(1e-12, max_iterations=2000), solver="cg",
                                fused_anyd=f)
    on, off = make(True), make(False)
    assert on.operator()._struct()[0].kind == 7 and off.operator()._struct()[0].kind == 3
    rhs = T(np.random.default_rng(81).standard_normal((500, 2)))
    assert relerr(on.solve(rhs), off.solve(rhs)) < 1e-6
    (m1, v1), (m0, v0) = on.predict_f(T(Xs)), off.predict_f(T(Xs))
    assert relerr(m1, m0) < 1e-6 and relerr(v1, v0) < 1e-6
    assert models.gpr_class((T(X), T(Y)), kernels.SquaredExponential(VAR, list(ls)), models.Gaussian(0.2),
                            fused_anyd=True).fused_anyd is True
    with pytest.raises(ValueError):
        make(None)


def test_trainable_cggp_and_gpr():
    """`TrainableCGGP(matrix_free=True, fused_anyd=True)`: loss and every gradient against `fused_anyd=False` at the
    bars the suite holds the matrix-free model to against the dense one (1e-8 / 1e-7,
    tests/test_gpu_cdgp_matrix_free.py), for the "batch" and "trace" data terms; `TrainableGPR(num_probes=,
    fused_anyd=True)` likewise; the refusals."""
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    X, Y, Z, _, ls = model_data(M=60)
    rng = np.random.default_rng(91)
    u = T(rng.standard_normal((60, 1)))
    counts = T(rng.integers(5, 15, size=(60, 1)).astype(F64))
    probes = T(rng.choice([-1.0, 1.0], size=(60, 5)))
    data = (T(X[:50]), T(Y[:50]))

    def run(m, *args, **kw):
        for p in m.parameters():
            p.grad = None
        loss = m.training_loss(*args, **kw)
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters()]).numpy()

    for term in ("batch", "trace"):
        make = lambda f: training.TrainableCGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z),
                                                ConjugateGradient(1e-13, max_iterations=2000), num_probes=5, pseudo_u=u,
                                                cluster_counts=counts, num_data=600, matrix_free=True, data_term=term,
                                                fused_anyd=f)
        (l1, g1), (l0, g0) = run(make(True), data, probes=probes), run(make(False), data, probes=probes)
        assert np.all(np.isfinite(g1)) and abs(l1 - l0) <= 1e-8 * abs(l0), (term, l1, l0)
        assert np.max(np.abs(g1 - g0)) <= 1e-7 * np.max(np.abs(g0)), term
    assert make(True).frozen_model().fused_anyd is True
    with pytest.raises(ValueError):
        training.TrainableCGGP(kernels.SquaredExponential(VAR, list(ls)), 0.3, T(Z), ConjugateGradient(1e-8),
                               pseudo_u=u, cluster_counts=counts, fused_anyd=True)  # no matrix_free
    gpr = lambda f: training.TrainableGPR(kernels.SquaredExponential(VAR, list(ls)), 0.2, T(X), T(Y), num_probes=4,
                                          conjugate_gradient=ConjugateGradient(1e-13, max_iterations=2000), fused_anyd=f)
    (l1, g1), (l0, g0) = run(gpr(True)), run(gpr(False))
    assert np.all(np.isfinite(g1)) and abs(l1 - l0) <= 1e-8 * abs(l0)
    assert np.max(np.abs(g1 - g0)) <= 1e-7 * np.max(np.abs(g0))
    assert gpr("auto").frozen_model().fused_anyd == "auto"
    with pytest.raises(ValueError):
        gpr("no")
