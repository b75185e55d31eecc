"""Single kernel values of every device route against long double, pair by pair, within a derived rounding bound.

A multiplier with a single 1 makes a product return one kernel value exactly (the other terms are k * 0, and adding
zeros is exact on the VALU, in the partial-sum reductions and on the matrix cores), so K[:, j] leaves through the code
a CG step runs.  Each value is held to `pair_reference.pair_bound` -- constants fixed by its derivation and checked on
the CPU in tests/test_pair_reference.py -- and pairs below the flush floor to the floor rule (`check_pairs`); no pair
is masked out.  The point sets (`pair_reference.range_set`, `shifted_set`, `edge_set`) hit every entry of both exp2
tables, a large |a|^2 folded into the SE magic constant, and both sides of the `safe` decision of the fast sweeps.

Every probe prints `pair-accuracy <route> ...: worst err / bound`; DESIGN section 4.8a records a run's figures.
"""

import numpy as np
import pytest
import torch

import pair_reference as pr
import switch_forms as sf

pytestmark = pytest.mark.gpu

LD = np.longdouble
VAR = pr.VARIANCE
DIMS = (1, 3, 8, 16, 17, 32)
F64, F32 = np.float64, np.float32
U64 = 2.0 ** -53


def dev():
    return torch.device("cuda:0")


def T(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev())


def spec_of(name, D, variance=VAR):
    from cggp import ops
    return ops.KernelSpec(name, variance, list(pr.lengthscales(D)), D)


def report(route, what, worst):
    print(f"pair-accuracy {route} {what}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------- the probed orientations and their references
class Orientation:
    """k(P, Q[cols]): P the owned side (one output row per point), Q the streamed side, probed at `cols`."""

    def __init__(self, label, name, P, Q, cols, dtype):
        self.label, self.cols = label, list(cols)
        self.P, self.Q = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)  # what the device is given
        D = P.shape[1]
        ls = pr.lengthscales(D)
        Qc = self.Q[self.cols]
        self.pv = pr.pair_values(name, VAR, ls, self.P, Qc)
        self.rel = pr.pair_bound(name, VAR, self.pv.s, self.pv.q, pr.scaled(name, ls, self.P), pr.scaled(name, ls, Qc), D,
                                 dtype)

    def one_hot(self, R):
        V = np.zeros((self.Q.shape[0], R))
        V[self.cols[:R], np.arange(R)] = 1.0
        return V


_ORIENTATIONS = {}


def orientations(name, D, dtype=F64, n_range=1 << 15):
    """Seven orientations per (kernel, D): the range set and its reverse (whole and the rows with tau < 8), the shifted
    clouds 4097 x 63 both ways (several streamed chunks, an odd streamed count, one-hots on the first and last streamed
    point, beside the pad row and on both sides of chunk boundaries, which fall on multiples of 64, 128 or 256), and the
    edge set both ways.  The first column of each is the one a single right-hand side probes."""
    key = (name, D, np.dtype(dtype).name, n_range)
    if key not in _ORIENTATIONS:
        n = n_range
        X, Z, _, near = pr.range_set(name, D, n)
        rows = [0, near // 2, near - 1, n - 1, n - 2, n // 4, n // 4 + 1, (3 * n) // 7]
        near_rows = [0, near // 2, near - 1, near - 2, n // 4, n // 4 + 1, (3 * n) // 7, 255]
        out = [Orientation("range", name, X, Z, range(8), dtype),
               Orientation("range-reversed", name, Z, X, rows, dtype),
               Orientation("range-near-reversed", name, Z, X[:near], near_rows, dtype)]
        X, Z, _ = pr.shifted_set(name, D, 4097, 63)
        out += [Orientation("shifted", name, X, Z, [0, 62, 61, 31, 32, 1, 17, 40], dtype),
                Orientation("shifted-reversed", name, Z, X, [0, 4096, 4095, 255, 256, 2047, 2048, 1000], dtype)]
        X, Z, _, far = pr.edge_set(name, D, 6444, 2500)
        out += [Orientation("edge", name, X, Z, [0, 1, 2499, 2047, 2048, 100, 1234, 2498], dtype),
                Orientation("edge-reversed", name, Z, X, [far[-1], far[-20], far[-40], far[-64], far[0], far[7], 0, 6443],
                            dtype)]
        _ORIENTATIONS[key] = out
    return _ORIENTATIONS[key]


def check(route, name, D, o, got, R, dtype, extra_rel=0.0, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    label = f"{route} {what} {name} D={D} {o.label} R={R} {np.dtype(dtype).name}"
    return pr.check_pairs(label, got, o.pv.columns(R), o.rel[:, :R], VAR, dtype, extra_rel=extra_rel, col_ids=o.cols)


def sweep_probe(route, name, D, dtype=F64, Rs=(1, 2, 4, 8), n_range=1 << 15):
    """knm_matvec(P, Q, one-hot) and kmn_matvec(Q, P, one-hot), COLS and ROWS, for every orientation: both return
    k(P, Q[cols]) with P owned and Q streamed."""
    from cggp import ops
    spec = spec_of(name, D)
    worst = 0.0
    for o in orientations(name, D, dtype, n_range):
        Pt, Qt = T(o.P, dtype), T(o.Q, dtype)
        for R in Rs:
            V = o.one_hot(R)
            got = {"knm cols": ops.knm_matvec(spec, Pt, Qt, T(V, dtype), ops.COLS),
                   "knm rows": ops.knm_matvec(spec, Pt, Qt, T(V.T, dtype), ops.ROWS).t(),
                   "kmn cols": ops.kmn_matvec(spec, Qt, Pt, T(V, dtype), ops.COLS),
                   "kmn rows": ops.kmn_matvec(spec, Qt, Pt, T(V.T, dtype), ops.ROWS).t()}
            torch.cuda.synchronize()
            for what, g in got.items():
                worst = max(worst, check(route, name, D, o, g, R, dtype, what=what))
    return worst


# ---------------------------------------------------------------- sweeps
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_default_fast_sweep(name, D):
    """sweep_fast_kernel as the default handle launches it (8192-entry table and 512 threads at D <= 16, 2048 entries
    at D <= 32), RC = 1, 2, 4, 8, both layouts, both entry points."""
    report("sweep_fast", f"{name} D={D}", sweep_probe("sweep_fast", name, D))


# (dimensions, right-hand sides) in which the row's form is the one that runs (`routes` of the row, tests/switch_forms.py)
SWEEP_ROWS = {
    "sweep_mfma": (DIMS, (1, 2, 4, 8)),
    "sweep_lds_tile": (DIMS, (1, 2, 4, 8)),
    "sweep_fast_256": (DIMS, (1,)),
    "sweep_fast_256_rpt2": ((1, 3, 8), (1,)),
    "sweep_fast_256_rpt3": ((1, 3, 8), (1,)),
    "sweep_rpt2_default_form": ((1, 3, 8), (1,)),
    "sweep_rpt32_1": ((17, 32), (1,)),
    "sweep_rpt_rc3": ((1, 3, 8), (2, 4)),
}


@pytest.mark.parametrize("name", pr.KINDS)
@pytest.mark.parametrize("row_id", list(SWEEP_ROWS))
def test_sweep_switch_row(row_id, name, monkeypatch):
    row = next(r for r in sf.FORMS if r["id"] == row_id)
    dims, Rs = SWEEP_ROWS[row_id]
    with sf.switched(monkeypatch, row["env"]):
        for D in dims:
            report(row_id, f"{name} D={D}", sweep_probe(row_id, name, D, Rs=Rs))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_fp32_sweep(name, D):
    """sweep_kernel<float> with v_exp_f32, held to the fp32 bound.  The first blocks of the range set have |a|^2 < 64
    (the scaled-sum SE loop), its tail and the shifted clouds (|a|^2 ~ 170 - 200) do not qualify."""
    report("sweep_fp32", f"{name} D={D}", sweep_probe("sweep_fp32", name, D, F32, Rs=(1, 2, 8), n_range=1 << 12))


# ---------------------------------------------------------------- D > 32
@pytest.mark.parametrize("D", [33, 77])
@pytest.mark.parametrize("name", pr.KINDS)
def test_generic_dimension(name, D):
    """generic.hip (dimensions staged through LDS): knm_matvec / kmn_matvec and k_dense."""
    from cggp import ops
    worst = sweep_probe("generic", name, D, Rs=(1, 8))
    spec = spec_of(name, D)
    for o in orientations(name, D):
        got = ops.k_dense(spec, T(o.P), T(o.Q[o.cols]))
        worst = max(worst, check("generic", name, D, o, got, 8, F64, what="k_dense"))
    report("generic", f"{name} D={D}", worst)


# ---------------------------------------------------------------- k_dense
@pytest.mark.parametrize("form", ["default", "kdense_ta16", "kdense_ta64"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_k_dense(dtype, form, monkeypatch):
    from cggp import ops
    env = {} if form == "default" else next(r for r in sf.FORMS if r["id"] == form)["env"]
    n_range = 1 << 15 if dtype == F64 else 1 << 12
    with sf.switched(monkeypatch, env):
        for name in pr.KINDS:
            worst = 0.0
            for D in DIMS:
                spec = spec_of(name, D)
                for o in orientations(name, D, dtype, n_range):
                    got = ops.k_dense(spec, T(o.P, dtype), T(o.Q[o.cols], dtype))
                    worst = max(worst, check(f"k_dense[{form}]", name, D, o, got, 8, dtype))
            report(f"k_dense[{form}]", f"{name} {np.dtype(dtype).name}", worst)


# ---------------------------------------------------------------- products of two values
def _single_row_case(name, D):
    """x = the origin, Z = every fourth row of a 4096-point range set: k(x, z_j) steps through the whole range (the
    output is M x M, so M stays at 1024)."""
    X, Zr, ls, _ = pr.range_set(name, D, 1 << 12)
    Z = X[::4]
    x = Zr[:1]
    pv = pr.pair_values(name, VAR, ls, Z, x)
    rel = pr.pair_bound(name, VAR, pv.s, pv.q, pr.scaled(name, ls, Z), pr.scaled(name, ls, x), D, F64)
    return x, Z, pv, rel


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
@pytest.mark.parametrize("form", ["two_stage", "contract_fused"])
def test_kmn_knm_single_row(form, name, D, monkeypatch):
    """K_mn K_nm with N = 1: out[i, j] = k_i k_j.  The default handle takes kmn_knm_two_stage (kernel values from
    k_dense, contracted by the syrk); the `contract_fused` row of tests/switch_forms.py takes kmn_knm_kernel of
    contract.hip, which evaluates mgp_profile on its own expansion chain and feeds the MFMA.  Bound: the two relative
    bounds plus u for the product; the floor rule with variance^2."""
    from cggp import ops
    env = {} if form == "two_stage" else next(r for r in sf.FORMS if r["id"] == form)["env"]
    x, Z, pv, rel = _single_row_case(name, D)
    with sf.switched(monkeypatch, env):
        got = ops.kmn_knm(spec_of(name, D), T(x), T(Z)).cpu().numpy()
    k = pv.k[:, 0]
    prod = pr.PairValues(k[:, None] * k[None, :], np.maximum(pv.s, pv.s.T), np.maximum(pv.q, pv.q.T))
    rel2 = rel + rel.T + U64
    report(f"kmn_knm[{form}]", f"{name} D={D}",
           pr.check_pairs(f"kmn_knm[{form}] N=1 {name} D={D} range", got, prod, rel2, VAR * VAR, F64))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_kmn_sq_colsum_single_row(name, D):
    """The squared-value instantiation of the LDS-tile sweep with N = 1, x the origin, Z the whole 2^15-point range
    set (every entry of its 2048-entry table): out[j] = k_j^2."""
    from cggp import ops
    o = orientations(name, D)[0]  # k(range X, origin) is its first column
    got = ops.kmn_sq_colsum(spec_of(name, D), T(o.Q[:1]), T(o.P)).cpu().numpy()[:, None]
    pv, rel = o.pv.columns(1), o.rel[:, :1]
    sq = pr.PairValues(pv.k * pv.k, pv.s, pv.q)
    report("kmn_sq_colsum", f"{name} D={D}",
           pr.check_pairs(f"kmn_sq_colsum N=1 {name} D={D} range", got, sq, 2.0 * rel + U64, VAR * VAR, F64))


# ---------------------------------------------------------------- k(X, X)
_KXX = {}


def _kxx_case(name, D):
    if (name, D) not in _KXX:
        X, _, ls, _ = pr.range_set(name, D, 1 << 16)
        cols = [0, X.shape[0] // 2]  # the origin, and a point with tau ~ 3
        pv = pr.pair_values(name, VAR, ls, X, X, cols)
        a = pr.scaled(name, ls, X)
        _KXX[(name, D)] = (X, cols, pv, pr.pair_bound(name, VAR, pv.s, pv.q, a, a[cols], D, F64))
    return _KXX[(name, D)]


@pytest.mark.parametrize("name", pr.KINDS)
@pytest.mark.parametrize("form", ["pair", "plain"])
def test_kxx_matvec(form, name, monkeypatch):
    """N = 2^16 with one column: the symmetric pair kernel of kxx.hip on the default handle, the self-sweep under
    MGP_KXX=plain.  out = K[:, j] + s2 e_j with s2 = 0.25: the diagonal entry has s2 taken off again here, and 2u added
    to its bound for the sum and the difference."""
    from cggp import ops
    s2 = 0.25
    with sf.switched(monkeypatch, {} if form == "pair" else {"MGP_KXX": "plain"}):
        for D in DIMS:
            X, cols, pv, rel = _kxx_case(name, D)
            Xt = T(X)
            worst = 0.0
            for c, j in enumerate(cols):
                V = np.zeros((X.shape[0], 1))
                V[j, 0] = 1.0
                got = ops.kxx_matvec(spec_of(name, D), Xt, s2, T(V)).cpu().numpy()
                got[j, 0] -= s2
                relc = rel[:, c:c + 1].copy()
                relc[j, 0] += 2.0 * U64 * (VAR + s2) / VAR
                one = pr.PairValues(pv.k[:, c:c + 1], pv.s[:, c:c + 1], pv.q[:, c:c + 1])
                worst = max(worst, pr.check_pairs(f"kxx_matvec[{form}] {name} D={D} range column {j}", got, one, relc, VAR,
                                                  F64, col_ids=[j]))
            report(f"kxx_matvec[{form}]", f"{name} D={D}", worst)


@pytest.mark.parametrize("name", pr.KINDS)
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_knm_project(route, name):
    """k(Xs, X) @ R with one-hot columns of R: the fused route of project.hip (D <= 32) and the generic one (D = 33)."""
    from cggp import ops
    for D in (DIMS if route == "fused" else (33,)):
        worst = 0.0
        for o in orientations(name, D):
            for layout in (ops.COLS, ops.ROWS):
                V = o.one_hot(8)
                _, proj = ops.knm_project(spec_of(name, D), T(o.P), T(o.Q), T(V if layout == ops.COLS else V.T),
                                          want_proj=True, r_layout=layout)
                worst = max(worst, check(f"knm_project[{route}]", name, D, o, proj, 8, F64))
        report(f"knm_project[{route}]", f"{name} D={D}", worst)


@pytest.mark.parametrize("name", pr.KINDS)
def test_kxx_pivchol_first_row(name):
    """max_rank = 1: the factor row is K[p, :] / sqrt(variance); 2u on top of the bound for the square root and the
    quotient."""
    from cggp import ops
    for D in DIMS:
        X, _, ls, _ = pr.range_set(name, D, 1 << 15)
        L, piv, _ = ops.kxx_pivchol(spec_of(name, D), T(X), 1)
        p = int(piv[0])
        pv = pr.pair_values(name, VAR, ls, X, X, [p])
        a = pr.scaled(name, ls, X)
        rel = pr.pair_bound(name, VAR, pv.s, pv.q, a, a[[p]], D, F64)
        root = np.sqrt(LD(VAR))
        row = pr.PairValues(pv.k / root, pv.s, pv.q)
        worst = pr.check_pairs(f"kxx_pivchol {name} D={D} range pivot {p}", L.cpu().numpy().T, row, rel, float(root), F64,
                               extra_rel=2.0 * U64, col_ids=[p])
        report("kxx_pivchol", f"{name} D={D}", worst)


# ---------------------------------------------------------------- derivatives of a single pair
GRAD_BAR = 1e-10  # of |term|: tests/test_gpu_sgpr_train.py::test_kmn_knm_vjp_against_long_double


def _grad_case(name, D, count=16):
    """Z = 256 rows of a range set (the origin first), x = the origin, and the probed rows: those whose distance part
    of the bound is below 1e-12 (so the bar is about the profile, not about cancellation) and whose value is above the
    flush floor, `count` of them spread over tau."""
    X, Zr, ls, _ = pr.range_set(name, D, 1 << 12)
    Z = X[::16]
    x = Zr[:1]
    pv = pr.pair_values(name, VAR, ls, x, Z, derivs=True)  # [1, 256(, D)]; dk_dz is the derivative in the rows of Z
    ds = pr.distance_bound(pr.scaled(name, ls, x), pr.scaled(name, ls, Z), D, F64)[0]
    q = pv.q[0].astype(F64)
    dist_part = np.log(2.0) * (ds if name == "se" else np.minimum(ds / q, np.sqrt(ds)))
    ok = np.flatnonzero((dist_part < 1e-12) & (pv.k[0] > LD(VAR) * LD(2) ** -900))
    assert ok.size >= count
    return x, Z, ls, pv, [int(ok[i]) for i in np.linspace(0, ok.size - 1, count).astype(int)]


def _hold_grad(label, got, want):
    got, want = np.asarray(got, dtype=F64), np.asarray(want)
    assert np.all(np.isfinite(got)), label
    err = np.abs(got.astype(LD) - want)
    bar = LD(GRAD_BAR) * np.abs(want)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, LD(1)), np.where(err > 0, LD(np.inf), LD(0))).astype(F64)
    assert np.all(err <= bar), f"{label}: got {got.tolist()}, want {want.astype(F64).tolist()}, err / bar {ratio.tolist()}"
    return float(ratio.max())


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_kxx_grad_single_pair(name, D):
    """kxx_grad with U = e_i, V = e_0: d k(x_i, x_0) / d(variance, l_d)."""
    from cggp import ops
    _, Z, _, pv, rows = _grad_case(name, D)
    Zt = T(Z)
    worst = 0.0
    for i in rows:
        U, V = np.zeros((Z.shape[0], 1)), np.zeros((Z.shape[0], 1))
        U[i, 0], V[0, 0] = 1.0, 1.0
        dv, dl = ops.kxx_grad(spec_of(name, D), Zt, T(U), T(V))
        label = f"kxx_grad {name} D={D} range pair ({i}, 0) s* = {float(pv.s[0, i]):.6g}"
        worst = max(worst, _hold_grad(label + " dvariance", [dv], pv.dk_dvariance[0, [i]]),
                    _hold_grad(label + " dlengthscales", dl, pv.dk_dls[0, i]))
    print(f"pair-accuracy kxx_grad {name} D={D}: worst err / (1e-10 |term|) {worst:.2e}")


@pytest.mark.parametrize("D", DIMS + (33, 77))
@pytest.mark.parametrize("name", pr.KINDS)
def test_k_dense_vjp_single_pair(name, D):
    """k_dense_vjp with a one-hot G (grad.hip; generic.hip above D = 32)."""
    from cggp import ops
    x, Z, _, pv, rows = _grad_case(name, D)
    xt, Zt = T(x), T(Z)
    worst = 0.0
    for i in rows:
        G = np.zeros((1, Z.shape[0]))
        G[0, i] = 1.0
        dv, dl = ops.k_dense_vjp(spec_of(name, D), xt, Zt, T(G))
        dv2, dl2 = ops.k_dense_vjp(spec_of(name, D), Zt, xt, T(G.T))
        label = f"k_dense_vjp {name} D={D} range pair (0, {i}) s* = {float(pv.s[0, i]):.6g}"
        for tag, a, b in (("", dv, dl), (" transposed", dv2, dl2)):
            worst = max(worst, _hold_grad(label + tag + " dvariance", [a], pv.dk_dvariance[0, [i]]),
                        _hold_grad(label + tag + " dlengthscales", b, pv.dk_dls[0, i]))
    print(f"pair-accuracy k_dense_vjp {name} D={D}: worst err / (1e-10 |term|) {worst:.2e}")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_kmn_knm_vjp_single_pair(name, D):
    """kmn_knm_vjp with N = 1, Gq = 0, Y = 1 and a one-hot Gb: W = e_m^T, so the result is the derivative of
    k(x, z_m) in variance, l_d and z_m; the other rows of dZ are exact zeros."""
    from cggp import ops
    x, Z, _, pv, rows = _grad_case(name, D)
    M = Z.shape[0]
    xt, Zt, Gq, Y = T(x), T(Z), T(np.zeros((M, M))), T(np.ones((1, 1)))
    worst = 0.0
    for m in rows:
        Gb = np.zeros((M, 1))
        Gb[m, 0] = 1.0
        dv, dl, dZ = ops.kmn_knm_vjp(spec_of(name, D), xt, Zt, Gq, Y, T(Gb), need_dZ=True)
        dZ = dZ.cpu().numpy()
        label = f"kmn_knm_vjp {name} D={D} range pair (0, {m}) s* = {float(pv.s[0, m]):.6g}"
        worst = max(worst, _hold_grad(label + " dvariance", [dv], pv.dk_dvariance[0, [m]]),
                    _hold_grad(label + " dlengthscales", dl, pv.dk_dls[0, m]),
                    _hold_grad(label + " dZ", dZ[m], pv.dk_dz[0, m]))
        assert not np.any(np.delete(dZ, m, axis=0)), label
    print(f"pair-accuracy kmn_knm_vjp {name} D={D}: worst err / (1e-10 |term|) {worst:.2e}")
