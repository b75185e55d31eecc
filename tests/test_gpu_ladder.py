"""Every fused (D <= 32) entry point on every rung of the padded-dimension ladder and every width of its column
passes, with dense multipliers (every entry normal, no zeros) against long double.

The cases are tests/ladder_plan.py's; tests/test_ladder_plan.py shows on the CPU that they reach every instantiation
the library's rules can pick.  References and bars are those of each entry point's own long-double test, imported:
`bar(kind)` on relmax for the symmetric product (tests/test_gpu_gpr.py) and the projection (tests/test_gpu_love.py),
1e-11 of the sum of |terms| for `mgp_kxx_grad` (tests/test_gpu_gpr_lml.py), 1e-10 of it for the two VJPs and 2e-4 in
fp32 (tests/test_gpu_sgpr_train.py, tests/test_gpu_training.py), and the accuracy contract of include/mgp.h inside
`test_gpu_rff.check_case`.  Every call is made twice and must return the same bits.  Each case prints its worst
error / bar; the last test prints the worst per entry point.
"""

import numpy as np
import pytest
import torch

import ladder_plan as lp
import love_reference as lr
from cggp import ops
from gpr_reference import kxx_product
from lml_reference import kxx_grad_reference
from sgpr_grad_reference import k_dense_vjp_reference, kmn_knm_vjp_reference
from test_gpu_gpr import bar, kxx_on, relmax, spec_of, sym_handle  # noqa: F401 (sym_handle: a fixture, MGP_KXX=sym)
from test_gpu_gpr_lml import KXX_GRAD_BAR
from test_gpu_love import default_handle, project_on
from test_gpu_rff import check_case
from test_gpu_sgpr_train import VJP_BAR
from test_gpu_training import DENSE_VJP_BARS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}  # entry -> [worst error / bar, its case, cases]
VAR = 1.3


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).to(DEV)


def note(case, ratio, what=""):
    w = WORST.setdefault(case.entry, [0.0, None, 0])
    w[2] += 1
    if ratio >= w[0]:
        w[0], w[1] = ratio, case.id
    print(f"ladder {case.id} DP={case.DP}{what}: worst error / bar {ratio:.2e}")


def points(case, rng, *lengths):
    """Standard-normal point sets and lengthscales of the order sqrt(D), so that kernel values between typical pairs
    are of order 0.1 on every rung and every pair carries weight in the sums."""
    D = case.D
    ls = np.linspace(0.7, 1.3, D) * np.sqrt(D)
    return [rng.standard_normal((n, D)) for n in lengths], ls


def ratios(got, ref, scale, bar_):
    got, ref, scale = (np.asarray(a, dtype=np.float64) for a in (got, ref, scale))
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / (bar_ * scale + 1e-300)))


# ---------------------------------------------------------------- mgp_kxx_matvec, the symmetric form
@pytest.mark.parametrize("case", lp.cases("kxx_matvec"), ids=repr)
def test_kxx_matvec(sym_handle, case):
    N, D, R = case.shape["N"], case.D, case.cols
    rng = np.random.default_rng([1, D, R])
    (X,), ls = points(case, rng, N)
    if case.kind != "se":
        X[N - 1] = X[0]  # distance exactly 0 between the first block and the ragged one
    V = rng.standard_normal((N, R))
    s2 = 0.37
    ref = kxx_product(case.kind, VAR, ls, X, s2, V)
    spec = spec_of(case.kind, VAR, ls, D)
    worst = 0.0
    for layout in (ops.COLS, ops.ROWS):
        Vin = T(V) if layout == ops.COLS else T(V.T)
        out = kxx_on(sym_handle, spec, T(X), s2, Vin, layout)
        assert torch.equal(out, kxx_on(sym_handle, spec, T(X), s2, Vin, layout))
        e = relmax(out if layout == ops.COLS else out.t(), ref)
        worst = max(worst, e / bar(case.kind))
    note(case, worst, f" groups {lp.kxx_cut(R)}")
    assert worst < 1.0


# ---------------------------------------------------------------- mgp_kxx_grad, the fused pair kernel
@pytest.mark.parametrize("case", lp.cases("kxx_grad"), ids=repr)
def test_kxx_grad(case):
    N, D, R = case.shape["N"], case.D, case.cols
    rng = np.random.default_rng([2, D, R])
    (X,), ls = points(case, rng, N)
    if case.kind != "se":
        X[N - 1] = X[0]
    U, V = rng.standard_normal((N, R)), rng.standard_normal((N, R))
    spec = ops.KernelSpec(case.kind, VAR, list(ls), D)
    dv, dl = ops.kxx_grad(spec, T(X), T(U), T(V))
    assert (dv, dl) == ops.kxx_grad(spec, T(X), T(U), T(V))
    assert (dv, dl) == ops.kxx_grad(spec, T(X), T(U.T), T(V.T), layout=ops.ROWS)  # the same columns, the same order
    rv, rl, sv, sl = kxx_grad_reference(case.kind, VAR, ls, X, U, V)
    worst = max(ratios(dv, rv, sv, KXX_GRAD_BAR), ratios(dl, rl, sl, KXX_GRAD_BAR))
    note(case, worst, f" passes {lp.kgrad_cut(R, case.DP, case.kind)}")
    assert worst <= 1.0


# ---------------------------------------------------------------- mgp_kmn_knm_vjp, its three forms
@pytest.mark.parametrize("case", lp.cases("kmn_knm_vjp"), ids=repr)
def test_kmn_knm_vjp(case):
    N, M, D, P = case.shape["N"], case.shape["M"], case.D, case.cols
    rng = np.random.default_rng([3, D, P, int(case.opts["gq"])])
    (X, Z), ls = points(case, rng, N, M)
    if case.kind != "se":
        X[N - 1] = Z[M - 1]  # a data row on an inducing point, in the ragged row block and the ragged column block
    Gq = rng.standard_normal((M, M)) if case.opts["gq"] else None
    Y = rng.standard_normal((N, P)) if P else None
    Gb = rng.standard_normal((M, P)) if P else None
    spec = ops.KernelSpec(case.kind, VAR, list(ls), D)
    rv, rl, rz, sv, sl, sz = kmn_knm_vjp_reference(case.kind, VAR, ls, X, Z, np.zeros((M, M)) if Gq is None else Gq,
                                                   Y, Gb)
    dev = [None if a is None else T(a) for a in (X, Z, Gq, Y, Gb)]
    worst = 0.0
    for want_dz in (True, False):
        dv, dl, dZ = ops.kmn_knm_vjp(spec, *dev, need_dZ=want_dz)
        dv2, dl2, dZ2 = ops.kmn_knm_vjp(spec, *dev, need_dZ=want_dz)
        assert dv == dv2 and dl == dl2
        worst = max(worst, ratios(dv, rv, sv, VJP_BAR), ratios(dl, rl, sl, VJP_BAR))
        if want_dz:
            assert dZ.shape == (M, D) and torch.equal(dZ, dZ2)
            worst = max(worst, ratios(dZ.cpu().numpy(), rz, sz, VJP_BAR))
        else:
            assert dZ is None and dZ2 is None
    form = lp.kvjp_form(case.opts["gq"], P)
    note(case, worst, f" {form}" + (f" passes {lp.kvjp_passes(P, case.DP, case.kind)}" if form == "rank_fused" else ""))
    assert worst <= 1.0


# ---------------------------------------------------------------- mgp_k_dense_vjp, both element types
@pytest.mark.parametrize("case", lp.cases("k_dense_vjp"), ids=repr)
def test_k_dense_vjp(case):
    na, nb, D = case.shape["na"], case.shape["nb"], case.D
    rng = np.random.default_rng([4, D])
    (A, B), ls = points(case, rng, na, nb)
    B += 0.3
    if case.kind != "se":
        B[nb - 1] = A[na - 1]
    G = rng.standard_normal((na, nb))
    spec = ops.KernelSpec(case.kind, VAR, list(ls), D)
    assert [str(d).split(".")[1] for d, _ in DENSE_VJP_BARS] == list(case.dtypes)
    worst = 0.0
    for dtype, bar_ in DENSE_VJP_BARS:
        Ad, Bd, Gd = T(A, dtype), T(B, dtype), T(G, dtype)
        dv, dl = ops.k_dense_vjp(spec, Ad, Bd, Gd)
        assert (dv, dl) == ops.k_dense_vjp(spec, Ad, Bd, Gd)
        # the reference on the values the device sees
        rv, rl, sv, sl = k_dense_vjp_reference(case.kind, VAR, ls, Ad.double().cpu().numpy(), Bd.double().cpu().numpy(),
                                               Gd.double().cpu().numpy())
        worst = max(worst, ratios(dv, rv, sv, bar_), ratios(dl, rl, sl, bar_))
    note(case, worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- mgp_knm_project, the fused route
@pytest.mark.parametrize("case", lp.cases("knm_project"), ids=repr)
def test_knm_project(case):
    B, N, D, r = case.shape["B"], case.shape["N"], case.D, case.cols
    rng = np.random.default_rng([5, D, r])
    (Xs, X), ls = points(case, rng, B, N)
    if case.kind != "se":
        Xs[B - 1] = X[N - 1]
    R = rng.standard_normal((N, r))
    ref_p, ref_s = lr.knm_project(case.kind, VAR, ls, Xs, X, R)
    layout = case.opts["layout"]
    Rd = T(R) if layout == ops.COLS else T(R.T)
    lib, h = default_handle()
    spec = spec_of(case.kind, VAR, ls, D)
    rc, proj, sq = project_on(lib, h, spec, T(Xs), T(X), Rd, layout)
    assert rc == 0, lib.mgp_last_error(h)
    rc, proj2, sq2 = project_on(lib, h, spec, T(Xs), T(X), Rd, layout)
    assert rc == 0 and torch.equal(proj, proj2) and torch.equal(sq, sq2)
    worst = max(relmax(proj, ref_p), relmax(sq, ref_s)) / bar(case.kind)
    note(case, worst, f" tile {lp.project_tile(r)} splits {case.opts['splits']}")
    assert worst < 1.0


# ---------------------------------------------------------------- mgp_rff_sample (fused route) and mgp_rff_features
@pytest.mark.parametrize("case", lp.cases("rff_sample"), ids=repr)
def test_rff_sample(case, monkeypatch):
    N, L, D, S = case.shape["N"], case.shape["L"], case.D, case.cols
    worst = 0.0
    for name in case.dtypes:
        rep = {}
        check_case(D, S, L, N, getattr(torch, name), case.opts["layout"], None, monkeypatch, seed=[6, D, S, L],
                   twice=True, report=rep, all_rows=True)  # every row: slot and block boundaries included
        worst = max(worst, rep["samples"], rep["features"])
    note(case, worst, f" chunks {case.opts['chunks']}")
    assert worst <= 1.0


def test_report_the_worst_ratios():
    """The figures of DESIGN 4.8d: the worst error / bar of every entry point over the plan's cases.  A print, filled
    by the tests above in this process: it is complete only when the whole module runs in one process (under `-k` or
    with the cases spread over workers it shows what this process ran); every case asserts its own bar."""
    for entry in lp.ENTRIES:
        if entry in WORST:
            ratio, ident, n = WORST[entry]
            print(f"ladder worst {lp.API[entry]}: {ratio:.2e} at {ident} ({n} of {len(lp.cases(entry))} cases)")
            assert ratio <= 1.0
