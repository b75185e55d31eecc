"""CG's two breakdown guards and the any-over-columns stopping rule: systems on which every comparison with `min_float`
or the threshold is decided by orders of magnitude, batches that hold columns of every lifetime, and the cases that
take them to each kernel site that repeats the guards (csrc/cg.hip: cg_update_fused_kernel, cg_update_kernel;
csrc/cg_dense1.hip: d1_tile_kernel + d1_update_kernel, d1_persist_full_kernel, d1_persist_blk_kernel; the recording
solve; the matrix-free operators and the external-z preconditioner).  Host arithmetic only (numpy; the route rules come
from cg_route_plan).  tests/test_guard_plan.py proves on the CPU that the cases can fail -- determinacy, every regime,
a mutated recurrence per guard -- and tests/test_gpu_cg_guards.py runs them against oracle/cg.py, column by column.

The matrix: A = s (2 I + U diag(1..q) U^T), U [n, q] orthonormal, q = 4: q + 1 distinct eigenvalues, so CG from zero
ends in at most q + 1 steps and 0.5 ||r||^2 falls from O(1) to rounding noise (~1e-30) in one step.

Columns (ROWS of rhs [Bt, n]; g, g2, ... seeded standard normal vectors, u_k the columns of U):
  a  g                                live for q + 1 steps, then held still by both guards
  b  0                                both guards see 0 from step 0: the column stays exactly 0.0, err exactly 0.0
  c  3e-10 g / |g|                    rz_0 = 9e-20 and p.Ap <= 6 rz_0 under the default floor: v = 0, err = 0.5 rz_0 for ever
  d  3 u_0                            an eigenvector: done after one step, frozen while the others are live
  e  2 u_1 - u_2 + w, w orthogonal to U, |w| = 1.5: done after three steps
  f  1e3 g2                           a large column beside the small ones
  g, h, i, k, l                       further generic columns (routes that take eight or nine)
  j  3e-5 g / |g|                     takes the last place under min_float = 1e-6: frozen from step 0 there, live by default
The batch order puts d first, so that a guard or a stopping rule read from column 0 freezes or stops everybody early.

Two more systems part the guards (with s = 1 the two guarded quantities cross the floor together; scales found by
search on the CPU):
  s = 1e-6 ("small"): p.Ap = O(s rz).  m: 1e-4 u_0 + 3e-7 g / |g| takes one step (p.Ap = 3e-14), which removes u_0; then
      p.Ap = 2e-20 m^2 stays under the floor with rz = 1e-14 above it -- gamma is zeroed, the beta term kept (beta = 1, p
      accumulates); t: 3e-7 g / |g| stalls from step 0 with rz_0 = 9e-14 above the floor; L: 1e3 g2 live.  A stall cannot
      end inside these cases without passing the floor at close range: while gamma = 0 the direction grows by r per step,
      p.Ap by a factor of at most 4 per step, so the way back over a band of 100 around the floor takes several steps
      inside it.  The cases therefore end in the stall; a kernel that guards gamma on rz instead of p.Ap moves m by 1e-3
      of its size there.
  s = 1e8 ("large"): x: 3e-9 g / |g| has rz_0 = 9e-18 under the floor and p.Ap from 1.8e-9 down to 8e-15 over five steps
      above it: steps are taken and the beta term is dropped at every one of them (steepest descent); L: 1e3 g2 live;
      b: zeros.
The Jacobi cases are the unit system under a similarity transform (jacobi_diagonal), the dense-preconditioner cases use
a Pinv that commutes with A (dense_pinv): every lifetime above stays what it is.
"""

from collections import namedtuple

import numpy as np

import cg_route_plan as rp

Q = 4
FLOOR = 1e-16          # the library's default min_float (reference :50)
BAR_F64 = (1e-9, 1e-6)  # the project's k-step bars: iterate (relative to the column's largest entry), 0.5 rz (relative)
FACTOR = 10.0          # determinacy: every guarded quantity is at least this factor away from what it is compared with

SCALE = {"unit": 1.0, "small": 1e-6, "large": 1e8}
COLS_BY_BT = {1: "e", 3: "cab", 6: "dbcaef", 8: "dbcaefgh", 9: "dbcaefghi"}  # batch order of the unit system


# ---------------------------------------------------------------- the systems
def basis(n):
    return np.linalg.qr(np.random.default_rng(7 * 10 ** 6 + n).standard_normal((n, Q)))[0]


def matrix(n, system="unit"):
    U = basis(n)
    A = (U * np.arange(1.0, Q + 1)) @ U.T
    A[np.diag_indices(n)] += 2.0
    return SCALE[system] * 0.5 * (A + A.T)


def _normal(n, j):
    return np.random.default_rng(8 * 10 ** 6 + 10 * n + j).standard_normal(n)


def column(name, n):
    U = basis(n)
    g = _normal(n, 0)
    if name == "a":
        return g
    if name == "b":
        return np.zeros(n)
    if name == "c":
        return 3e-10 * g / np.linalg.norm(g)
    if name == "d":
        return 3.0 * U[:, 0]
    if name == "e":
        w = _normal(n, 1)
        w -= U @ (U.T @ w)
        return 2.0 * U[:, 1] - U[:, 2] + 1.5 * w / np.linalg.norm(w)
    if name in "fL":
        return 1e3 * _normal(n, 2)
    if name in "ghikl":
        return _normal(n, 3 + "ghikl".index(name))
    if name == "j":  # live under the default floor, frozen from step 0 under min_float = 1e-6 (rz_0 = 9e-10)
        return 3e-5 * g / np.linalg.norm(g)
    if name == "m":
        return 1e-4 * U[:, 0] + 3e-7 * g / np.linalg.norm(g)
    if name == "t":
        return 3e-7 * g / np.linalg.norm(g)
    if name == "x":
        return 3e-9 * g / np.linalg.norm(g)
    raise KeyError(name)


def points(n, D=3):
    """Inputs of the matrix-free cases: uniform on [-2, 2]^D (squared-exponential kernel, variance 1, lengthscale 1)."""
    return np.random.default_rng(9 * 10 ** 6 + n).uniform(-2.0, 2.0, (n, D))


NOISE = 0.5  # the matrix-free systems: K + 0.5 I, and K + diag(lam), lam uniform on [0.5, 1.5]


def lam(n):
    return np.random.default_rng(9 * 10 ** 6 + n + 1).uniform(0.5, 1.5, n)


# ---------------------------------------------------------------- the cases
class Case(namedtuple("Case", "id family n Bt cols ks thr cap min_float pre start cycle dtype system env record note")):
    """family: fused | generic | tile | full | blk | record | matfree.  ks: fixed step counts (threshold 0); thr: the
    threshold of the stopping run (None for none) and cap its iteration cap.  pre: eye | jacobi | block | dense | lowrank; system: unit | small |
    large | kxx | kmm.  cycle None = no refresh.  env: the switches the handle is made under ({} = default route)."""

    def __repr__(self):
        return self.id

    @property
    def route(self):
        """The route-plan view of the case (tiers, modes, block sizes: cg_route_plan.Case)."""
        pre = "dense" if self.pre == "lowrank" else self.pre
        return rp.Case(self.id, self.n, self.Bt, max(self.ks), self.cycle, pre, self.start, self.dtype, self.record, "")

    @property
    def bar(self):
        if self.dtype == "f64":
            return BAR_F64
        return 4 * self.note[0], 4 * self.note[1]


def dense1_form(case):
    """The form of csrc/cg_dense1.hip a case takes on a 256-CU chip: None | tile | full | blk (cg.hip pcg_solve_t,
    cg_dense1.hip d1_persist_form, with the handle's MGP_CG_DENSE1 / MGP_CG_DENSE1_COLS)."""
    mode = int(case.env.get("MGP_CG_DENSE1", 3))
    n, nt = case.n, -(-case.n // 64)

    def full():
        r = min(8, rp.NUM_CUS // nt)
        return nt <= 32 and r >= 1 and -(-nt // r) <= 4

    def blk(bt):
        s = (nt + 2) // 3
        return nt <= 64 and s >= 6 and s * (s + 1) // 2 <= rp.NUM_CUS and (bt <= 6 or s >= 12)

    def form(bt):
        if mode < 3 or not 1024 <= n <= 8192 or not 1 <= bt <= 8:
            return None
        if mode == 3 and full():
            return "full"
        return "blk" if blk(bt) else "full" if full() else None

    if "MGP_CG_DENSE1_COLS" in case.env:
        cols = int(case.env["MGP_CG_DENSE1_COLS"])
    else:
        cols = 8 if form(8) else 6 if form(6) else 4 if n <= 4096 else 6
    if (case.system not in SCALE or mode == 0 or not 1024 <= n <= 8192 or not 1 <= case.Bt <= cols
            or case.pre not in ("eye", "jacobi") or case.cycle is not None or case.record):
        return None
    return form(case.Bt) or "tile"


def _case(id, family, n, Bt=9, cols=None, ks=(3, 7, 9), thr=1e-12, cap=50, min_float=FLOOR, pre="eye", start="zero", cycle=None,
          dtype="f64", system="unit", env=None, record=False, note=""):
    cols = COLS_BY_BT[Bt] if cols is None else cols
    assert len(cols) == Bt
    return Case(id, family, n, Bt, cols, tuple(ks), thr, cap, min_float, pre, start, cycle, dtype, system, env or {}, record,
                note)


TILE_ENV = {"MGP_CG_DENSE1": "1", "MGP_CG_DENSE1_COLS": "8"}


def _variants(family, n, Bt, **kw):
    """The case set every family gets once, at one size: other floors and the two systems that part the guards.  With a
    floor far under the rounding noise (1e-300, 0) a converged column iterates on noise, which no bar holds: those runs
    keep the columns that are live for q + 1 steps, stop at k = q, and hold the zero column at the equality 0 <= 0."""
    live = "bcafghi"[:Bt - 2]
    tag = f"{family}-{n}-{Bt}"
    out = [_case(f"{tag}-floor1e-6", family, n, Bt, cols=COLS_BY_BT[Bt][:-1] + "j", cap=12, min_float=1e-6, **kw)]
    out += [_case(f"{tag}-floor1e-300", family, n, Bt - 2, cols=live, ks=(Q,), thr=None, min_float=1e-300, **kw),
            _case(f"{tag}-floor0", family, n, Bt - 2, cols=live, ks=(Q,), thr=None, min_float=0.0, **kw)]
    for system, three, one in (("small", "mtL", "m"), ("large", "xLb", "x")):
        out += [_case(f"{tag}-{system}3", family, n, 3, cols=three, ks=(2, 5), thr=None, system=system, **kw),
                _case(f"{tag}-{system}1", family, n, 1, cols=one, ks=(2, 5), thr=None, system=system, **kw)]
    return out


CASES = []
# fused update: one size per thread-count family and two EPT values, Eye and Jacobi
for _n in (250, 513, 2049, 4097):
    for _pre in ("eye", "jacobi"):
        CASES.append(_case(f"fused-{_n}-{_pre}", "fused", _n, pre=_pre))
CASES += _variants("fused", 513, 9)
# generic update: block preconditioner (mode 0), refresh from a non-zero start (modes 1, 2), dense preconditioner with
# and without refresh (modes 3, 4, 5), the 1024-thread block.  The block preconditioner and the restarts of a refresh end the finite termination: those cases keep to the steps
# before any live column comes near the floor and have no stopping run
CASES += [_case("generic-block-512", "generic", 512, pre="block", ks=(3, 6), thr=None),
          _case("generic-refresh-257", "generic", 257, cycle=2, start="v0", thr=None),
          _case("generic-dense-333-plain", "generic", 333, 3, pre="dense"),
          _case("generic-dense-333-refresh", "generic", 333, 3, pre="dense", cycle=2, thr=None),
          _case("generic-8193-eye", "generic", 8193, ks=(3, 7))]
CASES += _variants("generic", 333, 9, pre="dense")
# two launches per iteration
for _bt in (1, 3, 6, 8):
    for _pre in ("eye", "jacobi"):
        CASES.append(_case(f"tile-1025-{_bt}-{_pre}", "tile", 1025, _bt, pre=_pre, env=TILE_ENV))
CASES += _variants("tile", 1025, 6, env=TILE_ENV)
# register-resident, full matrix
for _bt in (1, 6):
    for _pre in ("eye", "jacobi"):
        CASES.append(_case(f"full-1025-{_bt}-{_pre}", "full", 1025, _bt, pre=_pre))
CASES += _variants("full", 1025, 6)
# register-resident, super-blocks; 2113: n % 64 = 1, 34 tile rows (34 % 3 = 1)
CASES += [_case("blk-2049-1", "blk", 2049, 1), _case("blk-2049-6", "blk", 2049, 6),
          _case("blk-2113-6-jacobi", "blk", 2113, 6, pre="jacobi")]
CASES += _variants("blk", 2049, 6)
# the recording solve
CASES += [_case("record-513", "record", 513, record=True)]
CASES += _variants("record", 513, 9, record=True)
# matrix-free operators and the external-z preconditioner: they share the update kernels, not the start-up
# (their spectra are not tiny: the stopping run of the first ends at its cap with column c under the threshold from the
# start and column a far over it)
CASES += [_case("matfree-kxx-300", "matfree", 300, 3, ks=(3, 6), thr=1e-3, cap=6, system="kxx"),
          _case("matfree-kxx-300-lowrank", "matfree", 300, 3, ks=(3, 6), thr=None, system="kxx", pre="lowrank"),
          _case("matfree-kmm-300", "matfree", 300, 3, ks=(3, 6), thr=None, system="kmm"),
          _case("matfree-kxx-300-floor0", "matfree", 300, 3, ks=(3, 6), thr=None, system="kxx", min_float=0.0)]
# fp32: the floor is float32(1e-16), which post-convergence noise (~1e-11) never reaches: three steps, columns b, c, f
# among the others.  note = the distance of oracle/cg.py on float32 copies from its own float64 run, the largest over
# the columns of (iterate relative to the column's largest entry, 0.5 rz relative); the bar is four times it
F32 = [("fused", 513, 9, {}), ("generic", 512, 9, {}), ("tile", 1025, 6, TILE_ENV), ("full", 1025, 6, {}),
       ("blk", 2049, 6, {})]
F32_NOTES = {"f32-fused-513-9": (6.0e-07, 9.1e-06), "f32-generic-512-9": (1.7e-06, 1.4e-06),
             "f32-tile-1025-6": (7.0e-07, 8.0e-06), "f32-full-1025-6": (7.0e-07, 8.0e-06),
             "f32-blk-2049-6": (5.8e-07, 1.8e-06)}
CASES += [_case(f"f32-{_fam}-{_n}-{_bt}", _fam, _n, _bt, cols="bcafghikl"[:_bt], ks=(3,), thr=None, dtype="f32", env=_env,
                pre="block" if _fam == "generic" else "eye", note=F32_NOTES[f"f32-{_fam}-{_n}-{_bt}"])
          for _fam, _n, _bt, _env in F32]

FAMILIES = ("fused", "generic", "tile", "full", "blk", "record", "matfree")


# ---------------------------------------------------------------- inputs of a case
def operator_matrix(case):
    """The explicit matrix of the case's system (float64)."""
    if case.system in SCALE:
        A = matrix(case.n, case.system)
        if case.pre == "jacobi":
            h = np.sqrt(jacobi_diagonal(case.n))
            A = A * h[:, None] * h[None, :]
            A = 0.5 * (A + A.T)
        return A
    from oracle import kernels as ok
    K = ok.Kernel("se", 1.0, np.ones(3)).K(points(case.n))
    K = 0.5 * (K + K.T)
    K[np.diag_indices(case.n)] += NOISE if case.system == "kxx" else lam(case.n)
    return K


def dense_pinv(n):
    """Pinv = I / 2 + U diag(k / 4) U^T: any SPD matrix will do as z = r @ Pinv, and one that commutes with A keeps the
    q + 1 distinct eigenvalues (of Pinv A) and the eigenvectors, so the lifetimes of the columns stay what they are."""
    U = basis(n)
    P = (U * (0.25 * np.arange(1.0, Q + 1))) @ U.T
    P[np.diag_indices(n)] += 0.5
    return 0.5 * (P + P.T)


def jacobi_diagonal(n):
    """The diagonal D of the Jacobi cases, uniform on [1, 3]: their matrix is D^1/2 A D^1/2, their right-hand sides
    D^1/2 b and their preconditioner z = r / D, so that rz and p.Ap of every step -- and with them every lifetime -- are
    those of the unpreconditioned system (D^-1/2 r is its residual), while the kernels divide by a diagonal that varies."""
    return np.random.default_rng(6 * 10 ** 6 + n).uniform(1.0, 3.0, n)


def rhs(case):
    b = np.stack([column(c, case.n) for c in case.cols])
    return b * np.sqrt(jacobi_diagonal(case.n))[None, :] if case.pre == "jacobi" else b


def start(case):
    """Non-zero start: on the generic columns only (the lifetimes of b, c, d, e are those of a start from zero)."""
    v0 = np.zeros((case.Bt, case.n))
    if case.start == "v0":
        rng = np.random.default_rng(2 * 10 ** 6 + case.n)
        for j, c in enumerate(case.cols):
            w = 0.1 * rng.standard_normal(case.n)
            if c in "afghi":
                v0[j] = w * (1e3 if c == "f" else 1.0)
    return v0


def lowrank_factor(case, A, rank=8):
    """Rank-8 greedy pivoted Cholesky of K = A - NOISE I and its Woodbury factor: (L [8, n], dinv [n], B [8, n])."""
    import pivchol_reference as pr
    K = A - NOISE * np.eye(case.n)
    L, _ = pr.greedy_pivoted_cholesky(K, rank)
    B, _ = pr.woodbury_factor(L, NOISE)
    return L, np.full(case.n, 1.0 / NOISE), B


class LowRankPreconditioner:
    """z = r / D - (r B^T) B in the oracle's protocol (the arithmetic of pivchol_reference.pcg, batched)."""

    def __init__(self, dinv, B):
        self.dinv, self.B = dinv, B

    def __call__(self, vec, mat):
        z = vec * self.dinv[None, :] - (vec @ self.B.T) @ self.B
        return z, np.sum(z * vec, axis=-1, keepdims=True)


class DiagonalPreconditioner:
    """z = r / D for a given diagonal (the library's JacobiPreconditioner(diagonal=D)) in the oracle's protocol."""

    def __init__(self, diagonal):
        self.diagonal = diagonal

    def __call__(self, vec, mat):
        z = vec / self.diagonal[None, :]
        return z, np.sum(z * vec, axis=-1, keepdims=True)


def host_preconditioner(case, A):
    from oracle import cg as ocg
    if case.pre == "jacobi":
        return DiagonalPreconditioner(jacobi_diagonal(case.n))
    if case.pre == "block":
        return ocg.BlockPreconditioner(rp.block_indices(case.n))
    if case.pre == "dense":
        return ocg.DensePreconditioner(dense_pinv(case.n))
    if case.pre == "lowrank":
        _, dinv, B = lowrank_factor(case, A)
        return LowRankPreconditioner(dinv, B)
    return ocg.EyePreconditioner()


# ---------------------------------------------------------------- the recurrence, with its mutations
MUTATIONS = ("no_gamma_guard", "no_beta_guard", "guards_from_column_0", "stop_on_column_0", "lt_for_le",
             "floor_fixed_1e-16")


def recurrence(A, b, v0, thr, pre, max_it, cycle, min_float, mutation=None, dtype=np.float64):
    """cggp/conjugate_gradient.py:59-98 restated for row batches.  Unmutated it equals oracle/cg.py bit for bit
    (test_guard_plan).  Returns (v, steps, err [Bt, 1], trace, coef, last): trace[i] = (rz_old, p.Ap, 0.5 ||r||^2 before the
    step) per column, coef[i] = (gamma, beta, 0.5 rz after the step) per column, last = 0.5 ||r||^2 at the end."""
    T = np.dtype(dtype).type
    A = np.asarray(A, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    floor = T(1e-16) if mutation == "floor_fixed_1e-16" else T(min_float)
    zero, half, thr = T(0), T(0.5), T(thr)
    v = np.array(v0, dtype=dtype, copy=True)
    r = b - v @ A
    z, rz = pre(r, A)
    p = z
    i = 0
    trace, coef = [], []

    def under(x):
        m = x < floor if mutation == "lt_for_le" else x <= floor
        return np.broadcast_to(m[:1], m.shape) if mutation == "guards_from_column_0" else m

    def half_rr(r):
        return half * np.sum(np.square(r), axis=-1, keepdims=True)

    def go_on(r, i):
        over = half_rr(r) > thr
        if mutation == "stop_on_column_0":
            over = over[:1]
        return bool(np.any(over)) and i < max_it

    while go_on(r, i):
        pA = p @ A
        denom = np.sum(p * pA, axis=-1, keepdims=True)
        trace.append((rz[:, 0].copy(), denom[:, 0].copy(), half_rr(r)[:, 0]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            gamma = rz / denom
        if mutation != "no_gamma_guard":
            gamma = np.where(under(denom), zero, gamma)
        with np.errstate(invalid="ignore", over="ignore"):
            v = v + gamma * p
            reset = (i % cycle) == (cycle - 1)
            r = b - v @ A if reset else r - gamma * pA
            z, new_rz = pre(r, A)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            z_update = p * new_rz / rz
            beta = new_rz / rz
        if mutation != "no_beta_guard":
            z_update = np.where(under(rz), zero, z_update)
            beta = np.where(under(rz), zero, beta)
        with np.errstate(invalid="ignore", over="ignore"):
            p = z if reset else z + z_update
        coef.append(np.concatenate([gamma, zero * beta if reset else beta, half * new_rz], axis=1))
        rz = new_rz
        i += 1
    return v, i, half * rz, trace, np.array(coef, dtype=dtype).reshape(i, b.shape[0], 3), half_rr(r)[:, 0]


def run(case, k=None, mutation=None, dtype=np.float64, A=None):
    """The case on the host: k fixed steps at threshold 0, or (k None) the stopping run at the case's threshold."""
    A = operator_matrix(case) if A is None else A
    pre = host_preconditioner(case, A)
    cap = k if k is not None else case.cap
    cycle = case.cycle if case.cycle is not None else cap + 1
    return recurrence(A, rhs(case), start(case), 0.0 if k is not None else case.thr, pre, cap, cycle, case.min_float,
                      mutation, dtype)


def regimes(case, A=None):
    """Per column, from the unmutated trajectory of the longest fixed-step run: the step from which both guards hold
    the column to the end (None if never), and the steps with gamma zeroed / the beta term dropped alone."""
    _, steps, _, trace, _, _ = run(case, max(case.ks), A=A)
    f = case.min_float
    out = []
    for j in range(case.Bt):
        g = [trace[i][1][j] <= f for i in range(steps)]
        d = [trace[i][0][j] <= f for i in range(steps)]
        frozen = None
        for i in range(steps - 1, -1, -1):
            if not (g[i] and d[i]):
                break
            frozen = i
        out.append(dict(frozen_from=frozen, gamma_only=[i for i in range(steps) if g[i] and not d[i]],
                        beta_only=[i for i in range(steps) if d[i] and not g[i]],
                        live=[i for i in range(steps) if not g[i] and not d[i]]))
    return out


def determinate(case, A=None):
    """The worst factor between a guarded quantity and what it is compared with, over every step and column of the
    case's runs.  An exact zero counts as determinate: a zero column sums to 0.0 in every order."""
    worst = np.inf

    def gap(x, y):
        x = np.asarray(x, dtype=np.float64)
        x = x[x != 0.0]
        if x.size == 0:
            return np.inf
        if y == 0.0:
            return np.inf if np.all(x > 0) else 0.0
        with np.errstate(over="ignore"):
            return float(np.min(np.maximum(np.abs(x) / y, y / np.abs(x))))

    runs = [run(case, max(case.ks), A=A)] + ([run(case, None, A=A)] if case.thr else [])
    for q, (_, steps, err, trace, _, last) in enumerate(runs):
        for rz_old, d, hrr in trace:
            worst = min(worst, gap(rz_old, case.min_float), gap(d, case.min_float))
            if q == 1:
                worst = min(worst, gap(hrr, case.thr))
        if q == 1:  # the residual the run stopped on
            worst = min(worst, gap(last, case.thr))
    return worst


def column_distances(v, err, o_v, o_err):
    """Per column: max |v_b - o_b| / max |o_b| (0 where both are exactly zero, inf where only the oracle's is) and the
    relative distance of 0.5 rz (the same convention)."""
    v, err, o_v, o_err = (np.asarray(x, dtype=np.float64) for x in (v, err, o_v, o_err))
    dv, de = [], []
    for j in range(o_v.shape[0]):
        num, den = np.max(np.abs(v[j] - o_v[j])), np.max(np.abs(o_v[j]))
        dv.append(0.0 if num == 0.0 else np.inf if den == 0.0 or not np.isfinite(num) else num / den)
        num, den = abs(err[j, 0] - o_err[j, 0]), abs(o_err[j, 0])
        de.append(0.0 if num == 0.0 else np.inf if den == 0.0 or not np.isfinite(num) else num / den)
    return np.array(dv), np.array(de)


def f32_distance(case, A=None):
    """oracle/cg.py's arithmetic on float32 copies against its float64 run, the largest over the columns."""
    k = max(case.ks)
    v64, _, e64, _, _, _ = run(case, k, A=A)
    v32, _, e32, _, _, _ = run(case, k, dtype=np.float32, A=A)
    dv, de = column_distances(v32, e32, v64, e64)
    return float(dv.max()), float(de.max())


def killed_by(case, mutation, A=None):
    """Why a mutated recurrence fails the case, or None: a non-finite value, another step count, or a column moved by
    more than 1e3 times the bar (an exactly zero column: moved at all)."""
    for k in (max(case.ks),) + ((None,) if case.thr else ()):
        o_v, o_steps, o_err, _, _, _ = run(case, k, A=A)
        v, steps, err, _, _, _ = run(case, k, mutation, A=A)
        if steps != o_steps:
            return f"steps {steps} for {o_steps}"
        if not (np.all(np.isfinite(v)) and np.all(np.isfinite(err))):
            return "non-finite"
        dv, _ = column_distances(v, err, o_v, o_err)
        if dv.max() > 1e3 * case.bar[0]:
            return f"column {case.cols[int(dv.argmax())]} moved by {dv.max():.1e}"
    return None
