"""Nearest-centre assignment and cluster sums held to a high-precision reference: the rule an index vector must obey, the
bounds that rule is made of, the point sets and case tables of tests/test_assign_reference.py (CPU) and
tests/test_gpu_assign.py (MI355X).

Reference.  s*[i, j] is the quantity `nearest_kernel` (csrc/cluster.hip) and `nearest_generic_kernel` (csrc/generic.hip)
minimise, from the exact values of the dtype-rounded inputs: the raw squared distance for `sqeuclidean` and `euclidean`
(types 0, 1), c_kind^2 sum_d ((x_d - z_d) / l_d)^2 for `covariance` and `correlation` (types 2, 3) -- the `s` of
`pair_reference.pair_values`, formed by its two-long-double `r2`.  Up to N M D = LD_LIMIT that is what is used; above,
float64 direct differences in row blocks, whose own error (one rounding per difference, doubled by the square, one per
square, D - 1 in the sum: (D + 2) u64 s*; with lengthscales the division and the product with c^2 add four) is added
to every margin below.

Bound b[i, j] on the device's s.
* Expansion form (types 0, 2, 3): `pair_reference.distance_bound(a, b, D, dtype)` = (D + 6) u sum_d (|a_d| + |b_d|)^2 on
  the coordinates as the kernel scales them (raw for type 0, x c / l otherwise).  That bound was derived for the sweeps:
  two roundings per scaled coordinate, three fma chains of D steps (|a|^2, |b|^2, the cross term) and two joins.
  `nearest_kernel` has the same two roundings per coordinate, the same two norm chains, ONE join (|b|^2 + |a|^2) and
  the cross chain of D fmas started from it (the doubling of b is exact); `nearest_generic_kernel` has the norm chains of
  `row_sqnorm_kernel`, a D-step fma chain for a.b (the zero padding to 16 is exact) and two joins (fma(-2, a.b, |b|^2),
  then + |a|^2).  Neither has more roundings than the sweep; with raw inputs (scale 1) the coordinates carry none.
* Direct form (type 1): df_d = fl(a_d - b_d) = (a_d - b_d)(1 + e), |e| <= u, so df_d^2 is within (2u + u^2) of
  (a_d - b_d)^2; the D fmas s <- fl(df_d^2 + s) round D prefixes, each at most the final sum.  Every term is a relative
  error of a non-negative quantity, so |s - s*| <= gamma(D + 2) s*, gamma(n) = n u / (1 - n u): exactly 0 for coincident
  rows (every df is an exact 0), for both kernels.

Rule for idx (every row, nothing left out):
1. 0 <= idx[i] < M.
2. s*[i, idx[i]] - b[i, idx[i]] <= min_j (s*[i, j] + b[i, j]): no correct evaluation can prefer another centre by more.
   Where a single j satisfies it (a decided row) the index is pinned exactly.  Bitwise copies of a centre count as one
   candidate here (rule 3 decides among them); the share of undecided rows is capped at UNDECIDED_CAP so that rule 2
   cannot pass vacuously.
3. If a row of Z is a bitwise copy of a row with a lower index, idx never names the copy: equal inputs go through the
   same arithmetic to the same bits, both kernels keep a candidate only on a strict '<' while j ascends, and the generic
   kernel merges its 16 column groups by (value, index).  No tolerance.

Rule for best at the chosen pair (j = idx[i]; ds = b[i, j], u of the dtype):
* type 0: |best - s*| <= ds.
* type 1: best = fl(sqrt(max(s, 0))): |sqrt(s) - sqrt(s*)| <= ds / sqrt(s*) and <= sqrt(ds) (as `pair_bound` argues for
  q), the root itself is granted 2u: |best - sqrt(s*)| <= min(ds / sqrt(s*), sqrt(ds)) + 2u sqrt(s*); 0 where s* = 0.
* types 2, 3: rho = mgp_profile(-s) = k / variance is within rel rho* of rho* = f(s*), rel = `pair_reference.value_bound`
  (the value part of `pair_bound`) at ds.  correlation = fl(1 - rho): one more rounding,
      e3 = rel rho* + u (|1 - rho*| + rel rho*).
  covariance = fl(fl(2 variance) fl(1 - rho)): the variance is rounded to the dtype (the factor 2 is exact) and the
  product rounds once, two relative errors u on a value of at most 2 variance (|1 - rho*| + e3):
      e2 = 2 variance (e3 + 2u (|1 - rho*| + e3)).
  No tuned constant.

Cluster sums: long-double sum of y per cluster and column, exact integer counts; any order of the n_c - 1 additions of
a cluster's members (adding the exact zeros of the other rows, lanes or chunks rounds nothing) stays within
gamma(n_c) sum_{i in c} |y_i|.
"""

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pair_reference as pr

LD = np.longdouble
TYPES = ("sqeuclidean", "euclidean", "covariance", "correlation")
VARIANCE = pr.VARIANCE
LD_LIMIT = 4e6  # N M D up to which the reference is long double
BLOCK_ELEMS = 2e5  # n M D of one row block: its temporaries stay in cache
UNDECIDED_CAP = 0.03
U64 = 2.0 ** -53
WORKERS = min(8, os.cpu_count() or 1)  # threads over the row blocks of a long-double case
MI355X_CUS = 256  # what the CPU tests size the rows-per-thread cases with; the GPU tests read the device


def gamma(n, u):
    n = np.asarray(n, dtype=np.float64)
    return n * u / (1.0 - n * u)


# ---------------------------------------------------------------- reference distances and their bound
class _Setup:
    def __init__(self, dist_type, kind, ls, X, Z):
        X, Z = np.asarray(X), np.asarray(Z)
        assert X.dtype == Z.dtype and X.dtype in (np.float32, np.float64) and X.ndim == 2 and Z.ndim == 2
        self.dist_type, self.kind, self.dtype = dist_type, kind, X.dtype
        self.N, self.D = X.shape
        self.M = Z.shape[0]
        self.u = pr.unit_roundoff(self.dtype)
        self.raw = dist_type <= 1
        self.ls = np.ones(self.D) if self.raw else np.asarray(ls, dtype=np.float64).reshape(-1)
        self.c2 = LD(1) if self.raw else pr.profile_scale(kind) ** 2
        self.exact = float(self.N) * self.M * self.D <= LD_LIMIT
        self.ref_rel = 0.0 if self.exact else (self.D + (2 if self.raw else 6)) * U64
        self.X64, self.Z64 = X.astype(np.float64), Z.astype(np.float64)
        if self.exact:
            self.XL, self.ZL, self.lsL = X.astype(LD), Z.astype(LD), self.ls.astype(LD)
        if dist_type != 1:
            self.a = self.X64 if self.raw else pr.scaled(kind, self.ls, self.X64)
            self.b = self.Z64 if self.raw else pr.scaled(kind, self.ls, self.Z64)
        self.rows_per = max(1, int(BLOCK_ELEMS // (self.M * (self.D if self.exact else 4))))

    def block(self, i0, i1):
        """s* [n, M] (long double, or float64 above LD_LIMIT) and its bound [n, M] (float64) for rows i0 .. i1."""
        if self.exact:
            hi, _, _ = pr.r2(self.XL[i0:i1], self.ZL, self.lsL)
            s = self.c2 * hi
        else:
            s = np.zeros((i1 - i0, self.M))
            for d in range(self.D):
                w = self.X64[i0:i1, d, None] - self.Z64[None, :, d]
                if not self.raw:
                    w /= self.ls[d]
                w *= w
                s += w
            if not self.raw:
                s *= float(self.c2)
        s64 = s.astype(np.float64)
        if self.dist_type == 1:
            bound = gamma(self.D + 2, self.u) * s64
        else:
            bound = pr.distance_bound(self.a[i0:i1], self.b, self.D, self.dtype)
        return s, bound + self.ref_rel * s64


def distances(dist_type, kind, ls, X, Z, rows=None):
    """(s*, bound) [n, M] for all rows, or for `rows` = (i0, i1)."""
    st = _Setup(dist_type, kind, ls, X, Z)
    return st.block(*(rows or (0, st.N)))


def first_occurrence(Z):
    """first[j] = the lowest index whose row has the bits of row j."""
    Z = np.ascontiguousarray(Z)
    bits = Z.view(np.uint64 if Z.dtype == np.float64 else np.uint32)
    _, start, inverse = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    return start[np.asarray(inverse).reshape(-1)]


class Report:
    """undecided_share; ref_idx (first-index argmin of s*); decided [N]; best_ratio (worst err / bound of `best`, None
    without one); s_chosen, b_chosen [N]."""


def check_assignment(label, dist_type, kind, variance, ls, X, Z, idx=None, best=None):
    """Hold idx [N] (and best [N]) to the rules of the module docstring; idx = None checks the reference's own first-index
    argmin, which gives the undecided share of a planned case without a device.  Raises AssertionError naming the worst
    row; returns a Report."""
    st = _Setup(dist_type, kind, ls, X, Z)
    N, M = st.N, st.M
    own = idx is None
    if not own:
        idx = np.asarray(idx)
        assert idx.shape == (N,) and idx.dtype == np.int64, (label, idx.shape, idx.dtype)
        bad = np.flatnonzero((idx < 0) | (idx >= M))
        assert bad.size == 0, f"{label}: rule 1: {bad.size} of {N} indices outside [0, {M}); first row {bad[0]}: {idx[bad[0]]}"
    first = first_occurrence(Z)
    distinct = first == np.arange(M)
    if not own:
        bad = np.flatnonzero(~distinct[idx])
        assert bad.size == 0, (f"{label}: rule 3: {bad.size} of {N} rows name a copy of a lower-indexed centre; first row "
                               f"{bad[0]}: idx {idx[bad[0]]} is a copy of {first[idx[bad[0]]]}")
    rep = Report()
    rep.ref_idx = np.empty(N, dtype=np.int64)
    rep.decided = np.empty(N, dtype=bool)
    rep.s_chosen = np.empty(N, dtype=LD)
    rep.b_chosen = np.empty(N, dtype=np.float64)
    passed = np.empty(N, dtype=bool)
    excess = np.zeros(N, dtype=np.float64)

    def work(i0):  # row blocks are independent and write disjoint slices; numpy releases the GIL inside its loops
        i1 = min(N, i0 + st.rows_per)
        s, bound = st.block(i0, i1)
        ar = np.arange(i1 - i0)
        rep.ref_idx[i0:i1] = np.argmin(s, axis=1)
        j = rep.ref_idx[i0:i1] if own else idx[i0:i1]
        low = s - bound
        up = (s + bound).min(axis=1)
        cand = low <= up[:, None]
        rep.decided[i0:i1] = (cand & distinct[None, :]).sum(axis=1) == 1
        passed[i0:i1] = cand[ar, j]
        excess[i0:i1] = (low[ar, j] - up).astype(np.float64)
        rep.s_chosen[i0:i1] = s[ar, j]
        rep.b_chosen[i0:i1] = bound[ar, j]

    if st.exact:  # long double is compute-bound and gains from threads; the float64 blocks are memory-bound and do not
        with ThreadPoolExecutor(max_workers=WORKERS) as pool:
            list(pool.map(work, range(0, N, st.rows_per)))
    else:
        for i0 in range(0, N, st.rows_per):
            work(i0)
    if not passed.all():
        bad = np.flatnonzero(~passed)
        w = bad[np.argmax(excess[bad])]
        raise AssertionError(
            f"{label}: rule 2: {bad.size} of {N} rows chose a centre that no correct evaluation can prefer; worst row {w}: "
            f"idx {(rep.ref_idx if own else idx)[w]} with s* = {float(rep.s_chosen[w]):.17g} (bound {rep.b_chosen[w]:.3e}), "
            f"the reference's is {rep.ref_idx[w]}, past the limit by {excess[w]:.3e}")
    rep.undecided_share = float(np.mean(~rep.decided)) if N else 0.0
    assert rep.undecided_share <= UNDECIDED_CAP, \
        f"{label}: {rep.undecided_share:.2%} of the rows are undecided: rule 2 would check too little"
    rep.best_ratio = None
    if best is not None:
        rep.best_ratio = _check_best(label, st, variance, rep, np.asarray(best))
    return rep


def _check_best(label, st, variance, rep, best):
    assert best.shape == (st.N,) and best.dtype == st.dtype, (label, best.shape, best.dtype)
    assert np.all(np.isfinite(best)), f"{label}: non-finite best at rows {np.flatnonzero(~np.isfinite(best))[:4].tolist()}"
    u, s, ds = st.u, rep.s_chosen, rep.b_chosen
    s64 = s.astype(np.float64)
    if st.dist_type == 0:
        want, bound = s, ds.astype(LD)
    elif st.dist_type == 1:
        root = np.sqrt(s)
        r64 = root.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            dq = np.where(s64 > 0, np.minimum(ds / r64, np.sqrt(ds)), 0.0)
        want, bound = root, (dq + 2.0 * u * r64).astype(LD)
        zero = s == 0
        assert np.all(best[zero] == 0), f"{label}: coincident rows must give exactly 0: {best[zero][best[zero] != 0][:4]}"
    else:
        rho = pr.k_over_variance(st.kind, s / st.c2, np.zeros_like(s))
        q = np.sqrt(np.maximum(s, st.c2 * pr.R2_FLOOR)).astype(np.float64)
        rel = pr.value_bound(st.kind, ds, q, st.dtype)
        rho64 = rho.astype(np.float64)
        gap = np.abs(1.0 - rho64)
        e3 = rel * rho64 + u * (gap + rel * rho64)
        if st.dist_type == 3:
            want, bound = LD(1) - rho, e3.astype(LD)
        else:
            want = LD(2) * LD(variance) * (LD(1) - rho)
            bound = (2.0 * variance * (e3 + 2.0 * u * (gap + e3))).astype(LD)
    err = np.abs(best.astype(LD) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, LD(1)), np.where(err > 0, LD(np.inf), LD(0)))
    if np.any(err > bound):
        w = int(np.argmax(ratio))
        raise AssertionError(
            f"{label}: best: {int((err > bound).sum())} of {st.N} rows outside the bound; worst row {w}: got "
            f"{float(best[w]):.17e}, want {float(want[w]):.17e}, err {float(err[w]):.3e}, bound {float(bound[w]):.3e}")
    return float(ratio.max()) if ratio.size else 0.0


def check_cluster_sums(label, idx, Y, M, sums, counts):
    """sums [M, C] and counts [M] of Y [N, C] per cluster against the long-double sums: counts exactly, sums within
    gamma(n_c) sum |y|.  Returns the worst err / bound."""
    idx, Y, sums, counts = np.asarray(idx), np.asarray(Y), np.asarray(sums), np.asarray(counts)
    Y = Y.reshape(Y.shape[0], -1)
    sums = sums.reshape(M, -1)
    assert sums.shape == (M, Y.shape[1]) and counts.shape == (M,), (label, sums.shape, counts.shape)
    n = np.bincount(idx, minlength=M)
    bad = np.flatnonzero(counts.astype(np.int64) != n)
    assert bad.size == 0 and np.all(counts == np.floor(counts)), \
        f"{label}: {bad.size} counts differ; first cluster {bad[:1]}: {counts[bad[:1]]} for {n[bad[:1]]}"
    ref = np.zeros((M, Y.shape[1]), dtype=LD)
    mass = np.zeros((M, Y.shape[1]), dtype=np.float64)
    np.add.at(ref, idx, Y.astype(LD))
    np.add.at(mass, idx, np.abs(Y.astype(np.float64)))
    bound = gamma(n, pr.unit_roundoff(Y.dtype))[:, None] * mass
    err = np.abs(sums.astype(LD) - ref).astype(np.float64)
    if np.any(err > bound):
        c, col = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        raise AssertionError(f"{label}: {int((err > bound).sum())} sums outside the bound; cluster {c} column {col} ({n[c]} "
                             f"rows): got {float(sums[c, col]):.17e}, want {float(ref[c, col]):.17e}, bound {bound[c, col]:.3e}")
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------- point sets
SETS = ("cloud", "coincident", "duplicated")
TIE_PATTERNS = ("+1", "+16", "+64", "+150", "stack")
TIE_M = 200


def point_set(label, D, N, M, dtype, seed=0):
    """Standard-normal clouds X [N, D], Z [M, D]; "coincident": Z[:5] = X[:5]; "duplicated": the upper half of Z is a
    copy of the lower."""
    rng = np.random.default_rng([seed, 11, SETS.index(label), D, N, M])
    X, Z = rng.standard_normal((N, D)).astype(dtype), rng.standard_normal((M, D)).astype(dtype)
    if label == "coincident":
        k = min(5, N, M)
        Z[:k] = X[:k]
    elif label == "duplicated":
        Z[M - M // 2:] = Z[:M // 2]
    return X, Z


def tie_set(pattern, D, N, dtype, seed=0):
    """Z [200, D] (or [400, D] for "stack") with copies of 20 of the first 40 centres placed `pattern` further on -- the next
    column, the same column group of the generic kernel (+16), a later tile of the generic (+64) and of either kernel
    (+150) -- or the whole of vstack([Z, Z]); the first 40 rows of X sit on the copied centres, so their two distances
    are the same bits."""
    rng = np.random.default_rng([seed, 12, TIE_PATTERNS.index(pattern), D, N])
    X, Z = rng.standard_normal((N, D)).astype(dtype), rng.standard_normal((TIE_M, D)).astype(dtype)
    src = np.arange(0, 40, 2) if pattern == "+1" else np.r_[0:16, 32:36]  # 20 centres that no copy lands on
    if pattern == "stack":
        Z = np.vstack([Z, Z])
    else:
        Z[src + int(pattern)] = Z[src]
    k = min(N, 40)
    X[:k] = Z[np.resize(src, k)]
    return X, Z


# ---------------------------------------------------------------- case tables
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.id = (f"{TYPES[self.dist_type]}-{self.kind}-D{self.D}-N{self.N}-M{self.M}-{np.dtype(self.dtype).name}-"
                   f"{self.points}" + ("" if self.want_best else "-nobest"))

    def inputs(self):
        X, Z = point_set(self.points, self.D, self.N, self.M, self.dtype)
        return X, Z, pr.lengthscales(self.D)


def _covering(Ds, Ns, Ms, reps, seed):
    """Every D x dtype x distance type, `reps` times; the (N, M) pairs are dealt from shuffled decks of all of them, the
    kinds rotate so that each D meets all four on types 2 and 3, point sets and the NULL `best` rotate too."""
    rng = np.random.default_rng(seed)
    pairs = [(n, m) for n in Ns for m in Ms]
    deck, cases, c = [], [], 0
    for iD, D in enumerate(Ds):
        for it, dtype in enumerate((np.float64, np.float32)):
            for t in range(4):
                for rep in range(reps):
                    if not deck:
                        deck = [pairs[i] for i in rng.permutation(len(pairs))]
                    N, M = deck.pop()
                    cases.append(Case(dist_type=t, kind=pr.KINDS[(iD + t + 2 * rep + it) % 4], D=D, N=N, M=M, dtype=dtype,
                                      points=SETS[c % 3], want_best=c % 4 != 3))
                    c += 1
    return cases


FUSED_DS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)  # every rung of mgp_with_dp at its top and one past it
FUSED_NS = (1, 255, 257, 4097)
FUSED_MS = (1, 127, 128, 129, 300)  # one tile of 128 centres, the tile edge, three tiles
GENERIC_DS = (33, 40, 77)
GENERIC_NS = (1, 63, 65, 777)
GENERIC_MS = (1, 15, 17, 63, 64, 65, 130)


def fused_cases():
    return _covering(FUSED_DS, FUSED_NS, FUSED_MS, 2, 1)  # 160 cases, each (N, M) pair 8 times


def generic_cases():
    return _covering(GENERIC_DS, GENERIC_NS, GENERIC_MS, 4, 2)  # 96 cases, each (N, M) pair 3 or 4 times


def rows_per_thread(N, D, cus):
    """`nearest_t` (csrc/cluster.hip): rpt = D <= 8 ? 4 : 2, halved while ceil(N / (256 rpt)) < 2 CUs."""
    rpt = 4 if D <= 8 else 2
    while rpt > 1 and -(-N // (256 * rpt)) < 2 * cus:
        rpt >>= 1
    return rpt


def rpt_cases(cus):
    """The rows-per-thread instantiations: N just over each threshold of `nearest_t` (+ 37: the last block's strided rows
    run past N) and one block of rows under it: every (dtype, padded D, rows per thread, direct / expansion) that
    `nearest_t` can launch with more than one row per thread.  Each case carries the rows per thread it must take."""
    n4, n2 = 2 * cus * 1024 + 37, 2 * cus * 512 + 37
    at = [(D, n4, 4) for D in (2, 3, 8)] + [(D, n2, 2) for D in (3, 8)] + [(D, n2, 2) for D in (9, 16, 17, 32)]
    cases, c = [], 0
    for D, N, rpt in at:
        for dtype in (np.float64, np.float32):
            for t in (1, (0, 2, 3)[c % 3]):  # the direct and the expansion instantiation; the epilogues rotate
                cases.append(Case(dist_type=t, kind=pr.KINDS[c % 4], D=D, N=N, M=37, dtype=dtype, points="cloud",
                                  want_best=True, rpt=rpt))
                c += 1
    below = [(8, n4 - 2 * 1024, 2), (3, n2 - 2 * 512, 1), (17, n2 - 2 * 512, 1)]
    for D, N, rpt in below:
        for dtype in (np.float64, np.float32):
            cases.append(Case(dist_type=c % 4, kind=pr.KINDS[c % 4], D=D, N=N, M=37, dtype=dtype, points="cloud",
                              want_best=True, rpt=rpt))
            c += 1
    cases.append(Case(dist_type=0, kind="matern32", D=3, N=n4, M=130, dtype=np.float32, points="coincident",
                      want_best=True, rpt=4))
    for case in cases:
        assert rows_per_thread(case.N, case.D, cus) == case.rpt, case.id
    return cases
