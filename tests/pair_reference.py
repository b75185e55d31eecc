"""Per-pair kernel values in long double, the rounding bound a device value is held to, and the point sets the
per-pair probes run on (tests/test_pair_reference.py on the CPU, tests/test_gpu_pair_accuracy.py on the GPU).

A product with a one-hot multiplier returns single kernel values k(x_i, z_j): the other terms are k * 0 = 0 and
adding zeros is exact.  `pair_values` gives the same values from the same fp64 inputs to a few 1e-19 relative
(direct differences; the exponent's argument is carried as an unevaluated sum of two long doubles, because at
r^2 ~ 1500 one long double alone leaves 1e-16 in k), and `pair_bound` the relative error a correct evaluation in the
working precision may have.  Units are those of csrc/mgp_math.h: a = x c / l, s = |a - b|^2 = c^2 r^2 with the c of
`mgp_profile_scale`, k = variance * 2^(-s) (SE) or variance * poly(q) 2^(-q), q = sqrt(s) (Matern).
"""

import numpy as np

from lml_reference import _profile

LD = np.longdouble
KINDS = ("se", "matern12", "matern32", "matern52")
VARIANCE = 1.3
FUNCTION_BUDGET = 8.0  # F, in units of u: 4.5 shifted table form (tests/test_host_math.py) + 2 Matern polynomial + 1 variance, rounded up
R2_FLOOR = LD(1e-36)  # GPflow: r = sqrt(max(r2, 1e-36))


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24


def flush_floor_log2(dtype):
    """Pairs with k* < variance * 2^floor may come back as anything in [0, variance * 2^(floor + 1)]."""
    return -990 if np.dtype(dtype) == np.float64 else -120


def profile_scale(name):
    """c of mgp_profile_scale (csrc/mgp_math.h), in long double."""
    log2e = LD(1) / np.log(LD(2))
    if name == "se":
        return np.sqrt(LD(0.5) * log2e)
    return {"matern12": LD(1), "matern32": np.sqrt(LD(3)), "matern52": np.sqrt(LD(5))}[name] * log2e


def lengthscales(D):
    return np.linspace(0.8, 1.25, D)


# ---------------------------------------------------------------- two-long-double arithmetic (error-free transforms)
_SPLITTER = LD(2) ** 32 + LD(1)  # Dekker's split of a 64-bit significand


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = _SPLITTER * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _sqrt_const(v):
    """sqrt(v) as hi + lo."""
    hi = np.sqrt(LD(v))
    p, e = _two_prod(hi, hi)
    return hi, ((LD(v) - p) - e) / (LD(2) * hi)


def r2(Xb, Zc, ls):
    """r^2 = sum_d ((x_d - z_d) / l_d)^2 as hi + lo (relative error ~2^-120), and w = (x - z) / l.  Xb [n, D], Zc [C, D]."""
    d_hi, d_lo = _two_sum(Xb[:, None, :], -Zc[None, :, :])  # exact: both are fp64 values
    q1 = d_hi / ls
    p, e = _two_prod(q1, ls)
    q2 = (((d_hi - p) - e) + d_lo) / ls
    sq, se = _two_prod(q1, q1)
    se = se + LD(2) * q1 * q2
    hi = np.zeros(sq.shape[:2], dtype=LD)
    lo = np.zeros(sq.shape[:2], dtype=LD)
    for d in range(sq.shape[2]):
        hi, err = _two_sum(hi, sq[:, :, d])
        lo = lo + (err + se[:, :, d])
    hi, lo = _two_sum(hi, lo)
    return hi, lo, q1


def k_over_variance(name, hi, lo):
    """f = k / variance at r^2 = hi + lo."""
    if name == "se":
        return np.exp(LD(-0.5) * hi) * (LD(1) - LD(0.5) * lo)
    floor = ~(hi > R2_FLOOR)
    hi = np.where(floor, R2_FLOOR, hi)
    lo = np.where(floor, LD(0), lo)
    rh = np.sqrt(hi)
    p, e = _two_prod(rh, rh)
    rl = (((hi - p) - e) + lo) / (LD(2) * rh)
    ch, cl = {"matern12": (LD(1), LD(0)), "matern32": _sqrt_const(3), "matern52": _sqrt_const(5)}[name]
    ah, ae = _two_prod(ch, rh)  # argument a = sqrt(nu') r as ah + al
    al = ae + ch * rl + cl * rh
    e0 = np.exp(-ah)
    if name == "matern12":
        return e0 * (LD(1) - al)
    if name == "matern32":
        return (LD(1) + ah) * e0 * (LD(1) - al * ah / (LD(1) + ah))  # d ln f / da = -a / (1 + a)
    poly = LD(1) + ah + ah * ah / LD(3)
    return poly * e0 * (LD(1) - al * (ah / LD(3)) * (LD(1) + ah) / poly)  # d ln f / da = -(a / 3)(1 + a) / poly


class PairValues:
    """k, s, q [n, C]; with derivs: dk_dvariance [n, C], dk_dls and dk_dz [n, C, D]."""

    def __init__(self, k, s, q, dk_dvariance=None, dk_dls=None, dk_dz=None):
        self.k, self.s, self.q = k, s, q
        self.dk_dvariance, self.dk_dls, self.dk_dz = dk_dvariance, dk_dls, dk_dz

    def columns(self, R):
        """The first R probed columns."""
        return PairValues(self.k[:, :R], self.s[:, :R], self.q[:, :R])


def pair_values(name, variance, ls, X, Z, cols=None, derivs=False, block=2048):
    """Long-double k* = k(x_i, z_j) for every row i of X and every j in `cols` (all of Z when None), from the exact
    values of the inputs (fp64, or fp32 for the fp32 probes), with the scaled squared distance s* = c^2 r^2 and the
    Matern argument q* = sqrt(max(s*, c^2 1e-36)) (for SE: sqrt(s*)).  derivs: also dk/dvariance, dk/dl_d, dk/dz_d."""
    X = np.asarray(X).astype(LD)
    Zc = np.asarray(Z).astype(LD)
    if cols is not None:
        Zc = Zc[np.asarray(cols, dtype=np.int64)]
    D = X.shape[1]
    ls = np.asarray(ls, dtype=np.float64).astype(LD).reshape(-1)
    if ls.shape[0] == 1:
        ls = np.repeat(ls, D)
    var = LD(variance)
    c2 = profile_scale(name) ** 2
    n, C = X.shape[0], Zc.shape[0]
    k, s = np.empty((n, C), dtype=LD), np.empty((n, C), dtype=LD)
    dv = np.empty((n, C), dtype=LD) if derivs else None
    dl = np.empty((n, C, D), dtype=LD) if derivs else None
    dz = np.empty((n, C, D), dtype=LD) if derivs else None
    for i0 in range(0, n, block):
        hi, lo, w = r2(X[i0:i0 + block], Zc, ls)
        f = k_over_variance(name, hi, lo)
        k[i0:i0 + block] = var * f
        s[i0:i0 + block] = c2 * hi
        if derivs:
            _, fp = _profile(name, hi)
            g = (var * LD(-2)) * fp[:, :, None] / ls
            dv[i0:i0 + block] = f
            dl[i0:i0 + block] = g * w * w
            dz[i0:i0 + block] = g * w
    q = np.sqrt(np.maximum(s, c2 * R2_FLOOR))
    return PairValues(k, s, q, dv, dl, dz)


def scaled(name, ls, P):
    """a = x c / l in fp64 (what the bound measures norms with)."""
    return np.asarray(P, dtype=np.float64) * (float(profile_scale(name)) / np.asarray(ls, dtype=np.float64))


def distance_bound(a, b, D, dtype):
    """|Delta s| <= (D + 6) u sum_d (|a_d| + |b_d|)^2, [n, C] for a [n, D], b [C, D]."""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    S = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] + 2.0 * (a @ b.T)
    return (D + 6) * unit_roundoff(dtype) * S


def pair_bound(name, variance, s, q, a, b, D, dtype):
    """Relative bound on |k - k*| / k* for a correct evaluation of k(x, z) in `dtype` arithmetic by the expansion form
    (|a|^2 + |b|^2 - 2 a.b) and a base-2 exponential: [n, C] for s, q [n, C], a [n, D], b [C, D] (scaled coordinates).
    `variance` does not enter: the bound is relative (the product with the variance is one of F's roundings).

    Derivation, to first order in u (2^-53 for fp64, 2^-24 for fp32):

    Distance.  a_d = fl(x_d fl(c / l_d)) carries two roundings, so each of a_d^2, b_d^2 and 2 a_d b_d is off by 4u of
    itself: 4u S in all, S = sum_d (|a_d| + |b_d|)^2 = |a|^2 + |b|^2 + 2 |a|.|b|.  The three sums are fma chains; a
    chain rounds each prefix once, the prefixes of the positive chains average half their final value and those of
    the cross chain stay below |b|^2 + 2|a|.|b|, so D steps give D u S, and joining the chains (the subtraction of
    |a|^2, or its fold into the magic constant, and the magic add itself) two more roundings of at most S:
        |Delta s| <= (D + 6) u S.
    SE.  k = variance 2^(-s): |Delta k| / k <= ln2 |Delta s| + F u.
    Matern.  q = sqrt(max(s, floor)): |Delta q| <= |Delta s| / (q* + q) <= |Delta s| / q*, and, from
    |sqrt(x) - sqrt(y)| <= sqrt|x - y|, also <= sqrt|Delta s| (what is left at coincident points, the cusp).  The square
    root is within an ulp of exact (mgp_sqrt_pos: Goldschmidt step plus one correction): 2u q*.  With f = poly(q) 2^(-q)
    in base-2 units, d ln f / dq = -ln2 (Matern-1/2), -ln2 x / (1 + x) and -ln2 (x / 3)(1 + x) / (1 + x + x^2 / 3) with
    x = q ln2: |d ln f / dq| <= ln2 for all three.  So
        |Delta k| / k <= ln2 min(|Delta s| / q*, sqrt|Delta s|) + 2 u ln2 q* + F u.
    F = 8: 4.5u is what tests/test_host_math.py grants the shifted table form of 2^t, 2u the Matern polynomial (two
    fmas and the product with 2^(-q)), 1u the product with the variance; rounded up.
    Below the flush floor (k* < variance 2^-990 in fp64, 2^-120 in fp32) the bound does not apply: see `check_pairs`."""
    del variance
    return value_bound(name, distance_bound(a, b, D, dtype), q, dtype)


def value_bound(name, ds, q, dtype):
    """The value part of `pair_bound` for a given bound `ds` on |Delta s| (tests/assign_reference.py passes the direct
    form's bound, or adds what its float64 reference leaves): ln2 ds + F u (SE), ln2 min(ds / q*, sqrt ds) + 2 u ln2 q*
    + F u (Matern)."""
    u = unit_roundoff(dtype)
    ln2 = float(np.log(2.0))
    if name == "se":
        return ln2 * ds + FUNCTION_BUDGET * u
    q = np.asarray(q, dtype=np.float64)
    dq = np.minimum(ds / q, np.sqrt(ds))
    return ln2 * dq + 2.0 * u * ln2 * q + FUNCTION_BUDGET * u


def check_pairs(label, got, pv, rel, variance, dtype, extra_rel=0.0, row_ids=None, col_ids=None):
    """Hold got [n, C] to the long-double values: every entry finite; a pair with k* < variance 2^floor must lie in
    [0, variance 2^(floor + 1)] (the clamped loops of the fast kernels write an exact 0 below t = -1020: `kFlushLimit`,
    csrc/sweep.hip:455 and csrc/kxx.hip:118, used in `finish` / `values` as "t below the limit -> the pair contributes an
    exact 0"; the ldexp forms underflow gradually); every other pair within
    (rel + extra_rel) k*, no absolute slack.  No pair is left out.  Returns the worst err / bound over the pairs above
    the floor; raises AssertionError naming the worst offender."""
    got = np.asarray(got)
    assert got.shape == pv.k.shape, (label, got.shape, pv.k.shape)
    assert np.all(np.isfinite(got)), f"{label}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    g = got.astype(LD)
    fl = flush_floor_log2(dtype)
    below = pv.k < LD(variance) * LD(2) ** fl
    cap = LD(variance) * LD(2) ** (fl + 1)
    bad_low = below & ~((g >= 0) & (g <= cap))
    bound = (np.asarray(rel, dtype=np.float64) + extra_rel).astype(LD) * pv.k
    err = np.abs(g - pv.k)
    ratio = np.where(below, LD(0), err / np.where(bound > 0, bound, LD(1)))
    bad = bad_low | (~below & (err > bound))
    if np.any(bad):
        score = np.where(bad_low, LD(np.inf), ratio)
        i, j = np.unravel_index(int(np.argmax(np.where(bad, score, LD(-1)))), got.shape)
        ri = i if row_ids is None else row_ids[i]
        cj = j if col_ids is None else col_ids[j]
        rule = "flush floor" if bad_low[i, j] else "bound"
        raise AssertionError(
            f"{label}: {int(bad.sum())} of {bad.size} pairs outside the {rule}; worst pair ({ri}, {cj}): "
            f"s* = {float(pv.s[i, j]):.17g}, got {float(g[i, j]):.17e}, want {float(pv.k[i, j]):.17e}, "
            f"err {float(err[i, j]):.3e}, bound {float(bound[i, j]):.3e} (err / bound {float(ratio[i, j]):.3g})")
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------- point sets
def _rng(tag, name, D, seed):
    return np.random.default_rng([seed, tag, D, KINDS.index(name)])


def _rays(rng, n, D):
    v = rng.standard_normal((n, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _unscale(name, ls, A):
    return A * (ls / float(profile_scale(name)))


def safe_limit(name):
    """The fast sweeps run their unclamped loop while 2 (max|a|^2 + max|b|^2) is below this (csrc/sweep.hip, kNormLimit)."""
    return 1000.0 if name == "se" else 1.0e6


def range_set(name, D, n=1 << 15, seed=0):
    """X [n, D] on random rays from the origin, sorted by tau = s* (SE) or q* (Matern) to Z[0] = 0: the first
    n - n/4 values step through [0, U) with one value in every cell of width 1/8192 of every unit interval (U =
    (n - n/4) / 8192 when n >= 2^14).  In [1, U) the value sits in the middle 70 % of its cell, so each entry of the
    8192- and of the 2048-entry table is read there U - 1 times for certain; in [0, 1) it is anywhere in the cell, so
    the table's remainder g reaches its limits 2^-(TBITS+1) where the bound is smallest -- an error in the cubic
    coefficient of 2^g shows only there.  Then n/8 values fill [U, 8) and n/8 run log-spaced from 8 to 1100.  No
    cancellation: |a - 0|^2 = |a|^2.  Z [8, D]: the origin and seven points around it.  Returns X, Z, ls, n_near (the
    rows with tau < 8)."""
    rng = _rng(1, name, D, seed)
    ls = lengthscales(D)
    n_tail = n_mid = n // 8
    n_dense = n - n_tail - n_mid
    units = max(n_dense // 8192, 1)
    per = n_dense // units
    assert per * units == n_dense and units < 8
    width = np.where(np.arange(units) == 0, 1.0, 0.7)[:, None]  # unit 0: the whole cell, so that |g| reaches 2^-(TBITS+1)
    cell = np.arange(per)[None, :] + (rng.random((units, per)) - 0.5) * width
    dense = np.abs(np.arange(units)[:, None] + cell / per).ravel()
    mid = units + (8 - units) * (np.arange(n_mid) + rng.random(n_mid)) / n_mid
    tail = 8.0 * (1100.0 / 8.0) ** ((np.arange(n_tail) + rng.random(n_tail)) / n_tail)
    tau = np.sort(np.concatenate([dense, mid, tail]))
    tau[0] = 0.0  # a point on the origin itself: k = variance exactly
    rho = np.sqrt(tau) if name == "se" else tau
    X = _unscale(name, ls, _rays(rng, n, D) * rho[:, None])
    Z = _unscale(name, ls, np.concatenate([np.zeros((1, D)), 0.7 * rng.standard_normal((7, D))]))
    return X, Z, ls, n - n_tail


def shifted_set(name, D, N, M, seed=0):
    """Two clouds of scaled spread 0.5 around one centre with |centre|^2 = 170 (scaled |a|^2 up to about 200, so
    2 (aa + bb) < 1000 holds and the SE form runs with a large |a|^2 folded into its magic constant), with exact
    duplicates X[i] = Z[j] for a tenth of the smaller side."""
    rng = _rng(2, name, D, seed)
    ls = lengthscales(D)
    centre = np.sqrt(170.0 / D) * rng.choice([-1.0, 1.0], D)
    X = _unscale(name, ls, centre + 0.5 * rng.standard_normal((N, D)))
    Z = _unscale(name, ls, centre + 0.5 * rng.standard_normal((M, D)))
    ndup = max(1, min(N, M) // 10)
    Z[rng.choice(M, ndup, replace=False)] = X[rng.choice(N, ndup, replace=False)]
    Z[0], Z[M - 1] = X[0], X[N - 1]  # the first and the last streamed point are duplicates too
    return X, Z, ls


def edge_set(name, D, N, M, seed=0):
    """Straddles the `safe` decision of the fast sweeps, L = safe_limit(name).  Z[0] = -sqrt(0.24 L) e is the largest
    point of Z, the rest of Z an ordinary cloud.  X is an ordinary cloud in which, per run of 2048 rows, a few rows lie
    on +e (opposite Z[0]) and on random rays:
      run 0: |a|^2 = 0.255 L  -> 2 (0.255 + 0.24) L = 0.99 L, just below the limit;
      run 1: |a|^2 = 0.262 L  -> 1.004 L, just above (if there is a second run);
      last run: 64 rows with |a|^2 from 0.25 L to 0.30 L (Matern: 0.345 L) on +e: s* (SE) or q* (Matern) to Z[0] runs
                from about 980 to 1077, through t = -1000 and the flush floor and on to the end of the denormal range.
    So ordinary rows share a workgroup with far ones, and with X streamed (max |a|^2 = 0.30 L or 0.345 L) the block of Z that
    holds Z[0] is above the limit and the others below.  Returns X, Z, ls, far_rows (the special rows of X)."""
    rng = _rng(3, name, D, seed)
    ls = lengthscales(D)
    L = safe_limit(name)
    e = _rays(rng, 1, D)[0]
    A = 0.6 * rng.standard_normal((N, D))
    B = 0.6 * rng.standard_normal((M, D))
    B[0] = -np.sqrt(0.24 * L) * e
    runs = max(1, -(-N // 2048))
    far = []

    def put(lo, hi, count, frac, on_e):
        rows = rng.choice(np.arange(lo, hi), min(count, hi - lo), replace=False)
        fracs = np.linspace(frac[0], frac[1], len(rows)) if isinstance(frac, tuple) else np.full(len(rows), frac)
        for r, f in zip(rows, fracs):
            A[r] = np.sqrt(f * L) * (e if on_e else _rays(rng, 1, D)[0])
            far.append(int(r))

    for run in range(runs):
        lo, hi = run * 2048, min(N, (run + 1) * 2048)
        if run == runs - 1:
            put(lo, hi, 64, (0.25, 0.30 if name == "se" else 0.345), True)
        elif run == 0:
            put(lo, hi, 3, 0.255, True)
            put(lo, hi, 3, 0.255, False)
        elif run == 1:
            put(lo, hi, 3, 0.262, True)
            put(lo, hi, 3, 0.262, False)
    return _unscale(name, ls, A), _unscale(name, ls, B), ls, sorted(set(far))
