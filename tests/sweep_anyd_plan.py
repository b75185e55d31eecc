"""The launch plan of the fused any-D sweep (csrc/sweep_anyd.hip) as plain Python: tile sizes, the K slices, the
column-pass ladder, the chunk rule of the streamed set and the byte count of the `ws` arena -- pinned to the
expressions of the source by tests/test_sweep_anyd_plan.py -- the shapes tests/test_gpu_sweep_anyd.py runs, and an
fp64 emulation of the augmented-K chain in the kernel's order.
"""

import numpy as np

import pair_reference as pr

LD = np.longdouble
KINDS = pr.KINDS
NOMINAL_CUS = 256
FUSED_MAX_D = 32
MAX_D = 512

THREADS = 256
TR = 2               # kTRa: 16-row tiles per wave
OWN = 4 * TR * 16    # kOwn: owned rows per workgroup
NJT = 4              # kNJT: 16-column tiles per streamed tile
TILE = NJT * 16      # kTile: streamed points per LDS tile
KSL = 8              # kKSL: k-steps (of 4 columns of K) per slice
WIDTHS = (8, 4, 2, 1)


def ceil_div(a, b):
    return -(-a // b)


def k_steps(D):
    """KS: steps of 4 over K = D + 2 (the coordinates, |a|^2 / -1 and 1 / -|b|^2), padded with zeros."""
    return (D + 2 + 3) >> 2


def slices(D):
    """k-steps of every K slice, in the order the accumulator tiles see them."""
    ks = k_steps(D)
    return [min(KSL, ks - s0) for s0 in range(0, ks, KSL)]


def passes(R):
    """Column passes of R right-hand sides: the widest of 8, 4, 2, 1 that fits, repeatedly."""
    out = []
    while R > 0:
        w = next(w for w in WIDTHS if w <= R)
        out.append(w)
        R -= w
    return out


def chunk_plan(na, nb, num_cus=NOMINAL_CUS):
    """(nblk, nchunks, b_chunk) of anyd_plan."""
    nblk = ceil_div(na, OWN)
    target = 8 * num_cus
    nchunks = 1 if nblk >= 4 * num_cus else ceil_div(target, nblk)
    nchunks = max(1, min(nchunks, ceil_div(nb, TILE)))
    b_chunk = ceil_div(ceil_div(nb, nchunks), TILE) * TILE
    return nblk, ceil_div(nb, b_chunk), b_chunk


def chunk_sizes(na, nb, num_cus=NOMINAL_CUS):
    _, nchunks, b_chunk = chunk_plan(na, nb, num_cus)
    return [min(b_chunk, nb - c * b_chunk) for c in range(nchunks)]


def ws_bytes(na, nb, R, num_cus=NOMINAL_CUS):
    """The request on the ws arena: both squared-norm vectors, and the chunk partials of the widest pass."""
    _, nchunks, _ = chunk_plan(na, nb, num_cus)
    return 8 * (na + nb + (nchunks * na * passes(R)[0] if nchunks > 1 else 0))


# ---------------------------------------------------------------- the dimensions and shapes of the GPU tests
SLICE_EDGE_DIMS = (58, 62, 63)  # KS = 15, 16, 17: one k-step below, exactly at and one above two whole K slices
DIMS = (33, 34, 35, 36) + SLICE_EDGE_DIMS + (77, 90, 511, 512)
OWNED = (1, OWN - 1, OWN, OWN + 1, 3 * OWN + 7)
STREAMED = (1, TILE - 1, TILE + 1, 100, 150)  # one owned block: 100 -> chunks of 64 + 36, 150 -> 64 + 64 + 22
COLUMNS = WIDTHS + (WIDTHS[0] + 1, 0)
COLS, ROWS = 0, 1


class Case:
    """One dense-multiplier product: entry in {"knm", "kmn", "kxx"}; na owned and nb streamed points (kxx: na == nb)."""

    def __init__(self, entry, kind, D, na, nb, R, w_layout=COLS, out_layout=COLS, s2=0.0, tag=""):
        self.entry, self.kind, self.D, self.na, self.nb, self.R = entry, kind, D, na, nb, R
        self.w_layout, self.out_layout, self.s2 = w_layout, out_layout, s2
        self.id = f"{entry}-{kind}-D{D}-{na}x{nb}-R{R}-{'cr'[w_layout]}{'cr'[out_layout]}" + (f"-{tag}" if tag else "")

    def __repr__(self):
        return self.id


def dense_cases():
    """One factor at a time around (OWN + 1) x (TILE + 1) x 3 columns; the entry point alternates so that both
    orientations see every factor, the kernel kind cycles.  D = 77 carries the shape and column ladders, the
    slice-edge dimensions the layouts."""
    out = []
    kinds = list(KINDS)
    n = 0

    def add(D, na, nb, R, **kw):
        nonlocal n
        entry = kw.pop("entry", ("knm", "kmn")[n % 2])
        out.append(Case(entry, kinds[n % 4], D, na, nb, R, **kw))
        n += 1

    for D in DIMS:
        add(D, OWN + 1, TILE + 1, 3)
    for na in OWNED:
        for entry in ("knm", "kmn"):
            add(77, na, 100, 2, entry=entry)
    for nb in STREAMED:
        for entry in ("knm", "kmn"):
            add(77, OWN + 1, nb, 2, entry=entry)
    for R in COLUMNS:
        for entry in ("knm", "kmn"):
            add(77, OWN + 1, 150, R, entry=entry)
    for D, (wl, ol) in zip(SLICE_EDGE_DIMS + (77,), ((COLS, ROWS), (ROWS, COLS), (ROWS, ROWS), (ROWS, ROWS))):
        for entry in ("knm", "kmn"):
            add(D, OWN + 1, 150, 5, entry=entry, w_layout=wl, out_layout=ol)
    # a non-zero alpha * addend: (k(X, X) + s2 I) V, one chunk and three, both layouts
    for D, N, R, lay in ((77, OWN + 1, 3, COLS), (62, 150, 9, ROWS), (512, TILE + 1, 1, COLS)):
        add(D, N, N, R, entry="kxx", s2=0.37, w_layout=lay, out_layout=lay)
    return out


def unsplit_case(num_cus=NOMINAL_CUS):
    """Enough owned blocks that the streamed set is not split: one workgroup walks three streamed tiles, the last ragged."""
    na = 4 * num_cus * OWN
    assert chunk_plan(na, 150, num_cus)[1] == 1
    return Case("knm", "matern32", 33, na, 150, 1, tag="unsplit")


def points(case, seed=0):
    """Owned and streamed points of a dense case: standard normal clouds, the lengthscales stretched by sqrt(D) so that
    r^2 is about 2 at every D and the sums are of kernel values of order 1/e, not of underflowing ones."""
    rng = np.random.default_rng([seed, case.D, case.na, case.nb, KINDS.index(case.kind)])
    ls = pr.lengthscales(case.D) * np.sqrt(case.D)
    A = rng.standard_normal((case.na, case.D))
    B = A if case.entry == "kxx" else rng.standard_normal((case.nb, case.D))
    return A, B, ls


# ---------------------------------------------------------------- the chain in fp64
def _fma(a, b, c):
    """fl(a b + c) for float64 arrays through long double: the product carries 2^-64, the sum 2^-64, and the final
    rounding to float64 is off from the fused result by at most 2^-11 ulp -- far inside what the bound grants a step."""
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


def emulate_neg_s(name, ls, P, Q):
    """-s [n, C] as the kernel forms it, in float64: a = fl(x fl(c / l)), |a|^2 and |b|^2 as fma chains over d
    ascending, then one accumulator per pair over K ascending, slice by slice: D steps 2 a_d b_d, then |a|^2 (-1), then
    1 (-|b|^2); the zero padding adds nothing."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    D = P.shape[1]
    sc = float(pr.profile_scale(name)) / np.asarray(ls, dtype=np.float64)  # c / l_d: one rounding, as on the host
    a, b = P * sc, Q * sc
    na2, nb2 = np.zeros(P.shape[0]), np.zeros(Q.shape[0])
    for d in range(D):
        na2 = _fma(a[:, d], a[:, d], na2)
        nb2 = _fma(b[:, d], b[:, d], nb2)
    arow = np.concatenate([a, na2[:, None], np.ones((P.shape[0], 1))], axis=1)
    bcol = np.concatenate([b + b, -np.ones((Q.shape[0], 1)), -nb2[:, None]], axis=1)
    acc = np.zeros((P.shape[0], Q.shape[0]))
    k = 0
    for steps in slices(D):
        for _ in range(4 * steps):
            if k < D + 2:
                acc = _fma(arow[:, k][:, None], bcol[:, k][None, :], acc)
            k += 1
    return acc


def emulate_values(name, variance, ls, P, Q):
    """variance * profile(-s) of the emulated chain; the profile itself in long double (its own error is the bound's F)."""
    neg_s = emulate_neg_s(name, ls, P, Q).astype(LD)
    c2 = pr.profile_scale(name) ** 2
    if name == "se":
        return LD(variance) * np.exp2(neg_s)
    q = np.sqrt(np.maximum(-neg_s, c2 * pr.R2_FLOOR))
    x = q * np.log(LD(2))
    poly = {"matern12": LD(1), "matern32": LD(1) + x, "matern52": LD(1) + x + x * x / LD(3)}[name]
    return LD(variance) * poly * np.exp2(-q)


# ---------------------------------------------------------------- the point sets of the per-pair probes
PAIR_DIMS = (33, 77, 512)


def pair_sets(name, D):
    """(label, owned P, streamed Q, probed columns of Q) for both orientations of the shifted clouds (duplicates,
    |a|^2 ~ 170 - 200) and of the edge set (the clamp, t through -1000 and the flush floor)."""
    X, Z, _ = pr.shifted_set(name, D, 300, 63)
    out = [("shifted", X, Z, [0, 62, 61, 31, 32, 1, 17, 40]), ("shifted-reversed", Z, X, [0, 299, 298, 63, 64, 127, 128, 200])]
    X, Z, _, far = pr.edge_set(name, D, 2200, 300)
    out += [("edge", X, Z, [0, 1, 299, 63, 64, 100, 234, 298]),
            ("edge-reversed", Z, X, [far[-1], far[-20], far[-40], far[-64], far[0], far[3], 0, 2199])]
    return out
