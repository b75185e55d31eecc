"""References for the many-column form of the matrix-free (K_mm + Lambda) operator (`MGP_OP_KMM_LAMBDA_WIDE`,
csrc/project.hip): a long-double restatement of out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda) on the profiles of
tests/pair_reference.py, a restatement of the route's cut plan, and the case list the GPU tests take from that plan
(tests/test_kmm_wide_host.py on the CPU, tests/test_gpu_kmm_wide.py on the GPU).
"""

import numpy as np

import pair_reference as pr

LD = np.longdouble
KINDS = pr.KINDS
VARIANCE = pr.VARIANCE

# ---------------------------------------------------------------- the route's constants (csrc/project.hip)
GROUP = 256        # PJ_MAX_R: right-hand sides per launch of the main kernel
STEP = 16          # PK: streamed rows per step; a split is a multiple
SPLIT_FLOOR = 1024  # pj_plan: at least this many streamed rows per split
ROW_CHUNK = 1 << 16  # PJ_CHUNK_B: output rows per launch
FUSED_MAX_D = 32
FINISH_ROWS, FINISH_COLS = 64, 16  # tile of the finish kernel


# ---------------------------------------------------------------- long-double product
def inputs(M, D, seed=0):
    """Z [M, D], lengthscales [D], lambda [M] > 0: unit-spread points, lengthscales growing with sqrt(D) so that the
    kernel values stay well away from 0 at every D."""
    rng = np.random.default_rng([seed, M, D])
    Z = rng.standard_normal((M, D))
    ls = 0.6 + rng.random(D) * float(np.sqrt(D))
    lam = 0.05 + rng.random(M)
    return Z, ls, lam


def kmm_matrix(name, variance, ls, Z, block=128):
    """k(Z, Z) [M, M] in long double: r^2 from direct differences of the fp64 inputs (relative error ~1e-19), the
    profile by `pair_reference.k_over_variance`."""
    Zl = np.asarray(Z, dtype=np.float64).astype(LD)
    ls = np.asarray(ls, dtype=np.float64).astype(LD).reshape(-1)
    M = Zl.shape[0]
    K = np.empty((M, M), dtype=LD)
    for i0 in range(0, M, block):
        w = (Zl[i0:i0 + block, None, :] - Zl[None, :, :]) / ls
        hi = (w * w).sum(axis=2)
        K[i0:i0 + block] = LD(variance) * pr.k_over_variance(name, hi, np.zeros_like(hi))
    return K


def product(K, lam, P, rows=None):
    """P [Bt, M] (K + diag lam) in long double, for K from `kmm_matrix`; `rows`: those right-hand sides only."""
    Pl = np.asarray(P, dtype=np.float64).astype(LD)
    if rows is not None:
        Pl = Pl[np.asarray(rows, dtype=np.int64)]
    return Pl @ K + Pl * np.asarray(lam, dtype=np.float64).astype(LD)[None, :]


def probed_columns(M, Bt):
    """The right-hand sides of a product case that are held to long double.  A right-hand side is one chain of its own
    through the route (a column of the staged panel, of the accumulator tiles and of the finish tile), so up to
    M = 129 all of them; above, where numpy's long-double product runs at ~1e8 multiply-adds a second, the ones beside
    every cut a column index meets: both ends of the batch, of the first 16-column tile, of the 128-column tile choice
    and of the 256-column group (the whole batch is still held to the sweep form by the agreement test)."""
    if M <= 129:
        return list(range(Bt))
    marks = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, Bt - 2, Bt - 1)
    return sorted({b for b in marks if 0 <= b < Bt})


# ---------------------------------------------------------------- the cut plan
def dp_of(D):
    """The padded dimension of the fused kernels: the smallest of 2, 4, 8, 16, 32 that holds D."""
    for dp in (2, 4, 8, 16, 32):
        if D <= dp:
            return dp
    raise ValueError("D > 32 takes the sweep form")


def groups(Bt):
    """[(first column, width)]: groups of at most 256 right-hand sides."""
    return [(g0, min(GROUP, Bt - g0)) for g0 in range(0, Bt, GROUP)]


def row_tile(width):
    """Output rows per workgroup of the main kernel: 128 for a group of at most 128 columns, 64 above."""
    return 128 if width <= 128 else 64


def splits(tiles, M, num_cus):
    """`pj_plan`: (number of splits of the streamed rows, rows per split) for a launch of `tiles` row tiles -- about
    four workgroups per CU, at least 1024 streamed rows per split, a multiple of 16 each."""
    ns = -(-4 * num_cus // tiles)
    ns = max(1, min(ns, -(-M // SPLIT_FLOOR)))
    rw = -(-M // ns)
    rw = -(-rw // STEP) * STEP
    return max(1, -(-M // rw)), rw


def plan(M, Bt, num_cus=256):
    """One dict per launch pair (main + finish) of an application: the group, the row chunk, the tile, the splits and
    the bytes of split tiles it needs."""
    out = []
    for g0, width in groups(Bt):
        rp = -(-width // 16) * 16
        pb = row_tile(width)
        for c0 in range(0, M, ROW_CHUNK):
            rows = min(ROW_CHUNK, M - c0)
            tiles = -(-rows // pb)
            ns, rw = splits(tiles, M, num_cus)
            out.append(dict(g0=g0, width=width, padded=rp, c0=c0, rows=rows, tile=pb, tiles=tiles, splits=ns,
                            rows_per_split=rw, part_bytes=8 * ns * tiles * pb * rp))
    return out


def arena_bytes(M, D, Bt, num_cus=256):
    """Bytes of the `prj` arena an application or a solve with Bt right-hand sides reserves: the pack of Z and the
    split tiles of the launch that needs most, each rounded up to 256."""
    up = lambda b: (b + 255) & ~255
    return up(8 * M * (dp_of(D) + 1)) + up(max(p["part_bytes"] for p in plan(M, Bt, num_cus)))


# ---------------------------------------------------------------- the GPU product cases
PRODUCT_M = (1, 15, 17, 63, 65, 127, 129, 1040, 2049, 2065)
PRODUCT_COLUMNS = (1, 15, 16, 17, 33, 64, 65, 128, 129, 256, 257, 300)
PRODUCT_D = (1, 3, 8, 9, 32)
_NARROW, _MID, _WIDE = PRODUCT_COLUMNS[:4], PRODUCT_COLUMNS[4:8], PRODUCT_COLUMNS[8:]


def product_cases():
    """[(kind, D, M, column counts)]: every kind meets every M, D cycling.  Up to M = 129 a case runs every column
    count; above, where the long-double matrix alone costs seconds, one count of each instantiation family (<= 32,
    33 ... 128, > 128 columns), rotating so that over the four kinds every count meets a large M."""
    cases = []
    for ki, kind in enumerate(KINDS):
        for mi, M in enumerate(PRODUCT_M):
            D = PRODUCT_D[(mi + ki) % len(PRODUCT_D)]
            if M > 1040 and D == 32:  # the long-double matrix costs M^2 D: D = 32 meets two splits at M = 1040
                D = 3
            if M <= 129:
                cols = PRODUCT_COLUMNS
            else:
                q = (mi + ki) % 4
                cols = (_NARROW[q], _MID[q], _WIDE[q])
            cases.append((kind, D, M, tuple(cols)))
    return cases
