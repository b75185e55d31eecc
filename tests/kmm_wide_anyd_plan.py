"""The launch plan of the many-column (K_mm + Lambda) operator above 32 dimensions (csrc/kmm_wide_anyd.hip,
MGP_OP_KMM_LAMBDA_WIDE_ANYD) as plain Python: tile sizes, the K slices, the groups of right-hand sides, the split rule
of the streamed side and the byte count of the `prj` arena -- pinned to the expressions of the source by
tests/test_kmm_wide_anyd_plan.py -- and the shapes tests/test_gpu_kmm_wide_anyd.py runs.  The distance chain is that of
csrc/sweep_anyd.hip: `sweep_anyd_plan.emulate_neg_s` with the streamed point in the A role."""

import sweep_anyd_plan as ap

KIND = 8             # MGP_OP_KMM_LAMBDA_WIDE_ANYD
NOMINAL_CUS = 256
THREADS = 256        # kWThreads
OWN = 64             # kWOwn: output elements per workgroup
STEP = 32            # kWStep: streamed points per step; a split is a multiple
KSL = 8              # kWKSL: k-steps of 4 per K slice
MAX_R = 256          # kWMaxR: right-hand sides per group
MIN_SPLIT_ROWS = 256
FINISH_I, FINISH_B = 64, 16

ceil_div = ap.ceil_div
k_steps = ap.k_steps
slices = ap.slices


def align256(b):
    return (b + 255) & ~255


def groups(Bt):
    """Widths of the groups of right-hand sides: full groups of MAX_R, then the remainder."""
    return [min(MAX_R, Bt - g0) for g0 in range(0, Bt, MAX_R)]


def row_tiles(r):
    """NRT of the instantiation a group of r right-hand sides runs: 16-row tiles of P^T per wave."""
    return 2 if r <= 32 else 4 if r <= 64 else 8 if r <= 128 else 16


def split_plan(M, num_cus=NOMINAL_CUS):
    """(nblk, nsplit, rows) of wide_anyd_plan."""
    nblk = ceil_div(M, OWN)
    ns = ceil_div(2 * num_cus, nblk)
    ns = max(1, min(ns, ceil_div(M, MIN_SPLIT_ROWS)))
    rows = ceil_div(ceil_div(M, ns), STEP) * STEP
    return nblk, ceil_div(M, rows), rows


def pack_bytes(M, D):
    return align256(8 * 64 * k_steps(D) * ceil_div(M, 16))


def part_bytes(M, Bt, num_cus=NOMINAL_CUS):
    nblk, nsplit, _ = split_plan(M, num_cus)
    RP = ceil_div(min(Bt, MAX_R), 16) * 16
    return align256(8 * nsplit * nblk * OWN * RP)


def arena_bytes(M, D, Bt, num_cus=NOMINAL_CUS):
    """The request on the prj arena: the pack of Z, then the split tiles of the widest group."""
    return pack_bytes(M, D) + part_bytes(M, Bt, num_cus)


def terms(M, num_cus=NOMINAL_CUS):
    """The longest chain of products one split accumulates into one output: its streamed rows (padding included)."""
    return split_plan(M, num_cus)[2]


# ---------------------------------------------------------------- the shapes of the GPU tests
PAIR_DIMS = (33, 34, 62, 63, 77, 512)         # K = D + 2: 35, 36 (a slice and a bit), 64 (two whole slices), 65, 79, 514
PAIR_SIZES = (1, 15, 16, 17, 127, 128, 129, 391)  # a ragged tile, one workgroup and a wave past it, and a split (391)
WIDTHS = (1, 15, 16, 17, 128, 129, 255, 256, 257, 300)  # every instantiation, a full group, the remainder seams
DENSE_M, DENSE_D = 290, 40                    # two splits of 160 and 130 rows, two K slices


def probed(M):
    """Columns of a one-hot probe at M points: both ends, the middle and the starts of the last tile and workgroup."""
    c = {0, M - 1, M // 2, M // 3, (M - 1) // 16 * 16, (M - 1) // 64 * 64, max(M - 17, 0), min(M - 1, 160)}
    return sorted(c)[:8]
