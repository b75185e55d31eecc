"""The plan of csrc/quadform.hip's fused route (mgp_knm_quadform, include/mgp_predict.h) in plain Python: the row tile,
the column block, the pairing of the blocks, the chunking of the test rows and the scratch formula.
tests/test_quadform_plan.py pins every constant and rule to the expressions of the source by text; the GPU tests take
their shapes from here."""

T = 128            # QT: test rows per workgroup
C = 128            # QC: columns of C per block
STEP = 16          # QK: rows of Z (and of C) per step of the walk
CHUNK_B = 1 << 16  # QF_CHUNK_B: test rows per launch
FUSED_MAX_D = 32   # MGP_FUSED_MAX_D
PANEL_BYTES = 256 << 20  # the generic route's row panel of k(Xs, Z)
KINDS = ("se", "matern12", "matern32", "matern52")
DIMS = (1, 3, 8, 12, 17, 32)  # padded to 2, 4, 8, 16, 32, 32 (padded_dim): every rung, the top one ragged and full


def padded_dim(D):
    """DP of mgp_with_dp: the smallest of 2, 4, 8, 16, 32 that holds D."""
    for dp in (2, 4, 8, 16, 32):
        if D <= dp:
            return dp
    raise ValueError(D)


def blocks(M):
    """nJ: column blocks of C."""
    return (M + C - 1) // C


def pairs(M):
    """The blocks each workgroup of grid row y walks, in its order: the heavier block nJ-1-y first, then block y; the
    middle block of an odd nJ stands alone.  Every block appears exactly once."""
    nJ = blocks(M)
    out = []
    for y in range((nJ + 1) // 2):
        first, second = nJ - 1 - y, y
        out.append((first,) if first == second else (first, second))
    return out


def walk_steps(M, J):
    """Steps of 16 rows a workgroup takes for block J: i = 0 ... min(M, (J + 1) c)."""
    return (min(M, (J + 1) * C) + STEP - 1) // STEP


def grid(B, M):
    """(row tiles, block pairs) of each launch, one launch per chunk of CHUNK_B test rows."""
    out = []
    for c0 in range(0, B, CHUNK_B):
        bc = min(B - c0, CHUNK_B)
        out.append(((bc + T - 1) // T, (blocks(M) + 1) // 2))
    return out


def part_bytes(B, M):
    """The per-block row sums part[nJ][B'] of the largest chunk, rounded up to 256."""
    bpad = (min(B, CHUNK_B) + T - 1) // T * T
    return (8 * blocks(M) * bpad + 255) & ~255


def scratch_bytes(B, M, D):
    """What the fused route asks of the "prj" arena: the partials and the packed Z."""
    return part_bytes(B, M) + 8 * M * (padded_dim(D) + 1)


def generic_scratch_bytes(B, M, elem):
    """The generic route: the symmetric matrix, one row panel of k(Xs, Z) and its product, + 256."""
    rows = max(PANEL_BYTES // (M * elem), 64)
    rows = min(rows, B)
    return elem * (M * M + 2 * rows * M) + 256


def generic_panel_rows(B, M, elem):
    return min(max(PANEL_BYTES // (M * elem), 64), B)


def gemm_slices_bound(p, M, elem, cus):
    """The most the generic route's NT GEMM [p, M] x [M, M] asks of the "ws" arena: s contraction slices of the
    product when it has fewer than 2 CUs tiles of 128 x 128, s lowered until a slice holds 256 of the M terms (the
    aligned form lowers it further until 16 s divides M); 0 when s = 1."""
    tiles = ((M + 127) // 128) * ((p + 127) // 128)
    if tiles >= 2 * cus:
        return 0
    s = min(8, (2 * cus + tiles - 1) // tiles)
    while s > 1 and M // s < 256:
        s -= 1
    return s * elem * p * M if s > 1 else 0


def reserved(need):
    """What a growing handle allocates for a request of `need` bytes (mgp_reserve)."""
    return need + (need >> 2) + 4096


# the shapes of the GPU value test: the smallest that reach every seam, in units of T and C
M_VALUES = (1, C - 1, C, C + 1, 2 * C, 3 * C + 5)
B_VALUES = (1, T - 1, T + 1, 2 * T + 3)
