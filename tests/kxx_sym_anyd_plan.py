"""The launch plan of the symmetric self-kernel operator above 32 dimensions (csrc/kxx_sym_anyd.hip,
MGP_OP_KXX_NOISE_SYM_ANYD) as plain Python: the blocks, the cyclic deal of unordered block pairs, the chunks of d a
workgroup chains, the slots of a launch and the byte count of the `kxx` arena -- pinned to the expressions of the
source by tests/test_kxx_sym_anyd_plan.py -- and the shapes tests/test_gpu_kxx_sym_anyd.py runs."""

import sweep_anyd_plan as ap

KIND = 9             # MGP_OP_KXX_NOISE_SYM_ANYD
NOMINAL_CUS = 256
THREADS = 256        # kSThreads
NJ = 2               # kSNJ: kept 16-point tiles per wave
TB = 64 * NJ         # kSTB: points per block
NIT = 2              # kSNIT: streamed tiles per step
KSL = 8              # kSKSL: k-steps of 4 per K slice
COLS = 16            # kSCols: right-hand sides per group
SLOT_BUDGET = 1 << 29
MAX_SLOTS = 32768

ceil_div = ap.ceil_div
k_steps = ap.k_steps


def align256(b):
    return (b + 255) & ~255


def groups(Bt):
    """Widths of the groups of right-hand sides: full groups of COLS, then the remainder."""
    return [min(COLS, Bt - g0) for g0 in range(0, Bt, COLS)]


def plan(N, r, num_cus=NOMINAL_CUS):
    """sym_plan: (nb, npad, nd, DC, S) for a group of r live columns."""
    nb = ceil_div(N, TB)
    npad = nb * TB
    nd = nb // 2 + 1
    want = min(max(ceil_div(2 * num_cus, nb), 1), nd)
    dc = ceil_div(nd, want)
    maxs = min(max(SLOT_BUDGET // (npad * r * 8), 2), MAX_SLOTS)
    dc = min(dc, maxs - 1)
    cpl = max(maxs // (dc + 1), 1)
    S = min(cpl * dc, nd)
    return nb, npad, nd, dc, S


def launches(N, r, num_cus=NOMINAL_CUS):
    """(d0, nd, nch) of every tile launch of one group."""
    _, _, nd_total, dc, S = plan(N, r, num_cus)
    out = []
    for d0 in range(0, nd_total, S):
        nd = min(S, nd_total - d0)
        out.append((d0, nd, ceil_div(nd, dc)))
    return out


def tile_of(nb, I, d):
    """(J, what) of workgroup I at distance d: what in {"diag", "idle", "pair"}."""
    J = (I + d) % nb
    if d == 0:
        return J, "diag"
    if 2 * d == nb and I >= nb // 2:
        return J, "idle"
    return J, "pair"


def block_pairs(nb):
    """Every (I, J) the deal evaluates: the diagonal tiles and the active off-diagonal ones."""
    return [(I, tile_of(nb, I, d)[0]) for d in range(nb // 2 + 1) for I in range(nb) if tile_of(nb, I, d)[1] != "idle"]


def slot_writers(N, r, num_cus=NOMINAL_CUS):
    """Per launch, {(slot, block): number of workgroups that write the rows of that block in that slot}."""
    nb, _, _, dc, S = plan(N, r, num_cus)
    out = []
    for d0, nd, nch in launches(N, r, num_cus):
        w = {}
        for ch in range(nch):
            for I in range(nb):
                w[(S + ch, I)] = w.get((S + ch, I), 0) + 1  # the kept-side sums of the chunk
                for dd in range(ch * dc, min((ch + 1) * dc, nd)):
                    J, _ = tile_of(nb, I, d0 + dd)  # the streamed-side sums, or the zeros of a diagonal / idle tile
                    w[(dd, J)] = w.get((dd, J), 0) + 1
        out.append(w)
    return out


def path(nb, bi, bj):
    """How the output rows of block bi receive the right-hand sides of block bj: "diag" (the diagonal tile), "kept"
    (bi is the block its workgroup keeps: the tile goes in as the B operand from the result registers) or "streamed"
    (bi is streamed: the transposed tile from LDS)."""
    if bi == bj:
        return "diag"
    d = (bj - bi) % nb
    if d <= nb // 2 and tile_of(nb, bi, d)[1] == "pair":
        return "kept"
    return "streamed"


def pack_bytes(N, D):
    return align256(8 * 64 * k_steps(D) * (ceil_div(N, TB) * TB // 16))


def slot_bytes(N, r, num_cus=NOMINAL_CUS):
    _, npad, _, dc, S = plan(N, r, num_cus)
    return align256(8 * (S + ceil_div(S, dc)) * npad * r)


def arena_bytes(N, D, Bt, num_cus=NOMINAL_CUS):
    """The request on the kxx arena: pack, Wt, running sum, slots (the larger need of the call's two group widths)."""
    npad = ceil_div(N, TB) * TB
    widths = {min(Bt, COLS)} | ({Bt % COLS} if Bt > COLS and Bt % COLS else set())
    return pack_bytes(N, D) + 2 * align256(8 * COLS * npad) + max(slot_bytes(N, r, num_cus) for r in widths)


def terms(N, r, num_cus=NOMINAL_CUS):
    """The longest chain of products one accumulator takes: the DC blocks a workgroup streams past the block it keeps."""
    return TB * plan(N, r, num_cus)[3]


def slots(N, r, num_cus=NOMINAL_CUS):
    """The sums of the finish kernel over every launch, as the header counts them."""
    _, _, nd, dc, S = plan(N, r, num_cus)
    return nd + ceil_div(nd, dc) + 2 * ceil_div(nd, S)


def chain(N, Bt, num_cus=NOMINAL_CUS):
    """terms + slots + 3 of the header's bound, the largest over the call's groups."""
    return max(terms(N, r, num_cus) + slots(N, r, num_cus) for r in set(groups(Bt))) + 3


# ---------------------------------------------------------------- the shapes of the GPU tests
PAIR_DIMS = (33, 77, 512)
PAIR_SIZES = (100, 200, 300, 610)   # one block; nb = 2 (the even rule at d = nb/2); nb = 3; nb = 5, 610 = 16 * 38 + 2
WIDTHS = (1, 2, 5, 8, 16, 17, 33)   # both sides of the group seam
DENSE_N, DENSE_D = 300, 40


def chained_size(num_cus=NOMINAL_CUS):
    """The smallest N (two points past a block seam) at which a workgroup chains more than one d (DC > 1)."""
    nb = 2
    while plan(nb * TB, COLS, num_cus)[3] < 2:
        nb += 1
    return (nb - 1) * TB + 2


def probed(N):
    """Columns of a one-hot probe at N points: both ends, the middle, and both sides of the first, the middle and the
    last block seam (with up to five blocks: of every seam but one)."""
    nb = ceil_div(N, TB)
    c = {0, N - 1, N // 2, N // 3}
    for b in {1, nb // 2, nb - 1}:
        if 1 <= b < nb:
            c |= {b * TB - 1, b * TB}
    return sorted(c)
