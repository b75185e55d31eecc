"""The padded-dimension ladder and the column rungs of the fused (D <= 32) entry points, restated, and the cases that
reach every instantiation the rules can pick.

Every fused entry point of libmgp is compiled once per rung of the padded-dimension ladder (`mgp_with_dp`,
csrc/mgp_common.h) and, most of them, once per width of a pass over its right-hand-side columns.  The rules below are
the host arithmetic of the csrc functions they name (host only: no torch, no library); `reachable(entry)` is the set of
instantiations a rule can pick and `reached(case)` the ones a planned case runs.  tests/test_ladder_plan.py checks on
the CPU that the two sets are equal for every entry point, that every case's shape crosses the tile seams it states,
and that each restated expression still stands in the source; tests/test_gpu_ladder.py runs the cases with dense
multipliers (every entry normal, no zeros) against long double.

A case's shape is the smallest that fills the instantiation it names: three blocks of that instantiation's tile with a
ragged last one on every tiled axis (`Case.tiles`: axis -> (length, tile)), and one duplicate pair for the Matern kinds.
Every reachable rung appears at its top (D = 2, 4, 8, 16, 32) and one past the rung below (D = 1, 3, 5, 9, 17).  The
four kernel kinds rotate over the cases; Matern-1/2 stands on every rung of the two entry points whose pass widths
depend on it.

`COMPLETE` lists the entry points other tests already hold on every rung, so the whole matrix is in one place.
"""

import seam_plan as sp

KINDS = ("se", "matern12", "matern32", "matern52")
RUNGS = (2, 4, 8, 16, 32)
FUSED_MAX_D = 32
NUM_CUS = sp.NOMINAL_CUS
F64, F32 = "float64", "float32"


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the ladder (csrc/mgp_common.h, mgp_with_dp)
def with_dp(D, min_dp=2):
    """DP = the smallest of {2, 4, 8, 16, 32} that is >= max(D, min_dp); `mgp_with_dp<4>` is min_dp = 4."""
    assert 1 <= D <= FUSED_MAX_D
    return next(p for p in RUNGS if p >= max(D, min_dp))


def rungs(min_dp=2):
    return tuple(p for p in RUNGS if p >= min_dp)


def rung_ds(DP):
    """(one past the rung below, the top of the rung): a padded and a full instantiation.  Rung 2 starts at D = 1."""
    return (1 if DP == 2 else DP // 2 + 1), DP


# min_dp of each entry point's ladder (the template argument of its mgp_with_dp call)
MIN_DP = {"kxx_matvec": 4, "kxx_grad": 4, "rff_sample": 4, "kmn_knm_vjp": 4, "knm_project": 2, "k_dense_vjp": 2}
API = {"kxx_matvec": "mgp_kxx_matvec", "kxx_grad": "mgp_kxx_grad", "rff_sample": "mgp_rff_sample / mgp_rff_features",
       "kmn_knm_vjp": "mgp_kmn_knm_vjp", "knm_project": "mgp_knm_project", "k_dense_vjp": "mgp_k_dense_vjp"}
ENTRIES = tuple(API)


def greedy(count, widths):
    """Cut `count` columns into passes, each the widest of `widths` (descending) that still fits what is left."""
    out, left = [], count
    while left:
        w = next(w for w in widths if left >= w)
        out.append(w)
        left -= w
    return out


# ---------------------------------------------------------------- mgp_kxx_matvec, symmetric form (csrc/kxx.hip)
KXX_THREADS = 256
KXX_WIDTHS = (8, 4, 2, 1)


def kxx_cfg(DP, RC):
    """KxxCfg<DP, RC>: (RPT owned rows per lane, TB = 256 RPT rows per block, G streamed points per store of the
    column sums)."""
    RPT = 4 if (RC == 1 and DP <= 8) else (2 if (DP <= 8 or (DP <= 16 and RC <= 4)) else 1)
    return RPT, KXX_THREADS * RPT, (16 if RC >= 4 else 64 // RC)


def kxx_cut(R):
    """kxx_dp: groups of 8, 4, 2, 1 columns, the widest first."""
    return greedy(R, KXX_WIDTHS)


# ---------------------------------------------------------------- mgp_kxx_grad, fused form (csrc/kxx_grad.hip)
KGRAD_TB = 256


def kgrad_rc_max(DP, kind):
    return 16 if DP <= 16 and kind != "matern12" else 8


def kgrad_cut(R, DP, kind):
    """kgrad_fused: passes of RCM, 8, 4, 2, 1 columns, the widest first."""
    return greedy(R, tuple(sorted({kgrad_rc_max(DP, kind), 8, 4, 2, 1}, reverse=True)))


# ---------------------------------------------------------------- mgp_rff_sample, fused route (csrc/rff.hip)
RFF_THREADS = 256
RFF_MAX_S = 8


def rff_rpt(DP):
    return 4 if DP <= 8 else (2 if DP <= 16 else 1)


def rff_chunks(N, L, DP, num_cus=NUM_CUS):
    """fused_launch: (chunks the bases are split into over blockIdx.y, bases per chunk); more than one chunk runs
    rff_reduce_kernel."""
    bx = ceil_div(N, RFF_THREADS * rff_rpt(DP))
    n, want = 1, 4 * num_cus
    if bx < want:
        n = max(1, min(ceil_div(want, bx), ceil_div(L, 32), 256))
    lchunk = ceil_div(L, n)
    return ceil_div(L, lchunk), lchunk


# ---------------------------------------------------------------- mgp_kmn_knm_vjp (csrc/kmn_grad.hip)
KVJP_THREADS = 256  # columns of Z per workgroup
KVJP_TR = 32        # rows per staged tile; a row block is a whole multiple of it
KVJP_P_FUSED = 12


def kvjp_pc_max(DP, kind):
    return 16 if kind != "matern12" else 8


def kvjp_form(has_gq, P):
    return "run" if has_gq else ("rank_fused" if P <= KVJP_P_FUSED else "rank_panel")


def kvjp_passes(P, DP, kind):
    """kvjp_rank_fused: [(width of the instantiation, live columns)]; a pass is the narrowest of 2, 4, 8, PCM that
    holds what is left."""
    pcm, out, left = kvjp_pc_max(DP, kind), [], P
    while left:
        w = pcm if left > 8 else (8 if left > 4 else (4 if left > 2 else 2))
        pc = min(left, w)
        out.append((w, pc))
        left -= pc
    return out


def vjp_row_blocks(rows, cols, num_cus=NUM_CUS):
    """kvjp_max_row_blocks + kvjp_row_blocks, and the same rule in vjp_t of csrc/grad.hip: (row blocks, rows per
    block) for `rows` rows against `cols` columns in blocks of 256."""
    ncb = ceil_div(cols, 256)
    n = max(1, min(ceil_div(4 * num_cus, ncb), ceil_div(rows, 32)))
    rpb = ceil_div(ceil_div(rows, n), 32) * 32
    return ceil_div(rows, rpb), rpb


# ---------------------------------------------------------------- mgp_knm_project, fused route (csrc/project.hip)
def project_tile(r):
    """(MT, NQ) of knm_project_kernel: 32 MT test rows and 32 NQ padded columns per workgroup."""
    return (4, 1) if r <= 32 else (4, 2) if r <= 64 else (4, 4) if r <= 128 else (2, 8)


PROJECT_TILES = ((4, 1), (4, 2), (4, 4), (2, 8))


# ---------------------------------------------------------------- the sets
def kind_class(entry, kind):
    """The kinds a rule tells apart: Matern-1/2 narrows the widest pass of the two gradient pair kernels."""
    if entry in ("kxx_grad", "kmn_knm_vjp"):
        return "matern12" if kind == "matern12" else "other"
    return "any"


def reachable(entry):
    """Every (form, DP, pass width, kind class, dtype) the restated rule of `entry` can pick."""
    out = set()
    for DP in rungs(MIN_DP[entry]):
        if entry == "kxx_matvec":
            out |= {("sym", DP, rc, "any", F64) for rc in KXX_WIDTHS}
        elif entry == "kxx_grad":
            for kind in KINDS:
                out |= {("fused", DP, rc, kind_class(entry, kind), F64)
                        for rc in {kgrad_rc_max(DP, kind), 8, 4, 2, 1}}
        elif entry == "rff_sample":
            out |= {("fused", DP, S, "any", dt) for S in range(1, RFF_MAX_S + 1) for dt in (F64, F32)}
        elif entry == "kmn_knm_vjp":
            for kind in KINDS:
                kc = kind_class(entry, kind)
                out |= {("rank_fused", DP, w, kc, F64) for w in {2, 4, 8, kvjp_pc_max(DP, kind)}}
            out |= {(form, DP, dz, "any", F64) for form in ("run", "rank_panel") for dz in ("dz", "nodz")}
        elif entry == "knm_project":
            out |= {("fused", DP, t, "any", F64) for t in PROJECT_TILES}
        elif entry == "k_dense_vjp":
            out |= {("fused", DP, 1, "any", dt) for dt in (F64, F32)}
    return out


def reached(case):
    c = case
    if c.entry == "kxx_matvec":
        return {("sym", c.DP, rc, "any", F64) for rc in kxx_cut(c.cols)}
    if c.entry == "kxx_grad":
        return {("fused", c.DP, rc, kind_class(c.entry, c.kind), F64) for rc in kgrad_cut(c.cols, c.DP, c.kind)}
    if c.entry == "rff_sample":
        return {("fused", c.DP, c.cols, "any", dt) for dt in c.dtypes}
    if c.entry == "kmn_knm_vjp":
        form = kvjp_form(c.opts["gq"], c.cols)
        if form == "rank_fused":
            return {(form, c.DP, w, kind_class(c.entry, c.kind), F64) for w, _ in kvjp_passes(c.cols, c.DP, c.kind)}
        return {(form, c.DP, dz, "any", F64) for dz in ("dz", "nodz")}  # every case runs with dZ and without
    if c.entry == "knm_project":
        return {("fused", c.DP, project_tile(c.cols), "any", F64)}
    return {("fused", c.DP, 1, "any", dt) for dt in c.dtypes}


# ---------------------------------------------------------------- the case table
class Case:
    """entry, id, kind, D, DP; cols: the column count (R, P, S or r); dtypes the case runs in; shape: name -> length;
    tiles: axis -> (length, tile of the instantiation(s) the case names); opts: the entry point's own."""

    def __init__(self, entry, kind, D, cols, shape, tiles, dtypes=(F64,), tag="", **opts):
        self.entry, self.kind, self.D, self.cols = entry, kind, D, cols
        self.DP = with_dp(D, MIN_DP[entry])
        self.shape, self.tiles, self.dtypes, self.opts = shape, tiles, dtypes, opts
        self.id = f"{entry}-D{D}-{kind}-c{cols}" + (f"-{tag}" if tag else "")

    def __repr__(self):
        return self.id


def three_blocks(tile, extra=1):
    """Two whole blocks of `tile` and a ragged third."""
    return 2 * tile + extra


def _kxx_cases():
    out = []
    for i, DP in enumerate(rungs(4)):
        bottom, top = rung_ds(DP)
        # the top of the rung with every group width (15 = 8 + 4 + 2 + 1); one past the rung below with one group
        for j, (D, R) in enumerate(((bottom, (1, 2, 8, 4)[i]), (top, 15))):
            tbs = sorted({kxx_cfg(DP, rc)[1] for rc in kxx_cut(R)})
            N = three_blocks(tbs[-1])  # ragged against every narrower block of the same call as well
            k = 2 * i + j
            out.append(Case("kxx_matvec", KINDS[(k + k // 4) % 4], D, R, {"N": N},
                            {f"rows/{tb}": (N, tb) for tb in tbs}))
    return out


def _kgrad_cases():
    out, other = [], [k for k in KINDS if k != "matern12"]
    N = three_blocks(KGRAD_TB)
    for i, DP in enumerate(rungs(4)):
        bottom, top = rung_ds(DP)
        rcm = kgrad_rc_max(DP, "se")
        rows = [(top, other[i % 3], 2 * rcm - 1),        # every width of the rung: 16 + 8 + 4 + 2 + 1 or 8 + 4 + 2 + 1
                (bottom, other[(i + 1) % 3], rcm),       # one pass
                ((bottom, top)[i % 2], "matern12", 15)]  # Matern-1/2: 8 + 4 + 2 + 1 on every rung
        for D, kind, R in rows:
            out.append(Case("kxx_grad", kind, D, R, {"N": N}, {"rows": (N, KGRAD_TB)}))
    return out


def _rff_cases():
    out = []
    for i, DP in enumerate(rungs(4)):
        bottom, top = rung_ds(DP)
        N = three_blocks(RFF_THREADS * rff_rpt(DP))
        for S in range(1, RFF_MAX_S + 1):
            L = 100 if (S // 2 + i) % 2 else 29  # 100 bases: four chunks over blockIdx.y and the reduce; 29: one launch
            out.append(Case("rff_sample", "se", top if S % 2 else bottom, S, {"N": N, "L": L},
                            {"rows": (N, RFF_THREADS * rff_rpt(DP))}, dtypes=(F64, F32), tag=f"L{L}",
                            layout=(S + i) % 2, chunks=rff_chunks(N, L, DP)[0]))
    return out


def _kvjp_cases():
    out = []
    N, M = 4 * KVJP_TR + 3, KVJP_THREADS + 44
    shape, tiles = {"N": N, "M": M}, {"rows": (N, KVJP_TR), "cols": (M, KVJP_THREADS)}
    other = [k for k in KINDS if k != "matern12"]
    for i, DP in enumerate(rungs(4)):
        bottom, top = rung_ds(DP)
        # the Gq form (K panel, GEMM, pair kernel with and without dZ): both ends of the rung
        out.append(Case("kmn_knm_vjp", KINDS[i % 4], bottom, 3, shape, tiles, tag="gq", gq=True))
        out.append(Case("kmn_knm_vjp", KINDS[(i + 2) % 4], top, 0, shape, tiles, tag="gq", gq=True))
        # Gq = NULL inside the fused range: full passes of 2, 4, 8, 16 at the top, ragged ones (1, 3, 7, 11 live
        # columns) one past the rung below; Matern-1/2: 8 + 4 and 8 + 2
        for j, (Pt, Pb) in enumerate(((2, 1), (4, 3), (8, 7), (12, 11))):
            D, P = ((top, Pt), (bottom, Pb))[(i + j) % 2]
            out.append(Case("kmn_knm_vjp", other[(i + j) % 3], D, P, shape, tiles, tag="rank", gq=False))
        out.append(Case("kmn_knm_vjp", "matern12", top, 12, shape, tiles, tag="rank", gq=False))
        out.append(Case("kmn_knm_vjp", "matern12", bottom, 10 - i % 2, shape, tiles, tag="rank", gq=False))
        # one P beyond kVjpPFused: the W panel of the GEMM
        out.append(Case("kmn_knm_vjp", KINDS[(i + 1) % 4], (top, bottom)[i % 2], KVJP_P_FUSED + 1, shape, tiles,
                        tag="rank", gq=False))
    return out


def _project_cases():
    out = []
    N = 1024 + 5  # two splits of N (the rule allows one per 1024 rows of X), ragged against the 16-row step
    for i, DP in enumerate(rungs(2)):
        bottom, top = rung_ds(DP)
        for j, r in enumerate((17, 64, 100, 200)):  # one width per (MT, NQ); 64 fills its tile, the others are ragged
            D = (bottom, top)[(i + j) % 2]
            PB = sp.project_fused(1, N, D, r).PB
            B = three_blocks(PB)
            pl = sp.project_fused(B, N, D, r)
            out.append(Case("knm_project", KINDS[(i + j) % 4], D, r, {"B": B, "N": N},
                            {"rows": (B, pl.PB), "steps": (N, sp.PJ_STEP)}, layout=(i + j // 2) % 2,
                            splits=pl.launches[0][2], RP=pl.RP))
    return out


def _dense_cases():
    out = []
    na, nb = 4 * 32 + 3, three_blocks(256)
    k = 0
    for DP in rungs(2):
        for D in rung_ds(DP):
            out.append(Case("k_dense_vjp", KINDS[k % 4], D, 1, {"na": na, "nb": nb},
                            {"rows": (na, 32), "cols": (nb, 256)}, dtypes=(F64, F32)))
            k += 1
    return out


CASES = _kxx_cases() + _kgrad_cases() + _rff_cases() + _kvjp_cases() + _project_cases() + _dense_cases()


def cases(entry):
    return [c for c in CASES if c.entry == entry]


# ---------------------------------------------------------------- already complete on the ladder (not run again here)
# entry point -> (test that holds it, where its dimension list stands, the list)
COMPLETE = {
    "mgp_knm_matvec / mgp_kmn_matvec, VALU forms":
        ("tests/test_gpu_switch_forms.py::test_sweep_form", "tests/switch_forms.py::VALU_CASES",
         (1, 3, 8, 9, 16, 17, 32)),
    "mgp_knm_matvec / mgp_kmn_matvec, matrix-core forms (one per KS = (D + 5) / 4)":
        ("tests/test_gpu_switch_forms.py::test_sweep_form", "tests/switch_forms.py::MFMA_CASES",
         (2, 6, 10, 14, 18, 22, 26, 30, 32)),
    "mgp_nearest_center":
        ("tests/test_gpu_assign.py::test_fused_route", "tests/assign_reference.py::FUSED_DS",
         (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)),
    "mgp_kmn_sq_colsum":
        ("tests/test_gpu_switch_forms.py::test_kmn_sq_colsum", "tests/test_gpu_switch_forms.py::test_kmn_sq_colsum",
         (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)),
    "MGP_OP_KMM_LAMBDA_WIDE (the wide K_mm + Lambda operator)":
        ("tests/test_gpu_kmm_wide.py::test_products_against_long_double", "tests/kmm_wide_reference.py::PRODUCT_D",
         (1, 3, 8, 9, 32)),
}
