"""The chunk rules of the routes that cut their work into panels, restated, and the shapes that cross every cut.

Each rule below is the host arithmetic of one csrc function (budget, clamps, rounding, in the order the code applies
them).  For a shape it gives the cut positions on each axis and the bytes the rule asks of its arena, so that
tests/test_gpu_seams.py can prove with `mgp_arena_bytes` that the library crossed the cuts the plan names: if a budget
changes, the proof fails instead of the test quietly running on one panel.  tests/test_seam_plan.py checks on the CPU
that every planned case does cross what it claims and that the checked rows and columns sit on both sides of each cut.
"""

import numpy as np

BUDGET = 1 << 28       # bytes of one panel: csrc/generic.hip:130 and :506, csrc/project.hip:306, csrc/kxx_grad.hip:193, csrc/rff.hip:24
STREAM = 16384         # streamed points per panel: csrc/generic.hip:129, csrc/project.hip:305
PJ_CHUNK_B = 1 << 16   # test rows per launch of the fused projection: csrc/project.hip:27
PJ_STEP = 16           # rows of X per step of the fused projection (PK): csrc/project.hip:24
NOMINAL_CUS = 256      # compute units of an MI355X; the fused projection's split of N depends on them
KINDS = ("se", "matern12", "matern32", "matern52")


def elem(dtype):
    return np.dtype(dtype).itemsize


def cuts(n, step):
    """The interior chunk boundaries of range(0, n, step)."""
    return list(range(step, n, step))


class Plan:
    """axes: name -> (length, cuts); chunk: name -> chunk length; arena: (name of the handle's arena, bytes asked);
    whole: bytes one panel over the whole shape would take."""

    def __init__(self, axes, chunk, arena, whole):
        self.axes, self.chunk, self.arena, self.whole = axes, chunk, arena, whole

    def cuts(self, axis):
        return self.axes[axis][1]


def sweep_generic(na, nb, R, dtype):
    """sweep_generic_t, csrc/generic.hip:129-134 (chunk rule and arena) and :141-144 (loops): `na` owned rows, `nb`
    streamed points, arena `gen` = Wt [R, nb] | panel [rc, sc] | oc [R, rc]."""
    e = elem(dtype)
    sc = min(nb, STREAM)
    rc = BUDGET // (sc * e)
    rc = min(rc, na)
    rc = max(rc, 64)
    need = (R * nb + rc * sc + R * rc) * e + 256
    return Plan({"owned": (na, cuts(na, rc)), "streamed": (nb, cuts(nb, sc))}, {"owned": rc, "streamed": sc},
                ("gen", need), na * nb * e)


def sq_colsum_generic(N, M, dtype):
    """sq_colsum_generic_t, csrc/generic.hip:506-512 and :516: row chunks of X, a multiple of 256 rows, arena `gen` =
    panel [rc, M] | part [rc / 256, M]."""
    e = elem(dtype)
    rc = BUDGET // (M * e)
    rc = min(rc, N)
    rc = max(rc, 256)
    rc = rc // 256 * 256
    need = (rc * M + (rc // 256) * M) * e + 256
    return Plan({"rows": (N, cuts(N, rc))}, {"rows": rc}, ("gen", need), N * M * e)


def project_generic(B, N, r, dtype, cols_layout, want_proj):
    """project_generic, csrc/project.hip:305-311 and :322-326: test-row chunks x streamed chunks of X, arena `prj` =
    Rt [r, N] (COLS layout only) | panel [rc, sc] | pc [rc, r] (without proj only)."""
    e = elem(dtype)
    sc = min(N, STREAM)
    rc = BUDGET // (sc * e)
    rc = max(rc, 64)
    rc = min(rc, B)
    need = ((r * N if cols_layout else 0) + rc * sc + (0 if want_proj else rc * r)) * e + 256
    return Plan({"owned": (B, cuts(B, rc)), "streamed": (N, cuts(N, sc))}, {"owned": rc, "streamed": sc},
                ("prj", need), B * N * e)


def _pj_split(tiles, N, num_cus):
    """pj_plan, csrc/project.hip:244-254: (number of splits of N, rows per split)."""
    ns = (4 * num_cus + tiles - 1) // tiles
    ns = max(1, min(ns, (N + 1023) // 1024))
    rw = (N + ns - 1) // ns
    rw = (rw + PJ_STEP - 1) // PJ_STEP * PJ_STEP
    ns = max(1, (N + rw - 1) // rw)
    return ns, rw


def project_fused(B, N, D, r, num_cus=NOMINAL_CUS):
    """project_fused_dp, csrc/project.hip:260-283 (fp64, D <= 32, r <= 256): one launch per 2^16 test rows; every
    launch splits N by `_pj_split` into the shared arena `prj` = part [max over launches of splits x tiles x PB x RP]
    (rounded up to 256 bytes) | Xp [N, DP + 1].  `launches`: (first row, rows, splits, rows of X per split).  `whole`
    is what ONE launch over all B rows would ask for."""
    RP = (r + 15) // 16 * 16
    PB = 128 if r <= 128 else 64
    DP = next(p for p in (2, 4, 8, 16, 32) if p >= D)  # mgp_with_dp, csrc/mgp_common.h:296-306

    def part_bytes(rows):
        tiles = (rows + PB - 1) // PB
        ns, rw = _pj_split(tiles, N, num_cus)
        return ns * tiles * PB * RP * 8, ns, rw

    launches, part = [], 0
    for c0 in range(0, B, PJ_CHUNK_B):
        rows = min(B - c0, PJ_CHUNK_B)
        b, ns, rw = part_bytes(rows)
        part = max(part, b)
        launches.append((c0, rows, ns, rw))
    part = (part + 255) // 256 * 256
    xp = N * (DP + 1) * 8
    split_cuts = sorted({c for _, _, _, rw in launches for c in cuts(N, rw)})
    plan = Plan({"owned": (B, cuts(B, PJ_CHUNK_B)), "streamed": (N, split_cuts)},
                {"owned": PJ_CHUNK_B, "streamed": max(rw for _, _, _, rw in launches)}, ("prj", part + xp),
                B * N * 8)
    plan.launches = launches
    plan.PB, plan.RP, plan.DP = PB, RP, DP  # the instantiation's tile (tests/ladder_plan.py)
    return plan


def kgrad_panel(N, dtype):
    """kgrad_panel, csrc/kxx_grad.hip:193-196 and :200-201: row panels of G = U V^T, arena `kgrad` = G [rows, N]."""
    e = elem(dtype)
    rows = (BUDGET // e) // N
    rows = max(1, min(rows, N))
    return Plan({"rows": (N, cuts(N, rows))}, {"rows": rows}, ("kgrad", rows * N * e), N * N * e)


def rff_panel_rows(L, dtype):
    """sample_panel_t, csrc/rff.hip:238-241: rows of Phi [rows, 2 L] per panel (before the clamps to N and 64)."""
    return BUDGET // (2 * L * elem(dtype))


def arena_window(plan):
    """[low, high] for `mgp_arena_bytes` after the call on a fresh growing handle; 256 for a rounding a rule may add."""
    need = plan.arena[1]
    return need, 1.25 * need + 4096 + 256


def reserved_bytes(need):
    """What `mgp_reserve` (csrc/mgp_common.h:256) allocates on a growing handle for a first request of `need` bytes,
    and so what `mgp_arena_bytes` reports: a quarter more, plus 4 KiB."""
    return need + (need >> 2) + 4096


def asked_bytes(reserved):
    """The request behind a reported arena size, to within a byte (the inverse of `reserved_bytes`)."""
    return (reserved - 4096) / 1.25


def check_indices(n, cut_list, seed, extra=8):
    """For every cut c the indices c - 1, c, c + 1; the first and the last index; and `extra` seeded random ones drawn
    from the rest (so they are always `extra` more, as long as n allows)."""
    rng = np.random.default_rng([seed, n])
    idx = {0, n - 1}
    for c in cut_list:
        idx.update(i for i in (c - 1, c, c + 1) if 0 <= i < n)
    rest = np.setdiff1d(np.arange(n), np.fromiter(idx, dtype=np.int64))
    idx.update(int(i) for i in rng.choice(rest, min(extra, len(rest)), replace=False))
    return np.array(sorted(idx), dtype=np.int64)


def few_hot_indices(n, cut_list, seed, target=40):
    """The support of a few-hot multiplier over a contraction axis: `check_indices` filled up with seeded random
    indices to about `target`."""
    base = check_indices(n, cut_list, seed, extra=0)
    return check_indices(n, cut_list, seed + 1, extra=max(8, target - len(base)))


# ---------------------------------------------------------------- the case table (the smallest shapes crossing each cut)
F64, F32 = np.float64, np.float32


def _rot(i):
    return KINDS[i % 4]


API = {"sweep": "mgp_knm_matvec / mgp_kmn_matvec", "kxx_matvec": "mgp_kxx_matvec", "sq_colsum": "mgp_kmn_sq_colsum",
       "project_generic": "mgp_knm_project", "project_fused": "mgp_knm_project", "kxx_grad": "mgp_kxx_grad"}


class Case:
    def __init__(self, entry, ident, kind, dtype, D, shape, plan, targeted, **opts):
        self.entry, self.id, self.kind, self.dtype, self.D = entry, ident, kind, np.dtype(dtype), D
        self.shape, self.plan, self.targeted, self.opts = shape, plan, targeted, opts
        self.api = API[entry]

    def rows(self, axis, seed=0):
        n, cl = self.plan.axes[axis]
        return check_indices(n, cl, seed)

    def support(self, axis, seed=0):
        n, cl = self.plan.axes[axis]
        return few_hot_indices(n, cl, seed)

    def __repr__(self):
        return self.id


def _cases():
    out = []
    # knm_matvec / kmn_matvec: owned x streamed; the arena is sized by the widest multiplier, R = 3
    sweeps = [(F64, 33, 4101, 16421, ("owned", "streamed")), (F64, 77, 4101, 16421, ("owned", "streamed")),
              (F32, 33, 8197, 16421, ("owned", "streamed")), (F64, 33, 7010, 5000, ("owned",))]
    for i, (dt, D, na, nb, tg) in enumerate(sweeps):
        out.append(Case("sweep", f"sweep-{np.dtype(dt).name}-D{D}-{na}x{nb}", _rot(i), dt, D, (na, nb),
                        sweep_generic(na, nb, 3, dt), tg))
    # mgp_kxx_matvec: 9 row chunks x 2 streamed; and N = 7010, whose row chunk (4786) is not a power of two
    for i, (N, tg) in enumerate([(16421, ("owned", "streamed")), (7010, ("owned",))]):
        out.append(Case("kxx_matvec", f"kxx_matvec-float64-D33-{N}", _rot(1 + i), F64, 33, (N, N),
                        sweep_generic(N, N, 3, F64), tg))
    for i, (N, M) in enumerate([(4396, 16384), (6913, 5000)]):
        out.append(Case("sq_colsum", f"sq_colsum-float64-D33-{N}x{M}", _rot(2 + i), F64, 33, (N, M),
                        sq_colsum_generic(N, M, F64), ("rows",)))
    i = 0
    for dt, D, r in ((F64, 33, 17), (F64, 8, 257), (F32, 5, 64)):
        B = 8197 if dt == F32 else 4101
        for cols_layout in (True, False):
            for want_proj in (True, False):
                tag = f"{np.dtype(dt).name}-D{D}-r{r}-{'cols' if cols_layout else 'rows'}-{'proj' if want_proj else 'sq'}"
                out.append(Case("project_generic", "project_generic-" + tag, _rot(i), dt, D, (B, 16421),
                                project_generic(B, 16421, r, dt, cols_layout, want_proj), ("owned", "streamed"), r=r,
                                cols_layout=cols_layout, want_proj=want_proj))
                i += 1
    # a test-row chunk that is no power of two (6710 of 7010 rows), as the sweep's 7010 x 5000
    out.append(Case("project_generic", "project_generic-float64-D33-r17-cols-proj-7010x5000", _rot(i), F64, 33, (7010, 5000),
                    project_generic(7010, 5000, 17, F64, True, True), ("owned",), r=17, cols_layout=True, want_proj=True))
    for i, r in enumerate((17, 256)):
        B, N = PJ_CHUNK_B + 200, 3000
        out.append(Case("project_fused", f"project_fused-float64-D3-r{r}", _rot(i), F64, 3, (B, N),
                        project_fused(B, N, 3, r), ("owned",), r=r))
    for i, (dt, D, N, forced) in enumerate([(F64, 33, 6000, False), (F32, 3, 8500, False), (F64, 8, 6000, True)]):
        out.append(Case("kxx_grad", f"kxx_grad-{np.dtype(dt).name}-D{D}-{N}", _rot(3 + i), dt, D, (N, N),
                        kgrad_panel(N, dt), ("rows",), forced=forced))
    return out


CASES = _cases()


def cases(entry):
    return [c for c in CASES if c.entry == entry]
