"""The ladder plan on the CPU (tests/ladder_plan.py; the values are checked by tests/test_gpu_ladder.py): for every
entry point the instantiations its cases reach are exactly the ones its restated rule can pick, every case's shape
crosses the tile seams it states, and every restated rule still stands in csrc/ as the expression it was read from (a
changed rule fails here; an unrelated edit to the same file does not)."""

import os
import re

import pytest

import ladder_plan as lp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")


def source(name):
    """A source file with every run of white space collapsed to one blank."""
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


# ---------------------------------------------------------------- 1. reached == reachable
@pytest.mark.parametrize("entry", lp.ENTRIES)
def test_cases_reach_every_instantiation_the_rule_can_pick(entry):
    got = set().union(*(lp.reached(c) for c in lp.cases(entry)))
    want = lp.reachable(entry)
    assert got == want, (sorted(want - got, key=str), sorted(got - want, key=str))


def test_the_reachable_sets_are_the_ones_the_source_compiles():
    n = {e: len(lp.reachable(e)) for e in lp.ENTRIES}
    # kxx: 4 rungs x 4 groups; kxx_grad: 3 rungs x (5 + 4 widths) + rung 32 x 2 x 4; rff: 4 rungs x 8 widths x 2 types;
    # vjp: 4 rungs x (4 + 3 fused widths + 2 forms x dZ on / off); projection: 5 rungs x 4 tiles; dense VJP: 5 x 2 types
    assert n == {"kxx_matvec": 16, "kxx_grad": 35, "rff_sample": 64, "kmn_knm_vjp": 44, "knm_project": 20,
                 "k_dense_vjp": 10}


@pytest.mark.parametrize("entry", lp.ENTRIES)
def test_every_rung_at_its_top_and_one_past_the_rung_below(entry):
    ds = {c.D for c in lp.cases(entry)}
    for DP in lp.rungs(lp.MIN_DP[entry]):
        bottom, top = lp.rung_ds(DP)
        assert {bottom, top} <= ds, (entry, DP)
        assert lp.with_dp(bottom, lp.MIN_DP[entry]) == lp.with_dp(top, lp.MIN_DP[entry]) == DP
        if bottom > 1:
            assert lp.with_dp(bottom - 1) < DP  # one less is the rung below (on the full ladder)


def test_ladder():
    assert [lp.with_dp(D) for D in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [lp.with_dp(D, 4) for D in (1, 2, 3, 4, 5)] == [4, 4, 4, 4, 8]
    assert [lp.rung_ds(p) for p in lp.RUNGS] == [(1, 2), (3, 4), (5, 8), (9, 16), (17, 32)]
    with pytest.raises(AssertionError):
        lp.with_dp(33)


@pytest.mark.parametrize("entry", lp.ENTRIES)
def test_kinds_rotate_and_matern12_stands_where_it_changes_the_widths(entry):
    cs = lp.cases(entry)
    if entry == "rff_sample":  # no kernel kind: theta is the caller's
        return
    assert {c.kind for c in cs} == set(lp.KINDS), entry
    if entry in ("kxx_grad", "kmn_knm_vjp"):
        for DP in lp.rungs(4):
            assert any(c.kind == "matern12" and c.DP == DP for c in cs), (entry, DP)
    assert any(c.kind == "matern12" and c.DP <= 16 for c in cs)
    assert len({c.id for c in lp.CASES}) == len(lp.CASES)


# ---------------------------------------------------------------- 2. column counts: every width, and a single pass
def test_column_counts_per_rung():
    for DP in lp.rungs(4):
        kx = [lp.kxx_cut(c.cols) for c in lp.cases("kxx_matvec") if c.DP == DP]
        assert [8, 4, 2, 1] in kx and any(len(cut) == 1 for cut in kx)
        kg = [(c.kind, lp.kgrad_cut(c.cols, DP, c.kind)) for c in lp.cases("kxx_grad") if c.DP == DP]
        rcm = lp.kgrad_rc_max(DP, "se")
        assert any(k != "matern12" and cut == sorted({rcm, 8, 4, 2, 1}, reverse=True) for k, cut in kg)
        assert any(k != "matern12" and cut == [rcm] for k, cut in kg)
        assert ("matern12", [8, 4, 2, 1]) in kg
        vj = [c for c in lp.cases("kmn_knm_vjp") if c.DP == DP]
        assert {lp.kvjp_form(c.opts["gq"], c.cols) for c in vj} == {"run", "rank_fused", "rank_panel"}
        assert {c.cols for c in vj if not c.opts["gq"] and c.cols > lp.KVJP_P_FUSED} == {lp.KVJP_P_FUSED + 1}
        passes = [tuple(lp.kvjp_passes(c.cols, DP, c.kind)) for c in vj if c.opts["gq"] is False and c.cols <= 12]
        assert ((8, 8), (4, 4)) in passes and (((8, 8), (2, 2)) in passes or ((8, 8), (2, 1)) in passes)  # Matern-1/2
        live = {p for ps in passes for p in ps}
        for w in (2, 4, 8, 16):  # a full pass or a ragged one of every width on every rung
            assert any(p[0] == w for p in live), (DP, w)
    live = {p for c in lp.cases("kmn_knm_vjp") if not c.opts["gq"] and c.cols <= 12
            for p in lp.kvjp_passes(c.cols, c.DP, c.kind)}
    assert {(2, 2), (2, 1), (4, 4), (4, 3), (8, 8), (8, 7), (16, 12), (16, 11)} <= live
    assert lp.kxx_cut(15) == [8, 4, 2, 1] and lp.kxx_cut(11) == [8, 2, 1]
    assert lp.kgrad_cut(31, 16, "se") == [16, 8, 4, 2, 1] and lp.kgrad_cut(31, 16, "matern12") == [8, 8, 8, 4, 2, 1]
    assert lp.kgrad_cut(6, 8, "se") == [4, 2] and lp.kgrad_cut(16, 32, "se") == [8, 8]
    assert lp.kvjp_passes(12, 4, "matern12") == [(8, 8), (4, 4)]
    assert lp.kvjp_passes(9, 4, "matern12") == [(8, 8), (2, 1)]
    assert lp.kvjp_passes(12, 4, "se") == [(16, 12)] and lp.kvjp_passes(5, 32, "se") == [(8, 5)]


def test_rff_widths_types_layouts_and_the_split_over_the_bases():
    cs = lp.cases("rff_sample")
    for DP in lp.rungs(4):
        mine = [c for c in cs if c.DP == DP]
        assert sorted(c.cols for c in mine) == list(range(1, 9))
        assert {c.opts["layout"] for c in mine} == {0, 1}
        assert {c.opts["chunks"] for c in mine} == {1, 4}  # the direct store and rff_reduce_kernel on every rung
        assert all(c.dtypes == (lp.F64, lp.F32) for c in mine)
    for c in cs:  # the split is the rule's at any plausible CU count, not an accident of 256
        for cus in (64, 228, 256, 304):
            assert lp.rff_chunks(c.shape["N"], c.shape["L"], c.DP, cus)[0] == c.opts["chunks"]
    assert lp.rff_chunks(100_003, 1024, 8) == (11, 94) and lp.rff_chunks(257, 1024, 8) == (32, 32)


# ---------------------------------------------------------------- 3. shapes cross the seams they state
@pytest.mark.parametrize("case", lp.CASES, ids=repr)
def test_shape_fills_the_instantiation(case):
    assert case.tiles
    for axis, (n, tile) in case.tiles.items():
        assert n in case.shape.values(), (case.id, axis)
        assert lp.ceil_div(n, tile) >= 2 and n % tile != 0, (case.id, axis, n, tile)  # more than one block, ragged
    c = case
    if c.entry == "kxx_matvec":
        want = {f"rows/{lp.kxx_cfg(c.DP, rc)[1]}" for rc in lp.kxx_cut(c.cols)}
        assert set(c.tiles) == want
        n, tile = c.tiles[f"rows/{max(lp.kxx_cfg(c.DP, rc)[1] for rc in lp.kxx_cut(c.cols))}"]
        assert lp.ceil_div(n, tile) == 3  # three row blocks: the diagonal tile, a full pair and the ragged block
    elif c.entry == "kxx_grad":
        assert c.tiles["rows"] == (c.shape["N"], 256) and lp.ceil_div(c.shape["N"], 256) == 3
    elif c.entry == "rff_sample":
        assert c.tiles["rows"] == (c.shape["N"], 256 * lp.rff_rpt(c.DP)) and lp.ceil_div(*c.tiles["rows"]) == 3
        assert c.shape["N"] % 256 == 1  # the last block's rows run past N in every strided slot but the first
    elif c.entry == "kmn_knm_vjp":
        nrb, rpb = lp.vjp_row_blocks(c.shape["N"], c.shape["M"])
        assert nrb >= 3 and rpb == c.tiles["rows"][1] and c.shape["N"] - (nrb - 1) * rpb < rpb
        assert c.tiles["cols"] == (c.shape["M"], 256)
    elif c.entry == "knm_project":
        import seam_plan as sp
        pl = sp.project_fused(c.shape["B"], c.shape["N"], c.D, c.cols)
        assert (pl.DP, pl.PB, pl.RP) == (c.DP, c.tiles["rows"][1], c.opts["RP"])
        assert pl.PB == 32 * lp.project_tile(c.cols)[0] and lp.ceil_div(c.shape["B"], pl.PB) == 3
        (_, rows, ns, rw), = pl.launches
        assert ns == c.opts["splits"] >= 2 and 0 < c.shape["N"] - (ns - 1) * rw < rw
        for cus in (228, 304):
            assert sp.project_fused(c.shape["B"], c.shape["N"], c.D, c.cols, cus).launches[0][2] == ns
    else:
        nrb, rpb = lp.vjp_row_blocks(c.shape["na"], c.shape["nb"])
        assert nrb >= 3 and rpb == 32 and lp.ceil_div(c.shape["nb"], 256) == 3


def test_projection_column_tiles():
    rs = {}
    for c in lp.cases("knm_project"):
        rs.setdefault(lp.project_tile(c.cols), set()).add(c.cols)
    assert set(rs) == set(lp.PROJECT_TILES)
    assert any(r % 16 for v in rs.values() for r in v) and any(r % 32 == 0 for v in rs.values() for r in v)
    assert [lp.project_tile(r) for r in (1, 32, 33, 64, 65, 128, 129, 256)] == \
        [(4, 1), (4, 1), (4, 2), (4, 2), (4, 4), (4, 4), (2, 8), (2, 8)]


# ---------------------------------------------------------------- 4. the restated rules stand in the source
PINS = [
    # the ladder
    ("mgp_common.h", "template <int MIN_DP = 2, typename F> inline int mgp_with_dp(int D, F&& f) { "
                     "if constexpr (MIN_DP <= 2) if (D <= 2) return f(std::integral_constant<int, 2>{}); "
                     "if constexpr (MIN_DP <= 4) if (D <= 4) return f(std::integral_constant<int, 4>{}); "
                     "if constexpr (MIN_DP <= 8) if (D <= 8) return f(std::integral_constant<int, 8>{}); "
                     "if constexpr (MIN_DP <= 16) if (D <= 16) return f(std::integral_constant<int, 16>{}); "
                     "return f(std::integral_constant<int, 32>{}); }"),
    # KxxCfg and the column groups of kxx_dp
    ("kxx.hip", "constexpr int kKxxThreads = 256;"),
    ("kxx.hip", "static constexpr int RPT = (RC == 1 && DP <= 8) ? 4 : ((DP <= 8 || (DP <= 16 && RC <= 4)) ? 2 : 1);"),
    ("kxx.hip", "static constexpr int TB = kKxxThreads * RPT;"),
    ("kxx.hip", "static constexpr int G = RC >= 4 ? 16 : 64 / RC;"),
    ("kxx.hip", "if (left >= 8) { rc = 8; MGP_TRY(MGP_KXX_GROUP(8)); } else if (left >= 4) { rc = 4; "
                "MGP_TRY(MGP_KXX_GROUP(4)); } else if (left >= 2) { rc = 2; MGP_TRY(MGP_KXX_GROUP(2)); } "
                "else { rc = 1; MGP_TRY(MGP_KXX_GROUP(1)); }"),
    ("kxx.hip", "constexpr int RPT = KxxCfg<DP, RC>::RPT, TB = KxxCfg<DP, RC>::TB, NT = kKxxThreads, NROW = NT / 16;"),
    # kgrad_rc_max and its greedy cut
    ("kxx_grad.hip", "constexpr int kKgThreads = 256; constexpr int kKgTB = kKgThreads;"),
    ("kxx_grad.hip", "constexpr int kgrad_rc_max(int DP, int KIND) { return DP <= 16 && KIND != 1 ? 16 : 8; }"),
    ("kxx_grad.hip", "const int rc = left >= RCM ? RCM : (left >= 8 ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1)));"),
    ("kxx_grad.hip", "case 16: MGP_TRY((kgrad_pass<DP, KIND, kgrad_rc_max(DP, KIND)>"),
    ("kxx_grad.hip", "case 2: MGP_TRY((kgrad_pass<DP, KIND, 2>"),
    # the RFF rows per lane and the switch over S
    ("rff.hip", "constexpr int kRffThreads = 256; constexpr int kRffMaxS = 8;"),
    ("rff.hip", "constexpr int RPT = DP <= 8 ? 4 : (DP <= 16 ? 2 : 1);"),
    ("rff.hip", "MGP_RFF_S(1); MGP_RFF_S(2); MGP_RFF_S(3); MGP_RFF_S(4); MGP_RFF_S(5); MGP_RFF_S(6); MGP_RFF_S(7); "
                "MGP_RFF_S(8);"),
    ("rff.hip", "if (D > MGP_FUSED_MAX_D || S > kRffMaxS) return false;"),
    ("rff.hip", "const long want = 4L * h->num_cus; if (bx < want) { nchunks = (want + bx - 1) / bx; "
                "const long cap = (L + 31) / 32; if (nchunks > cap) nchunks = cap; if (nchunks > 256) nchunks = 256;"),
    # the three forms of the VJP and the pass widths of the fused rank-P form
    ("kmn_grad.hip", "constexpr int kVjpThreads = 256;"),
    ("kmn_grad.hip", "constexpr int kVjpTR = 32;"),
    ("kmn_grad.hip", "#define MGP_KVJP_P_FUSED 12 #endif constexpr int kVjpPFused = MGP_KVJP_P_FUSED;"),
    ("kmn_grad.hip", "constexpr int kvjp_pc_max(int DP, int KIND) { return KIND != 1 ? 16 : 8; }"),
    ("kmn_grad.hip", "const int w = left > 8 ? PCM : (left > 4 ? 8 : (left > 2 ? 4 : 2)); "
                     "const int pc = left < w ? left : w;"),
    ("kmn_grad.hip", "if (P <= kVjpPFused) return kvjp_rank_fused<DP, KIND>"),
    ("kmn_grad.hip", "return kvjp_rank_panel<DP, KIND>"),
    ("kmn_grad.hip", "long n = (4L * h->num_cus + ncb - 1) / ncb; const long cap = (rows + kVjpTR - 1) / kVjpTR;"),
    # the tile of the fused projection
    ("project.hip", "const int D = k->D, RP = (r + 15) / 16 * 16; const int PB = r <= 128 ? 128 : 64;"),
    ("project.hip", "if (r <= 32) MGP_PJ(4, 1); else if (r <= 64) MGP_PJ(4, 2); else if (r <= 128) MGP_PJ(4, 4); "
                    "else MGP_PJ(2, 8);"),
    ("project.hip", "constexpr int PB = 32 * MT;"),
    ("project.hip", "if (k->dtype == MGP_F32 || k->D > MGP_FUSED_MAX_D || r > PJ_MAX_R)"),
    # the dense VJP: the whole ladder in the element type of the call
    ("grad.hip", "return mgp_with_dp(D, [&](auto dp) { constexpr int DP = decltype(dp)::value;"),
    ("grad.hip", "hipLaunchKernelGGL((k_dense_vjp_kernel<T, DP, decltype(kind)::value>), grid, dim3(256)"),
    ("grad.hip", "constexpr int TA = 32;"),
    ("grad.hip", "const long max_y = (na + 31) / 32;"),
]


PINNED_TWICE = ("if (r <= 32) MGP_PJ(4, 1); else if (r <= 64) MGP_PJ(4, 2); else if (r <= 128) MGP_PJ(4, 4); "
                "else MGP_PJ(2, 8);", "const int PB = r <= 128 ? 128 : 64;")


@pytest.mark.parametrize("name,text", PINS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(PINS)])
def test_restated_rule_stands_in_the_source(name, text):
    """Every pinned expression stands exactly once; the projection's (MT, NQ) dispatch stands twice, in
    project_fused_dp and in the wide K_mm + Lambda operator (kmm_wide_dp), so an edit to either copy changes the
    count (its PB line is pinned together with the RP line before it, which only project_fused_dp has)."""
    want = 2 if text in PINNED_TWICE else 1
    assert source(name).count(text) == want, \
        f"csrc/{name} holds `{text}` {source(name).count(text)} times, not {want}: restate the rule in tests/ladder_plan.py"


def test_the_projection_tile_pins_sit_in_both_functions_that_carry_them():
    src = source("project.hip")
    for fn in ("int project_fused_dp(", "int kmm_wide_dp("):
        body = src[src.index(fn):]
        body = body[:body.index(" template <", 1)] if " template <" in body[1:] else body
        for text in PINNED_TWICE:
            assert body.count(text) == 1, (fn, text)


LADDER_CALLS = {"kxx.hip": ["<4>"], "kxx_grad.hip": ["<4>"], "rff.hip": ["<4>"], "kmn_grad.hip": ["<4>", "<4>"],
                "grad.hip": [""], "project.hip": ["", "", ""]}


@pytest.mark.parametrize("name", sorted(LADDER_CALLS))
def test_each_entry_point_starts_its_ladder_where_the_plan_says(name):
    assert re.findall(r"mgp_with_dp(<\d+>)?\(", source(name)) == LADDER_CALLS[name]
    entry = {"kxx.hip": "kxx_matvec", "kxx_grad.hip": "kxx_grad", "rff.hip": "rff_sample",
             "kmn_grad.hip": "kmn_knm_vjp", "grad.hip": "k_dense_vjp", "project.hip": "knm_project"}[name]
    assert lp.MIN_DP[entry] == (4 if LADDER_CALLS[name][0] else 2)


def test_fused_limit():
    with open(os.path.join(ROOT, "include", "mgp.h")) as f:
        assert re.search(r"#define MGP_FUSED_MAX_D (\d+)", f.read()).group(1) == str(lp.FUSED_MAX_D)


# ---------------------------------------------------------------- 5. the entry points other tests hold on the ladder
def _listed_ds(where):
    path, name = where.split("::")
    if path.endswith("switch_forms.py") and not path.endswith("test_gpu_switch_forms.py"):
        import switch_forms
        return tuple(sorted({c[1] for c in getattr(switch_forms, name)}))
    if name == "FUSED_DS":
        import assign_reference
        return tuple(assign_reference.FUSED_DS)
    if name == "PRODUCT_D":
        import kmm_wide_reference
        return tuple(kmm_wide_reference.PRODUCT_D)
    with open(os.path.join(ROOT, path)) as f:  # the literal list inside the named test
        body = f.read().split(f"def {name}(")[1]
    return tuple(int(v) for v in re.search(r"for D, \(N, M\) in zip\(\[([0-9, ]+)\]", body).group(1).split(","))


@pytest.mark.parametrize("entry", sorted(lp.COMPLETE))
def test_coverage_table_points_at_tests_that_exist_and_cover_the_ladder(entry):
    test, where, ds = lp.COMPLETE[entry]
    path, name = test.split("::")
    with open(os.path.join(ROOT, path)) as f:
        assert re.search(rf"^def {re.escape(name)}\(", f.read(), re.M), test
    assert _listed_ds(where) == ds, (entry, _listed_ds(where))
    if "matrix-core" not in entry:  # those are laddered by KS = (D + 5) / 4, one case per KS
        assert {lp.with_dp(D) for D in ds} == set(lp.RUNGS), entry
    else:
        assert {(D + 5) // 4 for D in ds} == set(range(1, 10))
