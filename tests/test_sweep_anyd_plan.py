"""tests/sweep_anyd_plan.py against csrc/sweep_anyd.hip (no GPU): the constants and rules of the plan are the
expressions of the source, the generated cases cross every cut the plan names, and an fp64 emulation of the
augmented-K chain in the kernel's slice order stays inside the bound the GPU test applies, on the GPU test's point
sets."""

import os
import re

import numpy as np
import pytest

import pair_reference as pr
import sweep_anyd_plan as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")


def source(name="sweep_anyd.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


# ---------------------------------------------------------------- 1. the plan is the source's
def test_constants_are_the_sources():
    s = source()
    assert f"constexpr int kThreadsA = {ap.THREADS};" in s
    assert f"constexpr int kTRa = {ap.TR};" in s
    assert "constexpr int kOwn = 4 * kTRa * 16;" in s and ap.OWN == 4 * ap.TR * 16 == 128
    assert f"constexpr int kNJT = {ap.NJT};" in s
    assert "constexpr int kTile = kNJT * 16;" in s and ap.TILE == 64
    assert f"constexpr int kKSL = {ap.KSL};" in s
    assert "static_assert(kNJT * 64 == kThreadsA" in s
    assert "const int KS = (D + 2 + 3) >> 2;" in s
    assert "const int nks = KS - s0 < kKSL ? KS - s0 : kKSL;" in s
    assert "for (int s0 = 0; s0 < KS; s0 += kKSL)" in s
    with open(os.path.join(ROOT, "include", "mgp.h")) as f:
        text = f.read()
    assert re.search(r"#define MGP_FUSED_MAX_D (\d+)", text).group(1) == str(ap.FUSED_MAX_D)
    assert re.search(r"#define MGP_MAX_D (\d+)", text).group(1) == str(ap.MAX_D)


def test_chunk_rule_is_the_sources():
    s = source()
    for expr in ("p.nblk = (na + kOwn - 1) / kOwn;", "const long target = 8L * num_cus;",
                 "long nchunks = p.nblk >= 4L * num_cus ? 1 : (target + p.nblk - 1) / p.nblk;",
                 "const long max_chunks = (nb + kTile - 1) / kTile;", "if (nchunks > max_chunks) nchunks = max_chunks;",
                 "if (nchunks < 1) nchunks = 1;", "long b_chunk = (nb + nchunks - 1) / nchunks;",
                 "b_chunk = (b_chunk + kTile - 1) / kTile * kTile;", "p.nchunks = (nb + b_chunk - 1) / b_chunk;"):
        assert expr in s, expr
    # the same rule, written out independently, over a grid of shapes
    for cus in (1, 64, 256, 304):
        for na in (1, 127, 128, 129, 391, 4 * cus * 128 - 128, 4 * cus * 128 - 127, 1 << 18):
            for nb in (1, 63, 64, 65, 100, 150, 4096, (1 << 18) + 5):
                nblk = (na + 127) // 128
                n = 1 if nblk >= 4 * cus else (8 * cus + nblk - 1) // nblk
                n = max(1, min(n, (nb + 63) // 64))
                bc = ((nb + n - 1) // n + 63) // 64 * 64
                assert ap.chunk_plan(na, nb, cus) == (nblk, (nb + bc - 1) // bc, bc)
                sizes = ap.chunk_sizes(na, nb, cus)
                assert sum(sizes) == nb and all(0 < c <= bc for c in sizes) and all(c == bc for c in sizes[:-1])


def test_ladder_and_ws_formula_are_the_sources():
    s = source()
    assert "int anyd_widest_pass(int R) { return R >= 8 ? 8 : (R >= 4 ? 4 : (R >= 2 ? 2 : 1)); }" in s
    assert "const int rc = anyd_widest_pass(left);" in s
    for w in ap.WIDTHS:
        assert f"MGP_ANYD_PASS({w});" in s
    assert ("const size_t need = ((size_t)na + (size_t)nb + (pl.nchunks > 1 ? (size_t)pl.nchunks * na * "
            "anyd_widest_pass(R) : (size_t)0)) * sizeof(double);") in s
    assert "MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, need));" in s
    assert "h->gen" not in s and "gen_bytes" not in s  # the generic-D arena is never touched
    assert s.count("mgp_reserve(") == 1
    assert "atomic" not in s.split("#include")[2].lower()  # no atomics in the code (the header comment says so)
    assert [ap.passes(R) for R in (0, 1, 2, 3, 5, 8, 9, 17)] == [[], [1], [2], [2, 1], [4, 1], [8], [8, 1], [8, 8, 1]]
    assert ap.ws_bytes(129, 65, 3) == 8 * (129 + 65 + 2 * 129 * 2)
    assert ap.ws_bytes(4 * 256 * 128, 150, 1) == 8 * (4 * 256 * 128 + 150)
    # the header states the same formula
    with open(os.path.join(ROOT, "include", "mgp_sweep_anyd.h")) as f:
        assert "8 (na + nb + [chunks > 1] chunks na RC) bytes" in re.sub(r"\s*\n \*\s*", " ", f.read())


def test_k_slices():
    assert ap.slices(33) == [8, 1] and ap.slices(58) == [8, 7] and ap.slices(62) == [8, 8]
    assert ap.slices(63) == [8, 8, 1] and ap.slices(77) == [8, 8, 4] and ap.slices(512) == [8] * 16 + [1]
    for D in range(33, 513):
        assert 0 <= 4 * sum(ap.slices(D)) - (D + 2) < 4 and all(1 <= k <= ap.KSL for k in ap.slices(D))
    assert {(D + 2) % 4 for D in ap.DIMS[:4]} == {0, 1, 2, 3}
    assert [ap.k_steps(D) for D in ap.SLICE_EDGE_DIMS] == [2 * ap.KSL - 1, 2 * ap.KSL, 2 * ap.KSL + 1]


# ---------------------------------------------------------------- 2. the generated cases cross every cut
def test_cases_cover_the_plan():
    cases = ap.dense_cases()
    assert len({c.id for c in cases}) == len(cases)
    base = [c for c in cases if (c.na, c.nb, c.R) == (ap.OWN + 1, ap.TILE + 1, 3) and c.entry != "kxx"]
    assert {c.D for c in base} == set(ap.DIMS) and set(ap.DIMS) >= {33, 34, 35, 36, 77, 90, 511, 512}
    for entry in ("knm", "kmn"):
        mine = [c for c in cases if c.entry == entry and c.D == 77]
        assert {c.na for c in mine} >= set(ap.OWNED) == {1, 127, 128, 129, 391}
        assert {c.nb for c in mine} >= set(ap.STREAMED)
        assert {c.R for c in mine} >= set(ap.COLUMNS) == {8, 4, 2, 1, 9, 0}
        assert {(c.w_layout, c.out_layout) for c in cases if c.entry == entry} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert ap.chunk_sizes(ap.OWN + 1, 100) == [64, 36] and ap.chunk_sizes(ap.OWN + 1, 150) == [64, 64, 22]
    assert ap.chunk_sizes(1, ap.TILE + 1) == [64, 1] and ap.chunk_sizes(1, ap.TILE - 1) == [63]
    assert {c.kind for c in cases} == set(ap.KINDS)
    kxx = [c for c in cases if c.entry == "kxx"]
    assert kxx and all(c.s2 > 0 and c.na == c.nb for c in kxx) and {len(ap.chunk_sizes(c.na, c.nb)) for c in kxx} >= {2, 3}
    u = ap.unsplit_case()
    assert ap.chunk_plan(u.na, u.nb) == (4 * ap.NOMINAL_CUS, 1, 192) and u.nb > 2 * ap.TILE and u.nb % ap.TILE


# ---------------------------------------------------------------- 3. a correct fp64 chain meets the GPU test's bound
@pytest.mark.parametrize("D", ap.PAIR_DIMS)
@pytest.mark.parametrize("name", pr.KINDS)
def test_emulated_chain_meets_the_pair_bound(name, D):
    """The chain of csrc/sweep_anyd.hip in float64 (squared norms as fma chains, then K ascending through the slices)
    against the long-double values, on the point sets of test_gpu_sweep_anyd.py and with its bound and no extra."""
    ls = pr.lengthscales(D)
    worst = 0.0
    for label, P, Q, cols in ap.pair_sets(name, D):
        Qc = Q[cols]
        pv = pr.pair_values(name, pr.VARIANCE, ls, P, Qc)
        rel = pr.pair_bound(name, pr.VARIANCE, pv.s, pv.q, pr.scaled(name, ls, P), pr.scaled(name, ls, Qc), D, np.float64)
        got = ap.emulate_values(name, pr.VARIANCE, ls, P, Qc)
        worst = max(worst, pr.check_pairs(f"emulated {name} D={D} {label}", got.astype(np.float64), pv, rel,
                                          pr.VARIANCE, np.float64))
    print(f"sweep_anyd emulation {name} D={D}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- 4. the "auto" rule is the measurement's
def test_auto_constants_follow_the_profile():
    """`fused_anyd_auto` takes the fused form only where profiles/sweep_anyd_times.json has it at or below 0.9 of the
    panel route at every measured point, and up to the largest such dimension per measured column count."""
    import json

    import torch

    from cggp import conjugate_gradient as cgm
    with open(os.path.join(ROOT, "profiles", "sweep_anyd_times.json")) as f:
        rows = [r for r in json.load(f)["rows"] if r["step"] == "sweeps"]
    dims = sorted({r["D"] for r in rows})
    assert dims == [33, 48, 77, 90, 128, 512] and {r["R"] for r in rows} == {1, 5, 8} == set(cgm.FUSED_ANYD_AUTO_MAX_D)
    assert {r["product"] for r in rows} == {"knm", "kmn"} and {r["kernel"] for r in rows} == {"se", "matern32"}
    assert len(rows) == 6 * 3 * 2 * 2 and all(r["N"] == 1 << 18 and r["M"] == 4096 for r in rows)
    for R, max_d in cgm.FUSED_ANYD_AUTO_MAX_D.items():
        worst = {D: max(r["fused_over_panel"] for r in rows if r["R"] == R and r["D"] == D) for D in dims}
        ok = [D for D in dims if all(worst[d] <= 0.9 for d in dims if d <= D)]
        assert max_d == max(ok), (R, worst)
    f64 = torch.float64
    assert cgm.fused_anyd_auto(f64, 77, 1) and cgm.fused_anyd_auto(f64, 512) and not cgm.fused_anyd_auto(f64, 32, 1)
    assert cgm.fused_anyd_auto(f64, 48, 5) and not cgm.fused_anyd_auto(f64, 77, 5)
    assert cgm.fused_anyd_auto(f64, 128, 8) and not cgm.fused_anyd_auto(f64, 512, 8)
    assert not cgm.fused_anyd_auto(f64, 40, 3) and not cgm.fused_anyd_auto(torch.float32, 77, 1)
