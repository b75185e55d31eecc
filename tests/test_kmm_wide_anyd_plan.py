"""tests/kmm_wide_anyd_plan.py and tests/kmm_wide_anyd_reference.py against csrc/kmm_wide_anyd.hip (no GPU): the
constants and rules of the plan are the expressions of the source, the shapes of the GPU test cross every cut the
plan names, the long-double reference agrees with a plain float64 product, an fp64 emulation of the kernel's chain
stays inside the bound the GPU test applies, and the `"auto"` constants are what the recorded measurement gives."""

import json
import os
import re

import numpy as np
import pytest

import kmm_wide_anyd_plan as wp
import kmm_wide_anyd_reference as wr
import pair_reference as pr
import sweep_anyd_plan as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")
LD = np.longdouble


def source(name="kmm_wide_anyd.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


# ---------------------------------------------------------------- 1. the plan is the source's
def test_constants_are_the_sources():
    s = source()
    for name, value in (("kWThreads", wp.THREADS), ("kWOwn", wp.OWN), ("kWStep", wp.STEP), ("kWKSL", wp.KSL),
                        ("kWMaxR", wp.MAX_R), ("kFI", wp.FINISH_I), ("kFB", wp.FINISH_B)):
        assert f"constexpr int {name} = {value};" in s, name
    assert wp.KSL == ap.KSL  # the K slices of csrc/sweep_anyd.hip: the same chain, so the same pair bound
    assert "const int KS = (D + 2 + 3) >> 2;" in s and "inline int wide_anyd_ks(int D) { return (D + 2 + 3) >> 2; }" in s
    assert "const int nks = KS - s0 < kWKSL ? KS - s0 : kWKSL;" in s
    assert "for (int s0 = 0; s0 < KS; s0 += kWKSL)" in s
    assert "constexpr int NIT = NRT <= 8 ? kWStep / 16 : 1;" in s
    for nrt in (2, 4, 8, 16):
        assert f"MGP_WA({nrt});" in s and wp.row_tiles(16 * nrt) == nrt and wp.row_tiles(16 * nrt - 15 if nrt > 2 else 1) == nrt
    assert "if (r <= 32) MGP_WA(2); else if (r <= 64) MGP_WA(4); else if (r <= 128) MGP_WA(8); else MGP_WA(16);" in s
    assert f"enum {{ MGP_OP_KMM_LAMBDA_WIDE_ANYD = {wp.KIND} }};" in re.sub(
        r"\s+", " ", open(os.path.join(ROOT, "include", "mgp_sweep_anyd.h")).read())
    cg = source("cg.hip")
    assert "case MGP_OP_KMM_LAMBDA_WIDE_ANYD:" in cg and "mgp_kmm_wide_anyd_prepare(h, op->kernel, op->Z, op->M, Bt, nullptr)" in cg
    assert "csrc/kmm_wide_anyd.hip" not in cg and "kmm_wide_anyd.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_split_and_group_rules_are_the_sources():
    s = source()
    for expr in ("p.nblk = (M + kWOwn - 1) / kWOwn;", "long ns = (2L * num_cus + p.nblk - 1) / p.nblk;",
                 "const long max_split = (M + 255) / 256;", "if (ns > max_split) ns = max_split;", "if (ns < 1) ns = 1;",
                 "long rows = (M + ns - 1) / ns;", "rows = (rows + kWStep - 1) / kWStep * kWStep;",
                 "p.nsplit = (M + rows - 1) / rows;", "for (long g0 = 0; g0 < Bt; g0 += kWMaxR)",
                 "const int r = (int)(Bt - g0 < kWMaxR ? Bt - g0 : kWMaxR), RP = (r + 15) / 16 * 16;"):
        assert expr in s, expr
    for cus in (1, 64, 256, 304):
        for M in (1, 15, 64, 65, 255, 256, 257, 290, 391, 512, 513, 4096, 1 << 14, (1 << 16) + 5):
            nblk = (M + 63) // 64
            ns = max(1, min((2 * cus + nblk - 1) // nblk, (M + 255) // 256))
            rows = ((M + ns - 1) // ns + 31) // 32 * 32
            assert wp.split_plan(M, cus) == (nblk, (M + rows - 1) // rows, rows)
            _, nsplit, rows = wp.split_plan(M, cus)
            assert rows % wp.STEP == 0 and (nsplit - 1) * rows < M <= nsplit * rows
            assert wp.terms(M, cus) == rows
    assert wp.split_plan(391) == (7, 2, 224) and wp.split_plan(290) == (5, 2, 160) and wp.split_plan(256) == (4, 1, 256)
    assert wp.split_plan(4096) == (64, 8, 512) and wp.split_plan(1 << 14) == (256, 2, 8192) and wp.split_plan(1 << 16)[1] == 1
    assert wp.groups(1) == [1] and wp.groups(256) == [256] and wp.groups(257) == [256, 1] and wp.groups(600) == [256, 256, 88]


def test_arena_formula_is_the_sources_and_the_headers():
    s = source()
    assert ("return ((size_t)((M + 15) / 16) * wide_anyd_ks(D) * 64 * sizeof(double) + 255) & ~(size_t)255;") in s
    assert "const long g = Bt < kWMaxR ? Bt : (long)kWMaxR;" in s and "const long RP = (g + 15) / 16 * 16;" in s
    assert "return ((size_t)pl.nsplit * pl.nblk * kWOwn * RP * sizeof(double) + 255) & ~(size_t)255;" in s
    assert ("MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, wide_anyd_pack_bytes(M, k->D) + "
            "wide_anyd_part_bytes(h, M, Bt)));") in s
    assert s.count("mgp_reserve(") == 1 and "h->ws" not in s and "h->gen" not in s  # the prj arena alone
    assert "atomic" not in s.split("#include")[2].lower() and "hipMalloc" not in s
    assert wp.arena_bytes(391, 62, 70) == 8 * 64 * 16 * 25 + 8 * 2 * 7 * 64 * 80 == 778240
    assert wp.arena_bytes(1, 33, 1) == 8 * 64 * 9 + 8 * 64 * 16
    assert wp.arena_bytes(300, 77, 600) == wp.arena_bytes(300, 77, 255) > wp.arena_bytes(300, 77, 240) > 0
    with open(os.path.join(ROOT, "include", "mgp_sweep_anyd.h")) as f:
        text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", f.read()))
    assert "bytes = align256(8 * 64 * KS * ceil(M / 16)) + align256(8 * nsplit * 64 * ceil(M / 64) * RP)" in text
    assert "rows = ceil(ceil(M / s) / 32) * 32, s = clamp(ceil(2 CUs / ceil(M / 64)), 1, ceil(M / 256))" in text


def test_gpu_shapes_cross_every_cut():
    assert [ap.k_steps(D) for D in wp.PAIR_DIMS] == [9, 9, 16, 17, 20, 129]  # a slice and a bit, two whole slices, one more
    assert {(D + 2) % 4 for D in wp.PAIR_DIMS} == {0, 1, 2, 3}
    assert [wp.slices(D)[-1] for D in (33, 62, 63)] == [1, 8, 1]
    assert set(wp.PAIR_SIZES) == {1, 15, 16, 17, 127, 128, 129, 391}
    assert {wp.split_plan(M)[1] for M in wp.PAIR_SIZES} == {1, 2} and wp.split_plan(wp.DENSE_M)[1] == 2
    assert wp.split_plan(391)[2] % 32 == 0 and 391 - wp.split_plan(391)[2] < wp.split_plan(391)[2]
    assert {wp.row_tiles(g) for Bt in wp.WIDTHS for g in wp.groups(Bt)} == {2, 4, 8, 16}
    assert {len(wp.groups(Bt)) for Bt in wp.WIDTHS} == {1, 2} and set(wp.WIDTHS) >= {1, 15, 16, 17, 128, 129, 255, 256, 257, 300}
    for M in wp.PAIR_SIZES:
        c = wp.probed(M)
        assert c == sorted(set(c)) and c[0] == 0 and M - 1 in c and all(0 <= j < M for j in c) and len(c) <= 8


# ---------------------------------------------------------------- 2. the reference, and the bound on the emulated chain
@pytest.mark.parametrize("name", pr.KINDS)
def test_reference_matches_a_float64_product(name):
    """Against oracle/kernels.py in float64: 1e-12 of the largest entry (Matern-1/2 1e-7: the cusp of the oracle's
    expansion-form distance at coincident points, as tests/test_kmm_wide_host.py)."""
    from oracle import kernels as ok
    M, D, Bt = 70, 40, 5
    Z, ls, lam = wr.inputs(D, M)
    pv, rel = wr.kernel_columns(name, ls, Z)
    assert pv.k.dtype == LD and rel.shape == (M, M) and np.all(rel > 0)
    P = np.random.default_rng(1).standard_normal((Bt, M))
    ref = wr.product(pv.k, lam, P)
    plain = P @ (ok.Kernel(name, wr.VARIANCE, ls).K(Z) + np.diag(lam))
    assert float(np.max(np.abs(ref - plain)) / np.max(np.abs(plain))) < (1e-7 if name == "matern12" else 1e-12)
    cols = [0, 33, 69]
    sub, rel_sub = wr.kernel_columns(name, ls, Z, cols)
    assert np.array_equal(sub.k, pv.k[:, cols]) and np.allclose(rel_sub, rel[:, cols], rtol=1e-12, atol=0)


@pytest.mark.parametrize("D,M", [(33, 129), (77, 290)])
@pytest.mark.parametrize("name", pr.KINDS)
def test_emulated_chain_meets_the_bound(name, D, M):
    """The kernel's chain in float64 -- the augmented-K distance of `sweep_anyd_plan.emulate_neg_s`, the profile, then
    per split one running sum over the streamed rows in order, the splits added in order, the variance, the lambda
    fma -- against the long-double product, inside `product_bound`, on the GPU test's inputs."""
    Z, ls, lam = wr.inputs(D, M, seed=1)
    pv, rel = wr.kernel_columns(name, ls, Z)
    kv = (ap.emulate_values(name, wr.VARIANCE, ls, Z, Z) / LD(wr.VARIANCE)).astype(np.float64)  # profile(-s), fp64
    P = np.random.default_rng([3, 17, M]).standard_normal((17, M))
    _, nsplit, rows = wp.split_plan(M)
    total = np.zeros((17, M))
    for z in range(nsplit):
        acc = np.zeros((17, M))
        for i in range(z * rows, min(M, (z + 1) * rows)):
            acc = ap._fma(P[:, i][:, None], kv[i][None, :], acc)
        total = total + acc
    got = ap._fma(lam[None, :], P, total * wr.VARIANCE)
    bound = wr.product_bound(pv.k, rel * pv.k, lam, P, M, wp.NOMINAL_CUS)
    worst = float((np.abs(got.astype(LD) - wr.product(pv.k, lam, P)) / bound).max())
    print(f"kmm-wide-anyd emulation {name} D={D} M={M}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_cg_trace_is_the_oracles_recurrence():
    from oracle import cg as ocg
    rng = np.random.default_rng(2)
    B = rng.standard_normal((30, 30))
    A = B @ B.T + 30 * np.eye(30)
    rhs = rng.standard_normal((3, 30)) * np.array([[1.0], [1e-8], [1e-9]])
    den, rz = wr.cg_trace(A, rhs, 4)
    for k in range(4):
        _, (steps, err) = ocg.conjugate_gradient(A, rhs, np.zeros_like(rhs), 0.0, max_iterations=k, max_steps_cycle=9)
        assert steps == k and np.allclose(0.5 * rz[k], err[:, 0], rtol=1e-12, atol=0)
    assert den.shape == rz.shape == (4, 3) and np.all(rz[0, 2:] <= 1e-16) and rz[0, 0] > 1


# ---------------------------------------------------------------- 3. the "auto" rule is the measurement's
def test_auto_constants_follow_the_profile():
    """`wide_anyd_auto` takes the kind exactly in the region tools/run_kmm_wide_anyd.py derives from
    profiles/kmm_wide_anyd_times.json: at most 0.9 of the faster existing route at every measured point of it."""
    import torch

    from cggp import conjugate_gradient as cgm
    with open(os.path.join(ROOT, "profiles", "kmm_wide_anyd_times.json")) as f:
        prof = json.load(f)
    rows = prof["rows"]
    assert {r["M"] for r in rows} == {1 << 12, 1 << 14, 1 << 16} and {r["D"] for r in rows} == {33, 77, 90, 128, 512}
    assert {r["columns"] for r in rows} == {16, 48, 64, 256} and {r["kernel"] for r in rows} == {"se", "matern32"}
    assert len(rows) == 3 * 5 * 4 * 2 and prof["counters"] == "no counter run was made"
    for r in rows:
        fastest = min(r["times"]["plain"]["best_ms"], r["times"]["anyd"]["best_ms"])
        assert r["wide_anyd_over_fastest"] == pytest.approx(r["times"]["wide_anyd"]["best_ms"] / fastest)
    f64 = torch.float64
    C, Mmin, Dmax = cgm.WIDE_ANYD_AUTO_MIN_COLUMNS, cgm.WIDE_ANYD_AUTO_MIN_M, cgm.WIDE_ANYD_AUTO_MAX_D
    chosen = prof["rule"]["chosen"]
    if chosen is None:
        assert C is None
        assert not any(cgm.wide_anyd_auto(f64, r["D"], r["columns"], r["M"]) for r in rows)
    else:
        assert (C, Mmin, Dmax) == (chosen["columns"], chosen["M"], chosen["max_d"]) and cgm.WIDE_ANYD_AUTO_MIN_D == 33
        inside = [r for r in rows if r["D"] <= Dmax and r["columns"] >= C and r["M"] >= Mmin]
        assert len(inside) == chosen["points"] and all(r["wide_anyd_over_fastest"] <= 0.9 for r in inside)
        for r in rows:
            assert cgm.wide_anyd_auto(f64, r["D"], r["columns"], r["M"]) == (r in inside)
        assert not cgm.wide_anyd_auto(f64, 32, 10 * C, 10 * Mmin) and not cgm.wide_anyd_auto(torch.float32, 77, 10 * C, 10 * Mmin)
        assert not cgm.wide_anyd_auto(f64, 33, C - 1, Mmin) and not cgm.wide_anyd_auto(f64, 33, C, Mmin - 1)
