"""tests/kxx_sym_anyd_plan.py against csrc/kxx_sym_anyd.hip (no GPU): the constants and rules of the plan are the
expressions of the source, every unordered block pair is dealt exactly once, every (slot, row) has one writer, the
scratch formula is the source's and the header's, the shapes of the GPU test cross every cut the plan names, an fp64
emulation of the kernel's chain stays inside the bound the GPU test applies, and the `"auto"` constants are what the
recorded measurement gives."""

import json
import os
import re

import numpy as np
import pytest

import kxx_sym_anyd_plan as sp
import pair_reference as pr
import sweep_anyd_plan as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")
LD = np.longdouble
U = 2.0 ** -53


def source(name="kxx_sym_anyd.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def header():
    with open(os.path.join(ROOT, "include", "mgp.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", f.read()))


# ---------------------------------------------------------------- 1. the plan is the source's
def test_constants_are_the_sources():
    s = source()
    for name, value in (("kSThreads", sp.THREADS), ("kSNJ", sp.NJ), ("kSNIT", sp.NIT), ("kSKSL", sp.KSL),
                        ("kSCols", sp.COLS)):
        assert f"constexpr int {name} = {value};" in s, name
    assert "constexpr int kSTB = 64 * kSNJ;" in s and sp.TB == 64 * sp.NJ == 128
    assert "constexpr size_t kSSlotBudget = (size_t)1 << 29;" in s and sp.SLOT_BUDGET == 1 << 29
    assert "constexpr size_t kKxxSlotBudget = (size_t)1 << 29;" in source("kxx.hip")  # bounded as kxx.hip bounds its slots
    assert sp.KSL == ap.KSL  # the K slices of csrc/sweep_anyd.hip: the same chain, so the same pair bound
    assert "const int KS = (D + 2 + 3) >> 2;" in s and "inline int sym_ks(int D) { return (D + 2 + 3) >> 2; }" in s
    assert "for (int s0 = 0; s0 < KS; s0 += kSKSL)" in s and "const int nks = KS - s0 < kSKSL ? KS - s0 : kSKSL;" in s
    assert "for (long g0 = 0; g0 < Bt; g0 += kSCols)" in s
    assert f"MGP_OP_KXX_NOISE_SYM_ANYD = {sp.KIND} }};" in header()
    cg = source("cg.hip")
    assert "case MGP_OP_KXX_NOISE_SYM_ANYD:" in cg
    assert "mgp_kxx_sym_anyd_prepare(h, op->kernel, op->X, op->N, Bt, nullptr)" in cg and "sym_hold.hold(op->X, op->N);" in cg
    assert "kxx_sym_anyd.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert "if (gate != nullptr && *gate == 0) return;" in s and s.count("if (gate != nullptr && *gate == 0) return;") == 4
    assert s.count("__global__") == 4  # every kernel of the file reads the gate word


def test_deal_and_plan_rules_are_the_sources():
    s = source()
    for expr in ("const long J = (I + dist) % nbk;", "const bool diag = dist == 0;",
                 "const bool idle = !diag && 2 * dist == nbk && I >= nbk / 2;",
                 "p.nbk = (N + kSTB - 1) / kSTB;", "p.npad = p.nbk * kSTB;", "p.nd_total = p.nbk / 2 + 1;",
                 "long want = (2L * num_cus + p.nbk - 1) / p.nbk;",
                 "want = want < 1 ? 1 : (want > p.nd_total ? p.nd_total : want);",
                 "long dc = (p.nd_total + want - 1) / want;",
                 "long maxs = (long)(kSSlotBudget / ((size_t)p.npad * r * sizeof(double)));",
                 "maxs = maxs < 2 ? 2 : (maxs > 32768 ? 32768 : maxs);", "if (dc > maxs - 1) dc = maxs - 1;",
                 "long cpl = maxs / (dc + 1);", "cpl = cpl < 1 ? 1 : cpl;", "const long s = cpl * dc;",
                 "p.S = (int)(s < p.nd_total ? s : p.nd_total);",
                 "const int dd0 = ch * dc, dd1 = dd0 + dc < nd ? dd0 + dc : nd;",
                 "double* st = slots + (long)dd * slot_stride + J * kSTB * r;",
                 "double* sd = slots + (long)(S + ch) * slot_stride + otile * 16 * r;",
                 "const int nch = (nd + pl.dc - 1) / pl.dc;", "const long slot_stride = npad * r;"):
        assert expr in s, expr
    for cus in (1, 64, 256, 304):
        for N in (1, 127, 128, 129, 610, 3970, 1 << 14, (1 << 15) + 3, 1 << 17):
            for r in (1, 5, 16):
                nb, npad, nd, dc, S = sp.plan(N, r, cus)
                assert nb == -(-N // 128) and npad == 128 * nb and nd == nb // 2 + 1 and 1 <= dc <= S <= nd
                used = S + -(-S // dc)
                assert used * npad * r * 8 <= max(sp.SLOT_BUDGET, 2 * npad * r * 8)  # the bound of kxx.hip
                ls = sp.launches(N, r, cus)
                assert sum(n for _, n, _ in ls) == nd and all(n <= S and c <= -(-S // dc) for _, n, c in ls)
                assert [d0 for d0, _, _ in ls] == list(range(0, nd, S))
    assert sp.plan(610, 16) == (5, 640, 3, 1, 3) and sp.plan(3970, 16) == (32, 4096, 17, 2, 17)
    assert sp.plan(1 << 15, 16) == (256, 1 << 15, 129, 65, 65) and sp.plan(1 << 17, 16)[3:] == (31, 31)
    assert sp.groups(1) == [1] and sp.groups(16) == [16] and sp.groups(17) == [16, 1] and sp.groups(40) == [16, 16, 8]


@pytest.mark.parametrize("nb", range(1, 10))
def test_every_unordered_block_pair_once(nb):
    pairs = sp.block_pairs(nb)
    assert len(pairs) == nb * (nb + 1) // 2
    assert {frozenset(p) for p in pairs} == {frozenset((i, j)) for i in range(nb) for j in range(i, nb)}
    assert sum(1 for I, J in pairs if I == J) == nb  # the diagonal tiles, once each
    for d in range(nb // 2 + 1):  # every d: the streamed blocks are a permutation of the blocks
        assert sorted(sp.tile_of(nb, I, d)[0] for I in range(nb)) == list(range(nb))
    for bi in range(nb):
        for bj in range(nb):
            p = sp.path(nb, bi, bj)
            assert (p == "diag") == (bi == bj)
            if bi != bj:  # one side of a pair is kept, the other streamed
                assert {p, sp.path(nb, bj, bi)} == {"kept", "streamed"}
                assert ((bi, bj) in pairs) == (p == "kept")


@pytest.mark.parametrize("N,r,cus", [(n, r, c) for n in (100, 200, 300, 610, 1100, 3970) for r, c in ((16, 256), (1, 8))])
def test_each_slot_and_row_has_one_writer(N, r, cus):
    nb, _, _, dc, S = sp.plan(N, r, cus)
    for (d0, nd, nch), writers in zip(sp.launches(N, r, cus), sp.slot_writers(N, r, cus)):
        want = {(dd, b) for dd in range(nd) for b in range(nb)} | {(S + ch, b) for ch in range(nch) for b in range(nb)}
        assert set(writers) == want and set(writers.values()) == {1}
        assert max(s for s, _ in writers) < S + -(-S // dc)  # inside the slots the arena holds


def test_arena_formula_is_the_sources_and_the_headers():
    s = source()
    assert "return (b + 255) & ~(size_t)255;" in s
    assert "return sym_align((size_t)(npad / 16) * sym_ks(D) * 64 * sizeof(double));" in s
    assert "return sym_align((size_t)npad * kSCols * sizeof(double));" in s
    assert "return sym_align((size_t)(pl.S + (pl.S + pl.dc - 1) / pl.dc) * pl.npad * r * sizeof(double));" in s
    assert "return sym_pack_bytes(pl.npad, D) + 2 * sym_wt_bytes(pl.npad) + sb;" in s
    assert "MGP_TRY(mgp_reserve(h, &h->kxx, &h->kxx_bytes, sym_arena_bytes(h, N, k->D, Bt)));" in s
    assert s.count("mgp_reserve(") == 1 and "h->ws" not in s and "h->gen" not in s and "h->prj" not in s  # the kxx arena alone
    assert "atomic" not in s.split("#include")[1].lower() and "hipMalloc" not in s
    formula = ("bytes = align256(8 * 64 * KS * N' / 16) + 2 * align256(8 * 16 * N') + "
               "align256(8 * (S + ceil(S / DC)) * N' * r)")
    assert formula in header() and formula in s
    for phrase in ("MGP_E_NOMEM from a fixed pool", "counted by mgp_workspace_bytes", "u (terms + slots + 3)",
                   "terms = 128 DC", "slots = nd + ceil(nd / DC) + 2 ceil(nd / S)", "two calls are bit-identical",
                   "exactly the code of MGP_OP_KXX_NOISE and give its bits", "N = 0 or Bt = 0 writes nothing",
                   "Every launch reads the gate word", "this error is why the kind is opt-in"):
        assert phrase in header(), phrase
    # the formula as written, evaluated independently
    for N, D, Bt, cus in ((391, 62, 21, 256), (100, 33, 1, 256), (610, 512, 16, 304), (1 << 15, 77, 33, 256)):
        npad = -(-N // 128) * 128
        KS = -(-(D + 2) // 4)
        a = lambda b: (b + 255) // 256 * 256

        def slot_term(r):
            _, _, _, dc, S = sp.plan(N, r, cus)
            return a(8 * (S + -(-S // dc)) * npad * r)

        widths = [min(Bt, 16)] + ([Bt % 16] if Bt > 16 and Bt % 16 else [])
        assert sp.arena_bytes(N, D, Bt, cus) == a(8 * 64 * KS * npad // 16) + 2 * a(8 * 16 * npad) + max(map(slot_term, widths))
    assert sp.arena_bytes(391, 62, 21) == 8 * 64 * 16 * 32 + 2 * 8 * 16 * 512 + 8 * 6 * 512 * 16 == 786432
    assert sp.chain(391, 21) == 128 + (3 + 3 + 2) + 3 and sp.terms(3970, 16) == 256 and sp.slots(1 << 15, 16) == 129 + 2 + 4


def test_gpu_shapes_cross_every_cut():
    assert [sp.ceil_div(N, sp.TB) for N in sp.PAIR_SIZES] == [1, 2, 3, 5] and 610 % 16 == 2
    assert sp.tile_of(2, 0, 1) == (1, "pair") and sp.tile_of(2, 1, 1) == (0, "idle")  # the even rule at d = nb/2
    assert all(sp.tile_of(3, I, 1)[1] == "pair" for I in range(3))
    assert [ap.k_steps(D) for D in sp.PAIR_DIMS] == [9, 20, 129]
    assert set(sp.WIDTHS) == {1, 2, 5, 8, 16, 17, 33} and {len(sp.groups(b)) for b in sp.WIDTHS} == {1, 2, 3}
    assert sp.ceil_div(sp.DENSE_N, sp.TB) == 3 and sp.DENSE_N % 16 and sp.DENSE_D > 32
    assert sp.chained_size() == 3970 and sp.plan(3970, 16)[3] == 2
    for N in sp.PAIR_SIZES + (3970, 1 << 15):
        c = sp.probed(N)
        assert c == sorted(set(c)) and c[0] == 0 and N - 1 in c and all(0 <= j < N for j in c) and len(c) <= 12
        nb = sp.ceil_div(N, sp.TB)
        paths = {sp.path(nb, bi, j // sp.TB) for bi in range(nb) for j in c}
        assert paths == ({"diag"} if nb == 1 else {"diag", "kept", "streamed"})


# ---------------------------------------------------------------- 2. the bound on the emulated chain
@pytest.mark.parametrize("name", pr.KINDS)
def test_emulated_chain_meets_the_bound(name):
    """The kernel's chain in float64 -- the augmented-K distance of `sweep_anyd_plan.emulate_neg_s` with the streamed
    point in the A role, the profile, then per block pair the kept-side sums (one accumulator over the streamed rows
    and the d of a chunk) and the streamed-side sums (per wave over its 32 kept points, the waves added in order), the
    slots in slot order, the variance, the s2 fma -- against the long-double product, inside the header's bound."""
    N, D, Bt, s2 = 300, 40, 5, 0.5
    X = np.random.default_rng([1, D, N]).standard_normal((N, D))
    ls = pr.lengthscales(D) * np.sqrt(D)
    pv = pr.pair_values(name, pr.VARIANCE, ls, X, X)
    a = pr.scaled(name, ls, X)
    pairb = pr.pair_bound(name, pr.VARIANCE, pv.s, pv.q, a, a, D, np.float64) * pv.k
    kv = (ap.emulate_values(name, pr.VARIANCE, ls, X, X) / LD(pr.VARIANCE)).astype(np.float64)  # [streamed i, kept j]
    P = np.random.default_rng([3, Bt, N]).standard_normal((Bt, N))
    nb, npad, nd, dc, S = sp.plan(N, Bt)
    Pp = np.zeros((Bt, npad))
    Pp[:, :N] = P
    Kp = np.ones((npad, npad))
    Kp[:N, :N] = kv
    blk = lambda b: slice(b * sp.TB, (b + 1) * sp.TB)
    total = np.zeros((Bt, npad))
    for d0, nd_l, nch in sp.launches(N, Bt):
        streamed = [np.zeros((Bt, npad)) for _ in range(nd_l)]
        kept = [np.zeros((Bt, npad)) for _ in range(nch)]
        for ch in range(nch):
            for I in range(nb):
                acc = np.zeros((Bt, sp.TB))
                for dd in range(ch * dc, min((ch + 1) * dc, nd_l)):
                    J, what = sp.tile_of(nb, I, d0 + dd)
                    if what == "idle":
                        continue
                    tile = Kp[blk(J), blk(I)]  # [i streamed, j kept]
                    for i in range(sp.TB):
                        acc = ap._fma(Pp[:, blk(J)][:, i][:, None], tile[i][None, :], acc)
                    if what == "pair":
                        waves = []
                        for w in range(4):
                            part = np.zeros((Bt, sp.TB))
                            for j in range(32 * w, 32 * w + 32):
                                part = ap._fma(Pp[:, blk(I)][:, j][:, None], tile[:, j][None, :], part)
                            waves.append(part)
                        streamed[dd][:, blk(J)] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
                kept[ch][:, blk(I)] = acc
        for part in streamed + kept:
            total = total + part
    got = ap._fma(np.full_like(P, s2), P, pr.VARIANCE * total[:, :N])
    Pl = P.astype(LD)
    want = Pl @ pv.k + LD(s2) * Pl
    Pa = np.abs(Pl)
    bound = Pa @ pairb.astype(LD) + U * sp.chain(N, Bt) * (Pa @ np.abs(pv.k)) + 2 * U * s2 * Pa
    worst = float((np.abs(got.astype(LD) - want) / bound).max())
    print(f"kxx-sym-anyd emulation {name}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- 3. the "auto" rule is the measurement's
def test_auto_constants_follow_the_profile():
    """`sym_anyd_auto` takes the kind exactly in the region tools/run_kxx_sym_anyd.py derives from
    profiles/kxx_sym_anyd_times.json: at most 0.9 of the faster existing route at every measured point of it."""
    import torch

    from cggp import conjugate_gradient as cgm
    with open(os.path.join(ROOT, "profiles", "kxx_sym_anyd_times.json")) as f:
        prof = json.load(f)
    rows = prof["rows"]
    assert {r["kernel"] for r in rows} == {"se", "matern32"} and prof["counters"] == "no counter run was made"
    assert {r["columns"] for r in rows} == {1, 5, 8, 16, 32} and {r["D"] for r in rows} <= {33, 77, 90, 128, 512}
    for r in rows:
        fastest = min(r["times"]["plain"]["best_ms"], r["times"]["anyd"]["best_ms"])
        assert r["sym_anyd_over_fastest"] == pytest.approx(r["times"]["sym_anyd"]["best_ms"] / fastest)
    f64 = torch.float64
    lo, hi = cgm.SYM_ANYD_AUTO_MIN_COLUMNS, cgm.SYM_ANYD_AUTO_MAX_COLUMNS
    Nmin, Dmax = cgm.SYM_ANYD_AUTO_MIN_N, cgm.SYM_ANYD_AUTO_MAX_D
    chosen = prof["rule"]["chosen"]
    if chosen is None:
        assert lo is None
        assert not any(cgm.sym_anyd_auto(f64, r["D"], r["columns"], r["N"]) for r in rows)
    else:
        assert (lo, hi, Nmin, Dmax) == (chosen["min_columns"], chosen["max_columns"], chosen["N"], chosen["max_d"])
        assert cgm.SYM_ANYD_AUTO_MIN_D == 33
        inside = [r for r in rows if r["D"] <= Dmax and lo <= r["columns"] <= hi and r["N"] >= Nmin]
        assert len(inside) == chosen["points"] and all(r["sym_anyd_over_fastest"] <= 0.9 for r in inside)
        for r in rows:
            assert cgm.sym_anyd_auto(f64, r["D"], r["columns"], r["N"]) == (r in inside)
        assert not cgm.sym_anyd_auto(f64, 32, lo, 10 * Nmin) and not cgm.sym_anyd_auto(torch.float32, 77, lo, 10 * Nmin)
        assert not cgm.sym_anyd_auto(f64, 33, hi + 1, Nmin) and not cgm.sym_anyd_auto(f64, 33, lo, Nmin - 1)
