"""tests/quadform_plan.py against csrc/quadform.hip and include/mgp_predict.h (no GPU): the constants and rules of the
plan are the expressions of the source, the pairing covers every block once with a balanced walk, and the scratch
formula is the one the source reserves and the header states."""

import os
import re

import quadform_plan as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")


def source(name="quadform.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def header():
    with open(os.path.join(ROOT, "include", "mgp_predict.h")) as f:
        return re.sub(r"[\s*]+", " ", f.read())


def test_constants_are_the_sources():
    s = source()
    assert f"constexpr int QK = {qp.STEP};" in s
    assert f"constexpr int QT = {qp.T};" in s
    assert f"constexpr int QC = {qp.C};" in s
    assert "constexpr long QF_CHUNK_B = 1L << 16;" in s and qp.CHUNK_B == 1 << 16
    assert "constexpr int MT = QT / 32, NQ = QC / 32;" in s  # 4 x 4 accumulator tiles of 16 x 16 per wave
    assert qp.T % 32 == 0 and qp.C % 32 == 0 and qp.C % qp.STEP == 0
    with open(os.path.join(ROOT, "include", "mgp.h")) as f:
        assert re.search(r"#define MGP_FUSED_MAX_D (\d+)", f.read()).group(1) == str(qp.FUSED_MAX_D)
    assert "if (k->dtype == MGP_F32 || k->D > MGP_FUSED_MAX_D)" in s  # the generic route's condition
    assert [qp.padded_dim(D) for D in qp.DIMS] == [2, 4, 8, 16, 32, 32]


def test_pairing_and_walk_are_the_sources():
    s = source()
    for expr in ("const long nJ = (M + QC - 1) / QC;",
                 "const int J = pass == 0 ? nJ - 1 - (int)blockIdx.y : (int)blockIdx.y;",
                 "if (pass == 1 && J == nJ - 1 - (int)blockIdx.y) break;",
                 "const long j0 = (long)J * QC;", "const long i_end = j0 + QC < M ? j0 + QC : M;",
                 "for (long i0 = 0; i0 < i_end; i0 += QK)",
                 "dim3((unsigned)tiles, (unsigned)((nJ + 1) / 2))", "const long tiles = (Bc + QT - 1) / QT;",
                 "for (long c0 = 0; c0 < B; c0 += QF_CHUNK_B)",
                 "const long Bc = B - c0 < QF_CHUNK_B ? B - c0 : QF_CHUNK_B;"):
        assert expr in s, expr
    for M in (1, 127, 128, 129, 256, 389, 640, 4096, 4097):
        pr = qp.pairs(M)
        assert sorted(J for p in pr for J in p) == list(range(qp.blocks(M)))  # every block once
        assert len(pr) == (qp.blocks(M) + 1) // 2
        assert all(len(p) == 2 for p in pr[:qp.blocks(M) // 2])
        if qp.blocks(M) % 2:
            assert pr[-1] == (qp.blocks(M) // 2,)
        # a pair walks nJ + 1 blocks, less what the ragged last block saves; the unpaired middle block about half
        full = [sum(qp.walk_steps(M, J) for J in p) for p in pr if len(p) == 2]
        assert not full or max(full) - min(full) <= qp.C // qp.STEP
        assert all(w <= (qp.blocks(M) + 1) * qp.C // qp.STEP for w in full)
    assert qp.grid(1, 1) == [(1, 1)] and qp.grid(2 * qp.T + 3, 3 * qp.C + 5) == [(3, 2)]
    assert qp.grid(qp.CHUNK_B + 1, 4096) == [(512, 16), (1, 16)]


def test_the_upper_triangle_alone_is_read():
    s = source()
    # the only loads of C on the fused route: the panel masked to i < col < M and the diagonal entry of a column < M
    assert "rg[u] = (col < M && i < col) ? C[i * ldc + col] : 0.0;" in s
    assert "const double cjj = col < M ? C[col * ldc + col] : 0.0;" in s
    fused = s.split("int quadform_fused_dp(")[0]
    assert fused.count("C[") == 2
    # the generic route reads it once, into the symmetric matrix
    assert "S[e] = i <= j ? C[i * ldc + j] : C[j * ldc + i];" in s
    assert s.count("C[") == 4
    # the exact doubling and the diagonal term
    assert "rp[m][g] = mgp_fma(mgp_fma(cjj, kd, a + a), kd, rp[m][g]);" in s
    assert "atomic" not in s.split("#include")[2].lower()


def test_auto_rule_is_the_one_the_measured_table_supports():
    """`fused_variance="auto"` takes the fused call from the smallest measured M on from which it took at most 0.9 of the
    composition's time at every measured point (both kernels); no such M: never."""
    import json
    from cggp import conjugate_gradient as cgm
    with open(os.path.join(ROOT, "profiles", "predict_quadform_times.json")) as f:
        rows = [r for r in json.load(f)["rows"] if r["step"] == "kernel"]
    assert {(r["kernel"], r["D"]) for r in rows} == {("se", 8), ("matern32", 32)}
    assert {r["M"] for r in rows} == {1024, 4096, 8192} and {r["B"] for r in rows} == {1 << 16}
    for r in rows:
        best = min(r["times"]["composed_8192"]["median_ms"], r["times"]["composed_one_batch"]["median_ms"])
        assert abs(r["fused_over_composed"] - r["times"]["fused"]["median_ms"] / best) < 1e-12
        assert r["rel_diff_to_composed"] < 1e-12
    ms = sorted({r["M"] for r in rows})
    ok_from = [m for m in ms if all(r["fused_over_composed"] <= 0.9 for r in rows if r["M"] >= m)]
    assert cgm.FUSED_VARIANCE_AUTO_MIN_M == (ok_from[0] if ok_from else None)


def test_scratch_formula_is_the_sources_and_the_headers():
    s = source()
    for expr in ("const long Bmax = B < QF_CHUNK_B ? B : QF_CHUNK_B;",
                 "const long Bpad_max = (Bmax + QT - 1) / QT * QT;",
                 "const size_t part_bytes = ((size_t)nJ * Bpad_max * sizeof(double) + 255) & ~(size_t)255;",
                 "MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, part_bytes + (size_t)M * (DP + 1) * sizeof(double)));",
                 "long rc_max = (long)((256ull << 20) / ((size_t)M * sizeof(T)));", "if (rc_max < 64) rc_max = 64;",
                 "if (rc_max > B) rc_max = B;",
                 "MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, (s_elems + 2 * panel_elems) * sizeof(T) + 256));"):
        assert expr in s, expr
    assert s.count("mgp_reserve(") == 2 and "h->gen" not in s and "h->ws" not in s  # one named arena per route
    assert qp.scratch_bytes(1, 1, 1) == 1024 + 8 * 3
    assert qp.scratch_bytes(2 * 128 + 3, 3 * 128 + 5, 8) == 8 * 4 * 384 + 8 * 389 * 9
    assert qp.scratch_bytes(1 << 20, 4096, 8) == 8 * 32 * (1 << 16) + 8 * 4096 * 9  # 16 MiB of partials at C3
    assert qp.generic_scratch_bytes(259, 389, 4) == 4 * (389 * 389 + 2 * 259 * 389) + 256
    assert qp.generic_scratch_bytes(1 << 20, 4096, 8) == 8 * (4096 * 4096 + 2 * 8192 * 4096) + 256
    h = header()
    assert "each counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that is too small" in h
    assert '("prj") alone: 8 nJ min(B\', 2^16) rounded up to 256, plus 8 M (D\' + 1) bytes' in h
    assert 'in "prj" elem (M^2 + 2 p M) + 256 bytes with p = min(B, max(64, 2^28 / (elem M))) panel rows' in h
    # the generic route's second arena: the NT GEMM's contraction slices (dense.hip), and never the generic-D arena
    assert 'in the reduction arena "ws" the contraction slices of the NT GEMM, s elem p M bytes' in h
    assert "s = min(8, ceil(2 CUs / (ceil(M / 128) ceil(p / 128))))" in h and '("gen") is never touched' in h
    d = source("dense.hip")
    for expr in ("const long big = ((n + 127) / 128) * ((m + 127) / 128);", "if (big >= 2L * h->num_cus) {",
                 "long nz = (2L * h->num_cus + big - 1) / big;", "if (nz > 8) nz = 8;",
                 "while (nz > 1 && (K % (16 * nz) != 0 || K / nz < 256)) --nz;",
                 "MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, (size_t)nz * tot * sizeof(T)));",
                 "while (nzu > 1 && K / nzu < 256) --nzu;",
                 "MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, (size_t)nzu * tot * sizeof(T)));"):
        assert expr in d, expr
    assert "mgp_reserve" not in source("generic.hip").split("int k_dense_generic_t(")[1].split("int sweep_generic_t(")[0]
    assert qp.gemm_slices_bound(259, 389, 8, 256) == 0 and qp.gemm_slices_bound(129, 129, 4, 256) == 0  # M < 512
    assert qp.gemm_slices_bound(300, 1024, 8, 256) == 4 * 8 * 300 * 1024  # 24 tiles: 8 wanted, 1024 / 4 = 256 terms each
    assert qp.gemm_slices_bound(8192, 4096, 8, 256) == 0  # 2048 tiles fill the chip
    assert "does not synchronise the stream" in h
    assert "models.py:343-345" in h and "SGPR.predict_f" in h
