"""The CG route plan on the CPU: the planned cases reach every launch form the solve driver can choose
(tests/cg_route_plan.py; the values are checked by tests/test_gpu_cg_routes.py)."""

import numpy as np

import cg_route_plan as rp


def test_rules_at_the_figures_worked_by_hand():
    # 256 CUs, nine right-hand sides, fp64
    assert [rp.skinny_slices(n, 9) for n in (256, 257, 512, 513, 1024, 2048, 2049, 4096, 4097, 8192)] == \
        [4, 5, 8, 9, 16, 16, 11, 8, 7, 4]
    assert rp.skinny_slices(64, 9) == 1 and rp.skinny_slices(4001, 8) == 8  # dense.hip: "n = 4001, Bt = 8: 9 -> 8 slices"
    assert rp.skinny_slices(4032, 64) == 4  # dense.hip: "63 row blocks x 4 slices"
    assert [rp.fused_tier(n) for n in (1, 256, 257, 8192, 8193)] == [(1, 256), (1, 256), (2, 256), (8, 1024), None]
    assert rp.update_threads(8192) == 256 and rp.update_threads(8193) == 1024


def test_no_case_takes_the_tile_scheme_and_ids_are_unique():
    assert len({c.id for c in rp.CASES}) == len(rp.CASES)
    for c in rp.CASES:
        assert not c.takes_dense1, c.id
        assert c.k <= 5  # the smallest 0.5 rz stays above min_float: no guard fires


def test_every_tier_is_entered_on_both_sides_of_its_edge():
    fused = [c for c in rp.CASES if c.fused and c.dtype == "f64" and not c.resets]
    for pre in ("eye", "jacobi"):
        sizes = {c.n for c in fused if c.pre == pre}
        for top, ept, nt in rp.FUSED_TIERS[:-1]:
            assert top in sizes and top + 1 in sizes, (pre, top)
            assert rp.fused_tier(top) == (ept, nt) != rp.fused_tier(top + 1)
        assert rp.FUSED_MAX_N in sizes
        # beyond the last tier: the generic kernel, same preconditioner
        assert any(c.n == rp.FUSED_MAX_N + 1 and c.pre == pre and not c.fused and not c.resets for c in rp.CASES)
    assert {rp.fused_tier(c.n) for c in fused} == {(e, t) for _, e, t in rp.FUSED_TIERS}


def test_each_thread_count_family_meets_a_deferred_and_a_reduced_product():
    fused = [c for c in rp.CASES if c.fused and c.dtype == "f64" and not c.resets]
    for nt in (256, 1024):
        ks = [c.slices for c in fused if rp.fused_tier(c.n)[1] == nt]
        assert any(rp.deferred(k) for k in ks) and any(not rp.deferred(k) for k in ks), (nt, ks)
    assert {1, 4, 5, 7, 8, 9, 11, 16} <= {c.slices for c in fused}
    # both ends of the deferred range's upper edge: 8 slices are left to the update, 9 are not
    assert rp.deferred(8) and not rp.deferred(9) and not rp.deferred(1)


def test_both_update_block_sizes_and_all_six_modes():
    seen = {}
    for c in rp.CASES:
        for m in c.modes:
            seen.setdefault(rp.update_threads(c.n), set()).add(m)
    assert seen[256] == {0, 1, 2, 3, 4, 5} == seen[1024], seen
    # the refresh steps of a fused solve go through the generic kernel too
    assert any(c.fused and c.resets and c.modes == {1, 2} for c in rp.CASES)
    # the recording solve and the fp32 rows: one per (EPT, NT) pair up to n = 2049
    assert sum(c.record for c in rp.CASES) == 1
    f32 = [c for c in rp.CASES if c.dtype == "f32"]
    assert sorted(rp.fused_tier(c.n) for c in f32) == sorted({rp.fused_tier(n) for n in range(1, 2050)})
    assert all(c.n <= 2049 and c.k == 3 and c.fused and len(c.note) == 2 for c in f32)


def test_systems_are_seeded_symmetric_and_the_blocks_disjoint():
    A = rp.matrix(257)
    assert np.array_equal(A, A.T) and np.array_equal(A, rp.matrix(257))
    assert np.linalg.eigvalsh(A)[0] >= 2.0 - 1e-12
    P = rp.dense_pinv(333)
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P)[0] >= 0.5 - 1e-12
    idx = rp.block_indices(512)
    assert idx.shape == (3, 8) and len(np.unique(idx)) == 24 and idx.min() >= 0 and idx.max() < 512
    c = next(c for c in rp.CASES if c.start == "v0")
    assert np.any(rp.start(c) != 0) and rp.rhs(c).shape == (c.Bt, c.n)
