"""The seam plan on the CPU: every planned case crosses the cuts it targets, ends each targeted axis in a ragged
chunk, and checks both sides of every cut (tests/seam_plan.py; the values are checked by tests/test_gpu_seams.py)."""

import numpy as np
import pytest

import seam_plan as sp


def _pow2(n):
    return n & (n - 1) == 0


@pytest.mark.parametrize("case", sp.CASES, ids=repr)
def test_case_crosses_its_cuts_and_ends_ragged(case):
    plan = case.plan
    assert set(case.targeted) <= set(plan.axes)
    for axis in case.targeted:
        n, cl = plan.axes[axis]
        assert len(cl) >= 1, (case.id, axis)
        assert all(0 < c < n for c in cl) and cl == sorted(set(cl))
    for axis in case.targeted:
        if case.entry == "project_fused" and axis == "streamed":
            continue  # the union of two launches' splits: not one chunk length
        n, cl = plan.axes[axis]
        step = plan.chunk[axis]
        assert cl == sp.cuts(n, step)
        assert 0 < n - cl[-1] < step, (case.id, axis, n - cl[-1], step)  # a ragged last chunk
    # the cut was needed: the arena the rule asks for is smaller than one panel over the whole shape
    assert plan.arena[1] < plan.whole, case.id
    lo, hi = sp.arena_window(plan)
    assert lo <= sp.reserved_bytes(plan.arena[1]) <= hi
    assert abs(sp.asked_bytes(sp.reserved_bytes(plan.arena[1])) - plan.arena[1]) <= 1


def test_fused_projection_launches_split_n_differently():
    for case in sp.cases("project_fused"):
        launches = case.plan.launches
        assert len(launches) == 2 and launches[1][0] == sp.PJ_CHUNK_B
        assert launches[0][2:] != launches[1][2:], launches
        assert len(case.plan.cuts("streamed")) >= 2
        # the same holds with a few CUs fewer
        for cus in (228, 240):
            alt = sp.project_fused(case.shape[0], case.shape[1], case.D, case.opts["r"], cus).launches
            assert alt[0][2:] != alt[1][2:]


def test_every_route_has_a_chunk_that_is_no_power_of_two():
    """Per route (chunk rule), not per exported name: mgp_knm_project's generic route must not pass on the fused one."""
    for entry in sorted(sp.API):
        lengths = [c.plan.chunk[a] for c in sp.cases(entry) for a in c.targeted]
        lengths += [rw for c in sp.cases(entry) for _, _, _, rw in getattr(c.plan, "launches", [])]
        assert any(not _pow2(v) for v in lengths), (entry, lengths)


def test_every_entry_point_meets_every_kernel_kind_or_rotates():
    for entry in sorted(set(sp.API)):
        kinds = [c.kind for c in sp.cases(entry)]
        assert len(set(kinds)) == min(len(kinds), 4), (entry, kinds)
    assert {c.kind for c in sp.CASES} == set(sp.KINDS)


@pytest.mark.parametrize("case", sp.CASES, ids=repr)
def test_checked_indices_sit_on_both_sides_of_every_cut(case):
    for axis, (n, cl) in case.plan.axes.items():
        for idx in (case.rows(axis), case.support(axis)):
            assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == n - 1
            have = set(idx.tolist())
            for c in cl:
                assert {c - 1, c, c + 1} & set(range(n)) <= have, (case.id, axis, c)
            forced = {0, n - 1} | {i for c in cl for i in (c - 1, c, c + 1)}
            assert len(have - forced) >= 8  # 8 seeded random ones on top, none coinciding with a forced index
        assert len(set(case.rows(axis).tolist()) - forced) == 8
        rows = case.rows(axis)
        assert np.array_equal(rows, case.rows(axis))  # seeded: the same on every call
        assert len(case.support(axis)) >= min(n, 30)
    drawn = sp.check_indices(10 ** 6, [], 3)
    assert len(drawn) == 10  # the first, the last and 8 random ones


def test_rules_at_the_clamps():
    # sweep: at least 64 owned rows however wide the streamed side (csrc/generic.hip:132); never more than na above that
    assert sp.sweep_generic(10, 16384, 1, np.float64).chunk["owned"] == 64
    assert sp.sweep_generic(100, 50, 1, np.float64).chunk == {"owned": 100, "streamed": 50}
    # projection: the clamp to B comes last (csrc/project.hip:307-308)
    assert sp.project_generic(10, 16384, 4, np.float64, True, True).chunk["owned"] == 10
    # column sums: a multiple of 256, at least 256
    assert sp.sq_colsum_generic(100, 5, np.float64).chunk["rows"] == 256
    assert sp.sq_colsum_generic(6913, 5000, np.float64).chunk["rows"] == 6656
    # the figures of the issue's table
    assert sp.sweep_generic(7010, 5000, 1, np.float64).cuts("owned") == [6710]
    assert sp.sweep_generic(8197, 16421, 1, np.float32).cuts("owned") == [4096, 8192]
    assert sp.kgrad_panel(6000, np.float64).chunk["rows"] == 5592
    assert sp.kgrad_panel(8500, np.float32).chunk["rows"] == 7895
    assert sp.rff_panel_rows(1024, np.float64) == 16384 and sp.rff_panel_rows(1024, np.float32) == 32768
    assert len(sp.sweep_generic(16421, 16421, 3, np.float64).cuts("owned")) == 8  # 9 row chunks
