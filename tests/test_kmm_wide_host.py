"""CPU side of the many-column (K_mm + Lambda) operator: the long-double reference of tests/kmm_wide_reference.py held
to a plain float64 product, its cut plan and case list, the `wide="auto"` rule and the argument refusals (which are
raised before any device call)."""

import numpy as np
import pytest
import torch

import kmm_wide_reference as kr
from oracle import kernels as ok


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("kind", kr.KINDS)
@pytest.mark.parametrize("M,D,Bt", [(1, 1, 3), (37, 3, 5), (130, 9, 17)])
def test_reference_matches_a_float64_product(kind, M, D, Bt):
    """Against oracle/kernels.py in float64: 1e-12 of the largest entry (float64 rounding of an M-term sum of O(1)
    terms is ~M 1e-16); Matern-1/2 1e-7, the cusp of the oracle's expansion-form distance at coincident points
    (r = sqrt(max(r2, 1e-36)) with r2 ~ 1e-16 on the diagonal: tests/test_gpu_gpr.py `bar`)."""
    Z, ls, lam = kr.inputs(M, D)
    P = np.random.default_rng(M).standard_normal((Bt, M))
    K = kr.kmm_matrix(kind, kr.VARIANCE, ls, Z)
    assert K.dtype == np.longdouble and np.array_equal(K, K.T)
    ref = kr.product(K, lam, P)
    plain = P @ (ok.Kernel(kind, kr.VARIANCE, ls).K(Z) + np.diag(lam))
    dist = float(np.max(np.abs(ref - plain)) / np.max(np.abs(plain)))
    print(f"{kind} M={M} D={D}: {dist:.2e}")
    assert dist < (1e-7 if kind == "matern12" else 1e-12)
    rows = [0, Bt - 1]
    assert np.array_equal(kr.product(K, lam, P, rows), ref[rows])


def test_reference_diagonal_and_lambda_term():
    Z, ls, lam = kr.inputs(20, 3)
    K = kr.kmm_matrix("se", 1.3, ls, Z)
    assert np.all(K.diagonal() == np.longdouble(1.3))
    out = kr.product(K, lam, np.eye(20))
    assert np.array_equal(out, K + np.diag(lam.astype(np.longdouble)))


# ---------------------------------------------------------------- the cut plan
def test_groups_tiles_and_splits():
    assert kr.groups(1) == [(0, 1)] and kr.groups(256) == [(0, 256)]
    assert kr.groups(257) == [(0, 256), (256, 1)] and kr.groups(600) == [(0, 256), (256, 256), (512, 88)]
    assert [kr.row_tile(w) for w in (1, 128, 129, 256)] == [128, 128, 64, 64]
    # at least 1024 streamed rows per split: one split up to 1024 rows, two from 1025 on wherever the row tiles leave
    # the chip unfilled (4 workgroups per CU)
    for cus in (64, 256, 1000):
        assert kr.splits(1, 1024, cus)[0] == 1
        assert kr.splits(1, 1025, cus) == (2, 528)
        assert kr.splits(17, 2049, cus) == (3, 688)
    ns, rw = kr.splits(2048, 1 << 17, 256)  # a large launch fills the chip by its row tiles alone
    assert (ns, rw) == (1, 1 << 17)
    for tiles, M in [(1, 1), (3, 2065), (9, 1040), (40, 5000)]:
        ns, rw = kr.splits(tiles, M, 256)
        assert rw % kr.STEP == 0 and (ns - 1) * rw < M <= ns * rw


def test_plan_covers_every_output_once_and_sizes_the_arena():
    for M, Bt in [(1, 1), (129, 300), (2065, 257), (70000, 130)]:
        seen = np.zeros((Bt, M), dtype=np.int32)
        for p in kr.plan(M, Bt):
            assert p["padded"] % 16 == 0 and p["width"] <= p["padded"] < p["width"] + 16
            assert p["tiles"] * p["tile"] >= p["rows"] > (p["tiles"] - 1) * p["tile"]
            seen[p["g0"]:p["g0"] + p["width"], p["c0"]:p["c0"] + p["rows"]] += 1
        assert np.all(seen == 1)
    assert kr.arena_bytes(300, 3, 16) == 12032 + 8 * 1 * 3 * 128 * 16  # pack 300 x (4 + 1) doubles rounded up to 256, one split
    assert kr.arena_bytes(2049, 8, 257) >= kr.arena_bytes(2049, 8, 256) > kr.arena_bytes(2049, 8, 128)
    with pytest.raises(ValueError):
        kr.dp_of(33)


def test_product_cases_hit_every_cut():
    cases = kr.product_cases()
    assert {c[0] for c in cases} == set(kr.KINDS) and {c[1] for c in cases} == set(kr.PRODUCT_D)
    for kind in kr.KINDS:
        assert sorted(c[2] for c in cases if c[0] == kind) == sorted(kr.PRODUCT_M)
    hit = set()
    for kind, D, M, cols in cases:
        for Bt in cols:
            for p in kr.plan(M, Bt):
                hit.add((p["tile"], min(p["splits"], 2), len(kr.groups(Bt)), p["padded"] // 16 * 16 == p["width"],
                         M % p["tile"] == 0 or M < p["tile"] or M % p["tile"] == 1))
            probed = kr.probed_columns(M, Bt)
            assert probed[0] == 0 and probed[-1] == Bt - 1 and (M > 129 or len(probed) == Bt)
    # both tiles, one split and several, one group and two
    assert {(t, s, g) for t, s, g, _, _ in hit} >= {(128, 1, 1), (64, 1, 1), (128, 2, 1), (64, 2, 1), (64, 1, 2),
                                                   (128, 1, 2), (64, 2, 2), (128, 2, 2)}
    big = [(M, Bt) for _, _, M, cols in cases if M > 129 for Bt in cols]
    assert {Bt for _, Bt in big} == set(kr.PRODUCT_COLUMNS)  # every column count meets a split launch
    assert all(kr.plan(M, Bt)[0]["splits"] >= 2 for M, Bt in big)


# ---------------------------------------------------------------- the "auto" rule and the refusals
def test_auto_rule_truth_table():
    from cggp import conjugate_gradient as cg
    C, M = cg.WIDE_MIN_COLUMNS, cg.WIDE_MIN_M
    f64, f32 = torch.float64, torch.float32
    assert cg.wide_auto(f64, 8, C, M) and cg.wide_auto(f64, 32, C + 1, 2 * M) and cg.wide_auto(f64, 1, 10 * C, M)
    assert not cg.wide_auto(f32, 8, C, M)
    assert not cg.wide_auto(f64, 33, C, M)
    assert not cg.wide_auto(f64, 8, C - 1, M)
    assert not cg.wide_auto(f64, 8, C, M - 1)
    assert cg.WIDE_MAX_D == kr.FUSED_MAX_D


class _Kernel:
    variance = 1.0

    def spec(self, D):
        raise AssertionError("the refusal comes first")


@pytest.mark.parametrize("bad", [None, 1, 0, "yes", "AUTO", 2.0])
def test_wide_argument_refusals(bad):
    from cggp.conjugate_gradient import KmmLambdaOperator, check_wide
    from cggp.models import CGGP
    from cggp.training import TrainableCGGP
    Z, lam = torch.zeros((4, 2), dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="wide must be"):
        KmmLambdaOperator(_Kernel(), Z, lam, wide=bad)
    with pytest.raises(ValueError, match="wide_solves must be"):
        CGGP(_Kernel(), 0.1, Z, None, matrix_free=True, wide_solves=bad)
    with pytest.raises(ValueError, match="wide_solves must be"):
        TrainableCGGP(_Kernel(), 0.1, Z, pseudo_u=lam, cluster_counts=lam, matrix_free=True, wide_solves=bad)
    for good in (False, True, "auto"):
        assert check_wide(good) is good


@pytest.mark.parametrize("value", [True, "auto"])
def test_wide_solves_needs_matrix_free(value):
    from cggp.models import CGGP, cdgp_class
    from cggp.training import TrainableCGGP
    Z, lam = torch.zeros((4, 2), dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="matrix_free=True"):
        CGGP(_Kernel(), 0.1, Z, None, wide_solves=value)
    with pytest.raises(ValueError, match="matrix_free=True"):
        cdgp_class(_Kernel(), 0.1, Z, wide_solves=value)
    with pytest.raises(ValueError, match="matrix_free=True"):
        TrainableCGGP(_Kernel(), 0.1, Z, pseudo_u=lam, cluster_counts=lam, wide_solves=value)


def test_kind_constant():
    from cggp import _hip
    assert (_hip.OP_KMM_LAMBDA, _hip.OP_KMM_LAMBDA_WIDE) == (2, 4)
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mgp.h")).read()
    assert "MGP_OP_KMM_LAMBDA_WIDE = 4" in header
