"""Host-side checks of the pivoted-Cholesky preconditioner for matrix-free CDGP: `set_factor(L, lam)` with a vector
diagonal against the numpy restatement of P = L^T L + Lambda (tests/cdgp_precond_reference.py), the `wide="auto"`
truth table and the argument refusals, the mirror of `MGP_PRE_LOWRANK_WIDE`, and the reference's own step counts on
the inputs of the GPU tests (tests/test_gpu_cdgp_precond.py holds the device to them)."""

import re

import numpy as np
import pytest
import torch

import cdgp_precond_reference as cr
from cggp import _hip
from cggp import conjugate_gradient as cgm
from cggp.conjugate_gradient import PivotedCholeskyPreconditioner


@pytest.fixture(scope="module")
def table_system():
    """SE, D = 2, lengthscale 1.5 at M = 2048: the system of the GPU iteration-count test."""
    K, lam, b = cr.system("se", 2, 1.5)
    return K, lam, b, cr.preconditioner(K, lam, 64)


def test_set_factor_with_a_vector_diagonal_is_the_inverse_of_p(table_system):
    K, lam, _, (dinv, B, log_det) = table_system
    M = K.shape[0]
    assert lam.min() < 0.002 and lam.max() == 0.1  # small and uneven: 0.1 / (1 ... 64)
    L, _ = cr.greedy_pivoted_cholesky(K, 64)
    P = L.T @ L + np.diag(lam)
    pre = PivotedCholeskyPreconditioner(rank=64).set_factor(torch.from_numpy(L), torch.from_numpy(lam))
    assert pre.rank_ == 64 and pre.diag_inv.shape == (M,)
    Pinv_P, _ = pre(torch.from_numpy(P), None)  # the rows of P through P^-1
    err = float(np.max(np.abs(Pinv_P.numpy() - np.eye(M))))
    print(f"|P^-1 P - I| = {err:.3e}")
    assert err <= 1e-10
    sld = np.linalg.slogdet(P)[1]
    assert abs(pre.log_det() - sld) <= 1e-12 * abs(sld)
    # the reference's Woodbury factor is the same map
    assert abs(log_det - sld) <= 1e-12 * abs(sld)
    z_ref, _ = cr.apply_reference(dinv, B, P[:5])
    assert np.max(np.abs(z_ref - np.eye(M)[:5])) <= 1e-10
    with pytest.raises(ValueError, match="positive"):
        pre.set_factor(torch.from_numpy(L), torch.from_numpy(np.where(np.arange(M) == 7, 0.0, lam)))


def test_auto_truth_table_and_argument_refusals(monkeypatch):
    for wide in (False, True, "auto"):
        assert PivotedCholeskyPreconditioner(wide=wide).wide == wide
    assert PivotedCholeskyPreconditioner().wide is False
    for bad in (None, 1, 0, "yes", "AUTO"):
        with pytest.raises(ValueError, match="wide"):
            PivotedCholeskyPreconditioner(wide=bad)
    f64, f32 = torch.float64, torch.float32
    always, never, auto = (PivotedCholeskyPreconditioner(wide=w) for w in (True, False, "auto"))
    for cols in (1, 16, 64, 10 ** 6):
        assert always._wide_for(f64, cols) and not always._wide_for(f32, cols)
        assert not never._wide_for(f64, cols) and not never._wide_for(f32, cols)
    monkeypatch.setattr(cgm, "LOWRANK_WIDE_MIN_COLUMNS", 48)
    assert [auto._wide_for(f64, c) for c in (1, 47, 48, 49, 256)] == [False, False, True, True, True]
    assert not any(auto._wide_for(f32, c) for c in (1, 48, 256))
    monkeypatch.setattr(cgm, "LOWRANK_WIDE_MIN_COLUMNS", None)  # no width qualified: never
    assert not any(auto._wide_for(f64, c) for c in (1, 48, 256, 10 ** 6))


def test_the_module_constant_is_none_or_a_measured_width():
    w = cgm.LOWRANK_WIDE_MIN_COLUMNS
    assert w is None or w in (16, 24, 32, 48, 64, 128, 256)  # the widths tools/run_cdgp_precond.py measures


def test_the_kind_is_mirrored_and_the_header_names_it():
    import os
    assert (_hip.PRE_LOWRANK, _hip.PRE_LOWRANK_WIDE) == (5, 6)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mgp.h")).read()
    assert re.search(r"MGP_PRE_LOWRANK_WIDE\s*=\s*6\b", text)
    assert re.search(r"#define MGP_VERSION 210\b", text)  # no version change


def test_other_operators_are_refused_with_a_pointer_to_matrix_free():
    class Other:
        shape = (4, 4)
        dtype = torch.float64

    with pytest.raises(TypeError, match="matrix_free=True") as info:
        PivotedCholeskyPreconditioner()._native(Other())
    assert "set_factor" in str(info.value) and "KmmLambdaOperator" in str(info.value)


def test_cdgp_class_hands_the_preconditioner_to_its_solver():
    import inspect
    from cggp import models
    sig = inspect.signature(models.cdgp_class)
    assert list(sig.parameters)[:5] == ["kernel", "likelihood", "iv", "error_threshold", "preconditioner"]
    assert sig.parameters["preconditioner"].default is None


def test_reference_step_counts_on_the_gpu_test_inputs(table_system):
    """The caps of the GPU test hold for the reference alone: 10 x preconditioned <= identity (4 against 408 when the
    feature was specified), and Jacobi does nothing."""
    K, lam, b, _ = table_system
    ident, jac, pc = cr.steps(K, lam, b), cr.steps(K, lam, b, jacobi=True), cr.steps(K, lam, b, rank=64)
    print(f"identity {ident} jacobi {jac} rank 64: {pc}")
    assert 10 * pc <= ident and pc <= 6 and ident >= 300
    assert jac >= 0.9 * ident


def test_arena_plans():
    # Bt = 70, k = 33, n = 1040 (the buffer-contract case of the GPU test): one 128 x 64 tile, 5 splits of 208 columns
    assert cr.wide_arena_bytes(70, 33, 1040, 256) == 8 * (5 + 1) * 128 * 64
    assert cr.narrow_arena_bytes(70, 33, 1040) == (9 + 1) * 16 * 33 * 8
    # bounded whatever n: at most 8 (4 CUs + 64) 128 64 bytes
    for n in (1, 1 << 12, 1 << 17, 1 << 22):
        for Bt, k in ((48, 1), (256, 128), (257, 130), (300, 1024)):
            assert 0 < cr.wide_arena_bytes(Bt, k, n, 256) <= 8 * (4 * 256 + 64) * 128 * 64
