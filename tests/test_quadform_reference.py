"""tests/quadform_reference.py held honest on the CPU: the upper-triangle definition is k^T sym(C) k, the prefix forms
are the forms of the leading blocks, NaN below the diagonal cannot reach the reference, and the SGPR variance matrix of
`SGPR.variance_matrix` reproduces the variance of the two-Cholesky closed form (oracle.models.SGPR.predict_f)."""

import numpy as np
import pytest

import pair_reference as pr
import quadform_reference as qr
from oracle import kernels as ok, models as om

LD = np.longdouble


def _problem(B=37, M=29, D=3, name="matern32", seed=0):
    rng = np.random.default_rng(seed)
    ls = pr.lengthscales(D)
    Xs, Z = rng.standard_normal((B, D)), rng.standard_normal((M, D))
    G = rng.standard_normal((M, M))
    return name, ls, Xs, Z, G @ G.T / M + np.diag(rng.random(M)), rng


def test_upper_triangle_definition_is_the_symmetric_form():
    name, ls, Xs, Z, C, rng = _problem()
    k = pr.pair_values(name, pr.VARIANCE, ls, Xs, Z).k
    q, mag = qr.form(k, C)
    ref = qr.symmetric_form(k, C)
    assert np.max(np.abs(q - ref) / mag) < 1e-17
    # and the plain symmetric product on symmetric input
    full = np.einsum("bi,ij,bj->b", k, C.astype(LD), k)
    assert np.max(np.abs(q - full) / mag) < 1e-17
    # an unsymmetric lower triangle does not enter
    C2 = C.copy()
    C2[np.tril_indices(C.shape[0], -1)] = np.nan
    q2, mag2 = qr.form(k, C2)
    assert np.array_equal(q2, q) and np.array_equal(mag2, mag)
    # an indefinite matrix: the magnitude dominates the form
    Ci = C - 2.0 * np.diag(np.diag(C))
    qi, magi = qr.form(k, Ci)
    ev = np.linalg.eigvalsh(Ci)
    assert ev[0] < 0 < ev[-1] and np.all(np.abs(qi) <= magi) and np.all(magi >= mag * (1 - 1e-15))


def test_prefix_forms_are_the_forms_of_the_leading_blocks():
    name, ls, Xs, Z, C, rng = _problem(B=11, M=23)
    k = pr.pair_values(name, pr.VARIANCE, ls, Xs, Z).k
    Q, MAG = qr.prefix_forms(k, C)
    for m in (1, 2, 7, 23):
        q, mag = qr.form(k[:, :m], C[:m, :m])
        assert np.max(np.abs(Q[:, m - 1] - q) / mag) < 1e-17 and np.max(np.abs(MAG[:, m - 1] - mag) / mag) < 1e-17
    q0, mag0 = qr.form(k[:, :0], C[:0, :0])
    assert q0.shape == (11,) and not q0.any() and not mag0.any()
    assert qr.bound(0.0, 23, MAG[:, -1], np.float64).shape == (11,)
    assert np.allclose(qr.bound(1e-15, 4, 2.0, np.float64), (2e-15 + 8 * 2.0 ** -53) * 2.0, rtol=1e-12)


@pytest.mark.parametrize("lengthscale", [1.0, 0.4])
@pytest.mark.parametrize("N,M", [(1500, 30), (4000, 300)])
def test_sgpr_variance_matrix_reproduces_the_closed_form(N, M, lengthscale):
    """var = k** - k^T C k against oracle.models.SGPR.predict_f to 1e-9 (jitter 1e-6, noise 0.1, the data of
    tests/test_gpu_parity.py's `model_problem`: D = 2, seed 3); the form is evaluated in long double so that what is
    measured is the matrix.

    What the route can and cannot do, measured with a long-double closed form as the truth: the oracle is within 1e-11 of
    it; a C formed in long double and rounded to fp64 within 6e-12; this route within 4.2e-11 (M = 30) and 2.6e-10
    (M = 300, lengthscales 1.0 and 0.4, cond(Kmm) 1.3e8 and 4.2e7).  What is left comes from the fp64 rounding of the cached K_mn K_nm, which
    L^-1 . L^-T amplifies in the directions of the small eigenvalues of Kmm: forming AAT from L^-1 K_mn instead (an
    N-sized product the model does not make) leaves 1.6e-11, and no M-sized rearrangement of the later steps (I - B^-1,
    an eigendecomposition of AAT, Kmm^-1 K_mn K_nm S^-1) changes it.  On other draws of the data at cond(Kmm) ~ 1e8 it ranged
    from 2e-10 to 7e-9, so 1e-9 is the bar on these cases, not a property of every data set; the models' 1e-6 has three
    orders of room."""
    rng = np.random.default_rng(3)
    D = 2
    X = rng.standard_normal((N, D))
    y = np.sin(X).sum(1, keepdims=True) + 0.3 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)]
    kern = ok.Kernel("se", 1.1, np.full(D, lengthscale))
    Xs = X[:200] + 0.1
    _, var0 = om.SGPR((X, y), kern, Z, 0.1, jitter=1e-6).predict_f(Xs)
    C = qr.sgpr_variance_matrix(X, Z, kern, 0.1, 1e-6)
    assert np.array_equal(C, C.T)
    ks = ok.Kuf(Z, kern, Xs).T  # [B, M]
    q, _ = qr.form(ks, C)
    var = kern.K_diag(Xs).astype(LD) - q
    err = float(np.max(np.abs(var - var0[:, 0])))
    cond = np.linalg.cond(ok.Kuu(Z, kern, jitter=1e-6))
    qs, _ = qr.form(ks, qr.sgpr_variance_matrix_subtractive(X, Z, kern, 0.1, 1e-6))
    err_sub = float(np.max(np.abs(kern.K_diag(Xs).astype(LD) - qs - var0[:, 0])))
    print(f"N={N} M={M} l={lengthscale}: cond(Kmm) {cond:.2e}, |var - oracle| {err:.2e} (subtractive form {err_sub:.2e})")
    assert err < 1e-9
