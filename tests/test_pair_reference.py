"""tests/pair_reference.py held honest on the CPU: its long-double kernel values against mpmath at 40 digits, and its
rounding bound against two float64 evaluations that are known to be correct -- the oracle (an expansion form, like the
device's) and the host build of csrc/mgp_math.h.  The bound's constants are fixed by the derivation in
`pair_reference.pair_bound`; these tests show a correct evaluation stays inside them."""

import ctypes
import os
import subprocess

import mpmath
import numpy as np
import pytest

import pair_reference as pr
from oracle.kernels import Kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "csrc")
SO = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd", "cggp", "libmgp_hostmath.so")
LD = np.longdouble
VAR = pr.VARIANCE


def cloud_set(name, D, N, M, shift, seed=0):
    """Standard-normal clouds in natural units moved `shift` along every axis, a tenth of Z copied from X."""
    rng = np.random.default_rng([seed, 4, D, int(shift)])
    X, Z = rng.standard_normal((N, D)) + shift, rng.standard_normal((M, D)) + shift
    Z[: M // 10] = X[: M // 10]
    return X, Z, pr.lengthscales(D)


def point_sets(name, D):
    """(label, X, Z, ls, cols): every set the GPU probes use, smaller, and the clouds the bound was first checked on."""
    X, Z, ls, _ = pr.range_set(name, D, 1 << 13)
    yield "range", X, Z, ls, None
    X, Z, ls = pr.shifted_set(name, D, 300, 200)
    yield "shifted", X, Z, ls, None
    X, Z, ls, far = pr.edge_set(name, D, 2300, 130)
    yield "edge", X, Z, ls, [0, 1, 2, 64, 129]
    for shift in (0, 3, 10):
        X, Z, ls = cloud_set(name, D, 200, 150, shift)
        yield f"cloud+{shift}", X, Z, ls, None


def _mpf(x):
    m, e = np.frexp(LD(x))
    return mpmath.mpf(int(m * LD(2) ** 64)) * mpmath.mpf(2) ** (int(e) - 64)


def _k_mp(name, variance, ls, x, z):
    r2 = sum(((mpmath.mpf(float(a)) - mpmath.mpf(float(b))) / mpmath.mpf(float(l))) ** 2 for a, b, l in zip(x, z, ls))
    if name == "se":
        return mpmath.mpf(variance) * mpmath.exp(-r2 / 2)
    r = mpmath.sqrt(max(r2, mpmath.mpf(10) ** -36))
    if name == "matern12":
        return mpmath.mpf(variance) * mpmath.exp(-r)
    a = mpmath.sqrt(3 if name == "matern32" else 5) * r
    poly = 1 + a if name == "matern32" else 1 + a + a * a / 3
    return mpmath.mpf(variance) * poly * mpmath.exp(-a)


@pytest.mark.parametrize("name", pr.KINDS)
def test_long_double_values_agree_with_mpmath(name):
    """About 500 pairs per kernel (2000 in all) from every point set, every D: 1e-18 relative, far pairs included."""
    worst, count = 0.0, 0
    with mpmath.workprec(140):
        for D in (1, 3, 8, 32):
            for label, X, Z, ls, cols in point_sets(name, D):
                rng = np.random.default_rng(count)
                cols = list(range(Z.shape[0])) if cols is None else cols
                rows = np.unique(np.concatenate([rng.choice(X.shape[0], 18), [0, X.shape[0] - 1]]))
                cj = [cols[c] for c in rng.choice(len(cols), 2)]
                if label == "edge":  # the far rows against the far column: s* ~ 1000
                    rows, cj = np.concatenate([rows, pr.edge_set(name, D, 2300, 130)[3][-4:]]), [0, cj[1]]
                pv = pr.pair_values(name, VAR, ls, X[rows], Z, cj)
                for a, i in enumerate(rows):
                    for b, j in enumerate(cj):
                        want = _k_mp(name, VAR, ls, X[i], Z[j])
                        err = abs(_mpf(pv.k[a, b]) / want - 1)
                        worst, count = max(worst, float(err)), count + 1
                        assert err < 1e-18, (name, D, label, int(i), int(j), float(pv.s[a, b]), float(err))
    assert count >= 500, count
    print(f"{name}: {count} pairs, worst relative difference {worst:.2e}")


def test_derivatives_are_those_of_the_profile():
    """dk/dvariance, dk/dl_d, dk/dz_d against central differences of the long-double k (step 1e-6: 1e-9 relative)."""
    for name in pr.KINDS:
        X, Z, ls = pr.shifted_set(name, 3, 40, 30)
        pv = pr.pair_values(name, VAR, ls, X, Z, derivs=True)
        h = 1e-6
        assert np.allclose((pv.k / LD(VAR)).astype(float), pv.dk_dvariance.astype(float), rtol=1e-15)
        for d in range(3):
            lp, lm, Zp, Zm = ls.copy(), ls.copy(), Z.copy(), Z.copy()
            lp[d] += h
            lm[d] -= h
            Zp[:, d] += h
            Zm[:, d] -= h
            fl = (pr.pair_values(name, VAR, lp, X, Z).k - pr.pair_values(name, VAR, lm, X, Z).k) / LD(lp[d] - lm[d])
            fz = (pr.pair_values(name, VAR, ls, X, Zp).k - pr.pair_values(name, VAR, ls, X, Zm).k) / (Zp[:, d] - Zm[:, d])
            m = pv.s > 1e-6  # off the duplicates (Matern-1/2 has a cusp there)
            scale = np.abs(pv.k).astype(float)
            assert np.all(np.abs((fl - pv.dk_dls[:, :, d]).astype(float))[m] <= 1e-8 * scale[m]), (name, d)
            assert np.all(np.abs((fz - pv.dk_dz[:, :, d]).astype(float))[m] <= 1e-8 * scale[m]), (name, d)


@pytest.mark.parametrize("D", [1, 3, 8, 32])
@pytest.mark.parametrize("name", pr.KINDS)
def test_float64_oracle_stays_under_the_bound(name, D):
    worst = 0.0
    for label, X, Z, ls, cols in point_sets(name, D):
        Zc = Z if cols is None else Z[cols]
        got = Kernel(name, VAR, ls).K(X, Zc)
        pv = pr.pair_values(name, VAR, ls, X, Zc)
        rel = pr.pair_bound(name, VAR, pv.s, pv.q, pr.scaled(name, ls, X), pr.scaled(name, ls, Zc), D, np.float64)
        worst = max(worst, pr.check_pairs(f"oracle {name} D={D} {label}", got, pv, rel, VAR, np.float64))
    print(f"{name} D={D}: worst err / bound {worst:.3f}")
    assert worst < 1.0


@pytest.fixture(scope="module")
def hm():
    so = os.environ.get("MGP_HOSTMATH_LIBRARY")  # as tests/test_host_math.py
    if not so:
        subprocess.run(["make", "-C", CSRC, "hostmath"], check=True, capture_output=True)
        so = SO
    lib = ctypes.CDLL(so)
    lib.mgp_host_profile.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    return lib


@pytest.mark.parametrize("kind,name", list(enumerate(pr.KINDS)))
def test_host_math_stays_under_the_value_part_of_the_bound(hm, kind, name):
    """mgp_profile of the host build at fl(s*): the distance part of the bound is replaced by what rounding s* to fp64
    leaves (u s*, i.e. ln2 u s* in an SE value and ln2 u q* / 2 in a Matern one); F u and the square root's 2 u ln2 q*
    stay."""
    u, ln2 = 2.0 ** -53, float(np.log(2.0))
    worst = 0.0
    for D in (1, 8):
        for label, X, Z, ls, cols in point_sets(name, D):
            Zc = Z if cols is None else Z[cols]
            pv = pr.pair_values(name, VAR, ls, X, Zc)
            s64 = np.ascontiguousarray(pv.s.astype(np.float64)).ravel()
            out = np.empty_like(s64)
            hm.mgp_host_profile(kind, s64.ctypes.data, out.ctypes.data, s64.size)
            q = pv.q.astype(np.float64)
            rel = pr.FUNCTION_BUDGET * u + (ln2 * u * pv.s.astype(np.float64) if name == "se" else 2.5 * u * ln2 * q)
            worst = max(worst, pr.check_pairs(f"host math {name} D={D} {label}", VAR * out.reshape(pv.k.shape), pv, rel,
                                              VAR, np.float64))
    print(f"{name}: worst err / bound {worst:.3f}")
    assert worst < 1.0
