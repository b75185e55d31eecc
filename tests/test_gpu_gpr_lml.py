"""Matrix-free exact-GPR marginal likelihood on the MI355X: the pair kernel of the hyper-parameter bilinear forms
(`mgp_kxx_grad`) against long double, its routes and determinism, the recording CG (`mgp_pcg_solve_record`) against
the plain solve and a numpy CG, the stochastic Lanczos estimate against eigh / slogdet, its gradient against the
Cholesky autograd, Adam training, and one N = 2^17 evaluation within a bounded memory footprint."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

from lml_reference import kxx_grad_reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KXX_GRAD_BAR = 1e-11  # of the sum of |terms|, against long double (shared with tests/test_gpu_ladder.py)


def _data(N, D, seed, dup=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (N, D))
    if dup:
        X[-dup:] = X[:dup]  # duplicate rows: r = 0 between distinct indices
    return X


def _call(hd, spec, X, U, V, layout=0):
    dv = ctypes.c_double(0.0)
    dl = (ctypes.c_double * 512)()
    k = spec.struct(1 if X.dtype == torch.float64 else 0)
    R = U.shape[1] if layout == 0 else U.shape[0]
    hd.check(hd.lib.mgp_kxx_grad(hd.h, ctypes.byref(k), ctypes.c_void_p(X.data_ptr()), X.shape[0],
                                 ctypes.c_void_p(U.data_ptr()), ctypes.c_void_p(V.data_ptr()), R, layout,
                                 ctypes.byref(dv), dl))
    return dv.value, [dl[d] for d in range(spec.D)]


CASES = [("se", 8, 5000, 16, 0), ("se", 3, 777, 5, 0), ("matern12", 3, 777, 5, 0), ("matern32", 3, 777, 5, 0),
         ("matern52", 3, 777, 5, 0), ("se", 1, 777, 1, 0), ("se", 17, 777, 16, 0), ("matern32", 32, 777, 16, 0),
         ("se", 3, 1, 5, 0), ("matern52", 3, 2, 5, 0), ("matern12", 3, 777, 16, 40), ("matern52", 8, 777, 5, 40)]


@pytest.mark.parametrize("name,D,N,R,dup", CASES)
def test_kxx_grad_against_long_double(name, D, N, R, dup):
    from cggp import ops
    X = _data(N, D, 10 + D + N, dup)
    rng = np.random.default_rng(N + R)
    U, V = rng.standard_normal((N, R)), rng.standard_normal((N, R))
    ls = np.linspace(0.6, 1.4, D)
    spec = ops.KernelSpec(name, 1.3, list(ls), D)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dv, dl = ops.kxx_grad(spec, t(X), t(U), t(V))
    rv, rl, sv, sl = kxx_grad_reference(name, 1.3, ls, X, U, V)
    assert np.isfinite(dv) and all(np.isfinite(dl))
    assert abs(dv - float(rv)) <= KXX_GRAD_BAR * float(sv)
    for d in range(D):
        assert abs(dl[d] - float(rl[d])) <= KXX_GRAD_BAR * max(float(sl[d]), 1e-300), (d, dl[d], float(rl[d]))
    # the [R, N] layout reads the same columns
    dv2, dl2 = ops.kxx_grad(spec, t(X), t(U.T), t(V.T), layout=ops.ROWS)
    assert dv2 == dv and dl2 == dl


def test_kxx_grad_routes_and_determinism():
    from cggp import _hip, ops
    N = 1500
    rng = np.random.default_rng(5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # D = 40 > 32: panel route, against long double
    X40, U, V = _data(600, 40, 1), rng.standard_normal((600, 3)), rng.standard_normal((600, 3))
    spec40 = ops.KernelSpec("matern32", 0.9, list(np.linspace(2.0, 4.0, 40)), 40)
    dv, dl = ops.kxx_grad(spec40, t(X40), t(U), t(V))
    rv, rl, sv, sl = kxx_grad_reference("matern32", 0.9, np.linspace(2.0, 4.0, 40), X40, U, V)
    assert abs(dv - float(rv)) <= 1e-11 * float(sv)
    assert max(abs(dl[d] - float(rl[d])) / float(sl[d]) for d in range(40)) <= 1e-11
    # fp32: panel route, fp32 arithmetic
    X3 = _data(600, 3, 2)
    spec3 = ops.KernelSpec("se", 1.1, [0.7, 1.0, 1.3], 3)
    dvf, dlf = ops.kxx_grad(spec3, t(X3).float(), t(U).float(), t(V).float())
    rv, rl, sv, sl = kxx_grad_reference("se", 1.1, [0.7, 1.0, 1.3], X3, U, V)
    assert abs(dvf - float(rv)) <= 1e-5 * float(sv)
    assert max(abs(dlf[d] - float(rl[d])) / float(sl[d]) for d in range(3)) <= 1e-5
    # fused and panel routes on one fp64 problem; two calls of each are bitwise equal
    X = t(_data(N, 8, 3))
    U, V = t(rng.standard_normal((N, 16))), t(rng.standard_normal((N, 16)))
    spec = ops.KernelSpec("se", 1.2, list(np.linspace(0.8, 1.5, 8)), 8)
    hd = _hip.get_handle(DEV)
    a1, a2 = _call(hd, spec, X, U, V), _call(hd, spec, X, U, V)
    assert a1 == a2
    old = os.environ.get("MGP_KXX_GRAD")
    os.environ["MGP_KXX_GRAD"] = "panel"
    try:
        hp = _hip.Handle(DEV.index or 0)
    finally:
        if old is None:
            del os.environ["MGP_KXX_GRAD"]
        else:
            os.environ["MGP_KXX_GRAD"] = old
    hp.sync_stream()
    b1, b2 = _call(hp, spec, X, U, V), _call(hp, spec, X, U, V)
    assert b1 == b2
    assert abs(a1[0] - b1[0]) <= 1e-11 * abs(b1[0])
    assert max(abs(x - y) / abs(y) for x, y in zip(a1[1], b1[1])) <= 1e-11


def test_bad_arguments_return_codes():
    from cggp import _hip, ops
    from cggp.conjugate_gradient import KxxNoiseOperator
    from cggp import kernels
    hd = _hip.get_handle(DEV)
    k = _hip.make_kernel_struct("se", _hip.F64, 2, 1.0, [1.0, 1.0])
    X = torch.zeros((8, 2), dtype=torch.float64, device=DEV)
    U = torch.zeros((8, 2), dtype=torch.float64, device=DEV)
    dv = ctypes.c_double(0.0)
    dl = (ctypes.c_double * 512)()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    L = hd.lib
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), 8, p(U), p(U), 0, 0, ctypes.byref(dv), dl) == -1  # R < 1
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), 8, p(U), p(U), 2, 7, ctypes.byref(dv), dl) == -1  # layout
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), None, 8, p(U), p(U), 2, 0, ctypes.byref(dv), dl) == -1
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), 8, None, p(U), 2, 0, ctypes.byref(dv), dl) == -1
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), 8, p(U), p(U), 2, 0, None, dl) == -1
    assert L.mgp_kxx_grad(hd.h, ctypes.byref(k), p(X), -1, p(U), p(U), 2, 0, ctypes.byref(dv), dl) < 0
    op = KxxNoiseOperator(kernels.SquaredExponential(1.0, [1.0, 1.0]), X, 0.1)
    st, keep = op._struct()
    B = torch.ones((1, 8), dtype=torch.float64, device=DEV)
    out, err, coef = torch.empty_like(B), torch.empty((1, 1), dtype=torch.float64, device=DEV), torch.empty(
        (10, 1, 3), dtype=torch.float64, device=DEV)
    stats = _hip.MgpCgStats()
    jac = _hip.MgpPrecond()
    jac.kind = _hip.PRE_JACOBI
    jac.diag_inv = B.data_ptr()
    args = lambda pre, c, cs: (hd.h, ctypes.byref(st), pre, p(B), None, 1, 1e-6, 10, 11, 1e-16, 10, p(out), p(err),
                               ctypes.byref(stats), c, cs)
    assert L.mgp_pcg_solve_record(*args(ctypes.byref(jac), p(coef), 10)) == -1
    assert L.mgp_pcg_solve_record(*args(None, None, 10)) == -1
    assert L.mgp_pcg_solve_record(*args(None, p(coef), -1)) == -1
    assert L.mgp_pcg_solve_record(*args(None, p(coef), 10)) == 0
    del keep


def _kxx_op(N, D, seed, s2=0.1, name="se", ls=(0.5, 1.0)):
    from cggp import kernels
    from cggp.conjugate_gradient import KxxNoiseOperator
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    kern = cls(1.0, list(np.linspace(ls[0], ls[1], D)))
    X = torch.from_numpy(_data(N, D, seed)).to(DEV)
    return KxxNoiseOperator(kern, X, s2), kern, X


@pytest.mark.parametrize("N", [2000, 9000])
def test_recording_solve_matches_plain_solve_and_numpy_cg(N):
    from cggp import ops
    from cggp.conjugate_gradient import EyePreconditioner, _solve_device
    # well conditioned (short lengthscales, unit noise): two correct CGs on operators that differ in the last bits
    # then agree to ~1e-13 over 30 steps, where at s2 = 0.1 the recurrence amplifies the difference to ~1e-7
    op, kern, X = _kxx_op(N, 3, N, s2=1.0, ls=(0.1, 0.2))
    rhs = torch.from_numpy(np.random.default_rng(1).standard_normal((3, N))).to(DEV)
    it = 200
    sol0, st0, err0 = _solve_device(op, rhs, None, 1e-10, EyePreconditioner(), it, it + 1, 1e-16, 10)
    sol1, err1, st1, coef = ops.pcg_solve_record(op, rhs, 1e-10, it)
    assert st1.iterations == st0.iterations and torch.equal(sol0, sol1) and torch.equal(err0, err1)
    assert coef.shape == (st1.iterations, 3, 3)
    # numpy CG on the dense matrix: the first 30 steps' coefficients
    A = (ops.k_dense(op.spec, X, X, jitter=1.0)).cpu().numpy()
    b = rhs.cpu().numpy()
    c = coef.cpu().numpy()
    for col in range(3):
        x = np.zeros(N)
        r = b[col].copy()
        pdir = r.copy()
        rz = r @ r
        steps = min(30, c.shape[0])  # the better-conditioned N = 2000 system converges in about 20
        assert steps >= 15
        for k in range(steps):
            Ap = A @ pdir
            g = rz / (pdir @ Ap)
            x += g * pdir
            r -= g * Ap
            rzn = r @ r
            beta = rzn / rz
            pdir = r + beta * pdir
            ref = np.array([g, beta, 0.5 * rzn])
            assert np.all(np.abs(c[k, col] - ref) <= 1e-9 * np.abs(ref)), (col, k, c[k, col], ref)
            rz = rzn


def _logm_quad(Khat, Z):
    lam, Q = torch.linalg.eigh(Khat)
    QZ = Q.t() @ Z
    return (QZ * QZ * torch.log(lam)[:, None]).sum(dim=0)  # z_i^T log(Khat) z_i


def test_slq_logdet_against_eigh_and_slogdet():
    from cggp import models, ops
    from cggp.conjugate_gradient import ConjugateGradient
    N = 4096
    _, kern, X = _kxx_op(N, 3, 7)
    Y = torch.sin(X.sum(dim=1, keepdim=True))
    m = models.GPR((X, Y), kern, noise_variance=0.1, conjugate_gradient=ConjugateGradient(1e-14))
    Khat = ops.k_dense(kern.spec(3), X, X, jitter=0.1)
    gen = torch.Generator().manual_seed(3)
    Z = (torch.randint(0, 2, (N, 8), generator=gen) * 2 - 1).to(DEV, torch.float64)
    est = m.log_marginal_likelihood_estimate(probes=Z)
    ref = float(_logm_quad(Khat, Z).mean())
    assert abs(est.log_det - ref) <= 1e-6 * abs(ref), (est.log_det, ref)
    assert est.converged and est.iterations > 0
    # the Cholesky value and the estimate share the data fit
    exact = m.log_marginal_likelihood()
    est64 = m.log_marginal_likelihood_estimate(num_probes=64, seed=1)
    sld = float(torch.linalg.slogdet(Khat)[1])
    assert abs(est64.log_det - sld) <= 4 * est64.std_error, (est64.log_det, sld, est64.std_error)
    assert abs((est64.value + 0.5 * est64.log_det) - (exact + 0.5 * sld)) <= 1e-8 * abs(exact)


@pytest.mark.parametrize("name", ["se", "matern32"])
def test_exact_probes_give_the_cholesky_value_and_gradient(name):
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    N = 512
    _, kern, X = _kxx_op(N, 3, 11, name=name)
    Y = torch.cos(2 * X[:, :1]) + 0.1 * torch.from_numpy(np.random.default_rng(0).standard_normal((N, 1))).to(DEV)
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    k0 = cls(1.3, [0.6, 0.8, 1.1])
    chol = training.TrainableGPR(k0, 0.15, X, Y)
    est = training.TrainableGPR(k0, 0.15, X, Y, num_probes=N, conjugate_gradient=ConjugateGradient(1e-20))
    est.probes = math.sqrt(N) * torch.eye(N, dtype=torch.float64, device=DEV)  # E[z z^T] = I exactly
    l0 = chol.log_marginal_likelihood()
    l1 = est.log_marginal_likelihood()
    frozen = est.frozen_model()
    parts = frozen.log_marginal_likelihood_estimate(probes=est.probes)
    sld = float(torch.linalg.slogdet(_khat(frozen))[1])
    assert abs(parts.log_det - sld) <= 1e-8 * abs(sld)
    assert abs(l1.item() - l0.item()) <= 1e-8 * abs(l0.item())
    g0 = torch.autograd.grad(l0, chol.parameters())
    g1 = torch.autograd.grad(l1, est.parameters())
    for a, b in zip(g0, g1):
        assert torch.allclose(b, a, rtol=1e-7, atol=1e-7 * float(a.abs().max())), (a, b)


def _khat(model):
    from cggp import ops
    X = model.data[0]
    return ops.k_dense(model._spec(), X, X, jitter=model.likelihood.variance)


def test_adam_training_on_the_estimate_tracks_cholesky_training():
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    N, D = 8192, 3
    rng = np.random.default_rng(21)
    Xn = rng.uniform(-2, 2, (N, D))
    Yn = np.sin(1.5 * Xn[:, :1]) * np.cos(Xn[:, 1:2]) + 0.3 * Xn[:, 2:3] + np.sqrt(0.1) * rng.standard_normal((N, 1))
    X, Y = torch.from_numpy(Xn).to(DEV), torch.from_numpy(Yn).to(DEV)
    k0 = kernels.SquaredExponential(0.3, [3.0, 3.0, 3.0])  # poor start: too smooth, too small
    exact = lambda m: _exact_lml(m, X, Y)
    mc = training.TrainableGPR(k0, 1.0, X, Y)
    me = training.TrainableGPR(k0, 1.0, X, Y, num_probes=15, conjugate_gradient=ConjugateGradient(1e-10))
    start = exact(me)
    training.train_using_adam_and_update((X, Y), mc, 40, N, 0.05)
    training.train_using_adam_and_update((X, Y), me, 40, N, 0.05)
    lc, le = exact(mc), exact(me)
    assert le > start
    assert abs(le - lc) <= 0.01 * abs(lc), (start, lc, le)


def _exact_lml(m, X, Y):
    from cggp import models
    g = models.GPR((X, Y), m.kernel.frozen(), noise_variance=m.likelihood_variance.value, solver="cholesky")
    return g.log_marginal_likelihood()


def test_lbfgs_runs_on_the_estimate():
    from cggp import kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    X = torch.from_numpy(_data(1000, 2, 4)).to(DEV)
    Y = torch.sin(X[:, :1])
    m = training.TrainableGPR(kernels.Matern52(1.0, [1.0, 1.0]), 0.2, X, Y, num_probes=4,
                              conjugate_gradient=ConjugateGradient(1e-10))
    training.train_vanilla_using_lbfgs((X, Y), m, None, 3)
    assert np.isfinite(float(m.training_loss()))
    assert m.frozen_model().solver == "cg"


def test_estimate_and_gradient_at_2_17_rows_without_an_n_by_n_matrix():
    from cggp import _hip, kernels, training
    from cggp.conjugate_gradient import ConjugateGradient
    N, D = 1 << 17, 8
    rng = np.random.default_rng(0)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)  # what earlier tests of the process still hold
    torch.cuda.reset_peak_memory_stats(DEV)
    X = torch.from_numpy(rng.standard_normal((N, D))).to(DEV)
    Y = torch.sin(X[:, :1]) + 0.3 * torch.from_numpy(rng.standard_normal((N, 1))).to(DEV)
    idx = DEV.index or 0
    shared = _hip._handles.get(idx)
    _hip._handles[idx] = _hip.Handle(idx)  # a fresh handle: its workspace is this evaluation's alone
    try:
        m = training.TrainableGPR(kernels.SquaredExponential(1.0, [2.0] * D), 0.1, X, Y, num_probes=15,
                                  conjugate_gradient=ConjugateGradient(1e-8))
        loss = m.training_loss()
        loss.backward()
        torch.cuda.synchronize()
        hd = _hip.get_handle(DEV)
        ws = hd.lib.mgp_workspace_bytes(hd.h)
    finally:
        if shared is None:
            del _hip._handles[idx]
        else:
            _hip._handles[idx] = shared
    assert np.isfinite(loss.item())
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    peak = torch.cuda.max_memory_allocated(DEV) - base
    assert peak + ws < 1.5 * 2**30, (peak, ws)
