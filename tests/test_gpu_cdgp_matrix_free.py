"""CDGP with K_mm never formed: `CGGP(matrix_free=True)` against the dense `CGGP`, `TrainableCGGP(matrix_free=True)`
against the dense `TrainableCGGP`, and the three autograd nodes against tests/cdgp_mf_reference.py (held to autograd on
the CPU by tests/test_cdgp_matrix_free_host.py).

Both sides solve to the threshold 1e-15 with a cap of 4 M steps and `min_float=1e-30`, so that neither stalls at the
default breakdown floor (0.5 |r|^2 ~ 1e-17) before it gets there: what is compared is two converged solves of the same
system, at D = 3 or 4 (the fused sweeps) and at D = 33 (the generic route)."""

import numpy as np
import pytest
import torch

import cdgp_mf_reference as ref
import switch_forms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def device_kernel(kind, variance, ls):
    from cggp import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[kind]
    return cls(variance=variance, lengthscales=[float(v) for v in ls])


def tight_cg(M, thr=1e-15):
    from cggp.conjugate_gradient import ConjugateGradient
    return ConjugateGradient(thr, max_iterations=4 * M, min_float=1e-30)


def problem(kind, D, M, N, seed=0):
    """Inputs on [-2, 2]^D, Z a subset of them (no empty cluster), pseudo_u and counts from the nearest-centre pass."""
    from cggp.optimize import nearest_centre_statistics
    rng = np.random.default_rng(seed + D)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = np.sin(X[:, :3]).sum(axis=1, keepdims=True) + 0.3 * rng.standard_normal((N, 1))
    Z = X[rng.choice(N, M, replace=False)]
    ls = rng.uniform(0.5, 0.9, D) * np.sqrt(D)
    kern = device_kernel(kind, 1.2, ls)
    _, sums, counts = nearest_centre_statistics(kern, T(Z), (T(X), T(y)))
    assert float(counts.min()) >= 1.0
    return T(X), T(y), T(Z), kern, (sums / counts)[:, None].contiguous(), counts[:, None].contiguous()


def rel(a, b):
    return abs(a - b) / abs(b)


def probes_of(M, P, seed):
    return T(2.0 * np.random.default_rng(seed).integers(0, 2, (M, P)) - 1.0)


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("kind,D", [("se", 3), ("matern32", 3), ("se", 33), ("matern32", 33)])
def test_model_parity_with_the_dense_model(kind, D):
    from cggp.models import CGGP
    M, N, s2 = 300, 1500, 0.4
    X, y, Z, kern, u, counts = problem(kind, D, M, N)
    make = lambda mf: CGGP(kern, s2, Z, tight_cg(M), num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=N,
                           matrix_free=mf)
    dense, free = make(False), make(True)
    for P in (5, 20):
        pr = probes_of(M, P, P)
        a, b = free.prior_kl(pr), dense.prior_kl(pr)
        print(f"{kind} D={D}: prior_kl P={P} {rel(a, b):.2e} (bar 1e-9)")
        assert rel(a, b) <= 1e-9
    for rows in (37, 64):
        xs = X[100:100 + rows]
        mu_d, var_d = dense.predict_f(xs)
        mu_f, var_f = free.predict_f(xs)
        dm, dv = float((mu_f - mu_d).abs().max()), float((var_f - var_d).abs().max())
        print(f"{kind} D={D}: predict_f rows={rows} mean {dm:.2e} variance {dv:.2e} (bar 1e-8)")
        assert mu_f.shape == (rows, 1) and var_f.shape == (rows, 1) and dm <= 1e-8 and dv <= 1e-8
        _, cov_f = free.predict_f(xs, full_cov=True)
        _, cov_d = dense.predict_f(xs, full_cov=True)
        assert cov_f.shape == (1, rows, rows)
        assert float((cov_f - cov_d).abs().max()) <= 1e-8
        assert float((cov_f[0].diagonal()[:, None] - var_f).abs().max()) <= 1e-8
    xs = X[:101]
    mu_b, var_b = free.predict_f_batched(xs, 37)  # batches of 37, 37 and 27 rows
    mu_f, var_f = free.predict_f(xs)
    assert float((mu_b - mu_f).abs().max()) <= 1e-8 and float((var_b - var_f).abs().max()) <= 1e-8
    pr = probes_of(M, 5, 7)
    data = (X[:64], y[:64])
    e_f, e_d = free.elbo(data, probes=pr), dense.elbo(data, probes=pr)
    print(f"{kind} D={D}: elbo {rel(e_f, e_d):.2e} (bar 1e-8)")
    assert rel(e_f, e_d) <= 1e-8
    eb_f = free.elbo_over_batches((X[:128], y[:128]), 64, shared_inverse=False, probes=pr)
    eb_d = dense.elbo_over_batches((X[:128], y[:128]), 64, shared_inverse=False, probes=pr)
    assert rel(eb_f, eb_d) <= 1e-8


def test_what_needs_an_m_by_m_array_is_refused():
    from cggp.models import CGGP, cdgp_class
    X, y, Z, kern, u, counts = problem("se", 3, 60, 300)
    kw = dict(pseudo_u=u, cluster_counts=counts, num_data=300)
    free = CGGP(kern, 0.4, Z, tight_cg(60), matrix_free=True, **kw)  # TypeError without the feature
    assert free.matrix_free and not CGGP(kern, 0.4, Z, tight_cg(60), **kw).matrix_free
    assert cdgp_class(kern, 0.4, Z, matrix_free=True, **kw).matrix_free
    with pytest.raises(ValueError, match="num_probes"):
        CGGP(kern, 0.4, Z, tight_cg(60), num_probes=None, matrix_free=True, **kw).prior_kl()
    with pytest.raises(ValueError, match="num_probes"):
        CGGP(kern, 0.4, Z, tight_cg(60), num_probes=None, matrix_free=True, **kw).elbo((X[:20], y[:20]))
    with pytest.raises(ValueError, match="shared_inverse"):
        free.predict_f_batched(X[:40], 20, shared_inverse=True)
    with pytest.raises(ValueError, match="shared_inverse"):
        free.elbo_over_batches((X[:40], y[:40]), 20)  # its default is the shared inverse
    with pytest.raises(ValueError, match="logdet_gradient"):
        free.logdet_gradient()
    # injected probes stand in for num_probes
    assert np.isfinite(CGGP(kern, 0.4, Z, tight_cg(60), num_probes=None, matrix_free=True, **kw).prior_kl(probes_of(60, 3, 1)))


def test_nothing_m_by_m_is_allocated(monkeypatch):
    from cggp import ops
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP
    M, N = 4096, 8192
    X, y, Z, kern, u, counts = problem("se", 3, M, N)
    seen = []
    for name in ("k_dense", "symm_matmul"):
        inner = getattr(ops, name)

        def wrapper(*args, _inner=inner, _name=name, **kwargs):
            out = _inner(*args, **kwargs)
            seen.append((_name, tuple(out.shape)))
            return out

        monkeypatch.setattr(ops, name, wrapper)
    free = CGGP(kern, 0.4, Z, ConjugateGradient(1e-8), num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=N,
                matrix_free=True)
    with switch_forms.switched(monkeypatch, {}) as hd:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base, ws0 = torch.cuda.memory_allocated(), hd.lib.mgp_workspace_bytes(hd.h)
        e = free.elbo((X[:32], y[:32]))
        mu, var = free.predict_f(X[:32])
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base + hd.lib.mgp_workspace_bytes(hd.h) - ws0
    assert np.isfinite(e) and bool(torch.isfinite(mu).all()) and bool((var > 0).all())
    print(f"peak above the start: {extra / 2 ** 20:.1f} MiB, one [M, M] array: {8 * M * M / 2 ** 20:.0f} MiB; {seen}")
    assert seen and all(shape != (M, M) for _, shape in seen), seen  # K_mn [M, 32] only
    assert extra < 8 * M * M


# ---------------------------------------------------------------- training
def trainable(kind, D, M, B, matrix_free, **kw):
    from cggp.training import TrainableCGGP
    X, y, Z, kern, u, counts = problem(kind, D, M, 1000, seed=3)
    m = TrainableCGGP(kern, 0.3, Z, tight_cg(M), num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=1000,
                      matrix_free=matrix_free, **kw)
    return m, (X[:B], y[:B])


def loss_and_grads(m, data, probes):
    for p in m.parameters():
        p.grad = None
    loss = m.training_loss(data, probes=probes)
    loss.backward()
    return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in m.parameters()]).numpy()


@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("kind,D", [("se", 4), ("matern32", 33)])
def test_training_loss_and_gradients_match_the_dense_model(kind, D, independent):
    M, B = 200, 50
    pr = probes_of(M, 5, 11)
    out = {}
    for mf in (False, True):
        m, data = trainable(kind, D, M, B, mf, independent_logdet_probes=independent)
        assert len(m.kernel.lengthscales_p.raw) == D  # ARD
        out[mf] = loss_and_grads(m, data, pr)
    (l_d, g_d), (l_f, g_f) = out[False], out[True]
    dist = np.max(np.abs(g_f - g_d)) / np.max(np.abs(g_d))
    print(f"{kind} D={D} independent={independent}: loss {rel(l_f, l_d):.2e} (bar 1e-8), "
          f"gradient [variance, {D} lengthscales, noise] {dist:.2e} (bar 1e-7)")
    assert g_f.shape == (D + 2,) and np.all(np.isfinite(g_f))
    assert rel(l_f, l_d) <= 1e-8 and dist <= 1e-7
    # one solve on [pseudo_u | K_mn | probes]: the same loss and gradient
    m, data = trainable(kind, D, M, B, True, independent_logdet_probes=independent, fused_solves=True)
    l_1, g_1 = loss_and_grads(m, data, pr)
    assert rel(l_1, l_d) <= 1e-8 and np.max(np.abs(g_1 - g_d)) / np.max(np.abs(g_d)) <= 1e-7


def test_training_refuses_the_exact_trace_and_freezes_matrix_free():
    m, data = trainable("se", 4, 60, 20, True)
    m.num_probes = None
    with pytest.raises(ValueError, match="num_probes"):
        m.elbo(data)
    assert m.frozen_model().matrix_free


def test_three_adam_steps_lower_the_loss():
    from cggp.training import train_using_adam_and_update
    m, data = trainable("se", 4, 200, 50, True)
    pr = probes_of(200, 5, 12)
    before = float(m.training_loss(data, probes=pr).detach())
    losses = train_using_adam_and_update(data, m, 3, 50, 0.05)
    after = float(m.training_loss(data, probes=pr).detach())
    print(f"{before:.6f} -> {after:.6f} ({losses})")
    assert len(losses) == 3 and np.all(np.isfinite(losses)) and after < before


# ---------------------------------------------------------------- the nodes against the host formulas
@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_the_nodes_send_back_what_the_host_formulas_say(kind):
    from cggp.training import _KzzLambdaLogdet, _KzzLambdaSolve, _KzzTimes
    M, D, R = 40, 3, 17
    rng = np.random.default_rng(9)
    c = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    Z, V, G = c(rng.uniform(-1.5, 1.5, (M, D))), c(rng.standard_normal((M, R))), c(rng.standard_normal((M, R)))
    lam, ls, variance = c(rng.uniform(0.3, 1.2, M)), c(rng.uniform(0.6, 1.4, D)), c(1.7)

    def close(name, got, want, bar):
        got, want = torch.as_tensor(got).detach().cpu().reshape(-1), torch.as_tensor(want).reshape(-1)
        dist = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{kind} {name}: {dist:.2e} (bar {bar:.0e})")
        assert dist <= bar, (name, dist)

    def leaves():
        return variance.clone().requires_grad_(True), ls.clone().requires_grad_(True)

    Zd, Vd, Gd = Z.to(DEV), V.to(DEV), G.to(DEV)
    v, l = leaves()
    Vl = Vd.clone().requires_grad_(True)
    out = _KzzTimes.apply(v, l, Zd, Vl, kind)
    (out * Gd).sum().backward()
    want = ref.kzz_times_backward(kind, variance, ls, Z, V, G)
    for name, g, w in zip(("times dV", "times dvariance", "times dls"), (Vl.grad, v.grad, l.grad), want):
        close(name, g, w, 1e-10)

    v, l = leaves()
    lamd, rhs = lam.to(DEV).requires_grad_(True), Vd.clone().requires_grad_(True)
    X = _KzzLambdaSolve.apply(v, l, lamd, rhs, Zd, kind, tight_cg(M, 1e-26))
    (X * Gd).sum().backward()
    want = ref.solve_backward(kind, variance, ls, lam, Z, V, G)
    for name, g, w in zip(("solve drhs", "solve dvariance", "solve dls", "solve dlam"),
                          (rhs.grad, v.grad, l.grad, lamd.grad), want):
        close(name, g, w, 1e-8)

    v, l = leaves()
    lamd = lam.to(DEV).requires_grad_(True)
    probes = probes_of(M, 5, 2)
    S = torch.linalg.solve(ref.kzz(kind, variance, ls, Z) + torch.diag(lam), probes.cpu())
    (0.7 * _KzzLambdaLogdet.apply(v, l, lamd, S.to(DEV), probes, Zd, kind, None)).backward()
    want = ref.logdet_backward(kind, variance, ls, lam, Z, S, probes.cpu(), df=0.7)
    for name, g, w in zip(("logdet dvariance", "logdet dls", "logdet dlam"), (v.grad, l.grad, lamd.grad), want):
        close(name, g, w, 1e-10)
