"""Whole-test-set prediction of the sparse models on the GPU: `SGPR.predict_f_batched` / `predict_y` /
`variance_matrix`, the `fused_variance` option of `CGGP.predict_f_batched(shared_inverse=True)` and the `batched` switch
of `rmse_nlpd`.

Tolerances.  Against the oracle: the project's north star, 1e-6 absolute on mean and variance.  Between the fused call
(`ops.knm_quadform`) and the composition (`ops.k_dense` + `ops.symm_matmul` + row sum) on the same matrix: the bound
derived in tests/quadform_reference.py, |difference| <= (2 eps_b + (M + 4) u) mag_b, once, as the issue sets it.  (Each
route is within that of the exact form, so the triangle inequality alone would grant twice as much; the tests do not
take it.  Worst observed: 0.006 of the bound.)"""

import numpy as np
import pytest
import torch

import pair_reference as pr
import quadform_reference as qr
from oracle import cluster as oc, kernels as ok, models as om

pytestmark = pytest.mark.gpu

S2 = 0.1


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def kernels_of(name, ls, variance=1.1):
    from cggp import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    return cls(variance=variance, lengthscales=list(ls)), ok.Kernel(name, variance, np.asarray(ls))


_PROBLEMS = {}


def problem(N, M, D=2, seed=3):
    """The data of tests/test_gpu_parity.py's `model_problem`, and 700 test rows."""
    if (N, M) not in _PROBLEMS:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((N, D))
        y = np.sin(X).sum(1, keepdims=True) + 0.3 * rng.standard_normal((N, 1))
        Z = X[rng.choice(N, M, replace=False)]
        _PROBLEMS[(N, M)] = (X, y, Z, X[:700] + 0.1)
    return _PROBLEMS[(N, M)]


def sgpr(X, y, Z, kern, **kw):
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import SGPR
    return SGPR((T(X), T(y)), kern, T(Z), S2, ConjugateGradient(1e-12, max_iterations=5000), jitter=1e-6, **kw)


def agreement_bound(name, variance, ls, Xs, Z, C):
    """(2 eps_b + (M + 4) u) mag_b [B] for the matrix C (numpy)."""
    pv = pr.pair_values(name, variance, ls, Xs, Z)
    eps = qr.row_eps(name, variance, ls, Xs, Z, pv, np.float64)[:, -1]
    _, mag = qr.form(pv.k, C)
    return qr.bound(eps, Z.shape[0], mag, np.float64)


# ---------------------------------------------------------------- SGPR against the oracle
@pytest.mark.parametrize("name", ["se", "matern32"])
@pytest.mark.parametrize("N,M", [(1500, 30), (4000, 300)])
def test_sgpr_predict_f_batched_against_the_oracle(N, M, name):
    X, y, Z, Xs = problem(N, M)
    ls = np.random.default_rng(0).random(2) ** 2 + 0.5
    kern, okern = kernels_of(name, ls)
    m = sgpr(X, y, Z, kern)
    mu0, var0 = om.SGPR((X, y), okern, Z, S2, jitter=1e-6).predict_f(Xs)
    xs = T(Xs)
    got = {}
    for fused in (False, True):
        for bs in (256, None):
            mu, var = m.predict_f_batched(xs, bs, fused_variance=fused)
            assert tuple(mu.shape) == (700, 1) and tuple(var.shape) == (700, 1)
            e_mu = float(np.max(np.abs(mu.cpu().numpy() - mu0)))
            e_var = float(np.max(np.abs(var.cpu().numpy() - var0)))
            print(f"SGPR {name} N={N} M={M} fused={fused} batch={bs}: |mean - oracle| {e_mu:.2e}, |var - oracle| {e_var:.2e}")
            assert e_mu < 1e-6 and e_var < 1e-6
            got[(fused, bs)] = (mu, var)
        # the chunking does not change a row's arithmetic
        assert torch.equal(got[(fused, 256)][0], got[(fused, None)][0])
        assert torch.equal(got[(fused, 256)][1], got[(fused, None)][1])
    C = m.variance_matrix()
    assert torch.equal(C, C.t())
    bound = agreement_bound(name, kern.variance, ls, Xs, Z, C.cpu().numpy())
    diff = np.abs((got[(True, None)][1] - got[(False, None)][1]).cpu().numpy()[:, 0])
    print(f"SGPR {name} N={N} M={M}: fused against composition, worst diff / bound {float(np.max(diff / bound)):.3f}")
    assert np.all(diff <= bound)
    # predict_y = predict_f + s2; "auto" is one of the two
    mf, vf = m.predict_f(xs[:64])
    my, vy = m.predict_y(xs[:64])
    assert torch.equal(my, mf) and torch.equal(vy, vf + S2)
    for fused in (False, True):  # and its whole-data-set form
        myb, vyb = m.predict_y_batched(xs, 256, fused_variance=fused)
        assert torch.equal(myb, got[(fused, 256)][0]) and torch.equal(vyb, got[(fused, 256)][1] + S2)
    va = m.predict_f_batched(xs, 256)[1]
    assert torch.equal(va, got[(True, 256)][1]) or torch.equal(va, got[(False, 256)][1])
    with pytest.raises(ValueError):
        m.predict_f_batched(xs, 256, fused_variance="yes")


# ---------------------------------------------------------------- SGPR caches and sharding
def test_sgpr_variance_matrix_cache_follows_the_parameters():
    X, y, Z, Xs = problem(1500, 30)
    xs = T(Xs[:300])
    kern, _ = kernels_of("se", [0.9, 1.2])
    m = sgpr(X, y, Z, kern)
    before = sgpr(X, y, Z, kernels_of("se", [0.9, 1.2])[0]).predict_f(xs)  # a model that never forms C
    m.variance_matrix()
    C0 = m._C
    assert C0 is not None and m.variance_matrix() is C0  # cached
    after = m.predict_f(xs)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])  # predict_f does not see the cache
    for fused in (False, True):
        m.kernel.lengthscales = [0.9, 1.2]
        m.likelihood.variance = S2
        base = m.predict_f_batched(xs, fused_variance=fused)
        m.kernel.lengthscales = [0.7, 1.0]
        moved = m.predict_f_batched(xs, fused_variance=fused)
        assert m._C is not C0 and not torch.equal(moved[1], base[1])
        fresh = sgpr(X, y, Z, kernels_of("se", [0.7, 1.0])[0]).predict_f_batched(xs, fused_variance=fused)
        assert torch.equal(moved[0], fresh[0]) and torch.equal(moved[1], fresh[1])  # not stale
        C1 = m._C
        m.likelihood.variance = 0.2
        moved = m.predict_f_batched(xs, fused_variance=fused)
        assert m._C is not C1
        from cggp.conjugate_gradient import ConjugateGradient
        from cggp.models import SGPR
        fresh = SGPR((T(X), T(y)), kernels_of("se", [0.7, 1.0])[0], T(Z), 0.2,
                     ConjugateGradient(1e-12, max_iterations=5000), jitter=1e-6).predict_f_batched(xs, fused_variance=fused)
        assert torch.equal(moved[0], fresh[0]) and torch.equal(moved[1], fresh[1])
        C0 = m._C
    m.invalidate()
    assert m._C is None


def test_sgpr_row_shards_through_the_allreduce_hook():
    """Two identical shards without a second process: the stand-in all-reduce doubles its buffer.  The model then is
    the model of the duplicated data."""
    X, y, Z, Xs = problem(1500, 30)
    ls = [0.4, 0.4]
    kern, okern = kernels_of("se", ls)

    class TwoIdenticalShards:
        world_size = 2
        calls = 0

        def __call__(self, t):
            TwoIdenticalShards.calls += 1
            t.mul_(2.0)

    # preconditioner=None and S formed up front: every N-sized quantity of this path (K_mn K_nm, K_mn y, the row count)
    # goes through the hook as a tensor, none through the collective operator of a CG step
    m = sgpr(X, y, Z, kern, allreduce=TwoIdenticalShards(), preconditioner=None)
    assert m.num_data == 3000
    m.dense_S()
    ref = om.SGPR((np.concatenate([X, X]), np.concatenate([y, y])), okern, Z, S2, jitter=1e-6)
    mu0, var0 = ref.predict_f(Xs)
    for fused in (False, True):
        mu, var = m.predict_f_batched(T(Xs), 256, fused_variance=fused)
        e_mu = float(np.max(np.abs(mu.cpu().numpy() - mu0)))
        e_var = float(np.max(np.abs(var.cpu().numpy() - var0)))
        print(f"sharded SGPR fused={fused}: |mean - oracle| {e_mu:.2e}, |var - oracle| {e_var:.2e}")
        assert e_mu < 1e-6 and e_var < 1e-6
    assert TwoIdenticalShards.calls >= 3
    # one shard alone is a different model
    _, var1 = om.SGPR((X, y), okern, Z, S2, jitter=1e-6).predict_f(Xs)
    assert np.max(np.abs(var1 - var0)) > 1e-4


# ---------------------------------------------------------------- CGGP
def cggp_model(**kw):
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import CGGP
    X, y, Z, Xs = problem(1500, 30)
    kern, okern = kernels_of("matern32", [0.8, 1.1])
    idx = oc.nearest_centre_sqdist(Z, X)
    u, counts = oc.cluster_stats(idx, y, Z.shape[0])
    m = CGGP(kern, S2, T(Z), ConjugateGradient(1e-15, max_iterations=3000), pseudo_u=T(u), cluster_counts=T(counts), **kw)
    return m, kern, Z, Xs


def test_cggp_fused_variance_against_the_composition():
    from cggp import ops
    from cggp.conjugate_gradient import ConjugateGradient
    m, kern, Z, Xs = cggp_model(num_probes=None)
    xs = T(Xs)
    default = m.predict_f_batched(xs, 256, shared_inverse=True)
    off = m.predict_f_batched(xs, 256, shared_inverse=True, fused_variance=False)
    on = m.predict_f_batched(xs, 256, shared_inverse=True, fused_variance=True)
    # the composition, rebuilt on the same Y (the statements of the method; the solve is deterministic)
    _, KmmLambda, _ = m._system()
    cg = m.conjugate_gradient
    tight = ConjugateGradient(min(cg.error_threshold ** 2, 1e-12), cg.preconditioner, cg.max_iterations,
                              cg.max_steps_cycle, min_float=cg.min_float, check_every=cg.check_every)
    Y = tight(KmmLambda, torch.eye(Z.shape[0], dtype=torch.float64, device=dev()))
    Y = (0.5 * (Y + Y.t())).contiguous()
    spec = kern.spec(2)
    want = []
    for s in range(0, 700, 256):
        xb = xs[s:s + 256]
        Knm = ops.k_dense(spec, xb, T(Z))
        want.append((kern.K_diag(xb) - (Knm * ops.symm_matmul(Y, Knm)).sum(dim=1))[:, None])
    want = torch.cat(want, 0)
    assert torch.equal(off[1], want) and torch.equal(default[1], want)  # False: the composition's bits, as before
    assert torch.equal(off[0], default[0]) and torch.equal(on[0], default[0])
    bound = agreement_bound("matern32", kern.variance, [0.8, 1.1], Xs, Z, Y.cpu().numpy())
    diff = np.abs((on[1] - want).cpu().numpy()[:, 0])
    print(f"CGGP fused against composition: worst diff / bound {float(np.max(diff / bound)):.3f}")
    assert np.all(diff <= bound)
    auto = m.predict_f_batched(xs, 256, shared_inverse=True, fused_variance="auto")
    assert torch.equal(auto[1], on[1]) or torch.equal(auto[1], off[1])
    with pytest.raises(ValueError):
        m.predict_f_batched(xs, 256, shared_inverse=True, fused_variance=1)
    with pytest.raises(ValueError):
        m.predict_f_batched(xs, 256, fused_variance=True)  # there is no shared inverse to apply


def test_cggp_matrix_free_still_refuses_the_shared_inverse():
    m, kern, Z, Xs = cggp_model(num_probes=5, num_data=1500, matrix_free=True)
    for fused in (False, True, "auto"):
        with pytest.raises(ValueError):
            m.predict_f_batched(T(Xs), 256, shared_inverse=True, fused_variance=fused)


# ---------------------------------------------------------------- rmse_nlpd
def test_rmse_nlpd_batched_switch():
    from cggp.models import rmse_nlpd
    X, y, Z, Xs = problem(1500, 30)
    rng = np.random.default_rng(9)
    ys = np.sin(Xs).sum(1, keepdims=True) + 0.3 * rng.standard_normal((700, 1))
    data = (T(Xs), T(ys))
    m = sgpr(X, y, Z, kernels_of("se", [0.4, 0.4])[0])
    looped = rmse_nlpd(m, data, 256)
    batched = rmse_nlpd(m, data, 256, batched=True)
    print(f"rmse_nlpd looped {looped}, batched {batched}")
    assert all(abs(b - a) <= 1e-9 * abs(a) for a, b in zip(looped, batched))
    whole = rmse_nlpd(m, data, None, batched=True)
    assert all(abs(b - a) <= 1e-9 * abs(a) for a, b in zip(looped, whole))
    # the default call is the loop over predict_f, statement for statement
    sq = lpd = 0.0
    for s in range(0, 700, 256):
        xb, yb = data[0][s:s + 256], data[1][s:s + 256]
        mu, var = m.predict_f(xb)
        lpd += m.likelihood.predict_log_density(xb, mu, var, yb).sum().item()
        sq += ((yb - mu) ** 2).sum().item()
    assert looped == (np.sqrt(sq / 700), -lpd / 700) and rmse_nlpd(m, data, batch_size=256, batched=False) == looped

    class Plain:  # a model without predict_f_batched takes the loop whatever the switch
        likelihood = m.likelihood
        predict_f = m.predict_f

    assert rmse_nlpd(Plain(), data, 256, batched=True) == looped
    # CDGP: the batched path is its per-batch prediction with the shared solve
    mc, _, _, _ = cggp_model(num_probes=None)
    a, b = rmse_nlpd(mc, data, 256), rmse_nlpd(mc, data, 256, batched=True)
    assert all(abs(y_ - x_) <= 1e-9 * abs(x_) for x_, y_ in zip(a, b))
