"""The pathwise form of the CDGP data term on the MI355X: `TrainableCGGP(data_term="pathwise")` and
`CGGP(data_term="pathwise")` against tests/cdgp_pathwise_reference.py (held to the restated reference samples and to the
batch form's expectation by tests/test_cdgp_pathwise_host.py), its seams, the panel backward beyond the fused kernel's
range, and the L-BFGS and Adam flows on it.

Bars: those of tests/test_gpu_cdgp_full.py for the same comparison, with its problems and CG settings (threshold
1e-15, at most 4 M steps, min_float 1e-30): 1e-8 on the loss, 1e-7 on [variance, lengthscales, noise] and on Z, each
relative to the group's largest entry.

Routes, as built: the prior draw is one `mgp_rff_sample` on B + M rows; its backward one `mgp_rff_sample_vjp` call on
all rows for dtheta (a lane per basis, the rows streamed in chunks) and one on Z for dZ; D = 33 or S = 9 walk feature
panels of `training.PANEL_BYTES`; the correction goes through `_KnmTimes` with S columns."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cdgp_pathwise_reference as pw
from test_gpu_cdgp_full import DEV, compare, make as make_full
from test_gpu_cdgp_matrix_free import T, probes_of, rel

pytestmark = pytest.mark.gpu
L_BASES = 96


def make(kind, D, M, N, matrix_free, S=5, L=L_BASES, **kw):
    return make_full(kind, D, M, N, matrix_free, data_term="pathwise", num_bases=L, num_samples=S, **kw)


def draw_of(m, seed):
    return tuple(t.to(DEV) for t in m.draw_pathwise(seed))


def loss_and_grads(m, data, probes, draw):
    """(loss, d[variance, lengthscales, noise] in the raw parameters, dZ or None)"""
    for p in m.parameters():
        p.grad = None
    loss = m.training_loss(data, probes=probes, pathwise=draw)
    loss.backward()
    ps = m.parameters()
    hyper = torch.cat([p.grad.reshape(-1) for p in ps[:3]]).numpy()
    return float(loss.detach()), hyper, (ps[3].grad.detach().cpu().numpy() if m.trainable_inducing else None)


@functools.lru_cache(maxsize=None)
def reference(kind, D, M, N, P, probe_seed, S=5, L=L_BASES, draw_seed=7, epsilon="matheron"):
    """the CPU reference at the model's starting point, in the model's raw (softplus) parameters; once per case"""
    m, (x, y) = make(kind, D, M, N, False, S=S, L=L)
    raws = [p.detach().clone().requires_grad_(True) for p in m.parameters()[:3]]
    Z = m.Z.detach().cpu().clone().requires_grad_(True)
    variance, ls, s2 = F.softplus(raws[0])[0], F.softplus(raws[1]), F.softplus(raws[2])[0]
    loss = -pw.elbo(kind, variance, ls, s2, Z, x.cpu(), y.cpu(), m.pseudo_u.cpu(), m.cluster_counts.cpu(),
                    probes_of(M, P, probe_seed).cpu(), m.draw_pathwise(draw_seed), epsilon=epsilon,
                    num_data=m.num_data)
    grads = torch.autograd.grad(loss, raws + [Z])
    return float(loss.detach()), torch.cat([g.reshape(-1) for g in grads[:3]]).numpy(), grads[3].numpy()


# ---------------------------------------------------------------- 1. loss and gradient against the reference
VARIANTS = {"plain": {}, "fused_solves": dict(fused_solves=True), "trainable_inducing": dict(trainable_inducing=True)}


@pytest.mark.parametrize("matrix_free", [False, True], ids=["dense", "matrix_free"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_loss_and_gradient_against_the_reference(kind, variant, matrix_free):
    D, M, N = 4, 200, 777
    m, data = make(kind, D, M, N, matrix_free, **VARIANTS[variant])
    assert m.data_term == "pathwise" and len(m.parameters()) == (4 if variant == "trainable_inducing" else 3)
    got = loss_and_grads(m, data, probes_of(M, 5, 11), draw_of(m, 7))
    compare(f"{kind} {variant} {'matrix-free' if matrix_free else 'dense'}", got, reference(kind, D, M, N, 5, 11), D)


def test_the_reference_convention_of_epsilon():
    kind, D, M, N = "matern32", 4, 200, 777
    m, data = make(kind, D, M, N, True, trainable_inducing=True, epsilon="reference")
    got = loss_and_grads(m, data, probes_of(M, 5, 11), draw_of(m, 7))
    compare("epsilon=reference", got, reference(kind, D, M, N, 5, 11, epsilon="reference"), D)


def test_wide_solves_and_a_preconditioned_cg_change_nothing():
    from cggp.conjugate_gradient import ConjugateGradient, PivotedCholeskyPreconditioner
    kind, D, M, N = "se", 4, 200, 777
    want = reference(kind, D, M, N, 5, 11)
    pr = probes_of(M, 5, 11)
    m, data = make(kind, D, M, N, True, wide_solves=True, trainable_inducing=True)
    compare("wide_solves=True", loss_and_grads(m, data, pr, draw_of(m, 7)), want, D)
    pre = PivotedCholeskyPreconditioner(rank=48)
    cg = ConjugateGradient(1e-15, preconditioner=pre, max_iterations=4 * M, min_float=1e-30)
    m, data = make(kind, D, M, N, True, cg=cg, trainable_inducing=True)
    compare("pivoted Cholesky, rank 48", loss_and_grads(m, data, pr, draw_of(m, 7)), want, D)
    assert pre.rank_ == 48  # the solves went through it


# ---------------------------------------------------------------- 2. seams
# (N, M, S): one row; one past the sweep's 4096-row chunk (and several streamed chunks of the VJP); one past the
# 256-column block of the pair kernel (dZ of the VJP: 257 owned rows); one sample and eight, the kernel's two ends
SEAMS = [(1, 200, 5), (4097, 100, 5), (777, 257, 5), (777, 200, 1), (777, 200, 8)]


@pytest.mark.parametrize("matrix_free", [False, True], ids=["dense", "matrix_free"])
@pytest.mark.parametrize("N,M,S", SEAMS)
def test_seams(N, M, S, matrix_free):
    kind, D = "matern32", 4
    m, data = make(kind, D, M, N, matrix_free, S=S, trainable_inducing=True)
    got = loss_and_grads(m, data, probes_of(M, 5, 13), draw_of(m, 7))
    compare(f"N={N} M={M} S={S} {'matrix-free' if matrix_free else 'dense'}", got,
            reference(kind, D, M, N, 5, 13, S=S), D)


@pytest.mark.parametrize("matrix_free", [False, True], ids=["dense", "matrix_free"])
def test_a_batch_without_rows_gives_minus_kl(matrix_free):
    kind, D, M = "matern32", 4, 200
    m, (x, y) = make(kind, D, M, 0, matrix_free, trainable_inducing=True)
    assert x.shape == (0, D) and y.shape == (0, 1)
    pr = probes_of(M, 5, 14)
    got = loss_and_grads(m, (x, y), pr, draw_of(m, 7))
    compare(f"no rows {'matrix-free' if matrix_free else 'dense'}", got, reference(kind, D, M, 0, 5, 14), D)
    frozen = m.frozen_model()
    kl = frozen.prior_kl(probes=pr)
    e = frozen.elbo((x, y), probes=pr)
    assert rel(e, -kl) <= 1e-12 and rel(-got[0], -kl) <= 1e-8
    assert m.pathwise_seed == 0 and frozen.pathwise_seed == 1  # an injected draw leaves the seed; a drawn one advances


# ---------------------------------------------------------------- 3. beyond the fused kernel's range
@pytest.mark.parametrize("panel_rows", [None, 300])
@pytest.mark.parametrize("D,S", [(33, 5), (4, 9)])
def test_the_panel_backward_at_33_dimensions_and_9_samples(monkeypatch, D, S, panel_rows):
    """theta alone at D = 33 (Z trainable at S = 9); one feature panel (the default 256 MiB holds all rows), and panels
    of 300 rows added in order"""
    from cggp import training
    kind, M, N = "matern32", 200, 777
    if panel_rows:
        monkeypatch.setattr(training, "PANEL_BYTES", 16 * L_BASES * panel_rows)
    m, data = make(kind, D, M, N, True, S=S, trainable_inducing=D <= 32)
    got = loss_and_grads(m, data, probes_of(M, 5, 15), draw_of(m, 7))
    want = reference(kind, D, M, N, 5, 15, S=S)
    compare(f"D={D} S={S} panels of {panel_rows or 'all'} rows", got, want if D <= 32 else want[:2] + (None,), D)
    if D > 32:
        with pytest.raises(ValueError, match="D <= 32"):
            make(kind, D, M, N, True, trainable_inducing=True)


# ---------------------------------------------------------------- 4. the samples and the frozen model
@pytest.mark.parametrize("epsilon", ["matheron", "reference"])
def test_reference_samples_are_pathwise_cluster_gp_samples(epsilon):
    from cggp import models
    kind, D, M, N = "se", 4, 200, 777
    m, (x, y) = make(kind, D, M, N, False)
    E, W, xi = m.draw_pathwise(3)
    frozen = m.frozen_model()
    gp = models.PathwiseClusterGP(frozen.kernel, frozen.likelihood.variance, m.Z, pseudo_u=m.pseudo_u,
                                  cluster_counts=m.cluster_counts, epsilon=epsilon)
    ls = torch.tensor(frozen.kernel.lengthscales, dtype=torch.float64)
    got = gp.pathwise_samples(x, L_BASES, 5, theta=E / ls[None, :], weights=W, xi=xi)[..., 0].cpu()
    want = pw.samples(kind, torch.tensor(frozen.kernel.variance, dtype=torch.float64), ls,
                      torch.tensor(frozen.likelihood.variance, dtype=torch.float64), m.Z.cpu(), x.cpu(),
                      m.pseudo_u.cpu(), m.cluster_counts.cpu(), (E, W, xi), epsilon=epsilon)
    assert got.shape == want.shape == (5, N)
    assert float((got - want).abs().max()) <= 1e-8 * float(want.abs().max())


@pytest.mark.parametrize("matrix_free", [False, True], ids=["dense", "matrix_free"])
def test_two_evaluations_are_bit_identical_and_the_frozen_model_agrees(matrix_free):
    m, data = make("matern32", 4, 200, 4097, matrix_free, trainable_inducing=True)
    pr, draw = probes_of(200, 5, 17), draw_of(m, 7)
    a, b = loss_and_grads(m, data, pr, draw), loss_and_grads(m, data, pr, draw)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    frozen = m.frozen_model()
    assert frozen.data_term == "pathwise"
    e = frozen.elbo(data, probes=pr, pathwise=draw)
    assert e == frozen.elbo(data, probes=pr, pathwise=draw) and rel(e, -a[0]) <= 1e-8
    # drawn, not injected: the seed advances and the draw changes the value
    e0, e1 = frozen.elbo(data, probes=pr), frozen.elbo(data, probes=pr)
    assert frozen.pathwise_seed == 2 and e0 != e1


# ---------------------------------------------------------------- 5. the flows
def test_lbfgs_on_the_full_data_stays_in_the_domain_and_lowers_the_loss():
    """`train_using_lbfgs_and_update` on all 20 000 rows with the default 5 probes and 5 samples and a trainable Z: the
    draw is held for the run, every evaluation is finite (the trace form left the domain here with 5 probes) and the
    loss at the held draw goes down."""
    from cggp.training import train_using_lbfgs_and_update
    kind, D, M, N = "matern32", 4, 200, 20000
    m, data = make(kind, D, M, N, True, trainable_inducing=True, cg=None)
    from cggp.models import rademacher
    pr = rademacher((M, 5), torch.float64, DEV, 0)  # the probes `train_using_lbfgs_and_update` fixes (probe_seed=0)
    draw = draw_of(m, 0)  # and the draw it holds (pathwise_seed = 0)
    seen = []
    inner = m.training_loss

    def recording(d, probes=None, pathwise=None):
        assert pathwise is not None
        out = inner(d, probes=probes, pathwise=pathwise)
        seen.append(float(out.detach()))
        return out

    m.training_loss = recording
    before = float(inner(data, probes=pr, pathwise=draw).detach())
    res = train_using_lbfgs_and_update(data, m, 3)
    m.training_loss = inner
    after = float(inner(data, probes=pr, pathwise=draw).detach())
    print(f"{before:.6f} -> {after:.6f} in {res.nit} iterations, {res.nfev} evaluations; variance "
          f"{m.kernel.variance_p.value:.4f}, lengthscales {np.round(m.kernel.lengthscales_p.value, 4)}, "
          f"noise {m.noise_p.value:.4f}")
    assert m.pathwise_seed == 1 and len(seen) == res.nfev and np.all(np.isfinite(seen))
    assert rel(seen[0], before) <= 1e-12  # the held draw is the one of seed 0
    assert 1 <= res.nit <= 3 and after < before and rel(after, res.fun) <= 1e-8
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters()) and m.noise_p.value > 1e-6


def test_adam_runs_on_minibatches_with_fresh_draws():
    from cggp.training import train_using_adam_and_update
    m, data = make("se", 4, 200, 777, True, trainable_inducing=True)
    start = [p.detach().clone() for p in m.parameters()]
    losses = train_using_adam_and_update(data, m, 3, 50, 0.05)
    print(losses)
    assert len(losses) == 3 and np.all(np.isfinite(losses)) and m.probe_seed == 3 and m.pathwise_seed == 3
    for p, p0 in zip(m.parameters(), start):
        assert bool(torch.isfinite(p).all()) and float((p.detach() - p0).abs().max()) > 0.0
