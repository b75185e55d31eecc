"""SGPR gradient on the host: the split of `training.TrainableSGPR`'s backward into [M, M] adjoints
(`training.sgpr_bound_adjoints`), the Kmm block and the N-sized VJP of (Q, b) -- the last in long double
(tests/sgpr_grad_reference.py) -- reproduces torch autograd of the explicit-K bound; and the Adam loop's full-data
branch for models that hold their data."""

import numpy as np
import pytest
import torch

from cggp import training
from sgpr_grad_reference import kernel_torch, kmn_knm_vjp_reference, sgpr_elbo_explicit

KERNELS = ["se", "matern12", "matern32", "matern52"]


def _problem(N=300, M=12, D=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, D))
    Y = np.sin(2.0 * X[:, :1]) + 0.1 * rng.standard_normal((N, 1))
    g = np.linspace(-1.8, 1.8, 4)
    Z = np.stack(np.meshgrid(g, np.linspace(-1.5, 1.5, 3)), axis=-1).reshape(-1, 2)[:M]
    Z = Z + 0.05 * rng.standard_normal(Z.shape)
    return X, Y, Z


@pytest.mark.parametrize("name", KERNELS)
def test_adjoints_composed_with_long_double_vjp_match_autograd(name):
    X, Y, Z = _problem()
    var0, ls0, s20, jitter = 1.3, np.array([0.9, 1.2]), 0.2, 1e-6
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    v, ls, s2, Zt = (t(var0).requires_grad_(), t(ls0).requires_grad_(), t(s20).requires_grad_(),
                     t(Z).requires_grad_())
    Xt, Yt = t(X), t(Y)
    ref = sgpr_elbo_explicit(name, v, ls, s2, Xt, Yt, Zt, jitter)
    gv, gl, gs, gZ = torch.autograd.grad(ref, [v, ls, s2, Zt])

    # step 1: [M, M] adjoints of the bound written in (Kmm_j, Q, b, s2, variance)
    with torch.no_grad():
        Knm = kernel_torch(name, t(var0), t(ls0), Xt, t(Z))
        Kmm_j = kernel_torch(name, t(var0), t(ls0), t(Z), t(Z)) + jitter * torch.eye(Z.shape[0], dtype=torch.float64)
        Q, b, yy = Knm.t() @ Knm, Knm.t() @ Yt, float((Yt * Yt).sum())
    val, Gq, Gb, GK, ds2, dvar = training.sgpr_bound_adjoints(Kmm_j, Q, b, yy, t(s20), t(var0), X.shape[0])
    assert abs(val - float(ref)) <= 1e-11 * abs(float(ref))
    # step 2: the Kmm block -- theta by the VJP of the explicit block, Z by training.kmm_grad_z
    v2, l2 = t(var0).requires_grad_(), t(ls0).requires_grad_()
    Kmm2 = kernel_torch(name, v2, l2, t(Z), t(Z))
    kv, kl = torch.autograd.grad(Kmm2, [v2, l2], grad_outputs=GK)
    kz = training.kmm_grad_z(name, var0, list(ls0), t(Z), GK)
    # step 3: the N-sized VJP of (Q, b), long double
    nv, nl, nz, _, _, _ = kmn_knm_vjp_reference(name, var0, ls0, X, Z, Gq.numpy(), Y, Gb.numpy())

    def close(a, b, tol=1e-9):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1e-300)

    assert close(dvar + float(kv) + float(nv), gv.numpy())
    assert close(kl.numpy() + nl.astype(np.float64), gl.numpy())
    assert close(ds2, gs.numpy())
    assert close(kz.numpy() + nz.astype(np.float64), gZ.numpy())


@pytest.mark.parametrize("name", KERNELS)
def test_kmm_grad_z_row_chunks(name):
    """`max_elems = 7 M D` makes kmm_grad_z walk its M = 30 rows in chunks of 7: five, the last of 2.  Against the
    default (one chunk) at 1e-14 relative, and against autograd through a direct-difference kernel matrix written here,
    L = sum(G * k(Z, Z)), at 1e-12 relative."""
    M, D = 30, 3
    rng = np.random.default_rng(11)
    Z = torch.tensor(rng.uniform(-1.5, 1.5, (M, D)))
    G = torch.tensor(rng.standard_normal((M, M)))
    var, ls = 1.3, [0.9, 1.2, 0.7]
    chunked = training.kmm_grad_z(name, var, ls, Z, G, max_elems=7 * M * D)
    assert 7 * M * D // (M * D) == 7 and -(-M // 7) == 5 and M % 7 == 2
    whole = training.kmm_grad_z(name, var, ls, Z, G)
    scale = float(whole.abs().max())
    assert float((chunked - whole).abs().max()) <= 1e-14 * scale

    Zt = Z.clone().requires_grad_()
    diff = (Zt[:, None, :] - Zt[None, :, :]) / torch.tensor(ls, dtype=torch.float64)
    r2 = (diff * diff).sum(dim=2)
    if name == "se":
        K = var * torch.exp(-0.5 * r2)
    else:
        r = torch.sqrt(torch.clamp(r2, min=1e-36))  # GPflow's floor: no gradient through the diagonal's r = 0
        c = {"matern12": 1.0, "matern32": 3.0 ** 0.5, "matern52": 5.0 ** 0.5}[name]
        poly = {"matern12": 1.0, "matern32": 1.0 + c * r, "matern52": 1.0 + c * r + 5.0 / 3.0 * r * r}[name]
        K = var * poly * torch.exp(-c * r)
    (gz,) = torch.autograd.grad((G * K).sum(), [Zt])
    assert float((chunked - gz).abs().max()) <= 1e-12 * float(gz.abs().max())


def test_kmm_grad_z_is_zero_on_duplicate_inducing_points_for_matern12():
    Z = torch.tensor([[0.1, 0.2], [0.1, 0.2], [1.0, -0.5]], dtype=torch.float64)
    G = torch.ones(3, 3, dtype=torch.float64)
    out = training.kmm_grad_z("matern12", 1.0, [1.0, 1.0], Z, G)
    assert torch.isfinite(out).all()


def test_adam_loop_takes_full_data_steps_for_internal_data_models():
    class Stub:
        internal_data = True
        num_probes = None

        def __init__(self):
            self.w = torch.tensor([2.0], dtype=torch.float64, requires_grad=True)
            self.calls = []

        def parameters(self):
            return [self.w]

        def training_loss(self, *args, **kwargs):
            self.calls.append((args, kwargs))
            return (self.w ** 2).sum()

    m = Stub()
    losses = training.train_using_adam_and_update(None, m, iterations=5, batch_size=7, learning_rate=0.1)
    assert len(losses) == 5 and losses[-1] < losses[0]
    assert m.calls == [((), {})] * 5


def test_trainable_sgpr_rejects_what_it_cannot_run():
    from cggp import kernels
    k = kernels.SquaredExponential(variance=1.0, lengthscales=[1.0, 1.0])
    X, Y, Z = (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, 1, dtype=torch.float64),
               torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        training.TrainableSGPR(k, 0.1, X.float(), Y.float(), Z.float())
    with pytest.raises(ValueError):
        training.TrainableSGPR(k, 0.1, X, torch.zeros(5, 2, dtype=torch.float64), Z)
    k33 = kernels.SquaredExponential(variance=1.0, lengthscales=[1.0] * 33)
    with pytest.raises(ValueError):
        training.TrainableSGPR(k33, 0.1, torch.zeros(5, 33, dtype=torch.float64), Y,
                               torch.zeros(3, 33, dtype=torch.float64))
