"""SGPR training at any input dimension on the MI355X: `mgp_kmn_knm_vjp_anyd` (include/mgp_anyd.h) against long double
with a derived bound, the old entry point's bits at D <= 32, determinism, shard additivity, the buffer contract and the
refusals, and `training.TrainableSGPR` at D = 33 and 77 against `models.SGPR.elbo` and autograd of the dense bound.

The bound (u = 2^-53), derived as DESIGN 4.8a derives the per-pair one.  An output is a sum of n terms W_nm t_nm
(t = f, f' delta^2 or f' delta; n = N M for dvariance and the lengthscales, N for an element of dZ), scaled once.
  * W_nm is an inner product of length M (+ P) formed by the GEMM from K values that carry their own few roundings:
    |W - exact| <= (M + P + 8) u Wa_nm, Wa = sum_j |K_nj| |G2_jm| + sum_p |Y_np| |Gb_mp| the companion of W
    (tests/kvjp_reference.py), which also bounds |W|.
  * t_nm is formed with at most 3 D + 32 roundings: per dimension the scaling of a and of b and the fma of the
    squared difference (3 D), then the profile and its slope (exp2 polynomial, square root, division: < 24), the
    products W f', (W f') delta, the fma with delta and the final scale (< 8).
  * the n additions of the sum, in whatever fixed order, add at most n u of the sum of |terms|.
To first order |output - exact| <= (n + 3 D + 32 + M + P + 8) u S, S = the output's companion sum of Wa |t| (scaled).
The GEMM adds its M products in blocks, not left to right, and K's own error is amplified by the profile; both are
inside the factor 4 the bound is given as margin: BOUND = 4 (n + 3 D + 32 + M + P + 8) u S.  A case that needs more is
a finding."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from buffer_contract import guarded
from kvjp_reference import kvjp_reference
from sgpr_grad_reference import kernel_torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KERNELS = ["se", "matern12", "matern32", "matern52"]
U = 2.0 ** -53
N, M = 130, 70  # two full 64-row tiles + 2 rows, 64 + 6 columns; panel_rows = 64: three panels, the last of 2 rows
VAR = 1.4


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ls(D):
    return np.sqrt(D) * np.linspace(0.7, 1.3, D)  # unequal; r2 = O(1) at every D


@functools.lru_cache(maxsize=None)
def _case(name, D, P=1, with_gq=True, dup=False, n=N, m=M):
    """inputs and their long-double reference, computed once per shape and shared (never modified)"""
    rng = np.random.default_rng(1000 * D + 10 * P + KERNELS.index(name))
    X = rng.uniform(-1.5, 1.5, (n, D))
    Z = rng.uniform(-1.5, 1.5, (m, D))
    if dup:
        X[5] = Z[3]  # a data row equal to an inducing point: r = 0, the Matern floor
        X[n - 1] = Z[m - 1]  # and one in the ragged last tile / last panel
    Gq = rng.standard_normal((m, m)) if with_gq else None
    Y = rng.standard_normal((n, P)) if P else None
    Gb = rng.standard_normal((m, P)) if P else None
    ref = kvjp_reference(name, VAR, _ls(D), X, Z, Gq, Y, Gb)
    return X, Z, Gq, Y, Gb, ref


def _opt(a):
    return None if a is None else t(a)


def _check(got, ref, n, m, D, P, want_dz):
    dv, dl, dZ = got
    base = 3 * D + 32 + m + P + 8
    bv = 4 * (n * m + base) * U * float(ref.sv)
    bl = 4 * (n * m + base) * U * ref.sl.astype(np.float64)
    ev = abs(dv - float(ref.dv))
    el = np.abs(np.array(dl) - ref.dl.astype(np.float64))
    print(f"dvariance err/bound {ev / bv:.3g}  dl max err/bound {np.max(el / bl):.3g}")
    assert np.isfinite(dv) and np.all(np.isfinite(dl)) and len(dl) == D
    assert ev <= bv
    assert np.all(el <= bl)
    if want_dz:
        dZ = dZ.cpu().numpy()
        bz = 4 * (n + base) * U * ref.sz.astype(np.float64)
        ez = np.abs(dZ - ref.dZ.astype(np.float64))
        print(f"dZ max err/bound {np.max(ez / np.maximum(bz, 1e-300)):.3g}")
        assert dZ.shape == (m, D) and np.all(np.isfinite(dZ))
        assert np.all(ez <= bz)  # a zero companion (a column that only meets the floor) demands an exact zero
    else:
        assert dZ is None


# ---------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("panel_rows", [0, 64])
@pytest.mark.parametrize("want_dz", [True, False])
@pytest.mark.parametrize("D", [33, 48, 77, 90])
@pytest.mark.parametrize("name", KERNELS)
def test_values_against_long_double(name, D, want_dz, panel_rows):
    from cggp import ops
    X, Z, Gq, Y, Gb, ref = _case(name, D)
    spec = ops.KernelSpec(name, VAR, list(_ls(D)), D)
    got = ops.kmn_knm_vjp_anyd(spec, t(X), t(Z), t(Gq), t(Y), t(Gb), need_dZ=want_dz, panel_rows=panel_rows)
    _check(got, ref, N, M, D, 1, want_dz)


@pytest.mark.parametrize("panel_rows", [0, 64])
@pytest.mark.parametrize("name", KERNELS)
def test_values_rank_cotangent_alone(name, panel_rows):
    """Gq = None: W = Y Gb^T alone, P = 3, at D = 33"""
    from cggp import ops
    X, Z, _, Y, Gb, ref = _case(name, 33, P=3, with_gq=False)
    spec = ops.KernelSpec(name, VAR, list(_ls(33)), 33)
    got = ops.kmn_knm_vjp_anyd(spec, t(X), t(Z), None, t(Y), t(Gb), need_dZ=True, panel_rows=panel_rows)
    _check(got, ref, N, M, 33, 3, True)


@pytest.mark.parametrize("panel_rows", [0, 64])
@pytest.mark.parametrize("name", KERNELS)
def test_values_with_rows_copied_from_z(name, panel_rows):
    from cggp import ops
    X, Z, Gq, Y, Gb, ref = _case(name, 33, dup=True)
    spec = ops.KernelSpec(name, VAR, list(_ls(33)), 33)
    got = ops.kmn_knm_vjp_anyd(spec, t(X), t(Z), t(Gq), t(Y), t(Gb), need_dZ=True, panel_rows=panel_rows)
    _check(got, ref, N, M, 33, 1, True)


@pytest.mark.parametrize("name", ["matern12", "matern32", "matern52"])
def test_pair_at_the_matern_floor_adds_exactly_zero(name):
    """one data row equal to the one inducing point: the only pair sits at GPflow's floor, where the slope is 0"""
    from cggp import ops
    D = 33
    rng = np.random.default_rng(7)
    Z = rng.uniform(-1.5, 1.5, (1, D))
    spec = ops.KernelSpec(name, VAR, list(_ls(D)), D)
    dv, dl, dZ = ops.kmn_knm_vjp_anyd(spec, t(Z.copy()), t(Z), t(np.array([[0.7]])), t(np.array([[1.3]])),
                                      t(np.array([[-0.4]])), need_dZ=True)
    assert dl == [0.0] * D and float(dZ.abs().max()) == 0.0
    w = VAR * 1.4 + 1.3 * -0.4  # K (Gq + Gq^T) + y gb at K = variance
    assert abs(dv - w) <= 16 * U * (VAR * 1.4 + 1.3 * 0.4)


def test_values_with_two_column_blocks():
    """M = 260: more than the 256 columns of one workgroup of the pair kernel, and 4 + a ragged column tile"""
    from cggp import ops
    n, m, D = 70, 260, 33
    X, Z, Gq, Y, Gb, ref = _case("matern32", D, n=n, m=m)
    spec = ops.KernelSpec("matern32", VAR, list(_ls(D)), D)
    got = ops.kmn_knm_vjp_anyd(spec, t(X), t(Z), t(Gq), t(Y), t(Gb), need_dZ=True, panel_rows=0)
    _check(got, ref, n, m, D, 1, True)


# ---------------------------------------------------------------------------------------------- 2. old bits
@pytest.mark.parametrize("with_gq", [True, False])
@pytest.mark.parametrize("D", [8, 32])
@pytest.mark.parametrize("name", KERNELS)
def test_old_entry_points_bits_at_fused_dimensions(name, D, with_gq):
    from cggp import ops
    rng = np.random.default_rng(D)
    X, Z = t(rng.uniform(-1.5, 1.5, (N, D))), t(rng.uniform(-1.5, 1.5, (M, D)))
    Gq = t(rng.standard_normal((M, M))) if with_gq else None
    Y, Gb = t(rng.standard_normal((N, 2))), t(rng.standard_normal((M, 2)))
    spec = ops.KernelSpec(name, VAR, list(np.linspace(0.7, 1.3, D)), D)
    for want_dz in (True, False):
        old = ops.kmn_knm_vjp(spec, X, Z, Gq, Y, Gb, need_dZ=want_dz)
        new = ops.kmn_knm_vjp_anyd(spec, X, Z, Gq, Y, Gb, need_dZ=want_dz, panel_rows=0)
        assert old[0] == new[0] and old[1] == new[1]
        assert (old[2] is None and new[2] is None) if not want_dz else torch.equal(old[2], new[2])


# ---------------------------------------------------------------------------------------------- 3. reproducibility, shards
def test_reproducible_shards_add_up_and_empty_input():
    from cggp import ops
    D = 77
    X, Z, Gq, Y, Gb, ref = _case("matern52", D)
    Xt, Zt, Gqt, Yt, Gbt = t(X), t(Z), t(Gq), t(Y), t(Gb)
    spec = ops.KernelSpec("matern52", VAR, list(_ls(D)), D)
    a = ops.kmn_knm_vjp_anyd(spec, Xt, Zt, Gqt, Yt, Gbt, need_dZ=True)
    b = ops.kmn_knm_vjp_anyd(spec, Xt, Zt, Gqt, Yt, Gbt, need_dZ=True)
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    p = ops.kmn_knm_vjp_anyd(spec, Xt[:70], Zt, Gqt, Yt[:70], Gbt, need_dZ=True)
    q = ops.kmn_knm_vjp_anyd(spec, Xt[70:], Zt, Gqt, Yt[70:], Gbt, need_dZ=True)
    # both the one-call result and the sum of the shards lie within the bound of the long-double value; the shard sum
    # adds one more rounding per output
    _check((p[0] + q[0], list(np.add(p[1], q[1])), p[2] + q[2]), ref, N, M, D, 1, True)
    base = 3 * D + 32 + M + 1 + 8
    assert abs(p[0] + q[0] - a[0]) <= 4 * (N * M + base) * U * float(ref.sv)
    assert np.all(np.abs(np.add(p[1], q[1]) - a[1]) <= 4 * (N * M + base) * U * ref.sl.astype(np.float64))
    assert np.all((p[2] + q[2] - a[2]).abs().cpu().numpy() <= 4 * (N + base) * U * ref.sz.astype(np.float64))
    e = ops.kmn_knm_vjp_anyd(spec, Xt[:0], Zt, Gqt, Yt[:0], Gbt, need_dZ=True)
    assert e[0] == 0.0 and e[1] == [0.0] * D and e[2].shape == (M, D) and float(e[2].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- 4. buffer contract
def _raw_call(k, X, n, Z, m, Gq, Y, Gb, P, panel_rows, dZ_ptr, dls=None):
    from cggp import _hip
    hd = _hip.get_handle(DEV)
    dv = ctypes.c_double(0.0)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)() if dls is None else dls
    vp = lambda p: ctypes.c_void_p(p) if p else ctypes.c_void_p(0)
    rc = hd.lib.mgp_kmn_knm_vjp_anyd(hd.h, ctypes.byref(k), vp(X), n, vp(Z), m, vp(Gq), vp(Y), vp(Gb), P, panel_rows,
                                     ctypes.byref(dv), dls, vp(dZ_ptr))
    torch.cuda.synchronize()
    return rc, dv.value, dls


@pytest.mark.parametrize("panel_rows", [0, 64])
@pytest.mark.parametrize("offset", [0, 1])
def test_buffer_contract(offset, panel_rows):
    from cggp import _hip
    D, P = 33, 1
    X, Z, Gq, Y, Gb, ref = _case("matern32", D)
    k = _hip.make_kernel_struct("matern32", _hip.F64, D, VAR, list(_ls(D)))
    ins = {}
    for name, a in (("X", X), ("Z", Z), ("Gq", Gq), ("Y", Y), ("Gb", Gb)):
        _, g = guarded(a.shape, torch.float64, offset, DEV)
        ins[name] = g.upload(torch.from_numpy(a))
    dZ, gz = guarded((M, D), torch.float64, offset, DEV)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)(*([123.25] * _hip.MGP_MAX_D))
    rc, dv, dls = _raw_call(k, ins["X"].ptr, N, ins["Z"].ptr, M, ins["Gq"].ptr, ins["Y"].ptr, ins["Gb"].ptr, P,
                            panel_rows, gz.ptr, dls)
    assert rc == 0
    gz.check_output(name="dZ")  # [M, D] fully written, nothing beyond it touched
    for name, g in ins.items():
        g.check_input(name)
    assert all(dls[d] == 123.25 for d in range(D, _hip.MGP_MAX_D))  # entries >= D are not the call's
    _check((dv, [dls[d] for d in range(D)], dZ.clone()), ref, N, M, D, P, True)
    # dZ = NULL is accepted: nothing is written for it, the scalars are the same bits
    rc2, dv2, dls2 = _raw_call(k, ins["X"].ptr, N, ins["Z"].ptr, M, ins["Gq"].ptr, ins["Y"].ptr, ins["Gb"].ptr, P,
                               panel_rows, 0)
    assert rc2 == 0 and dv2 == dv and [dls2[d] for d in range(D)] == [dls[d] for d in range(D)]
    gz.check_output(name="dZ after the NULL call")
    for name, g in ins.items():
        g.check_input(name)


# ---------------------------------------------------------------------------------------------- 5. errors
def test_refusals():
    from cggp import _hip, ops
    D = 33
    X, Z, Gq, Y, Gb, _ = _case("se", D)
    spec = ops.KernelSpec("se", VAR, list(_ls(D)), D)
    with pytest.raises(_hip.MgpError, match="error -3.*fp64"):  # MGP_E_DTYPE
        ops.kmn_knm_vjp_anyd(spec, t(X).float(), t(Z).float(), t(Gq).float())
    spec513 = ops.KernelSpec("se", 1.0, [1.0], 513)
    with pytest.raises(ValueError, match="513"):  # the binding refuses D > MGP_MAX_D
        ops.kmn_knm_vjp_anyd(spec513, t(np.zeros((4, 513))), t(np.zeros((3, 513))), t(np.zeros((3, 3))))
    with pytest.raises(ValueError):
        ops.kmn_knm_vjp_anyd(spec, t(X), t(Z), t(Gq), panel_rows=-1)
    k = _hip.make_kernel_struct("se", _hip.F64, D, VAR, list(_ls(D)))
    Xt, Zt = t(X), t(Z)
    rc, _, _ = _raw_call(k, Xt.data_ptr(), N, Zt.data_ptr(), M, 0, 0, 0, 0, 0, 0)  # Gq = NULL with P = 0
    assert rc == -1  # MGP_E_BADARG
    rc, _, _ = _raw_call(k, Xt.data_ptr(), N, Zt.data_ptr(), M, t(Gq).data_ptr(), 0, 0, 0, -5, 0)
    assert rc == -2  # MGP_E_SHAPE: panel_rows < 0
    # the model: D > MGP_MAX_D is refused, and above D = 32 so are host tensors (at D <= 32 the constructor is as it was)
    from cggp import kernels, training
    Xs, Ys, Zs = _sgpr_problem(33)
    k513 = kernels.SquaredExponential(variance=1.0, lengthscales=[1.0] * 513)
    with pytest.raises(ValueError, match="D <= 512"):
        training.TrainableSGPR(k513, 0.1, t(np.zeros((5, 513))), t(np.zeros((5, 1))), t(np.zeros((3, 513))))
    with pytest.raises(ValueError, match="on the GPU"):
        training.TrainableSGPR(_kernel("se", 33), 0.3, torch.from_numpy(Xs), t(Ys), t(Zs))


# ---------------------------------------------------------------------------------------------- 6., 7. the model
def _kernel(name, D):
    from cggp import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name]
    return cls(variance=1.2, lengthscales=list(np.sqrt(D) * np.linspace(0.8, 1.2, D)))


@functools.lru_cache(maxsize=None)
def _sgpr_problem(D, n=200, m=20):
    rng = np.random.default_rng(D)
    X = rng.uniform(-2.0, 2.0, (n, D))
    Y = np.sin(1.5 * X[:, :1]) * np.cos(X[:, 1:2]) + 0.1 * rng.standard_normal((n, 1))
    Z = X[rng.choice(n, m, replace=False)] + 0.01 * rng.standard_normal((m, D))
    return X, Y, Z


def _dense_bound(name, variance, ls, s2, X, Y, Z, jitter):
    """the collapsed bound restated densely on the CPU: `training.sgpr_bound` over torch-built K_mm, K_mn K_nm, K_mn y"""
    from cggp import training
    K = kernel_torch(name, variance, ls, X, Z)
    Kmm = kernel_torch(name, variance, ls, Z, Z) + jitter * torch.eye(Z.shape[0], dtype=torch.float64)
    return training.sgpr_bound(Kmm, K.t() @ K, K.t() @ Y, (Y * Y).sum(), s2, variance, float(X.shape[0]))


def _loss_and_grads(m):
    for p in m.parameters():
        p.grad = None
    loss = m.training_loss()
    loss.backward()
    return float(loss.detach()), [p.grad.detach().cpu().clone() for p in m.parameters()]


@pytest.mark.parametrize("tip", [True, False])
@pytest.mark.parametrize("name", ["se", "matern32"])
@pytest.mark.parametrize("D", [33, 77])
def test_trainable_sgpr_above_32_dimensions(D, name, tip):
    from cggp import models, training
    X, Y, Z = _sgpr_problem(D)
    make = lambda **kw: training.TrainableSGPR(_kernel(name, D), 0.3, t(X), t(Y), t(Z), trainable_inducing=tip, **kw)
    m = make()
    loss, got = _loss_and_grads(m)
    ref = -models.SGPR((t(X), t(Y)), _kernel(name, D), t(Z), 0.3, jitter=1e-6).elbo()
    assert abs(loss - float(ref)) <= 1e-10 * abs(float(ref))
    # the gradient against autograd through the dense bound on the CPU, per parameter block
    cpu = lambda a: torch.tensor(a, dtype=torch.float64)
    raws = [p.detach().cpu().clone().requires_grad_() for p in m.parameters()]
    f = torch.nn.functional.softplus
    Zr = raws[3] if tip else cpu(Z)
    val = -_dense_bound(name, f(raws[0])[0], f(raws[1]), f(raws[2])[0], cpu(X), cpu(Y), Zr, 1e-6)
    want = torch.autograd.grad(val, raws)
    assert len(got) == len(want) == (4 if tip else 3)
    for g, w in zip(got, want):
        rel = float((g - w).abs().max()) / float(w.abs().max())
        print(f"block {tuple(w.shape)} rel err {rel:.3g}")
        assert rel <= 1e-8
    # 7. a single-rank identity all-reduce changes nothing, bit for bit
    loss_ar, got_ar = _loss_and_grads(make(allreduce=lambda buf: None))
    assert loss_ar == loss and all(torch.equal(a, b) for a, b in zip(got_ar, got))
    # training runs as it stands: three Adam steps and two L-BFGS iterations lower the loss, every value finite
    start = loss
    losses = training.train_using_adam_and_update(None, m, iterations=3, batch_size=None, learning_rate=0.01)
    after_adam = float(m.training_loss())
    assert np.all(np.isfinite(losses)) and after_adam < start
    training.train_using_lbfgs_and_update((m.X, m.Y), m, 2)
    after_lbfgs = float(m.training_loss())
    assert np.isfinite(after_lbfgs) and after_lbfgs < after_adam
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    mu, var = m.frozen_model().predict_f(t(X[:16]))
    assert mu.shape[0] == 16 and bool(torch.isfinite(mu).all()) and bool(torch.isfinite(var).all())
