"""CDGP with trainable inducing inputs on the MI355X.

`mgp_kmn_knm_vjp` with Gq = NULL (the cotangent W = Y Gb^T alone) against long double, its determinism, shard
additivity, edge cases, memory and buffer contract; the three matrix-free autograd nodes with Z.requires_grad against
CPU autograd through dense formulas; `TrainableCGGP(trainable_inducing=True)`, dense and matrix-free, against
tests/cdgp_tip_reference.py (held to finite differences by tests/test_cdgp_tip_host.py) and each other; Adam and
L-BFGS.

As built (csrc/kmn_grad.hip): P <= P_FUSED = 12 takes the fused pair kernel, in passes of at most PC = 16 columns
(PC = 8 for Matern-1/2), each pass as wide as the narrowest of 2, 4, 8, PC that holds what is left; larger P takes the
W panels of the NT GEMM.  The cases below therefore hit: fused passes of width 2, 4, 8 and 16, the pass seam of the
fused form (Matern-1/2 at P = 9 = PC + 1: 8 + 2, and at P = 12: 8 + 4), both sides of P_FUSED (12 and 13), and the panel
form at PC + 1 and 2 PC + 1 of the wider passes (17, 33), at P = 16, 40 and 300."""

import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cdgp_tip_reference as tip
import switch_forms
from buffer_contract import Guarded
from sgpr_grad_reference import kmn_knm_vjp_reference
from test_gpu_cdgp_matrix_free import probes_of, rel, tight_cg, trainable

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_FUSED = 12


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def vjp_inputs(N, M, D, P, seed, same=False, dup=0):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, (M, D))
    X = Z if same else rng.uniform(-2.0, 2.0, (N, D))
    if dup:
        X[:dup] = Z[:dup]  # data rows equal to inducing points: the 1e-36 floor of the Matern slopes
    return X, Z, rng.standard_normal((X.shape[0], P)), rng.standard_normal((M, P))


def check_against_long_double(name, D, X, Z, Y, Gb, got, want_dz=True):
    ls = np.linspace(0.7, 1.3, D)
    dv, dl, dZ = got
    rv, rl, rz, sv, sl, sz = kmn_knm_vjp_reference(name, 1.4, ls, X, Z, np.zeros((Z.shape[0],) * 2), Y, Gb)
    errs = [abs(dv - float(rv)) / float(sv),
            float(np.max(np.abs(np.array(dl) - rl.astype(np.float64)) / sl.astype(np.float64)))]
    assert np.isfinite(dv) and np.all(np.isfinite(dl))
    if want_dz:
        dZ = dZ.cpu().numpy()
        assert dZ.shape == Z.shape and np.all(np.isfinite(dZ))
        errs.append(float(np.max(np.abs(dZ - rz.astype(np.float64)) / (sz.astype(np.float64) + 1e-300))))
    else:
        assert dZ is None
    print(f"{name} D={D} N={X.shape[0]} M={Z.shape[0]} P={Y.shape[1]}: " + " ".join(f"{e:.1e}" for e in errs)
          + " (bar 1e-10)")
    assert max(errs) <= 1e-10


def spec_of(name, D):
    from cggp import ops
    return ops.KernelSpec(name, 1.4, list(np.linspace(0.7, 1.3, D)), D)


# ---------------------------------------------------------------- 1. the entry point against long double
# (kernel, D, N, M, P, X is Z, rows of X copied from Z)
CASES = [("se", 5, 777, 37, 2, False, 0), ("matern32", 17, 4097, 130, 1, False, 0), ("se", 1, 65, 1, 3, False, 0),
         ("matern52", 32, 1, 37, 16, False, 0), ("matern12", 3, 300, 300, 6, True, 0),
         ("matern12", 8, 500, 70, 5, False, 70), ("matern32", 8, 500, 70, 5, False, 70),
         # PC + 1 and 2 PC + 1: a pass seam of the fused form where P <= P_FUSED, the panel form beyond
         ("matern12", 3, 777, 37, 9, False, 0), ("matern12", 3, 777, 37, 17, False, 0),
         ("se", 5, 777, 37, 17, False, 0), ("se", 5, 777, 37, 33, False, 0), ("matern32", 32, 300, 37, 9, False, 0),
         # either side of P_FUSED (a 16-wide pass; 8 + 4 for Matern-1/2), and well above it
         ("matern52", 5, 777, 130, 12, False, 0), ("matern12", 17, 777, 130, 12, False, 0),
         ("matern52", 5, 777, 130, 13, False, 0), ("se", 5, 777, 130, 300, False, 0),
         ("matern32", 3, 300, 300, 300, True, 0), ("matern12", 8, 500, 70, 40, False, 70)]


@pytest.mark.parametrize("name,D,N,M,P,same,dup", CASES)
def test_rank_p_cotangent_against_long_double(name, D, N, M, P, same, dup):
    from cggp import ops
    X, Z, Y, Gb = vjp_inputs(N, M, D, P, N + 7 * M + D + P, same, dup)
    Zt = T(Z)
    Xt = Zt if same else T(X)
    got = ops.kmn_knm_vjp(spec_of(name, D), Xt, Zt, None, T(Y), T(Gb), need_dZ=True)
    check_against_long_double(name, D, X, Z, Y, Gb, got)
    # without dZ: the same hyper-parameter gradients
    got = ops.kmn_knm_vjp(spec_of(name, D), Xt, Zt, None, T(Y), T(Gb))
    check_against_long_double(name, D, X, Z, Y, Gb, got, want_dz=False)


# ---------------------------------------------------------------- 2. determinism and edge cases
@pytest.mark.parametrize("P", [3, 300])
def test_two_calls_are_bit_identical_and_shards_add_up(P):
    from cggp import ops
    N, M, D, s = 2001, 130, 5, 777
    X, Z, Y, Gb = vjp_inputs(N, M, D, P, 3)
    spec = spec_of("matern32", D)
    Xt, Zt, Yt, Gbt = T(X), T(Z), T(Y), T(Gb)
    a = ops.kmn_knm_vjp(spec, Xt, Zt, None, Yt, Gbt, need_dZ=True)
    b = ops.kmn_knm_vjp(spec, Xt, Zt, None, Yt, Gbt, need_dZ=True)
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    p = ops.kmn_knm_vjp(spec, Xt[:s], Zt, None, Yt[:s], Gbt, need_dZ=True)
    q = ops.kmn_knm_vjp(spec, Xt[s:], Zt, None, Yt[s:], Gbt, need_dZ=True)
    ls = np.linspace(0.7, 1.3, D)
    _, _, _, sv, sl, sz = kmn_knm_vjp_reference("matern32", 1.4, ls, X, Z, np.zeros((M, M)), Y, Gb)
    assert abs(p[0] + q[0] - a[0]) <= 1e-12 * float(sv)
    assert np.all(np.abs(np.add(p[1], q[1]) - a[1]) <= 1e-12 * sl.astype(np.float64))
    assert np.all((p[2] + q[2] - a[2]).abs().cpu().numpy() <= 1e-12 * sz.astype(np.float64))


def test_empty_input_and_refusals():
    from cggp import _hip, ops
    X, Z, Y, Gb = (T(a) for a in vjp_inputs(50, 37, 5, 2, 4))
    spec = spec_of("se", 5)
    e = ops.kmn_knm_vjp(spec, X[:0], Z, None, Y[:0], Gb, need_dZ=True)
    assert e[0] == 0.0 and e[1] == [0.0] * 5 and e[2].shape == (37, 5) and float(e[2].abs().max()) == 0.0
    with pytest.raises(ValueError, match="needs Y and Gb"):
        ops.kmn_knm_vjp(spec, X, Z, None)
    with pytest.raises(ValueError, match="needs Y and Gb"):
        ops.kmn_knm_vjp(spec, X, Z, None, None, None, True)
    with pytest.raises(ValueError, match="P >= 1"):
        ops.kmn_knm_vjp(spec, X, Z, None, Y[:, :0], Gb[:, :0])
    # libmgp itself: Gq = NULL with P = 0 is a bad argument
    hd = _hip.get_handle(DEV)
    k = spec.struct(_hip.dtype_code(X))
    dv, dl = ctypes.c_double(0.0), (ctypes.c_double * _hip.MGP_MAX_D)()
    rc = hd.lib.mgp_kmn_knm_vjp(hd.h, ctypes.byref(k), _hip.ptr(X), 50, _hip.ptr(Z), 37, None, None, None, 0,
                                ctypes.byref(dv), dl, None)
    assert rc != 0 and b"Gq = NULL" in hd.lib.mgp_last_error(hd.h)
    with pytest.raises(_hip.MgpError, match="fp64"):
        ops.kmn_knm_vjp(spec, X.float(), Z.float(), None, Y.float(), Gb.float())
    with pytest.raises(_hip.MgpError, match="D = 33"):
        ops.kmn_knm_vjp(spec_of("se", 33), T(np.zeros((4, 33))), T(np.zeros((3, 33))), None, T(np.zeros((4, 1))),
                        T(np.zeros((3, 1))))


# ---------------------------------------------------------------- 3. memory
@pytest.mark.parametrize("P", [4, 300])
def test_nothing_n_by_m_or_m_by_m_is_reserved(monkeypatch, P):
    """N = M = 8192 on a fresh handle.  Fused form (P = 4): under one eighth of an [N, M] array (64 MiB; the pack,
    the partials and dZ come to about 10 MB).  Panel form (P = 300): under two 256 MiB panels plus an eighth of
    8 M^2 -- room for W panels and the partials, none for G2 on top of them."""
    from cggp import ops
    M, D = 8192, 3
    _, Z, Y, Gb = vjp_inputs(M, M, D, P, 5, same=True)
    Zt, Yt, Gbt = T(Z), T(Y), T(Gb)
    bound = 8 * M * M // 8 if P <= P_FUSED else 2 * (256 << 20) + 8 * M * M // 8
    with switch_forms.switched(monkeypatch, {}) as hd:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base, ws0 = torch.cuda.memory_allocated(), hd.lib.mgp_workspace_bytes(hd.h)
        dv, dl, dZ = ops.kmn_knm_vjp(spec_of("se", D), Zt, Zt, None, Yt, Gbt, need_dZ=True)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base + hd.lib.mgp_workspace_bytes(hd.h) - ws0
    print(f"P={P}: {extra / 2 ** 20:.1f} MiB above the start (bound {bound / 2 ** 20:.0f} MiB)")
    assert np.isfinite(dv) and bool(torch.isfinite(dZ).all())
    assert 0 < extra < bound


# ---------------------------------------------------------------- 4. the buffer contract of the new route
def guarded_call(hd, spec, arrays, N, M, P, D):
    """one raw call with every array in a guard-banded buffer whose payload starts one element past a 16-byte
    boundary; returns (dvariance, dl, the Guarded of dZ, the Guardeds of the inputs)"""
    from cggp import _hip
    ins = {}
    for key, a in arrays.items():
        ins[key] = Guarded(a.shape, torch.float64, 1, DEV).upload(torch.from_numpy(np.ascontiguousarray(a)))
    out = Guarded((M, D), torch.float64, 1, DEV)
    k = spec.struct(_hip.F64)
    dv, dl = ctypes.c_double(0.0), (ctypes.c_double * _hip.MGP_MAX_D)()
    p = lambda g: ctypes.c_void_p(g.ptr)
    hd.check(hd.lib.mgp_kmn_knm_vjp(hd.h, ctypes.byref(k), p(ins["X"]), N, p(ins["Z"]), M, None, p(ins["Y"]),
                                    p(ins["Gb"]), P, ctypes.byref(dv), dl, p(out)))
    return dv.value, [dl[d] for d in range(D)], out, ins


@pytest.mark.parametrize("name,D,P", [("se", 5, 3), ("matern12", 3, 11), ("matern32", 32, 9), ("matern52", 5, 40)])
def test_guard_bands_stay_and_dz_is_fully_written(name, D, P):
    from cggp import _hip
    N, M = 333, 70
    X, Z, Y, Gb = vjp_inputs(N, M, D, P, 6)
    hd = _hip.get_handle(DEV)
    dv, dl, out, ins = guarded_call(hd, spec_of(name, D), dict(X=X, Z=Z, Y=Y, Gb=Gb), N, M, P, D)
    torch.cuda.synchronize()
    for key, g in ins.items():
        g.check_input(key)
    out.check_output(None, "dZ")
    check_against_long_double(name, D, X, Z, Y, Gb, (dv, dl, out.payload))


def test_a_call_behind_an_unfinished_producer_on_a_side_stream():
    """the wrapper's read-back of the host scalars must wait for the stream the call was enqueued on; the inputs are
    filled by copies queued behind ~20 matrix products of 4096^3"""
    from cggp import ops
    N, M, D, P = 777, 130, 5, 6
    X, Z, Y, Gb = vjp_inputs(N, M, D, P, 7)
    staged = dict(X=T(X), Z=T(Z), Y=T(Y), Gb=T(Gb))
    bufs = {k: torch.full_like(v, float("nan")) for k, v in staged.items()}
    a = (torch.randn((4096, 4096), generator=torch.Generator().manual_seed(0)) / 64.0).to(DEV)
    b = torch.empty_like(a)
    side = torch.cuda.Stream(device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        x = a
        for _ in range(10):
            torch.matmul(x, a, out=b)
            x = torch.matmul(b, a)
        e1.record()
        for k in bufs:
            bufs[k].copy_(staged[k], non_blocking=True)
        dv, dl, dZ = ops.kmn_knm_vjp(spec_of("matern32", D), bufs["X"], bufs["Z"], None, bufs["Y"], bufs["Gb"],
                                     need_dZ=True)
        dZ = dZ.clone()
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= 5.0, "the producers were too short: the test proves nothing"
    check_against_long_double("matern32", D, X, Z, Y, Gb, (dv, dl, dZ))


# ---------------------------------------------------------------- 5. the three nodes with Z.requires_grad
@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_the_nodes_send_back_the_gradient_in_z(kind):
    from cggp.training import _KzzLambdaLogdet, _KzzLambdaSolve, _KzzTimes
    M, D, R = 40, 3, 17
    rng = np.random.default_rng(9)
    c = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    Z, V, G = c(rng.uniform(-1.5, 1.5, (M, D))), c(rng.standard_normal((M, R))), c(rng.standard_normal((M, R)))
    lam, ls, variance = c(rng.uniform(0.3, 1.2, M)), c(rng.uniform(0.6, 1.4, D)), c(1.7)

    def close(name, got, want, bar):
        got, want = torch.as_tensor(got).detach().cpu().reshape(-1), torch.as_tensor(want).detach().reshape(-1)
        dist = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{kind} {name}: {dist:.2e} (bar {bar:.0e})")
        assert dist <= bar, (name, dist)

    def leaves(*extra):
        return [t.clone().requires_grad_(True) for t in (variance, ls, Z) + extra]

    def device_leaves(*extra):
        return (variance.clone().requires_grad_(True), ls.clone().requires_grad_(True),
                Z.to(DEV).requires_grad_(True)) + tuple(t.to(DEV).requires_grad_(True) for t in extra)

    Gd = G.to(DEV)
    # K V
    v, l, z, Vl = leaves(V)
    want = torch.autograd.grad(((tip.kzz(kind, v, l, z) @ Vl) * G).sum(), [v, l, z, Vl])
    v, l, z, Vl = device_leaves(V)
    (_KzzTimes.apply(v, l, z, Vl, kind) * Gd).sum().backward()
    for name, g, w in zip(("times dvariance", "times dls", "times dZ", "times dV"), (v.grad, l.grad, z.grad, Vl.grad),
                          want):
        close(name, g, w, 1e-10)
    assert z.grad.shape == (M, D) and z.grad.device == z.device

    # (K + diag lam)^-1 rhs
    v, l, z, rhs, lm = leaves(V, lam)
    X = torch.linalg.solve(tip.kzz(kind, v, l, z) + torch.diag(lm), rhs)
    want = torch.autograd.grad((X * G).sum(), [v, l, z, rhs, lm])
    v, l, z, rhs, lm = device_leaves(V, lam)
    (_KzzLambdaSolve.apply(v, l, lm, rhs, z, kind, tight_cg(M, 1e-26)) * Gd).sum().backward()
    for name, g, w in zip(("solve dvariance", "solve dls", "solve dZ", "solve drhs", "solve dlam"),
                          (v.grad, l.grad, z.grad, rhs.grad, lm.grad), want):
        close(name, g, w, 1e-8)

    # the log-determinant's estimator, S handed in
    probes = probes_of(M, 5, 2)
    v, l, z, lm = leaves(lam)
    A = tip.kzz(kind, v, l, z) + torch.diag(lm)
    S = torch.linalg.solve(A, probes.cpu()).detach()
    want = torch.autograd.grad(0.7 * (S * (A @ probes.cpu())).sum() / 5, [v, l, z, lm])
    v, l, z, lm = device_leaves(lam)
    (0.7 * _KzzLambdaLogdet.apply(v, l, lm, S.to(DEV), probes, z, kind, None)).backward()
    for name, g, w in zip(("logdet dvariance", "logdet dls", "logdet dZ", "logdet dlam"),
                          (v.grad, l.grad, z.grad, lm.grad), want):
        close(name, g, w, 1e-10)


# ---------------------------------------------------------------- 6. the model
M_MODEL, B_MODEL = 200, 50


def model_loss_and_grads(m, data, probes):
    for p in m.parameters():
        p.grad = None
    loss = m.training_loss(data, probes=probes)
    loss.backward()
    ps = m.parameters()
    hyper = torch.cat([p.grad.reshape(-1) for p in ps[:3]]).numpy()
    return float(loss.detach()), hyper, ps[3].grad.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference_loss_and_grads(kind, D, independent):
    """the CPU reference at the model's starting point, in the model's raw (softplus) parameters; computed once"""
    from cggp.models import rademacher
    m, (x, y) = trainable(kind, D, M_MODEL, B_MODEL, False, trainable_inducing=True)
    raws = [p.detach().clone().requires_grad_(True) for p in m.parameters()[:3]]
    Z = m.Z.detach().cpu().clone().requires_grad_(True)
    variance, ls, s2 = F.softplus(raws[0])[0], F.softplus(raws[1]), F.softplus(raws[2])[0]
    probes = probes_of(M_MODEL, 5, 11).cpu()
    own = rademacher((M_MODEL, 5), torch.float64, DEV, m.logdet_probe_seed).cpu() if independent else None
    loss = -tip.elbo(kind, variance, ls, s2, Z, x.cpu(), y.cpu(), m.pseudo_u.cpu(), m.cluster_counts.cpu(), probes,
                     num_data=m.num_data, logdet_probes=own)
    grads = torch.autograd.grad(loss, raws + [Z])
    return float(loss.detach()), torch.cat([g.reshape(-1) for g in grads[:3]]).numpy(), grads[3].numpy()


def compare(tag, got, want, D):
    (l_g, h_g, z_g), (l_w, h_w, z_w) = got, want
    dh = np.max(np.abs(h_g - h_w)) / np.max(np.abs(h_w))
    dz = np.max(np.abs(z_g - z_w)) / np.max(np.abs(z_w))
    print(f"{tag}: loss {rel(l_g, l_w):.2e} (bar 1e-8), [variance, {D} lengthscales, noise] {dh:.2e}, Z {dz:.2e} "
          "(bar 1e-7)")
    assert h_g.shape == (D + 2,) and z_g.shape == (M_MODEL, D)
    assert np.all(np.isfinite(h_g)) and np.all(np.isfinite(z_g))
    assert rel(l_g, l_w) <= 1e-8 and dh <= 1e-7 and dz <= 1e-7


@pytest.mark.parametrize("variant", ["plain", "fused_solves", "independent_logdet_probes"])
@pytest.mark.parametrize("kind,D", [("se", 4), ("matern32", 4)])
def test_loss_and_gradient_with_z_dense_matrix_free_and_reference_agree(kind, D, variant):
    kw = {} if variant == "plain" else {variant: True}
    independent = variant == "independent_logdet_probes"
    want = reference_loss_and_grads(kind, D, independent)
    pr = probes_of(M_MODEL, 5, 11)
    out = {}
    for mf in (False, True):
        m, data = trainable(kind, D, M_MODEL, B_MODEL, mf, trainable_inducing=True, **kw)
        assert len(m.parameters()) == 4 and m.parameters()[3] is m.Z
        out[mf] = model_loss_and_grads(m, data, pr)
        compare(f"{kind} D={D} {variant} {'matrix-free' if mf else 'dense'} against the reference", out[mf], want, D)
    compare(f"{kind} D={D} {variant} matrix-free against dense", out[True], out[False], D)


def test_the_dense_model_trains_z_at_33_dimensions():
    kind, D = "matern32", 33
    m, data = trainable(kind, D, M_MODEL, B_MODEL, False, trainable_inducing=True)
    got = model_loss_and_grads(m, data, probes_of(M_MODEL, 5, 11))
    compare(f"{kind} D={D} dense against the reference", got, reference_loss_and_grads(kind, D, False), D)
    with pytest.raises(ValueError, match="D <= 32"):
        trainable(kind, D, M_MODEL, B_MODEL, True, trainable_inducing=True)


# ---------------------------------------------------------------- 7. the flow
def test_adam_moves_z_and_the_frozen_model_takes_a_copy():
    from cggp.training import train_using_adam_and_update
    m, data = trainable("se", 4, 200, 50, True, trainable_inducing=True)
    pr = probes_of(200, 5, 12)
    z0 = m.Z.detach().clone()
    before = float(m.training_loss(data, probes=pr).detach())
    losses = train_using_adam_and_update(data, m, 3, 50, 0.05)
    after = float(m.training_loss(data, probes=pr).detach())
    moved = float((m.Z.detach() - z0).abs().max())
    print(f"{before:.6f} -> {after:.6f} ({losses}), Z moved by up to {moved:.3e}")
    assert len(losses) == 3 and np.all(np.isfinite(losses)) and after < before
    assert moved > 0.0 and bool(torch.isfinite(m.Z).all())
    frozen = m.frozen_model()
    fz = frozen.inducing_variable.Z
    assert frozen.matrix_free and torch.equal(fz, m.Z.detach()) and not fz.requires_grad
    assert fz.data_ptr() != m.Z.data_ptr()
    with torch.no_grad():
        m.Z.add_(1.0)
    assert not torch.equal(fz, m.Z.detach())


def test_lbfgs_takes_z_among_the_parameters():
    from cggp.training import train_using_lbfgs_and_update
    m, data = trainable("matern32", 4, 200, 50, True, trainable_inducing=True)
    z0 = m.Z.detach().clone()
    res = train_using_lbfgs_and_update(data, m, 2)
    assert res is not None and np.isfinite(res.fun)
    assert res.x.shape == (4 + 2 + 200 * 4,) and np.all(np.isfinite(res.x))
    assert float((m.Z.detach() - z0).abs().max()) > 0.0 and bool(torch.isfinite(m.Z).all())


@pytest.mark.parametrize("matrix_free", [False, True])
def test_z_stays_frozen_by_default(matrix_free):
    m, data = trainable("se", 4, 200, 50, matrix_free)
    m.training_loss(data, probes=probes_of(200, 5, 12)).backward()
    assert len(m.parameters()) == 3 and not m.Z.requires_grad and m.Z.grad is None
    assert all(p.grad is not None for p in m.parameters())
