"""The fused any-D random-Fourier-feature kernels (MGP_RFF_ANYD on `mgp_rff_sample` / `mgp_rff_sample_vjp`,
csrc/rff_anyd.hip, include/mgp_pathwise.h) against the long-double reference of tests/rff_vjp_reference.py.

Bounds (the header states them; tests/rff_anyd_reference.py evaluates them; nothing in them is fitted to the output):
    |out(s, n) - exact|    <= u (8 + (K + 2) P + 2 len + nsplit + 2) |scale| sum_l (|W[s, l]| + |W[s, L + l]|)
    |dtheta[l, d] - exact| <= u (8 + (K + 2) P + S + len + nsplit + 4)
                              |scale| sum_n sum_s |G(s, n)| (|W[s, l]| + |W[s, L + l]|) |x_n[d]|
and the same for dX with |theta_l[d]| and the sum over l; K = 4 ceil(D / 4), P = max_nl sum_d |x_nd theta_ld|, len
and nsplit by the split rule.  The long-double reference's own error (2^-64 times the same sums) is 2^-11 of that.

Without the feature every test here fails at its first flagged call: the layout word is `bad out_layout` /
`bad g_layout`, and the `anyd=` / `rff_anyd=` keywords are a TypeError.
"""

import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import rff_anyd_reference as ra
from buffer_contract import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MGP_E_BADARG, MGP_E_DTYPE, MGP_E_NOMEM = -1, -3, -6  # include/mgp.h
OPS = ("forward", "dtheta", "dX", "both")


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def make(N, L, D, S, seed, kind="se", lscale=1.0):
    from cggp import kernels, rff
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    if kind == "se":
        theta = rng.standard_normal((L, D)) / lscale
    else:  # Matern-1/2 law: Cauchy-tailed frequencies
        theta = rff.basis_theta_parameter(kernels.Matern12(lengthscales=[lscale] * D), L, rng).numpy()
    W = rng.standard_normal((S, 2 * L))
    G = rng.standard_normal((S, N))
    return X, theta, W, math.sqrt(1.7 / max(L, 1)), G


@functools.lru_cache(maxsize=None)
def problem(N, L, D, S, kind="se", lscale=1.0):
    """inputs, long-double results and bounds of a case; computed once and left unchanged"""
    X, theta, W, scale, G = make(N, L, D, S, seed=N + 3 * L + 5 * D + 7 * S, kind=kind, lscale=lscale)
    return (X, theta, W, scale, G), reference(X, theta, W, scale, G)


def reference(X, theta, W, scale, G):
    rt, rx = ra.vjp(X, theta, W, scale, G)
    bt, bx = ra.vjp_bounds(X, theta, W, scale, G, num_cus())
    return {"forward": (ra.forward(X, theta, W, scale), ra.forward_bound(X, theta, W, scale, num_cus())),
            "dtheta": (rt, bt), "dX": (rx, bx)}


def run(args, op, layout, anyd=True):
    """{name: numpy} of the outputs `op` asks for; G and out are [S, N] here, handed over in `layout`."""
    from cggp import ops
    X, theta, W, scale, G = args
    rows = layout == ops.ROWS
    if op == "forward":
        out = ops.rff_sample(T(X), T(theta), T(W), scale, layout, anyd=anyd)
        torch.cuda.synchronize()
        return {"forward": (out if rows else out.t()).cpu().numpy()}
    dt, dx = ops.rff_sample_vjp(T(X), T(theta), T(W), scale, T(G) if rows else T(G.T), layout,
                                want_dtheta=op != "dX", want_dX=op != "dtheta", anyd=anyd)
    torch.cuda.synchronize()
    assert (dt is None) == (op == "dX") and (dx is None) == (op == "dtheta")
    return {k: v.cpu().numpy() for k, v in (("dtheta", dt), ("dX", dx)) if v is not None}


def hold(got, ref, tag):
    for name, g in got.items():
        want, bound = ref[name]
        assert g.shape == want.shape and np.all(np.isfinite(g)), (tag, name)
        err = np.abs(g - want.astype(np.float64))
        ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
        print(f"{tag} {name}: worst error / bound {ratio:.3g}")
        assert np.all(err <= bound), (tag, name, ratio)


# (N, L, D, S): the smallest case; D = 36 where K is an exact multiple of 4; 64 / 65 across a K-slice boundary (8
# k-steps of 4); 77 and 90 (the reference's UCI sets) with more than one owner workgroup and odd tile remainders;
# 256 / 257 across the output-dimension group boundary and 512, the largest D
CASES = [(1, 1, 33, 1), (17, 15, 33, 5), (64, 32, 36, 2), (50, 40, 64, 4), (50, 40, 65, 4), (130, 65, 77, 5),
         (300, 257, 90, 8), (67, 33, 256, 3), (67, 33, 257, 3), (40, 33, 512, 8)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case", CASES, ids=["N%d_L%d_D%d_S%d" % c for c in CASES])
def test_against_long_double(case, op):
    from cggp import ops
    args, ref = problem(*case)
    rows = run(args, op, ops.ROWS)
    hold(rows, ref, f"{case} rows")
    cols = run(args, op, ops.COLS)
    hold(cols, ref, f"{case} cols")
    for k in rows:  # the layout only changes where G is read and out is written
        assert np.array_equal(rows[k], cols[k]), k


@pytest.mark.parametrize("op", OPS)
def test_matern12_large_phases(op):
    """Cauchy frequencies at lengthscale 1e-3: phases of 1e4 - 1e6 rad, reduced exactly in revolutions."""
    from cggp import ops
    args, ref = problem(130, 65, 77, 5, kind="matern12", lscale=1e-3)
    ph = np.abs(args[0] @ args[1].T)
    assert 1e4 < float(np.max(ph)) and float(np.median(ph)) < 1e6
    hold(run(args, op, ops.ROWS), ref, "matern12")


def test_values_on_both_sides_of_every_cut():
    """Few owned points, a long streamed side, in both roles: cotangent (dtheta) / weights (forward, dX) only on the
    last point before and the first point after every cut the plan names, so every output is a sum of terms that reach
    it through different partials."""
    from cggp import ops
    cu = num_cus()
    # dtheta: 40 owned bases, 1000 streamed rows
    N, L, D, S = 1000, 40, 77, 5
    cuts = ra.cuts(L, N, 1, cu)
    assert ra.split_plan(L, N, 1, cu) == (4, 16) and cuts == [256, 512, 768]
    X, theta, W, scale, G = make(N, L, D, S, seed=9)
    keep = np.zeros(N, dtype=bool)
    keep[[c - 1 for c in cuts] + cuts] = True
    args = (X, theta, W, scale, G * keep[None, :])
    hold(run(args, "dtheta", ops.ROWS), reference(*args), "cut dtheta")
    # forward and dX: 40 owned rows, 1000 streamed bases
    N, L = 40, 1000
    assert ra.cuts(N, L, 1, cu) == cuts
    X, theta, W, scale, G = make(N, L, D, S, seed=10)
    mask = np.zeros(L, dtype=bool)
    mask[[c - 1 for c in cuts] + cuts] = True
    Wk = W * np.concatenate([mask, mask])[None, :]
    args = (X, theta, Wk, scale, G)
    ref = reference(*args)
    hold(run(args, "forward", ops.ROWS), ref, "cut forward")
    hold(run(args, "dX", ops.COLS), ref, "cut dX")
    # and the dense form of the same shapes: every split full
    args = (X, theta, W, scale, G)
    ref = reference(*args)
    for op in ("forward", "dX"):
        hold(run(args, op, ops.ROWS), ref, "split " + op)


def test_two_calls_same_bits():
    from cggp import ops
    for case in ((300, 257, 90, 8), (40, 1000, 77, 5)):
        args = make(*case, seed=3)
        for op in ("forward", "both"):
            a, b = run(args, op, ops.ROWS), run(args, op, ops.ROWS)
            assert all(np.array_equal(a[k], b[k]) for k in a)


@contextlib.contextmanager
def fresh_handle(pool=0):
    """A handle nothing else has touched; pool > 0: a fixed workspace of that many bytes."""
    from cggp import _hip
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
    lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    try:
        yield lib, h
    finally:
        torch.cuda.synchronize()
        lib.mgp_destroy(h)


def raw(lib, h, op, dev, N, L, D, S, scale, layout, dtype=None):
    """the C calls on device tensors dev = (X, theta, W, G); returns (rc, outputs)"""
    from cggp import _hip
    p = lambda t: ctypes.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    X, th, W, G = dev
    dtype = _hip.F64 if dtype is None else dtype
    if op == "forward":
        out = torch.empty((S, N), dtype=torch.float64, device=DEV)
        rc = lib.mgp_rff_sample(h, dtype, p(X), N, D, p(th), L, p(W), S, scale, p(out), layout)
        return rc, (out,)
    dt = torch.empty((L, D), dtype=torch.float64, device=DEV) if op != "dX" else None
    dx = torch.empty((N, D), dtype=torch.float64, device=DEV) if op != "dtheta" else None
    rc = lib.mgp_rff_sample_vjp(h, dtype, p(X), N, D, p(th), L, p(W), S, scale, p(G), layout, p(dt), p(dx))
    return rc, tuple(t for t in (dt, dx) if t is not None)


@pytest.mark.parametrize("op", ["forward", "both"])
def test_stateless_behind_poison_in_every_arena(op):
    """Alone on a fresh handle; then on another handle behind larger calls on NaN inputs that fill the arenas the route
    shares ("gen" by the flagged calls themselves and by the panel route, "ws" by the plain fused calls): same bits."""
    from cggp import _hip
    N, L, D, S = 130, 65, 77, 5
    X, theta, W, scale, G = make(N, L, D, S, seed=4)
    dev = (T(X), T(theta), T(W), T(G))
    flag = _hip.ROWS | _hip.RFF_ANYD
    with fresh_handle() as (lib, h):
        rc, alone = raw(lib, h, op, dev, N, L, D, S, scale, flag)
        assert rc == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    with fresh_handle() as (lib, h):
        big = (nan(400, D), nan(300, D), nan(8, 600), nan(8, 400))
        for o in ("forward", "both"):  # the route's own arena, larger and full of NaN
            assert raw(lib, h, o, big, 400, 300, D, 8, 1.0, flag)[0] == 0
        assert raw(lib, h, "forward", big, 400, 300, D, 8, 1.0, _hip.ROWS)[0] == 0  # the panel route: "gen"
        small = (nan(400, 8), nan(300, 8), nan(8, 600), nan(8, 400))
        for o in ("forward", "both"):  # the plain fused calls: "gen" and "ws"
            assert raw(lib, h, o, small, 400, 300, 8, 8, 1.0, _hip.ROWS)[0] == 0
        assert lib.mgp_arena_bytes(h, b"gen") > 0 and lib.mgp_arena_bytes(h, b"ws") > 0
        rc, behind = raw(lib, h, op, dev, N, L, D, S, scale, flag)
        assert rc == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(alone, behind))


def test_flag_outside_the_route_is_the_plain_call():
    """D = 8, and S = 9 on the forward: with the flag the plain code, bit for bit."""
    from cggp import ops
    for case in ((70, 33, 8, 5), (70, 33, 40, 9)):
        args = make(*case, seed=6)
        a, b = run(args, "forward", ops.ROWS, anyd=True), run(args, "forward", ops.ROWS, anyd=False)
        assert np.array_equal(a["forward"], b["forward"])
    args = make(70, 33, 8, 5, seed=6)
    a, b = run(args, "both", ops.COLS, anyd=True), run(args, "both", ops.COLS, anyd=False)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_refusals():
    from cggp import _hip, ops
    hd = _hip.get_handle(DEV)
    lib = hd.lib
    o = lambda *s: torch.ones(s, dtype=torch.float64, device=DEV)
    N, L, D = 5, 4, 33
    dev = (o(N, D), o(L, D), o(2, 2 * L), o(2, N))
    flag = _hip.ROWS | _hip.RFF_ANYD
    assert raw(lib, hd.h, "both", dev, N, L, D, 2, 1.0, flag)[0] == 0
    assert raw(lib, hd.h, "forward", dev, N, L, D, 2, 1.0, flag)[0] == 0
    # fp32 and S = 9 in the backward pass
    assert raw(lib, hd.h, "both", dev, N, L, D, 2, 1.0, flag, dtype=_hip.F32)[0] == MGP_E_DTYPE
    dev9 = (o(N, D), o(L, D), o(9, 2 * L), o(9, N))
    assert raw(lib, hd.h, "dtheta", dev9, N, L, D, 9, 1.0, flag)[0] == MGP_E_BADARG
    assert b"S = 9" in lib.mgp_last_error(hd.h)
    # any other bit of the layout word
    for bad in (flag | 2, flag | 32, _hip.COLS | 4 | _hip.RFF_ANYD, -1):
        assert raw(lib, hd.h, "forward", dev, N, L, D, 2, 1.0, bad)[0] == MGP_E_BADARG
        assert b"bad out_layout" in lib.mgp_last_error(hd.h)
        assert raw(lib, hd.h, "both", dev, N, L, D, 2, 1.0, bad)[0] == MGP_E_BADARG
        assert b"bad g_layout" in lib.mgp_last_error(hd.h)
    assert raw(lib, hd.h, "forward", dev, N, L, D, 2, 1.0, _hip.ROWS | 4)[0] == MGP_E_BADARG  # and without the flag
    # the plain backward call still refuses D = 33; the flagged one D = 513
    assert raw(lib, hd.h, "dtheta", dev, N, L, D, 2, 1.0, _hip.ROWS)[0] == MGP_E_BADARG
    assert b"33" in lib.mgp_last_error(hd.h)
    assert raw(lib, hd.h, "dtheta", dev, N, L, 513, 2, 1.0, flag)[0] == MGP_E_BADARG
    # both outputs NULL
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    X, th, W, G = dev
    assert lib.mgp_rff_sample_vjp(hd.h, _hip.F64, p(X), N, D, p(th), L, p(W), 2, 1.0, p(G), flag, None,
                                  None) == MGP_E_BADARG
    assert b"both NULL" in lib.mgp_last_error(hd.h)
    torch.cuda.synchronize()
    with pytest.raises(_hip.MgpError):  # the wrapper: fp32 reaches libmgp and is refused there
        ops.rff_sample_vjp(*(t.float() for t in (X, th, W)), 1.0, G.float(), anyd=True)


def test_zero_cotangent_and_empty_sides():
    from cggp import ops
    X, theta, W, scale, G = make(70, 33, 40, 5, seed=5)
    got = run((X, theta, W, scale, np.zeros_like(G)), "both", ops.ROWS)
    assert not got["dtheta"].any() and not got["dX"].any()
    e = lambda *s: torch.empty(s, dtype=torch.float64, device=DEV)
    sent = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=DEV)
    dt, dx = ops.rff_sample_vjp(e(0, 40), T(theta), T(W), scale, e(5, 0), ops.ROWS, want_dX=True, anyd=True)  # N = 0
    assert dt.shape == (33, 40) and torch.count_nonzero(dt) == 0 and dx.shape == (0, 40)
    dt, dx = ops.rff_sample_vjp(T(X), e(0, 40), e(5, 0), scale, T(G), ops.ROWS, want_dX=True, anyd=True)  # L = 0
    assert dx.shape == (70, 40) and torch.count_nonzero(dx) == 0 and dt.shape == (0, 40)
    out = ops.rff_sample(T(X), e(0, 40), e(5, 0), scale, ops.ROWS, anyd=True)  # L = 0: zeros
    assert out.shape == (5, 70) and torch.count_nonzero(out) == 0
    assert ops.rff_sample(e(0, 40), T(theta), T(W), scale, ops.ROWS, anyd=True).shape == (5, 0)
    # the C calls: N = 0 writes nothing to out / dX, L = 0 nothing to dtheta
    from cggp import _hip
    hd = _hip.get_handle(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    flag = _hip.ROWS | _hip.RFF_ANYD
    keep, dth = sent(8), sent(33, 40)
    assert hd.lib.mgp_rff_sample(hd.h, _hip.F64, p(keep), 0, 40, p(T(theta)), 33, p(T(W)), 5, scale, p(keep), flag) == 0
    assert hd.lib.mgp_rff_sample_vjp(hd.h, _hip.F64, p(keep), 0, 40, p(T(theta)), 33, p(T(W)), 5, scale, p(keep), flag,
                                     p(dth), p(keep)) == 0
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all()) and torch.count_nonzero(dth) == 0


@pytest.mark.parametrize("op", ["forward", "dtheta", "dX"])
def test_guard_bands(op):
    """Inputs and outputs one element past a 16-byte boundary between guard bands: every documented element written,
    nothing else touched, no input changed."""
    from cggp import _hip
    N, L, D, S = 37, 21, 45, 3
    X, theta, W, scale, G = make(N, L, D, S, seed=8)
    ins = [guarded(a.shape, torch.float64, 1, DEV)[1].upload(torch.from_numpy(a)) for a in (X, theta, W, G)]
    shapes = {"forward": [(S, N)], "dtheta": [(L, D)], "dX": [(N, D)]}[op]
    outs = [guarded(s, torch.float64, 1, DEV)[1] for s in shapes]
    hd = _hip.get_handle(DEV)
    p = lambda g: ctypes.c_void_p(g.ptr)
    flag = _hip.ROWS | _hip.RFF_ANYD
    if op == "forward":
        rc = hd.lib.mgp_rff_sample(hd.h, _hip.F64, p(ins[0]), N, D, p(ins[1]), L, p(ins[2]), S, scale, p(outs[0]), flag)
    else:
        rc = hd.lib.mgp_rff_sample_vjp(hd.h, _hip.F64, p(ins[0]), N, D, p(ins[1]), L, p(ins[2]), S, scale, p(ins[3]),
                                       flag, p(outs[0]) if op == "dtheta" else None, p(outs[0]) if op == "dX" else None)
    assert rc == 0, hd.lib.mgp_last_error(hd.h)
    torch.cuda.synchronize()
    for g, name in zip(ins, ("X", "theta", "W", "G")):
        g.check_input(name)
    outs[0].check_output(name=op)
    hold({op: outs[0].payload.cpu().numpy()}, reference(X, theta, W, scale, G), "guarded")


@pytest.mark.parametrize("op", ["forward", "dtheta", "dX", "both"])
def test_fixed_pool_of_the_documented_bytes(op):
    """A fixed pool of exactly the header's bytes serves the call with the bits of a growing handle; one byte less is
    MGP_E_NOMEM (never an allocation).  40 owned points against 1000 streamed (and the reverse): with partials."""
    from cggp import _hip
    N, L, D, S = (1000, 40, 77, 5) if op == "dtheta" else (40, 1000, 77, 5)
    X, theta, W, scale, G = make(N, L, D, S, seed=13)
    dev = (T(X), T(theta), T(W), T(G))
    flag = _hip.ROWS | _hip.RFF_ANYD
    need = ra.scratch_bytes(N, L, D, num_cus(), op)

    def attempt(pool):
        with fresh_handle(pool) as (lib, h):
            base = int(lib.mgp_workspace_bytes(h))
            rc, outs = raw(lib, h, op, dev, N, L, D, S, scale, flag)
            torch.cuda.synchronize()
            return rc, base, int(lib.mgp_workspace_bytes(h)), int(lib.mgp_arena_bytes(h, b"gen")), \
                lib.mgp_last_error(h), outs

    rc, _, _, gen, _, free = attempt(0)
    assert rc == 0 and gen >= need  # a growing handle rounds up
    rc, base, used, gen, _, roomy = attempt(64 << 20)
    assert rc == 0 and gen == need and used == ra.a256(base) + need  # the documented bytes, from one arena
    rc, _, used2, _, _, exact = attempt(used)
    assert rc == 0 and used2 == used
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(free, roomy, exact))
    rc, _, _, _, msg, _ = attempt(used - 1)
    assert rc == MGP_E_NOMEM and b"fixed workspace exhausted" in msg


# ---------------------------------------------------------------- models
def test_rff_sample_node_agrees_with_the_panel_route():
    """`_RffSample` with the keyword at D = 40 against the same node without it (feature panels forward,
    `_rff_vjp_panels` backward): each side within its bound of the exact value, so the two within the sum -- the panel
    route's bound being the plain call's form with the whole streamed side as one chain (a K = N or L GEMM):
    u (8 (1 + P) + 2 S + D + streamed + 4) times the same sums."""
    from cggp.training import _RffSample
    B, M, L, D, S = 90, 30, 50, 40, 5
    X, theta, W, scale, G = make(B + M, L, D, S, seed=12)
    out = {}
    for anyd in (False, True):
        th, Z = T(theta).requires_grad_(True), T(X[B:]).requires_grad_(True)
        sc = torch.tensor(scale, dtype=torch.float64, device=DEV, requires_grad=True)
        prior = _RffSample.apply(th, sc, T(X[:B]), Z, T(W), anyd) if anyd else _RffSample.apply(th, sc, T(X[:B]), Z, T(W))
        prior.backward(T(G))
        out[anyd] = [t.detach().cpu().numpy() for t in (prior, th.grad, Z.grad, sc.grad)]
    ref = reference(X, theta, W, scale, G)
    hold({"forward": out[True][0], "dtheta": out[True][1]}, ref, "node")
    refz = reference(X[B:], theta, W, scale, G[:, B:])
    hold({"dX": out[True][2]}, refz, "node dZ")
    pmax = float(np.max(np.abs(X) @ np.abs(theta).T))
    absw = abs(scale) * (np.abs(W[:, :L]) + np.abs(W[:, L:])).sum(axis=1)
    panel_f = ra.U * (8 * (1 + pmax) + 2 * L + 2) * absw[:, None]
    assert np.all(np.abs(out[True][0] - out[False][0]) <= ref["forward"][1] + panel_f)
    A = abs(scale) * (np.abs(G).T @ (np.abs(W[:, :L]) + np.abs(W[:, L:])))
    panel_t = ra.U * (8 * (1 + pmax) + 2 * S + D + (B + M) + 4) * (A.T @ np.abs(X))
    assert np.all(np.abs(out[True][1] - out[False][1]) <= ref["dtheta"][1] + panel_t)
    panel_z = ra.U * (8 * (1 + pmax) + 2 * S + D + L + 4) * (A[B:] @ np.abs(theta))
    assert np.all(np.abs(out[True][2] - out[False][2]) <= refz["dX"][1] + panel_z)
    assert abs(out[True][3] - out[False][3]) <= 1e-12 * abs(out[False][3]) + 1e-300


def test_trainable_cggp_and_pathwise_cluster_gp():
    """`TrainableCGGP(data_term="pathwise", rff_anyd=True)` loss + backward at D = 40 (N = 300, M = 24, L = 64, S = 5)
    against `rff_anyd=False`, and `PathwiseClusterGP(rff_anyd=True).pathwise_samples` likewise.  The two prior draws
    differ by at most the two bounds (some 1e-13 of the draw); what follows is the same code on both sides, a tightly
    converged CG included (threshold 1e-15), so the difference is that perturbation times the conditioning of
    K_mm + Lambda: the bars are those of tests/test_gpu_cdgp_pathwise.py for two routes of one model, 1e-8 on the
    loss and 1e-7 on each gradient group, relative to the group's largest entry."""
    from cggp.models import PathwiseClusterGP
    from test_gpu_cdgp_full import compare, make as make_full
    from test_gpu_cdgp_matrix_free import probes_of
    from test_gpu_cdgp_pathwise import draw_of, loss_and_grads
    D, M, N, L, S = 40, 24, 300, 64, 5
    got = {}
    for anyd in (False, True):
        m, data = make_full("se", D, M, N, False, data_term="pathwise", num_bases=L, num_samples=S, rff_anyd=anyd)
        got[anyd] = loss_and_grads(m, data, probes_of(M, 5, 11), draw_of(m, 7))
    compare("rff_anyd True against False", got[True], got[False], D)
    frozen = m.frozen_model()
    assert frozen.rff_anyd is True
    gp = {a: PathwiseClusterGP(frozen.kernel, frozen.likelihood.variance, m.Z, pseudo_u=m.pseudo_u,
                               cluster_counts=m.cluster_counts, rff_anyd=a) for a in (False, True)}
    a, b = (gp[k].pathwise_samples(data[0], L, S, seed=5)[..., 0].cpu().numpy() for k in (False, True))
    assert a.shape == (S, N) and np.max(np.abs(a - b)) <= 1e-8 * np.max(np.abs(a))


def test_auto_follows_the_measured_table():
    """`rff_anyd="auto"` inside a measured region (S = 5, N L = 2^22) gives the bits of True, outside it (a sample count
    that was not measured; N L below the smallest measured) those of False."""
    from cggp import kernels, rff
    N, L, D = 4096, 1024, 40
    X, theta, W, _, _ = make(N, L, D, 5, seed=14)
    kern = kernels.SquaredExponential(variance=1.3, lengthscales=[2.0] * D)
    draw = lambda W_, n, setting: rff.rff_sample(T(X[:n]), kern, L, W_.shape[0], theta=T(theta), weights=T(W_),
                                                 rff_anyd=setting)
    assert rff.rff_anyd_auto(torch.float64, D, 5, N, L) and not rff.rff_anyd_auto(torch.float64, D, 3, N, L)
    on, off, auto = (draw(W, N, s) for s in (True, False, "auto"))
    assert torch.equal(auto, on) and not torch.equal(on, off)
    assert float((on - off).abs().max()) <= 1e-12 * float(off.abs().max())
    assert torch.equal(draw(W[:3], N, "auto"), draw(W[:3], N, False))
    assert torch.equal(draw(W, N // 2, "auto"), draw(W, N // 2, False))
