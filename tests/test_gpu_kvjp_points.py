"""`mgp_k_dense_vjp_points` (include/mgp_points.h) on the GPU: the four outputs against the long-double reference of
tests/kvjp_points_reference.py at the project's fp64 VJP bar (1e-10 of each output's sum of |terms|), the panel seams,
the buffer contract, the memory bound, and the models that take it through `fused_point_grads=True`."""

import ctypes

import numpy as np
import pytest
import torch

from buffer_contract import Guarded
from kvjp_points_reference import VJP_BAR, excess, k_dense_vjp_points_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KERNELS = ["se", "matern12", "matern32", "matern52"]
E_BADARG, E_SHAPE, E_DTYPE, E_NOMEM = -1, -2, -3, -6  # include/mgp.h


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def spec_of(name, D, variance=1.3):
    from cggp import ops
    return ops.KernelSpec(name, variance, list(np.linspace(0.7, 1.4, D) * np.sqrt(D)), D)


def inputs(na, nb, D, seed, dup=0):
    rng = np.random.default_rng(seed)
    A, B = rng.uniform(-2.0, 2.0, (na, D)), rng.uniform(-2.0, 2.0, (nb, D))
    if dup:
        B[:dup] = A[:dup]  # coincident points: pairs (i, i), i < dup
    return A, B, rng.standard_normal((na, nb))


def check(name, spec, A, B, G, got, tag="", parts=("dv", "dl", "dA", "dB")):
    """every requested output within VJP_BAR of its sum of |terms|; prints the figures first"""
    ref = k_dense_vjp_points_reference(name, spec.variance, spec.lengthscales, A, B, G)
    dv, dl, dA, dB = got
    have = dict(dv=dv, dl=np.array(dl), dA=None if dA is None else dA.cpu().numpy(),
                dB=None if dB is None else dB.cpu().numpy())
    ex = {p: excess(have[p], ref[p], ref["s" + p[1:]]) for p in parts if have[p] is not None}
    print(f"{tag} {name} D={spec.D} [{A.shape[0]}, {B.shape[0]}]: error / (1e-10 sum|terms|) = "
          + ", ".join(f"{p} {v:.2e}" for p, v in ex.items()))
    for p, v in ex.items():
        assert np.all(np.isfinite(have[p])) and v <= 1.0, (p, v)
    return ref


# ---------------------------------------------------------------- 1. D <= 32: the ladder and the edges
SHAPES = [(1, 1), (31, 33), (32, 255), (33, 32), (255, 257), (256, 31), (257, 300), (300, 256), (1, 300), (300, 1)]
# a covering subset of the shapes per D (all of them at D = 32); the kernel and the view (ldg = nb + 5) are chosen by
# the case's running number, independently of which shapes are taken: every D sees all four kernels and both layouts
_TAKEN = [(D, na, nb) for i, D in enumerate([1, 3, 8, 17, 32]) for j, (na, nb) in enumerate(SHAPES)
          if (i + j) % 2 == 0 or D == 32]
LADDER = [(KERNELS[c % 4], D, na, nb, (c // 4 + c) % 2 == 1) for c, (D, na, nb) in enumerate(_TAKEN)]


@pytest.mark.parametrize("name,D,na,nb,view", LADDER)
def test_ladder_against_long_double(name, D, na, nb, view):
    from cggp import ops
    A, B, G = inputs(na, nb, D, 100 * D + na + nb)
    spec = spec_of(name, D)
    Gt = T(G)
    if view:  # ldg = nb + 5
        wide = torch.full((na, nb + 5), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, :nb] = Gt
        Gt = wide[:, :nb]
        assert Gt.stride(0) == nb + 5
    check(name, spec, A, B, G, ops.k_dense_vjp_points(spec, T(A), T(B), Gt), "ladder")


@pytest.mark.parametrize("D", [5, 40])
def test_a_one_row_cotangent_with_any_row_stride(D):
    """torch counts a [1, nb] tensor as contiguous whatever its row stride; the wrapper must not hand that stride on"""
    from cggp import ops
    nb = 70
    A, B, G = inputs(1, nb, D, 11 + D)
    spec = spec_of("matern32", D)
    Gt = T(G).as_strided((1, nb), (1, 1))
    assert Gt.is_contiguous() and Gt.stride(0) < nb
    check("matern32", spec, A, B, G, ops.k_dense_vjp_points(spec, T(A), T(B), Gt), "one row")


@pytest.mark.parametrize("name,D", [("se", 3), ("matern12", 8), ("matern32", 17), ("matern52", 32), ("se", 48)])
def test_one_side_or_none_and_the_scalars_of_k_dense_vjp(name, D):
    from cggp import ops
    na, nb = 257, 130
    A, B, G = inputs(na, nb, D, 7 + D)
    spec = spec_of(name, D)
    At, Bt, Gt = T(A), T(B), T(G)
    both = ops.k_dense_vjp_points(spec, At, Bt, Gt)
    only_a = ops.k_dense_vjp_points(spec, At, Bt, Gt, need_dB=False)
    only_b = ops.k_dense_vjp_points(spec, At, Bt, Gt, need_dA=False)
    none = ops.k_dense_vjp_points(spec, At, Bt, Gt, need_dA=False, need_dB=False)
    assert only_a[3] is None and only_b[2] is None and none[2] is None and none[3] is None
    ref = check(name, spec, A, B, G, only_a, "dA only")
    check(name, spec, A, B, G, only_b, "dB only")
    check(name, spec, A, B, G, none, "scalars only")
    assert torch.equal(only_a[2], both[2]) and torch.equal(only_b[3], both[3])
    dv, dl = ops.k_dense_vjp(spec, At, Bt, Gt)
    assert excess(dv, ref["dv"], ref["sv"]) <= 1.0 and excess(np.array(dl), ref["dl"], ref["sl"]) <= 1.0


@pytest.mark.parametrize("name,D", [("se", 8), ("matern12", 3), ("matern32", 32), ("matern52", 33)])
def test_the_same_pointer_twice_with_a_non_symmetric_cotangent(name, D):
    from cggp import ops
    M = 130
    Z, _, G = inputs(M, M, D, 21 + D)
    spec = spec_of(name, D)
    Zt = T(Z)
    dv, dl, dA, dB = ops.k_dense_vjp_points(spec, Zt, Zt, T(G))
    ref = check(name, spec, Z, Z, G, (dv, dl, dA, dB), "A is B")
    both = excess((dA + dB).cpu().numpy(), ref["dA"] + ref["dB"], ref["sA"] + ref["sB"])
    print(f"dA + dB: {both:.2e}")
    assert both <= 1.0


@pytest.mark.parametrize("name", ["matern12", "matern52"])
@pytest.mark.parametrize("D", [3, 33])
def test_duplicated_rows_are_finite_and_add_exactly_nothing(name, D):
    """20 rows of B equal rows of A.  With the cotangent zero everywhere BUT on those pairs, dl, dA and dB are exactly
    0; with a full cotangent everything is finite and within the bar."""
    from cggp import ops
    na, nb, dup = 70, 65, 20
    A, B, G = inputs(na, nb, D, 5 + D, dup=dup)
    spec = spec_of(name, D)
    got = ops.k_dense_vjp_points(spec, T(A), T(B), T(G))
    check(name, spec, A, B, G, got, "duplicates")
    Gd = np.zeros_like(G)
    Gd[np.arange(dup), np.arange(dup)] = G[np.arange(dup), np.arange(dup)]
    dv, dl, dA, dB = ops.k_dense_vjp_points(spec, T(A), T(B), T(Gd))
    assert np.isfinite(dv) and dv != 0.0
    assert all(v == 0.0 for v in dl) and float(dA.abs().max()) == 0.0 and float(dB.abs().max()) == 0.0


# ---------------------------------------------------------------- 2. D > 32
@pytest.mark.parametrize("name", ["se", "matern32"])
@pytest.mark.parametrize("na,nb", [(1, 37), (65, 63), (130, 257)])
@pytest.mark.parametrize("D", [33, 48, 77, 512])
def test_above_32_dimensions_against_long_double(name, D, na, nb):
    from cggp import ops
    A, B, G = inputs(na, nb, D, D + na)
    spec = spec_of(name, D)
    check(name, spec, A, B, G, ops.k_dense_vjp_points(spec, T(A), T(B), T(G)), "any-D")


# ---------------------------------------------------------------- 3. seams
@pytest.mark.parametrize("name,D", [("matern32", 5), ("se", 32), ("matern52", 40)])
def test_panel_seams_agree_and_repeat_bit_for_bit(name, D):
    from cggp import ops
    na, nb = 100, 70
    A, B, G = inputs(na, nb, D, 31 + D)
    spec = spec_of(name, D)
    At, Bt, Gt = T(A), T(B), T(G)
    for rows in (0, 1, 32, 33, na - 1, na):
        a = ops.k_dense_vjp_points(spec, At, Bt, Gt, panel_rows=rows)
        b = ops.k_dense_vjp_points(spec, At, Bt, Gt, panel_rows=rows)
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        check(name, spec, A, B, G, a, f"panel_rows={rows}")


# ---------------------------------------------------------------- 4. the contract
def raw_call(hd, spec, A, na, B, nb, G, ldg, panel_rows, dA, dB, dv=True, dl=True, dtype=None):
    from cggp import _hip
    k = spec.struct(_hip.F64 if dtype is None else dtype)
    v, l = ctypes.c_double(0.0), (ctypes.c_double * _hip.MGP_MAX_D)()
    p = lambda g: None if g is None else ctypes.c_void_p(g.ptr if isinstance(g, Guarded) else g.data_ptr())
    rc = hd.lib.mgp_k_dense_vjp_points(hd.h, ctypes.byref(k), p(A), na, p(B), nb, p(G), ldg, panel_rows,
                                       ctypes.byref(v) if dv else None, l if dl else None, p(dA), p(dB))
    return rc, v.value, [l[d] for d in range(spec.D)]


@pytest.mark.parametrize("name,D", [("se", 5), ("matern12", 16), ("matern32", 32), ("matern52", 40)])
def test_guard_bands_stay_and_inputs_are_unchanged(name, D):
    from cggp import _hip
    na, nb, ldg = 133, 70, 75
    A, B, G = inputs(na, nb, D, 41 + D)
    Gw = np.zeros((na, ldg))
    Gw[:, :nb] = G
    up = lambda a: Guarded(a.shape, torch.float64, 1, DEV).upload(torch.from_numpy(np.ascontiguousarray(a)))
    gA, gB, gG = up(A), up(B), up(Gw)
    oA, oB = Guarded((na, D), torch.float64, 1, DEV), Guarded((nb, D), torch.float64, 1, DEV)
    hd = _hip.get_handle(DEV)
    spec = spec_of(name, D)
    rc, dv, dl = raw_call(hd, spec, gA, na, gB, nb, gG, ldg, 0, oA, oB)
    torch.cuda.synchronize()
    assert rc == 0
    for key, g in (("A", gA), ("B", gB), ("G", gG)):
        g.check_input(key)
    oA.check_output(None, "dA")
    oB.check_output(None, "dB")
    check(name, spec, A, B, G, (dv, dl, oA.payload, oB.payload), "guarded")


def test_empty_sides_shards_and_refusals():
    from cggp import _hip, ops
    na, nb, D = 601, 130, 5
    A, B, G = inputs(na, nb, D, 3)
    spec = spec_of("matern32", D)
    At, Bt, Gt = T(A), T(B), T(G)
    for a, b in ((At[:0], Bt), (At, Bt[:0])):
        g = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=DEV)
        dv, dl, dA, dB = ops.k_dense_vjp_points(spec, a, b, g)
        assert dv == 0.0 and dl == [0.0] * D and dA.shape == (a.shape[0], D) and dB.shape == (b.shape[0], D)
        assert float(dA.abs().sum()) == 0.0 and float(dB.abs().sum()) == 0.0
    whole = ops.k_dense_vjp_points(spec, At, Bt, Gt)
    s = 235  # uneven row shards add up to the whole
    p, q = ops.k_dense_vjp_points(spec, At[:s], Bt, Gt[:s]), ops.k_dense_vjp_points(spec, At[s:], Bt, Gt[s:])
    assert abs(p[0] + q[0] - whole[0]) <= 1e-12 * abs(whole[0])
    assert np.max(np.abs(np.add(p[1], q[1]) - whole[1])) <= 1e-12 * np.max(np.abs(whole[1]))
    assert float((p[3] + q[3] - whole[3]).abs().max()) <= 1e-12 * float(whole[3].abs().max())
    cat = torch.cat([p[2], q[2]])  # a row of dA sees all its columns in either call (the column blocks may differ)
    assert float((cat - whole[2]).abs().max()) <= 1e-12 * float(whole[2].abs().max())
    hd = _hip.get_handle(DEV)
    dA, dB = torch.empty((na, D), dtype=torch.float64, device=DEV), torch.empty((nb, D), dtype=torch.float64, device=DEV)
    assert raw_call(hd, spec, At, na, Bt, nb, Gt, nb, 0, dA, dB, dtype=_hip.F32)[0] == E_DTYPE
    assert raw_call(hd, spec, At, na, Bt, nb, Gt, nb - 1, 0, dA, dB)[0] == E_SHAPE
    assert raw_call(hd, spec, At, na, Bt, nb, Gt, nb, -1, dA, dB)[0] == E_SHAPE
    assert raw_call(hd, spec, At, na, Bt, nb, Gt, nb, 0, dA, dB, dv=False)[0] == E_BADARG
    assert raw_call(hd, spec, At, na, Bt, nb, Gt, nb, 0, dA, dB, dl=False)[0] == E_BADARG
    with pytest.raises(_hip.MgpError, match="fp64"):
        ops.k_dense_vjp_points(spec, At.float(), Bt.float(), Gt.float())
    with pytest.raises(ValueError, match="panel_rows"):
        ops.k_dense_vjp_points(spec, At, Bt, Gt, panel_rows=-1)
    with pytest.raises(ValueError, match="512"):
        ops.k_dense_vjp_points(spec_of("se", 513), T(np.zeros((2, 513))), T(np.zeros((2, 513))), T(np.zeros((2, 2))))


def header_bytes(na, nb, D, want_a, want_b, panel_rows=0, cus=256):
    """the scratch formula of include/mgp_points.h"""
    al = lambda x: (x + 255) // 256 * 256
    c = lambda x, y: -(-x // y)
    big = D > 32
    DP = next(p for p in (2, 4, 8, 16, 32) if p >= min(D, 32))
    W, S = (D, c(D, 32)) if big else (DP, 1)
    if big:
        R0 = min(max(16, min(2 ** 25 // nb, 2 ** 24 // D) // 16 * 16), 2 ** 21)
    else:
        R0 = 2 ** 24 // DP
    R = min(na, panel_rows or R0, 2 ** 21 if big else 1 << 62)
    Bb = max(1, min(c(4 * cus, c(nb, 256) * S), c(R, 32), 2 ** 24 // (nb * W) if want_b else 1 << 62))
    Ba = max(1, min(c(4 * cus, c(R, 256) * S), c(nb, 32), 2 ** 24 // (R * W)))
    total = (al(8 * Bb * nb * W) + al(8 * nb * W) if want_b else 0) + (al(8 * Ba * R * W) if want_a else 0)
    if big:
        return total + al(8 * Bb * c(nb, 256) * 32 * S) + al(8 * c(nb, 64) * c(R, 64)) + al(8 * (32 * S + 1)) \
            + (2 if want_a else 1) * al(8 * R * nb)
    return total + al(8 * Bb * c(nb, 256) * (DP + 1)) + al(8 * (DP + 1))


@pytest.mark.parametrize("D,want_a", [(5, True), (32, False), (40, True)])
def test_a_fixed_pool_of_the_headers_size_is_enough_and_one_byte_less_is_not(D, want_a):
    from cggp import _hip
    na, nb = 300, 130
    A, B, G = inputs(na, nb, D, 51)
    At, Bt, Gt = T(A), T(B), T(G)
    dA = torch.empty((na, D), dtype=torch.float64, device=DEV) if want_a else None
    dB = torch.empty((nb, D), dtype=torch.float64, device=DEV)
    lib = _hip.load_library()
    props = torch.cuda.get_device_properties(DEV)
    need = header_bytes(na, nb, D, want_a, True, cus=props.multi_processor_count)
    spec = spec_of("matern52", D)
    rcs = {}
    for size in (need - 1, need):
        h = ctypes.c_void_p()
        assert lib.mgp_create_ex(ctypes.byref(h), 0, size) == 0

        class Hd:
            pass
        hd = Hd()
        hd.lib, hd.h = lib, h
        try:
            rcs[size] = raw_call(hd, spec, At, na, Bt, nb, Gt, nb, 0, dA, dB)
            used = lib.mgp_workspace_bytes(h)
        finally:
            lib.mgp_destroy(h)
    assert rcs[need - 1][0] == E_NOMEM and rcs[need][0] == 0 and used == need
    check("matern52", spec, A, B, G, (rcs[need][1], rcs[need][2], dA, dB), "fixed pool")


def test_a_call_behind_an_unfinished_producer_on_a_side_stream():
    """the inputs are filled by copies queued behind ~20 matrix products of 4096^3 on the stream the call goes to"""
    from cggp import ops
    na, nb, D = 333, 130, 5
    A, B, G = inputs(na, nb, D, 61)
    staged = dict(A=T(A), B=T(B), G=T(G))
    bufs = {k: torch.full_like(v, float("nan")) for k, v in staged.items()}
    a = (torch.randn((4096, 4096), generator=torch.Generator().manual_seed(0)) / 64.0).to(DEV)
    b = torch.empty_like(a)
    side = torch.cuda.Stream(device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spec = spec_of("matern32", D)
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
        dv, dl, dA, dB = ops.k_dense_vjp_points(spec, bufs["A"], bufs["B"], bufs["G"])
        dA, dB = dA.clone(), dB.clone()
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= 5.0, "the producers were too short: the test proves nothing"
    check("matern32", spec, A, B, G, (dv, dl, dA, dB), "behind a producer")


# ---------------------------------------------------------------- 5. memory
def test_one_block_backward_holds_no_temporary_of_the_blocks_size(monkeypatch):
    """_KBlock forward and backward at na = nb = 2048, D = 32 with fused_point_grads=True, on a handle of its own whose
    fixed pool is exactly the header's formula for that call: the call succeeds, the handle has then used exactly that
    many bytes, all of them in the one arena -- and one byte less is MGP_E_NOMEM.  torch's peak grows by at most 8 MiB
    (dA and dB are 1 MiB together; the torch route holds several 128 MiB temporaries)."""
    import switch_forms
    from cggp import _hip, kernels
    from cggp.training import TrainableKernel
    M, D = 2048, 32
    A, B, G = inputs(M, M, D, 71)
    kern = TrainableKernel(kernels.Matern32(variance=1.2, lengthscales=list(np.linspace(0.8, 1.2, D) * np.sqrt(D))))
    At, Bt, Gt = T(A).requires_grad_(True), T(B).requires_grad_(True), T(G)
    need = header_bytes(M, M, D, True, True, cus=torch.cuda.get_device_properties(DEV).multi_processor_count)
    with switch_forms.switched(monkeypatch, {"MGP_WORKSPACE_BYTES": str(need)}) as hd:
        K = kern.K(At, Bt, fused_point_grads=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        K.backward(Gt)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        used, arena = hd.lib.mgp_workspace_bytes(hd.h), hd.lib.mgp_arena_bytes(hd.h, b"kgrad")
    print(f"torch peak grew by {grown / 2 ** 20:.2f} MiB; handle used {used} bytes, kgrad arena {arena}, formula {need} "
          f"({need / 2 ** 20:.1f} MiB)")
    assert grown <= 8 << 20
    assert At.grad.shape == (M, D) and Bt.grad.shape == (M, D)
    assert bool(torch.isfinite(At.grad).all()) and bool(torch.isfinite(Bt.grad).all())
    assert used == need and arena == need
    assert need < 8 * M * M * D // 8  # the formula itself: under an eighth of one [na, nb, D] temporary (256 MiB)
    with switch_forms.switched(monkeypatch, {"MGP_WORKSPACE_BYTES": str(need - 1)}) as hd:
        dA, dB = torch.empty_like(At.grad), torch.empty_like(Bt.grad)
        rc = raw_call(hd, spec_of("matern32", D), At.detach(), M, Bt.detach(), M, Gt, M, 0, dA, dB)[0]
    assert rc == E_NOMEM


# ---------------------------------------------------------------- 6. the models
def spy_on_the_torch_route(monkeypatch):
    from cggp import training
    calls = []
    for fn in ("k_grad_points", "kmm_grad_z"):
        orig = getattr(training, fn)
        monkeypatch.setattr(training, fn, lambda *a, _f=fn, _o=orig, **k: (calls.append(_f), _o(*a, **k))[1])
    return calls


@pytest.mark.parametrize("kind,D", [("se", 3), ("matern32", 33)])
def test_dense_cdgp_batch_form_against_the_reference(monkeypatch, kind, D):
    import test_gpu_cdgp_tip as tp
    from test_gpu_cdgp_matrix_free import probes_of, trainable
    calls = spy_on_the_torch_route(monkeypatch)
    want = tp.reference_loss_and_grads(kind, D, False)
    pr = probes_of(tp.M_MODEL, 5, 11)
    m, data = trainable(kind, D, tp.M_MODEL, tp.B_MODEL, False, trainable_inducing=True, fused_point_grads=True)
    got = tp.model_loss_and_grads(m, data, pr)
    assert calls == []
    tp.compare(f"{kind} D={D} dense, fused point gradients", got, want, D)
    m0, data0 = trainable(kind, D, tp.M_MODEL, tp.B_MODEL, False, trainable_inducing=True)
    off = tp.model_loss_and_grads(m0, data0, pr)
    assert off[0] == got[0] and calls != []  # the forward pass does not change; the default takes the torch route


@pytest.mark.parametrize("term", ["trace", "pathwise"])
def test_dense_cdgp_trace_and_pathwise_forms_against_their_references(monkeypatch, term):
    import test_gpu_cdgp_full as fl
    import test_gpu_cdgp_pathwise as pw
    from test_gpu_cdgp_matrix_free import probes_of
    kind, D, M, N = "matern32", 3, 200, 777
    calls = spy_on_the_torch_route(monkeypatch)
    pr = probes_of(M, 5, 11)
    out = {}
    for fused in (True, False):
        kw = dict(trainable_inducing=True, fused_point_grads=fused)
        if term == "trace":
            m, data = fl.make(kind, D, M, N, False, **kw)
            out[fused] = fl.loss_and_grads(m, data, pr)
        else:
            m, data = pw.make(kind, D, M, N, False, **kw)
            out[fused] = pw.loss_and_grads(m, data, pr, pw.draw_of(m, 7))
        if fused:
            assert calls == []
    want = fl.reference(kind, D, M, N, 5, 11) if term == "trace" else pw.reference(kind, D, M, N, 5, 11)
    fl.compare(f"{kind} D={D} {term}, fused point gradients", out[True], want, D)
    assert out[True][0] == out[False][0] and calls != []


@pytest.mark.parametrize("name,D", [("se", 3), ("matern32", 33)])
def test_trainable_sgpr_against_the_explicit_bound(monkeypatch, name, D):
    from cggp import training
    from sgpr_grad_reference import sgpr_elbo_explicit
    from test_gpu_sgpr_train import _kernel, _sgpr_problem
    calls = spy_on_the_torch_route(monkeypatch)
    X, Y, Z = _sgpr_problem(D=D)
    if D > 3:  # that file's lengthscales are for 3 dimensions: keep the scaled distances where they are there
        from cggp import kernels
        ls = list(np.linspace(0.8, 1.2, D) * np.sqrt(D / 3.0))
        _kernel = lambda name, D: {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[name](
            variance=1.2, lengthscales=ls)
    m = training.TrainableSGPR(_kernel(name, D), 0.3, T(X), T(Y), T(Z), trainable_inducing=True, fused_point_grads=True)
    from cggp import ops
    dense, orig = [], ops.k_dense_vjp
    monkeypatch.setattr(ops, "k_dense_vjp", lambda *a, **k: (dense.append(1), orig(*a, **k))[1])
    loss = m.training_loss()
    loss.backward()
    assert calls == [] and dense == []  # K_mm's hyper-parameter sums and its dZ come from the one fused call
    ps = m.parameters()
    got = [ps[0].grad, ps[1].grad, ps[2].grad, ps[3].grad.cpu()]
    raws = [p.detach().cpu().clone().requires_grad_() for p in ps]
    f = torch.nn.functional.softplus
    cpu = lambda a: torch.tensor(a, dtype=torch.float64)
    val = -sgpr_elbo_explicit(name, f(raws[0])[0], f(raws[1]), f(raws[2])[0], cpu(X), cpu(Y), raws[3], 1e-6)
    want = torch.autograd.grad(val, raws)
    for g, w in zip(got, want):
        d = float((g - w).abs().max()) / float(w.abs().max())
        print(f"sgpr {name} D={D}: {d:.2e} (bar 1e-7)")
        assert d <= 1e-7
    m0 = training.TrainableSGPR(_kernel(name, D), 0.3, T(X), T(Y), T(Z), trainable_inducing=True)
    loss0 = m0.training_loss()
    loss0.backward()
    assert float(loss0.detach()) == float(loss.detach()) and "kmm_grad_z" in calls and len(dense) >= 1


def test_adam_and_lbfgs_run_with_fused_point_gradients(monkeypatch):
    from cggp import training
    from test_gpu_cdgp_matrix_free import trainable
    from test_gpu_sgpr_train import _kernel, _sgpr_problem
    calls = spy_on_the_torch_route(monkeypatch)
    m, data = trainable("se", 4, 200, 50, False, trainable_inducing=True, fused_point_grads=True)
    z0 = m.Z.detach().clone()
    losses = training.train_using_adam_and_update(data, m, 1, 50, 0.05)
    assert len(losses) == 1 and np.all(np.isfinite(losses)) and float((m.Z.detach() - z0).abs().max()) > 0.0
    res = training.train_using_lbfgs_and_update(data, m, 2)
    assert res is not None and np.isfinite(res.fun) and bool(torch.isfinite(m.Z).all())
    X, Y, Z = _sgpr_problem(seed=9)
    s = training.TrainableSGPR(_kernel("matern32", 3), 0.5, T(X), T(Y), T(Z), trainable_inducing=True,
                               fused_point_grads=True)
    losses = training.train_using_adam_and_update(None, s, iterations=1, batch_size=None, learning_rate=0.05)
    assert np.all(np.isfinite(losses))
    training.train_using_lbfgs_and_update((s.X, s.Y), s, 2)
    assert np.isfinite(float(s.training_loss())) and bool(torch.isfinite(s.Z).all())
    assert calls == []
