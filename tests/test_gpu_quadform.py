"""mgp_knm_quadform (include/mgp_predict.h, csrc/quadform.hip) on the GPU: values against long double on every seam of
the plan (tests/quadform_plan.py), the region of C that is never read, the generic route (fp32, D = 33), bit-identity,
the buffer contract and the scratch rule.

The bound, derived in tests/quadform_reference.py: |q - q*| <= (2 eps_b + (M + 4) u) mag_b, mag_b = |k|^T |C_upper form| |k|
the form with absolute values, eps_b the per-pair relative bound of `pair_reference.pair_bound` for the expansion-form
distance maximised over the row's pairs (2 eps: every term holds two kernel values), u the unit roundoff; (M + 4) u is
the first-order bound of a sum whose terms pass through at most M + 4 roundings (the accumulation of column j over the
rows i < j, the two fused multiply-adds that add C_jj k_j and multiply by k_j, the scale).  The docstring there also
says what that count leaves out.  Every test prints the worst err / bound it saw.

Shapes.  One set of test rows [2 t + 3, D], inducing points [3 c + 5, D] and matrices [3 c + 5, 3 c + 5] per kernel
kind and dimension; every smaller case is a leading block of it (the long-double forms of all leading blocks come from
one product, `quadform_reference.prefix_forms`), passed as a row-major view with ldc = 3 c + 5 > M."""

import contextlib
import ctypes

import numpy as np
import pytest
import torch

import buffer_contract as bc
import pair_reference as pr
import quadform_plan as qp
import quadform_reference as qr

pytestmark = pytest.mark.gpu

LD = np.longdouble
VAR = pr.VARIANCE
BMAX, MMAX = max(qp.B_VALUES), max(qp.M_VALUES)
NP = {"f64": np.float64, "f32": np.float32}
TORCH = {"f64": torch.float64, "f32": torch.float32}


def dev():
    return torch.device("cuda:0")


def T(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev())


def spec_of(name, D, ls=None):
    from cggp import ops
    return ops.KernelSpec(name, VAR, list(pr.lengthscales(D) if ls is None else ls), D)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def report(what, worst):
    print(f"quadform {what}: worst err / bound {worst:.3f}")


@contextlib.contextmanager
def fresh_handle(pool=0):
    """A handle nothing else has touched; pool > 0: a fixed workspace of that many bytes."""
    from cggp import _hip
    lib = _hip.load_library()
    h = ctypes.c_void_p()
    assert lib.mgp_create_ex(ctypes.byref(h), 0, pool) == 0
    lib.mgp_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    try:
        yield lib, h
    finally:
        torch.cuda.synchronize()
        lib.mgp_destroy(h)


def raw(lib, h, k, Xs, B, Z, M, C, ldc, q):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else (0 if t is None else t.data_ptr()))
    return lib.mgp_knm_quadform(h, ctypes.byref(k) if k is not None else None, p(Xs), B, p(Z), M, p(C), ldc, p(q))


# ---------------------------------------------------------------- the shared reference
_REF = {}


def matrices(M, seed):
    """C = G G^T / M + diag (positive definite) and one indefinite matrix (its diagonal negated, signs of a third of
    the off-diagonal entries flipped symmetrically)."""
    rng = np.random.default_rng([11, M, seed])
    G = rng.standard_normal((M, M))
    spd = G @ G.T / M + np.diag(0.5 + rng.random(M))
    flip = np.triu(rng.random((M, M)) < 1.0 / 3.0, 1)
    sign = np.where(flip | flip.T, -1.0, 1.0)
    indef = spd * sign - 2.0 * np.diag(np.diag(spd))
    return {"spd": spd, "indefinite": indef}


def reference(name, D, dt="f64"):
    """Points, matrices and the long-double forms of every leading block, computed once per (kind, D, dtype)."""
    key = (name, D, dt)
    if key not in _REF:
        rng = np.random.default_rng([5, D, pr.KINDS.index(name)])
        ls = pr.lengthscales(D)
        Xs = (1.2 * rng.standard_normal((BMAX, D)) / np.sqrt(D)).astype(NP[dt])
        Z = (1.2 * rng.standard_normal((MMAX, D)) / np.sqrt(D)).astype(NP[dt])
        Z[5], Z[MMAX - 1] = Xs[0], Xs[BMAX - 1]  # coincident points: k = variance, the Matern cusp
        pv = pr.pair_values(name, VAR, ls, Xs, Z)
        eps = qr.row_eps(name, VAR, ls, Xs.astype(np.float64), Z.astype(np.float64), pv, NP[dt])
        forms = {}
        for label, C in matrices(MMAX, D).items():
            C = C.astype(NP[dt])
            forms[label] = (C,) + qr.prefix_forms(pv.k, C)
        _REF[key] = (ls, Xs, Z, eps, forms)
    return _REF[key]


def worst_ratio(got, B, M, eps, Q, MAG, dt):
    got = np.asarray(got)
    assert got.shape == (B,) and np.all(np.isfinite(got)), got
    if M == 0:
        assert not got.any()
        return 0.0
    err = np.abs(got.astype(LD) - Q[:B, M - 1])
    bound = qr.bound(eps[:B, M - 1], M, MAG[:B, M - 1], NP[dt])
    return float(np.max(err / bound))


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("D", qp.DIMS)
@pytest.mark.parametrize("name", qp.KINDS)
def test_values_against_long_double(name, D):
    """Every M in {1, c-1, c, c+1, 2c, 3c+5} with every B in {1, t-1, t+1, 2t+3}, both matrices, on the fused route."""
    from cggp import ops
    ls, Xs, Z, eps, forms = reference(name, D)
    spec = spec_of(name, D, ls)
    xs, z = T(Xs), T(Z)
    worst = 0.0
    for label, (C, Q, MAG) in forms.items():
        c = T(C)
        for M in qp.M_VALUES:
            for B in qp.B_VALUES:
                got = ops.knm_quadform(spec, xs[:B], z[:M], c[:M, :M]).cpu().numpy()
                r = worst_ratio(got, B, M, eps, Q, MAG, "f64")
                assert r <= 1.0, (label, M, B, r)
                worst = max(worst, r)
    report(f"{name} D={D}", worst)


def test_more_than_one_chunk_of_test_rows():
    """B = CHUNK_B + t + 1: two launches, the second with its own row offset; rows repeat, so must the results."""
    from cggp import ops
    name, D, M = "matern52", 3, qp.C + 1
    ls, Xs, Z, eps, forms = reference(name, D)
    C, Q, MAG = forms["spd"]
    B = qp.CHUNK_B + qp.T + 1
    assert len(qp.grid(B, M)) == 2
    idx = np.arange(B) % BMAX
    got = ops.knm_quadform(spec_of(name, D, ls), T(Xs[idx]), T(Z[:M]), T(C)[:M, :M]).cpu().numpy()
    one = got[:BMAX]
    report("two chunks", worst_ratio(one, BMAX, M, eps, Q, MAG, "f64"))
    assert worst_ratio(one, BMAX, M, eps, Q, MAG, "f64") <= 1.0
    assert np.array_equal(got, one[idx])


# ---------------------------------------------------------------- the generic route
def test_fp32_takes_the_generic_route_against_long_double():
    from cggp import ops
    name, D = "matern32", 8
    ls, Xs, Z, eps, forms = reference(name, D, "f32")
    spec = spec_of(name, D, ls)
    worst = 0.0
    for label, (C, Q, MAG) in forms.items():
        c = T(C, np.float32)
        for M, B in ((1, 1), (qp.C - 1, qp.T + 1), (qp.C + 1, qp.T - 1), (MMAX, BMAX)):
            got = ops.knm_quadform(spec, T(Xs, np.float32)[:B], T(Z, np.float32)[:M], c[:M, :M])
            assert got.dtype == torch.float32
            r = worst_ratio(got.cpu().numpy(), B, M, eps, Q, MAG, "f32")
            assert r <= 1.0, (label, M, B, r)
            worst = max(worst, r)
    report("fp32 generic", worst)


def test_d33_takes_the_generic_route_to_the_same_bound():
    """D = 33 > MGP_FUSED_MAX_D: panels by direct differences, held to the bound of the fused (expansion-form) arithmetic."""
    from cggp import _hip, ops
    name, D = "se", 33
    ls, Xs, Z, eps, forms = reference(name, D)
    spec = spec_of(name, D, ls)
    worst = 0.0
    for label, (C, Q, MAG) in forms.items():
        for M, B in ((qp.C + 1, qp.T + 1), (MMAX, BMAX)):
            with fresh_handle() as (lib, h):
                q = torch.empty((B,), dtype=torch.float64, device=dev())
                c = T(C)[:M, :M].contiguous()
                assert raw(lib, h, spec.struct(_hip.F64), T(Xs)[:B], B, T(Z)[:M], M, c, M, q) == 0, lib.mgp_last_error(h)
                torch.cuda.synchronize()
                # the route: the arena holds the symmetric matrix and two panels, not the fused partials
                assert lib.mgp_arena_bytes(h, b"prj") == qp.reserved(qp.generic_scratch_bytes(B, M, 8))
                # M < 512: the GEMM has no contraction slices; mgp_k_dense takes no scratch at D = 33
                assert qp.gemm_slices_bound(B, M, 8, cus()) == 0 and lib.mgp_arena_bytes(h, b"ws") == 0
                assert lib.mgp_arena_bytes(h, b"gen") == 0
            assert torch.equal(q, ops.knm_quadform(spec, T(Xs)[:B], T(Z)[:M], c))
            r = worst_ratio(q.cpu().numpy(), B, M, eps, Q, MAG, "f64")
            assert r <= 1.0, (label, M, B, r)
            worst = max(worst, r)
    report("D=33 generic", worst)


ROUTES = [pytest.param("se", 8, "f64", id="fused"), pytest.param("matern32", 8, "f32", id="generic-f32"),
          pytest.param("se", 33, "f64", id="generic-d33")]


# ---------------------------------------------------------------- the unread region, bit-identity
@pytest.mark.parametrize("name,D,dt", ROUTES)
def test_unread_region_and_bit_identity(name, D, dt):
    """NaN in every entry below the diagonal and in the columns M ... ldc-1 (ldc = M + 3) gives the bits of a clean
    symmetric C with zeros there; two calls give the same bits."""
    from cggp import _hip
    ls, Xs, Z, eps, forms = reference(name, D, dt)
    C, Q, MAG = forms["indefinite"]
    M, B, ldc = MMAX, BMAX, MMAX + 3
    clean = np.zeros((M, ldc), dtype=NP[dt])
    clean[:, :M] = C
    dirty = clean.copy()
    dirty[np.tril_indices(M, -1)] = np.nan
    dirty[:, M:] = np.nan
    assert np.isnan(dirty).sum() == M * (M - 1) // 2 + 3 * M
    k = spec_of(name, D, ls).struct(_hip.F64 if dt == "f64" else _hip.F32)
    hd = _hip.get_handle(dev())
    xs, z = T(Xs, NP[dt]), T(Z, NP[dt])
    outs = []
    for Cm in (clean, dirty, dirty):
        q = torch.full((B,), float("nan"), dtype=TORCH[dt], device=dev())
        hd.check(raw(hd.lib, hd.h, k, xs, B, z, M, T(Cm, NP[dt]), ldc, q))
        torch.cuda.synchronize()
        outs.append(q)
    assert worst_ratio(outs[0].cpu().numpy(), B, M, eps, Q, MAG, dt) <= 1.0
    iv = torch.int64 if dt == "f64" else torch.int32
    assert torch.equal(outs[0].view(iv), outs[1].view(iv)), "the unread region reached the result"
    assert torch.equal(outs[1].view(iv), outs[2].view(iv)), "two calls differ"


# ---------------------------------------------------------------- the buffer contract
@pytest.mark.parametrize("name,D,dt", ROUTES)
def test_guards_inputs_and_offset_bases(name, D, dt):
    """Guard bands round q untouched, every element of q written, inputs bit for bit as uploaded, all bases one element
    past a 16-byte boundary; the result is the right one and the one of aligned bases."""
    from cggp import _hip, ops
    ls, Xs, Z, eps, forms = reference(name, D, dt)
    C, Q, MAG = forms["spd"]
    M, B = 2 * qp.C + 1, qp.T + 1
    Cm = np.ascontiguousarray(C[:M, :M])
    k = spec_of(name, D, ls).struct(_hip.F64 if dt == "f64" else _hip.F32)
    td = TORCH[dt]
    gX = bc.guarded((B, D), td, 1, dev())[1].upload(torch.from_numpy(Xs[:B].copy()))
    gZ = bc.guarded((M, D), td, 1, dev())[1].upload(torch.from_numpy(Z[:M].copy()))
    gC = bc.guarded((M, M), td, 1, dev())[1].upload(torch.from_numpy(Cm))
    gQ = bc.guarded((B,), td, 1, dev())[1]
    hd = _hip.get_handle(dev())
    hd.check(raw(hd.lib, hd.h, k, gX.ptr, B, gZ.ptr, M, gC.ptr, M, gQ.ptr))
    torch.cuda.synchronize()
    for g, label in ((gX, "Xs"), (gZ, "Z"), (gC, "C")):
        g.check_input(label)
    gQ.check_output(None, "q")
    assert worst_ratio(gQ.payload.cpu().numpy(), B, M, eps, Q, MAG, dt) <= 1.0
    aligned = ops.knm_quadform(spec_of(name, D, ls), T(Xs[:B], NP[dt]), T(Z[:M], NP[dt]), T(Cm, NP[dt]))
    assert worst_ratio(aligned.cpu().numpy(), B, M, eps, Q, MAG, dt) <= 1.0
    if dt == "f64" and D <= qp.FUSED_MAX_D:
        # the fused kernels use no load wider than an element; the generic route's GEMM picks its loads by alignment
        assert torch.equal(aligned, gQ.payload), "the result depends on the base address"


@pytest.mark.parametrize("name,D,dt", ROUTES)
def test_stale_arena_does_not_reach_the_result(name, D, dt):
    """clean, then a larger call on NaN inputs in the same dtype (it writes the whole arena the clean call reads) and a
    call in the other dtype, then clean again: the same bits."""
    from cggp import _hip
    ls, Xs, Z, eps, forms = reference(name, D, dt)
    C, _, _ = forms["spd"]
    M, B = qp.C + 1, qp.T + 1
    other = "f32" if dt == "f64" else "f64"
    code = {"f64": _hip.F64, "f32": _hip.F32}
    spec = spec_of(name, D, ls)

    def run(lib, h, d, B_, M_, poison):
        xs, z, c = T(Xs[:B_], NP[d]), T(Z[:M_], NP[d]), T(C[:M_, :M_], NP[d])
        if poison:
            xs, z, c = (torch.full_like(t, float("nan")) for t in (xs, z, c))
        q = torch.empty((B_,), dtype=TORCH[d], device=dev())
        assert raw(lib, h, spec.struct(code[d]), xs, B_, z, M_, c, M_, q) == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
        return q

    with fresh_handle() as (lib, h):
        first = run(lib, h, dt, B, M, False)
        held = lib.mgp_arena_bytes(h, b"prj")
        assert held > 0
        run(lib, h, dt, BMAX, MMAX, True)
        run(lib, h, other, BMAX, MMAX, True)
        assert lib.mgp_arena_bytes(h, b"prj") > held
        third = run(lib, h, dt, B, M, False)
    assert torch.equal(first, third) and bool(torch.isfinite(first).all())


def _delay():
    """~20 matmuls of 4096^3 on the current stream; the two events that bracket them"""
    g = torch.Generator(device="cpu").manual_seed(0)
    a = (torch.randn((4096, 4096), generator=g) / 64.0).to(dev())
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    x = a
    for _ in range(10):
        torch.matmul(x, a, out=b)
        x = torch.matmul(b, a)
    e1.record()
    return e0, e1


def test_call_enqueued_behind_unfinished_producers():
    """On a side stream behind ~20 large matmuls: copies that overwrite sentinel-filled inputs with the real ones, the
    call, a clone of q; one synchronisation at the end.  A read ahead of the stream order sees NaN."""
    from cggp import ops
    name, D = "matern32", 8
    ls, Xs, Z, eps, forms = reference(name, D)
    C, Q, MAG = forms["spd"]
    M, B = 2 * qp.C + 1, qp.T + 1
    vals = [T(Xs[:B]), T(Z[:M]), T(np.ascontiguousarray(C[:M, :M]))]
    bufs = [bc.guarded(v.shape, torch.float64, 0, dev())[1].expect(v) for v in vals]
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0, e1 = _delay()
        for g, v in zip(bufs, vals):
            g.payload.copy_(v, non_blocking=True)
        q = ops.knm_quadform(spec_of(name, D, ls), *[g.payload for g in bufs]).clone()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"producers ran for {ms:.1f} ms")
    assert ms >= 5.0, f"the producers ran for {ms:.2f} ms only: the test proves nothing"
    for g in bufs:
        g.check_input()
    assert worst_ratio(q.cpu().numpy(), B, M, eps, Q, MAG, "f64") <= 1.0


@pytest.mark.parametrize("name,D,dt", ROUTES)
def test_empty_inputs_and_refusals(name, D, dt):
    """B = 0 writes nothing, M = 0 writes zeros, ldc < M and NULL q are refused with q untouched."""
    from cggp import _hip, ops
    ls, Xs, Z, eps, forms = reference(name, D, dt)
    C, _, _ = forms["spd"]
    spec, td, nd = spec_of(name, D, ls), TORCH[dt], NP[dt]
    k = spec.struct(_hip.F64 if dt == "f64" else _hip.F32)
    hd = _hip.get_handle(dev())
    M, B = 5, 7
    xs, z, c = T(Xs[:B], nd), T(Z[:M], nd), T(C[:M, :M], nd)
    gQ = bc.guarded((B,), td, 0, dev())[1]
    assert raw(hd.lib, hd.h, k, xs, 0, z, M, c, M, gQ.ptr) == 0  # B = 0
    torch.cuda.synchronize()
    gQ.check_output(np.zeros(B, dtype=bool), "q at B = 0")
    assert raw(hd.lib, hd.h, k, xs, B, z, M, c, M - 1, gQ.ptr) == -1  # ldc < M: MGP_E_BADARG
    assert raw(hd.lib, hd.h, k, xs, B, z, M, c, M, None) == -1  # NULL q
    assert raw(hd.lib, hd.h, None, xs, B, z, M, c, M, gQ.ptr) == -1  # NULL kernel
    torch.cuda.synchronize()
    gQ.check_output(np.zeros(B, dtype=bool), "q after refused calls")
    assert raw(hd.lib, hd.h, k, xs, B, None, 0, None, 0, gQ.ptr) == 0  # M = 0: zeros
    torch.cuda.synchronize()
    gQ.check_output(None, "q at M = 0")
    assert not gQ.payload.any()
    assert tuple(ops.knm_quadform(spec, xs[:0], z, c).shape) == (0,)
    zero = ops.knm_quadform(spec, xs, z[:0], c[:0, :0])
    assert zero.dtype == td and torch.equal(zero, torch.zeros((B,), dtype=td, device=dev()))


# ---------------------------------------------------------------- scratch
@pytest.mark.parametrize("B,M,D", [(2 * qp.T + 3, 3 * qp.C + 5, 8), (qp.T - 1, qp.C + 1, 17)])
def test_scratch_is_the_headers_formula_in_one_arena(B, M, D):
    """A fresh handle holds the "prj" arena alone, sized by the header's formula (as `mgp_reserve` rounds it); a fixed
    pool of exactly the formula serves the call with the same bits; one byte less is MGP_E_NOMEM with q untouched."""
    from cggp import _hip
    name = "matern52"
    ls, Xs, Z, eps, forms = reference(name, D)
    C, Q, MAG = forms["spd"]
    k = spec_of(name, D, ls).struct(_hip.F64)
    xs, z, c = T(Xs[:B]), T(Z[:M]), T(np.ascontiguousarray(C[:M, :M]))
    need = qp.scratch_bytes(B, M, D)
    with fresh_handle() as (lib, h):
        q0 = torch.empty((B,), dtype=torch.float64, device=dev())
        assert raw(lib, h, k, xs, B, z, M, c, M, q0) == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
        assert lib.mgp_arena_bytes(h, b"prj") == qp.reserved(need)
        for other in (b"ws", b"cg", b"opws", b"kxx", b"kgrad", b"pch", b"gen", b"pack"):
            assert lib.mgp_arena_bytes(h, other) == 0, other
        assert lib.mgp_workspace_bytes(h) >= lib.mgp_arena_bytes(h, b"prj")
    assert worst_ratio(q0.cpu().numpy(), B, M, eps, Q, MAG, "f64") <= 1.0
    with fresh_handle(pool=need) as (lib, h):
        q1 = torch.empty((B,), dtype=torch.float64, device=dev())
        assert raw(lib, h, k, xs, B, z, M, c, M, q1) == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
        assert lib.mgp_workspace_bytes(h) == need
    assert torch.equal(q0, q1)
    with fresh_handle(pool=need - 1) as (lib, h):
        gQ = bc.guarded((B,), torch.float64, 0, dev())[1]
        assert raw(lib, h, k, xs, B, z, M, c, M, gQ.ptr) == -6  # MGP_E_NOMEM
        torch.cuda.synchronize()
        gQ.check_output(np.zeros(B, dtype=bool), "q after MGP_E_NOMEM")


@pytest.mark.parametrize("D,dt", [(8, "f32"), (33, "f64")])
def test_generic_route_scratch_is_two_arenas(D, dt):
    """M = 640 >= 512, where the NT GEMM of the generic route may cut its contraction into slices: "prj" holds the
    header's formula exactly, "ws" at most the header's slice bound, "gen" nothing; a fixed pool of the two together
    serves the call with the same bits; a pool one byte short of the first arena is MGP_E_NOMEM with q untouched."""
    from cggp import _hip
    B, M, elem = 300, 640, 4 if dt == "f32" else 8
    rng = np.random.default_rng([17, D])
    ls = pr.lengthscales(D)
    xs = T(1.2 * rng.standard_normal((B, D)) / np.sqrt(D), NP[dt])
    z = T(1.2 * rng.standard_normal((M, D)) / np.sqrt(D), NP[dt])
    G = rng.standard_normal((M, M))
    c = T(G @ G.T / M + np.eye(M), NP[dt])
    k = spec_of("matern52", D, ls).struct(_hip.F32 if dt == "f32" else _hip.F64)
    prj = qp.generic_scratch_bytes(B, M, elem)
    ws_bound = qp.gemm_slices_bound(qp.generic_panel_rows(B, M, elem), M, elem, cus())
    assert ws_bound > 0
    with fresh_handle() as (lib, h):
        q0 = torch.empty((B,), dtype=TORCH[dt], device=dev())
        assert raw(lib, h, k, xs, B, z, M, c, M, q0) == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
        ws = lib.mgp_arena_bytes(h, b"ws")
        print(f"generic {dt} D={D}: prj {lib.mgp_arena_bytes(h, b'prj')}, ws {ws} (bound {qp.reserved(ws_bound)})")
        assert lib.mgp_arena_bytes(h, b"prj") == qp.reserved(prj)
        assert ws <= qp.reserved(ws_bound)
        for other in (b"gen", b"cg", b"opws", b"kxx", b"kgrad", b"pch", b"pack"):
            assert lib.mgp_arena_bytes(h, other) == 0, other
    # against the composition in fp64
    from cggp import ops
    spec64 = spec_of("matern52", D, ls)
    K = ops.k_dense(spec64, xs.double(), z.double())
    Cu = torch.triu(c.double())
    S = Cu + torch.triu(c.double(), 1).t()
    want = ((K @ S) * K).sum(dim=1)
    assert float((q0.double() - want).abs().max() / want.abs().max()) < (1e-4 if dt == "f32" else 1e-12)
    with fresh_handle(pool=((prj + 255) & ~255) + ws_bound) as (lib, h):
        q1 = torch.empty((B,), dtype=TORCH[dt], device=dev())
        assert raw(lib, h, k, xs, B, z, M, c, M, q1) == 0, lib.mgp_last_error(h)
        torch.cuda.synchronize()
    assert torch.equal(q0, q1)
    with fresh_handle(pool=prj - 1) as (lib, h):
        gQ = bc.guarded((B,), TORCH[dt], 0, dev())[1]
        assert raw(lib, h, k, xs, B, z, M, c, M, gQ.ptr) == -6  # MGP_E_NOMEM
        torch.cuda.synchronize()
        gQ.check_output(np.zeros(B, dtype=bool), "q after MGP_E_NOMEM")
