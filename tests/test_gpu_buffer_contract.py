"""What every entry point of include/*.h does to the memory it is handed (tests/contract_table.py has one row per
entry point; tests/buffer_contract.py the guard-banded buffers).

A. every case with all device pointers 16-byte aligned, then all of them one element past a 16-byte boundary: both runs
   meet the existing reference at the existing bar, write exactly the documented region of every output between
   untouched 64 KiB guard bands, leave every input bit for bit as uploaded, and agree bit for bit with each other
   unless the row says a host dispatch reads a pointer value (then the route taken is printed).
B. a fresh handle runs the case, then the same entry point on NaN inputs in the same dtype (the same route: it writes
   every arena the case reads, which `mgp_arena_bytes` attests) and in the other dtype (or a larger finite problem
   where NaN has no meaning), then the case again: the third result is the first, bit for bit.
C. on a side stream, behind a chain of matmuls that keeps it busy for >= 5 ms: copies that overwrite sentinel-filled
   inputs with the real ones, the call, clones of the outputs; one synchronisation at the end.  A read ahead of the
   stream order sees NaN."""

import ctypes
import os

import numpy as np
import pytest
import torch

import contract_table as ct
from buffer_contract import Guarded
from cggp import _hip

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH = {"f64": torch.float64, "f32": torch.float32}
OTHER = {"f64": "f32", "f32": "f64"}
MIN_DELAY_MS = 5.0

CASES = [pytest.param(r, ci, dt, id=f"{r.name[4:]}-{ci}-{dt}") for r in ct.TABLE for ci in range(len(r.cases))
         for dt in r.dtypes]


def _handle_with(env):
    lib = _hip.load_library()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    h = ctypes.c_void_p()
    try:
        assert lib.mgp_create_ex(ctypes.byref(h), 0, 0) == 0
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return lib, h


@pytest.fixture(scope="module")
def handle():
    """a handle of this module's own; MGP_KXX=sym so that mgp_kxx_matvec and MGP_OP_KXX_NOISE run csrc/kxx.hip at
    these sizes (the default routes N < 2^16 to the sweep, which mgp_knm_matvec covers)"""
    lib, h = _handle_with({"MGP_KXX": "sym"})
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


@pytest.fixture(scope="module")
def aside_handle():
    """MGP_SGPR_KMM_ASIDE=2: the s2 Kmm p product of a one-column SGPR application always forks onto the aside stream"""
    lib, h = _handle_with({"MGP_SGPR_KMM_ASIDE": "2"})
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


def _tensor(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if t.dtype == torch.int64 else t.to(TORCH[dt])


_DELAY = {}


def _delay():
    """~20 matmuls of 4096^3 on the current stream; returns the two events that bracket them"""
    if not _DELAY:
        g = torch.Generator(device="cpu").manual_seed(0)
        _DELAY["a"] = (torch.randn((4096, 4096), generator=g) / 64.0).to(DEV)
        _DELAY["b"] = torch.empty_like(_DELAY["a"])
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a, b = _DELAY["a"], _DELAY["b"]
    e0.record()
    x = a
    for _ in range(10):
        torch.matmul(x, a, out=b)
        x = torch.matmul(b, a)
    e1.record()
    return e0, e1


class Run:
    """One call of a row's entry point on guard-banded buffers."""

    def __init__(self, row, c, dt, offset, ins=None):
        self.row, self.c, self.dt = row, c, dt
        self.ins = ct.build_inputs(row, c, dt) if ins is None else ins
        self.gin, self.gout, self.host, self.delay_ms = {}, {}, {}, None
        self.values = {k: _tensor(v, dt) for k, v in self.ins.items() if not k.startswith("_")}
        for k, v in self.values.items():
            self.gin[k] = Guarded(v.shape, v.dtype, offset, DEV)
        for k, (shape, kind) in row.outs(c, dt).items():
            self.gout[k] = Guarded(shape, torch.int64 if kind == "i64" else TORCH[dt], offset, DEV)

    def pointers(self):
        p = {k: v for k, v in self.ins.items() if k.startswith("_")}
        for k, g in list(self.gin.items()) + list(self.gout.items()):
            p[k] = ctypes.c_void_p(g.ptr)
        return p

    def addresses(self):
        return {k: g.ptr for k, g in list(self.gin.items()) + list(self.gout.items())}

    def _call(self, lib, h, stream):
        lib.mgp_set_stream(h, ctypes.c_void_p(stream.cuda_stream))
        rc, self.host = self.row.call(lib, h, self.c, self.dt, self.pointers())
        assert rc == 0, (self.row.name, self.c, self.dt, rc, lib.mgp_last_error(h))

    def sync(self, lib, h):
        """upload, synchronise, call on the current stream, synchronise"""
        for k, g in self.gin.items():
            g.upload(self.values[k])
        torch.cuda.synchronize()
        self._call(lib, h, torch.cuda.current_stream(DEV))
        torch.cuda.synchronize()
        self.got = {k: g.payload.clone() for k, g in self.gout.items()}
        return self

    def behind_producers(self, lib, h, side):
        """everything enqueued on `side` behind a busy stream; the inputs hold the sentinel until their copy runs"""
        staged = {k: v.to(DEV) for k, v in self.values.items()}
        for k, g in self.gin.items():
            g.expect(staged[k])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            e0, e1 = _delay()
            for k, g in self.gin.items():
                g.payload.copy_(staged[k], non_blocking=True)
            self._call(lib, h, side)
            self.got = {k: g.payload.clone() for k, g in self.gout.items()}
        torch.cuda.synchronize()  # the one synchronisation
        self.delay_ms = e0.elapsed_time(e1)
        return self

    def results(self):
        got = {k: v.cpu().numpy() for k, v in self.got.items()}
        got.update(self.host)
        return got

    def check(self, ref):
        """the reference bar, then the written / untouched regions and guards of every output, then every input"""
        written = self.row.check(self.c, self.dt, self.ins, self.results(), ref)
        assert set(written) == set(self.gout), (self.row.name, sorted(written), sorted(self.gout))
        for k, g in self.gout.items():
            g.check_output(written[k], name=f"{self.row.name} {k}")
        for k, g in self.gin.items():
            g.check_input(name=f"{self.row.name} {k}")

    def same_bits(self, other):
        for k in self.got:
            a, b = self.got[k], other.got[k]
            if not torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int64),
                               b.view(torch.int32 if b.element_size() == 4 else torch.int64)):
                return False
        for k, v in self.host.items():
            if not np.array_equal(np.asarray(v), np.asarray(other.host[k])):
                return False
        return True


# ---------------------------------------------------------------------------------------------------- family A
@pytest.mark.parametrize("row,ci,dt", CASES)
def test_guards_full_write_input_preservation_at_both_alignments(handle, row, ci, dt):
    lib, h = handle
    c = row.cases[ci]
    ref = ct.reference(row, ci, dt)
    runs = []
    for offset in (0, 1):
        r = Run(row, c, dt, offset).sync(lib, h)
        if row.reads_pointer(c, dt):
            print(f"{row.name} {c} {dt} offset {offset}: {row.route(c, dt, r.addresses())}")
        r.check(ref)
        runs.append(r)
    if not row.reads_pointer(c, dt):
        assert runs[0].same_bits(runs[1]), f"{row.name} {c} {dt}: the result depends on the base address"


def test_p_alone_off_the_boundary_takes_the_checked_route(handle):
    """Kmm aligned, P one element off: before the check of `p` in `symm_gemv_rows_t` the slab kernel's 16-byte loads of
    p ran on an 8-byte base.  gfx950 carries such a load out, so a build without the check passes this too (DESIGN
    4.8b); the test pins the result at this argument pattern, whichever route serves it."""
    lib, h = handle
    row = ct.BY_NAME["mgp_operator_apply"]
    ci = [i for i, x in enumerate(row.cases) if x.get("slab")][0]
    c = row.cases[ci]
    r = Run(row, c, "f64", 0)
    r.gin["P"] = Guarded(r.values["P"].shape, torch.float64, 1, DEV)
    assert r.gin["Kmm"].ptr % 16 == 0 and r.gin["P"].ptr % 16 == 8
    r.sync(lib, h).check(ct.reference(row, ci, "f64"))


@pytest.fixture(scope="module")
def skinny_reg_handle():
    """MGP_SKINNY=reg: `symm_skinny_kernel`, whose 4-element loads of A now also depend on A's base"""
    lib, h = _handle_with({"MGP_SKINNY": "reg"})
    yield lib, h
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,Bt", [(200, 5), (256, 130), (64, 37), (1001, 5)])
def test_register_form_of_the_skinny_product_at_both_alignments(skinny_reg_handle, n, Bt, dt):
    """n % 4 == 0 with A one element off a 16-byte boundary is the case the new condition in `symm_skinny_kernel`
    decides (2 <= Bt <= 128; 130 takes the GEMM and 1001 the element loads on either handle)"""
    lib, h = skinny_reg_handle
    row = ct.BY_NAME["mgp_symm_matmul"]
    c = dict(n=n, Bt=Bt)
    for offset in (0, 1):
        r = Run(row, c, dt, offset).sync(lib, h)
        r.check(row.reference(c, dt, r.ins))


# ---------------------------------------------------------------------------------------------------- family B
def _nan_inputs(row, c, dt):
    ins = ct.build_inputs(row, c, dt)
    for k, v in ins.items():
        if not k.startswith("_") and v.dtype != np.int64 and k not in row.poison_keep:
            ins[k] = np.full_like(v, np.nan)
    return ins


def _poisons(row, c, dt):
    """(case, dtype, inputs) of the poison runs.  The first is in the dtype of the clean case and takes the clean
    case's route -- the host dispatch depends on shapes, dtype, kernel parameters and alignments, never on values --
    so it writes every arena the clean case reads: csrc/kxx.hip and the packed set of the fast sweep exist for fp64
    alone, and only an fp64 poison reaches them.  The second, in the other dtype where there is one, dirties the
    arenas both dtypes share with bit patterns of another width (what the `cg` bug was found with)."""
    out = []
    for pdt in [dt] + ([OTHER[dt]] if len(row.dtypes) == 2 else []):
        if row.poison == "finite":
            out.append((row.poison_case, pdt, ct.build_inputs(row, row.poison_case, pdt)))
        else:
            out.append((c, pdt, _nan_inputs(row, c, pdt)))
    return out


def _arenas_held(lib, h):
    return {a for a in ct.ARENAS if lib.mgp_arena_bytes(h, a.encode()) > 0}


def _fresh():
    return _handle_with({"MGP_KXX": "sym"})


STALE = [p for p in CASES if "B" not in p.values[0].missing]


@pytest.mark.parametrize("row,ci,dt", STALE)
def test_stale_arenas_do_not_reach_the_result(row, ci, dt):
    """clean, poison, clean on a handle nothing else has touched; the library attests (`mgp_arena_bytes`) that the
    same-dtype poison, alone on a second fresh handle, reserves every arena the clean case reserved"""
    c = row.cases[ci]
    lib, h = _fresh()
    lib2, h2 = _fresh()
    try:
        first = Run(row, c, dt, 0).sync(lib, h)
        used = _arenas_held(lib, h)
        poisons = _poisons(row, c, dt)
        pc, pdt, pins = poisons[0]
        Run(row, pc, pdt, 0, ins=pins).sync(lib2, h2)
        hit = _arenas_held(lib2, h2)
        print(f"{row.name} {c} {dt}: clean run holds {sorted(used)}, same-dtype poison holds {sorted(hit)}")
        assert hit >= used, f"{row.name} {c} {dt}: the poison misses {sorted(used - hit)}"
        for pc, pdt, pins in poisons:
            Run(row, pc, pdt, 0, ins=pins).sync(lib, h)  # what it computes does not matter: it dirties the arenas
        third = Run(row, c, dt, 0).sync(lib, h)
        third.check(ct.reference(row, ci, dt))
        assert third.same_bits(first), f"{row.name} {c} {dt}: the result depends on what an earlier call left in an arena"
    finally:
        torch.cuda.synchronize()
        lib.mgp_destroy(h)
        lib2.mgp_destroy(h2)


def test_arenas_each_row_reaches_as_the_library_reports_them():
    """every case of a row on one fresh handle per row: the arenas `mgp_arena_bytes` then reports are the row's
    `arenas` (the table documents, the library attests), rows that claim no scratch hold none, and the rows of
    family B together reach all nine"""
    wrong, reached = [], set()
    for row in ct.TABLE:
        lib, h = _fresh()
        try:
            for c in row.cases:
                for dt in row.dtypes:
                    Run(row, c, dt, 0).sync(lib, h)
            held = _arenas_held(lib, h)
        finally:
            torch.cuda.synchronize()
            lib.mgp_destroy(h)
        print(f"{row.name}: {sorted(held)}")
        if held != set(row.arenas):
            wrong.append((row.name, sorted(held), sorted(row.arenas)))
        if "B" not in row.missing:
            reached |= held
    assert not wrong, wrong
    assert reached == set(ct.ARENAS), sorted(set(ct.ARENAS) - reached)


# ---------------------------------------------------------------------------------------------------- family C
@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream(device=DEV)


@pytest.mark.parametrize("row,ci,dt", CASES)
def test_call_enqueued_behind_unfinished_producers(handle, side, row, ci, dt):
    lib, h = handle
    c = row.cases[ci]
    r = Run(row, c, dt, ci % 2).behind_producers(lib, h, side)
    print(f"producers ran for {r.delay_ms:.1f} ms")
    assert r.delay_ms >= MIN_DELAY_MS, f"the producers ran for {r.delay_ms:.2f} ms only: the test proves nothing"
    r.check(ct.reference(row, ci, dt))


def _oracle_kernel_and_cls(kind, ls):
    from cggp import kernels
    from oracle import kernels as ok
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32, "matern52": kernels.Matern52}[kind]
    return cls(variance=ct.VAR, lengthscales=list(ls)), ok.Kernel(kind, ct.VAR, ls)


@pytest.mark.parametrize("Bt", [1, 5])
@pytest.mark.parametrize("op", ["dense", "kmm_lambda", "kxx", "sgpr"])
def test_conjugate_gradient_facade_behind_unfinished_producers(side, op, Bt):
    """`ConjugateGradient` on the four operator kinds: the operator's tensors and the right-hand sides are still being
    produced when the solve is enqueued; 5 fixed steps against the oracle's loop (1e-9,
    test_cg_fixed_iterations_match_oracle)"""
    from cggp.conjugate_gradient import (ConjugateGradient, DenseOperator, KmmLambdaOperator, KxxNoiseOperator,
                                         SgprNormalOperator)
    from oracle import cg as ocg
    rng = np.random.default_rng(100 + Bt)
    n, D, k = 200, 5, 5
    ls = ct.lengthscales(rng, D)
    kern, okern = _oracle_kernel_and_cls("matern32", ls)
    X, Z, lam = rng.standard_normal((777, D)), rng.standard_normal((n, D)), rng.uniform(0.5, 1.5, n)
    if op == "dense":
        A = ct._spd(rng, n)
        parts = dict(A=A)
    elif op == "kmm_lambda":
        A = okern.K(Z) + np.diag(lam)
        parts = dict(Z=Z, lam=lam)
    elif op == "kxx":
        A = okern.K(Z) + 1.0 * np.eye(n)
        parts = dict(Z=Z)
    else:
        K = okern.K(X, Z)
        A = 1.0 * (okern.K(Z) + 1e-6 * np.eye(n)) + K.T @ K
        parts = dict(X=X, Z=Z)
    b = rng.standard_normal((n, Bt))  # the facade's column layout
    parts["b"] = b
    staged = {name: torch.from_numpy(v).to(DEV) for name, v in parts.items()}
    bufs = {name: torch.full_like(v, float("nan")) for name, v in staged.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0, e1 = _delay()
        for name in bufs:
            bufs[name].copy_(staged[name], non_blocking=True)
        if op == "dense":
            oper = DenseOperator(bufs["A"])
        elif op == "kmm_lambda":
            oper = KmmLambdaOperator(kern, bufs["Z"], bufs["lam"])
        elif op == "kxx":
            oper = KxxNoiseOperator(kern, bufs["Z"], 1.0)
        else:
            oper = SgprNormalOperator(kern, bufs["X"], bufs["Z"], 1.0, jitter=1e-6, max_rhs=Bt)
        sol, (steps, err) = ConjugateGradient(0.0, max_iterations=k).solve_with_stats(oper, bufs["b"])
        sol = sol.clone()
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= MIN_DELAY_MS
    o_sol, (o_steps, o_err) = ocg.ConjugateGradient(0.0, max_iterations=k).solve_with_stats(A, b)
    assert int(steps) == k == o_steps
    assert ct.relerr(sol.cpu().numpy(), o_sol) < 1e-9


@pytest.mark.parametrize("name", ["mgp_dot_all", "mgp_k_dense_vjp", "mgp_kxx_grad", "mgp_kmn_knm_vjp",
                                  "mgp_kmn_knm_vjp_anyd"])
def test_host_scalar_wrappers_behind_unfinished_producers(side, name):
    """the `cggp.ops` wrappers that hand host scalars back: their read-back must wait for the stream the call was
    enqueued on (the process-wide handle follows torch's current stream, `Handle.sync_stream`)"""
    from cggp import ops
    row, ci, dt = ct.BY_NAME[name], 0, "f64"
    c = row.cases[ci]
    ins = ct.build_inputs(row, c, dt)
    staged = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ins.items() if not k.startswith("_")}
    bufs = {k: torch.full_like(v, float("nan")) for k, v in staged.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0, e1 = _delay()
        for k in bufs:
            bufs[k].copy_(staged[k], non_blocking=True)
        if name == "mgp_dot_all":
            got = dict(out=ops.dot_all(bufs["A"], bufs["B"]))
        elif name == "mgp_k_dense_vjp":
            spec = ops.KernelSpec(c["kind"], 1.4, list(ins["_ls"]), c["D"])
            dv, dl = ops.k_dense_vjp(spec, bufs["A"], bufs["B"], bufs["G"][:, :c["nb"]].contiguous())
            got = dict(dv=dv, dl=np.asarray(dl))
        elif name == "mgp_kxx_grad":
            spec = ops.KernelSpec(c["kind"], ct.VAR, list(ins["_ls"]), c["D"])
            dv, dl = ops.kxx_grad(spec, bufs["X"], bufs["U"], bufs["V"], layout=c["layout"])
            got = dict(dv=dv, dl=np.asarray(dl))
        elif name == "mgp_kmn_knm_vjp_anyd":  # case 0: D = 33, the staged route (`ops.kmn_knm_vjp` stops at D = 32)
            assert c["D"] == 33
            spec = ops.KernelSpec(c["kind"], row.VARIANCE, list(ins["_ls"]), c["D"])
            dv, dl, dZ = ops.kmn_knm_vjp_anyd(spec, bufs["X"], bufs["Z"], bufs["Gq"], bufs.get("Y"), bufs.get("Gb"),
                                              need_dZ=True, panel_rows=c["panel_rows"])
            got = dict(dv=dv, dl=np.asarray(dl), dZ=dZ.clone())
        else:
            spec = ops.KernelSpec(c["kind"], ct.VAR, list(ins["_ls"]), c["D"])
            dv, dl, dZ = ops.kmn_knm_vjp(spec, bufs["X"], bufs["Z"], bufs["Gq"], bufs.get("Y"), bufs.get("Gb"),
                                         need_dZ=True)
            got = dict(dv=dv, dl=np.asarray(dl), dZ=dZ.clone())
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= MIN_DELAY_MS
    if "dZ" in got:
        got["dZ"] = got["dZ"].cpu().numpy()
    row.check(c, dt, ins, got, ct.reference(row, ci, dt))


def test_forked_sgpr_route_behind_unfinished_producers(aside_handle, side):
    """MGP_SGPR_KMM_ASIDE=2: `mgp_operator_apply` and a 5-step `mgp_pcg_solve` of MGP_OP_SGPR with one right-hand
    side fork the s2 Kmm p product onto the library's own stream; the fork must wait for p (and Kmm) to be produced"""
    lib, h = aside_handle
    apply_row, solve_row = ct.BY_NAME["mgp_operator_apply"], ct.BY_NAME["mgp_pcg_solve"]
    c = dict(op="sgpr", n=130, N=777, Bt=1, D=5, kind="se", s2=1.0)
    for row, case in ((apply_row, c), (solve_row, dict(c, k=5, v0=False))):
        for offset in (0, 1):
            r = Run(row, case, "f64", offset).behind_producers(lib, h, side)
            assert r.delay_ms >= MIN_DELAY_MS
            r.check(row.reference(case, "f64", r.ins))
