"""No call's result depends on its handle's history (plans: tests/sequence_plan.py; rows: tests/contract_table.py).

`cggp/_hip.py` keeps one handle per device, so every call of a training or prediction loop shares nine reused arenas
and two device copies of kernel scales with whatever ran before it -- another entry point -- and the handle follows
torch's current stream.  The property, for every element of every sequence here: a clean call returns, bit for bit,
what the same call returns alone on a fresh handle.  Both runs use the same guard-banded buffers (rows whose host
dispatch reads a pointer value take the same route), both handles are created with MGP_KXX=sym, the outputs are
refilled with the sentinel before every run, and the fresh-handle result -- computed once per (row, case, dtype, inputs)
and shared by the module -- is also held to the row's reference bar.

rings     per arena, the rows that reach it in table order form a cycle: clean, the next row's poison run (NaN inputs
          or its finite poison case; its cases are tried in the plan's order until `mgp_arena_bytes` reports the
          arena held), clean again.
shuffles  two seeded permutations of every (row, case, dtype), in slices of 40 on one handle each, the poison run of
          the previous element's row before every clean call.
scales    the lengthscale memo of the any-D sweeps (l1, l2, l1; D = 40 then D = 33 on a prefix; se then matern32) and
          every ordered pair of the generic-D rows, which leave c / l, 1 / l, variance (-2 / l) or raw scales in the
          one device buffer they share.
streams   work enqueued through one handle runs in call order across `mgp_set_stream` (include/mgp.h): X behind busy
          producers on one stream, Y through the same handle on another; events say which ran first."""

import types

import numpy as np
import pytest
import torch

import contract_table as ct
import sequence_plan as sp
from buffer_contract import SENTINEL_BITS, _bits
from test_gpu_buffer_contract import DEV, MIN_DELAY_MS, Run, _delay, _handle_with, _poisons  # (_poisons: _nan_inputs)

pytestmark = pytest.mark.gpu


def _fresh():
    return _handle_with({"MGP_KXX": "sym"})


def _destroy(lib, h):
    torch.cuda.synchronize()
    lib.mgp_destroy(h)


def _go(run, lib, h):
    """one synchronous run on outputs that hold the sentinel again (a call that skips an element must not find the
    previous run's value there)"""
    for g in run.gout.values():
        _bits(g.flat).fill_(SENTINEL_BITS[g.dtype])
    return run.sync(lib, h)


def _snapshot(run):
    return types.SimpleNamespace(got={k: v.clone() for k, v in run.got.items()}, host=dict(run.host))


_ALONE = {}


def alone(name, ci, dt, ins=None, tag=None, c=None):
    """(the Run and its buffers, its result alone on a fresh handle): once per key, held to the row's reference"""
    key = (name, ci, dt, tag)
    if key not in _ALONE:
        row = ct.BY_NAME[name]
        c = row.cases[ci] if c is None else c
        run = Run(row, c, dt, 0, ins=ins)
        lib, h = _fresh()
        try:
            _go(run, lib, h)
        finally:
            _destroy(lib, h)
        run.check(ct.reference(row, ci, dt) if ins is None else row.reference(c, dt, run.ins))
        _ALONE[key] = (run, _snapshot(run))
    return _ALONE[key]


def _poison(lib, h, name, ci, dt):
    """the first poison run of family B for that row and case: NaN inputs, or the row's finite poison case"""
    row = ct.BY_NAME[name]
    pc, pdt, pins = _poisons(row, row.cases[ci], dt)[0]
    Run(row, pc, pdt, 0, ins=pins).sync(lib, h)


# ---------------------------------------------------------------------------------------------------- rings
RING = [pytest.param(*it, id=f"{it[0]}-{it[1][4:]}-{it[2]}-{it[3]}-after-{it[4][4:]}") for it in sp.ring_items()]


@pytest.mark.parametrize("arena,reader,ci,dt,writer", RING)
def test_ring_of_an_arena(arena, reader, ci, dt, writer):
    run, first = alone(reader, ci, dt)
    w = ct.BY_NAME[writer]
    wdt = sp.writer_dtype(w, dt)
    lib, h = _fresh()
    try:
        _go(run, lib, h)
        assert run.same_bits(first), f"{reader} {run.c} {dt}: two fresh handles disagree"
        tried = []
        for wdtype in [wdt] + [d for d in w.dtypes if d != wdt]:
            for wi in sp.writer_cases(arena, reader, ci, dt, w):
                _poison(lib, h, writer, wi, wdtype)
                tried.append((wi, wdtype))
                if lib.mgp_arena_bytes(h, arena.encode()) > 0:
                    break
            if lib.mgp_arena_bytes(h, arena.encode()) > 0:
                break
        assert lib.mgp_arena_bytes(h, arena.encode()) > 0, f"no case of {writer} reserved `{arena}` (tried {tried})"
        _go(run, lib, h)
        assert run.same_bits(first), (f"{reader} {run.c} {dt}: the result depends on what {writer} "
                                      f"(cases {tried}) left behind, arena `{arena}`")
    finally:
        _destroy(lib, h)


# ---------------------------------------------------------------------------------------------------- shuffles
SLICES = [pytest.param(pairs, id=f"shuffle{k}-slice{s}") for k, s, pairs in sp.shuffle_slices()]


@pytest.mark.parametrize("pairs", SLICES)
def test_shuffled_slice_on_one_handle(pairs):
    lib, h = _fresh()
    log = []
    try:
        for (name, ci, dt), (pname, pci, pdt) in pairs:
            run, first = alone(name, ci, dt)
            _poison(lib, h, pname, pci, pdt)
            log.append(f"poison of {pname} case {pci} {pdt}")
            _go(run, lib, h)
            log.append(f"{name} case {ci} {dt}")
            assert run.same_bits(first), (f"{name} {run.c} {dt} differs from its result alone on a fresh handle; "
                                          f"the calls before it, oldest first: {log[-6:-1]}")
    finally:
        _destroy(lib, h)


# ---------------------------------------------------------------------------------------------------- scales
def _anyd(D, ls=None, kind="se"):
    """mgp_knm_matvec_anyd on 129 x 65 points (two owned blocks, two chunks) with 3 columns; `ls` replaces the case's
    lengthscales.  -> (Run, its result alone on a fresh handle)"""
    row = ct.BY_NAME["mgp_knm_matvec_anyd"]
    c = dict(na=129, nb=65, D=D, R=3, kind=kind, wl=ct.COLS, ol=ct.COLS)
    ins = ct.build_inputs(row, c, "f64")
    if ls is not None:
        ins["_ls"] = np.asarray(ls, dtype=np.float64)
    return alone(row.name, None, "f64", ins=ins, c=c, tag=("anyd", D, kind, ins["_ls"].tobytes()))


def test_anyd_scale_memo_follows_the_lengthscales_the_dimension_and_the_kind():
    """`anyd_upload_scales` (csrc/sweep_anyd.hip) uploads c / l when the host copy differs in length or content: l1,
    l2, l1 again; then D = 33 with the first 33 entries of l1, directly after the D = 40 call; then the same l with
    another kernel kind, whose c differs"""
    l1 = _anyd(40)[0].ins["_ls"]
    l2 = sp.other_lengthscales(l1)
    steps = [("D=40 l1", _anyd(40)), ("D=40 l2", _anyd(40, l2)), ("D=40 l1 again", _anyd(40)),
             ("D=33, the first 33 entries of l1", _anyd(33, l1[:33])), ("D=40 l1 after D=33", _anyd(40)),
             ("D=40 l1 matern32", _anyd(40, kind="matern32")), ("D=40 l1 se after matern32", _anyd(40))]
    lib, h = _fresh()
    try:
        for i, (what, (run, first)) in enumerate(steps):
            _go(run, lib, h)
            assert run.same_bits(first), f"{what}: differs from a fresh handle after {[s[0] for s in steps[:i]]}"
    finally:
        _destroy(lib, h)


def _d33(name, other=False):
    row = ct.BY_NAME[name]
    ci = sp.d33_case(row)
    if not other:
        return alone(name, ci, "f64")
    ins = ct.build_inputs(row, row.cases[ci], "f64")
    ins["_ls"] = sp.other_lengthscales(ins["_ls"])
    return alone(name, ci, "f64", ins=ins, tag="other lengthscales")


@pytest.mark.parametrize("a,b", sp.generic_d_pairs(), ids=lambda n: n[4:])
def test_generic_d_rows_do_not_read_each_others_scales(a, b):
    """a, then b with other lengthscales, then a again: every writer of `h->dparams` puts another scale there (c / l,
    1 / l, variance (-2 / l), raw) and every reader must have uploaded its own"""
    steps = [(a, _d33(a)), (b + " with other lengthscales", _d33(b, other=True)), (a + " again", _d33(a))]
    lib, h = _fresh()
    try:
        for what, (run, first) in steps:
            _go(run, lib, h)
            assert run.same_bits(first), f"{what}: differs from its result alone on a fresh handle"
    finally:
        _destroy(lib, h)


# ---------------------------------------------------------------------------------------------------- streams
@pytest.fixture(scope="module")
def streams():
    return torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)


@pytest.mark.parametrize("x,y,shared", sp.stream_pairs(),
                         ids=lambda v: v[4:] if isinstance(v, str) else "+".join(v) or "none")
def test_work_through_one_handle_runs_in_call_order_across_a_stream_change(streams, x, y, shared):
    """X is enqueued on stream A behind producers that keep A busy; the handle is then pointed at the idle stream B and
    Y enqueued.  The contract of `mgp_set_stream`: B waits for what the handle gave A.  `eA` is recorded on A behind X,
    `eB` on B behind Y: without the ordering Y and `eB` complete while A is still in its producers and
    `eA.elapsed_time(eB)` is negative.  Both calls are warmed first, so no arena grows while work is queued."""
    sA, sB = streams
    rx, fx = alone(x, sp.STREAM_CASE[x], "f64")
    ry, fy = alone(y, sp.STREAM_CASE[y], "f64")
    lib, h = _fresh()
    try:
        _go(rx, lib, h)
        _go(ry, lib, h)  # warm: every arena either call needs has its size
        held = {a: lib.mgp_arena_bytes(h, a.encode()) for a in ct.ARENAS}
        assert all(held[a] > 0 for a in shared), (shared, held)
        for r in (rx, ry):
            for k, g in r.gin.items():
                g.upload(r.values[k])
            for g in r.gout.values():
                _bits(g.flat).fill_(SENTINEL_BITS[g.dtype])
        eA, eB = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(sA):
            e0, e1 = _delay()
            rx._call(lib, h, sA)
            rx.got = {k: g.payload.clone() for k, g in rx.gout.items()}
            eA.record(sA)
        with torch.cuda.stream(sB):
            ry._call(lib, h, sB)
            ry.got = {k: g.payload.clone() for k, g in ry.gout.items()}
            eB.record(sB)
        torch.cuda.synchronize()  # the one synchronisation
        delay, gap = e0.elapsed_time(e1), eA.elapsed_time(eB)
        print(f"{x} -> {y}: producers ran for {delay:.1f} ms, eA -> eB {gap:.3f} ms")
        assert delay >= MIN_DELAY_MS, f"the producers ran for {delay:.2f} ms only: the test proves nothing"
        assert {a: lib.mgp_arena_bytes(h, a.encode()) for a in ct.ARENAS} == held, "an arena grew while work was queued"
        assert gap >= 0, f"{y} on the second stream finished {-gap:.3f} ms before {x} on the first"
        rx.check(ct.reference(rx.row, sp.STREAM_CASE[x], "f64"))
        ry.check(ct.reference(ry.row, sp.STREAM_CASE[y], "f64"))
        assert rx.same_bits(fx) and ry.same_bits(fy), (x, y)
    finally:
        _destroy(lib, h)
