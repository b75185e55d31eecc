"""tests/sequence_plan.py against tests/contract_table.py (no GPU needed): every row is read and written once in every
arena it lists, no row is read behind itself, the shuffles cover every (row, case, dtype) once each, and the plan is
the same in every process."""

import hashlib
import os
import subprocess
import sys

import numpy as np

import contract_table as ct
import sequence_plan as sp


def test_every_row_is_reader_and_writer_once_in_every_arena_it_lists():
    for arena in ct.ARENAS:
        pairs = sp.ring_pairs(arena)
        names = [r.name for r in ct.TABLE if arena in r.arenas]
        assert len(names) >= 2, f"{arena}: a ring needs two rows"
        assert sorted(p[0] for p in pairs) == sorted(names) == sorted(p[1] for p in pairs)
        assert all(reader != writer for reader, writer in pairs), arena
    for row in ct.TABLE:
        mine = [it for it in sp.ring_items() if it[1] == row.name]
        assert sorted(set(it[0] for it in mine)) == sorted(row.arenas), row.name
        assert len(mine) == len(row.arenas) * len(row.cases) * len(row.dtypes), row.name
        for arena in row.arenas:  # and it is the poison behind exactly one other row there
            assert len(set(it[1] for it in sp.ring_items() if it[0] == arena and it[4] == row.name)) == 1


def test_writer_cases_are_a_rotation_of_all_of_the_writers_cases():
    for arena, reader, ci, dt, writer in sp.ring_items():
        w = ct.BY_NAME[writer]
        order = sp.writer_cases(arena, reader, ci, dt, w)
        assert sorted(order) == list(range(len(w.cases)))
        assert sp.writer_dtype(w, dt) in w.dtypes and (dt not in w.dtypes or sp.writer_dtype(w, dt) == dt)
    starts = {sp.writer_cases(a, r, ci, dt, ct.BY_NAME[w])[0] for a, r, ci, dt, w in sp.ring_items() if a == "ws"}
    assert len(starts) > 1  # the pairs of a ring do not all start from the writer's first case


def test_shuffles_cover_every_triple_once_and_differ():
    t = sp.triples()
    assert len(t) == len(set(t)) == sum(len(r.cases) * len(r.dtypes) for r in ct.TABLE)
    perms = [sp.shuffle(k) for k in range(sp.SHUFFLES)]
    for p in perms:
        assert sorted(p) == sorted(t) and p != t
    assert perms[0] != perms[1]
    slices = sp.shuffle_slices()
    assert len(slices) == sp.SHUFFLES * -(-len(t) // sp.SLICE)
    for k in range(sp.SHUFFLES):
        mine = [s for s in slices if s[0] == k]
        assert [s[1] for s in mine] == list(range(len(mine)))
        flat = [pair for s in mine for pair in s[2]]
        assert all(1 <= len(s[2]) <= sp.SLICE for s in mine)
        assert [e for e, _ in flat] == perms[k]
        assert [p for _, p in flat] == [perms[k][-1]] + perms[k][:-1]  # the predecessor in the permutation, cyclically


def test_scale_and_stream_plans_name_cases_that_exist():
    for name in sp.GENERIC_D_ROWS:
        row = ct.BY_NAME[name]
        assert row.cases[sp.d33_case(row)]["D"] == 33 and "f64" in row.dtypes
    pairs = sp.generic_d_pairs()
    assert len(pairs) == len(set(pairs)) == 30 and all(a != b for a, b in pairs)
    ls = ct.lengthscales(np.random.default_rng(0), 33)
    other = sp.other_lengthscales(ls)
    assert other.shape == ls.shape and np.all(other > 0) and not np.any(other == ls)
    sps = sp.stream_pairs()
    assert len(sps) == 12 and all(x != y for x, y, _ in sps)
    for x, y, shared in sps:
        assert (shared == ()) == ("mgp_knm_quadform" in (x, y)), (x, y, shared)  # as the docstring says
        for n in (x, y):
            row = ct.BY_NAME[n]
            assert not row.host_scalars and "pcg" not in n and 0 <= sp.STREAM_CASE[n] < len(row.cases)


def _digest():
    h = hashlib.sha256()
    h.update(repr(sp.ring_items()).encode())
    h.update(repr([sp.writer_cases(a, r, ci, dt, ct.BY_NAME[w]) for a, r, ci, dt, w in sp.ring_items()]).encode())
    h.update(repr(sp.shuffle_slices()).encode())
    h.update(repr((sp.generic_d_pairs(), sp.stream_pairs(), sorted(sp.counts().items(), key=str))).encode())
    return h.hexdigest()


def test_the_plan_is_the_same_in_another_process_with_another_hash_seed():
    """`zlib.crc32`, never `hash`: a process with another PYTHONHASHSEED computes the same plan, digest for digest"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="1" if os.environ.get("PYTHONHASHSEED") != "1" else "2")
    code = ("import sys; sys.path.insert(0, %r); import conftest, test_sequence_plan as t; print(t._digest())" % here)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=here)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == _digest()


def test_counts_are_the_ones_the_design_document_quotes():
    c = sp.counts()
    print(c)
    assert c["triples"] == len(sp.triples()) and c["ring_items"] == sum(n for _, n in c["rings"].values())
    assert c["shuffle_calls"] == 2 * sp.SHUFFLES * c["triples"]  # a poison run and a clean run per element
    assert all(rows >= 2 for rows, _ in c["rings"].values())
