"""tests/contract_table.py against every header of include/: every exported function is either a row of the table or
excluded with a reason, and the table is well formed (no GPU needed)."""

import numpy as np

import contract_table as ct
from test_abi import declared_symbols, declared_symbols_by_header

EXPECTED_ROWS = """mgp_knm_matvec mgp_kmn_matvec mgp_k_dense mgp_kmn_knm mgp_kmn_sq_colsum mgp_kxx_matvec mgp_kxx_pivchol
mgp_lowrank_apply mgp_knm_project mgp_kxx_grad mgp_kmn_knm_vjp mgp_symm_matmul mgp_pcg_solve mgp_pcg_solve_record
mgp_operator_apply mgp_kmm_lambda_matvec mgp_colwise_dot mgp_dot_all mgp_nearest_center mgp_cluster_stats
mgp_segment_sums mgp_k_dense_vjp mgp_rff_features mgp_rff_sample mgp_knm_matvec_anyd mgp_kmn_matvec_anyd
mgp_kxx_matvec_anyd mgp_kmn_knm_vjp_anyd mgp_k_dense_vjp_points mgp_rff_sample_vjp mgp_knm_quadform""".split()

HEADERS = ["mgp.h", "mgp_anyd.h", "mgp_pathwise.h", "mgp_points.h", "mgp_predict.h", "mgp_sweep_anyd.h"]


def test_every_exported_function_is_a_row_or_excluded_with_a_reason():
    by_header = declared_symbols_by_header()
    assert sorted(by_header) == HEADERS and by_header["mgp.h"] == declared_symbols()
    assert all(by_header[hd] for hd in HEADERS), "a header that declares nothing: the expression no longer matches it"
    names = sorted(set(n for v in by_header.values() for n in v))
    assert sum(len(v) for v in by_header.values()) == len(names)  # no function is declared twice
    rows = [r.name for r in ct.TABLE]
    assert len(rows) == len(set(rows)) == 31 and sorted(rows) == sorted(EXPECTED_ROWS)
    for hd, declared in by_header.items():
        for n in declared:
            assert (n in ct.BY_NAME) != (n in ct.EXCLUDED), f"{n}: exported by include/{hd}, " \
                "needs exactly one of a row in tests/contract_table.py or an entry of EXCLUDED"
    for n, why in ct.EXCLUDED.items():
        assert n in names, f"{n} is excluded but not exported"
        assert len(why) >= 4
    assert set(ct.BY_NAME) <= set(names)


def test_rows_are_well_formed():
    for row in ct.TABLE:
        assert row.dtypes and set(row.dtypes) <= {"f64", "f32"} and row.cases
        assert set(row.arenas) <= set(ct.ARENAS)
        assert set(row.missing) <= {"A", "B", "C"} and all(len(v) > 10 for v in row.missing.values())
        assert ("B" in row.missing) == (not row.arenas), row.name  # a stale-arena case wherever there is an arena
        assert row.poison in ("nan", "finite") and (row.poison == "finite") == (row.poison_case is not None)
        if len(row.dtypes) == 1:
            assert row.poison == "finite", row.name  # no other dtype to poison in: a larger finite problem
        seeds = [row.seed(c) for c in row.cases]
        assert len(set(seeds)) == len(seeds)
        for c in list(row.cases) + ([row.poison_case] if row.poison_case else []):
            for dt in row.dtypes:
                ins = row.ins(c, dt, np.random.default_rng(row.seed(c)))
                again = row.ins(c, dt, np.random.default_rng(row.seed(c)))
                outs = row.outs(c, dt)
                assert not set(ins) & set(outs)
                assert ins or outs
                for k, v in ins.items():
                    assert np.array_equal(v, again[k], equal_nan=True)
                    if not k.startswith("_"):
                        assert v.dtype in (np.float64, np.int64), (row.name, k, v.dtype)
                for k, (shape, kind) in outs.items():
                    assert kind in ("T", "i64") and all(s >= 1 for s in shape), (row.name, k, shape)
    # (which arenas a row really reaches is the library's to say: tests/test_gpu_buffer_contract.py asks it)


def test_poison_cases_are_at_least_as_large_in_every_dimension():
    for row in ct.TABLE:
        if row.poison_case is None:
            continue
        for c in row.cases:
            for k, v in c.items():
                if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and k in ("N", "M", "D", "P", "na", "nb",
                                                                                          "max_rank"):
                    if k == "D":
                        continue  # the arenas scale with the padded D; checked by the shapes below
                    assert row.poison_case[k] >= v, (row.name, k)


def test_references_of_the_small_cases_are_finite():
    """the cheap end of the table evaluates on the CPU: a typo in a reference shows here, not on the GPU"""
    for row in ct.TABLE:
        for ci, c in enumerate(row.cases):
            if max([v for v in c.values() if isinstance(v, int) and not isinstance(v, bool)] + [0]) > 130:
                continue
            for dt in row.dtypes:
                ref = ct.reference(row, ci, dt)
                flat = ref if isinstance(ref, tuple) else (ref,)
                for a in flat:
                    if a is not None:
                        assert np.all(np.isfinite(np.asarray(a, dtype=np.float64))), (row.name, c, dt)


def test_route_printer_on_the_slab_case():
    """`OperatorApply.route` (the restatement of csrc/dense.hip's dispatch that the GPU tests print beside a case that
    reads a pointer; the library does not report its route) says what the log should: vector loads when Kmm and p are
    both 16-byte aligned, scalar loads otherwise, the slab kernel while the slab has at most 8 rows per CU.  The
    library itself is held to the result by tests/test_gpu_buffer_contract.py."""
    row = ct.BY_NAME["mgp_operator_apply"]
    c = [x for x in row.cases if x.get("slab")][0]
    assert c["n"] % 128 == 0 and c["n"] >= 1024 and c["Bt"] == 1
    base = dict(Kmm=1 << 20, P=1 << 21)
    for cus in (256, 304):
        assert "slab kernel, 16-byte loads of Kmm and p" in row.route(c, "f64", base, cus)
        assert "slab kernel, scalar" in row.route(c, "f64", dict(base, P=base["P"] + 8), cus)
        assert "slab kernel, scalar" in row.route(c, "f64", dict(base, Kmm=base["Kmm"] + 8), cus)
        assert "slab kernel, scalar" in row.route(c, "f32", dict(base, P=base["P"] + 4), cus)
    assert "row GEMV" in row.route(c, "f64", base, num_cus=32)  # 512 rows are more than 8 per CU of a small part
