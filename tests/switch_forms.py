"""The forms behind libmgp's environment switches, one row per switch value, and what each row is held to.

`mgp_create` reads the switches into the handle (csrc/api.hip); DESIGN section 4.8 lists them.  Each row names the
entry point, the shapes that route into the form (worked out from the dispatch code cited in `routes`), the
reference and the bar.  tests/test_gpu_switch_forms.py runs the rows on the GPU; tests/test_switch_inventory.py
checks on the CPU that every switch csrc/ reads is a row here or in EXEMPT.

Bars are those of the default form's existing test: 1e-11 of max |ref| for fp64 kernel products (1e-9 for
Matern-1/2, tests/test_gpu_parity.py::test_knm_kmn_matvec_fp64), 2e-4 for fp32 against fp64, 1e-12 / 1e-13 for the
symmetric products (test_symm_matmul_fp64 / test_symm_gemv_upper_triangle_path), 1e-9 for k-step CG iterates
(test_cg_fixed_iterations_match_oracle).  `same_as_default`: the form changes only timing or launch boundaries and
keeps the summation order, so its result must also equal the default handle's bit for bit.
"""

import contextlib

KINDS = ("se", "matern12", "matern32", "matern52")
NUM_CUS = 256  # MI355X

# ---------------------------------------------------------------- sweep cases: (kind, D, N, M, R, layout, sgpr)
# D = 2, 6, ..., 30, 32 are the KS = 1..9 instantiations of sweep_mfma.hip (KS = (D + 5) / 4); M or N above 512 splits
# the streamed set into 256-point tiles, so reduce_partials_m_kernel runs
MFMA_CASES = [
    ("se", 2, 1, 1, 1, "cols", False),
    ("matern12", 6, 63, 1100, 2, "rows", False),
    ("matern32", 10, 257, 600, 3, "cols", True),
    ("matern52", 14, 65, 4097, 4, "cols", False),
    ("se", 18, 600, 63, 5, "rows", True),
    ("matern12", 22, 1030, 65, 8, "cols", False),
    ("matern32", 26, 65, 1030, 13, "rows", False),
    ("matern52", 30, 4097, 17, 1, "cols", True),
    ("se", 32, 300, 257, 2, "cols", False),
]
# DP tiers 2 / 4 / 8 / 16 / 32 of the VALU forms at D = 1, 3, 8, 9, 16, 17, 32; RC 1, 2, 4, 8 (R = 13 = 8 + 4 + 1)
VALU_CASES = [
    ("se", 1, 1, 4097, 1, "cols", False),
    ("matern12", 3, 63, 700, 2, "rows", True),
    ("matern32", 8, 4097, 63, 3, "cols", False),
    ("matern52", 9, 257, 600, 4, "rows", False),
    ("se", 16, 600, 257, 5, "cols", True),
    ("matern12", 17, 65, 1030, 8, "cols", False),
    ("matern32", 32, 1030, 65, 13, "rows", False),
    ("matern52", 8, 300, 300, 1, "cols", True),
]
ONE_RHS_CASES = [  # forms that exist for one right-hand side only
    ("se", 1, 63, 4097, 1, "cols", False),
    ("matern12", 3, 1030, 257, 1, "rows", True),
    ("matern32", 8, 4097, 65, 1, "cols", False),
    ("matern52", 5, 65, 1030, 1, "cols", False),
]
D17_32_CASES = [("se", 17, 600, 257, 1, "cols", True), ("matern32", 32, 1030, 65, 1, "rows", False),
                ("matern52", 24, 65, 1030, 1, "cols", False)]
RC_CASES = [("se", 8, 600, 257, 2, "cols", False), ("matern12", 3, 1030, 65, 3, "rows", True),
            ("matern52", 5, 65, 1030, 4, "cols", False)]
# tiny lengthscales, huge coordinates, coincident points (tests/test_properties.py::
# test_gpu_fused_products_at_extreme_scales): (kind, D, N, M, ls_scale, x_scale, seed)
EXTREME_CASES = [("se", 8, 300, 200, 1e-3, 1.0, 1), ("matern12", 3, 200, 150, 1.0, 300.0, 2),
                 ("matern32", 17, 150, 120, 1e-2, 30.0, 3), ("matern52", 2, 300, 100, 1e4, 1.0, 4)]

# fast-kernel chunking: the three block decodes of sweep_fast_kernel (sweep.hip), chosen by nchunks.
# (env, kind, D, N, M, R, branch); knm direction: N owned rows, M streamed points
CHUNK_CASES = [
    ({"MGP_SWEEP_TARGET": "1", "MGP_SWEEP_GRAN": "64"}, "se", 8, 63, 8192, 1, "xcd8"),
    ({"MGP_SWEEP_TARGET": "1", "MGP_SWEEP_GRAN": "64"}, "matern32", 4, 63, 8192, 2, "xcd8"),
    ({"MGP_SWEEP_TARGET": "1", "MGP_SWEEP_GRAN": "256"}, "matern52", 8, 63, 700, 1, "few"),
    ({"MGP_SWEEP_TARGET": "1", "MGP_SWEEP_GRAN": "256"}, "se", 6, 63, 1000, 4, "few"),
    ({"MGP_SWEEP_TARGET": "1", "MGP_SWEEP_GRAN": "64"}, "matern12", 8, 63, 8193, 1, "linear"),
    ({"MGP_SWEEP_TARGET": "2", "MGP_SWEEP_GRAN": "128"}, "matern32", 16, 65, 1700, 2, "linear"),
]


def fast_chunks(env, D, N, M, R):
    """nchunks of launch_sweep (sweep.hip) for the default fast kernel (MGP_SWEEP_FAST=2, fp64) at num_cus = 256."""
    target_per_cu = int(env.get("MGP_SWEEP_TARGET", 16))
    gran_env = int(env.get("MGP_SWEEP_GRAN", 0))
    nosplit_env = int(env.get("MGP_NOSPLIT_PER_CU", 4))
    dp = 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32
    rc = 8 if R >= 8 else 4 if R >= 4 else 2 if R >= 2 else 1
    rpt = (1 if dp > 16 else 2) if rc > 1 else (4 if dp <= 8 else 2)  # default MGP_SWEEP_RPT* values
    fnt = 512 if dp <= 16 else 256
    nblk = -(-N // (fnt * rpt))
    target = target_per_cu * NUM_CUS * 256 // fnt
    nosplit = max(nosplit_env, 8)
    nchunks = 1 if nblk * (fnt // 256) >= nosplit * NUM_CUS else -(-target // nblk)
    gran = gran_env if gran_env > 0 else (256 if dp <= 8 else 128 if dp <= 16 else 64)
    nchunks = max(1, min(nchunks, -(-M // gran)))
    b_chunk = -(-M // nchunks)
    b_chunk = -(-b_chunk // gran) * gran
    return -(-M // b_chunk)


def decode_branch(nchunks):
    """The block decode sweep_fast_kernel takes for nchunks streamed chunks."""
    if nchunks % 8 == 0:
        return "xcd8"
    return "few" if nchunks <= 4 else "linear"


# ---------------------------------------------------------------- the table
FORMS = [
    # -------- sweeps (knm_matvec, kmn_matvec, the addend form of mgp_operator_apply on MGP_OP_SGPR)
    dict(id="sweep_mfma", env={"MGP_SWEEP": "mfma"}, entry="sweep", cases=MFMA_CASES + [c for c in EXTREME_CASES],
         routes="sweep.hip mgp_sweep: fp64 and sweep_mode 1 -> mgp_sweep_mfma_f64 (sweep_mfma.hip, KS = (D + 5) / 4)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_lds_tile", env={"MGP_SWEEP_FAST": "0"}, entry="sweep", cases=VALU_CASES + EXTREME_CASES,
         routes="launch_sweep: fast_on false -> sweep_kernel<double, DP, KIND, RC> (RC 1, 2, 4, 8)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_fast_256", env={"MGP_SWEEP_FAST": "1"}, entry="sweep", cases=ONE_RHS_CASES + D17_32_CASES,
         routes="launch_sweep: RC 1, sweep_fast 1 -> sweep_fast_kernel<DP, KIND, 1, 4|2, 256, 11> (RC > 1: sweep_kernel)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_fast_256_rpt2", env={"MGP_SWEEP_FAST": "1", "MGP_SWEEP_RPT": "2"}, entry="sweep",
         cases=ONE_RHS_CASES[:3], routes="D <= 8, RC 1, fnt 256, frpt 2 -> sweep_fast_kernel<DP, KIND, 1, 2, 256, 11>",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_fast_256_rpt3", env={"MGP_SWEEP_FAST": "1", "MGP_SWEEP_RPT": "3"}, entry="sweep",
         cases=ONE_RHS_CASES[:3], routes="D <= 8, RC 1, fnt 256, frpt 3 -> sweep_fast_kernel<DP, KIND, 1, 3, 256, 11>",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_rpt2_default_form", env={"MGP_SWEEP_RPT": "2"}, entry="sweep", cases=ONE_RHS_CASES[:3],
         same_as_default=True,
         routes="MGP_SWEEP_FAST=2, D <= 8, RC 1: the 512-thread RPT 4 kernel, grid sized for RPT 4 (the switch "
                "applies to MGP_SWEEP_FAST=1)", ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_rpt32_1", env={"MGP_SWEEP_RPT32": "1"}, entry="sweep", cases=D17_32_CASES,
         routes="16 < D <= 32, RC 1, frpt 1 -> sweep_fast_kernel<32, KIND, 1, 1, 256, 11, false>",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_rpt_rc3", env={"MGP_SWEEP_RPT_RC": "3"}, entry="sweep", cases=RC_CASES,
         routes="D <= 8, RC 2 or 4, frpt 3 -> sweep_fast_kernel<DP, KIND, RC, 3, 512, 13, true>",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_pf_every_trip", env={"MGP_PF_TRIPS": "1"}, entry="sweep", cases=VALU_CASES[:5],
         same_as_default=True, routes="fast kernel: pf_mask 0 (a prefetch every loop trip)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_pf_none", env={"MGP_PF_AHEAD": "0"}, entry="sweep", cases=VALU_CASES[5:],
         same_as_default=True, routes="fast kernel: prefetch distance 0", ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_pf_far", env={"MGP_PF_AHEAD": "1048576", "MGP_PF_TRIPS": "4"}, entry="sweep", cases=RC_CASES,
         same_as_default=True,
         routes="fast kernel: 1 MB ahead; the packed-point and weight reservations grow by pf_ahead (sweep.hip)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_chunking", env={}, entry="chunks", cases=CHUNK_CASES,
         routes="launch_sweep nchunks -> sweep_fast_kernel block decode (nchunks % 8 == 0 / <= 4 padded / linear)",
         ref="long double", bar="1e-11 (Matern-1/2 1e-9)"),
    dict(id="sweep_nosplit", env={"MGP_NOSPLIT_PER_CU": "1", "MGP_SWEEP_TARGET": "64"}, entry="sweep32",
         cases=[("se", 1, 262145, 257, 1)],
         routes="fp32 sweep_kernel: nblk = 257 >= 1 * 256 CUs -> one chunk (default: 2 chunks + reduce_few_partials)",
         ref="fp64", bar="2e-4"),
    # -------- kxx
    dict(id="kxx_min_n_0", env={"MGP_KXX_MIN_N": "0"}, entry="kxx", cases=[("matern32", 5, 1000), ("se", 8, 333)],
         routes="mgp_kxx_matvec: one column, N >= kxx_min_n -> the symmetric pair kernel (kxx.hip); equal to MGP_KXX=sym",
         ref="long double", bar="1e-11"),
    # -------- dense
    dict(id="tri_form_0", env={"MGP_TRI_MIN_N": "64", "MGP_TRI_FORM": "0"}, entry="symm1",
         cases=[64, 65, 100, 257, 1000, 1088],
         routes="symm_matmul_t: Bt 1, n >= tri_min_n -> symm_gemv_tri_kernel + symm_gemv_tri_reduce_kernel",
         ref="long double", bar="1e-13 (fp64), 2e-5 (fp32)"),
    dict(id="tri_form_1", env={"MGP_TRI_MIN_N": "64", "MGP_TRI_FORM": "1"}, entry="symm1",
         cases=[64, 65, 100, 257, 1000, 1088],
         routes="symm_matmul_t: Bt 1, n >= tri_min_n -> symm_gemv_tri_bfly_kernel + tile table",
         ref="long double", bar="1e-13 (fp64), 2e-5 (fp32)"),
    dict(id="skinny_reg", env={"MGP_SKINNY": "reg"}, entry="symm",
         cases=[(301, 2), (1001, 16), (301, 17), (1001, 33), (301, 64), (257, 65), (301, 128)],
         routes="symm_matmul_t: 2 <= Bt <= 128, skinny_mode 0 -> transpose_pad_kernel + symm_skinny_kernel<T, NBT>",
         ref="long double", bar="1e-12"),
    dict(id="skinny_bpc", env={"MGP_SKINNY_BPC": "3"}, entry="symm", cases=[(1001, 8), (1001, 40), (513, 100)],
         routes="symm_skinny_lds_launch: k slices from 3 workgroups per CU", ref="long double", bar="1e-12"),
    dict(id="skinny_stagger", env={"MGP_SKINNY_STAGGER": "50"}, entry="symm", cases=[(1001, 8), (1000, 3)],
         same_as_default=True, routes="symm_skinny_lds_kernel: start-up s_sleep per phase, same sums",
         ref="long double", bar="1e-12"),
    dict(id="skinny_stagger_max", env={"MGP_SKINNY_STAGGER": "100"}, entry="symm", cases=[(1001, 8), (4096, 40)],
         same_as_default=True, routes="stagger 100: no sleep, LDS and pipelined kernels as default",
         ref="long double", bar="1e-12"),
    dict(id="gemm_no_ksplit", env={"MGP_GEMM_KSPLIT": "0"}, entry="symm",
         cases=[(1001, 700), (530, 129), (999, 1000)],
         routes="gemm_nt_launch: gemm_ksplit 0 -> 64x64 tiles, no contraction slices (shapes of "
                "test_symm_matmul_ragged_gemm_regime)", ref="fp64 (as that test)", bar="1e-12"),
    dict(id="kdense_ta16", env={"MGP_KDENSE_TA": "16"}, entry="k_dense",
         cases=[("se", 3, 40, 300), ("matern12", 9, 63, 257), ("matern32", 17, 1, 65), ("matern52", 32, 63, 100)],
         routes="k_dense_t: ta 16 at every D", ref="long double", bar="1e-12 (fp64), 3e-5 (fp32)"),
    dict(id="kdense_ta64", env={"MGP_KDENSE_TA": "64"}, entry="k_dense",
         cases=[("se", 3, 40, 300), ("matern12", 8, 63, 257), ("matern32", 17, 1, 65), ("matern52", 9, 63, 100)],
         routes="k_dense_t: ta 64 at every D, also N < 64", ref="long double", bar="1e-12 (fp64), 3e-5 (fp32)"),
    # -------- CG on a dense matrix: (n, Bt)
    dict(id="skinny_defer_0", env={"MGP_SKINNY_DEFER": "0"}, entry="cg", cases=[(1500, 9), (1001, 40), (600, 16)],
         routes="cg.hip: Bt above the tile scheme's columns -> skinny product; slices reduced by skinny_reduce_kernel",
         ref="oracle/cg.py", bar="1e-9"),
    dict(id="d1_owner_spread_0", env={"MGP_D1_OWNER_SPREAD": "0"}, entry="cg", cases=[(3000, 3), (4001, 5), (2049, 2)],
         routes="cg_dense1.hip: 2048 < n <= 4096, Bt >= 2 -> super-block form, columns of a chunk owned by one workgroup",
         ref="oracle/cg.py", bar="1e-9"),
    dict(id="d1_first_poll", env={"MGP_D1_FIRST_POLL": "0"}, entry="cg", cases=[(1500, 1), (3000, 2)],
         same_as_default=True, routes="register-resident dense CG: no sleep before the owners' first poll",
         ref="oracle/cg.py", bar="1e-9"),
    dict(id="d1_first_poll_long", env={"MGP_D1_FIRST_POLL": "200"}, entry="cg", cases=[(2048, 1), (4096, 4)],
         same_as_default=True, routes="register-resident dense CG: a long sleep before the owners' first poll",
         ref="oracle/cg.py", bar="1e-9"),
    dict(id="tri_min_n_small_cg", env={"MGP_TRI_MIN_N": "64"}, entry="cg", cases=[(300, 1), (300, 3), (100, 2)],
         routes="mgp_dense1_eligible: n >= tri_min_n -> register-resident forms (cg_dense1.hip) below n = 1024",
         ref="oracle/cg.py", bar="1e-9"),
    # -------- contraction K_mn K_nm: (kind, D, N, M, dtype); N spans two full panels and a ragged tail
    dict(id="contract_panel_nz1", env={"MGP_CONTRACT_PANEL_MB": "1", "MGP_CONTRACT_NZ": "1"}, entry="contract",
         cases=[("se", 3, None, 77, "f64"), ("matern32", 8, None, 300, "f32")],
         routes="kmn_knm_two_stage: rc == rows -> NZ-sliced mgp_syrk_nt_upper, then the ragged tail",
         ref="long double", bar="1e-11 (fp64), 2e-4 (fp32)"),
    dict(id="contract_panel_nz3", env={"MGP_CONTRACT_PANEL_MB": "1", "MGP_CONTRACT_NZ": "3"}, entry="contract",
         cases=[("matern52", 2, None, 129, "f64"), ("se", 5, None, 1, "f32")],
         routes="as above, 3 slices", ref="long double", bar="1e-11 (fp64), 2e-4 (fp32)"),
    dict(id="contract_panel_nz16", env={"MGP_CONTRACT_PANEL_MB": "1", "MGP_CONTRACT_NZ": "16"}, entry="contract",
         cases=[("matern12", 3, None, 128, "f64"), ("matern52", 4, None, 77, "f32"), ("se", 2, None, 1, "f64")],
         routes="as above, 16 slices", ref="long double", bar="1e-11 (Matern-1/2 1e-9; fp32 2e-4)"),
    dict(id="contract_panel_nz64", env={"MGP_CONTRACT_PANEL_MB": "1", "MGP_CONTRACT_NZ": "64"}, entry="contract",
         cases=[("se", 8, None, 300, "f64"), ("matern32", 3, None, 129, "f32")],
         routes="as above, 64 slices", ref="long double", bar="1e-11 (fp64), 2e-4 (fp32)"),
    dict(id="contract_fused", env={"MGP_CONTRACT": "fused"}, entry="contract",
         cases=[("se", 8, 3001, 77, "f64"), ("matern32", 17, 1000, 129, "f64"), ("matern52", 3, 2000, 300, "f32")],
         routes="mgp_kmn_knm: MGP_CONTRACT=fused (read per call), D <= 32 -> kmn_knm_t (contract.hip)",
         ref="long double", bar="1e-11 (fp64), 2e-4 (fp32)"),
    # -------- multi-rank SGPR step on a one-rank communicator
    dict(id="fuse_agree_0", env={"MGP_FUSE_AGREE": "0"}, entry="comm", cases=[("f64",), ("f32",)],
         same_as_default=True,
         routes="cg.hip: coll && !fuse_agree -> put_gate_word_kernel and finish_allreduce_kernel as launches of their own",
         ref="the fused form and the no-collective solve", bar="bitwise"),
]


@contextlib.contextmanager
def switched(monkeypatch, env):
    """A handle made under `env`, installed as the handle of device 0 for the duration (GPU tests only: torch and
    the library are imported here, so that the CPU inventory test can read the table without them)."""
    import torch

    from cggp import _hip
    _hip.get_handle(torch.device("cuda:0"))  # the default handle exists first, so it can be restored
    prev = _hip._handles.get(0)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        hd = _hip.Handle(0)
        _hip._handles[0] = hd
        try:
            yield hd
        finally:
            torch.cuda.synchronize()
            _hip._handles[0] = prev
            hd.lib.mgp_destroy(hd.h)
            hd.h = None


def table_switches():
    """Every variable some row sets."""
    out = set()
    for row in FORMS:
        out.update(row["env"])
        if row["entry"] == "chunks":
            for case in row["cases"]:
                out.update(case[0])
    return out


# Switches with no row: the value is the node id of the existing test that covers them, or a reason.
EXEMPT = {
    "MGP_D1_INJECT_ABSENT":
        "tests/test_gpu_dense1.py::test_a_missing_workgroup_makes_the_register_resident_solve_fail_over_not_hang",
    "MGP_CG_DENSE1": "tests/test_gpu_dense1.py::test_every_form_of_the_dense_cg_gives_the_oracle_steps",
    "MGP_CG_DENSE1_COLS": "tests/test_gpu_dense1.py::test_every_form_of_the_dense_cg_gives_the_oracle_steps",
    "MGP_CG_PIPELINE_POLLS": "tests/test_gpu_dense1.py::test_every_form_of_the_dense_cg_gives_the_oracle_steps",
    "MGP_KXX": "tests/test_gpu_gpr.py::test_kxx_against_sweep_at_size",
    "MGP_KXX_GRAD": "tests/test_gpu_gpr_lml.py::test_kxx_grad_routes_and_determinism",
    "MGP_RFF_ROUTE": "tests/test_gpu_rff.py::test_rff_parity",
    "MGP_SKINNY_PIPE": "tests/test_gpu_parity.py::test_symm_matmul_pipelined_form",
    "MGP_SGPR_KMM_ASIDE": "tests/test_gpu_parity.py::test_sgpr_kmm_product_beside_the_sweep_at_small_sizes",
    "MGP_D1_TRACE": "diagnosis output: writes a per-iteration timeline file and drains the stream; no result changes",
}
# MGP_SKINNY_STAGGER 101..107 (dense.hip, symm_skinny_lds_launch) are not rows either: 101-104 are ablations that
# drop the MFMAs, the loads after the first step, the barriers or the LDS operand reads -- their results are wrong
# on purpose and only their timing is of use; 105-107 write per-workgroup timelines behind the slice partials and
# give correct results (with one k slice they now run the plain kernels, since there is no slice buffer to hold
# the timeline).  Rows 1-100 are the `skinny_stagger*` rows above.
