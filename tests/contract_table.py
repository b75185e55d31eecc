"""The buffer contract of every exported function of include/*.h that takes a device pointer, one row each.

A row names the device inputs and outputs of its entry point, the regions of every output the header documents as
written and as untouched, the reference and the bar of the test that already covers the arithmetic (quoted by test
name; no bar here is looser), the shapes, whether a host dispatch reads a pointer value (then the results at two base
alignments agree to the bar only, otherwise bit for bit), which of the handle's reused arenas the cases reach, and how
a stale-arena run poisons them.  tests/test_gpu_buffer_contract.py runs three families over the table;
tests/test_contract_table_host.py checks it against the header.

Importing this module needs no GPU: arrays are numpy, calls are made through the ctypes library the caller passes."""

import ctypes
import math
import zlib

import numpy as np

from cggp import _hip
from oracle import cg as ocg
from oracle import distance as od
from oracle import kernels as ok

# the bars of the tests that already cover the arithmetic, imported where they exist as names
from test_gpu_gpr import bar as kxx_bar  # noqa: E402  (long-double products: 1e-11, Matern-1/2 1e-7)
from test_gpu_rff import U as _RFF_U  # noqa: E402
from test_gpu_switch_forms import product_bar  # noqa: E402  (oracle products: 1e-11, Matern-1/2 1e-9)

import torch  # noqa: E402

LD = np.longdouble
NP = {"f64": np.float64, "f32": np.float32}
CODE = {"f64": _hip.F64, "f32": _hip.F32}
U = {"f64": _RFF_U[torch.float64], "f32": _RFF_U[torch.float32]}  # the unit roundoffs of the rff bound
COLS, ROWS = _hip.COLS, _hip.ROWS
ARENAS = ("ws", "cg", "opws", "kxx", "kgrad", "pch", "prj", "gen", "pack")
VAR = 1.3

# exported functions that take no caller-owned device buffer (or none whose contents the call defines)
EXCLUDED = {
    "mgp_version": "handle: no pointer", "mgp_create": "handle", "mgp_create_ex": "handle",
    "mgp_workspace_bytes": "handle", "mgp_arena_bytes": "handle: host string only",
    "mgp_destroy": "handle", "mgp_set_stream": "handle",
    "mgp_last_error": "handle", "mgp_build_arch": "handle",
    "mgp_profile_enable": "profile: host pointers only", "mgp_profile_read": "profile: host pointers only",
    "mgp_profile_read_each": "profile: host pointers only", "mgp_profile_read_clocks": "profile: host pointers only",
    "mgp_comm_unique_id": "comm: needs several GPUs (tests/test_gpu_rccl.py)",
    "mgp_comm_init_rank": "comm", "mgp_comm_init_all": "comm", "mgp_comm_destroy": "comm", "mgp_comm_size": "comm",
    "mgp_comm_rank": "comm", "mgp_comm_group_begin": "comm", "mgp_comm_group_end": "comm",
    "mgp_allreduce_sum": "comm: in place by definition, needs several GPUs (tests/test_gpu_rccl.py)",
    "mgp_comm_last_error": "comm",
    "mgp_host_last_error": "host cover tree", "mgp_covertree_build": "host cover tree: host pointers only",
    "mgp_covertree_destroy": "host cover tree", "mgp_covertree_num_levels": "host cover tree",
    "mgp_covertree_level_size": "host cover tree", "mgp_covertree_level_radius": "host cover tree",
    "mgp_covertree_level_nodes": "host cover tree: host outputs",
    "mgp_covertree_level_rows": "host cover tree: host outputs",
    "mgp_covertree_build_device": "reads x_dev only; every output is a host-side tree (tests/test_gpu_covertree.py "
                                  "compares it node for node with the host build)",
}


def rnd(a, dt):
    """the values the device sees, as float64"""
    return np.asarray(a, dtype=NP[dt]).astype(np.float64)


def relerr(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


def points(rng, n, D):
    return rng.standard_normal((n, D))


def lengthscales(rng, D):
    return 0.6 + rng.random(D) * math.sqrt(D)


def kstruct(kind, dt, D, ls, var=VAR):
    return _hip.make_kernel_struct(kind, CODE[dt], D, var, list(ls))


def full(shape):
    return np.ones(shape, dtype=bool)


def none(shape):
    return np.zeros(shape, dtype=bool)


def kbar(kind, dt, f64=1e-12, f32=2e-4, m12=1e-9):
    """fp64 kernel products against the float64 oracle: 1e-12 (Matern-1/2: the 1e-9 of test_knm_kmn_matvec_fp64, the
    sqrt of GPflow's cancelled squared distance, in the oracle as much as here); fp32: the 2e-4 of test_sweep_fp32"""
    if dt == "f32":
        return f32
    return min(m12 if kind == "matern12" else f64, product_bar(kind))  # never looser than the project's own


class Row:
    """Defaults of a table row; `cases` is a list of dicts, `ins` / `outs` name the device buffers of a case."""
    name = None
    dtypes = ("f64", "f32")
    arenas = ()           # arenas of the handle the cases reach
    poison = "nan"        # stale-arena run: "nan" = the same case with NaN inputs in the other dtype; "finite" =
                          # `poison_case` (a larger finite problem), where NaN has no meaning or fp64 is the only dtype
    poison_case = None
    poison_keep = ()      # inputs a "nan" poison leaves finite
    host_scalars = False  # returns host values after synchronising the stream
    cases = ()
    missing = {}          # family -> reason, where a family does not apply

    def seed(self, c):
        # a stable hash (str hashes are salted per process; the inputs of a case must not change between runs)
        return zlib.crc32(repr((self.name, sorted((k, str(v)) for k, v in c.items()))).encode()) & 0x7FFFFFFF

    def ins(self, c, dt, rng):
        raise NotImplementedError

    def outs(self, c, dt):
        """name -> (allocated shape, "T" | "i64")"""
        raise NotImplementedError

    def call(self, lib, h, c, dt, p):
        """p[name] -> c_void_p of every device buffer (None for one the case leaves NULL); returns (rc, host values)"""
        raise NotImplementedError

    def reference(self, c, dt, ins):
        raise NotImplementedError

    def check(self, c, dt, ins, got, ref):
        """assert the bar; return name -> written mask (True written / False untouched) for every output"""
        raise NotImplementedError

    def reads_pointer(self, c, dt):
        """a host dispatch of this case reads a pointer value: two base alignments agree to the bar, not bit for bit"""
        return False

    def route(self, c, dt, ptrs, num_cus=256):
        """which dispatch the host is expected to take, for cases that read a pointer (printed by the test; a
        restatement of csrc/dense.hip for the reader of a log, not something the library reports)"""
        return ""


def _vec(layout, n, R):
    return (n, R) if layout == COLS else (R, n)


def _as_cols(a, layout):
    return a if layout == COLS else a.T


# ---------------------------------------------------------------------------------------------------- sweeps
class _Sweep(Row):
    """mgp_knm_matvec / mgp_kmn_matvec: out = k(X, Z) V or k(Z, X) W"""
    arenas = ("pack", "gen", "ws")  # fp64 D <= 32: packed streamed set, transposed weights (R > 1), chunk partials;
                                    # D = 33: the generic panels
    cases = [dict(N=1, M=1, R=1, D=1, kind="se", layout=COLS),
             dict(N=65, M=37, R=3, D=5, kind="matern32", layout=ROWS),
             dict(N=777, M=130, R=8, D=17, kind="matern52", layout=COLS),
             dict(N=4097, M=130, R=11, D=32, kind="se", layout=ROWS),
             dict(N=777, M=37, R=3, D=33, kind="se", layout=COLS),
             dict(N=4097, M=37, R=1, D=5, kind="matern12", layout=COLS)]
    transpose = False

    def ins(self, c, dt, rng):
        nv = c["N"] if self.transpose else c["M"]
        return dict(X=points(rng, c["N"], c["D"]), Z=points(rng, c["M"], c["D"]),
                    V=rng.standard_normal(_vec(c["layout"], nv, c["R"])), _ls=lengthscales(rng, c["D"]))

    def outs(self, c, dt):
        return dict(out=(_vec(c["layout"], c["M"] if self.transpose else c["N"], c["R"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        fn = lib.mgp_kmn_matvec if self.transpose else lib.mgp_knm_matvec
        return fn(h, ctypes.byref(k), p["X"], c["N"], p["Z"], c["M"], p["V"], c["R"], c["layout"], p["out"],
                  c["layout"]), {}

    def reference(self, c, dt, ins):
        K = ok.Kernel(c["kind"], VAR, ins["_ls"]).K(rnd(ins["X"], dt), rnd(ins["Z"], dt))
        V = _as_cols(rnd(ins["V"], dt), c["layout"])
        return (K.T if self.transpose else K) @ V

    def check(self, c, dt, ins, got, ref):
        e = relerr(_as_cols(got["out"], c["layout"]), ref)
        assert e < kbar(c["kind"], dt), (self.name, c, dt, e)
        return dict(out=None)


class KnmMatvec(_Sweep):
    name = "mgp_knm_matvec"


class KmnMatvec(_Sweep):
    name = "mgp_kmn_matvec"
    transpose = True
    cases = _Sweep.cases + [dict(N=0, M=37, R=3, D=5, kind="se", layout=COLS)]  # a rank without rows: zeros written


class KDense(Row):
    """out[na, ld >= nb] = k(A, B) (+ jitter, + diag_add on the diagonal); columns nb..ld-1 untouched"""
    name = "mgp_k_dense"
    arenas = ()
    missing = {"B": "needs no scratch: every element of the block is a function of one row of A and one of B"}
    cases = [dict(na=65, nb=37, D=5, kind="se", pad=3, diag=False),
             dict(na=777, nb=130, D=17, kind="matern32", pad=1, diag=False),
             dict(na=130, nb=130, D=33, kind="matern52", pad=5, diag=True),
             dict(na=37, nb=37, D=1, kind="se", pad=1, diag=True),
             dict(na=4097, nb=1, D=1, kind="se", pad=1, diag=False),
             dict(na=1, nb=37, D=32, kind="matern12", pad=0, diag=False)]
    JITTER = 1e-3

    def ins(self, c, dt, rng):
        d = dict(A=points(rng, c["na"], c["D"]), _ls=lengthscales(rng, c["D"]))
        d["B"] = points(rng, c["nb"], c["D"])
        if c["diag"]:
            d["B"] = d["A"].copy()  # the diagonal terms belong to a self block, as Kuu builds it
            d["diag_add"] = rng.random(c["na"]) + 0.1
        return d

    def outs(self, c, dt):
        return dict(out=((c["na"], c["nb"] + c["pad"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_k_dense(h, ctypes.byref(k), p["A"], c["na"], p["B"], c["nb"], p["out"], c["nb"] + c["pad"],
                               self.JITTER if c["diag"] else 0.0, p.get("diag_add")), {}

    def reference(self, c, dt, ins):
        K = ok.Kernel(c["kind"], VAR, ins["_ls"]).K(rnd(ins["A"], dt), rnd(ins["B"], dt))
        if c["diag"]:
            K = K + self.JITTER * np.eye(c["na"]) + np.diag(rnd(ins["diag_add"], dt))
        return K

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"][:, :c["nb"]], ref)
        # test_k_dense: 1e-12 / 3e-5 (no Matern-1/2 case here has coincident points)
        assert e < (1e-12 if dt == "f64" else 3e-5), (self.name, c, dt, e)
        m = none((c["na"], c["nb"] + c["pad"]))
        m[:, :c["nb"]] = True
        return dict(out=m)


class _Contract(Row):
    cases = [dict(N=777, M=37, D=5, kind="se"), dict(N=4097, M=130, D=17, kind="matern32"),
             dict(N=65, M=1, D=1, kind="se"), dict(N=1, M=37, D=32, kind="matern52"),
             dict(N=777, M=130, D=33, kind="se")]

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), Z=points(rng, c["M"], c["D"]), _ls=lengthscales(rng, c["D"]))

    def _K(self, c, dt, ins):
        return ok.Kernel(c["kind"], VAR, ins["_ls"]).K(rnd(ins["X"], dt), rnd(ins["Z"], dt))


class KmnKnm(_Contract):
    """out[M, M] = K_mn K_nm"""
    name = "mgp_kmn_knm"
    arenas = ("opws",)  # the K^T row panel, the contraction slices and the tile table

    def outs(self, c, dt):
        return dict(out=((c["M"], c["M"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_kmn_knm(h, ctypes.byref(k), p["X"], c["N"], p["Z"], c["M"], p["out"]), {}

    def reference(self, c, dt, ins):
        K = self._K(c, dt, ins)
        return K.T @ K

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        # test_kmn_knm, test_kmn_knm_fp32_and_ragged
        assert e < (product_bar(c["kind"]) if dt == "f64" else 2e-4), (self.name, c, dt, e)
        return dict(out=None)


class KmnSqColsum(_Contract):
    """out[M] = sum_i k(x_i, z_m)^2"""
    name = "mgp_kmn_sq_colsum"
    arenas = ("ws", "gen")

    def outs(self, c, dt):
        return dict(out=((c["M"],), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_kmn_sq_colsum(h, ctypes.byref(k), p["X"], c["N"], p["Z"], c["M"], p["out"]), {}

    def reference(self, c, dt, ins):
        K = self._K(c, dt, ins)
        return np.sum(K * K, axis=0)

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        assert e < (product_bar(c["kind"]) if dt == "f64" else 2e-4), (self.name, c, dt, e)  # as test_gpu_switch_forms
        return dict(out=None)


# ------------------------------------------------------------------------------------------------ exact GPR
class KxxMatvec(Row):
    """out = (k(X, X) + s2 I) V; on a MGP_KXX=sym handle fp64 with one column runs csrc/kxx.hip"""
    name = "mgp_kxx_matvec"
    arenas = ("kxx", "ws")  # fp64 on a MGP_KXX=sym handle: csrc/kxx.hip; fp32: the sweep's chunk partials
    S2 = 0.37
    cases = [dict(N=4097, D=5, R=1, kind="se", layout=COLS), dict(N=777, D=17, R=3, kind="matern32", layout=ROWS),
             dict(N=65, D=32, R=1, kind="matern52", layout=ROWS), dict(N=1, D=1, R=1, kind="se", layout=COLS),
             dict(N=777, D=1, R=1, kind="matern32", layout=ROWS),
             dict(N=0, D=5, R=3, kind="se", layout=COLS)]  # N = 0 writes nothing (output allocated for 2 rows)

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), V=rng.standard_normal(_vec(c["layout"], c["N"], c["R"])),
                    _ls=lengthscales(rng, c["D"]))

    def outs(self, c, dt):
        return dict(out=(_vec(c["layout"], c["N"] or 2, c["R"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_kxx_matvec(h, ctypes.byref(k), p["X"], c["N"], self.S2, p["V"], c["R"], c["layout"], p["out"],
                                  c["layout"]), {}

    def reference(self, c, dt, ins):
        from gpr_reference import kxx_product
        if c["N"] == 0:
            return None
        V = _as_cols(rnd(ins["V"], dt), c["layout"])
        return np.asarray(kxx_product(c["kind"], VAR, ins["_ls"], rnd(ins["X"], dt), self.S2, V), dtype=np.float64)

    def check(self, c, dt, ins, got, ref):
        if c["N"] == 0:
            return dict(out=none(got["out"].shape))
        e = relerr(_as_cols(got["out"], c["layout"]), ref)
        # tests/test_gpu_gpr.py bar(kind) against the long-double product; fp32: the sweep's 2e-4
        assert e < (2e-4 if dt == "f32" else kxx_bar(c["kind"])), (self.name, c, dt, e)
        return dict(out=None)


class KxxPivchol(Row):
    """L[max_rank, N], piv[max_rank], diag[N] (may be NULL), host rank; rows / entries from the rank on untouched"""
    name = "mgp_kxx_pivchol"
    dtypes = ("f64",)
    arenas = ("pch",)
    poison = "finite"  # the pivot search compares: NaN has no defined order, and the entry point is fp64 only
    poison_case = dict(N=5001, D=5, kind="matern52", max_rank=70, rel_tol=0.0, diag=True)
    host_scalars = True
    cases = [dict(N=777, D=1, kind="se", max_rank=64, rel_tol=1e-4, diag=True),  # stops early: untouched rows
             dict(N=4097, D=5, kind="matern32", max_rank=11, rel_tol=0.0, diag=True),
             dict(N=65, D=33, kind="se", max_rank=8, rel_tol=0.0, diag=False),
             dict(N=1, D=5, kind="se", max_rank=3, rel_tol=0.0, diag=True)]

    def ins(self, c, dt, rng):
        # U(-3, 3)^D with lengthscales ~ sqrt(D): the inputs of tests/test_gpu_pivchol.py, whose RANKS table keeps the
        # residual maximum meaningful (D = 1: rank <= 12, reached here through rel_tol)
        return dict(X=rng.uniform(-3.0, 3.0, (c["N"], c["D"])),
                    _ls=np.linspace(0.8, 1.6, c["D"]) * math.sqrt(c["D"]))

    def outs(self, c, dt):
        rows = min(c["max_rank"], c["N"])
        d = dict(L=((rows, c["N"]), "T"), piv=((rows,), "i64"))
        if c["diag"]:
            d["diag"] = ((c["N"],), "T")
        return d

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        rank = ctypes.c_int32(-1)
        rc = lib.mgp_kxx_pivchol(h, ctypes.byref(k), p["X"], c["N"], c["max_rank"], c["rel_tol"], p["L"], p["piv"],
                                 p.get("diag"), ctypes.byref(rank))
        return rc, dict(rank=rank.value)

    def reference(self, c, dt, ins):
        from pivchol_reference import greedy_pivoted_cholesky, kernel_matrix
        K = kernel_matrix(c["kind"], VAR, ins["_ls"], ins["X"], dtype=np.float64)
        return len(greedy_pivoted_cholesky(K, c["max_rank"], c["rel_tol"])[1])

    def check(self, c, dt, ins, got, ref):
        from pivchol_reference import forced_pivoted_cholesky, kernel_rows
        N, rank = c["N"], got["rank"]
        rows = min(c["max_rank"], N)
        assert rank == ref, (self.name, c, rank, ref)  # test_rel_tol_stop_matches_the_reference...
        assert 0 < rank <= rows and (c["rel_tol"] == 0.0 or rank < rows)
        piv = got["piv"][:rank]
        assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < N
        kr = kernel_rows(c["kind"], VAR, ins["_ls"], ins["X"], piv)
        where = {int(q): i for i, q in enumerate(piv)}
        Lr, before, dr = forced_pivoted_cholesky(lambda q: kr[where[q]], np.full(N, LD(VAR)), [int(q) for q in piv])
        err = float(np.max(np.abs(got["L"][:rank].astype(LD) - Lr)))
        assert err <= 1e-10 * math.sqrt(VAR), (self.name, c, err)  # test_factor_against_long_double_with_forced_pivots
        written = dict(L=np.repeat((np.arange(rows) < rank)[:, None], N, axis=1), piv=np.arange(rows) < rank)
        if c["diag"]:
            assert float(np.max(np.abs(got["diag"].astype(LD) - dr))) <= 1e-10
            written["diag"] = None
        return written


class LowrankApply(Row):
    """Z[Bt, n] = diag_inv o R - (R B^T) B"""
    name = "mgp_lowrank_apply"
    arenas = ("pch",)
    cases = [dict(Bt=1, k=1, n=1), dict(Bt=5, k=33, n=777), dict(Bt=16, k=8, n=4097), dict(Bt=3, k=3, n=65),
             dict(Bt=40, k=11, n=777), dict(Bt=0, k=3, n=65)]  # Bt = 0 writes nothing (output allocated for one row)

    def ins(self, c, dt, rng):
        return dict(diag_inv=0.5 + rng.random(c["n"]), B=rng.standard_normal((c["k"], c["n"])) / math.sqrt(c["n"]),
                    R=rng.standard_normal((max(c["Bt"], 1), c["n"])))

    def outs(self, c, dt):
        return dict(Z=((max(c["Bt"], 1), c["n"]), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_lowrank_apply(h, CODE[dt], p["diag_inv"], p["B"], c["k"], c["n"], p["R"], c["Bt"], p["Z"]), {}

    def reference(self, c, dt, ins):
        dinv, B, R = rnd(ins["diag_inv"], dt), rnd(ins["B"], dt), rnd(ins["R"], dt)
        return dinv[None, :] * R - (R @ B.T) @ B, np.abs(dinv[None, :] * R) + (np.abs(R) @ np.abs(B).T) @ np.abs(B)

    def check(self, c, dt, ins, got, ref):
        if c["Bt"] == 0:
            return dict(Z=none(got["Z"].shape))
        val, scale = ref
        e = float(np.max(np.abs(got["Z"].astype(np.float64) - val) / scale))
        assert e <= (1e-12 if dt == "f64" else 1e-5), (self.name, c, dt, e)  # test_lowrank_apply_against_numpy
        return dict(Z=None)


class KnmProject(Row):
    """proj[B, r] = k(Xs, X) R, sqnorm[b] = |proj[b]|^2; either may be NULL"""
    name = "mgp_knm_project"

    def reads_pointer(self, c, dt):
        # generic route (fp32, D > 32, r > 256): R and the panels enter the NT GEMM, whose vector form reads alignments
        return dt == "f32" or c["D"] > 32 or c["r"] > 256
    arenas = ("prj", "ws")
    cases = [dict(B=65, N=777, D=5, r=64, kind="se", layout=COLS, null=()),           # fused
             dict(B=130, N=777, D=17, r=257, kind="matern32", layout=ROWS, null=()),   # generic (r > 256)
             dict(B=37, N=4097, D=32, r=11, kind="matern52", layout=ROWS, null=("proj",)),
             dict(B=1, N=65, D=1, r=1, kind="se", layout=COLS, null=("sqnorm",)),
             dict(B=37, N=130, D=33, r=8, kind="se", layout=COLS, null=()),            # generic (D > 32)
             dict(B=0, N=65, D=5, r=8, kind="se", layout=COLS, null=())]               # B = 0 writes nothing

    def ins(self, c, dt, rng):
        return dict(Xs=points(rng, max(c["B"], 1), c["D"]), X=points(rng, c["N"], c["D"]),
                    R=rng.standard_normal(_vec(c["layout"], c["N"], c["r"])), _ls=lengthscales(rng, c["D"]))

    def outs(self, c, dt):
        d = dict(proj=((max(c["B"], 1), c["r"]), "T"), sqnorm=((max(c["B"], 1),), "T"))
        return {k: v for k, v in d.items() if k not in c["null"]}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_knm_project(h, ctypes.byref(k), p["Xs"], c["B"], p["X"], c["N"], p["R"], c["r"], c["layout"],
                                   p.get("proj"), p.get("sqnorm")), {}

    def reference(self, c, dt, ins):
        from love_reference import knm_project
        pr, sq = knm_project(c["kind"], VAR, ins["_ls"], rnd(ins["Xs"], dt), rnd(ins["X"], dt),
                             _as_cols(rnd(ins["R"], dt), c["layout"]))
        return np.asarray(pr, dtype=np.float64), np.asarray(sq, dtype=np.float64)

    def check(self, c, dt, ins, got, ref):
        names = [n for n in ("proj", "sqnorm") if n not in c["null"]]
        if c["B"] == 0:
            return {n: none(got[n].shape) for n in names}
        # tests/test_gpu_love.py: bar(kind) of test_project_matches_longdouble, 2e-4 of the fp32 test
        bar = 2e-4 if dt == "f32" else kxx_bar(c["kind"])
        for n, r in zip(("proj", "sqnorm"), ref):
            if n in names:
                e = relerr(got[n], r)
                assert e < bar, (self.name, c, dt, n, e)
        return {n: None for n in names}

    def route(self, c, dt, ptrs, num_cus=256):
        return "fused" if (dt == "f64" and c["D"] <= 32 and c["r"] <= 256) else "generic (panels + NT GEMM)"


class KxxGrad(Row):
    """host dvariance, dlengthscales[D] = sum_r u_r^T dK/dtheta v_r"""
    name = "mgp_kxx_grad"
    arenas = ("kgrad", "ws")  # fused: packed rows and partials; fp32 / D = 33: a panel of U V^T, then mgp_k_dense_vjp
    host_scalars = True
    cases = [dict(N=777, D=17, R=5, kind="se", layout=COLS), dict(N=4097, D=1, R=1, kind="matern32", layout=ROWS),
             dict(N=65, D=32, R=3, kind="matern52", layout=COLS), dict(N=1, D=1, R=1, kind="se", layout=COLS),
             dict(N=130, D=33, R=8, kind="se", layout=ROWS)]

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), U=rng.standard_normal(_vec(c["layout"], c["N"], c["R"])),
                    V=rng.standard_normal(_vec(c["layout"], c["N"], c["R"])), _ls=np.linspace(0.6, 1.4, c["D"]))

    def outs(self, c, dt):
        return {}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        dv, dl = ctypes.c_double(float("nan")), (ctypes.c_double * _hip.MGP_MAX_D)()
        rc = lib.mgp_kxx_grad(h, ctypes.byref(k), p["X"], c["N"], p["U"], p["V"], c["R"], c["layout"], ctypes.byref(dv),
                              dl)
        return rc, dict(dv=dv.value, dl=np.array([dl[d] for d in range(c["D"])]))

    def reference(self, c, dt, ins):
        from lml_reference import kxx_grad_reference
        return kxx_grad_reference(c["kind"], VAR, ins["_ls"], rnd(ins["X"], dt),
                                  _as_cols(rnd(ins["U"], dt), c["layout"]), _as_cols(rnd(ins["V"], dt), c["layout"]))

    def check(self, c, dt, ins, got, ref):
        rv, rl, sv, sl = ref
        bar = 1e-11 if dt == "f64" else 1e-5  # test_kxx_grad_against_long_double and its fp32 lines
        assert abs(got["dv"] - float(rv)) <= bar * float(sv), (self.name, c, dt, got["dv"], float(rv))
        for d in range(c["D"]):
            assert abs(got["dl"][d] - float(rl[d])) <= bar * max(float(sl[d]), 1e-300), (self.name, c, dt, d)
        return {}


class KmnKnmVjp(Row):
    """host dvariance, dlengthscales; dZ[M, D] (may be NULL); Y / Gb optional"""
    name = "mgp_kmn_knm_vjp"
    dtypes = ("f64",)

    def reads_pointer(self, c, dt):
        return c["P"] > 0  # W = K G2 + Y Gb^T: Y and Gb enter the NT GEMM, whose vector form reads their alignment
    arenas = ("kgrad",)
    poison = "finite"  # fp64 only: a larger finite problem
    poison_case = dict(N=4500, M=140, D=32, P=16, kind="matern52", dZ=True)
    host_scalars = True
    cases = [dict(N=777, M=37, D=5, P=2, kind="se", dZ=True), dict(N=4097, M=130, D=17, P=0, kind="matern32", dZ=True),
             dict(N=65, M=1, D=1, P=1, kind="se", dZ=False), dict(N=1, M=37, D=32, P=16, kind="matern52", dZ=True)]

    def ins(self, c, dt, rng):
        d = dict(X=points(rng, c["N"], c["D"]), Z=points(rng, c["M"], c["D"]), Gq=rng.standard_normal((c["M"], c["M"])),
                 _ls=lengthscales(rng, c["D"]))
        if c["P"]:
            d["Y"], d["Gb"] = rng.standard_normal((c["N"], c["P"])), rng.standard_normal((c["M"], c["P"]))
        return d

    def outs(self, c, dt):
        return dict(dZ=((c["M"], c["D"]), "T")) if c["dZ"] else {}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        dv, dl = ctypes.c_double(float("nan")), (ctypes.c_double * _hip.MGP_MAX_D)()
        rc = lib.mgp_kmn_knm_vjp(h, ctypes.byref(k), p["X"], c["N"], p["Z"], c["M"], p["Gq"], p.get("Y"), p.get("Gb"),
                                 c["P"], ctypes.byref(dv), dl, p.get("dZ"))
        return rc, dict(dv=dv.value, dl=np.array([dl[d] for d in range(c["D"])]))

    def reference(self, c, dt, ins):
        from sgpr_grad_reference import kmn_knm_vjp_reference
        return kmn_knm_vjp_reference(c["kind"], VAR, ins["_ls"], ins["X"], ins["Z"], ins["Gq"], ins.get("Y"),
                                     ins.get("Gb"))

    def check(self, c, dt, ins, got, ref):
        rv, rl, rz, sv, sl, sz = ref  # test_kmn_knm_vjp_against_long_double: 1e-10 of the sum of |terms|
        f = lambda a: np.asarray(a, dtype=np.float64)
        assert abs(got["dv"] - float(rv)) <= 1e-10 * float(sv), (self.name, c, got["dv"], float(rv))
        assert np.all(np.abs(got["dl"] - f(rl)) <= 1e-10 * f(sl)), (self.name, c)
        if c["dZ"]:
            assert np.all(np.abs(got["dZ"] - f(rz)) <= 1e-10 * f(sz) + 1e-300), (self.name, c)
            return dict(dZ=None)
        return {}

    def route(self, c, dt, ptrs, num_cus=256):
        return "panel GEMMs (vector form by alignment of Y, Gb)" if c["P"] else "panel GEMM on arena operands"


class KDenseVjp(Row):
    """host dvariance, dlengthscales for G = dL/dK [na, ldg]; pad columns nb..ldg-1 of G are never read"""
    name = "mgp_k_dense_vjp"
    arenas = ("ws",)
    host_scalars = True
    cases = [dict(na=777, nb=130, D=5, kind="se", pad=3), dict(na=1, nb=37, D=17, kind="matern32", pad=1),
             dict(na=4097, nb=1, D=1, kind="matern52", pad=1), dict(na=65, nb=37, D=33, kind="se", pad=2),
             dict(na=130, nb=65, D=32, kind="matern12", pad=0)]

    def ins(self, c, dt, rng):
        G = np.full((c["na"], c["nb"] + c["pad"]), np.nan)  # NaN in the pad columns: it must not reach the result
        G[:, :c["nb"]] = rng.standard_normal((c["na"], c["nb"]))
        return dict(A=points(rng, c["na"], c["D"]), B=points(rng, c["nb"], c["D"]) + 0.3, G=G,
                    _ls=np.linspace(0.7, 1.3, c["D"]) * math.sqrt(c["D"]))

    def outs(self, c, dt):
        return {}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"], var=1.4)
        dv, dl = ctypes.c_double(float("nan")), (ctypes.c_double * _hip.MGP_MAX_D)()
        rc = lib.mgp_k_dense_vjp(h, ctypes.byref(k), p["A"], c["na"], p["B"], c["nb"], p["G"], c["nb"] + c["pad"],
                                 ctypes.byref(dv), dl)
        return rc, dict(dv=dv.value, dl=np.array([dl[d] for d in range(c["D"])]))

    def reference(self, c, dt, ins):
        from sgpr_grad_reference import k_dense_vjp_reference
        return k_dense_vjp_reference(c["kind"], 1.4, ins["_ls"], rnd(ins["A"], dt), rnd(ins["B"], dt),
                                     rnd(ins["G"][:, :c["nb"]], dt))

    def check(self, c, dt, ins, got, ref):
        rv, rl, sv, sl = ref
        bar = 1e-10 if dt == "f64" else 2e-4  # test_k_dense_vjp_against_long_double
        assert np.isfinite(got["dv"]) and np.all(np.isfinite(got["dl"])), (self.name, c, dt)
        assert abs(got["dv"] - float(rv)) <= bar * float(sv), (self.name, c, dt, got["dv"], float(rv))
        assert np.all(np.abs(got["dl"] - rl.astype(np.float64)) <= bar * sl.astype(np.float64)), (self.name, c, dt)
        return {}


# --------------------------------------------------------------------------------------------- dense product, CG
def _spd(rng, n):
    Q = rng.standard_normal((n, n))
    return Q @ Q.T / n + 2.0 * np.eye(n)  # the well-conditioned matrix of test_cg_fixed_iterations_match_oracle


class SymmMatmul(Row):
    """out[Bt, n] = P[Bt, n] @ A for symmetric A"""
    name = "mgp_symm_matmul"

    def reads_pointer(self, c, dt):
        return True  # dense.hip: gemm_vec_ok (Bt > 128), the skinny forms (2 <= Bt <= 128), the row GEMV (Bt = 1)
    arenas = ("ws",)
    cases = [dict(n=200, Bt=1), dict(n=200, Bt=5), dict(n=1001, Bt=1), dict(n=1001, Bt=5), dict(n=1024, Bt=1),
             dict(n=256, Bt=130), dict(n=1, Bt=1), dict(n=65, Bt=37)]

    def ins(self, c, dt, rng):
        A = rng.standard_normal((c["n"], c["n"]))
        return dict(A=A + A.T, P=rng.standard_normal((c["Bt"], c["n"])))

    def outs(self, c, dt):
        return dict(out=((c["Bt"], c["n"]), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_symm_matmul(h, CODE[dt], p["A"], c["n"], p["P"], c["Bt"], p["out"]), {}

    def reference(self, c, dt, ins):
        return rnd(ins["P"], dt) @ rnd(ins["A"], dt)

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        assert e < (1e-12 if dt == "f64" else 1e-4), (self.name, c, dt, e)  # test_symm_matmul_fp64 / _fp32
        return dict(out=None)

    def route(self, c, dt, ptrs, num_cus=256):
        n, Bt, es = c["n"], c["Bt"], 8 if dt == "f64" else 4
        a, q = ptrs["A"], ptrs["P"]
        if Bt > 128:
            return "NT GEMM, " + ("vector" if (n % 16 == 0 and n % (16 // es) == 0 and (a | q) % 16 == 0) else "ragged")
        if Bt >= 2:
            return "skinny, " + ("32-byte loads" if (n % 4 == 0 and a % 32 == 0 and q % 32 == 0) else "element-aligned")
        if n >= 1024:
            return "upper-triangle tiles"
        return "row GEMV, " + ("16-byte rows" if (n % (16 // es) == 0 and a % 16 == 0) else "scalar")


def _operator(c, dt, p):
    """mgp_operator of a case's `op` kind on the case's buffers -> (struct, keepalive)"""
    a = lambda name: p[name].value  # the address behind a c_void_p
    st = _hip.MgpOperator()
    st.dtype = CODE[dt]
    st.n = c["n"]
    if c["op"] == "dense":
        st.kind = _hip.OP_DENSE
        st.A = a("A")
        return st, None
    keep = kstruct(c["kind"], dt, c["D"], p["_ls"])
    st.kernel = ctypes.pointer(keep)
    if c["op"] == "kmm_lambda":
        st.kind, st.Z, st.M, st.lam = _hip.OP_KMM_LAMBDA, a("Z"), c["n"], a("lam")
    elif c["op"] == "kxx":
        st.kind, st.X, st.N, st.s2 = _hip.OP_KXX_NOISE, a("X"), c["n"], c["s2"]
    else:
        st.kind, st.X, st.N, st.Z, st.M, st.s2 = _hip.OP_SGPR, a("X"), c["N"], a("Z"), c["n"], c["s2"]
        st.Kmm = a("Kmm")
        st.kmm_row_begin, st.kmm_row_end = c.get("slab", (0, 0))
    return st, keep


def _operator_ins(c, dt, rng):
    n = c["n"]
    if c["op"] == "dense":
        return dict(A=_spd(rng, n))
    D = c["D"]
    ls = lengthscales(rng, D)
    if c["op"] == "kmm_lambda":
        return dict(Z=points(rng, n, D), lam=rng.uniform(0.5, 1.5, n), _ls=ls)
    if c["op"] == "kxx":
        return dict(X=points(rng, n, D), _ls=ls)
    Z = points(rng, n, D)
    Kmm = ok.Kernel(c["kind"], VAR, ls).K(rnd(Z, dt)) + 1e-6 * np.eye(n)
    return dict(X=points(rng, c["N"], D), Z=Z, Kmm=Kmm, _ls=ls)


def _operator_dense(c, dt, ins):
    """the explicit matrix of the operator, from the values the device sees"""
    if c["op"] == "dense":
        return rnd(ins["A"], dt)
    kern = ok.Kernel(c["kind"], VAR, ins["_ls"])
    if c["op"] == "kmm_lambda":
        return kern.K(rnd(ins["Z"], dt)) + np.diag(rnd(ins["lam"], dt))
    if c["op"] == "kxx":
        return kern.K(rnd(ins["X"], dt)) + c["s2"] * np.eye(c["n"])
    K = kern.K(rnd(ins["X"], dt), rnd(ins["Z"], dt))
    Kmm = rnd(ins["Kmm"], dt).copy()
    rb, re = c.get("slab", (0, 0))
    if (rb, re) != (0, 0):  # only this slab of the replicated s2 Kmm p term is added (a rank's share)
        keep = np.zeros(c["n"], dtype=bool)
        keep[rb:re] = True
        Kmm[~keep, :] = 0.0
        return c["s2"] * Kmm.T + K.T @ K  # out = p @ A with column j of the Kmm term present for j in the slab
    return c["s2"] * Kmm + K.T @ K


class OperatorApply(Row):
    """out[Bt, n] = P[Bt, n] @ Op for the four operator kinds"""
    name = "mgp_operator_apply"

    def reads_pointer(self, c, dt):
        return c["op"] in ("dense", "sgpr")  # these two go through dense.hip's dispatches; the sweeps read no pointer
    arenas = ("opws", "ws", "pack", "kxx", "gen")
    cases = [dict(op="dense", n=200, Bt=5), dict(op="dense", n=1001, Bt=1),
             dict(op="kmm_lambda", n=130, Bt=3, D=5, kind="matern32"),
             dict(op="kxx", n=777, Bt=1, D=17, kind="se", s2=0.37),
             dict(op="sgpr", n=37, N=777, Bt=1, D=5, kind="se", s2=0.1),
             dict(op="sgpr", n=130, N=4097, Bt=5, D=17, kind="matern52", s2=0.1),
             # the slab kernel (n % 128 == 0, n >= 1024, one right-hand side) that vector-loads p
             dict(op="sgpr", n=1024, N=65, Bt=1, D=5, kind="se", s2=0.1, slab=(0, 512))]

    def ins(self, c, dt, rng):
        d = _operator_ins(c, dt, rng)
        d["P"] = rng.standard_normal((c["Bt"], c["n"]))
        return d

    def outs(self, c, dt):
        return dict(out=((c["Bt"], c["n"]), "T"))

    def call(self, lib, h, c, dt, p):
        st, keep = _operator(c, dt, p)
        return lib.mgp_operator_apply(h, ctypes.byref(st), p["P"], c["Bt"], p["out"]), {}

    def reference(self, c, dt, ins):
        return rnd(ins["P"], dt) @ _operator_dense(c, dt, ins)

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        # dense: test_symm_matmul_fp64 / _fp32; matrix-free: test_kmm_lambda_operator / test_sgpr_operator_and_cg
        # (1e-11), fp32 the sweep's 2e-4
        if c["op"] == "dense":
            bar = 1e-12 if dt == "f64" else 1e-4
        else:
            bar = product_bar(c["kind"]) if dt == "f64" else 2e-4
        assert e < bar, (self.name, c, dt, e)
        return dict(out=None)

    def route(self, c, dt, ptrs, num_cus=256):
        if c["op"] == "dense":
            return SymmMatmul().route(dict(n=c["n"], Bt=c["Bt"]), dt, ptrs)
        if c["op"] == "sgpr" and c["Bt"] == 1:
            n, vw = c["n"], 2 if dt == "f64" else 4
            rb, re = c.get("slab", (0, n))
            vec = n % vw == 0 and ptrs["Kmm"] % 16 == 0
            if re - rb <= 8 * num_cus and n >= 1024:
                wide = vec and n % (64 * vw) == 0 and ptrs["P"] % 16 == 0
                return "Kmm slab kernel, " + ("16-byte loads of Kmm and p" if wide else "scalar loads")
            return "Kmm row GEMV, " + ("16-byte rows" if vec else "scalar")
        return "matrix-free sweeps"


class _Cg(Row):
    """k fixed steps of the device CG (threshold 0) against the oracle's loop on the explicit matrix"""

    def reads_pointer(self, c, dt):
        return c["op"] in ("dense", "sgpr")  # as mgp_operator_apply
    arenas = ("cg", "ws", "opws", "pack", "kxx", "gen")
    poison_keep = ("B", "V0")  # a NaN right-hand side ends the solve before the operator is applied once: the poison
                               # is a NaN operator under the clean right-hand sides, as the existing `cg` test does it
    record = False
    cases = [dict(op="dense", n=200, Bt=1, k=5, v0=True), dict(op="dense", n=200, Bt=5, k=5, v0=False),
             dict(op="dense", n=1001, Bt=1, k=5, v0=False), dict(op="dense", n=1001, Bt=5, k=5, v0=True),
             dict(op="kmm_lambda", n=130, Bt=3, k=5, D=5, kind="matern32", v0=False),
             dict(op="kxx", n=777, Bt=1, k=5, D=17, kind="se", s2=1.0, v0=False),
             dict(op="sgpr", n=37, N=777, Bt=5, k=3, D=5, kind="se", s2=1.0, v0=False)]

    def ins(self, c, dt, rng):
        d = _operator_ins(c, dt, rng)
        d["B"] = rng.standard_normal((c["Bt"], c["n"]))
        if c["v0"]:
            d["V0"] = np.zeros((c["Bt"], c["n"]))
        return d

    def outs(self, c, dt):
        d = dict(V_out=((c["Bt"], c["n"]), "T"), err_out=((c["Bt"],), "T"))
        if self.record:
            d["coef"] = ((c["k"] + c.get("spare", 0), c["Bt"], 3), "T")
        return d

    def call(self, lib, h, c, dt, p):
        st, keep = _operator(c, dt, p)
        stats = _hip.MgpCgStats()
        args = [h, ctypes.byref(st), None, p["B"], p.get("V0"), c["Bt"], c.get("thr", 0.0), c["k"] + c.get("spare", 0),
                c["k"] + c.get("spare", 0) + 1, 1e-16, 10, p["V_out"], p["err_out"], ctypes.byref(stats)]
        if self.record:
            rc = lib.mgp_pcg_solve_record(*args, p["coef"], c["k"] + c.get("spare", 0))
        else:
            rc = lib.mgp_pcg_solve(*args)
        return rc, dict(iterations=stats.iterations)

    def reference(self, c, dt, ins):
        A, b = _operator_dense(c, dt, ins), rnd(ins["B"], dt)
        sol, (steps, err) = ocg.conjugate_gradient(A, b, np.zeros_like(b), 0.0, max_iterations=c["k"])
        return sol, np.asarray(err).reshape(-1), steps

    def check(self, c, dt, ins, got, ref):
        sol, err, steps = ref
        assert got["iterations"] == c["k"] == steps, (self.name, c, got["iterations"])
        e = relerr(got["V_out"], sol)
        ee = float(np.max(np.abs(got["err_out"].astype(np.float64) - err) / err))
        # test_cg_fixed_iterations_match_oracle: 1e-9 on the iterate, 1e-6 on 0.5 rz.  fp32: the oracle's own loop run
        # in float32 on these systems differs from its float64 run by at most 1.3e-6 on the iterate and 2.5e-6 on 0.5 rz
        # (numpy, every case of this row); another summation order and the fp32 kernel values of the matrix-free
        # operators get 16x and 40x that: 2e-5 and 1e-4 (the project's only fp32 CG bar so far is the 1e-4 of
        # test_cg_start_up_ignores_stale_arena_contents on a converged solve)
        assert e < (1e-9 if dt == "f64" else 2e-5), (self.name, c, dt, e)
        assert ee < (1e-6 if dt == "f64" else 1e-4), (self.name, c, dt, ee)
        return dict(V_out=None, err_out=None)

    def route(self, c, dt, ptrs, num_cus=256):
        if c["op"] != "dense":
            return "device loop over the matrix-free operator"
        if self.record:
            return "device loop (the recording solve never takes the register-resident route)"
        if c["n"] <= 4096 and c["Bt"] <= 4:
            return "register-resident solve"
        return "tile route (skinny product + fused update)"


class PcgSolve(_Cg):
    name = "mgp_pcg_solve"


class PcgSolveRecord(_Cg):
    """... and coef[k, b, 0:3] = (gamma, beta, 0.5 rz) for every step taken; rows of steps not taken untouched"""
    name = "mgp_pcg_solve_record"
    arenas = ("cg", "kxx", "ws")  # its cases: the dense and the K_XX operator
    record = True
    cases = [dict(op="dense", n=200, Bt=1, k=5, v0=False), dict(op="dense", n=1001, Bt=5, k=5, v0=False),
             dict(op="kxx", n=777, Bt=3, k=5, D=5, kind="se", s2=1.0, v0=False),
             # converges long before the cap: the rows of coef from `iterations` on stay as they were
             dict(op="dense", n=200, Bt=3, k=0, spare=60, thr=1e-10, v0=False)]

    def reference(self, c, dt, ins):
        A, b = _operator_dense(c, dt, ins), rnd(ins["B"], dt)
        steps = c["k"] or 8  # the early-stopping case is compared over its first steps
        coef = np.zeros((steps, c["Bt"], 3))
        x = np.zeros_like(b)
        for col in range(c["Bt"]):  # the loop of test_recording_solve_matches_plain_solve_and_numpy_cg
            r = b[col].copy()
            pd = r.copy()
            rz = r @ r
            for k in range(steps):
                Ap = A @ pd
                g = rz / (pd @ Ap)
                x[col] += g * pd
                r -= g * Ap
                rzn = r @ r
                coef[k, col] = (g, rzn / rz, 0.5 * rzn)
                pd = r + (rzn / rz) * pd
                rz = rzn
        return x, coef

    def check(self, c, dt, ins, got, ref):
        x, coef = ref
        it, rows = got["iterations"], c["k"] + c.get("spare", 0)
        # test_recording_solve_matches_plain_solve_and_numpy_cg; fp32 as _Cg's 0.5 rz
        cbar = 1e-9 if dt == "f64" else 1e-4
        if c["k"]:
            assert it == c["k"], (self.name, c, it)
            assert relerr(got["V_out"], x) < (1e-9 if dt == "f64" else 2e-5), (self.name, c, dt)
            steps = it
        else:
            # 0.5 |r|^2 from ~1e2 to 1e-10 on a matrix of condition 3 (|r| falls by (sqrt 3 - 1) / (sqrt 3 + 1) = 0.27 a
            # step): about 11 steps; the first 8 (fp32: 4) are compared, while the residual is far above its floor
            steps = 8 if dt == "f64" else 4
            assert steps <= it < rows - 8, (self.name, c, it)
            assert np.all(got["err_out"] <= 1e-10)
        g = got["coef"][:steps].astype(np.float64)
        assert np.all(np.abs(g - coef[:steps]) <= cbar * np.abs(coef[:steps])), (self.name, c, dt)
        m = np.zeros((rows, c["Bt"], 3), dtype=bool)
        m[:it] = True
        return dict(V_out=None, err_out=None, coef=m)


class KmmLambdaMatvec(Row):
    """out[R, M] = V[R, M] @ (k(Z, Z) + diag(lambda))"""
    name = "mgp_kmm_lambda_matvec"
    arenas = ("pack", "gen", "ws")
    cases = [dict(M=130, R=1, D=5, kind="se"), dict(M=37, R=11, D=17, kind="matern32"), dict(M=1, R=3, D=1, kind="se"),
             dict(M=130, R=8, D=33, kind="matern52"), dict(M=777, R=3, D=32, kind="se")]

    def ins(self, c, dt, rng):
        return dict(Z=points(rng, c["M"], c["D"]), lam=rng.uniform(0.01, 0.5, c["M"]),
                    V=rng.standard_normal((c["R"], c["M"])), _ls=lengthscales(rng, c["D"]))

    def outs(self, c, dt):
        return dict(out=((c["R"], c["M"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        return lib.mgp_kmm_lambda_matvec(h, ctypes.byref(k), p["Z"], c["M"], p["lam"], p["V"], c["R"], p["out"]), {}

    def reference(self, c, dt, ins):
        return rnd(ins["V"], dt) @ (ok.Kernel(c["kind"], VAR, ins["_ls"]).K(rnd(ins["Z"], dt)) +
                                    np.diag(rnd(ins["lam"], dt)))

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        assert e < (product_bar(c["kind"]) if dt == "f64" else 2e-4), (self.name, c, dt, e)  # test_kmm_lambda_matvec
        return dict(out=None)


# ------------------------------------------------------------------------------------------------- reductions
class ColwiseDot(Row):
    name = "mgp_colwise_dot"
    arenas = ()
    missing = {"B": "needs no scratch: partial sums stay in registers and LDS"}
    cases = [dict(rows=300, cols=77), dict(rows=1, cols=1), dict(rows=4097, cols=5), dict(rows=65, cols=130)]

    def ins(self, c, dt, rng):
        return dict(A=rng.standard_normal((c["rows"], c["cols"])), B=rng.standard_normal((c["rows"], c["cols"])))

    def outs(self, c, dt):
        return dict(out=((c["cols"],), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_colwise_dot(h, CODE[dt], p["A"], p["B"], c["rows"], c["cols"], p["out"]), {}

    def reference(self, c, dt, ins):
        return np.sum(rnd(ins["A"], dt) * rnd(ins["B"], dt), axis=0)

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["out"], ref)
        # test_colwise_dot_and_dot_all: 1e-13 of the largest sum; fp32: u sqrt(rows / 4) |partial sum| of the
        # sequential fp32 accumulation stays below 1e-6 of it at these sizes, 1e-5 allowed
        assert e < (1e-13 if dt == "f64" else 1e-5), (self.name, c, dt, e)
        return dict(out=None)


class DotAll(Row):
    name = "mgp_dot_all"
    arenas = ("ws",)
    host_scalars = True
    cases = [dict(count=300 * 77), dict(count=1), dict(count=4097), dict(count=1 << 20)]

    def ins(self, c, dt, rng):
        return dict(A=rng.standard_normal(c["count"]), B=rng.standard_normal(c["count"]))

    def outs(self, c, dt):
        return {}

    def call(self, lib, h, c, dt, p):
        out = ctypes.c_double(float("nan"))
        rc = lib.mgp_dot_all(h, CODE[dt], p["A"], p["B"], c["count"], ctypes.byref(out))
        return rc, dict(out=out.value)

    def reference(self, c, dt, ins):
        A, B = rnd(ins["A"], dt).astype(LD), rnd(ins["B"], dt).astype(LD)
        return float(np.sum(A * B)), float(np.sum(np.abs(A * B)))

    def check(self, c, dt, ins, got, ref):
        val, scale = ref
        # test_colwise_dot_and_dot_all: |err| < 1e-10 at 23100 terms whose |terms| sum to ~1.47e4: 6.5e-15 of that sum;
        # the accumulation is fp64 for both dtypes (the products of fp32 inputs are exact in fp64)
        assert abs(got["out"] - val) <= 6.5e-15 * scale, (self.name, c, dt, got["out"], val)
        return {}


# ------------------------------------------------------------------------------------------------- clustering
class NearestCenter(Row):
    """idx[N] (int64) = argmin_m d(Z_m, X_i); best[N] the distance (may be NULL)"""
    name = "mgp_nearest_center"
    arenas = ("gen",)  # D = 33: squared norms of both sets
    DIST = {"sqeuclidean": 0, "euclidean": 1, "covariance": 2, "correlation": 3}
    cases = [dict(N=777, M=37, D=5, dist="sqeuclidean", best=True),
             dict(N=4097, M=130, D=17, dist="euclidean", best=True),
             dict(N=65, M=1, D=1, dist="covariance", best=True), dict(N=1, M=37, D=32, dist="correlation", best=False),
             dict(N=777, M=130, D=33, dist="sqeuclidean", best=True)]

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), Z=points(rng, c["M"], c["D"]), _ls=lengthscales(rng, c["D"]))

    def outs(self, c, dt):
        d = dict(idx=((c["N"],), "i64"))
        if c["best"]:
            d["best"] = ((c["N"],), "T")
        return d

    def call(self, lib, h, c, dt, p):
        k = kstruct("matern32", dt, c["D"], p["_ls"])
        return lib.mgp_nearest_center(h, ctypes.byref(k), self.DIST[c["dist"]], p["X"], c["N"], p["Z"], c["M"],
                                      p["idx"], p.get("best")), {}

    def reference(self, c, dt, ins):
        X, Z = rnd(ins["X"], dt), rnd(ins["Z"], dt)
        if c["dist"] == "sqeuclidean":
            return ok.square_distance(Z, X).T
        fn = od.create_distance_fn(ok.Kernel("matern32", VAR, ins["_ls"]), c["dist"])
        return fn((Z[None, :, :], X[:, None, :]))

    def check(self, c, dt, ins, got, ref):
        idx = got["idx"]
        assert idx.min() >= 0 and idx.max() < c["M"]
        chosen = ref[np.arange(c["N"]), idx]
        # test_nearest_center: the chosen distance is the minimum to 1e-10, best agrees to 1e-9; fp32: the values carry
        # u |x|^2 of the expansion form (test_nearest_center_any_dimension_fp32...: 1e-4)
        tol, btol = (1e-10, 1e-9) if dt == "f64" else (1e-4 * max(1.0, float(np.max(ref))), 1e-4)
        assert np.max(np.abs(chosen - ref.min(1))) < tol, (self.name, c, dt)
        if c["best"]:
            assert relerr(got["best"], chosen) < btol, (self.name, c, dt, relerr(got["best"], chosen))
            return dict(idx=None, best=None)
        return dict(idx=None)


class ClusterStats(Row):
    """sums[M], counts[M] of y per cluster"""
    name = "mgp_cluster_stats"
    arenas = ("ws",)
    poison = "finite"  # the index input has no NaN: a larger finite problem in the other dtype
    poison_case = dict(N=9001, M=140)
    cases = [dict(N=777, M=37), dict(N=4097, M=130), dict(N=65, M=1), dict(N=1, M=37)]

    def ins(self, c, dt, rng):
        idx = rng.integers(0, c["M"], c["N"])
        if c["M"] > 4:
            idx[idx == 3] = 4  # an empty cluster
        return dict(idx=idx.astype(np.int64), y=rng.standard_normal(c["N"]))

    def outs(self, c, dt):
        return dict(sums=((c["M"],), "T"), counts=((c["M"],), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_cluster_stats(h, CODE[dt], p["idx"], p["y"], c["N"], c["M"], p["sums"], p["counts"]), {}

    def reference(self, c, dt, ins):
        ref = np.zeros(c["M"])
        np.add.at(ref, ins["idx"], rnd(ins["y"], dt))
        return ref, np.bincount(ins["idx"], minlength=c["M"]).astype(np.float64)

    def check(self, c, dt, ins, got, ref):
        sums, cnt = ref
        assert np.array_equal(got["counts"].astype(np.float64), cnt), (self.name, c, dt)
        e = relerr(got["sums"], sums)
        assert e < (1e-12 if dt == "f64" else 1e-5), (self.name, c, dt, e)  # test_cluster_stats_sorted_and_sweep_agree
        return dict(sums=None, counts=None)


class SegmentSums(Row):
    """sums[M, C] = per-cluster column sums of Y[N, C], rows grouped by `order` / `offsets`"""
    name = "mgp_segment_sums"
    arenas = ()
    missing = {"B": "needs no scratch: one workgroup sums a cluster's run in registers"}
    cases = [dict(N=777, M=37, C=4), dict(N=4097, M=130, C=1), dict(N=65, M=1, C=3), dict(N=100, M=300, C=3)]

    def ins(self, c, dt, rng):
        idx = rng.integers(0, c["M"], c["N"])
        order = np.argsort(idx, kind="stable").astype(np.int64)
        offsets = np.zeros(c["M"] + 1, dtype=np.int64)
        np.cumsum(np.bincount(idx, minlength=c["M"]), out=offsets[1:])
        return dict(order=order, offsets=offsets, Y=rng.standard_normal((c["N"], c["C"])), _idx=idx)

    def outs(self, c, dt):
        return dict(sums=((c["M"], c["C"]), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_segment_sums(h, CODE[dt], p["order"], p["offsets"], p["Y"], c["N"], c["C"], c["M"],
                                    p["sums"]), {}

    def reference(self, c, dt, ins):
        ref = np.zeros((c["M"], c["C"]))
        np.add.at(ref, ins["_idx"], rnd(ins["Y"], dt))
        return ref

    def check(self, c, dt, ins, got, ref):
        e = relerr(got["sums"], ref)
        assert e < (1e-12 if dt == "f64" else 1e-5), (self.name, c, dt, e)  # test_cluster_stats_sorted_and_sweep_agree
        return dict(sums=None)


# ------------------------------------------------------------------------------------- random Fourier features
def _rff_parts(X, th):
    P = X.astype(LD) @ th.astype(LD).T
    return np.cos(P), np.sin(P), np.abs(X) @ np.abs(th).T


class RffFeatures(Row):
    """out[n, 0:L] = cos, out[n, L:2L] = sin, rows ld >= 2L apart; columns 2L..ld-1 untouched"""
    name = "mgp_rff_features"
    arenas = ("gen",)  # theta / 2 pi, transposed
    cases = [dict(N=777, D=5, L=37, pad=3), dict(N=4097, D=17, L=1, pad=1), dict(N=65, D=33, L=130, pad=0),
             dict(N=1, D=1, L=8, pad=5), dict(N=0, D=5, L=8, pad=1)]  # N = 0 writes nothing (allocated for one row)

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), theta=rng.standard_normal((c["L"], c["D"])))

    def outs(self, c, dt):
        return dict(out=((max(c["N"], 1), 2 * c["L"] + c["pad"]), "T"))

    def call(self, lib, h, c, dt, p):
        return lib.mgp_rff_features(h, CODE[dt], p["X"], c["N"], c["D"], p["theta"], c["L"], p["out"],
                                    2 * c["L"] + c["pad"]), {}

    def reference(self, c, dt, ins):
        return _rff_parts(rnd(ins["X"], dt), rnd(ins["theta"], dt))

    def check(self, c, dt, ins, got, ref):
        L = c["L"]
        if c["N"] == 0:
            return dict(out=none(got["out"].shape))
        cos, sin, Pabs = ref
        bound = 8 * U[dt] * (1 + Pabs)  # include/mgp.h, tests/test_gpu_rff.py
        o = got["out"].astype(np.float64)
        assert np.all(np.abs(o[:, :L] - cos) <= bound) and np.all(np.abs(o[:, L:2 * L] - sin) <= bound), (self.name, c, dt)
        m = none(o.shape)
        m[:, :2 * L] = True
        return dict(out=m)


class RffSample(Row):
    """out(s, n) = scale * sum_l (W[s, l] cos + W[s, L + l] sin); [S, N] (MGP_ROWS) or [N, S] (MGP_COLS)"""
    name = "mgp_rff_sample"

    def reads_pointer(self, c, dt):
        return c["D"] > 32 or c["S"] > 8  # panel route: the NT GEMM against W reads W's alignment
    arenas = ("gen", "ws")
    cases = [dict(N=777, D=5, L=37, S=3, layout=ROWS), dict(N=4097, D=17, L=130, S=8, layout=COLS),
             dict(N=65, D=33, L=37, S=1, layout=ROWS), dict(N=777, D=5, L=130, S=11, layout=COLS),
             dict(N=1, D=1, L=1, S=1, layout=ROWS), dict(N=0, D=5, L=8, S=3, layout=ROWS)]

    def ins(self, c, dt, rng):
        return dict(X=points(rng, c["N"], c["D"]), theta=rng.standard_normal((c["L"], c["D"])),
                    W=rng.standard_normal((c["S"], 2 * c["L"])))

    def outs(self, c, dt):
        n = max(c["N"], 1)
        return dict(out=((c["S"], n) if c["layout"] == ROWS else (n, c["S"]), "T"))

    def _scale(self, c):
        return math.sqrt(1.7 / c["L"])

    def call(self, lib, h, c, dt, p):
        return lib.mgp_rff_sample(h, CODE[dt], p["X"], c["N"], c["D"], p["theta"], c["L"], p["W"], c["S"],
                                  self._scale(c), p["out"], c["layout"]), {}

    def reference(self, c, dt, ins):
        cos, sin, Pabs = _rff_parts(rnd(ins["X"], dt), rnd(ins["theta"], dt))
        W, L, scale = rnd(ins["W"], dt), c["L"], self._scale(c)
        ref = LD(scale) * (W[:, :L].astype(LD) @ cos.T + W[:, L:].astype(LD) @ sin.T)
        absw = np.abs(W[:, :L]) + np.abs(W[:, L:])
        u = U[dt]  # the bound of tests/test_gpu_rff.py::check_case
        bound = scale * (absw @ (8 * u * (1 + Pabs)).T) + scale * u * (4 * math.sqrt(2 * L) + 2) * absw.sum(1)[:, None]
        return ref.astype(np.float64), bound

    def check(self, c, dt, ins, got, ref):
        if c["N"] == 0:
            return dict(out=none(got["out"].shape))
        val, bound = ref
        g = got["out"].astype(np.float64)
        g = g if c["layout"] == ROWS else g.T
        assert np.all(np.abs(g - val) <= bound), (self.name, c, dt, float(np.max(np.abs(g - val) / bound)))
        return dict(out=None)

    def route(self, c, dt, ptrs, num_cus=256):
        return "fused sweep" if (c["D"] <= 32 and c["S"] <= 8) else "feature panels + NT GEMM"


# ------------------------------------------------------------------ the entry points of the five later headers
def _num_cus():
    """compute units of the device the call runs on (the chunk rule of a bound depends on it); the nominal 256 of an
    MI355X where there is no GPU (the host tests evaluate references only)"""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


class _SweepAnyd(Row):
    """mgp_knm_matvec_anyd / mgp_kmn_matvec_anyd / mgp_kxx_matvec_anyd (include/mgp_sweep_anyd.h): `na` owned points
    (the rows of the result), `nb` streamed ones, R columns.  fp64 above 32 dimensions is the fused route, held to
    `dense_reference` of tests/test_gpu_sweep_anyd.py (the long-double product and the bound built on
    `pair_reference.pair_bound`) on that test's own inputs; fp32 and D <= 32 are, by the header, exactly the code of
    the plain name, and are held to the plain rows' bar (`kbar`) against the float64 oracle."""
    entry = None
    # fused route: `ws` alone (both squared-norm vectors and the chunk partials).  The fallbacks are the plain names':
    # fp64 D = 17 the packed streamed set (and, R > 1, the transposed weights in `gen`), fp32 above D = 32 the panels
    arenas = ("ws", "gen", "pack")

    def _case(self, c):
        from sweep_anyd_plan import Case
        return Case(self.entry, c["kind"], c["D"], c["na"], c["nb"], c["R"], c["wl"], c["ol"], c.get("s2", 0.0))

    def _fused(self, c, dt):
        return dt == "f64" and c["D"] > 32

    @staticmethod
    def dense_bound(case, A, B, ls, W):
        """(want, tol) of `dense_reference` (tests/test_gpu_sweep_anyd.py) for given points, lengthscales and
        multipliers; `reference` below holds the two to each other bit for bit on every case of the table"""
        import pair_reference as pr
        u = 2.0 ** -53
        pv = pr.pair_values(case.kind, VAR, ls, A, B)
        rel = pr.pair_bound(case.kind, VAR, pv.s, pv.q, pr.scaled(case.kind, ls, A), pr.scaled(case.kind, ls, B),
                            case.D, np.float64)
        Wl = W.astype(LD)
        want = pv.k @ Wl
        tol = (rel.astype(LD) * pv.k) @ np.abs(Wl) + (case.nb + 2) * u * (pv.k @ np.abs(Wl))
        if case.entry == "kxx":
            want = want + LD(case.s2) * Wl
            tol = tol + u * (np.abs(want) + LD(case.s2) * np.abs(Wl))
        return want, tol

    def ins(self, c, dt, rng):
        from sweep_anyd_plan import points as anyd_points
        case = self._case(c)
        A, B, ls = anyd_points(case)
        # the multipliers of `dense_reference`, restated: its rng, its shape
        W = np.random.default_rng([7, case.na, case.nb, case.R]).standard_normal((case.nb, case.R))
        d = dict(A=A, V=W if c["wl"] == COLS else np.ascontiguousarray(W.T), _ls=ls)
        if self.entry != "kxx":
            d["B"] = B
        return d

    def outs(self, c, dt):
        return dict(out=(_vec(c["ol"], c["na"] or 2, c["R"]), "T"))

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        if self.entry == "kxx":
            return lib.mgp_kxx_matvec_anyd(h, ctypes.byref(k), p["A"], c["na"], c["s2"], p["V"], c["R"], c["wl"],
                                           p["out"], c["ol"]), {}
        if self.entry == "knm":  # X owned, Z streamed
            return lib.mgp_knm_matvec_anyd(h, ctypes.byref(k), p["A"], c["na"], p["B"], c["nb"], p["V"], c["R"],
                                           c["wl"], p["out"], c["ol"]), {}
        return lib.mgp_kmn_matvec_anyd(h, ctypes.byref(k), p["B"], c["nb"], p["A"], c["na"], p["V"], c["R"], c["wl"],
                                       p["out"], c["ol"]), {}

    def reference(self, c, dt, ins):
        if c["na"] == 0 or c["nb"] == 0:
            return None
        if self._fused(c, dt):
            from test_gpu_sweep_anyd import dense_reference
            case = self._case(c)
            W = _as_cols(ins["V"], c["wl"])
            B = ins["B"] if "B" in ins else ins["A"]
            # `dense_reference` draws its own lengthscales: a call sequence that changes them
            # (tests/test_gpu_call_sequences.py) gets the same bound from the same functions on the values it used
            want, tol = self.dense_bound(case, ins["A"], B, ins["_ls"], W)
            A0, B0, ls0, W0, want0, tol0 = dense_reference(case)
            if np.array_equal(ls0, ins["_ls"]):  # the table's own inputs: the existing test's reference, to the bit
                assert np.array_equal(A0, ins["A"]) and np.array_equal(B0, B) and np.array_equal(W0, W)
                assert np.array_equal(want0, want) and np.array_equal(tol0, tol)
            return want.astype(np.float64), tol.astype(np.float64)
        A = rnd(ins["A"], dt)
        V = _as_cols(rnd(ins["V"], dt), c["wl"])
        K = ok.Kernel(c["kind"], VAR, ins["_ls"]).K(A, rnd(ins["B"], dt) if "B" in ins else A)
        return K @ V + c.get("s2", 0.0) * V if self.entry == "kxx" else K @ V

    def check(self, c, dt, ins, got, ref):
        if c["na"] == 0:  # no owned point: nothing is written
            return dict(out=none(got["out"].shape))
        g = _as_cols(got["out"], c["ol"])
        if c["nb"] == 0:  # no streamed point: zeros
            assert not g.any(), (self.name, c, dt)
            return dict(out=None)
        if self._fused(c, dt):
            want, tol = ref
            ratio = float(np.max(np.abs(g.astype(LD) - want) / tol))
            assert np.all(np.isfinite(g)) and ratio <= 1.0, (self.name, c, dt, ratio)
        else:
            e = relerr(g, ref)
            assert e < kbar(c["kind"], dt), (self.name, c, dt, e)
        return dict(out=None)


def _anyd_cases(extra):
    # owned block 128, streamed tile 64, K slices of 32 columns: (129, 65) two owned blocks and two chunks, (129, 150)
    # three chunks (the partials of `ws`); D = 33 a slice and one k-step, 63 two whole slices and one k-step, 77 two
    # and a half; R = 9 a pass of 8 and one of 1
    return [dict(na=1, nb=1, D=33, R=1, kind="se", wl=COLS, ol=COLS),
            dict(na=129, nb=65, D=63, R=3, kind="matern32", wl=ROWS, ol=ROWS),
            dict(na=129, nb=150, D=77, R=9, kind="matern52", wl=COLS, ol=ROWS),
            dict(na=129, nb=65, D=17, R=3, kind="se", wl=ROWS, ol=COLS)] + extra  # D = 17: the plain route


class KnmMatvecAnyd(_SweepAnyd):
    name = "mgp_knm_matvec_anyd"
    entry = "knm"
    cases = _anyd_cases([dict(na=65, nb=0, D=33, R=3, kind="se", wl=COLS, ol=COLS),    # M = 0: zeros
                         dict(na=0, nb=65, D=33, R=3, kind="se", wl=COLS, ol=COLS)])   # N = 0: nothing written


class KmnMatvecAnyd(_SweepAnyd):
    name = "mgp_kmn_matvec_anyd"
    entry = "kmn"
    cases = _anyd_cases([dict(na=65, nb=0, D=33, R=3, kind="se", wl=COLS, ol=COLS),    # N = 0: zeros
                         dict(na=0, nb=65, D=33, R=3, kind="se", wl=COLS, ol=COLS)])   # M = 0: nothing written


class KxxMatvecAnyd(_SweepAnyd):
    name = "mgp_kxx_matvec_anyd"
    entry = "kxx"
    # the D = 17 fallback on a MGP_KXX=sym handle is csrc/kxx.hip for fp64
    arenas = ("ws", "gen", "kxx")
    cases = [dict(na=1, nb=1, D=33, R=1, kind="se", wl=COLS, ol=COLS, s2=0.37),
             dict(na=129, nb=129, D=63, R=3, kind="matern32", wl=ROWS, ol=ROWS, s2=0.37),
             dict(na=150, nb=150, D=77, R=9, kind="matern52", wl=COLS, ol=ROWS, s2=0.37),
             dict(na=129, nb=129, D=17, R=3, kind="se", wl=ROWS, ol=COLS, s2=0.37),
             dict(na=0, nb=0, D=33, R=3, kind="se", wl=COLS, ol=COLS, s2=0.37)]  # N = 0: nothing written


class KmnKnmVjpAnyd(Row):
    """mgp_kmn_knm_vjp_anyd (include/mgp_anyd.h): host dvariance, dlengthscales; dZ[M, D] (may be NULL); Gq may be NULL
    with P >= 1.  Above 32 dimensions: `kvjp_reference` and the derived bound of tests/test_gpu_sgpr_train_anyd.py
    (`_check`, called as it stands).  At D <= 32 the header promises the implementation and the bits of
    mgp_kmn_knm_vjp: the 1e-10 of the sum of |terms| of that row (test_kmn_knm_vjp_against_long_double), the companions
    being those of `kvjp_reference`."""
    name = "mgp_kmn_knm_vjp_anyd"
    dtypes = ("f64",)
    arenas = ("kgrad",)
    poison = "finite"  # fp64 only: a larger finite problem
    poison_case = dict(N=300, M=140, D=65, P=2, panel_rows=0, gq=True, dZ=True, kind="matern52")
    host_scalars = True
    VARIANCE = 1.4
    # N = 130, M = 70: two 64-row tiles and two rows, 64 + 6 columns; panel_rows = 33: four panels, the last of 31 rows
    cases = [dict(N=130, M=70, D=33, P=1, panel_rows=0, gq=True, dZ=True, kind="se"),
             dict(N=130, M=70, D=65, P=2, panel_rows=33, gq=True, dZ=True, kind="matern32"),
             dict(N=130, M=70, D=33, P=1, panel_rows=33, gq=False, dZ=True, kind="matern52"),  # Gq = NULL
             dict(N=65, M=37, D=5, P=0, panel_rows=33, gq=True, dZ=True, kind="matern32"),
             dict(N=130, M=70, D=65, P=0, panel_rows=0, gq=True, dZ=False, kind="matern12"),   # dZ = NULL
             dict(N=0, M=37, D=33, P=1, panel_rows=0, gq=True, dZ=True, kind="se")]            # N = 0: zeros

    def reads_pointer(self, c, dt):
        return c["P"] > 0  # Y and Gb enter the NT GEMM, whose vector form reads their alignment (as mgp_kmn_knm_vjp)

    def ins(self, c, dt, rng):
        n = max(c["N"], 1)  # N = 0: one row allocated, none read
        d = dict(X=rng.uniform(-1.5, 1.5, (n, c["D"])), Z=rng.uniform(-1.5, 1.5, (c["M"], c["D"])),
                 _ls=math.sqrt(c["D"]) * np.linspace(0.7, 1.3, c["D"]))
        if c["gq"]:
            d["Gq"] = rng.standard_normal((c["M"], c["M"]))
        if c["P"]:
            d["Y"], d["Gb"] = rng.standard_normal((n, c["P"])), rng.standard_normal((c["M"], c["P"]))
        return d

    def outs(self, c, dt):
        return dict(dZ=((c["M"], c["D"]), "T")) if c["dZ"] else {}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"], var=self.VARIANCE)
        dv, dl = ctypes.c_double(float("nan")), (ctypes.c_double * _hip.MGP_MAX_D)()
        rc = lib.mgp_kmn_knm_vjp_anyd(h, ctypes.byref(k), p["X"], c["N"], p["Z"], c["M"], p.get("Gq"), p.get("Y"),
                                      p.get("Gb"), c["P"], c["panel_rows"], ctypes.byref(dv), dl, p.get("dZ"))
        return rc, dict(dv=dv.value, dl=np.array([dl[d] for d in range(c["D"])]))

    def reference(self, c, dt, ins):
        from kvjp_reference import kvjp_reference
        N = c["N"]
        return kvjp_reference(c["kind"], self.VARIANCE, ins["_ls"], ins["X"][:N], ins["Z"], ins.get("Gq"),
                              ins["Y"][:N] if c["P"] else None, ins.get("Gb"))

    def check(self, c, dt, ins, got, ref):
        f = lambda a: np.asarray(a, dtype=np.float64)
        if c["N"] == 0:  # every companion sum is 0: the bound demands exact zeros (`_check` prints err / bound)
            assert got["dv"] == 0.0 and not got["dl"].any() and not got["dZ"].any(), (self.name, c)
            assert float(ref.sv) == 0.0 and not f(ref.dv).any() and not f(ref.dZ).any()
        elif c["D"] > 32:
            from test_gpu_sgpr_train_anyd import _check
            dZ = torch.from_numpy(np.ascontiguousarray(got["dZ"])) if c["dZ"] else None
            _check((got["dv"], list(got["dl"]), dZ), ref, c["N"], c["M"], c["D"], c["P"], c["dZ"])
        else:
            assert abs(got["dv"] - float(ref.dv)) <= 1e-10 * float(ref.sv), (self.name, c, got["dv"], float(ref.dv))
            assert np.all(np.abs(got["dl"] - f(ref.dl)) <= 1e-10 * f(ref.sl)), (self.name, c)
            if c["dZ"]:
                assert np.all(np.abs(got["dZ"] - f(ref.dZ)) <= 1e-10 * f(ref.sz) + 1e-300), (self.name, c)
        return dict(dZ=None) if c["dZ"] else {}

    def route(self, c, dt, ptrs, num_cus=256):
        return "panel GEMMs (vector form by alignment of Y, Gb)"


class KDenseVjpPoints(Row):
    """mgp_k_dense_vjp_points (include/mgp_points.h): host dvariance, dlengthscales; dA[na, D], dB[nb, D] (either may
    be NULL); G[na, ldg] with NaN in the columns nb..ldg-1, which are never read; A and B may be one pointer.
    `k_dense_vjp_points_reference` at `VJP_BAR` of each output's sum of |terms| (tests/test_gpu_kvjp_points.py)."""
    name = "mgp_k_dense_vjp_points"
    dtypes = ("f64",)
    arenas = ("kgrad",)
    poison = "finite"  # fp64 only: a larger finite problem
    poison_case = dict(na=300, nb=300, D=65, pad=3, panel_rows=0, null=(), same=False, kind="matern52")
    host_scalars = True
    # DP = 4, 32 and the two staged routes (two and three slices of 32 dimensions); 257 = a block of 256 lanes and one;
    # panel_rows = 33: panels of 33 rows, the last shorter
    cases = [dict(na=1, nb=37, D=3, pad=3, panel_rows=0, null=(), same=False, kind="se"),
             dict(na=257, nb=130, D=32, pad=3, panel_rows=33, null=(), same=False, kind="matern12"),
             dict(na=130, nb=257, D=33, pad=3, panel_rows=0, null=("dA",), same=False, kind="matern32"),
             dict(na=257, nb=130, D=65, pad=3, panel_rows=33, null=("dB",), same=False, kind="matern52"),
             dict(na=130, nb=130, D=33, pad=3, panel_rows=0, null=(), same=True, kind="se"),   # A is B
             dict(na=0, nb=37, D=3, pad=3, panel_rows=0, null=(), same=False, kind="se")]      # na = 0: zeros

    def ins(self, c, dt, rng):
        na = max(c["na"], 1)  # na = 0: one row allocated, none read
        G = np.full((na, c["nb"] + c["pad"]), np.nan)  # NaN in the pad columns: it must not reach a result
        G[:, :c["nb"]] = rng.standard_normal((na, c["nb"]))
        d = dict(A=rng.uniform(-2.0, 2.0, (na, c["D"])), G=G, _ls=np.linspace(0.7, 1.4, c["D"]) * math.sqrt(c["D"]))
        if not c["same"]:
            d["B"] = rng.uniform(-2.0, 2.0, (c["nb"], c["D"]))
        return d

    def outs(self, c, dt):
        d = dict(dA=((max(c["na"], 1), c["D"]), "T"), dB=((c["nb"], c["D"]), "T"))
        return {k: v for k, v in d.items() if k not in c["null"]}

    def call(self, lib, h, c, dt, p):
        k = kstruct(c["kind"], dt, c["D"], p["_ls"])
        dv, dl = ctypes.c_double(float("nan")), (ctypes.c_double * _hip.MGP_MAX_D)()
        rc = lib.mgp_k_dense_vjp_points(h, ctypes.byref(k), p["A"], c["na"], p["A"] if c["same"] else p["B"], c["nb"],
                                        p["G"], c["nb"] + c["pad"], c["panel_rows"], ctypes.byref(dv), dl, p.get("dA"),
                                        p.get("dB"))
        return rc, dict(dv=dv.value, dl=np.array([dl[d] for d in range(c["D"])]))

    KEYS = ("dv", "dl", "dA", "dB", "sv", "sl", "sA", "sB")

    def reference(self, c, dt, ins):
        from kvjp_points_reference import k_dense_vjp_points_reference
        na = c["na"]
        A = ins["A"][:na]
        ref = k_dense_vjp_points_reference(c["kind"], VAR, ins["_ls"], A, A if c["same"] else ins["B"],
                                           ins["G"][:na, :c["nb"]])
        return tuple(np.asarray(ref[k]) for k in self.KEYS)

    def check(self, c, dt, ins, got, ref):
        from kvjp_points_reference import VJP_BAR, excess
        ref = dict(zip(self.KEYS, ref))
        names = [n for n in ("dA", "dB") if n not in c["null"]]
        for n in ["dv", "dl"] + names:
            g = got[n][:c["na"]] if n == "dA" else got[n]
            assert np.all(np.isfinite(g)), (self.name, c, n)
            e = excess(g, ref[n], ref["s" + n[1:]], VJP_BAR)
            assert e <= 1.0, (self.name, c, n, e)
        written = {n: None for n in names}
        if c["na"] == 0:
            assert got["dv"] == 0.0 and not got["dl"].any() and not got["dB"].any(), (self.name, c)
            written["dA"] = none(got["dA"].shape)  # no row of A: nothing to write
        return written


class RffSampleVjp(Row):
    """mgp_rff_sample_vjp (include/mgp_pathwise.h): dtheta[L, D], dX[N, D], either may be NULL; G [S, N] or [N, S].
    `rff_vjp_reference.vjp` and `rff_vjp_reference.bounds`, the bound the header states (tests/test_gpu_rff_vjp.py)."""
    name = "mgp_rff_sample_vjp"
    dtypes = ("f64",)
    arenas = ("gen", "ws")  # the streamed records; the chunk partials
    poison = "finite"  # fp64 only: a larger finite problem
    poison_case = dict(N=300, L=300, D=32, S=8, layout=ROWS, null=())
    # DP = 4, 8, 16, 32; (33, 257): two streamed chunks for dtheta and a second owner block of one basis; (257, 1) the
    # reverse; (70, 255): three chunks of rows, eight of bases
    cases = [dict(N=33, L=257, D=1, S=1, layout=ROWS, null=()),
             dict(N=257, L=1, D=8, S=8, layout=COLS, null=()),
             dict(N=70, L=255, D=9, S=8, layout=ROWS, null=("dX",)),
             dict(N=70, L=255, D=32, S=1, layout=COLS, null=("dtheta",)),
             dict(N=0, L=37, D=8, S=1, layout=ROWS, null=()),   # N = 0: zeros to dtheta, nothing to dX
             dict(N=33, L=0, D=9, S=8, layout=COLS, null=())]   # L = 0: zeros to dX, nothing to dtheta

    def _scale(self, c):
        return math.sqrt(1.7 / max(c["L"], 1))

    def ins(self, c, dt, rng):
        n, l = max(c["N"], 1), max(c["L"], 1)  # an empty side: one row allocated, none read
        return dict(X=rng.standard_normal((n, c["D"])), theta=rng.standard_normal((l, c["D"])),
                    W=rng.standard_normal((c["S"], 2 * l)),
                    G=rng.standard_normal((c["S"], n) if c["layout"] == ROWS else (n, c["S"])))

    def outs(self, c, dt):
        d = dict(dtheta=((max(c["L"], 1), c["D"]), "T"), dX=((max(c["N"], 1), c["D"]), "T"))
        return {k: v for k, v in d.items() if k not in c["null"]}

    def call(self, lib, h, c, dt, p):
        return lib.mgp_rff_sample_vjp(h, CODE[dt], p["X"], c["N"], c["D"], p["theta"], c["L"], p["W"], c["S"],
                                      self._scale(c), p["G"], c["layout"], p.get("dtheta"), p.get("dX")), {}

    def _args(self, c, ins):
        N, L = c["N"], c["L"]
        G = ins["G"] if c["layout"] == ROWS else ins["G"].T
        W = ins["W"] if L else ins["W"][:, :0]
        return ins["X"][:N], ins["theta"][:L], W, self._scale(c), G[:, :N]

    def reference(self, c, dt, ins):
        from rff_vjp_reference import vjp
        return vjp(*self._args(c, ins))

    def check(self, c, dt, ins, got, ref):
        from rff_vjp_reference import bounds
        N, L = c["N"], c["L"]
        if N == 0 or L == 0:  # no streamed term: zeros for every owner; no owner: nothing written
            assert not got["dtheta"][:L].any() and not got["dX"][:N].any(), (self.name, c)
            return dict(dtheta=None if L else none(got["dtheta"].shape), dX=None if N else none(got["dX"].shape))
        written = {}
        for n, r, b in zip(("dtheta", "dX"), ref, bounds(*self._args(c, ins), _num_cus())):
            if n in c["null"]:
                continue
            err = np.abs(got[n] - r.astype(np.float64))
            assert np.all(np.isfinite(got[n])) and np.all(err <= b), (self.name, c, n,
                                                                     float(np.max(err / np.where(b > 0, b, 1.0))))
            written[n] = None
        return written


class KnmQuadform(Row):
    """mgp_knm_quadform (include/mgp_predict.h): q[B] = k(xs_b, Z) C k(Z, xs_b) for the upper triangle of C[M, ldc]; the
    lower triangle and the columns M..ldc-1 hold NaN and are never read.  `quadform_reference.form` and `.bound` on
    `pair_reference.pair_bound`, as tests/test_gpu_quadform.py holds both routes to them."""
    name = "mgp_knm_quadform"
    arenas = ("prj",)  # fused: block partials and the packed Z; generic (fp32, D = 33): sym(C) and two panels (no NT
                       # GEMM slices in `ws` below M = 512)
    PAD = 3
    # tile 128 x 128, inner step 16: M = 127 / 129 / 257 one block short, two, three (the middle one paired with itself)
    cases = [dict(B=1, M=1, D=5, kind="se"), dict(B=129, M=127, D=32, kind="matern32"),
             dict(B=129, M=257, D=5, kind="matern52"), dict(B=1, M=129, D=33, kind="se"),
             dict(B=0, M=37, D=5, kind="se"),    # B = 0: nothing written
             dict(B=129, M=0, D=5, kind="se")]   # M = 0: zeros

    def reads_pointer(self, c, dt):
        return dt == "f32" or c["D"] > 32  # the generic route's NT GEMM picks its loads by alignment

    def ins(self, c, dt, rng):
        import pair_reference as pr
        B, M, D = max(c["B"], 1), max(c["M"], 1), c["D"]  # an empty side: one row allocated, none read
        Xs, Z = 1.2 * rng.standard_normal((B, D)) / math.sqrt(D), 1.2 * rng.standard_normal((M, D)) / math.sqrt(D)
        if M > 5:
            Z[5] = Xs[0]  # a coincident pair: k = variance, the Matern cusp
        Gm = rng.standard_normal((M, M))
        C = np.full((M, M + self.PAD), np.nan)  # NaN below the diagonal and in the pad columns
        C[:, :M] = Gm @ Gm.T / M + np.diag(0.5 + rng.random(M))
        C[np.tril_indices(M, -1)] = np.nan
        return dict(Xs=Xs, Z=Z, C=C, _ls=pr.lengthscales(D))

    def outs(self, c, dt):
        return dict(q=((max(c["B"], 1),), "T"))

    def call(self, lib, h, c, dt, p):
        import pair_reference as pr
        k = kstruct(c["kind"], dt, c["D"], p["_ls"], var=pr.VARIANCE)
        return lib.mgp_knm_quadform(h, ctypes.byref(k), p["Xs"], c["B"], p["Z"], c["M"], p["C"],
                                    max(c["M"], 1) + self.PAD, p["q"]), {}

    def reference(self, c, dt, ins):
        import pair_reference as pr
        import quadform_reference as qr
        B, M = c["B"], c["M"]
        if B == 0 or M == 0:
            return None
        Xs, Z, C = rnd(ins["Xs"], dt), rnd(ins["Z"], dt), rnd(ins["C"][:, :M], dt)
        pv = pr.pair_values(c["kind"], pr.VARIANCE, ins["_ls"], Xs, Z)
        q, mag = qr.form(pv.k, C)
        eps = qr.row_eps(c["kind"], pr.VARIANCE, ins["_ls"], Xs, Z, pv, NP[dt])[:, -1]
        return np.asarray(q, dtype=np.float64), qr.bound(eps, M, mag, NP[dt])

    def check(self, c, dt, ins, got, ref):
        if c["B"] == 0:
            return dict(q=none(got["q"].shape))
        if c["M"] == 0:
            assert not got["q"].any(), (self.name, c, dt)
            return dict(q=None)
        q, bound = ref
        g = got["q"].astype(np.float64)
        assert np.all(np.isfinite(g)) and np.all(np.abs(g - q) <= bound), (self.name, c, dt,
                                                                           float(np.max(np.abs(g - q) / bound)))
        return dict(q=None)

    def route(self, c, dt, ptrs, num_cus=256):
        return "fused" if (dt == "f64" and c["D"] <= 32) else "generic (sym(C), panels through mgp_k_dense, NT GEMM)"


TABLE = [KnmMatvec(), KmnMatvec(), KDense(), KmnKnm(), KmnSqColsum(), KxxMatvec(), KxxPivchol(), LowrankApply(),
         KnmProject(), KxxGrad(), KmnKnmVjp(), SymmMatmul(), PcgSolve(), PcgSolveRecord(), OperatorApply(),
         KmmLambdaMatvec(), ColwiseDot(), DotAll(), NearestCenter(), ClusterStats(), SegmentSums(), KDenseVjp(),
         RffFeatures(), RffSample(), KnmMatvecAnyd(), KmnMatvecAnyd(), KxxMatvecAnyd(), KmnKnmVjpAnyd(),
         KDenseVjpPoints(), RffSampleVjp(), KnmQuadform()]
BY_NAME = {r.name: r for r in TABLE}


def build_inputs(row, c, dt):
    """the deterministic inputs of a case: float arrays rounded to the dtype, int64 arrays and `_` entries as they are"""
    rng = np.random.default_rng(row.seed(c))
    return row.ins(c, dt, rng)


_REF = {}


def reference(row, ci, dt):
    """computed once per (row, case, dtype) and shared by every test that needs it"""
    key = (row.name, ci, dt)
    if key not in _REF:
        c = row.cases[ci]
        _REF[key] = row.reference(c, dt, build_inputs(row, c, dt))
    return _REF[key]
