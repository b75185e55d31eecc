"""Batched preconditioned conjugate gradient -- host mirror of `cggp/conjugate_gradient.py`.

Same names, argument order and shapes as the reference:

* `conjugate_gradient(matrix, rhs[Bt,n], initial_solution[Bt,n], error_threshold,
  preconditioner=None, max_iterations=None, max_steps_cycle=100)
  -> (solution[Bt,n], (steps, error[Bt,1]))`                      (reference :24-32,120)
* `ConjugateGradient(error_threshold, preconditioner=None, max_iterations=None,
  max_steps_cycle=None)`; `__call__(matrix[n,n], rhs[n,Bt], initial_solution=None) -> [n,Bt]`
  (reference :160-212)
* `CGPreconditioner / EyePreconditioner / BlockPreconditioner`     (reference :125-157)
* `PivotedCholeskyPreconditioner(rank, rel_tol, wide)`: build-side addition for `KxxNoiseOperator` (exact GPR) and
  `KmmLambdaOperator` (matrix-free CDGP)

The loop itself (`cg_step`, the stopping rule, the breakdown guards, the residual refresh)
runs in libmgp (`csrc/cg.hip`); this module only validates, lays tensors out and wires the
custom gradient (reference :100-118).  Build-side additions, none replacing reference
behaviour: `matrix` may be a `LinearOperator` (matrix-free forms), `JacobiPreconditioner`,
`ConjugateGradient.solve_with_stats`, `min_float` / `check_every` knobs.
"""

import ctypes

import numpy as np
import torch

from . import _hip, ops

MIN_FLOAT = 1e-16  # reference :50


# --------------------------------------------------------------------------- operators
class LinearOperator:
    """Symmetric n x n operator the device CG can apply (`matrix` generalised)."""

    shape = None
    dtype = None
    device = None

    def _struct(self):
        """(MgpOperator, keepalive objects)"""
        raise NotImplementedError

    def _struct_for(self, columns):
        """`_struct()` for a solve or product with `columns` right-hand sides (operators whose form depends on it)."""
        return self._struct()

    def rmatmul(self, P):
        """P [Bt,n] @ Op -> [Bt,n] (the layout of `state.p @ A`, reference :65)."""
        P = _hip.check_tensor(P, "P", dtype=self.dtype)
        if P.dim() != 2 or P.shape[1] != self.shape[0]:
            raise ValueError(f"P shape {tuple(P.shape)} does not match n={self.shape[0]}")
        out = torch.empty_like(P)
        if P.shape[0] == 0:
            return out
        hd = _hip.get_handle(self.device)
        st, keep = self._struct_for(P.shape[0])
        hd.check(hd.lib.mgp_operator_apply(hd.h, ctypes.byref(st), _hip.ptr(P), P.shape[0], _hip.ptr(out)))
        del keep
        return out

    def matmul(self, V):
        """Op @ V [n,R] -> [n,R]."""
        return self.rmatmul(V.t().contiguous()).t().contiguous()

    def diag(self):
        raise NotImplementedError

    def dense(self):
        """Explicit [n,n] matrix (tests, small n)."""
        eye = torch.eye(self.shape[0], dtype=self.dtype, device=self.device)
        return self.rmatmul(eye)


class DenseOperator(LinearOperator):
    def __init__(self, matrix):
        matrix = _hip.check_tensor(matrix, "matrix")
        if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1]:
            raise ValueError(f"matrix must be [n,n], got {tuple(matrix.shape)}")
        self.A = matrix
        self.shape = tuple(matrix.shape)
        self.dtype = matrix.dtype
        self.device = matrix.device

    def _struct(self):
        st = _hip.MgpOperator()
        st.kind = _hip.OP_DENSE
        st.dtype = _hip.dtype_code(self.A)
        st.n = self.shape[0]
        st.A = self.A.data_ptr()
        return st, (self.A,)

    def diag(self):
        return self.A.diagonal().clone()

    def dense(self):
        return self.A


# `wide="auto"` takes the many-column form from these sizes on: at every measured point with at least that many columns
# and that M it took at most 0.9 of the sweep form's best time, for both measured kernel configurations, one application
# and a 20-step solve alike; no smaller width does at any M (at 32 columns the SE solve at M = 2^17 is at 0.91).
# 2^12 is the smallest M measured (profiles/kmm_wide_times.json)
WIDE_MIN_COLUMNS = 48
WIDE_MIN_M = 1 << 12
WIDE_MAX_D = 32  # MGP_FUSED_MAX_D: above it, and in fp32, libmgp applies the sweep form whatever the kind


def check_wide(wide, name="wide"):
    """`wide` / `wide_solves` as given, or `ValueError`: False, True or "auto"."""
    if isinstance(wide, bool) or (isinstance(wide, str) and wide == "auto"):
        return wide
    raise ValueError(f"{name} must be False, True or 'auto', got {wide!r}")


def wide_auto(dtype, D, columns, M):
    """The rule behind `wide="auto"`: fp64, D <= 32, at least WIDE_MIN_COLUMNS columns and M >= WIDE_MIN_M."""
    return (dtype == torch.float64 and int(D) <= WIDE_MAX_D and int(columns) >= WIDE_MIN_COLUMNS
            and int(M) >= WIDE_MIN_M)


# `fused_anyd="auto"` takes the fused any-D sweeps (include/mgp_sweep_anyd.h) for fp64 inputs at
# FUSED_ANYD_AUTO_MIN_D <= D <= FUSED_ANYD_AUTO_MAX_D[columns]: per measured column count, the largest measured dimension
# up to which the fused form took at most 0.9 of the panel route's time at every measured point -- both kernels, both
# orientations, N = 2^18, M = 4096, D in {33, 48, 77, 90, 128, 512} (profiles/sweep_anyd_times.json).  One
# column: everywhere (0.10 - 0.85).  Eight: up to D = 128 (0.19 - 0.87; 1.14 for K_nm V at D = 512).  Five, which
# runs as a pass of 4 and a pass of 1 and so forms every distance twice: up to D = 48 (0.21 - 0.84; K_nm V is at 1.17 - 1.24
# from D = 77 on).  The panel route's time hardly depends on the column count, the fused form's does, so a column count
# that was not measured is not taken.
FUSED_ANYD_AUTO_MIN_D = 33
FUSED_ANYD_AUTO_MAX_D = {1: 512, 5: 48, 8: 128}


def check_fused_anyd(fused_anyd, name="fused_anyd"):
    """`fused_anyd` as given, or `ValueError`: False, True or "auto"."""
    return check_wide(fused_anyd, name)


def fused_anyd_auto(dtype, D, columns=1):
    """The rule behind `fused_anyd="auto"`: fp64, a measured column count, and
    FUSED_ANYD_AUTO_MIN_D <= D <= FUSED_ANYD_AUTO_MAX_D[columns]."""
    return (dtype == torch.float64 and int(columns) in FUSED_ANYD_AUTO_MAX_D
            and FUSED_ANYD_AUTO_MIN_D <= int(D) <= FUSED_ANYD_AUTO_MAX_D[int(columns)])


def use_fused_anyd(fused_anyd, dtype, D, columns=1):
    """Whether a product or operator with this setting takes the `_anyd` name or kind (which, in fp32 or at D <= 32, is
    the plain one inside libmgp) for `columns` right-hand sides."""
    if fused_anyd == "auto":
        return fused_anyd_auto(dtype, D, columns)
    return bool(fused_anyd)


# `fused_point_grads="auto"` takes `ops.k_dense_vjp_points` (include/mgp_points.h) for the point gradients of a dense
# kernel block [na, nb] where the fused call took at most 0.9 of the time of the torch route (`ops.k_dense_vjp` +
# `training.k_grad_points`) at every measured point: fp64 device tensors, D <= FUSED_POINT_GRADS_AUTO_MAX_D (the
# largest measured dimension) and na * nb >= FUSED_POINT_GRADS_AUTO_MIN_PAIRS (the smallest measured block, [4096, 256])
# -- K_mm at M = 2048 .. 16384 and K_mn [4096, 256], [4096, 1000], SE at D = 8, Matern-3/2 at D = 32 and D = 77
# (profiles/kvjp_points_times.json, "auto").  None for the pair count: no such region, "auto" means False.
FUSED_POINT_GRADS_AUTO_MIN_PAIRS = 1 << 20
FUSED_POINT_GRADS_AUTO_MAX_D = 77


def check_fused_point_grads(fused_point_grads, name="fused_point_grads"):
    """`fused_point_grads` as given, or `ValueError`: False, True or "auto"."""
    return check_wide(fused_point_grads, name)


def fused_point_grads_auto(dtype, D, na, nb):
    """The rule behind `fused_point_grads="auto"`: fp64, D <= FUSED_POINT_GRADS_AUTO_MAX_D and a block of at least
    FUSED_POINT_GRADS_AUTO_MIN_PAIRS pairs."""
    return (FUSED_POINT_GRADS_AUTO_MIN_PAIRS is not None and dtype == torch.float64
            and int(D) <= FUSED_POINT_GRADS_AUTO_MAX_D and int(na) * int(nb) >= FUSED_POINT_GRADS_AUTO_MIN_PAIRS)


def use_fused_point_grads(fused_point_grads, A, B):
    """Whether the point gradients of k(A, B) with this setting come from `ops.k_dense_vjp_points`.  fp32 tensors and
    host tensors take the torch route whatever the setting: the entry point is fp64 device code only."""
    if fused_point_grads is False or A.dtype != torch.float64 or B.dtype != torch.float64 or not (A.is_cuda and B.is_cuda):
        return False
    if fused_point_grads == "auto":
        return fused_point_grads_auto(A.dtype, A.shape[1], A.shape[0], B.shape[0])
    return True


# `fused_variance="auto"` takes `ops.knm_quadform` (include/mgp_predict.h) for the whole-test-set variance k C k of
# SGPR and CDGP where the fused kernel took at most 0.9 of the time of the composition (`ops.k_dense` + `ops.symm_matmul`
# + row sum) at every measured point: fp64, D <= 32 and M >= FUSED_VARIANCE_AUTO_MIN_M, both measured kernels, B = 2^16
# (profiles/predict_quadform_times.json).  None: no such region exists and "auto" means False -- measured,
# fused / composition: 0.98, 1.09, 1.09 at M = 1024, 4096, 8192 for SE at D = 8 and 1.68, 1.96, 1.98 for Matern-3/2 at D = 32.
FUSED_VARIANCE_AUTO_MIN_M = None
FUSED_VARIANCE_MAX_D = 32  # MGP_FUSED_MAX_D: above it, and in fp32, libmgp runs the composition itself


def check_fused_variance(fused_variance, name="fused_variance"):
    """`fused_variance` as given, or `ValueError`: False, True or "auto"."""
    return check_wide(fused_variance, name)


def fused_variance_auto(dtype, D, M):
    """The rule behind `fused_variance="auto"`."""
    return (FUSED_VARIANCE_AUTO_MIN_M is not None and dtype == torch.float64 and int(D) <= FUSED_VARIANCE_MAX_D
            and int(M) >= FUSED_VARIANCE_AUTO_MIN_M)


def use_fused_variance(fused_variance, dtype, D, M):
    """Whether a whole-test-set variance with this setting calls `ops.knm_quadform` (True: always) or composes the
    form from `ops.k_dense`, `ops.symm_matmul` and a row sum."""
    if fused_variance == "auto":
        return fused_variance_auto(dtype, D, M)
    return bool(fused_variance)


# `wide_anyd="auto"` takes the many-column form above 32 dimensions (`MGP_OP_KMM_LAMBDA_WIDE_ANYD`,
# include/mgp_sweep_anyd.h) where it took at most 0.9 of the time of the FASTER of the two existing routes (the plain
# kind's panels, `MGP_OP_KMM_LAMBDA_ANYD`) at every measured point of a region: fp64,
# WIDE_ANYD_AUTO_MIN_D <= D <= WIDE_ANYD_AUTO_MAX_D, at least WIDE_ANYD_AUTO_MIN_COLUMNS columns and
# M >= WIDE_ANYD_AUTO_MIN_M -- M in {2^12, 2^14, 2^16}, D in {33, 77, 90, 128, 512}, 16, 48, 64 and 256 columns, SE and
# Matern-3/2 (profiles/kmm_wide_anyd_times.json).  None for the column count: no such region, "auto" means
# False -- measured, new / faster existing route: 0.87 - 3.6 from 48 columns on (0.07 - 0.14 of MGP_OP_KMM_LAMBDA_ANYD at 256
# columns, but the plain kind's panels are faster still); at or below 0.9 only at 16 columns, and there not everywhere.
WIDE_ANYD_AUTO_MIN_COLUMNS = None
WIDE_ANYD_AUTO_MIN_M = 1 << 12
WIDE_ANYD_AUTO_MIN_D = 33
WIDE_ANYD_AUTO_MAX_D = 512


def check_wide_anyd(wide_anyd, name="wide_anyd"):
    """`wide_anyd` as given, or `ValueError`: False, True or "auto"."""
    return check_wide(wide_anyd, name)


def wide_anyd_auto(dtype, D, columns, M):
    """The rule behind `wide_anyd="auto"`."""
    return (WIDE_ANYD_AUTO_MIN_COLUMNS is not None and dtype == torch.float64
            and WIDE_ANYD_AUTO_MIN_D <= int(D) <= WIDE_ANYD_AUTO_MAX_D and int(columns) >= WIDE_ANYD_AUTO_MIN_COLUMNS
            and int(M) >= WIDE_ANYD_AUTO_MIN_M)


# `sym_anyd="auto"` takes the symmetric form above 32 dimensions (`MGP_OP_KXX_NOISE_SYM_ANYD`, include/mgp.h) where it
# took at most 0.9 of the time of the FASTER of the two existing routes (`MGP_OP_KXX_NOISE`'s panels,
# `MGP_OP_KXX_NOISE_ANYD`) at every measured point of a region: fp64, SYM_ANYD_AUTO_MIN_D <= D <= SYM_ANYD_AUTO_MAX_D,
# SYM_ANYD_AUTO_MIN_COLUMNS <= columns <= SYM_ANYD_AUTO_MAX_COLUMNS and N >= SYM_ANYD_AUTO_MIN_N
# -- N in {2^14, 2^16, 2^17}, D in {33, 77, 90, 128, 512}, 1, 5, 8, 16 and 32 columns, SE and Matern-3/2
# (profiles/kxx_sym_anyd_times.json).  Measured, new / faster existing route: 0.26 - 0.81 in the region
# below (96 points); outside it 0.82 - 1.10 at one column and 1.18 - 1.21 at D = 512 with 32 columns (0.59 - 0.75 at
# D = 512 with 5 to 16 columns: a valid region too, but the smaller one).  None for the column count would mean that no
# region qualifies and "auto" is False.
SYM_ANYD_AUTO_MIN_COLUMNS = 5
SYM_ANYD_AUTO_MAX_COLUMNS = 32
SYM_ANYD_AUTO_MIN_N = 1 << 14
SYM_ANYD_AUTO_MIN_D = 33
SYM_ANYD_AUTO_MAX_D = 128


def check_sym_anyd(sym_anyd, name="sym_anyd"):
    """`sym_anyd` as given, or `ValueError`: False, True or "auto"."""
    return check_wide(sym_anyd, name)


def sym_anyd_auto(dtype, D, columns, N):
    """The rule behind `sym_anyd="auto"`."""
    return (SYM_ANYD_AUTO_MIN_COLUMNS is not None and dtype == torch.float64
            and SYM_ANYD_AUTO_MIN_D <= int(D) <= SYM_ANYD_AUTO_MAX_D
            and SYM_ANYD_AUTO_MIN_COLUMNS <= int(columns) <= SYM_ANYD_AUTO_MAX_COLUMNS and int(N) >= SYM_ANYD_AUTO_MIN_N)


def anyd_matvec(fused_anyd, which, spec, X, *args, **kwargs):
    """`ops.knm_matvec`, `ops.kmn_matvec` or `ops.kxx_matvec` (`which` = "knm", "kmn", "kxx"; the arguments after `spec`
    are theirs), or its `_anyd` form under the rule of `use_fused_anyd`: the one helper the models route their direct
    products through."""
    V = args[1]  # (Z, V, ...) or, for kxx, (s2, V, ...)
    layout = args[2] if len(args) > 2 else kwargs.get("v_layout", kwargs.get("w_layout", ops.COLS))
    columns = V.shape[1] if layout == ops.COLS else V.shape[0]
    name = which + "_matvec" + ("_anyd" if use_fused_anyd(fused_anyd, X.dtype, spec.D, columns) else "")
    return getattr(ops, name)(spec, X, *args, **kwargs)


class KmmLambdaOperator(LinearOperator):
    """(k(Z,Z) + diag(lam)) applied matrix-free (row M2, matrix-free alternative).

    `wide=False`: libmgp's fused sweep, 8 right-hand sides per launch (`MGP_OP_KMM_LAMBDA`).  `wide=True`: the
    many-column form (`MGP_OP_KMM_LAMBDA_WIDE`: each kernel value evaluated once per 256 right-hand sides and contracted
    on the fp64 matrix cores; fp32 and D > 32 take the sweep form inside libmgp).  `wide="auto"`: the many-column form
    iff `wide_auto(dtype, D, columns, M)`, decided per solve or product, where the column count is known.

    `fused_anyd` (False, True or "auto"): at D > 32, where `wide` falls back to the sweep, `MGP_OP_KMM_LAMBDA_ANYD` -- the
    fused any-D sweep instead of kernel panels (fp64; fp32 gives the plain kind's bits).  At D <= 32 `wide` decides.

    `wide_anyd` (False, True or "auto"): at D > 32 in fp64, `MGP_OP_KMM_LAMBDA_WIDE_ANYD` -- the many-column form with
    the distance tiles on the matrix cores, each kernel value evaluated once per 256 right-hand sides and no kernel
    panel.  It is asked first: True, or "auto" and `wide_anyd_auto(dtype, D, columns, M)`, takes the kind; otherwise,
    and at D <= 32 or in fp32 always, `fused_anyd` and `wide` decide as above."""

    def __init__(self, kernel, Z, lam, wide=False, fused_anyd=False, wide_anyd=False):
        self.wide = check_wide(wide)
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.wide_anyd = check_wide_anyd(wide_anyd)
        self.Z = _hip.check_tensor(Z, "Z")
        self.lam = _hip.check_tensor(lam, "lam", dtype=self.Z.dtype).reshape(-1)
        M = self.Z.shape[0]
        if self.lam.shape[0] != M:
            raise ValueError("lam must have M entries")
        self.kernel = kernel
        self.spec = kernel.spec(self.Z.shape[1])
        self.shape = (M, M)
        self.dtype = self.Z.dtype
        self.device = self.Z.device

    def kind_for(self, columns):
        """The operator kind libmgp is handed for `columns` right-hand sides."""
        D = self.Z.shape[1]
        if D > WIDE_MAX_D and self.dtype == torch.float64 and self.wide_anyd is not False:
            if self.wide_anyd is True or wide_anyd_auto(self.dtype, D, max(int(columns), 1), self.shape[0]):
                return _hip.OP_KMM_LAMBDA_WIDE_ANYD
        if D > WIDE_MAX_D and use_fused_anyd(self.fused_anyd, self.dtype, D, max(int(columns), 1)):
            return _hip.OP_KMM_LAMBDA_ANYD
        wide = self.wide
        if wide == "auto":
            wide = wide_auto(self.dtype, D, columns, self.shape[0])
        return _hip.OP_KMM_LAMBDA_WIDE if wide else _hip.OP_KMM_LAMBDA

    def _struct(self):
        return self._struct_for(0)

    def _struct_for(self, columns):
        k = self.spec.struct(_hip.dtype_code(self.Z))
        st = _hip.MgpOperator()
        st.kind = self.kind_for(columns)
        st.dtype = k.dtype
        st.n = self.shape[0]
        st.kernel = ctypes.pointer(k)
        st.Z = self.Z.data_ptr()
        st.M = self.shape[0]
        st.lam = self.lam.data_ptr()
        return st, (k, self.Z, self.lam)

    def diag(self):
        return self.lam + self.kernel.variance


class KxxNoiseOperator(LinearOperator):
    """(k(X,X) + noise_variance I) applied matrix-free, each unordered pair of rows once (`mgp_kxx_matvec`): the
    system of exact GP regression, `GPR`'s K + s2 I without the [N,N] matrix.  Single device.

    `fused_anyd` (False, True or "auto"): `MGP_OP_KXX_NOISE_ANYD` -- at D > 32 in fp64 the fused any-D sweep instead of
    kernel panels; elsewhere the plain kind's bits.

    `sym_anyd` (False, True or "auto"): at D > 32 in fp64, `MGP_OP_KXX_NOISE_SYM_ANYD` -- each unordered pair of rows
    once on the fp64 matrix cores, up to 16 right-hand sides per pass.  It is asked first: True, or "auto" and
    `sym_anyd_auto(dtype, D, columns, N)`, takes the kind; otherwise, and at D <= 32 or in fp32 always, `fused_anyd`
    decides as above."""

    def __init__(self, kernel, X, noise_variance, fused_anyd=False, sym_anyd=False):
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.sym_anyd = check_sym_anyd(sym_anyd)
        self.X = _hip.check_tensor(X, "X")
        if self.X.dim() != 2:
            raise ValueError(f"X must be [N, D], got {tuple(self.X.shape)}")
        self.noise_variance = float(noise_variance)
        if not self.noise_variance >= 0.0:
            raise ValueError("noise_variance must be >= 0")
        self.kernel = kernel
        self.spec = kernel.spec(self.X.shape[1])
        N = self.X.shape[0]
        self.shape = (N, N)
        self.dtype = self.X.dtype
        self.device = self.X.device

    def _struct(self):
        return self._struct_for(1)

    def kind_for(self, columns):
        """The operator kind libmgp is handed for `columns` right-hand sides."""
        D, columns = self.X.shape[1], max(int(columns), 1)
        if D > WIDE_MAX_D and self.dtype == torch.float64 and self.sym_anyd is not False:
            if self.sym_anyd is True or sym_anyd_auto(self.dtype, D, columns, self.shape[0]):
                return _hip.OP_KXX_NOISE_SYM_ANYD
        anyd = use_fused_anyd(self.fused_anyd, self.dtype, D, columns)
        return _hip.OP_KXX_NOISE_ANYD if anyd else _hip.OP_KXX_NOISE

    def _struct_for(self, columns):
        k = self.spec.struct(_hip.dtype_code(self.X))
        st = _hip.MgpOperator()
        st.kind = self.kind_for(columns)
        st.dtype = k.dtype
        st.n = self.shape[0]
        st.kernel = ctypes.pointer(k)
        st.X = self.X.data_ptr()
        st.N = self.shape[0]
        st.s2 = self.noise_variance
        return st, (k, self.X)

    def diag(self):
        return torch.full((self.shape[0],), self.kernel.variance + self.noise_variance, dtype=self.dtype,
                          device=self.device)


class SgprNormalOperator(LinearOperator):
    """S = s2 (Kmm + jitter I) + K_mn K_nm over this rank's rows of X (row S1).

    K_nm is never materialised: each application is two fused N x M sweeps.  With
    `allreduce` set (see `parallel.make_allreduce`) the local [Bt,M] partial K_mn(K_nm p) is
    summed over ranks once per application; Kmm, Z and the CG state are replicated.

    `fused_anyd` (False, True or "auto"): `MGP_OP_SGPR_ANYD` -- at D > 32 in fp64 the two local sweeps run the fused
    any-D kernel instead of kernel panels (the collective is untouched); elsewhere the plain kind's bits.
    """

    def __init__(self, kernel, X, Z, noise_variance, jitter=0.0, allreduce=None, max_rhs=1, kmm_rows=None,
                 fused_anyd=False):
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.X = _hip.check_tensor(X, "X")
        self.Z = _hip.check_tensor(Z, "Z", dtype=self.X.dtype)
        if self.X.dim() != 2 or self.Z.dim() != 2 or self.X.shape[1] != self.Z.shape[1]:
            raise ValueError("X [N,D] and Z [M,D] must share D")
        self.kernel = kernel
        self.spec = kernel.spec(self.Z.shape[1])
        self.s2 = float(noise_variance)
        M = self.Z.shape[0]
        self.Kmm = ops.k_dense(self.spec, self.Z, self.Z, jitter=float(jitter))
        self.shape = (M, M)
        self.dtype = self.Z.dtype
        self.device = self.Z.device
        self.allreduce = allreduce
        # rows of Kmm whose s2*Kmm.p term this rank contributes before the all-reduce
        # (parallel.kmm_slab(M)); the slabs of all ranks must tile [0, M)
        self.kmm_rows = kmm_rows if allreduce is not None else None
        self._partial = None
        self._cb = None
        self.reserve(max_rhs)

    @property
    def _comm(self):
        """libmgp RCCL communicator when the exchange is native (parallel.AllReduce on backend nccl)."""
        return getattr(self.allreduce, "comm", None)

    def _world(self):
        w = getattr(self.allreduce, "world_size", None)
        if w is None:
            import torch.distributed as dist
            w = dist.get_world_size() if dist.is_initialized() else 1
        return int(w)

    def _ensure_partial(self, Bt):
        # hook path only (gloo rehearsal): the collective addresses this buffer as a torch tensor.
        # Bt*M partial + 1 agreement word (csrc/cg.hip: every rank must have taken part in a step)
        need = Bt * self.shape[0] + 1
        if self._partial is None or self._partial.numel() < need:
            self._partial = torch.empty((need,), dtype=self.dtype, device=self.device)
            buf = self._partial

            def _cb(ctx, ptr_, count, dtype_c, stream):
                try:
                    # libmgp enqueued the partial on `stream` (its handle's stream == torch's current one,
                    # _hip.get_handle); make that explicit for the collective
                    if stream:  # NULL = the legacy default stream, which is torch's default stream too
                        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=buf.device)):
                            self.allreduce(buf[:count])
                    else:
                        with torch.cuda.stream(torch.cuda.default_stream(buf.device)):
                            self.allreduce(buf[:count])
                    return 0
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1

            self._cb = _hip.ALLREDUCE_FN(_cb)

    def reserve(self, Bt):
        if self.allreduce is not None and self._comm is None:
            self._ensure_partial(Bt)

    def _struct(self):
        return self._struct_for(1)

    def _struct_for(self, columns):
        k = self.spec.struct(_hip.dtype_code(self.Z))
        st = _hip.MgpOperator()
        anyd = use_fused_anyd(self.fused_anyd, self.dtype, self.Z.shape[1], max(int(columns), 1))
        st.kind = _hip.OP_SGPR_ANYD if anyd else _hip.OP_SGPR
        st.dtype = k.dtype
        st.n = self.shape[0]
        st.kernel = ctypes.pointer(k)
        st.X = self.X.data_ptr() if self.X.shape[0] > 0 else None
        st.N = self.X.shape[0]
        st.Z = self.Z.data_ptr()
        st.M = self.shape[0]
        st.Kmm = self.Kmm.data_ptr()
        st.s2 = self.s2
        keep = (k, self.X, self.Z, self.Kmm)
        if self.allreduce is not None:
            if self._comm is not None:  # native RCCL: no callback, no staging buffer
                st.comm = self._comm.ptr
                keep += (self._comm,)
            else:
                st.allreduce = self._cb
                st.partial_buf = self._partial.data_ptr()
                st.world_size = self._world()
                keep += (self._partial, self._cb)
            if self.kmm_rows is not None:
                st.kmm_row_begin, st.kmm_row_end = int(self.kmm_rows[0]), int(self.kmm_rows[1])
            else:  # no slab given: rank 0 alone adds the replicated term
                import torch.distributed as dist
                st.kmm_row_begin, st.kmm_row_end = (0, self.shape[0]) if dist.get_rank() == 0 else (0, -1)
        return st, keep

    def rmatmul(self, P):
        self.reserve(P.shape[0])
        return super().rmatmul(P)

    def diag(self):
        """diag(S) = s2 diag(Kmm_j) + sum_i k(x_i, z_m)^2 (one fused sweep, summed over ranks)."""
        d = ops.kmn_sq_colsum(self.spec, self.X, self.Z)
        if self.allreduce is not None:
            self.allreduce(d)
        return d + self.s2 * self.Kmm.diagonal()


def as_operator(matrix):
    if isinstance(matrix, LinearOperator):
        return matrix
    if isinstance(matrix, torch.Tensor):
        return DenseOperator(matrix)
    raise TypeError("matrix must be a [n,n] CUDA tensor or a LinearOperator")


# --------------------------------------------------------------------------- preconditioners
class CGPreconditioner:
    """Protocol of reference :125-128: `__call__(vec [Bt,n], mat) -> (z, rz)`.

    The CG loop is device resident.  The preconditioners libmgp knows (Eye / Jacobi / Block / Dense)
    describe themselves through `_native(op)` and run inside its kernels.  ANY OTHER subclass -- a user's
    own `__call__`, as the reference allows -- is served through libmgp's callback kind: once per step the
    library hands the residual batch over, `__call__(r, mat)` is run on the solve's stream (torch ops), and
    its `z` goes back into the loop; `rz` is recomputed by the library exactly as `sum(z * r, -1)`."""

    def _native(self, op):
        return None

    def _native_for(self, op, Bt):
        nat = self._native(op)
        if nat is not None:
            return nat
        n = op.shape[0]
        r_buf = torch.empty((Bt, n), dtype=op.dtype, device=op.device)
        z_buf = torch.empty_like(r_buf)
        mat = op.A if isinstance(op, DenseOperator) else op  # what the reference passes as `mat` (:77,:89)

        def _cb(ctx, r_ptr, z_ptr, bt, nn, stream):
            try:
                st = torch.cuda.ExternalStream(stream, device=r_buf.device) if stream else \
                    torch.cuda.default_stream(r_buf.device)
                with torch.cuda.stream(st):
                    z = self(r_buf, mat)[0]
                    z_buf.copy_(z.reshape(z_buf.shape))
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        fn = _hip.PRECOND_FN(_cb)
        st = _hip.MgpPrecond()
        st.kind = _hip.PRE_CALLBACK
        st.apply = fn
        st.cb_r = r_buf.data_ptr()
        st.cb_z = z_buf.data_ptr()
        return st, (r_buf, z_buf, fn, mat)

    def __call__(self, vec, mat):
        raise NotImplementedError


class EyePreconditioner(CGPreconditioner):
    """reference :131-134: z = vec, rz = sum(vec^2, -1, keepdims)."""

    def _native(self, op):
        st = _hip.MgpPrecond()
        st.kind = _hip.PRE_EYE
        return st, ()

    def __call__(self, vec, mat):
        return vec, (vec * vec).sum(dim=-1, keepdim=True)


class JacobiPreconditioner(CGPreconditioner):
    """z = vec / diag(A) (build-side addition)."""

    def __init__(self, diagonal=None):
        self.diagonal = diagonal

    def _dinv(self, op):
        d = self.diagonal if self.diagonal is not None else op.diag()
        return (1.0 / d.reshape(-1)).to(op.dtype).contiguous()

    def _native(self, op):
        dinv = self._dinv(op)
        st = _hip.MgpPrecond()
        st.kind = _hip.PRE_JACOBI
        st.diag_inv = dinv.data_ptr()
        return st, (dinv,)

    def __call__(self, vec, mat):
        z = vec * self._dinv(as_operator(mat))[None, :]
        return z, (z * vec).sum(dim=-1, keepdim=True)


class BlockPreconditioner(CGPreconditioner):
    """Block-Jacobi with the reference's constructor `BlockPreconditioner(block_indices[nb,bs])`.

    The reference implementation (:137-157) gathers on the batch axis and never scatters back
    (shape-inconsistent with the solver, no call sites, untested); this is the intended
    operation -- per block solve A[idx,idx] z[idx] = vec[idx] -- and is parity-unpinned.
    Block inverses are formed once per solve on the host (nb small dense Cholesky problems).
    """

    def __init__(self, block_indices):
        bi = torch.as_tensor(block_indices)
        if bi.dim() != 2:
            raise ValueError("block_indices must be [num_blocks, block_size]")
        self.block_indices = bi.to(torch.int64)

    def _setup(self, op):
        A = op.dense()
        idx = self.block_indices.to(A.device)
        flat = idx.reshape(-1)
        if flat.numel() != torch.unique(flat).numel():
            raise ValueError("block indices must not overlap")
        if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= A.shape[0]):
            raise ValueError("block index out of range")
        blocks = A[idx[:, :, None], idx[:, None, :]].cpu().numpy().astype(np.float64)
        inv = np.empty_like(blocks)
        for k in range(blocks.shape[0]):
            L = np.linalg.cholesky(blocks[k])
            Li = np.linalg.inv(L)
            inv[k] = Li.T @ Li
        binv = torch.from_numpy(inv).to(device=A.device, dtype=A.dtype).contiguous()
        return idx.contiguous(), binv

    def _native(self, op):
        idx, binv = self._setup(op)
        st = _hip.MgpPrecond()
        st.kind = _hip.PRE_BLOCK
        st.block_size = idx.shape[1]
        st.num_blocks = idx.shape[0]
        st.block_index = idx.data_ptr()
        st.block_inv = binv.data_ptr()
        return st, (idx, binv)

    def __call__(self, vec, mat):
        idx, binv = self._setup(as_operator(mat))
        z = vec.clone()
        for k in range(idx.shape[0]):
            z[:, idx[k]] = vec[:, idx[k]] @ binv[k].t()
        return z, (z * vec).sum(dim=-1, keepdim=True)


class DensePreconditioner(CGPreconditioner):
    """z = vec @ Pinv for a symmetric positive-definite `Pinv` [n, n] held on the device
    (build-side addition; the product runs on the same symmetric-product kernels as `p @ A`)."""

    def __init__(self, inverse):
        self.inverse = _hip.check_tensor(inverse, "inverse")
        if self.inverse.dim() != 2 or self.inverse.shape[0] != self.inverse.shape[1]:
            raise ValueError("inverse must be a square [n, n] tensor")

    def _native(self, op):
        if self.inverse.shape[0] != op.shape[0] or self.inverse.dtype != op.dtype:
            raise ValueError(f"preconditioner is {tuple(self.inverse.shape)} {self.inverse.dtype}, "
                             f"operator is n={op.shape[0]} {op.dtype}")
        st = _hip.MgpPrecond()
        st.kind = _hip.PRE_DENSE
        st.dense_inv = self.inverse.data_ptr()
        return st, (self.inverse,)

    def __call__(self, vec, mat):
        z = ops.symm_matmul(self.inverse, vec)
        return z, (z * vec).sum(dim=-1, keepdim=True)


class SubsampledNormalPreconditioner(DensePreconditioner):
    """Dense preconditioner for the SGPR normal matrix S = s2 Kmm + Kmn Knm (`SgprNormalOperator`):

        P = s2 Kmm + (N / n_s) Ks^T Ks,   Ks = k(X[sample], Z),

    i.e. the same matrix with the N-row Gram term replaced by an n_s-row Monte-Carlo estimate
    (n_s = `rows_per_inducing` * M rows drawn without replacement, per rank from its own shard and
    all-reduced, so every rank holds the same P).  `P^-1` comes from one Cholesky on the device.
    Cost: one `kmn_knm` contraction over n_s rows -- a few CG steps' worth -- against a cut in
    the step count from O(cond) to tens (PCG section)."""

    def __init__(self, operator, rows_per_inducing=32, seed=0, jitter=0.0):
        if not isinstance(operator, SgprNormalOperator):
            raise TypeError("SubsampledNormalPreconditioner needs an SgprNormalOperator")
        X, Z = operator.X, operator.Z
        M, N_local = Z.shape[0], X.shape[0]
        world = 1
        if operator.allreduce is not None:  # the ranks the operator's own exchange spans (it may be a sub-group)
            world = int(getattr(operator.allreduce, "world_size", 0) or 0)
            if world < 1:
                import torch.distributed as dist
                world = dist.get_world_size() if dist.is_initialized() else 1
        n_s = min(N_local, max(1, (int(rows_per_inducing) * M + world - 1) // world))
        # shards hold different rows, so one seed gives independent samples per rank
        gen = torch.Generator(device=X.device).manual_seed(int(seed))
        sel = torch.randperm(N_local, generator=gen, device=X.device)[:n_s]  # on the device: 10 ms less
        G = ops.kmn_knm(operator.spec, X[sel].contiguous(), Z)  # Ks^T Ks  [M, M]
        tot = torch.tensor([float(n_s), float(N_local)], dtype=torch.float64, device=X.device)
        if operator.allreduce is not None:
            operator.allreduce(G.view(-1))
            operator.allreduce(tot)
        n_tot, N_tot = float(tot[0]), float(tot[1])
        # factorise in fp64 whatever the operator's dtype: P inherits cond(S) ~ cond(Kmm)^2
        P = operator.s2 * operator.Kmm.double() + (N_tot / n_tot) * G.double()
        P = 0.5 * (P + P.t())
        eye = torch.eye(M, dtype=P.dtype, device=P.device)
        # In a dtype narrower than fp64 the operator itself is only known to eps ||S||: eigenvalues of
        # P below that are noise, and P^-1 rounded to that dtype would not stay positive definite
        # (measured: the fp32 solve diverges).  Lift them to the rounding level -- nothing is lost.
        eps = float(torch.finfo(operator.dtype).eps)
        bump = float(jitter) if operator.dtype == torch.float64 else max(float(jitter), eps * float(P.diagonal().sum()))
        floor = eps * float(P.diagonal().mean())
        for _ in range(12):
            L, info = torch.linalg.cholesky_ex(P + bump * eye if bump else P)
            if int(info) == 0:
                break
            # not numerically positive definite (rounding of the Gram term in the operator's dtype):
            # lift the spectrum by a step relative to that rounding and retry
            bump = max(10.0 * bump, floor)
        else:
            raise RuntimeError("SubsampledNormalPreconditioner: P is not positive definite")
        self.jitter_used = bump
        Pinv = torch.cholesky_inverse(L)
        self.sample_rows = int(n_tot)
        super().__init__((0.5 * (Pinv + Pinv.t())).to(operator.dtype).contiguous())


# `wide="auto"` of `PivotedCholeskyPreconditioner` takes the many-column application (`MGP_PRE_LOWRANK_WIDE`) from this
# many right-hand sides on.  The rule, fixed before measuring: the smallest measured width such that at every measured
# point with at least that many columns (rank 128; 16, 24, 32, 48, 64, 128, 256 columns; n = 2^12, 2^14, 2^16, 2^17) a
# CG start-up with the many-column form took at most 0.9 of the same start-up with the 16-column form.  It held at all
# 28 points, from 0.82 (16 columns, n = 2^12) down to 0.10 (256 columns), so the rule gives the smallest width measured;
# below it nothing was measured and "auto" keeps the 16-column form (tools/run_cdgp_precond.py,
# profiles/cdgp_precond_times.json).  None would mean that no width qualified.
LOWRANK_WIDE_MIN_COLUMNS = 16


def lowrank_wide_auto(dtype, columns):
    """The rule behind `PivotedCholeskyPreconditioner(wide="auto")`: fp64 and at least LOWRANK_WIDE_MIN_COLUMNS columns."""
    return (dtype == torch.float64 and LOWRANK_WIDE_MIN_COLUMNS is not None
            and int(columns) >= LOWRANK_WIDE_MIN_COLUMNS)


class PivotedCholeskyPreconditioner(CGPreconditioner):
    """P = L^T L + D with L [k, N] the rank-k partial pivoted Cholesky factor of K = k(X, X) and D = s2 I: the
    standard preconditioner of the exact-GP system K + s2 I (Harbrecht et al. 2012; Gardner et al. 2018).  Build-side
    addition, opt-in: `ConjugateGradient(thr, preconditioner=PivotedCholeskyPreconditioner())`.

    For matrix-free CDGP (`KmmLambdaOperator`, either form: `CGGP(..., matrix_free=True)`,
    `TrainableCGGP(..., matrix_free=True)`) the same with K = k(Z, Z) and D = diag(lambda), lambda = s2 / cluster size.
    L depends on (Z, kernel, rank, rel_tol) only and is kept while those stay; the Woodbury part (B, D^-1, log|P|) is
    re-formed when the values of lambda change (compared by value: the models make a new lambda tensor per call).  The
    factor is a constant of a solve: it is built from detached values and no gradient flows through it.

    `wide` (False, True or "auto") picks, per solve, the kernels that apply P^-1 inside the device CG loop: False
    libmgp's `MGP_PRE_LOWRANK` (16 right-hand sides per group of launches), True its many-column form
    `MGP_PRE_LOWRANK_WIDE` (256 per group, both products on the fp64 matrix cores), "auto" the many-column form from
    `LOWRANK_WIDE_MIN_COLUMNS` right-hand sides on.  fp32 solves and recording solves (`ops.pcg_solve_record`) take
    `MGP_PRE_LOWRANK` whatever `wide` says; `solve()` is `mgp_lowrank_apply` always.

    P^-1 = D^-1 - B^T B with B = C^-1 L D^-1 and C C^T = I_k + L D^-1 L^T (Woodbury), O(N k) per application;
    log|P| = 2 sum log C_ii + sum log D in closed form; z = L^T g1 + sqrt(D) g2 is a draw from N(0, P).

    Inside the device CG loop it is libmgp's `MGP_PRE_LOWRANK` kind.  The factor (`mgp_kxx_pivchol`, matrix-free) is
    built for a `KxxNoiseOperator` or a `KmmLambdaOperator` on first use, cached, and rebuilt when the operator's kernel
    parameters, noise or points change; any other operator is a `TypeError`.  `rank_` holds the rank reached
    (`rel_tol` may stop the factor early).  It pays where K has a low-rank part -- low-dimensional inputs, smooth kernels -- and does nothing for
    high-dimensional inputs with short lengthscales.  `set_factor(L, D)` installs a hand-made factor
    (any device, also the CPU: `__call__`, `log_det` and `sample` are plain torch)."""

    def __init__(self, rank=128, rel_tol=1e-10, wide=False):
        self.wide = check_wide(wide)
        self.rank = int(rank)
        if not 1 <= self.rank <= 1024:
            raise ValueError("rank must be in [1, 1024]")
        self.rel_tol = float(rel_tol)
        if not 0.0 <= self.rel_tol < 1.0:
            raise ValueError("rel_tol must be in [0, 1)")
        self.rank_ = None
        self.L = self.D = self.diag_inv = self.B = self.piv = None
        self._log_det = None
        self._key = self._key_ref = None
        self._normals = None
        self._kmm_key = self._kmm_L = self._kmm_lam = None  # KmmLambdaOperator: the key of L, L, the lambda B was formed with

    def set_factor(self, L, D):
        """P = diag(D) + L^T L from a given L [k, n] and positive D (a number or [n])."""
        n = L.shape[1]
        D = torch.as_tensor(D, dtype=L.dtype, device=L.device)
        D = D.expand(n).contiguous() if D.dim() == 0 else D.reshape(n).contiguous()
        if not bool((D > 0).all()):
            raise ValueError("D must be positive")
        self.L, self.D = L.contiguous(), D
        self.diag_inv = (1.0 / D).contiguous()
        k = L.shape[0]
        LD = self.L * self.diag_inv[None, :]
        M = torch.eye(k, dtype=L.dtype, device=L.device) + LD @ self.L.t()
        C = torch.linalg.cholesky(0.5 * (M + M.t()))
        # B = C^-1 (L D^-1) through the explicit k x k inverse of the triangular factor and one GEMM: a triangular solve
        # with n right-hand sides is not served by the BLAS at n = 2^17 (cond(C) = sqrt(cond(I + L D^-1 L^T)), harmless)
        Cinv = torch.linalg.solve_triangular(C, torch.eye(k, dtype=L.dtype, device=L.device), upper=False)
        self.B = (Cinv @ LD).contiguous()
        self._log_det = float(2.0 * torch.log(C.diagonal()).sum() + torch.log(D).sum())
        self.rank_ = k
        self._key = None
        return self

    def _prepare(self, op):
        """Build (or reuse) the factor of a `KxxNoiseOperator` or a `KmmLambdaOperator`; a factor given through
        `set_factor` stays."""
        if self.L is not None and self._key is None:
            if self.L.shape[1] != op.shape[0]:
                raise ValueError(f"the factor has n={self.L.shape[1]}, the operator n={op.shape[0]}")
            return
        if not isinstance(op, (KxxNoiseOperator, KmmLambdaOperator)):
            raise TypeError("PivotedCholeskyPreconditioner builds its factor for a KxxNoiseOperator (K + s2 I of exact "
                            "GP regression) or a KmmLambdaOperator (K_mm + Lambda of matrix-free CDGP) only, got "
                            f"{type(op).__name__}; use CGGP(..., matrix_free=True) for CDGP, or set_factor(L, D) for "
                            "another matrix")
        if op.dtype != torch.float64:
            raise TypeError("PivotedCholeskyPreconditioner needs an fp64 operator (the factor is fp64 only)")
        if isinstance(op, KmmLambdaOperator):
            return self._prepare_kmm(op)
        if not op.noise_variance > 0.0:
            raise ValueError("PivotedCholeskyPreconditioner needs noise_variance > 0")
        X = op.X
        key = (id(X), X._version, tuple(X.shape), op.spec.kind, op.spec.variance, tuple(op.spec.lengthscales),
               op.noise_variance, self.rank, self.rel_tol)
        if key == self._key:
            return
        L, piv, _ = ops.kxx_pivchol(op.spec, X, self.rank, self.rel_tol)
        self.set_factor(L, op.noise_variance)
        self.piv = piv
        self._key, self._key_ref = key, X  # the reference keeps id(X) from being reused

    def _prepare_kmm(self, op):
        """K = k(Z, Z), D = diag(lambda): L on the key of the exact-GP path with Z for X, B on the values of lambda."""
        lam = op.lam.detach()
        if not bool((lam > 0).all()):
            raise ValueError("PivotedCholeskyPreconditioner needs lambda > 0 everywhere")
        Z = op.Z
        key = (id(Z), Z._version, tuple(Z.shape), op.spec.kind, op.spec.variance, tuple(op.spec.lengthscales),
               self.rank, self.rel_tol)
        fresh = key != self._kmm_key
        if fresh:
            L, piv, _ = ops.kxx_pivchol(op.spec, Z.detach(), self.rank, self.rel_tol)
            self._kmm_key, self._kmm_L, self.piv = key, L, piv
            self._key_ref = Z  # keeps id(Z) from being reused
        if fresh or self._kmm_lam is None or self._key != ("kmm", key) or not torch.equal(lam, self._kmm_lam):
            self.set_factor(self._kmm_L, lam)
            self._kmm_lam = lam.clone()
            self._key = ("kmm", key)  # not a hand-made factor: the next operator is looked at again

    def _wide_for(self, dtype, columns):
        wide = self.wide
        if wide == "auto":
            wide = lowrank_wide_auto(dtype, columns)
        return bool(wide) and dtype == torch.float64

    def _native_for(self, op, Bt):
        st, keep = self._native(op)
        if st.kind == _hip.PRE_LOWRANK and self._wide_for(op.dtype, Bt):
            st.kind = _hip.PRE_LOWRANK_WIDE
        return st, keep

    def _native(self, op):
        self._prepare(op)
        if self.B.dtype != op.dtype or self.B.device != op.device:
            raise ValueError("the factor and the operator differ in dtype or device")
        st = _hip.MgpPrecond()
        if self.rank_ == 0:  # nothing low-rank found (rel_tol stopped at once): P = D
            st.kind = _hip.PRE_JACOBI
            st.diag_inv = self.diag_inv.data_ptr()
            return st, (self.diag_inv,)
        st.kind = _hip.PRE_LOWRANK
        st.diag_inv = self.diag_inv.data_ptr()
        st.dense_inv = self.B.data_ptr()
        st.num_blocks = self.rank_
        return st, (self.diag_inv, self.B)

    def _require(self):
        if self.B is None:
            raise RuntimeError("no factor yet: solve with a KxxNoiseOperator or a KmmLambdaOperator first, or call "
                               "set_factor(L, D)")

    def solve(self, vec):
        """P^-1 applied to the rows of vec [Bt, n]: `mgp_lowrank_apply` on the GPU, torch elsewhere."""
        self._require()
        if vec.is_cuda and self.rank_ > 0:
            return ops.lowrank_apply(self.diag_inv, self.B, vec.contiguous())
        return vec * self.diag_inv[None, :] - (vec @ self.B.t()) @ self.B

    def __call__(self, vec, mat):
        if self.B is None or (self._key is not None and isinstance(mat, (KxxNoiseOperator, KmmLambdaOperator))):
            self._prepare(as_operator(mat))
        z = vec * self.diag_inv[None, :] - (vec @ self.B.t()) @ self.B
        return z, (z * vec).sum(dim=-1, keepdim=True)

    def log_det(self):
        """log|P| = 2 sum log C_ii + sum log D (= ... + N log s2 for the exact-GP system)."""
        self._require()
        return self._log_det

    def sample(self, t, generator=None, seed=0):
        """Z [n, t] = L^T g1 + sqrt(D) g2 with g1 [rank, t], g2 [n, t] standard normal from a seeded CPU
        `torch.Generator` (`generator`, or one made from `seed`), so E[Z Z^T] / t = P.  With `seed` the normals are
        drawn once for (seed, n, t) and for the full `rank`, so a rebuilt factor re-forms Z from the same draws."""
        self._require()
        n, t = self.L.shape[1], int(t)
        if generator is not None:
            g2 = torch.randn((n, t), generator=generator, dtype=torch.float64)
            g1 = torch.randn((self.rank, t), generator=generator, dtype=torch.float64)
        else:
            nk = (int(seed), n, t, self.rank)
            if self._normals is None or self._normals[0] != nk:
                gen = torch.Generator().manual_seed(int(seed))
                g2 = torch.randn((n, t), generator=gen, dtype=torch.float64)
                g1 = torch.randn((self.rank, t), generator=gen, dtype=torch.float64)
                self._normals = (nk, g1.to(self.L.device), g2.to(self.L.device))
            g1, g2 = self._normals[1], self._normals[2]
        g1 = g1.to(device=self.L.device, dtype=self.L.dtype)[:self.rank_]
        g2 = g2.to(device=self.L.device, dtype=self.L.dtype)
        return self.L.t() @ g1 + torch.sqrt(self.D)[:, None] * g2


# --------------------------------------------------------------------------- solver
def _solve_device(op, rhs, initial_solution, error_threshold, preconditioner, max_iterations,
                  max_steps_cycle, min_float, check_every):
    rhs = _hip.check_tensor(rhs, "rhs", dtype=op.dtype)
    if rhs.dim() != 2 or rhs.shape[1] != op.shape[0]:
        raise ValueError(f"rhs must be [Bt, n={op.shape[0]}], got {tuple(rhs.shape)}")
    Bt, n = rhs.shape
    v0 = None
    if initial_solution is not None:
        v0 = _hip.check_tensor(initial_solution, "initial_solution", dtype=op.dtype, shape=(Bt, n))
    if preconditioner is None:
        preconditioner = EyePreconditioner()
    if max_iterations is None:
        max_iterations = n  # reference :47-48
    max_iterations = int(max_iterations)
    max_steps_cycle = int(max_steps_cycle)
    if max_steps_cycle < 1:
        raise ValueError("max_steps_cycle must be >= 1")
    sol = torch.empty_like(rhs)
    err = torch.empty((Bt, 1), dtype=op.dtype, device=op.device)
    stats = _hip.MgpCgStats()
    if Bt > 0:
        if isinstance(op, SgprNormalOperator):
            op.reserve(Bt)
        hd = _hip.get_handle(op.device)
        st, keep = op._struct_for(Bt)
        pst, pkeep = preconditioner._native_for(op, Bt)
        hd.check(hd.lib.mgp_pcg_solve(
            hd.h, ctypes.byref(st), ctypes.byref(pst), _hip.ptr(rhs), _hip.ptr(v0), Bt,
            float(error_threshold), max_iterations, max_steps_cycle, float(min_float), int(check_every),
            _hip.ptr(sol), _hip.ptr(err), ctypes.byref(stats)))
        del keep, pkeep
    return sol, stats, err


def _adjoint_solve(op, sol, rhs, err, dx, cfg, zero_start):
    """db with db A = dx for the backward pass of a solve `sol A = rhs` (rows; `err` = 0.5 rz of that solve): the
    shortcut or the warm start of `_CGFunction` where they apply, else the device CG from zero."""
    dx = dx.contiguous()
    db = None
    warm = None
    if zero_start:
        rr = (rhs * rhs).sum(dim=1, keepdim=True)
        c = (dx * rhs).sum(dim=1, keepdim=True) / torch.where(rr > 0, rr, torch.ones_like(rr))
        tol = 1e-12 if dx.dtype == torch.float64 else 1e-5
        if bool(((dx - c * rhs).abs().max() <= tol * dx.abs().max()).item()):
            # err = 0.5 rz of the forward solve (= 0.5||r||^2 for the identity preconditioner; for
            # others recompute the true residual of c*sol below through the warm start)
            thr = float(cfg[0])
            plain = cfg[1] is None or isinstance(cfg[1], EyePreconditioner)
            if plain and bool(((c * c) * err <= thr).all().item()):
                db = c * sol
                conjugate_gradient.backward_shortcuts += 1
            else:
                warm = (c * sol).contiguous()
                conjugate_gradient.backward_warm_starts += 1
    if db is None:
        db, _, _ = _solve_device(op, dx, warm, *cfg)
    return db


class _CGFunction(torch.autograd.Function):
    """Custom gradient of reference :100-118: db = CG(A, dx) from zero, dA = -solution^T @ db.

    Shortcut: when every row of the incoming `dx` is a multiple of the same row of the forward
    right-hand side -- `dx_b = c_b rhs_b`, which is what a loss that touches the solution only through
    `sum(rhs * solution)` sends back (the predictive-variance term `sum(Kmn * W)` of the ELBO,
    `cggp/models.py:343`) -- then `c_b solution_b` solves `db A = dx` with residual `c_b r_b`, i.e.
    `0.5||r||^2 = c_b^2 err_b`.  It is returned as it stands only when that already meets the reference's
    absolute rule `<= error_threshold` for every row (the second solve would then stop at step 0 or
    land within the same tolerance); otherwise it is the INITIAL SOLUTION of the second solve, which
    then needs a few steps instead of a full solve.  `conjugate_gradient.backward_shortcuts` counts the
    first case, `backward_warm_starts` the second."""

    @staticmethod
    def forward(ctx, matrix, rhs, initial_solution, cfg):
        op = as_operator(matrix)
        sol, stats, err = _solve_device(op, rhs, initial_solution, *cfg)
        ctx.cfg = cfg
        ctx.matrix = matrix
        ctx.zero_start = initial_solution is None
        ctx.save_for_backward(sol, rhs, err)
        ctx.mark_non_differentiable(err)
        ctx.stats = stats
        return sol, err

    @staticmethod
    def backward(ctx, dx, _derr):
        sol, rhs, err = ctx.saved_tensors
        db = _adjoint_solve(as_operator(ctx.matrix), sol, rhs, err, dx, ctx.cfg, ctx.zero_start)
        dA = None
        if isinstance(ctx.matrix, torch.Tensor) and ctx.needs_input_grad[0]:
            dA = -(sol.t() @ db)  # [n,Bt]x[Bt,n] library GEMM (rank-Bt update)
        return dA, db, None, None


def conjugate_gradient(matrix, rhs, initial_solution, error_threshold, preconditioner=None,
                       max_iterations=None, max_steps_cycle=100, *, min_float=MIN_FLOAT, check_every=10):
    """Solve `V A = B` for row batches (reference `conjugate_gradient`, :24-122).

    Returns `(solution [Bt,n], (steps, error [Bt,1]))` with `steps` an int32 scalar tensor and
    `error = 0.5 * rz_final` (reference :96-98,120).
    """
    cfg = (error_threshold, preconditioner, max_iterations, max_steps_cycle, min_float, check_every)
    needs_grad = torch.is_grad_enabled() and (
        (isinstance(matrix, torch.Tensor) and matrix.requires_grad) or rhs.requires_grad)
    if needs_grad:
        sol, err = _CGFunction.apply(matrix, rhs, initial_solution, cfg)
        steps = torch.tensor(-1, dtype=torch.int32)  # not tracked on the differentiable path
        return sol, (steps, err)
    op = as_operator(matrix)
    sol, stats, err = _solve_device(op, rhs, initial_solution, *cfg)
    steps = torch.tensor(stats.iterations, dtype=torch.int32)
    conjugate_gradient.last_stats = stats
    return sol, (steps, err)


conjugate_gradient.last_stats = None
conjugate_gradient.backward_shortcuts = 0
conjugate_gradient.backward_warm_starts = 0


class ConjugateGradient:
    """Callable facade of reference :160-212 (column layout in and out, stats dropped)."""

    def __init__(self, error_threshold, preconditioner=None, max_iterations=None, max_steps_cycle=None,
                 *, min_float=MIN_FLOAT, check_every=10):
        self.error_threshold = error_threshold
        if preconditioner is None:
            preconditioner = EyePreconditioner()
        self.preconditioner = preconditioner
        self.max_iterations = max_iterations
        self.max_steps_cycle = max_steps_cycle
        self.min_float = min_float
        self.check_every = check_every
        self.last_stats = None

    def config(self, n):
        """The argument tuple of the device solve for an n x n system, defaults resolved as the reference does."""
        max_iterations = self.max_iterations if self.max_iterations is not None else n  # :190-192
        max_steps_cycle = self.max_steps_cycle if self.max_steps_cycle is not None else max_iterations + 1  # :194-196
        return (self.error_threshold, self.preconditioner, max_iterations, max_steps_cycle, self.min_float,
                self.check_every)

    def solve_with_stats(self, matrix, rhs, initial_solution=None):
        """`stats_conjugate_gradient` of `cggp/paper_condition_wasserstein.py:262-294`."""
        rhs_t = rhs.t().contiguous()  # :183
        init_t = None if initial_solution is None else initial_solution.t().contiguous()  # :185-188
        thr, pre, max_iterations, max_steps_cycle, min_float, check_every = self.config(matrix.shape[-1])
        sol, stats = conjugate_gradient(
            matrix, rhs_t, init_t, thr, preconditioner=pre, max_iterations=max_iterations,
            max_steps_cycle=max_steps_cycle, min_float=min_float, check_every=check_every)
        self.last_stats = stats
        return sol.t().contiguous(), stats  # :211

    def __call__(self, matrix, rhs, initial_solution=None):
        return self.solve_with_stats(matrix, rhs, initial_solution)[0]
