"""Tensor-level wrappers over the C ABI (include/mgp.h).  No arithmetic happens here.

Every function takes CUDA(HIP) torch tensors, validates shapes on the host (the kernels
assume them) and enqueues libmgp work on torch's current stream.
"""

import ctypes

import torch

from . import _hip
from ._hip import COLS, ROWS  # noqa: F401


class KernelSpec:
    """Host-side kernel hyper-parameters in the form libmgp takes them (row K2)."""

    def __init__(self, kind, variance, lengthscales, D):
        self.kind = kind
        self.variance = float(variance)
        ls = [float(x) for x in (lengthscales if hasattr(lengthscales, "__len__") else [lengthscales])]
        self.lengthscales = ls * D if len(ls) == 1 else ls
        self.D = int(D)
        if len(self.lengthscales) != self.D:
            raise ValueError(f"lengthscales has {len(self.lengthscales)} entries, inputs have D={self.D}")

    def struct(self, dtype_c):
        return _hip.make_kernel_struct(self.kind, dtype_c, self.D, self.variance, self.lengthscales)


def _points(t, name, D=None, dtype=None):
    t = _hip.check_tensor(t, name, dtype=dtype)
    if t.dim() != 2:
        raise ValueError(f"{name} must be [n, D], got {tuple(t.shape)}")
    if D is not None and t.shape[1] != D:
        raise ValueError(f"{name} has D={t.shape[1]}, expected {D}")
    return t


def knm_matvec(spec, X, Z, V, v_layout=COLS, out_layout=None):
    """out = k(X, Z) @ V.  V [M,R] (COLS) or [R,M] (ROWS); out [N,R] or [R,N]."""
    return _knm_matvec("mgp_knm_matvec", spec, X, Z, V, v_layout, out_layout)


def knm_matvec_anyd(spec, X, Z, V, v_layout=COLS, out_layout=None):
    """`knm_matvec` by `mgp_knm_matvec_anyd` (include/mgp_sweep_anyd.h): fp64 at D > 32 the fused any-D sweep on the
    matrix cores, no kernel panel in memory; fp32 or D <= 32 exactly `knm_matvec`."""
    return _knm_matvec("mgp_knm_matvec_anyd", spec, X, Z, V, v_layout, out_layout)


def _knm_matvec(entry, spec, X, Z, V, v_layout, out_layout):
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    V = _hip.check_tensor(V, "V", dtype=X.dtype)
    if V.dim() != 2:
        raise ValueError("V must be 2-D")
    M = Z.shape[0]
    R = V.shape[1] if v_layout == COLS else V.shape[0]
    if (V.shape[0] if v_layout == COLS else V.shape[1]) != M:
        raise ValueError(f"V shape {tuple(V.shape)} does not match M={M}")
    out_layout = v_layout if out_layout is None else out_layout
    N = X.shape[0]
    out = torch.empty((N, R) if out_layout == COLS else (R, N), dtype=X.dtype, device=X.device)
    if N == 0 or R == 0:
        return out
    # M == 0 (empty inducing set) goes through the C-ABI too: libmgp writes the zeros
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    hd.check(getattr(hd.lib, entry)(hd.h, ctypes.byref(k), _hip.ptr(X), N, _hip.ptr(Z), M, _hip.ptr(V), R,
                                     v_layout, _hip.ptr(out), out_layout))
    return out


def kxx_matvec(spec, X, s2, V, v_layout=COLS, out_layout=None):
    """out = (k(X, X) + s2 I) @ V, each unordered pair of rows evaluated once (fp64, D <= 32).
    V [N,R] (COLS) or [R,N] (ROWS); out [N,R] or [R,N]."""
    return _kxx_matvec("mgp_kxx_matvec", spec, X, s2, V, v_layout, out_layout)


def kxx_matvec_anyd(spec, X, s2, V, v_layout=COLS, out_layout=None):
    """`kxx_matvec` by `mgp_kxx_matvec_anyd`: fp64 at D > 32 the fused any-D sweep of X against itself with s2 V as its
    addend (every ordered pair); fp32 or D <= 32 exactly `kxx_matvec`."""
    return _kxx_matvec("mgp_kxx_matvec_anyd", spec, X, s2, V, v_layout, out_layout)


def _kxx_matvec(entry, spec, X, s2, V, v_layout, out_layout):
    X = _points(X, "X", spec.D)
    V = _hip.check_tensor(V, "V", dtype=X.dtype)
    if V.dim() != 2:
        raise ValueError("V must be 2-D")
    N = X.shape[0]
    R = V.shape[1] if v_layout == COLS else V.shape[0]
    if (V.shape[0] if v_layout == COLS else V.shape[1]) != N:
        raise ValueError(f"V shape {tuple(V.shape)} does not match N={N}")
    s2 = float(s2)
    if not s2 >= 0.0:
        raise ValueError("s2 must be >= 0")
    out_layout = v_layout if out_layout is None else out_layout
    out = torch.empty((N, R) if out_layout == COLS else (R, N), dtype=X.dtype, device=X.device)
    if N == 0 or R == 0:
        return out
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    hd.check(getattr(hd.lib, entry)(hd.h, ctypes.byref(k), _hip.ptr(X), N, s2, _hip.ptr(V), R, v_layout,
                                     _hip.ptr(out), out_layout))
    return out


def kxx_grad(spec, X, U, V, layout=COLS):
    """(sum_r u_r^T dK/dvariance v_r: float, [sum_r u_r^T dK/dl_d v_r for d < D]) for K = k(X, X) without noise, every
    pair of rows (diagonal included), nothing N x N formed.  U, V [N, R] (COLS) or [R, N] (ROWS)."""
    X = _points(X, "X", spec.D)
    U = _hip.check_tensor(U, "U", dtype=X.dtype)
    V = _hip.check_tensor(V, "V", dtype=X.dtype)
    N = X.shape[0]
    if U.dim() != 2 or U.shape != V.shape or (U.shape[0] if layout == COLS else U.shape[1]) != N:
        raise ValueError(f"U {tuple(U.shape)} and V {tuple(V.shape)} must both be [N={N}, R] (COLS) or [R, N] (ROWS)")
    R = U.shape[1] if layout == COLS else U.shape[0]
    dvar = ctypes.c_double(0.0)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)()
    if N and R:
        hd = _hip.get_handle(X.device)
        k = spec.struct(_hip.dtype_code(X))
        hd.check(hd.lib.mgp_kxx_grad(hd.h, ctypes.byref(k), _hip.ptr(X), N, _hip.ptr(U), _hip.ptr(V), R, layout,
                                     ctypes.byref(dvar), dls))
    return dvar.value, [dls[d] for d in range(spec.D)]


def kmn_knm_vjp(spec, X, Z, Gq, Y=None, Gb=None, need_dZ=False):
    """VJP of (theta, Z) -> (Q, B) = (K_mn K_nm, K_mn Y), K = k(X, Z), at the cotangents Gq [M, M] (need not be
    symmetric) and Gb [M, P]: (dvariance: float, [dl_d for d < D], dZ [M, D] or None).  Nothing N x M beyond one row
    panel is formed (`mgp_kmn_knm_vjp`).  fp64 and D <= 32 only: libmgp refuses anything else (MgpError).

    `Gq=None` means Gq = 0: the cotangent of K is then W = Y Gb^T alone, of rank P, nothing [M, M] is touched and Y and
    Gb are required (ValueError without them).  X and Z may be the same tensor; with Y = [U | V] and Gb = [V | U] on
    (Z, Z) the cotangent is U V^T + V U^T, so dZ is the whole gradient of sum_r u_r^T k(Z, Z) v_r in Z and dvariance,
    dl are twice `kxx_grad(spec, Z, U, V)`."""
    return _kmn_knm_vjp(spec, X, Z, Gq, Y, Gb, need_dZ, None)


def kmn_knm_vjp_anyd(spec, X, Z, Gq, Y=None, Gb=None, need_dZ=False, panel_rows=0):
    """`kmn_knm_vjp` at any D <= 512 (`mgp_kmn_knm_vjp_anyd`, include/mgp_anyd.h): the same arguments and the same
    return.  At D <= 32 it runs `kmn_knm_vjp`'s implementation (the same bits with `panel_rows=0`); above, the kernel
    panel and the pair kernels stage the dimensions through LDS slice by slice.  `panel_rows`: rows of X per panel,
    0 = at most 256 MiB of K per panel."""
    panel_rows = int(panel_rows)
    if panel_rows < 0:
        raise ValueError("panel_rows must be >= 0")
    return _kmn_knm_vjp(spec, X, Z, Gq, Y, Gb, need_dZ, panel_rows)


def _kmn_knm_vjp(spec, X, Z, Gq, Y, Gb, need_dZ, panel_rows):
    """the two wrappers above: `panel_rows=None` calls `mgp_kmn_knm_vjp`, a number `mgp_kmn_knm_vjp_anyd`"""
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    N, M = X.shape[0], Z.shape[0]
    if M < 1:
        raise ValueError("kmn_knm_vjp needs M >= 1")
    if Gq is None:
        if Y is None or Gb is None:
            raise ValueError("Gq=None (a rank-P cotangent Y Gb^T) needs Y and Gb")
    else:
        Gq = _hip.check_tensor(Gq, "Gq", dtype=X.dtype, shape=(M, M))
    if (Y is None) != (Gb is None):
        raise ValueError("Y and Gb go together")
    P = 0
    if Y is not None:
        Y = _hip.check_tensor(Y, "Y", dtype=X.dtype)
        if Y.dim() != 2 or Y.shape[0] != N:
            raise ValueError(f"Y must be [N={N}, P], got {tuple(Y.shape)}")
        P = Y.shape[1]
        Gb = _hip.check_tensor(Gb, "Gb", dtype=X.dtype, shape=(M, P))
    if Gq is None and P < 1:
        raise ValueError("Gq=None needs P >= 1 columns in Y and Gb")
    dZ = torch.empty((M, spec.D), dtype=X.dtype, device=X.device) if need_dZ else None
    dvar = ctypes.c_double(0.0)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)()
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    if panel_rows is None:
        hd.check(hd.lib.mgp_kmn_knm_vjp(hd.h, ctypes.byref(k), _hip.ptr(X), N, _hip.ptr(Z), M, _hip.ptr(Gq),
                                        _hip.ptr(Y if P else None), _hip.ptr(Gb if P else None), P, ctypes.byref(dvar),
                                        dls, _hip.ptr(dZ)))
    else:
        hd.check(hd.lib.mgp_kmn_knm_vjp_anyd(hd.h, ctypes.byref(k), _hip.ptr(X), N, _hip.ptr(Z), M, _hip.ptr(Gq),
                                             _hip.ptr(Y if P else None), _hip.ptr(Gb if P else None), P, panel_rows,
                                             ctypes.byref(dvar), dls, _hip.ptr(dZ)))
    return dvar.value, [dls[d] for d in range(spec.D)], dZ


def kxx_pivchol(spec, X, max_rank, rel_tol=0.0):
    """Rank-`max_rank` partial pivoted Cholesky of K = k(X, X) (no noise), matrix-free (`mgp_kxx_pivchol`): greedy
    pivots on the residual diagonal, stopping early once its sum is <= rel_tol * N * variance.  fp64 only.

    Returns (L [rank, N] with K ~= L^T L, piv [rank] int64, diag [N] = the residual diagonal)."""
    X = _points(X, "X", spec.D)
    N = X.shape[0]
    max_rank = int(max_rank)
    if not 1 <= max_rank <= 1024:
        raise ValueError(f"max_rank must be in [1, 1024], got {max_rank}")
    rows = min(max_rank, N)
    L = torch.empty((rows, N), dtype=X.dtype, device=X.device)
    piv = torch.empty((rows,), dtype=torch.int64, device=X.device)
    diag = torch.empty((N,), dtype=X.dtype, device=X.device)
    rank = ctypes.c_int32(0)
    if N > 0:
        hd = _hip.get_handle(X.device)
        k = spec.struct(_hip.dtype_code(X))
        hd.check(hd.lib.mgp_kxx_pivchol(hd.h, ctypes.byref(k), _hip.ptr(X), N, max_rank, float(rel_tol), _hip.ptr(L),
                                        _hip.ptr(piv), _hip.ptr(diag), ctypes.byref(rank)))
    return L[:rank.value], piv[:rank.value], diag


def lowrank_apply(diag_inv, B, R):
    """Z [Bt, n] = diag_inv * R - (R @ B^T) @ B for R [Bt, n], B [k, n], diag_inv [n] (`mgp_lowrank_apply`): one
    application of the diagonal-plus-low-rank preconditioner `MGP_PRE_LOWRANK`."""
    R = _hip.check_tensor(R, "R")
    if R.dim() != 2:
        raise ValueError(f"R must be [Bt, n], got {tuple(R.shape)}")
    Bt, n = R.shape
    B = _hip.check_tensor(B, "B", dtype=R.dtype)
    if B.dim() != 2 or B.shape[1] != n or B.shape[0] < 1:
        raise ValueError(f"B must be [k >= 1, n={n}], got {tuple(B.shape)}")
    diag_inv = _hip.check_tensor(diag_inv, "diag_inv", dtype=R.dtype, shape=(n,))
    Z = torch.empty_like(R)
    if Bt and n:
        hd = _hip.get_handle(R.device)
        hd.check(hd.lib.mgp_lowrank_apply(hd.h, _hip.dtype_code(R), _hip.ptr(diag_inv), _hip.ptr(B), B.shape[0], n,
                                          _hip.ptr(R), Bt, _hip.ptr(Z)))
    return Z


def knm_project(spec, Xs, X, R, want_proj=False, r_layout=COLS):
    """(sqnorm [B], proj [B, r] or None): proj = k(Xs, X) @ R for a wide dense R ([N, r] COLS or [r, N] ROWS) and
    sqnorm[b] = sum_j proj[b, j]^2, k(Xs, X) never formed on the fused route (`mgp_knm_project`: fp64, D <= 32,
    r <= 256) -- the query of a Lanczos variance cache."""
    Xs = _points(Xs, "Xs", spec.D)
    X = _points(X, "X", spec.D, Xs.dtype)
    R = _hip.check_tensor(R, "R", dtype=Xs.dtype)
    if r_layout not in (COLS, ROWS):
        raise ValueError(f"bad r_layout {r_layout}")
    B, N = Xs.shape[0], X.shape[0]
    if R.dim() != 2 or (R.shape[0] if r_layout == COLS else R.shape[1]) != N:
        raise ValueError(f"R must be [N={N}, r] (COLS) or [r, N] (ROWS), got {tuple(R.shape)}")
    r = R.shape[1] if r_layout == COLS else R.shape[0]
    sqnorm = torch.empty((B,), dtype=Xs.dtype, device=Xs.device)
    proj = torch.empty((B, r), dtype=Xs.dtype, device=Xs.device) if want_proj else None
    if B > 0:
        # N == 0 or r == 0 goes through the C-ABI too: libmgp writes the zeros
        hd = _hip.get_handle(Xs.device)
        k = spec.struct(_hip.dtype_code(Xs))
        hd.check(hd.lib.mgp_knm_project(hd.h, ctypes.byref(k), _hip.ptr(Xs), B, _hip.ptr(X), N, _hip.ptr(R), r,
                                        r_layout, _hip.ptr(proj), _hip.ptr(sqnorm)))
    return sqnorm, proj


def knm_quadform(spec, Xs, Z, C):
    """q [B] = k(xs_b, Z) C k(Z, xs_b) for a symmetric C [M, M] given by its upper triangle (`mgp_knm_quadform`,
    include/mgp_predict.h): the entries below the diagonal are never read.  k(Xs, Z) is never formed on the fused route
    (fp64, D <= 32).  C may be a row-major view with a row stride >= M (columns contiguous)."""
    Xs = _points(Xs, "Xs", spec.D)
    Z = _points(Z, "Z", spec.D, Xs.dtype)
    B, M = Xs.shape[0], Z.shape[0]
    if not torch.is_tensor(C) or C.dim() != 2 or tuple(C.shape) != (M, M):
        raise ValueError(f"C must be [M={M}, M], got {tuple(C.shape) if torch.is_tensor(C) else type(C)}")
    if C.dtype != Xs.dtype or C.device != Xs.device:
        raise ValueError(f"C must be {Xs.dtype} on {Xs.device}, got {C.dtype} on {C.device}")
    if M > 1 and C.stride(1) != 1:
        raise ValueError("C must have contiguous columns")
    ldc = C.stride(0) if M > 1 else max(M, 1)
    if M > 1 and ldc < M:
        raise ValueError(f"row stride {ldc} of C is less than M={M}")
    q = torch.empty((B,), dtype=Xs.dtype, device=Xs.device)
    if B > 0:
        # M == 0 goes through the C-ABI too: libmgp writes the zeros
        hd = _hip.get_handle(Xs.device)
        k = spec.struct(_hip.dtype_code(Xs))
        hd.check(hd.lib.mgp_knm_quadform(hd.h, ctypes.byref(k), _hip.ptr(Xs), B, _hip.ptr(Z), M, _hip.ptr(C), ldc,
                                         _hip.ptr(q)))
    return q


def pcg_solve_record(op, rhs, error_threshold, max_iterations=None, min_float=1e-16, check_every=10,
                     preconditioner=None):
    """CG from zero on `op` (a `conjugate_gradient.LinearOperator`) for the rows of rhs [Bt, n], no residual refresh,
    recording every step taken (`mgp_pcg_solve_record`).  `preconditioner`: None (the identity) or a
    `CGPreconditioner` whose native form libmgp records with (`EyePreconditioner`, `PivotedCholeskyPreconditioner`).

    Returns (solution [Bt, n], err [Bt, 1] = 0.5 rz, stats, coef [steps, Bt, 3] = (gamma, beta, 0.5 rz after the step))."""
    rhs = _hip.check_tensor(rhs, "rhs", dtype=op.dtype)
    if rhs.dim() != 2 or rhs.shape[1] != op.shape[0]:
        raise ValueError(f"rhs must be [Bt, n={op.shape[0]}], got {tuple(rhs.shape)}")
    Bt, n = rhs.shape
    max_iterations = n if max_iterations is None else int(max_iterations)
    sol = torch.empty_like(rhs)
    err = torch.empty((Bt, 1), dtype=op.dtype, device=op.device)
    coef = torch.zeros((max(max_iterations, 0), Bt, 3), dtype=op.dtype, device=op.device)
    stats = _hip.MgpCgStats()
    if Bt > 0:
        hd = _hip.get_handle(op.device)
        st, keep = op._struct_for(Bt)
        if preconditioner is None:
            pre, pkeep = _hip.MgpPrecond(), ()
            pre.kind = _hip.PRE_EYE
        else:
            nat = preconditioner._native(op)
            if nat is None:
                raise TypeError("the recording solve takes the identity or a preconditioner libmgp applies itself")
            pre, pkeep = nat
        hd.check(hd.lib.mgp_pcg_solve_record(
            hd.h, ctypes.byref(st), ctypes.byref(pre), _hip.ptr(rhs), None, Bt, float(error_threshold), max_iterations,
            max_iterations + 1, float(min_float), int(check_every), _hip.ptr(sol), _hip.ptr(err), ctypes.byref(stats),
            _hip.ptr(coef), coef.shape[0]))
        del keep, pkeep
    return sol, err, stats, coef[:stats.iterations]


def kmn_matvec(spec, X, Z, W, w_layout=COLS, out_layout=None):
    """out = k(Z, X) @ W = K_nm^T W.  W [N,R] (COLS) or [R,N] (ROWS); out [M,R] or [R,M]."""
    return _kmn_matvec("mgp_kmn_matvec", spec, X, Z, W, w_layout, out_layout)


def kmn_matvec_anyd(spec, X, Z, W, w_layout=COLS, out_layout=None):
    """`kmn_matvec` by `mgp_kmn_matvec_anyd`: fp64 at D > 32 the fused any-D sweep, the rows of X cut into chunks whose
    partials are added in chunk order (bit-reproducible); fp32 or D <= 32 exactly `kmn_matvec`."""
    return _kmn_matvec("mgp_kmn_matvec_anyd", spec, X, Z, W, w_layout, out_layout)


def _kmn_matvec(entry, spec, X, Z, W, w_layout, out_layout):
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    W = _hip.check_tensor(W, "W", dtype=X.dtype)
    if W.dim() != 2:
        raise ValueError("W must be 2-D")
    N, M = X.shape[0], Z.shape[0]
    R = W.shape[1] if w_layout == COLS else W.shape[0]
    if (W.shape[0] if w_layout == COLS else W.shape[1]) != N:
        raise ValueError(f"W shape {tuple(W.shape)} does not match N={N}")
    out_layout = w_layout if out_layout is None else out_layout
    out = torch.empty((M, R) if out_layout == COLS else (R, M), dtype=X.dtype, device=X.device)
    if M == 0 or R == 0:
        return out
    # N == 0 (a rank without rows) goes through the C-ABI too: libmgp writes the zeros
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    hd.check(getattr(hd.lib, entry)(hd.h, ctypes.byref(k), _hip.ptr(X), N, _hip.ptr(Z), M, _hip.ptr(W), R,
                                     w_layout, _hip.ptr(out), out_layout))
    return out


def k_dense(spec, A, B, jitter=0.0, diag_add=None):
    """out [na, nb] = k(A, B) (+ jitter I) (+ diag(diag_add)); the diagonal terms need na == nb."""
    A = _points(A, "A", spec.D)
    B = _points(B, "B", spec.D, A.dtype)
    na, nb = A.shape[0], B.shape[0]
    if (jitter != 0.0 or diag_add is not None) and na != nb:
        raise ValueError("diagonal terms need a square block")
    if diag_add is not None:
        diag_add = _hip.check_tensor(diag_add, "diag_add", dtype=A.dtype).reshape(-1)
        if diag_add.shape[0] != na:
            raise ValueError("diag_add length mismatch")
    out = torch.empty((na, nb), dtype=A.dtype, device=A.device)
    if na == 0 or nb == 0:
        return out
    hd = _hip.get_handle(A.device)
    k = spec.struct(_hip.dtype_code(A))
    hd.check(hd.lib.mgp_k_dense(hd.h, ctypes.byref(k), _hip.ptr(A), na, _hip.ptr(B), nb, _hip.ptr(out), nb,
                                float(jitter), _hip.ptr(diag_add)))
    return out


def k_dense_vjp(spec, A, B, G):
    """(dL/dvariance: float, dL/dlengthscales: list[D]) for K = k(A,B) given G = dL/dK (row F2)."""
    A = _points(A, "A", spec.D)
    B = _points(B, "B", spec.D, A.dtype)
    G = _hip.check_tensor(G, "G", dtype=A.dtype, shape=(A.shape[0], B.shape[0]))
    dvar = ctypes.c_double(0.0)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)()
    if A.shape[0] and B.shape[0]:
        hd = _hip.get_handle(A.device)
        k = spec.struct(_hip.dtype_code(A))
        hd.check(hd.lib.mgp_k_dense_vjp(hd.h, ctypes.byref(k), _hip.ptr(A), A.shape[0], _hip.ptr(B), B.shape[0],
                                        _hip.ptr(G), B.shape[0], ctypes.byref(dvar), dls))
    return dvar.value, [dls[d] for d in range(spec.D)]


def k_dense_vjp_points(spec, A, B, G, need_dA=True, need_dB=True, panel_rows=0):
    """(dL/dvariance: float, [dL/dl_d for d < D], dA [na, D] or None, dB [nb, D] or None) for K = k(A, B) given the dense
    cotangent G = dL/dK [na, nb] (`mgp_k_dense_vjp_points`, include/mgp_points.h): the scalars of `k_dense_vjp` and the
    point gradients of `training.k_grad_points` from fused pair kernels, no [., ., D] temporary.  fp64 and D <= 512;
    G may be a row-major view with a row stride >= nb (anything else is copied); A and B may be the same tensor, and
    dA + dB is then `training.kmm_grad_z(Z, G)`.  `panel_rows`: rows of A per panel, 0 = the library's rule."""
    panel_rows = int(panel_rows)
    if panel_rows < 0:
        raise ValueError("panel_rows must be >= 0")
    A = _points(A, "A", spec.D)
    B = _points(B, "B", spec.D, A.dtype)
    na, nb = A.shape[0], B.shape[0]
    if not isinstance(G, torch.Tensor) or G.dim() != 2 or tuple(G.shape) != (na, nb):
        raise ValueError(f"G must be [na={na}, nb={nb}], got {tuple(G.shape) if isinstance(G, torch.Tensor) else G}")
    if G.dtype != A.dtype:
        raise TypeError(f"G has dtype {G.dtype}, expected {A.dtype}")
    if na and nb and not (G.stride(1) == 1 and G.stride(0) >= nb):
        G = G.contiguous()
    if not G.is_cuda:
        raise RuntimeError(f"G must live on the GPU (got {G.device}); the hot path has no CPU fallback")
    # one row: torch calls any row stride contiguous, and the library never steps by it
    ldg = G.stride(0) if na > 1 and nb else nb
    dA = torch.empty((na, spec.D), dtype=A.dtype, device=A.device) if need_dA else None
    dB = torch.empty((nb, spec.D), dtype=A.dtype, device=A.device) if need_dB else None
    dvar = ctypes.c_double(0.0)
    dls = (ctypes.c_double * _hip.MGP_MAX_D)()
    hd = _hip.get_handle(A.device)
    k = spec.struct(_hip.dtype_code(A))
    hd.check(hd.lib.mgp_k_dense_vjp_points(hd.h, ctypes.byref(k), _hip.ptr(A), na, _hip.ptr(B), nb, _hip.ptr(G), ldg,
                                           panel_rows, ctypes.byref(dvar), dls, _hip.ptr(dA), _hip.ptr(dB)))
    return dvar.value, [dls[d] for d in range(spec.D)], dA, dB


def kmm_lambda_matvec(spec, Z, lam, V):
    """out [R,M] = V [R,M] @ (k(Z,Z) + diag(lam)), matrix-free (row M2)."""
    Z = _points(Z, "Z", spec.D)
    M = Z.shape[0]
    lam = _hip.check_tensor(lam, "lam", dtype=Z.dtype, shape=(M,))
    V = _hip.check_tensor(V, "V", dtype=Z.dtype)
    if V.dim() != 2 or V.shape[1] != M:
        raise ValueError(f"V must be [R, M={M}], got {tuple(V.shape)}")
    out = torch.empty_like(V)
    if V.shape[0] == 0 or M == 0:
        return out
    hd = _hip.get_handle(Z.device)
    k = spec.struct(_hip.dtype_code(Z))
    hd.check(hd.lib.mgp_kmm_lambda_matvec(hd.h, ctypes.byref(k), _hip.ptr(Z), M, _hip.ptr(lam), _hip.ptr(V),
                                          V.shape[0], _hip.ptr(out)))
    return out


def kmn_knm(spec, X, Z):
    """out [M,M] = k(Z,X) k(X,Z) on the matrix cores (row S1)."""
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    M = Z.shape[0]
    out = torch.empty((M, M), dtype=X.dtype, device=X.device)
    if M == 0:
        return out
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    hd.check(hd.lib.mgp_kmn_knm(hd.h, ctypes.byref(k), _hip.ptr(X), X.shape[0], _hip.ptr(Z), M, _hip.ptr(out)))
    return out


def kmn_sq_colsum(spec, X, Z):
    """out [M] = sum_i k(x_i, z_m)^2 = diag(K_mn K_nm)."""
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    M = Z.shape[0]
    out = torch.empty((M,), dtype=X.dtype, device=X.device)
    if M == 0:
        return out
    hd = _hip.get_handle(X.device)
    k = spec.struct(_hip.dtype_code(X))
    hd.check(hd.lib.mgp_kmn_sq_colsum(hd.h, ctypes.byref(k), _hip.ptr(X), X.shape[0], _hip.ptr(Z), M, _hip.ptr(out)))
    return out


def symm_matmul(A, P):
    """out [Bt,n] = P [Bt,n] @ A [n,n] for symmetric A (row M2)."""
    A = _hip.check_tensor(A, "A")
    P = _hip.check_tensor(P, "P", dtype=A.dtype)
    if A.dim() != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("A must be square")
    if P.dim() != 2 or P.shape[1] != A.shape[0]:
        raise ValueError(f"P shape {tuple(P.shape)} does not match n={A.shape[0]}")
    out = torch.empty_like(P)
    if P.numel() == 0:
        return out
    hd = _hip.get_handle(A.device)
    hd.check(hd.lib.mgp_symm_matmul(hd.h, _hip.dtype_code(A), _hip.ptr(A), A.shape[0], _hip.ptr(P), P.shape[0],
                                    _hip.ptr(out)))
    return out


def colwise_dot(A, B):
    """out [cols] = sum over rows of A*B (tf.reduce_sum(A * B, axis=0), models.py:343)."""
    A = _hip.check_tensor(A, "A")
    B = _hip.check_tensor(B, "B", dtype=A.dtype, shape=tuple(A.shape))
    if A.dim() != 2:
        raise ValueError("A must be 2-D")
    out = torch.empty((A.shape[1],), dtype=A.dtype, device=A.device)
    if A.shape[1] == 0:
        return out
    hd = _hip.get_handle(A.device)
    hd.check(hd.lib.mgp_colwise_dot(hd.h, _hip.dtype_code(A), _hip.ptr(A), _hip.ptr(B), A.shape[0], A.shape[1],
                                    _hip.ptr(out)))
    return out


def dot_all(A, B):
    """float(sum(A*B)) accumulated in fp64 (Hutchinson trace, models.py:313)."""
    A = _hip.check_tensor(A, "A")
    B = _hip.check_tensor(B, "B", dtype=A.dtype)
    if A.numel() != B.numel():
        raise ValueError("size mismatch")
    hd = _hip.get_handle(A.device)
    out = ctypes.c_double(0.0)
    hd.check(hd.lib.mgp_dot_all(hd.h, _hip.dtype_code(A), _hip.ptr(A), _hip.ptr(B), A.numel(), ctypes.byref(out)))
    return out.value


DIST_TYPES = {"sqeuclidean": 0, "euclidean": 1, "covariance": 2, "correlation": 3}


def nearest_center(spec, X, Z, distance_type="sqeuclidean", return_distance=True):
    """idx [N] int64 = argmin_m d(Z_m, X_i); optional best distance [N] (row F1)."""
    X = _points(X, "X", spec.D)
    Z = _points(Z, "Z", spec.D, X.dtype)
    if Z.shape[0] == 0:
        raise ValueError("need at least one centre")
    N = X.shape[0]
    idx = torch.empty((N,), dtype=torch.int64, device=X.device)
    best = torch.empty((N,), dtype=X.dtype, device=X.device) if return_distance else None
    if N > 0:
        hd = _hip.get_handle(X.device)
        k = spec.struct(_hip.dtype_code(X))
        hd.check(hd.lib.mgp_nearest_center(hd.h, ctypes.byref(k), DIST_TYPES[distance_type], _hip.ptr(X), N,
                                           _hip.ptr(Z), Z.shape[0], _hip.ptr(idx), _hip.ptr(best)))
    return (idx, best) if return_distance else idx


def cluster_stats(idx, y, M, method="auto"):
    """(sums, counts [M]) of y per cluster, deterministic order.  y [N] -> sums [M]; y [N,C] ->
    sums [M,C].

    "sweep": the fused N x M transpose sweep (`mgp_cluster_stats`, one column per launch).
    "sorted": group the rows by cluster with one stable device sort, then `mgp_segment_sums` --
    N C work instead of N M C.  "auto" takes the sort once N M exceeds 2^29 pairs (C3: 0.40 ms vs
    0.93 ms; C2, 2e8 pairs: 0.21 vs 0.09 ms) or several columns are asked for (C3, 8 columns: 0.55 ms
    vs 7.4 ms)."""
    idx = _hip.check_tensor(idx, "idx", dtype=torch.int64).reshape(-1)
    y = _hip.check_tensor(y, "y")
    multi = y.dim() == 2 and y.shape[1] > 1
    Y = y if multi else y.reshape(-1, 1)
    N, C = Y.shape
    if idx.shape[0] != N:
        raise ValueError("idx / y length mismatch")
    if method == "auto":
        method = "sorted" if (C > 1 or N * M > (1 << 29)) else "sweep"
    hd = _hip.get_handle(y.device)
    if method == "sweep":
        cols, counts = [], None
        for c in range(C):
            sums = torch.empty((M,), dtype=y.dtype, device=y.device)
            counts = torch.empty((M,), dtype=y.dtype, device=y.device)
            col = Y[:, c].contiguous()
            hd.check(hd.lib.mgp_cluster_stats(hd.h, _hip.dtype_code(y), _hip.ptr(idx), _hip.ptr(col), N, M,
                                              _hip.ptr(sums), _hip.ptr(counts)))
            cols.append(sums)
        sums = torch.stack(cols, dim=1)
    elif method == "sorted":
        if N and (int(idx.min()) < 0 or int(idx.max()) >= M):
            raise ValueError("cluster index out of range")
        order = torch.argsort(idx, stable=True)
        cnt = torch.bincount(idx, minlength=M)
        offsets = torch.zeros((M + 1,), dtype=torch.int64, device=idx.device)
        torch.cumsum(cnt, dim=0, out=offsets[1:])
        sums = torch.empty((M, C), dtype=y.dtype, device=y.device)
        Yc = Y.contiguous()
        hd.check(hd.lib.mgp_segment_sums(hd.h, _hip.dtype_code(y), _hip.ptr(order), _hip.ptr(offsets), _hip.ptr(Yc),
                                         N, C, M, _hip.ptr(sums)))
        counts = cnt.to(y.dtype)
    else:
        raise ValueError(f"unknown method {method!r}")
    return (sums if multi else sums[:, 0].contiguous()), counts


def rff_features(X, theta):
    """Phi [N, 2L] = [cos(X theta^T) | sin(X theta^T)] (`basis_vectors`, reference `cggp/rff.py:48-57`); theta [L, D]
    in radians."""
    X = _points(X, "X")
    theta = _points(theta, "theta", X.shape[1], X.dtype)
    N, D = X.shape
    L = theta.shape[0]
    out = torch.empty((N, 2 * L), dtype=X.dtype, device=X.device)
    if N == 0 or L == 0:
        return out
    hd = _hip.get_handle(X.device)
    hd.check(hd.lib.mgp_rff_features(hd.h, _hip.dtype_code(X), _hip.ptr(X), N, D, _hip.ptr(theta), L, _hip.ptr(out),
                                     2 * L))
    return out


def rff_sample(X, theta, W, scale, out_layout=ROWS, anyd=False):
    """scale * W [S, 2L] @ Phi(X)^T without forming Phi where D <= 32 and S <= 8 (`rff_sample`, reference
    `cggp/rff.py:60-73`).  out [S, N] (ROWS) or [N, S] (COLS).  `anyd=True` ORs `MGP_RFF_ANYD` into the layout word:
    fp64, D > 32 and S <= 8 then take the fused any-D kernels of csrc/rff_anyd.hip instead of feature panels;
    anything else is the plain call."""
    X = _points(X, "X")
    theta = _points(theta, "theta", X.shape[1], X.dtype)
    N, D = X.shape
    L = theta.shape[0]
    W = _hip.check_tensor(W, "W", dtype=X.dtype)
    if W.dim() != 2 or W.shape[1] != 2 * L:
        raise ValueError(f"W must be [S, 2L={2 * L}], got {tuple(W.shape)}")
    S = W.shape[0]
    if out_layout not in (COLS, ROWS):
        raise ValueError(f"bad out_layout {out_layout}")
    out = torch.empty((S, N) if out_layout == ROWS else (N, S), dtype=X.dtype, device=X.device)
    if N == 0 or S == 0:
        return out
    # L == 0 goes through the C-ABI too: libmgp writes the zeros
    hd = _hip.get_handle(X.device)
    hd.check(hd.lib.mgp_rff_sample(hd.h, _hip.dtype_code(X), _hip.ptr(X), N, D, _hip.ptr(theta), L, _hip.ptr(W), S,
                                   float(scale), _hip.ptr(out), out_layout | (_hip.RFF_ANYD if anyd else 0)))
    return out


def rff_sample_vjp(X, theta, W, scale, G, g_layout=ROWS, want_dtheta=True, want_dX=False, anyd=False):
    """Backward pass of `rff_sample` at the cotangent G [S, N] (ROWS) or [N, S] (COLS): (dtheta [L, D] or None,
    dX [N, D] or None) by `mgp_rff_sample_vjp` (include/mgp_pathwise.h), phases as in the forward pass.  fp64,
    D <= 32 and 1 <= S <= 8 only: libmgp refuses anything else (MgpError).  `anyd=True` ORs `MGP_RFF_ANYD` into the
    layout word, which opens 32 < D <= 512 (csrc/rff_anyd.hip) and changes nothing else.  The derivative in `scale` is
    sum(G o out) / scale and needs no call."""
    X = _points(X, "X")
    theta = _points(theta, "theta", X.shape[1], X.dtype)
    N, D = X.shape
    L = theta.shape[0]
    W = _hip.check_tensor(W, "W", dtype=X.dtype)
    if W.dim() != 2 or W.shape[1] != 2 * L:
        raise ValueError(f"W must be [S, 2L={2 * L}], got {tuple(W.shape)}")
    S = W.shape[0]
    if g_layout not in (COLS, ROWS):
        raise ValueError(f"bad g_layout {g_layout}")
    G = _hip.check_tensor(G, "G", dtype=X.dtype, shape=(S, N) if g_layout == ROWS else (N, S))
    if not (want_dtheta or want_dX):
        raise ValueError("rff_sample_vjp: nothing asked for (want_dtheta and want_dX are both False)")
    dtheta = torch.empty((L, D), dtype=X.dtype, device=X.device) if want_dtheta else None
    dX = torch.empty((N, D), dtype=X.dtype, device=X.device) if want_dX else None
    if (N == 0 or not want_dX) and (L == 0 or not want_dtheta):
        return dtheta, dX  # no element to write; N == 0 or L == 0 with one goes through the C-ABI: libmgp writes the zeros
    hd =_hip.get_handle(X.device)
    hd.check(hd.lib.mgp_rff_sample_vjp(hd.h, _hip.dtype_code(X), _hip.ptr(X), N, D, _hip.ptr(theta), L, _hip.ptr(W), S,
                                       float(scale), _hip.ptr(G), g_layout | (_hip.RFF_ANYD if anyd else 0),
                                       _hip.ptr(dtheta), _hip.ptr(dX)))
    return dtheta, dX
