"""Training step through CG (next row F2) -- host mirror of the reference's trainable path.

What the reference does under `tf.GradientTape` (`cggp/optimize.py:198-254`,
`train_using_adam_and_update`): minimise `-elbo(batch)` (`cggp/models.py:125-134`) of a CGGP model
with Adam over the kernel variance / lengthscales and the likelihood variance (Z and pseudo_u are
frozen, `models.py:219-220`), where every `(Kmm+Lambda)^-1` is the CG with its custom gradient
(`conjugate_gradient.py:100-118`) and `log|Kmm+Lambda|` enters only through `eval_logdet`'s
backward (`models.py:30-44`).

Here: the hyper-parameters are positive `Parameter`s (softplus, as gpflow.utilities.positive());
kernel blocks are an autograd node whose forward is `mgp_k_dense` and whose backward is the fused
`mgp_k_dense_vjp` reduction; the CG solves are `_CGFunction` (device loop forward and backward);
`eval_logdet` is the node of `cggp.models`; the remaining small dense algebra (`Kmm @ a`,
elementwise likelihood terms) is torch on the device so the tape is end to end.
"""

import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip, ops
from .conjugate_gradient import (ConjugateGradient, anyd_matvec, check_fused_anyd, check_fused_point_grads,
                                 check_sym_anyd, use_fused_point_grads)
from .kernels import Stationary
from .models import check_data_term, check_pathwise, draw_pathwise, eval_logdet, rademacher


class Parameter:
    """Positive parameter: value = softplus(raw) + lower (gpflow.utilities.positive())."""

    def __init__(self, value, lower=0.0):
        v = np.atleast_1d(np.asarray(value, dtype=np.float64)) - lower
        if np.any(v <= 0):
            raise ValueError("initial value must exceed the lower bound")
        raw = np.where(v > 30.0, v, np.log(np.expm1(np.minimum(v, 30.0))))
        self.raw = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
        self.lower = float(lower)
        self.scalar = np.ndim(value) == 0

    def __call__(self):
        t = F.softplus(self.raw) + self.lower
        return t[0] if self.scalar else t

    @property
    def value(self):
        t = self().detach()
        return float(t) if self.scalar else t.tolist()


class _KBlock(torch.autograd.Function):
    """K = k(A, B) (+ jitter I): forward `mgp_k_dense`, backward `mgp_k_dense_vjp`; where A or B needs a gradient
    (trainable inducing inputs) it comes from `k_grad_points`.  K(Z) passes Z twice and autograd adds the two.
    With `fused_point_grads` (the rule of `use_fused_point_grads`) a backward pass that needs a point gradient is ONE
    `mgp_k_dense_vjp_points` call for the hyper-parameters and the sides that need one."""

    @staticmethod
    def forward(ctx, variance, lengthscales, A, B, kind, jitter, fused_point_grads=False):
        D = A.shape[1]
        spec = ops.KernelSpec(kind, float(variance), [float(x) for x in lengthscales.reshape(-1)], D)
        ctx.spec, ctx.v_shape, ctx.l_shape = spec, variance.shape, lengthscales.shape
        ctx.fused_point_grads = fused_point_grads
        ctx.save_for_backward(A, B)
        return ops.k_dense(spec, A, B, jitter=jitter)

    @staticmethod
    def backward(ctx, G):
        A, B = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dA = dB = None
        if (need_a or need_b) and use_fused_point_grads(ctx.fused_point_grads, A, B):
            dvar, dls, dA, dB = ops.k_dense_vjp_points(ctx.spec, A.detach(), B.detach(), G, need_dA=need_a,
                                                       need_dB=need_b)
        else:
            dvar, dls = ops.k_dense_vjp(ctx.spec, A, B, G.contiguous())
            if need_a or need_b:
                dA, dB = k_grad_points(ctx.spec.kind, ctx.spec.variance, ctx.spec.lengthscales, A, B, G)
        gv = torch.tensor(dvar, dtype=torch.float64).reshape(ctx.v_shape)
        n_l = int(np.prod(ctx.l_shape)) if len(ctx.l_shape) else 1
        gl = torch.tensor(dls if n_l > 1 else [sum(dls)], dtype=torch.float64).reshape(ctx.l_shape)
        grads = (gv, gl, dA if need_a else None, dB if need_b else None, None, None, None)
        return grads[:len(ctx.needs_input_grad)]  # `fused_point_grads` is optional in apply()


class TrainableKernel:
    """A stationary kernel whose variance / lengthscales are `Parameter`s."""

    def __init__(self, kernel: Stationary):
        self.name = kernel.name
        self.variance_p = Parameter(kernel.variance)
        ls = kernel.lengthscales
        self.lengthscales_p = Parameter(ls if len(ls) > 1 else ls[0])

    def parameters(self):
        return [self.variance_p.raw, self.lengthscales_p.raw]

    def K(self, X, X2=None, jitter=0.0, fused_point_grads=False):
        """k(X, X2) (+ jitter I) as an autograd node.  `fused_point_grads` (False, True or "auto"): where X or X2 needs a
        gradient, the backward pass is one `ops.k_dense_vjp_points` call instead of `ops.k_dense_vjp` +
        `k_grad_points` -- always (True) or by the measured rule (`conjugate_gradient.fused_point_grads_auto`).  fp32
        tensors and host tensors take the torch route whatever the setting."""
        X2 = X if X2 is None else X2
        ls = self.lengthscales_p()
        if ls.dim() == 0:
            ls = ls.reshape(1)
        if check_fused_point_grads(fused_point_grads) is False:
            return _KBlock.apply(self.variance_p(), ls, X, X2, self.name, float(jitter))
        return _KBlock.apply(self.variance_p(), ls, X, X2, self.name, float(jitter), fused_point_grads)

    def frozen(self):
        """Plain kernel with the current values (non-differentiable fast paths: predict, metrics)."""
        from . import kernels
        cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
               "matern52": kernels.Matern52}[self.name]
        ls = self.lengthscales_p.value
        return cls(variance=self.variance_p.value, lengthscales=ls if isinstance(ls, list) else [ls])


class _LogdetFromSolution(torch.autograd.Function):
    """`eval_logdet` (`cggp/models.py:21-48`) when K^-1 Zp is already at hand: value 0.0, gradient
    (K^-1 Zp)(df Zp)^T / P (`:40-42`) -- the estimator the reference recomputes with a second CG."""

    @staticmethod
    def forward(ctx, matrix, solution, probes):
        ctx.save_for_backward(solution, probes)
        return torch.zeros((), dtype=matrix.dtype, device=matrix.device)

    @staticmethod
    def backward(ctx, df):
        lv, probes = ctx.saved_tensors
        return (lv @ (df * probes).t()) / probes.shape[1], None, None


def _frozen_kernel(kind, variance, lengthscales):
    from . import kernels
    cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
           "matern52": kernels.Matern52}[kind]
    return cls(variance=float(variance), lengthscales=[float(v) for v in lengthscales.reshape(-1)])


def _theta_grads(dvar, dls, v_shape, l_shape):
    """(dvariance, dlengthscales) of a libmgp bilinear form as CPU tensors of the parameters' shapes (one shared
    lengthscale collects the sum, as `_KBlock`)."""
    n_l = int(np.prod(l_shape)) if len(l_shape) else 1
    gl = torch.tensor(dls if n_l > 1 else [sum(dls)], dtype=torch.float64).reshape(l_shape)
    return torch.tensor(dvar, dtype=torch.float64).reshape(v_shape), gl


def _kzz_bilinear_grads(spec, Z, U, V, need_z):
    """(dvariance, [dl_d], dZ or None) of sum_r u_r^T k(Z, Z) v_r for U, V [M, R], nothing [M, M] formed.  Without dZ:
    `mgp_kxx_grad`, as ever.  With it: ONE `mgp_kmn_knm_vjp` call on (Z, Z) with Gq = NULL, Y = [U | V], Gb = [V | U],
    whose cotangent U V^T + V U^T makes its dZ the whole derivative in Z (both arguments of k) and its dvariance, dl
    twice the bilinear form's, halved here."""
    if not need_z:
        dvar, dls = ops.kxx_grad(spec, Z, U, V)
        return dvar, dls, None
    Zd = Z.detach()
    Y, Gb = torch.cat([U, V], dim=1), torch.cat([V, U], dim=1)
    dvar, dls, dZ = ops.kmn_knm_vjp(spec, Zd, Zd, None, Y, Gb, need_dZ=True)
    return 0.5 * dvar, [0.5 * v for v in dls], dZ


class _KzzTimes(torch.autograd.Function):
    """k(Z, Z) V for V [M, R], K never formed: forward `mgp_knm_matvec` on (Z, Z); backward dV = k(Z, Z) G and
    (dvariance, dlengthscales) = sum_r g_r^T (dK/dtheta) v_r by `mgp_kxx_grad`; when Z needs a gradient, all three of
    (dvariance, dlengthscales, dZ) by `_kzz_bilinear_grads`."""

    @staticmethod
    def forward(ctx, variance, lengthscales, Z, V, kind, fused_anyd=False):
        ctx.spec = ops.KernelSpec(kind, float(variance), [float(x) for x in lengthscales.reshape(-1)], Z.shape[1])
        ctx.v_shape, ctx.l_shape, ctx.fused_anyd = variance.shape, lengthscales.shape, fused_anyd
        V = V.contiguous()
        ctx.save_for_backward(Z, V)
        return anyd_matvec(fused_anyd, "knm", ctx.spec, Z, Z, V)

    @staticmethod
    def backward(ctx, G):
        Z, V = ctx.saved_tensors
        G = G.contiguous()
        dvar, dls, dZ = _kzz_bilinear_grads(ctx.spec, Z, G, V, ctx.needs_input_grad[2])
        gv, gl = _theta_grads(dvar, dls, ctx.v_shape, ctx.l_shape)
        dV = anyd_matvec(ctx.fused_anyd, "knm", ctx.spec, Z, Z, G) if ctx.needs_input_grad[3] else None
        return (gv, gl, dZ, dV, None, None)[:len(ctx.needs_input_grad)]  # `fused_anyd` is optional in apply()


class _KzzLambdaSolve(torch.autograd.Function):
    """X = (k(Z, Z) + diag lam)^-1 rhs for rhs [M, R] by the device CG on `KmmLambdaOperator`.  Backward, with
    Gb = (k(Z, Z) + diag lam)^-1 G (`_adjoint_solve`: the shortcut and the warm start of `_CGFunction` where they
    apply): d rhs = Gb, (dvariance, dlengthscales) = -sum_r gb_r^T (dK/dtheta) x_r (`mgp_kxx_grad`),
    dlam = -sum_r Gb o X; when Z needs a gradient, dZ of the same form by `_kzz_bilinear_grads`."""

    @staticmethod
    def forward(ctx, variance, lengthscales, lam, rhs, Z, kind, cg, wide=False, fused_anyd=False, wide_anyd=False):
        from .conjugate_gradient import KmmLambdaOperator, _solve_device
        kern = _frozen_kernel(kind, variance, lengthscales)
        ctx.op = KmmLambdaOperator(kern, Z, lam.detach().contiguous(), wide=wide, fused_anyd=fused_anyd,
                                   wide_anyd=wide_anyd)
        ctx.cfg = cg.config(Z.shape[0])
        ctx.v_shape, ctx.l_shape = variance.shape, lengthscales.shape
        rows = rhs.detach().t().contiguous()
        sol, _, err = _solve_device(ctx.op, rows, None, *ctx.cfg)
        ctx.save_for_backward(sol, rows, err)
        return sol.t().contiguous()

    @staticmethod
    def backward(ctx, G):
        from .conjugate_gradient import _adjoint_solve
        sol, rows, err = ctx.saved_tensors
        op = ctx.op
        Gb = _adjoint_solve(op, sol, rows, err, G.t().contiguous(), ctx.cfg, True).contiguous()
        dZ = None
        if ctx.needs_input_grad[4]:
            dvar, dls, dZ = _kzz_bilinear_grads(op.spec, op.Z, Gb.t(), sol.t(), True)
            dZ = -dZ
        else:
            dvar, dls = ops.kxx_grad(op.spec, op.Z, Gb, sol, ops.ROWS)
        gv, gl = _theta_grads(-dvar, [-v for v in dls], ctx.v_shape, ctx.l_shape)
        grads = (gv, gl, -(Gb * sol).sum(dim=0), Gb.t().contiguous(), dZ, None, None, None, None, None)
        return grads[:len(ctx.needs_input_grad)]  # `wide`, `fused_anyd`, `wide_anyd` are optional in apply()


class _KzzLambdaLogdet(torch.autograd.Function):
    """`eval_logdet` on the operator: value 0.0; backward (dvariance, dlengthscales) = df sum_r s_r^T (dK/dtheta) z_r / P
    and dlam = df sum_r S o Zp / P, with S = (k(Z, Z) + diag lam)^-1 Zp handed in (the trace estimator's solve, reused)
    or, when `solution` is None, solved in the backward pass as the reference does (`cggp/models.py:38-41`); when Z
    needs a gradient, dZ of the same form by `_kzz_bilinear_grads`."""

    @staticmethod
    def forward(ctx, variance, lengthscales, lam, solution, probes, Z, kind, cg, wide=False, fused_anyd=False,
                wide_anyd=False):
        ctx.kind, ctx.cg, ctx.have, ctx.wide, ctx.fused_anyd = kind, cg, solution is not None, wide, fused_anyd
        ctx.wide_anyd = wide_anyd
        ctx.v_shape, ctx.l_shape = variance.shape, lengthscales.shape
        ctx.theta = (float(variance), lengthscales.detach().clone())
        ctx.save_for_backward(lam.detach(), probes, Z, *((solution,) if ctx.have else ()))
        return torch.zeros((), dtype=Z.dtype, device=Z.device)

    @staticmethod
    def backward(ctx, df):
        from .conjugate_gradient import KmmLambdaOperator
        lam, probes, Z = ctx.saved_tensors[:3]
        kern = _frozen_kernel(ctx.kind, *ctx.theta)
        if ctx.have:
            S = ctx.saved_tensors[3]
        else:
            with torch.no_grad():
                S = ctx.cg(KmmLambdaOperator(kern, Z, lam.contiguous(), wide=ctx.wide, fused_anyd=ctx.fused_anyd,
                                             wide_anyd=ctx.wide_anyd),
                           probes)
        P = probes.shape[1]
        scale = float(df) / P
        dvar, dls, dZ = _kzz_bilinear_grads(kern.spec(Z.shape[1]), Z, S.contiguous(), probes.contiguous(),
                                            ctx.needs_input_grad[5])
        gv, gl = _theta_grads(scale * dvar, [scale * v for v in dls], ctx.v_shape, ctx.l_shape)
        grads = (gv, gl, scale * (S * probes).sum(dim=1), None, None, None if dZ is None else scale * dZ, None, None,
                 None, None, None)
        return grads[:len(ctx.needs_input_grad)]  # `wide`, `fused_anyd`, `wide_anyd` are optional in apply()


PANEL_BYTES = 256 << 20  # the largest row panel of a [B, M] cotangent that `_knm_theta_grads_panels` forms


def _knm_theta_grads_panels(spec, x, Z, G, V):
    """(dvariance, [dl_d]) of sum(G o (k(x, Z) V)) for G [B, R], V [M, R] at any D <= 512: row panels of the cotangent
    W = G V^T of at most `PANEL_BYTES` through `mgp_k_dense_vjp`, added in row order.  No dZ on this route."""
    B, M = x.shape[0], Z.shape[0]
    rows = max(1, PANEL_BYTES // (8 * M))
    dvar, dls = 0.0, [0.0] * spec.D
    Vt = V.t().contiguous()
    for i0 in range(0, B, rows):
        pv, pl = ops.k_dense_vjp(spec, x[i0:i0 + rows], Z, G[i0:i0 + rows] @ Vt)
        dvar += pv
        dls = [s + p for s, p in zip(dls, pl)]
    return dvar, dls


class _KnmTimes(torch.autograd.Function):
    """k(x, Z) [V | C] for V [M, R], C [M, Rc] (C a constant: the probes), the [B, M] block never formed: forward ONE
    `mgp_knm_matvec` on the R + Rc columns.  Backward at G [B, R + Rc]: dV = k(Z, x) G[:, :R] by `mgp_kmn_matvec`, and
    (dvariance, dlengthscales, dZ) by ONE `mgp_kmn_knm_vjp` call with Gq = NULL, Y = G and Gb = [V | C] -- the cotangent
    of the block is G [V | C]^T, of rank R + Rc.  D > 32 (which that entry point refuses): dvariance and dlengthscales
    by `_knm_theta_grads_panels`; a Z that needs a gradient there is refused at the model's construction."""

    @staticmethod
    def forward(ctx, variance, lengthscales, Z, V, C, x, kind, fused_anyd=False):
        ctx.spec = ops.KernelSpec(kind, float(variance), [float(v) for v in lengthscales.reshape(-1)], Z.shape[1])
        ctx.v_shape, ctx.l_shape, ctx.live = variance.shape, lengthscales.shape, V.shape[1]
        ctx.fused_anyd = fused_anyd
        VC = torch.cat([V.detach(), C.detach()], dim=1).contiguous()
        Zd = Z.detach()
        ctx.save_for_backward(Zd, VC, x)
        return anyd_matvec(fused_anyd, "knm", ctx.spec, x, Zd, VC)

    @staticmethod
    def backward(ctx, G):
        Zd, VC, x = ctx.saved_tensors
        G = G.contiguous()
        spec, need_z = ctx.spec, ctx.needs_input_grad[2]
        if spec.D <= 32:
            dvar, dls, dZ = ops.kmn_knm_vjp(spec, x, Zd, None, G, VC, need_dZ=need_z)
        else:
            if need_z:
                raise ValueError(f"the trace form's gradient in Z needs D <= 32, got D={spec.D}")
            dvar, dls = _knm_theta_grads_panels(spec, x, Zd, G, VC)
            dZ = None
        gv, gl = _theta_grads(dvar, dls, ctx.v_shape, ctx.l_shape)
        dV = None
        if ctx.needs_input_grad[3]:
            dV = anyd_matvec(ctx.fused_anyd, "kmn", spec, x, Zd, G[:, :ctx.live].contiguous())
        return (gv, gl, dZ, dV, None, None, None, None)[:len(ctx.needs_input_grad)]  # `fused_anyd` is optional


def _rff_vjp_panels(x, theta, W, scale, G, want_dX=False):
    """(dtheta [L, D], dX [N, D] or None) of sum(G o rff_sample(x, theta, W, scale)) for G [S, N], by row chunks of at
    most `PANEL_BYTES` of feature panels [cos | sin] (`rff.basis_vectors`: `mgp_rff_features` on the device, torch on the
    host): Q = scale ((G^T W_s) o cos - (G^T W_c) o sin), dtheta += Q^T x, dX = Q theta.  The route of `_RffSample`
    outside `mgp_rff_sample_vjp`'s range (D > 32 or S > 8), and on host tensors the reference of its tests."""
    from . import rff
    N, L = x.shape[0], theta.shape[0]
    rows = max(1, PANEL_BYTES // (16 * max(L, 1)))
    Wc, Ws = W[:, :L], W[:, L:]
    dtheta = torch.zeros_like(theta)
    dX = torch.empty_like(x) if want_dX else None
    for i0 in range(0, N, rows):
        xb, Gb = x[i0:i0 + rows].contiguous(), G[:, i0:i0 + rows].t()
        phi = rff.basis_vectors(xb, theta)
        Q = scale * ((Gb @ Ws) * phi[:, :L] - (Gb @ Wc) * phi[:, L:])
        dtheta += Q.t() @ xb
        if want_dX:
            dX[i0:i0 + rows] = Q @ theta
    return dtheta, dX


class _RffSample(torch.autograd.Function):
    """Prior function samples [S, B + M] = scale W Phi([x; Z])^T on random Fourier features, differentiable in the
    frequencies theta [L, D], in scale (a 0-dim tensor, sqrt(variance / L)) and in Z.  Forward: ONE `mgp_rff_sample` on
    the B + M rows.  Backward at G [S, B + M]: dtheta from one `mgp_rff_sample_vjp` call on all rows, dZ from a second
    call on the M rows of Z alone (only when Z needs a gradient), dscale = sum(G o out) / scale by `mgp_dot_all`.
    D > 32 or S > 8 (which that entry point refuses): `_rff_vjp_panels` -- unless `rff_anyd` (False, True or "auto", as
    `rff.rff_sample`) sends the D > 32, S <= 8 calls to the fused any-D kernels (MGP_RFF_ANYD)."""

    @staticmethod
    def forward(ctx, theta, scale, x, Z, W, rff_anyd=False):
        from . import rff
        pts = torch.cat([x, Z.detach()], dim=0).contiguous()
        theta, W = theta.detach().contiguous(), W.contiguous()
        ctx.scale, ctx.B = float(scale), x.shape[0]
        ctx.rff_anyd = rff.check_rff_anyd(rff_anyd)
        anyd = pts.is_cuda and rff.use_rff_anyd(rff_anyd, pts.dtype, pts.shape[1], W.shape[0], pts.shape[0],
                                                theta.shape[0])
        out = ops.rff_sample(pts, theta, W, ctx.scale, ops.ROWS, anyd=anyd)
        ctx.save_for_backward(pts, theta, W, out, scale)
        return out

    @staticmethod
    def backward(ctx, G):
        pts, theta, W, out, scale = ctx.saved_tensors
        G = G.contiguous()
        D, S, B = pts.shape[1], W.shape[0], ctx.B
        from . import rff
        fused = D <= 32 and S <= 8
        L = theta.shape[0]
        anyd = lambda n, op: pts.is_cuda and rff.use_rff_anyd(ctx.rff_anyd, pts.dtype, D, S, n, L, op)
        need_theta, need_scale, need_z = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        dtheta = dZ = dscale = None
        if need_theta:
            if fused or anyd(pts.shape[0], "dtheta"):
                dtheta, _ = ops.rff_sample_vjp(pts, theta, W, ctx.scale, G, ops.ROWS, anyd=not fused)
            else:
                dtheta, _ = _rff_vjp_panels(pts, theta, W, ctx.scale, G)
        if need_z:
            Zd, Gz = pts[B:].contiguous(), G[:, B:].contiguous()
            if fused or anyd(Zd.shape[0], "dX"):
                _, dZ = ops.rff_sample_vjp(Zd, theta, W, ctx.scale, Gz, ops.ROWS, want_dtheta=False, want_dX=True,
                                           anyd=not fused)
            else:
                _, dZ = _rff_vjp_panels(Zd, theta, W, ctx.scale, Gz, want_dX=True)
        if need_scale:
            v = ops.dot_all(G, out) / ctx.scale if ctx.scale != 0.0 else 0.0
            dscale = torch.tensor(v, dtype=scale.dtype, device=scale.device).reshape(scale.shape)
        return (dtheta, dscale, None, dZ, None, None)[:len(ctx.needs_input_grad)]  # `rff_anyd` is optional in apply()


class _KmnKnm(torch.autograd.Function):
    """Q = k(Z, x) k(x, Z) [M, M] by `mgp_kmn_knm`; backward `mgp_kmn_knm_vjp` with the dense cotangent Gq, as
    `_SGPRElbo` (fp64, D <= 32)."""

    @staticmethod
    def forward(ctx, variance, lengthscales, Z, x, kind):
        ctx.spec = ops.KernelSpec(kind, float(variance), [float(v) for v in lengthscales.reshape(-1)], Z.shape[1])
        ctx.v_shape, ctx.l_shape = variance.shape, lengthscales.shape
        Zd = Z.detach()
        ctx.save_for_backward(Zd, x)
        return ops.kmn_knm(ctx.spec, x, Zd)

    @staticmethod
    def backward(ctx, G):
        Zd, x = ctx.saved_tensors
        dvar, dls, dZ = ops.kmn_knm_vjp(ctx.spec, x, Zd, G.contiguous(), need_dZ=ctx.needs_input_grad[2])
        gv, gl = _theta_grads(dvar, dls, ctx.v_shape, ctx.l_shape)
        return gv, gl, dZ, None, None


class TrainableCGGP:
    """Differentiable `CGGP.elbo` (`cggp/models.py:125-134,293-354`).

    The log-det gradient reuses `K^-1 Zp` of the trace estimator's probe solve instead of running
    the reference's second probe solve in the backward pass (same estimator, one CG less per step).
    `fused_solves=True` additionally sends `pseudo_u`, `Kmn` and the probes through ONE device CG as
    columns of one right-hand side; measured slower at C2 sizes (72.9 vs 67.2 ms per Adam step)
    because the reference's "any column not converged" stopping rule then makes the 1000-column
    GEMM-regime solve run as long as the slowest (Rademacher) columns, so it is off by default.

    `matrix_free=True`: the same ELBO with K_mm never formed, at any M.  The Z-Z block enters through three autograd
    nodes -- `_KzzTimes` (k(Z, Z) V), `_KzzLambdaSolve` (the device CG on `KmmLambdaOperator`) and `_KzzLambdaLogdet` --
    whose backward passes contract dL/dK with dK/dtheta by `mgp_kxx_grad`; the [M, B] block of a batch keeps `_KBlock`.
    The exact trace (`num_probes=None` without `probes`) needs M right-hand sides and raises `ValueError`.
    `fused_solves=True` works there too: one operator solve on the columns [pseudo_u, K_mn, probes].
    `fused_anyd` (False, True or "auto"; with `matrix_free=True` only) is handed to every `KmmLambdaOperator` and is
    the rule of the K(Z, Z) and K(x, Z) products of the autograd nodes (forward and the `dV` of their backward), as in
    `models.CGGP`; the hyper-parameter gradients keep their entry points.
    `wide_solves` (False, True or "auto"; with `matrix_free=True` only) is handed to every `KmmLambdaOperator`, as in
    `models.CGGP`.
    `wide_anyd` (False, True or "auto"; with `matrix_free=True` only) likewise: at D > 32 in fp64 the solves of
    `_KzzLambdaSolve` and `_KzzLambdaLogdet` run `MGP_OP_KMM_LAMBDA_WIDE_ANYD` (include/mgp_sweep_anyd.h), always or
    under `conjugate_gradient.wide_anyd_auto`.

    `fused_point_grads` (False, True or "auto"; default False: the code above, bit for bit) is handed to every
    `self.kernel.K(...)` block: with a trainable Z the backward pass of a block is then one `mgp_k_dense_vjp_points` call
    (include/mgp_points.h) instead of `mgp_k_dense_vjp` + `k_grad_points` -- always (True) or where it was measured at
    most 0.9 of the torch route (`conjugate_gradient.fused_point_grads_auto`).  The forward pass does not change; fp32
    and host tensors take the torch route whatever the setting.

    `trainable_inducing=True` (the reference's `--tip`: `set_trainable(model.inducing_variable, tip)`,
    `paper_cli_geospatial.py:237`): the model keeps its own copy of Z as a leaf, `parameters()` ends with it and
    `frozen_model()` hands over a detached copy.  The dense model differentiates its kernel blocks in Z by
    `k_grad_points` (any D); with `matrix_free=True` each of the three nodes makes one `mgp_kmn_knm_vjp` call on (Z, Z)
    with a rank-2R cotangent (fp64, D <= 32: `ValueError` at construction beyond).  `pseudo_u` and `cluster_counts`
    stay frozen (`models.py:220`).  The reference's `--tip` flow passes `update_fn=None`; replacing `model.Z` from an
    `update_fn` while it is trainable is not supported (the optimiser would keep stepping the old leaf).

    `data_term="trace"` (default "batch": everything above, the reference's form): the sum of the rows'
    predictive variances enters as `B variance - tr(A^-1 K_mn K_nm)`, A = K_mm + Lambda, and the trace is estimated
    with the probes Zp of the KL term, whose solves S = A^-1 Zp are shared:

        [mu | U | V] = K_nm [a | S | Zp],    sum_n var_exp_n = -(B/2) log(2 pi s2)
                                                 - (|y - mu|^2 + B variance - (1/P) sum_p U_p . V_p) / (2 s2)

    so every solve has 1 + P columns whatever B is, the rows pass through `_KnmTimes` (`mgp_knm_matvec` forward;
    `mgp_kmn_matvec` and ONE `mgp_kmn_knm_vjp` call of 2 P + 1 columns backward) and nothing [M, B] is formed: this is
    the form for the full data set (`train_using_lbfgs_and_update`) and works on a minibatch alike.  KL, scale, the
    log-det node and the probe handling are those of "batch"; `fused_solves=True` sends [pseudo_u | probes] through
    one solve; `wide_solves` has nothing to widen.  With exact probes (`probes = sqrt(M) I`) it equals "batch"; with P
    Rademacher probes it is an unbiased estimate of it (the README gives the spread).  `num_probes=None` without
    `probes=`: the dense model forms Q = K_mn K_nm (`mgp_kmn_knm`, D <= 32) and takes both traces from one M-column
    solve, tr(A^-1 (K_mm + (scale / s2) Q)), which equals "batch" at `num_probes=None`; the matrix-free model raises
    `ValueError`, as above.  fp64 only.  D > 32: variance, lengthscales and noise only -- the kernel gradient then
    walks row panels of the rank-(2 P + 1) cotangent (at most 256 MiB) through `mgp_k_dense_vjp`; with
    `trainable_inducing=True` that is a `ValueError` at construction.

    `data_term="pathwise"` (the reference's `PathwiseClusterGP.elbo`, `cggp/models.py:357-420`, made
    trainable): the likelihood term from S = `num_samples` pathwise posterior samples on L = `num_bases` random Fourier
    features,

        f_s = phi(x) w_s sqrt(variance / L) + K_nm A^-1 (u - phi(Z) w_s sqrt(variance / L) - eps_s),
        data term = -(1/2) [sum_sn (y_n - f_sn)^2 / (S s2) + B log(2 pi s2)] scale,

    with theta = E / lengthscales the reparameterised frequencies (E the base draws, Matern factor included), the prior
    draw one `_RffSample` node on [x; Z] (`mgp_rff_sample` forward, `mgp_rff_sample_vjp` backward), eps = sqrt(lam) xi
    (`epsilon="matheron"`, the default here: the expectation over W and xi is then the "batch" data term up to the
    random-feature truncation) or lam xi ("reference"), the S-column solve through `_KzzLambdaSolve` or the dense CG and
    the correction through `_KnmTimes`.  The [M, M] solve has S columns whatever B is, the quadratic part is >= 0 on every
    draw, and the sum over rows averages itself.  KL, scale, the log-det node and the probe handling are those of the
    other forms; `fused_solves=True` sends [pseudo_u | probes | u - f_Z - eps] through one solve.  The draws (E, W, xi)
    come from `pathwise_seed`, which advances per call like `probe_seed`, or are injected as
    `elbo(data, pathwise=(E, W, xi))` (`draw_pathwise`).  fp64 only; D > 32 or S > 8: the prior draw's backward pass walks
    row chunks of feature panels (`_rff_vjp_panels`), and `trainable_inducing=True` at D > 32 is a `ValueError`.
    `rff_anyd` (False, True or "auto"; with `data_term="pathwise"` only, anything but False with another data term is a
    `ValueError`) sends the prior draw and its backward pass at D > 32, S <= 8 to libmgp's fused any-D kernels
    (MGP_RFF_ANYD, include/mgp_pathwise.h) instead; "auto" follows `rff.rff_anyd_auto`."""

    def __init__(self, kernel, noise_variance, Z, conjugate_gradient=None, num_probes=5, *, pseudo_u, cluster_counts,
                 num_data=None, fused_solves=False, independent_logdet_probes=False, matrix_free=False,
                 wide_solves=False, trainable_inducing=False, data_term="batch", num_bases=1024, num_samples=5,
                 epsilon="matheron", fused_anyd=False, fused_point_grads=False, wide_anyd=False, rff_anyd=False):
        from .conjugate_gradient import check_wide
        from .rff import check_rff_anyd
        self.rff_anyd = check_rff_anyd(rff_anyd)
        if self.rff_anyd is not False and data_term != "pathwise":
            raise ValueError(f"rff_anyd needs data_term='pathwise': no other data term draws random Fourier features "
                             f"(got data_term={data_term!r})")
        self.fused_point_grads = check_fused_point_grads(fused_point_grads)
        self.wide_anyd = check_wide(wide_anyd, "wide_anyd")
        if self.wide_anyd is not False and not matrix_free:
            raise ValueError("wide_anyd needs matrix_free=True: without it there is no operator to widen")
        self.wide_solves = check_wide(wide_solves, "wide_solves")
        if self.wide_solves is not False and not matrix_free:
            raise ValueError("wide_solves needs matrix_free=True: without it there is no operator to widen")
        self.fused_anyd = check_fused_anyd(fused_anyd)
        if self.fused_anyd is not False and not matrix_free:
            raise ValueError("fused_anyd needs matrix_free=True: without it K_mm is a dense matrix and no sweep runs")
        self.data_term = check_data_term(data_term, Z.dtype, Z.shape[1], trainable_inducing)
        self.num_bases, self.num_samples, self.epsilon = check_pathwise(num_bases, num_samples, epsilon)
        self.pathwise_seed = 0
        self.kernel = kernel if isinstance(kernel, TrainableKernel) else TrainableKernel(kernel)
        self.noise_p = Parameter(noise_variance)
        self.trainable_inducing = bool(trainable_inducing)
        if self.trainable_inducing:
            if matrix_free and Z.shape[1] > 32:
                raise ValueError(f"matrix_free=True with trainable_inducing=True needs D <= 32, got D={Z.shape[1]} "
                                 "(the dense model takes any D)")
            Z = Z.detach().clone().contiguous().requires_grad_(True)
        self.Z = Z
        self.pseudo_u = pseudo_u.reshape(-1, 1)
        self.cluster_counts = cluster_counts.reshape(-1, 1)
        self.conjugate_gradient = conjugate_gradient or ConjugateGradient(1e-6)
        self.num_probes = num_probes
        self.num_data = num_data
        self.probe_seed = 0
        self.fused_solves = bool(fused_solves)
        # True: the reference's estimator exactly -- `eval_logdet`'s backward draws its OWN Rademacher probes and
        # runs its own probe solve (`cggp/models.py:38-41`), independent of the trace estimator's (`:310`).
        # False (default): K^-1 Zp of the trace solve is reused -- same expectation, one CG less per step, but the
        # two estimates are then correlated
        self.independent_logdet_probes = bool(independent_logdet_probes)
        self.logdet_probe_seed = 1 << 20
        self.matrix_free = bool(matrix_free)

    def parameters(self):
        ps = self.kernel.parameters() + [self.noise_p.raw]
        return ps + [self.Z] if self.trainable_inducing else ps

    def _elbo_matrix_free(self, data, probes):
        x, y = data
        Z, cg, kind = self.Z, self.conjugate_gradient, self.kernel.name
        dev, dt, M = Z.device, Z.dtype, Z.shape[0]
        if self.num_probes is None and probes is None:
            raise ValueError("matrix_free=True needs num_probes (or probes=): the exact trace solves M right-hand sides")
        s2 = self.noise_p().to(device=dev, dtype=dt)
        var_p, ls = self.kernel.variance_p(), self.kernel.lengthscales_p()
        if ls.dim() == 0:
            ls = ls.reshape(1)
        var_f = var_p.to(device=dev, dtype=dt)
        lam = s2 / self.cluster_counts[:, 0]  # diag_variance, :226-228
        Kmn = self.kernel.K(Z, x, fused_point_grads=self.fused_point_grads)  # :334
        if probes is None:
            probes = rademacher((M, self.num_probes), dt, dev, self.probe_seed)
            self.probe_seed += 1
        P = probes.shape[1]
        times_kzz = lambda V: _KzzTimes.apply(var_p, ls, Z, V, kind, self.fused_anyd)
        wide = self.wide_solves
        solve = lambda rhs: _KzzLambdaSolve.apply(var_p, ls, lam, rhs, Z, kind, cg, wide, self.fused_anyd,
                                                          self.wide_anyd)
        if self.fused_solves:
            B = Kmn.shape[1]
            sol = solve(torch.cat([self.pseudo_u, Kmn, probes], dim=1))  # :303, :339, :311 in one solve
            a, W, S = sol[:, :1], sol[:, 1:1 + B], sol[:, 1 + B:]
        else:
            a, W, S = solve(self.pseudo_u), solve(Kmn), solve(probes)  # :303 / :339, :340, :311
        fvar = (var_f - (Kmn * W).sum(dim=0))[:, None]  # :343-345
        fmu = Kmn.t() @ a  # :351
        var_exp = -0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(s2) - 0.5 * ((y - fmu) ** 2 + fvar) / s2
        trace = (S * times_kzz(probes)).sum() / P  # :312-314
        quad = (times_kzz(a) * a).sum()  # :316-317
        if self.independent_logdet_probes:
            own = rademacher((M, P), dt, dev, self.logdet_probe_seed)  # fresh draw, :38-39
            self.logdet_probe_seed += 1
            logdet = _KzzLambdaLogdet.apply(var_p, ls, lam, None, own, Z, kind, cg, wide,
                                            self.fused_anyd, self.wide_anyd)  # solved in the backward pass
        else:
            logdet = _KzzLambdaLogdet.apply(var_p, ls, lam, S.detach(), probes, Z, kind, cg, wide,
                                            self.fused_anyd, self.wide_anyd)  # K^-1 Zp reused
        const = torch.log(lam).sum()  # :321
        kl = 0.5 * (quad - trace + logdet - const)
        scale = 1.0 if self.num_data is None else float(self.num_data) / float(x.shape[0])  # :163-169
        return var_exp.sum() * scale - kl

    def _probed_kl(self, probes, solve, times_kzz, KL, lam, var_p, ls, extra=None):
        """The KL term with Hutchinson probes, shared by the "trace" and "pathwise" forms, dense (KL = K_mm + Lambda)
        and matrix-free (KL None): (kl, a, S, probes, w) with a = A^-1 pseudo_u, S = A^-1 probes and, when `extra`
        [M, R] is given, w = A^-1 extra -- further columns of the one solve under `fused_solves`, a solve of their own
        otherwise."""
        Z, cg, kind = self.Z, self.conjugate_gradient, self.kernel.name
        dev, dt, M = Z.device, Z.dtype, Z.shape[0]
        if probes is None:
            probes = rademacher((M, self.num_probes), dt, dev, self.probe_seed)
            self.probe_seed += 1
        P = probes.shape[1]
        w = None
        if self.fused_solves:
            cols = [self.pseudo_u, probes] + ([] if extra is None else [extra])
            sol = solve(torch.cat(cols, dim=1))  # :303 / :339 and :311 in one solve
            a, S = sol[:, :1], sol[:, 1:1 + P]
            if extra is not None:
                w = sol[:, 1 + P:]
        else:
            a, S = solve(self.pseudo_u), solve(probes)  # :303 / :339, :311
            if extra is not None:
                w = solve(extra)
        trace = (S * times_kzz(probes)).sum() / P  # :312-314
        quad = (times_kzz(a) * a).sum()  # :316-317
        own = None
        if self.independent_logdet_probes:
            own = rademacher((M, P), dt, dev, self.logdet_probe_seed)  # fresh draw, :38-39
            self.logdet_probe_seed += 1
        if self.matrix_free:  # solved in the backward pass from `own`, else K^-1 Zp reused
            logdet = _KzzLambdaLogdet.apply(var_p, ls, lam, None if own is not None else S.detach(),
                                            probes if own is None else own, Z, kind, cg, self.wide_solves,
                                            self.fused_anyd, self.wide_anyd)
        elif own is not None:
            logdet = eval_logdet(KL, cg, P, own)  # second probe solve in the backward pass, :40-42
        else:
            logdet = _LogdetFromSolution.apply(KL, S.detach(), probes)  # :319 with K^-1 Zp reused
        const = torch.log(lam).sum()  # :321
        return 0.5 * (quad - trace + logdet - const), a, S, probes, w

    def _elbo_trace(self, data, probes):
        """`elbo` with `data_term="trace"`, dense and matrix-free (the class docstring has the formulas)."""
        x, y = data
        Z, cg, kind = self.Z, self.conjugate_gradient, self.kernel.name
        dev, dt, M, B = Z.device, Z.dtype, Z.shape[0], x.shape[0]
        exact = self.num_probes is None and probes is None
        if self.matrix_free and exact:
            raise ValueError("matrix_free=True needs num_probes (or probes=): the exact trace solves M right-hand sides")
        s2 = self.noise_p().to(device=dev, dtype=dt)
        var_p, ls = self.kernel.variance_p(), self.kernel.lengthscales_p()
        if ls.dim() == 0:
            ls = ls.reshape(1)
        var_f = var_p.to(device=dev, dtype=dt)
        lam = s2 / self.cluster_counts[:, 0]  # diag_variance, :226-228
        if self.matrix_free:
            wide = self.wide_solves
            times_kzz = lambda V: _KzzTimes.apply(var_p, ls, Z, V, kind, self.fused_anyd)
            solve = lambda rhs: _KzzLambdaSolve.apply(var_p, ls, lam, rhs, Z, kind, cg, wide, self.fused_anyd,
                                                          self.wide_anyd)
        else:
            Kmm = self.kernel.K(Z, fused_point_grads=self.fused_point_grads)  # :300 / :333
            KL = Kmm + torch.diag(lam)  # add_diagonal, :301 / :337
            times_kzz = lambda V: Kmm @ V
            solve = lambda rhs: cg(KL, rhs)
        knm_times = lambda V, C: _KnmTimes.apply(var_p, ls, Z, V, C, x.contiguous(), kind, self.fused_anyd)
        scale = 1.0 if self.num_data is None or B == 0 else float(self.num_data) / float(B)  # :163-169
        const = torch.log(lam).sum()  # :321
        log_norm = -0.5 * B * (math.log(2.0 * math.pi) + torch.log(s2))
        if exact:  # the dense model alone
            a = solve(self.pseudo_u)  # :303 / :339
            quad = (times_kzz(a) * a).sum()  # :316-317
            logdet = eval_logdet(KL, cg, None, None)  # :319
            if B == 0:
                return 0.5 * torch.diagonal(solve(Kmm)).sum() - 0.5 * (quad + logdet - const)  # :304-306
            # tr(A^-1 K_mm) of the KL term and (scale / s2) tr(A^-1 Q) of the data term from one M-column solve
            Q = _KmnKnm.apply(var_p, ls, Z, x.contiguous(), kind)
            both = torch.diagonal(solve(Kmm + (scale / s2) * Q)).sum()
            fmu = knm_times(a, a.new_empty((M, 0)))
            data_sum = log_norm - 0.5 * (((y - fmu) ** 2).sum() + B * var_f) / s2
            return data_sum * scale + 0.5 * both - 0.5 * (quad + logdet - const)
        kl, a, S, probes, _ = self._probed_kl(probes, solve, times_kzz, None if self.matrix_free else KL, lam, var_p, ls)
        P = probes.shape[1]
        if B == 0:
            return -kl
        out = knm_times(torch.cat([a, S], dim=1), probes)  # [mu | U | V], [B, 2 P + 1]
        fmu, U, V = out[:, :1], out[:, 1:1 + P], out[:, 1 + P:]
        data_sum = log_norm - 0.5 * (((y - fmu) ** 2).sum() + B * var_f - (U * V).sum() / P) / s2
        return data_sum * scale - kl

    def draw_pathwise(self, seed):
        """(E, W, xi) of one `data_term="pathwise"` evaluation (`models.draw_pathwise`) at the model's sizes."""
        return draw_pathwise(self.kernel.name, self.Z.shape[1], self.Z.shape[0], self.num_bases, self.num_samples, seed)

    def _elbo_pathwise(self, data, probes, pathwise):
        """`elbo` with `data_term="pathwise"`, dense and matrix-free (the class docstring has the formulas)."""
        x, y = data
        Z, cg, kind = self.Z, self.conjugate_gradient, self.kernel.name
        dev, dt, M, B, D = Z.device, Z.dtype, Z.shape[0], x.shape[0], Z.shape[1]
        exact = self.num_probes is None and probes is None
        if self.matrix_free and exact:
            raise ValueError("matrix_free=True needs num_probes (or probes=): the exact trace solves M right-hand sides")
        if pathwise is None:
            pathwise = self.draw_pathwise(self.pathwise_seed)
            self.pathwise_seed += 1
        E, W, xi = (torch.as_tensor(t).to(device=dev, dtype=dt).contiguous() for t in pathwise)
        L, S = E.shape[0], W.shape[0]
        if E.shape != (L, D) or W.shape != (S, 2 * L) or xi.shape != (S, M) or L < 1 or S < 1:
            raise ValueError(f"pathwise=(E [L, D={D}], W [S, 2L], xi [S, M={M}]) expected, got {tuple(E.shape)}, "
                             f"{tuple(W.shape)}, {tuple(xi.shape)}")
        s2 = self.noise_p().to(device=dev, dtype=dt)
        var_p, ls = self.kernel.variance_p(), self.kernel.lengthscales_p()
        if ls.dim() == 0:
            ls = ls.reshape(1)
        lam = s2 / self.cluster_counts[:, 0]  # diag_variance, :226-228
        KL = None
        if self.matrix_free:
            wide = self.wide_solves
            times_kzz = lambda V: _KzzTimes.apply(var_p, ls, Z, V, kind, self.fused_anyd)
            solve = lambda rhs: _KzzLambdaSolve.apply(var_p, ls, lam, rhs, Z, kind, cg, wide, self.fused_anyd,
                                                          self.wide_anyd)
        else:
            Kmm = self.kernel.K(Z, fused_point_grads=self.fused_point_grads)  # :300 / :333
            KL = Kmm + torch.diag(lam)  # add_diagonal, :301 / :337
            times_kzz = lambda V: Kmm @ V
            solve = lambda rhs: cg(KL, rhs)
        rhs = None
        if B > 0:
            theta = E / ls.to(device=dev, dtype=dt)[None, :]  # the reparameterised frequencies, reference rff.py:20-45
            prior = _RffSample.apply(theta, torch.sqrt(var_p / L), x.contiguous(), Z, W,
                                     self.rff_anyd)  # [S, B + M], :397-402
            eps = (torch.sqrt(lam) if self.epsilon == "matheron" else lam)[None, :] * xi  # :404-408
            rhs = (self.pseudo_u[:, 0][None, :] - prior[:, B:] - eps).t()  # [M, S], :414
        if exact:  # the dense model alone
            a = solve(self.pseudo_u)  # :303 / :339
            quad = (times_kzz(a) * a).sum()  # :316-317
            trace = torch.diagonal(solve(Kmm)).sum()  # :304-306
            kl = 0.5 * (quad - trace + eval_logdet(KL, cg, None, None) - torch.log(lam).sum())  # :319-322
            w = solve(rhs) if B > 0 else None
        else:
            kl, _, _, _, w = self._probed_kl(probes, solve, times_kzz, KL, lam, var_p, ls, extra=rhs)
        if B == 0:
            return -kl
        corr = _KnmTimes.apply(var_p, ls, Z, w, w.new_empty((M, 0)), x.contiguous(), kind,
                               self.fused_anyd)  # [B, S], :418
        f = prior[:, :B] + corr.t()  # :419
        sq = ((y.reshape(1, -1) - f) ** 2).sum()  # :384-385
        scale = 1.0 if self.num_data is None else float(self.num_data) / float(B)  # :163-169
        data_sum = -0.5 * (sq / (S * s2) + B * (math.log(2.0 * math.pi) + torch.log(s2)))  # :386-388
        return data_sum * scale - kl

    def elbo(self, data, probes=None, pathwise=None):
        if self.data_term == "trace":
            return self._elbo_trace(data, probes)
        if self.data_term == "pathwise":
            return self._elbo_pathwise(data, probes, pathwise)
        if self.matrix_free:
            return self._elbo_matrix_free(data, probes)
        x, y = data
        dev, dt = self.Z.device, self.Z.dtype
        cg = self.conjugate_gradient
        s2 = self.noise_p().to(device=dev, dtype=dt)
        var_f = self.kernel.variance_p().to(device=dev, dtype=dt)
        Kmm = self.kernel.K(self.Z, fused_point_grads=self.fused_point_grads)  # :300 / :333
        lam = s2 / self.cluster_counts[:, 0]  # diag_variance, :226-228
        KL = Kmm + torch.diag(lam)  # add_diagonal, :301 / :337
        Kmn = self.kernel.K(self.Z, x, fused_point_grads=self.fused_point_grads)  # :334
        fused = self.fused_solves and not (self.num_probes is None and probes is None)
        reuse = fused
        if fused:
            if probes is None:
                probes = rademacher((Kmm.shape[0], self.num_probes), dt, dev, self.probe_seed)
                self.probe_seed += 1
            B = Kmn.shape[1]
            sol = cg(KL, torch.cat([self.pseudo_u, Kmn, probes], dim=1))  # :303, :339, :311 in one solve
            a, W, S = sol[:, :1], sol[:, 1:1 + B], sol[:, 1 + B:]
        else:
            a = cg(KL, self.pseudo_u)  # :303 / :339
            W = cg(KL, Kmn)  # :340
        fvar = (var_f - (Kmn * W).sum(dim=0))[:, None]  # :343-345
        fmu = Kmn.t() @ a  # :351
        var_exp = -0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(s2) - 0.5 * ((y - fmu) ** 2 + fvar) / s2
        # prior_kl, :293-322
        if fused:
            trace = (S * (Kmm @ probes)).sum() / probes.shape[1]  # :312-314
        elif self.num_probes is None and probes is None:
            trace = torch.diagonal(cg(KL, Kmm)).sum()  # :304-306
        else:
            if probes is None:
                probes = rademacher((Kmm.shape[0], self.num_probes), dt, dev, self.probe_seed)
                self.probe_seed += 1
            S = cg(KL, probes)  # :311
            trace = (S * (Kmm @ probes)).sum() / probes.shape[1]  # :312-314
            reuse = True
        quad = ((Kmm @ a) * a).sum()  # :316-317
        if reuse and self.independent_logdet_probes:
            P = probes.shape[1]
            own = rademacher((Kmm.shape[0], P), dt, dev, self.logdet_probe_seed)  # fresh draw, :38-39
            self.logdet_probe_seed += 1
            logdet = eval_logdet(KL, cg, P, own)  # second probe solve in the backward pass, :40-42
        elif reuse:
            logdet = _LogdetFromSolution.apply(KL, S.detach(), probes)  # :319 with K^-1 Zp reused
        else:
            logdet = eval_logdet(KL, cg, self.num_probes if probes is None else probes.shape[1], probes)  # :319
        const = torch.log(lam).sum()  # :321
        kl = 0.5 * (quad - trace + logdet - const)
        scale = 1.0 if self.num_data is None else float(self.num_data) / float(x.shape[0])  # :163-169
        return var_exp.sum() * scale - kl

    def training_loss(self, data, probes=None, pathwise=None):
        return -self.elbo(data, probes=probes, pathwise=pathwise)

    def frozen_model(self):
        from .models import CGGP
        Z = self.Z.detach().clone() if self.trainable_inducing else self.Z
        return CGGP(self.kernel.frozen(), self.noise_p.value, Z, self.conjugate_gradient,
                    num_probes=self.num_probes, pseudo_u=self.pseudo_u, cluster_counts=self.cluster_counts,
                    num_data=self.num_data, matrix_free=self.matrix_free, wide_solves=self.wide_solves,
                    data_term=self.data_term, num_bases=self.num_bases, num_samples=self.num_samples,
                    epsilon=self.epsilon, fused_anyd=self.fused_anyd, wide_anyd=self.wide_anyd,
                    rff_anyd=self.rff_anyd)


class _GPRLmlEstimate(torch.autograd.Function):
    """Stochastic Lanczos estimate of log N(y | 0, K + s2 I) (`GPR.log_marginal_likelihood_estimate`) as an autograd
    node over (variance, lengthscales, s2).  Backward, with alpha = Khat^-1 Y and W = Khat^-1 Z of the forward solve:

        dLML/dtheta = 1/2 sum_p alpha_p^T dK alpha_p - 1/2 (P / t) sum_i (Khat^-1 z_i)^T dK z_i

    -- one `mgp_kxx_grad` call with u = 1/2 [alpha, -(P/t) W] and v = [alpha, Z]; the s2 term is the same form with
    dK = I, sum(u * v).  It is the Hutchinson estimate of the gradient (unbiased), not the exact derivative of the
    fixed-probe value.

    With a `PivotedCholeskyPreconditioner` P on `cg` the probes are draws from N(0, P) (`probes`, or
    `P.sample(num_probes, seed=seed)` when `probes` is None) and the trace term is E[(Khat^-1 z)^T dK (P^-1 z)]:
    v = [alpha, P^-1 Z].  P is held fixed within one evaluation (it is not differentiated); the estimator stays
    unbiased because E[z z^T] = P whatever P is."""

    @staticmethod
    def forward(ctx, variance, lengthscales, s2, X, Y, probes, kind, cg, num_probes=None, seed=0, fused_anyd=False,
                sym_anyd=False):
        from . import kernels
        from .models import GPR
        cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
               "matern52": kernels.Matern52}[kind]
        kern = cls(variance=float(variance), lengthscales=[float(v) for v in lengthscales.reshape(-1)])
        model = GPR((X, Y), kern, noise_variance=float(s2), conjugate_gradient=cg, solver="cg", fused_anyd=fused_anyd,
                    sym_anyd=sym_anyd)
        if probes is None:
            est, alpha, W, Z = model._lml_estimate(num_probes=num_probes, seed=seed)
        else:
            est, alpha, W, Z = model._lml_estimate(probes=probes)
        P, t = Y.shape[1], Z.shape[1]
        U = 0.5 * torch.cat([alpha, -(float(P) / t) * W], dim=1).contiguous()
        V = torch.cat([alpha, Z], dim=1).contiguous()
        ctx.spec, ctx.l_shape = kern.spec(X.shape[1]), lengthscales.shape
        ctx.save_for_backward(X, U, V)
        ctx.estimate = est
        return torch.tensor(est.value, dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        X, U, V = ctx.saved_tensors
        dvar, dls = ops.kxx_grad(ctx.spec, X, U, V)
        ds2 = float((U * V).sum())
        n_l = int(np.prod(ctx.l_shape)) if len(ctx.l_shape) else 1
        gl = torch.tensor(dls if n_l > 1 else [sum(dls)], dtype=torch.float64).reshape(ctx.l_shape)
        grads = (g * torch.tensor(dvar, dtype=torch.float64), g * gl, g * torch.tensor(ds2, dtype=torch.float64),
                 None, None, None, None, None, None, None, None, None)
        return grads[:len(ctx.needs_input_grad)]  # `num_probes`, `seed`, `fused_anyd`, `sym_anyd` are optional in apply()


class TrainableGPR:
    """Exact GP regression with trainable kernel and noise (the `paper_cli_gpr.py` flow: L-BFGS on the marginal
    likelihood).

    `num_probes=None` (default): `training_loss` is -log N(y | 0, K + s2 I) with K through `TrainableKernel.K`
    (`mgp_k_dense` forward, `mgp_k_dense_vjp` backward) and a torch Cholesky -- N x N memory.

    `num_probes=t`: matrix-free at any N.  The value is `GPR.log_marginal_likelihood_estimate` with t Rademacher
    probes (drawn once from `probe_seed`, fixed per model so repeated evaluations at one theta agree; `resample_probes`
    draws new ones), solved by `conjugate_gradient` (default `ConjugateGradient(1e-8)`, from zero: Lanczos needs
    x0 = 0, so there is no warm start).  With `ConjugateGradient(thr, preconditioner=PivotedCholeskyPreconditioner())`
    the solve is preconditioned and the probes are draws from N(0, P) re-formed from the current factor and the normals
    of `probe_seed`; a probe set assigned to `self.probes` by the caller is then taken as draws with E[z z^T] = P.
    The gradient comes from one `mgp_kxx_grad` call (`_GPRLmlEstimate`).  It is
    an unbiased estimate of the true gradient, NOT the exact derivative of the fixed-probe value, so an L-BFGS line
    search may see the two disagree: Adam is the tested optimiser here.

    `fused_anyd` (False, True or "auto"): the setting of the matrix-free estimate's `KxxNoiseOperator` and of the
    frozen model, as on `models.GPR`; the gradient call (`mgp_kxx_grad`) is not affected.  `sym_anyd` (False, True or
    "auto"): the same for `MGP_OP_KXX_NOISE_SYM_ANYD`, the symmetric operator above 32 dimensions."""

    def __init__(self, kernel, noise_variance, X, Y, *, num_probes=None, probe_seed=0, conjugate_gradient=None,
                 fused_anyd=False, sym_anyd=False):
        self.fused_anyd = check_fused_anyd(fused_anyd)  # the matrix-free estimate's operator and the frozen model's
        self.sym_anyd = check_sym_anyd(sym_anyd)
        self.kernel = TrainableKernel(kernel)
        self.likelihood_variance = Parameter(noise_variance)
        self.X, self.Y = X, Y
        self.num_probes = None if num_probes is None else int(num_probes)
        if self.num_probes is not None and self.num_probes < 1:
            raise ValueError("num_probes must be None or >= 1")
        self.probe_seed = int(probe_seed)
        self.conjugate_gradient = conjugate_gradient or ConjugateGradient(1e-8)
        self.probes = self._drawn_probes = None
        if self.num_probes is not None:
            self.resample_probes(self.probe_seed)

    def resample_probes(self, seed=None):
        """Draw a new fixed probe set [N, num_probes] (seeded CPU `torch.Generator`; `seed=None`: the next seed)."""
        if self.num_probes is None:
            raise ValueError("resample_probes needs num_probes")
        self.probe_seed = self.probe_seed + 1 if seed is None else int(seed)
        gen = torch.Generator().manual_seed(self.probe_seed)
        z = torch.randint(0, 2, (self.X.shape[0], self.num_probes), generator=gen, dtype=torch.int64) * 2 - 1
        self.probes = self._drawn_probes = z.to(device=self.X.device, dtype=self.X.dtype)
        return self.probes

    def parameters(self):
        return self.kernel.parameters() + [self.likelihood_variance.raw]

    def _sampled_probes(self):
        """True when the CG carries a `PivotedCholeskyPreconditioner` and no explicit probe set was installed
        (`self.probes` replaced by the caller): the probes are then sampled from N(0, P)."""
        from .conjugate_gradient import PivotedCholeskyPreconditioner
        return (isinstance(self.conjugate_gradient.preconditioner, PivotedCholeskyPreconditioner)
                and self.probes is self._drawn_probes)

    def log_marginal_likelihood(self, data=None):
        X, Y = (self.X, self.Y) if data is None else data
        N, P = Y.shape
        s2 = self.likelihood_variance()
        if self.num_probes is not None and self._sampled_probes():
            # probes from N(0, P): g1, g2 are drawn once per probe_seed and Z = L^T g1 + sigma g2 is re-formed from
            # the factor of the current theta, so repeated evaluations at one theta agree
            ls = self.kernel.lengthscales_p()
            if ls.dim() == 0:
                ls = ls.reshape(1)
            return _GPRLmlEstimate.apply(self.kernel.variance_p(), ls, s2, X.contiguous(), Y.contiguous(), None,
                                         self.kernel.name, self.conjugate_gradient, self.num_probes, self.probe_seed,
                                         self.fused_anyd, self.sym_anyd)
        if self.num_probes is not None:
            probes = self.probes if self.probes.shape[0] == N else None
            if probes is None:  # another row count than the model's own data: a draw of that size
                gen = torch.Generator().manual_seed(self.probe_seed)
                probes = (torch.randint(0, 2, (N, self.num_probes), generator=gen, dtype=torch.int64) * 2 - 1).to(
                    device=X.device, dtype=X.dtype)
            ls = self.kernel.lengthscales_p()
            if ls.dim() == 0:
                ls = ls.reshape(1)
            return _GPRLmlEstimate.apply(self.kernel.variance_p(), ls, s2, X.contiguous(), Y.contiguous(), probes,
                                         self.kernel.name, self.conjugate_gradient, None, 0, self.fused_anyd,
                                         self.sym_anyd)
        K = self.kernel.K(X) + s2.to(X.device) * torch.eye(N, dtype=X.dtype, device=X.device)
        L = torch.linalg.cholesky(K)
        v = torch.linalg.solve_triangular(L, Y, upper=False)
        return (-0.5 * N * P * math.log(2.0 * math.pi) - P * torch.log(L.diagonal()).sum()
                - 0.5 * (v * v).sum())

    def training_loss(self, data=None, probes=None):
        return -self.log_marginal_likelihood(data)

    def frozen_model(self, **gpr_kwargs):
        """The trained model as a `GPR`; `variance` / `variance_rank` are forwarded to it."""
        from .models import GPR
        unknown = set(gpr_kwargs) - {"variance", "variance_rank"}
        if unknown:
            raise TypeError(f"frozen_model() got unexpected keyword arguments {sorted(unknown)}")
        if self.num_probes is not None:
            return GPR((self.X, self.Y), self.kernel.frozen(), noise_variance=self.likelihood_variance.value,
                       conjugate_gradient=self.conjugate_gradient, solver="cg", fused_anyd=self.fused_anyd,
                       sym_anyd=self.sym_anyd, **gpr_kwargs)
        return GPR((self.X, self.Y), self.kernel.frozen(), noise_variance=self.likelihood_variance.value,
                   solver="cholesky", fused_anyd=self.fused_anyd, sym_anyd=self.sym_anyd, **gpr_kwargs)


def sgpr_bound(Kmm_j, Q, b, yy, s2, variance, N):
    """Titsias' collapsed bound (GPflow `SGPR.elbo`, as `models.SGPR.elbo` forms it) as a torch function of the [M, M]
    quantities: Kmm_j = k(Z, Z) + jitter I, Q = K_mn K_nm, b = K_mn y [M, 1], yy = y^T y, s2 the noise variance,
    `variance` the kernel variance (the trace term), N the number of data rows."""
    L = torch.linalg.cholesky(Kmm_j)
    T1 = torch.linalg.solve_triangular(L, Q, upper=False)
    AAT = torch.linalg.solve_triangular(L, T1.t(), upper=False) / s2  # A A^T = L^-1 Q L^-T / s2
    B = AAT + torch.eye(Q.shape[0], dtype=Q.dtype, device=Q.device)
    LB = torch.linalg.cholesky(B)
    Aerr = torch.linalg.solve_triangular(L, b, upper=False) / torch.sqrt(s2)
    c = torch.linalg.solve_triangular(LB, Aerr, upper=False) / torch.sqrt(s2)
    const = -0.5 * N * math.log(2.0 * math.pi)
    logdet = -torch.log(LB.diagonal()).sum() - 0.5 * N * torch.log(s2)
    quad = -0.5 * yy / s2 + 0.5 * (c * c).sum()
    trace = -0.5 * N * variance / s2 + 0.5 * AAT.diagonal().sum()
    return const + logdet + quad + trace


def sgpr_bound_adjoints(Kmm_j, Q, b, yy, s2, variance, N):
    """Value and adjoints of `sgpr_bound` (step 1 of the SGPR gradient: [M, M] work only, two Choleskys and triangular
    solves), by torch autograd on the device of the inputs: (value: float, Gq = dL/dQ, Gb = dL/db, G_Kmm = dL/dKmm_j,
    d_s2, d_variance) -- the last two the direct derivatives (floats).  Gq need not be symmetric."""
    dev, dt = Q.device, Q.dtype
    # leaves made here, not views of them: this also runs inside a backward pass, where grad mode is off
    as_t = lambda v: (v.detach().to(device=dev, dtype=dt) if isinstance(v, torch.Tensor)
                      else torch.tensor(float(v), dtype=dt, device=dev)).reshape(()).clone().requires_grad_(True)
    Kt, Qt, bt = (t.detach().clone().requires_grad_(True) for t in (Kmm_j, Q, b))
    s2t, vt = as_t(s2), as_t(variance)
    yyt = torch.as_tensor(float(yy), dtype=dt, device=dev)
    with torch.enable_grad():
        val = sgpr_bound(Kt, Qt, bt, yyt, s2t, vt, float(N))
        gK, gQ, gb, gs2, gv = torch.autograd.grad(val, [Kt, Qt, bt, s2t, vt])
    return float(val.detach()), gQ, gb, gK, float(gs2), float(gv)


def _profile_grad(name, r2):
    """df/dr2 of f = k / variance at the scaled squared distance (csrc/grad.hip's forms; Matern-1/2: 0 below GPflow's
    1e-36 floor)."""
    if name == "se":
        return -0.5 * torch.exp(-0.5 * r2)
    floor = ~(r2 > 1e-36)
    r = torch.sqrt(torch.where(floor, torch.full_like(r2, 1e-36), r2))
    zero = torch.zeros_like(r2)
    if name == "matern12":
        return torch.where(floor, zero, -torch.exp(-r) / (2.0 * r))
    if name == "matern32":
        s3 = math.sqrt(3.0)
        return torch.where(floor, zero, -1.5 * torch.exp(-s3 * r))
    s5 = math.sqrt(5.0)
    return torch.where(floor, zero, (-5.0 / 6.0) * (1.0 + s5 * r) * torch.exp(-s5 * r))


def kmm_grad_z(name, variance, lengthscales, Z, G, max_elems=1 << 24):
    """dL/dZ [M, D] through Kmm = k(Z, Z) (+ a constant jitter) given G = dL/dKmm: row i collects
    sum_j (G_ij + G_ji) dk(z_i, z_j)/dz_i, direct differences, rows in chunks of at most `max_elems` M D temporaries."""
    ls = torch.as_tensor(lengthscales, dtype=Z.dtype, device=Z.device).reshape(-1)
    A = Z / ls
    S = G + G.t()
    M, D = Z.shape
    out = torch.empty_like(Z)
    step = max(1, max_elems // max(1, M * D))
    for i0 in range(0, M, step):
        diff = A[i0:i0 + step, None, :] - A[None, :, :]
        fp = _profile_grad(name, (diff * diff).sum(dim=2))
        out[i0:i0 + step] = ((S[i0:i0 + step] * fp)[:, :, None] * diff).sum(dim=1)
    return out * (2.0 * float(variance) / ls)


def k_grad_points(name, variance, lengthscales, A, B, G, max_elems=1 << 24):
    """(dA [na, D], dB [nb, D]) through K = k(A, B) given a dense cotangent G = dL/dK [na, nb]:
    dA_i = sum_j G_ij dk(a_i, b_j)/da_i and dB_j = sum_i G_ij dk(a_i, b_j)/db_j, direct differences, any D, rows of A in
    chunks of at most `max_elems` temporaries.  For the dense blocks only (K_mn of a batch, K_mm of the dense model); at
    A = B = Z, dA + dB is `kmm_grad_z(Z, G)`."""
    ls = torch.as_tensor(lengthscales, dtype=A.dtype, device=A.device).reshape(-1)
    As, Bs = A.detach() / ls, B.detach() / ls
    (na, D), nb = As.shape, Bs.shape[0]
    dA, dB = torch.empty_like(As), torch.zeros_like(Bs)
    step = max(1, max_elems // max(1, nb * D))
    for i0 in range(0, na, step):
        diff = As[i0:i0 + step, None, :] - Bs[None, :, :]
        w = (G[i0:i0 + step] * _profile_grad(name, (diff * diff).sum(dim=2)))[:, :, None] * diff
        dA[i0:i0 + step] = w.sum(dim=1)
        dB -= w.sum(dim=0)
    scale = 2.0 * float(variance) / ls
    return dA * scale, dB * scale


class _SGPRElbo(torch.autograd.Function):
    """`models.SGPR.elbo` as an autograd node over (variance, lengthscales, s2, Kmm_j, Z).  Forward: Q by
    `mgp_kmn_knm`, b by `mgp_kmn_matvec`, y^T y, summed over ranks with `allreduce`, then `sgpr_bound`.  Backward:
    `sgpr_bound_adjoints`; the Kmm_j cotangent goes back to the caller (`TrainableKernel.K`, whose backward is
    `mgp_k_dense_vjp`) and, for a trainable Z, through `kmm_grad_z` -- or, when the model's `fused_point_grads` applies
    and Kmm_j came without a graph, both through one `mgp_k_dense_vjp_points` call here; the N-sized part is one
    `mgp_kmn_knm_vjp` call (`mgp_kmn_knm_vjp_anyd` above D = 32), and its [dvariance, dl, dZ] partials are summed over
    ranks by ONE all-reduce."""

    @staticmethod
    def forward(ctx, variance, lengthscales, s2, Kmm_j, Z, model, X, Y):
        D = X.shape[1]
        spec = ops.KernelSpec(model.kernel.name, float(variance), [float(v) for v in lengthscales.reshape(-1)], D)
        Zd = Z.detach()
        Q = ops.kmn_knm(spec, X, Zd)
        b = anyd_matvec(model.fused_anyd, "kmn", spec, X, Zd, Y)
        yy = ops.dot_all(Y, Y)
        if model.allreduce is not None:
            model.allreduce(Q.view(-1))
            model.allreduce(b.view(-1))
            t = torch.tensor([yy], dtype=torch.float64, device=X.device)
            model.allreduce(t)
            yy = t.item()
        dev = X.device
        s2d = s2.detach().to(device=dev, dtype=X.dtype)
        vd = variance.detach().to(device=dev, dtype=X.dtype)
        value = sgpr_bound(Kmm_j.detach(), Q, b, yy, s2d, vd, float(model.num_data))
        ctx.spec, ctx.model, ctx.yy = spec, model, yy
        ctx.v_shape, ctx.l_shape, ctx.s_shape = variance.shape, lengthscales.shape, s2.shape
        ctx.save_for_backward(Kmm_j.detach(), Q, b, s2d, vd, Zd, X, Y)
        return value.detach().cpu()

    @staticmethod
    def backward(ctx, g):
        Kmm_j, Q, b, s2d, vd, Zd, X, Y = ctx.saved_tensors
        model, spec = ctx.model, ctx.spec
        g = float(g)
        _, Gq, Gb, GK, ds2, dvar = sgpr_bound_adjoints(Kmm_j, Q, b, ctx.yy, s2d, vd, model.num_data)
        need_z = ctx.needs_input_grad[4]
        D, M = spec.D, Zd.shape[0]
        vjp = ops.kmn_knm_vjp_anyd if D > _hip.MGP_FUSED_MAX_D else ops.kmn_knm_vjp  # D <= 32 keeps its entry point
        nv, nl, nz = vjp(spec, X, Zd, Gq.contiguous(), Y, Gb.contiguous(), need_dZ=need_z)
        if model.allreduce is not None:  # this rank's rows only: one all-reduce of [dvariance, dl, dZ]
            parts = [torch.tensor([nv] + list(nl), dtype=torch.float64, device=X.device)]
            if need_z:
                parts.append(nz.reshape(-1))
            buf = torch.cat(parts)
            model.allreduce(buf)
            nv, nl = float(buf[0]), buf[1:1 + D].tolist()
            if need_z:
                nz = buf[1 + D:].reshape(M, D)
        kz = None
        if need_z and not ctx.needs_input_grad[3] and use_fused_point_grads(model.fused_point_grads, Zd, Zd):
            # `TrainableSGPR.elbo` handed over a K_mm block without a graph: its whole VJP is this one call on (Z, Z),
            # the hyper-parameter sums and both arguments of k(Z, Z) (the jitter is a constant)
            kv, kl, dA, dB = ops.k_dense_vjp_points(spec, Zd, Zd, GK)
            nv, nl, kz = nv + kv, [a + b for a, b in zip(nl, kl)], dA + dB
        gv = torch.tensor(g * (dvar + nv), dtype=torch.float64).reshape(ctx.v_shape)
        n_l = int(np.prod(ctx.l_shape)) if len(ctx.l_shape) else 1
        gl = torch.tensor([g * v for v in nl] if n_l > 1 else [g * sum(nl)], dtype=torch.float64).reshape(ctx.l_shape)
        gs = torch.tensor(g * ds2, dtype=torch.float64).reshape(ctx.s_shape)
        gZ = None
        if need_z:
            if kz is None:
                kz = kmm_grad_z(spec.kind, spec.variance, spec.lengthscales, Zd, GK)
            gZ = g * (nz + kz)
        return gv, gl, gs, g * GK, gZ, None, None, None


class TrainableSGPR:
    """SGPR (Titsias' collapsed bound, `models.SGPR`) with trainable kernel variance / lengthscales, noise variance
    and, with `trainable_inducing=True`, inducing inputs Z (the reference's `--tip`: `set_trainable(
    model.inducing_variable, tip)`, `paper_cli_geospatial.py:237`).  The model holds its data (`internal_data`):
    `train_using_adam_and_update` takes one full-data step per iteration (`cggp/optimize.py:215-216`).

    `elbo()` equals `models.SGPR(...).elbo()` at the same values and is an autograd node (`_SGPRElbo`) whose backward
    needs nothing N x M: one `mgp_kmn_knm_vjp` call for the N-sized part.  With `allreduce` (same contract as
    `models.SGPR`: X, Y are this rank's rows) the forward sums Q, K_mn y and y^T y over ranks and the backward makes one
    all-reduce of its N-sized partials, so every rank ends with the same gradient.  fp64, Y [N, 1]; any D <= 512: above
    D = 32 the N-sized part is `mgp_kmn_knm_vjp_anyd`, whose kernels stage the dimensions through LDS, and the
    constructor refuses X, Y, Z that are not on the GPU (ValueError).  `fused_anyd` (False, True or "auto"): the rule
    of the bound's `K_mn y` product and the setting of the frozen model, as on `models.SGPR`; `mgp_kmn_knm` and the VJP
    are not affected.  `fused_point_grads` (False, True or "auto"; default False): the K_mm block's setting -- with a
    trainable Z its whole VJP, the hyper-parameter sums and the gradient in Z, is then ONE `mgp_k_dense_vjp_points` call
    on (Z, Z) in place of `mgp_k_dense_vjp` + `kmm_grad_z` (always, or by the measured rule of
    `conjugate_gradient.fused_point_grads_auto`); with a frozen Z, or with host tensors, nothing changes."""

    num_probes = None
    internal_data = True

    def __init__(self, kernel, noise_variance, X, Y, Z, *, jitter=1e-6, trainable_inducing=False, allreduce=None,
                 num_data=None, conjugate_gradient=None, fused_anyd=False, fused_point_grads=False):
        self.fused_anyd = check_fused_anyd(fused_anyd)  # K_mn y of the bound, and the frozen model's sweeps
        self.fused_point_grads = check_fused_point_grads(fused_point_grads)  # the K_mm block's gradient in Z
        for name, t in (("X", X), ("Y", Y), ("Z", Z)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"TrainableSGPR needs fp64 tensors: {name} is "
                                 f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if X.dim() != 2 or Z.dim() != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError(f"X [N, D] and Z [M, D] expected, got {tuple(X.shape)} and {tuple(Z.shape)}")
        if X.shape[1] > _hip.MGP_MAX_D:
            raise ValueError(f"TrainableSGPR needs D <= {_hip.MGP_MAX_D}, got D={X.shape[1]}")
        if X.shape[1] > _hip.MGP_FUSED_MAX_D and not (X.is_cuda and Y.is_cuda and Z.is_cuda):
            # above the fused kernels' D the model is refused here when it cannot run, not at its first backward:
            # every kernel of the any-D route is device code and there is no host path
            raise ValueError(f"TrainableSGPR at D={X.shape[1]} > {_hip.MGP_FUSED_MAX_D} needs X, Y and Z on the GPU")
        if Y.dim() != 2 or Y.shape != (X.shape[0], 1):
            raise ValueError(f"Y must be [N={X.shape[0]}, 1], got {tuple(Y.shape)}")
        self.kernel = kernel if isinstance(kernel, TrainableKernel) else TrainableKernel(kernel)
        self.noise_p = Parameter(noise_variance)
        self.X, self.Y = X.contiguous(), Y.contiguous()
        self.trainable_inducing = bool(trainable_inducing)
        self.Z = Z.detach().clone().contiguous().requires_grad_(self.trainable_inducing)
        self.jitter = float(jitter)
        self.allreduce = allreduce
        if num_data is None:  # global row count, as models.SGPR agrees it
            num_data = self.X.shape[0]
            if allreduce is not None:
                t = torch.tensor([float(num_data)], dtype=torch.float64, device=self.X.device)
                allreduce(t)
                num_data = int(round(t.item()))
        self.num_data = int(num_data)
        self.conjugate_gradient = conjugate_gradient or ConjugateGradient(1e-6)

    def parameters(self):
        ps = self.kernel.parameters() + [self.noise_p.raw]
        return ps + [self.Z] if self.trainable_inducing else ps

    def elbo(self, data=None):
        X, Y = (self.X, self.Y) if data is None else (data[0].contiguous(), data[1].contiguous())
        ls = self.kernel.lengthscales_p()
        if ls.dim() == 0:
            ls = ls.reshape(1)
        Zd = self.Z.detach()
        if self.trainable_inducing and use_fused_point_grads(self.fused_point_grads, Zd, Zd):
            with torch.no_grad():  # the same forward call; `_SGPRElbo.backward` takes the block's whole VJP in one call
                Kmm_j = self.kernel.K(Zd, jitter=self.jitter)
        else:
            Kmm_j = self.kernel.K(Zd, jitter=self.jitter)
        return _SGPRElbo.apply(self.kernel.variance_p(), ls, self.noise_p(), Kmm_j, self.Z, self, X, Y)

    def training_loss(self, data=None, probes=None):
        return -self.elbo(data)

    def frozen_model(self):
        from .models import SGPR
        return SGPR((self.X, self.Y), self.kernel.frozen(), self.Z.detach().clone(), self.noise_p.value,
                    self.conjugate_gradient, jitter=self.jitter, allreduce=self.allreduce, num_data=self.num_data,
                    fused_anyd=self.fused_anyd)


def train_using_adam_and_update(data, model, iterations, batch_size, learning_rate, update_fn=None,
                                update_during_training=None, monitor=None, seed=0):
    """`cggp/optimize.py:198-254`: shuffled minibatches, one Adam step per iteration, optional
    inducing-parameter update after each step, monitor callback per iteration.  A model with `internal_data` (SGPR)
    takes one full-data `training_loss()` per step instead (`:215-216`); `data` and `batch_size` are then unused."""
    # models that hold their data (SGPR) take one full-data step per iteration, no minibatch draw (:215-216)
    internal = getattr(model, "internal_data", False)
    if not internal:
        x, y = data
        n = x.shape[0]
        gen = torch.Generator().manual_seed(seed)
    opt = torch.optim.Adam(model.parameters(), lr=learning_rate)
    update_during_training = update_during_training and (update_fn is not None)

    if update_fn is not None:
        update_fn()
    if monitor is not None:
        monitor(0)
    if not internal:
        perm, pos = torch.randperm(n, generator=gen), 0
    losses = []
    for iteration in range(iterations):
        opt.zero_grad()
        if internal:
            loss = model.training_loss()
            loss.backward()
            opt.step()
            losses.append(float(loss))
            if update_during_training:
                update_fn()
            if monitor is not None:
                monitor(iteration)
            continue
        if pos + batch_size > n:
            perm, pos = torch.randperm(n, generator=gen), 0
        idx = perm[pos:pos + batch_size].to(x.device)
        pos += batch_size
        loss = model.training_loss((x[idx], y[idx]))
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if update_during_training:
            update_fn()
        if monitor is not None:
            monitor(iteration)
    return losses


def train_using_lbfgs_and_update(data, model, max_num_iters, update_fn=None, update_during_training=None,
                                 monitor=None, probe_seed=0):
    """`cggp/optimize.py:152-195`: full-batch L-BFGS (scipy `L-BFGS-B`, what `gpflow.optimizers.Scipy`
    drives) over the model's trainable parameters; `update_fn` / `monitor` are called before the
    first step and after every accepted step, as the reference's `step_callback`.

    L-BFGS needs a deterministic objective, so when the model estimates the trace / log-det terms
    with Hutchinson probes the SAME probes (drawn once from `probe_seed`) are used for every
    evaluation; a `data_term="pathwise"` model's draw (from its `pathwise_seed`) is held in the same way.
    Returns scipy's `OptimizeResult` (None when `max_num_iters` is 0, as upstream)."""
    from scipy.optimize import minimize

    params = model.parameters()
    sizes = [p.numel() for p in params]
    x, y = data
    probes = None
    if model.num_probes is not None and hasattr(model, "Z"):  # TrainableGPR keeps its own fixed probes
        probes = rademacher((model.Z.shape[0], model.num_probes), model.Z.dtype, model.Z.device, probe_seed)
    held = {}
    if getattr(model, "data_term", None) == "pathwise":  # and ONE draw of the bases, weights and noise
        held["pathwise"] = model.draw_pathwise(model.pathwise_seed)
        model.pathwise_seed += 1

    def assign(flat):
        off = 0
        with torch.no_grad():
            for p, n in zip(params, sizes):
                p.copy_(torch.from_numpy(flat[off:off + n].copy()).reshape(p.shape))
                off += n

    def value_and_grad(flat):
        assign(flat)
        for p in params:
            p.grad = None
        loss = model.training_loss((x, y), probes=probes, **held)
        loss.backward()
        g = np.concatenate([p.grad.detach().cpu().numpy().reshape(-1) for p in params])
        return float(loss), g.astype(np.float64)

    state = {"iteration": 0}

    def internal_update_fn(iteration):
        if update_during_training and (update_fn is not None):
            update_fn()
        if monitor is not None:
            monitor(iteration)

    def callback(_xk):
        state["iteration"] += 1
        internal_update_fn(state["iteration"])

    internal_update_fn(0)
    if max_num_iters > 0:
        x0 = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in params]).astype(np.float64)
        result = minimize(value_and_grad, x0, jac=True, method="L-BFGS-B", callback=callback,
                          options=dict(maxiter=int(max_num_iters)))
        assign(result.x)
        return result
    internal_update_fn(-1)
    if monitor is not None and hasattr(monitor, "close"):
        monitor.close()
    return None


def train_vanilla_using_lbfgs(data, model, clustering_fn, max_num_iters, probe_seed=0):
    """`cggp/optimize.py:127-150`: full-batch L-BFGS over the model's trainable parameters, no inducing-point
    update (`clustering_fn` is accepted and unused, as upstream)."""
    return train_using_lbfgs_and_update(data, model, max_num_iters, update_fn=None, update_during_training=False,
                                        probe_seed=probe_seed)


def train_vanilla_using_lbfgs_and_standard_ip_update(data, model, clustering_fn, max_num_iters, probe_seed=0):
    """`cggp/optimize.py:101-124`: as above, with `model.Z <- clustering_fn()` after every L-BFGS step (the
    reference's own comment notes that this converges to poor minima; kept for call compatibility)."""
    def update_fn():
        model.Z = clustering_fn().to(model.Z.dtype)

    return train_using_lbfgs_and_update(data, model, max_num_iters, update_fn=update_fn, update_during_training=True,
                                        probe_seed=probe_seed)
