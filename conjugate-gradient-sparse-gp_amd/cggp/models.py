"""Model surface of the hot path -- host mirror of `cggp/models.py` (rows M1-M6, S1).

`CGGP` (the CDGP model: every (Kmm+Lambda)^-1 applied by CG), its Cholesky twin `ClusterGP`,
`eval_logdet`, and a CG form of SGPR.  Names, constructor keywords, method signatures and
returned shapes follow the reference (`cggp/models.py:21-48,176-354`, `cggp/cli_utils.py:439-446`);
`GPR` is the exact regression baseline the reference takes from GPflow (`gpr_class`, `cggp/cli_utils.py:449-452`);
kernel evaluation, the K_nm products, the dense `p @ A` and the CG loop run in libmgp.
"""

import math
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .conjugate_gradient import (ConjugateGradient, KmmLambdaOperator, KxxNoiseOperator, PivotedCholeskyPreconditioner,
                                 SgprNormalOperator, SubsampledNormalPreconditioner, anyd_matvec, check_fused_anyd,
                                 check_fused_variance, check_sym_anyd, check_wide, use_fused_variance)
from .kernels import InducingPoints, Kuf, Kuu, inducingpoint_wrapper  # noqa: F401 (InducingPoints re-exported)
from .likelihoods import Gaussian
from .slq import slq_log_quadratic


def rademacher(shape, dtype, device, seed):
    """+-1 probes from a documented stream: numpy PCG64(seed), `2*integers(0,2)-1`.

    The reference draws them with `tfp.random.rademacher` (`cggp/models.py:39,310`), whose
    stream cannot be reproduced outside TFP, so parity tests inject `probes=`.
    """
    z = 2 * np.random.default_rng(seed).integers(0, 2, size=shape) - 1
    return torch.from_numpy(z.astype(np.float64)).to(device=device, dtype=dtype)


DATA_TERMS = ("batch", "trace", "pathwise")


def check_data_term(data_term, dtype, D, trainable_inducing=False):
    """The constructor checks of `data_term`, shared by `CGGP` and `training.TrainableCGGP`."""
    if data_term not in DATA_TERMS:
        raise ValueError(f"data_term must be one of {DATA_TERMS}, got {data_term!r}")
    if data_term != "batch":
        if dtype != torch.float64:
            raise ValueError(f'data_term="{data_term}" is fp64 only, got {dtype}')
        if trainable_inducing and D > 32:
            raise ValueError(f'data_term="{data_term}" with trainable_inducing=True needs D <= 32, got D={D}')
    return data_term


def check_pathwise(num_bases, num_samples, epsilon):
    """The constructor checks of the `data_term="pathwise"` arguments, shared like `check_data_term`."""
    if int(num_bases) != num_bases or num_bases < 1:
        raise ValueError(f"num_bases must be a positive integer, got {num_bases!r}")
    if int(num_samples) != num_samples or num_samples < 1:
        raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
    if epsilon not in ("reference", "matheron"):
        raise ValueError(f"epsilon must be one of ('reference', 'matheron'), got {epsilon!r}")
    return int(num_bases), int(num_samples), epsilon


def draw_pathwise(kernel_name, D, M, num_bases, num_samples, seed):
    """(E [L, D], W [S, 2L], xi [S, M]) float64 CPU tensors, the draws of one `data_term="pathwise"` evaluation, in the
    stream order of `PathwiseClusterGP.pathwise_samples` (numpy PCG64 from `seed`: bases, weights, noise).  E is the
    base draw of the frequencies at unit lengthscales, Matern factor sqrt(nu / chi2) included
    (`rff.basis_theta_parameter`): theta = E / lengthscales is the reparameterisation the bound differentiates."""
    from . import kernels, rff
    cls = {"se": kernels.SquaredExponential, "matern12": kernels.Matern12, "matern32": kernels.Matern32,
           "matern52": kernels.Matern52}[kernel_name]
    rng = np.random.default_rng(seed)
    E = rff.basis_theta_parameter(cls(variance=1.0, lengthscales=[1.0] * int(D)), num_bases, rng, dim=int(D))
    W = rff.rff_weights(num_samples, num_bases, rng)
    xi = torch.from_numpy(rng.standard_normal((int(num_samples), int(M))))
    return E, W, xi


class _EvalLogdet(torch.autograd.Function):
    """`eval_logdet` custom gradient (`cggp/models.py:26-46`): forward 0.0, backward
    df * CG(K, I)^T (exact) or CG(K, Zp) (df Zp)^T / P (probes)."""

    @staticmethod
    def forward(ctx, matrix, cg, num_probes, probes):
        ctx.cg, ctx.num_probes, ctx.probes = cg, num_probes, probes
        ctx.save_for_backward(matrix)
        return torch.zeros((), dtype=matrix.dtype, device=matrix.device)  # :46

    @staticmethod
    def backward(ctx, df):
        (matrix,) = ctx.saved_tensors
        with torch.no_grad():
            grad = eval_logdet_grad(matrix, ctx.cg, df, ctx.num_probes, ctx.probes)
        return grad, None, None, None


def eval_logdet_grad(matrix, cg, df=1.0, num_probes=None, probes=None, seed=0):
    """The backward of `eval_logdet` as a plain function (`cggp/models.py:30-44`)."""
    n = matrix.shape[-1]
    if num_probes is None and probes is None:
        eye = torch.eye(n, dtype=matrix.dtype, device=matrix.device)  # :33
        inv = cg(matrix, eye)  # :34
        return df * inv.t()  # :35-36
    if probes is None:
        probes = rademacher((n, num_probes), matrix.dtype, matrix.device, seed)  # :38-39
    P = probes.shape[1]
    rv = df * probes  # :40
    lv = cg(matrix, probes)  # :41
    return (lv @ rv.t()) / P  # :42  ([n,P]x[P,n] rank-P library GEMM)


def eval_logdet(matrix, cg, num_probes=None, probes=None):
    """`cggp/models.py:21-48`: value is the constant 0.0, only the gradient carries log|K|."""
    return _EvalLogdet.apply(matrix, cg, num_probes, probes)


class LpSVGP:
    """`cggp/models.py:51-173` (Panos et al. SVGP with diagonal q-covariance): parameters `nu [M,1]`
    and `diag_variance [M,1]`; Cholesky solves on the [M,M] matrix libmgp builds.  The base of the
    reference's class tree; `ClusterGP` replaces `nu`/`diag_variance` by pseudo_u and sigma^2/counts."""

    def __init__(self, kernel, likelihood, inducing_variable, *, mean_function=None, num_latent_gps=1, nu=None,
                 diag_variance=None, num_data=None):
        assert num_latent_gps == 1, "One latent GP is allowed"  # :76
        self.kernel = kernel
        self.likelihood = likelihood if not isinstance(likelihood, (int, float)) else Gaussian(likelihood)
        self.inducing_variable = inducingpoint_wrapper(inducing_variable)
        self.mean_function = mean_function
        self.num_data = num_data
        Z = self.inducing_variable.Z
        shape = (Z.shape[0], 1)
        self.nu = (torch.zeros(shape, dtype=Z.dtype, device=Z.device) if nu is None  # :93
                   else torch.as_tensor(nu, dtype=Z.dtype, device=Z.device).reshape(shape).clone())
        self.diag_variance = (torch.full(shape, 1e-4, dtype=Z.dtype, device=Z.device) if diag_variance is None  # :94
                              else torch.as_tensor(diag_variance, dtype=Z.dtype, device=Z.device).reshape(shape).clone())

    def _mean(self, Xnew):
        return 0.0 if self.mean_function is None else self.mean_function(Xnew)

    def _K(self):
        Kmm = Kuu(self.inducing_variable, self.kernel, jitter=0.0)  # :112 / :141
        return Kmm, Kuu(self.inducing_variable, self.kernel, jitter=0.0, diag_add=self.diag_variance[:, 0])

    def prior_kl(self):  # :107-120
        Kmm, K = self._K()
        nut = self.nu.t().contiguous()
        quad = ops.dot_all(ops.symm_matmul(Kmm, nut), nut)
        L = torch.linalg.cholesky(K)
        trace = torch.cholesky_solve(Kmm, L).diagonal().sum().item()
        logdet = (2.0 * torch.log(L.diagonal())).sum().item() - torch.log(self.diag_variance).sum().item()
        return 0.5 * (quad - trace + logdet)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):  # :136-161
        assert not full_output_cov
        _, K = self._K()
        Kmn = Kuf(self.inducing_variable, self.kernel, Xnew)
        L = torch.linalg.cholesky(K)
        A = torch.linalg.solve_triangular(L, Kmn, upper=False)
        if not full_cov:
            fvar = (self.kernel.K_diag(Xnew) - ops.colwise_dot(A, A))[:, None]
        else:
            fvar = (self.kernel.K(Xnew) - A.t() @ A)[None, ...]
        fmu = ops.knm_matvec(self.kernel.spec(Xnew.shape[1]), Xnew, self.inducing_variable.Z, self.nu)  # :157
        return fmu + self._mean(Xnew), fvar

    def scale(self, batch_size, dtype=None):  # :163-169
        return 1.0 if self.num_data is None else float(self.num_data) / float(batch_size)

    def elbo(self, data):  # :125-134
        x, y = data
        kl = self.prior_kl()
        f_mean, f_var = self.predict_f(x)
        var_exp = self.likelihood.variational_expectations(x, f_mean, f_var, y)
        return var_exp.sum().item() * self.scale(x.shape[0]) - kl

    def maximum_log_likelihood_objective(self, data):  # :122-123
        return self.elbo(data)

    def q_moments(self, full_cov=False):  # :171-173
        return self.predict_f(self.inducing_variable.Z, full_cov=full_cov)


class ClusterGP:
    """Cluster-data GP with Cholesky solves (`cggp/models.py:176-276`); parameter container of
    row M6.  The Cholesky factorisation itself is a plain library call (torch.linalg) on the
    [M,M] matrix libmgp builds; it is the twin the CG model is checked against."""

    def __init__(self, kernel, likelihood, inducing_variable, *, mean_function=None, num_latent_gps=1,
                 cluster_counts=None, num_data=None, pseudo_u=None):
        assert num_latent_gps == 1, "One latent GP is allowed"  # :189
        self.kernel = kernel
        self.likelihood = likelihood if not isinstance(likelihood, (int, float)) else Gaussian(likelihood)
        self.inducing_variable = inducingpoint_wrapper(inducing_variable)
        self.mean_function = mean_function
        self.num_latent_gps = num_latent_gps
        self.num_data = num_data
        Z = self.inducing_variable.Z
        M = Z.shape[0]
        shape = (M, num_latent_gps)
        if pseudo_u is not None:
            pseudo_u = torch.as_tensor(pseudo_u, dtype=Z.dtype, device=Z.device)
            if tuple(pseudo_u.shape) != shape:  # :204-205
                raise ValueError("Pseudo-u argument shape must match actual pseudo-u shape.")
            self.pseudo_u = pseudo_u.clone()
        else:
            self.pseudo_u = torch.zeros(shape, dtype=Z.dtype, device=Z.device)  # nu = 0, :93
        if cluster_counts is not None:
            cluster_counts = torch.as_tensor(cluster_counts, dtype=Z.dtype, device=Z.device)
            if tuple(cluster_counts.shape) != shape:  # :209-210
                raise ValueError("Cluster counts argument shape must match pseudo-u shape.")
            self.cluster_counts = cluster_counts.clone()
        else:
            self.cluster_counts = torch.ones(shape, dtype=Z.dtype, device=Z.device)  # :213

    # ---- parameters
    @property
    def nu(self):  # :222-224
        raise NotImplementedError(f"This property is not supported in {self.__class__}")

    @property
    def diag_variance(self):  # :226-228
        return self.likelihood.variance / self.cluster_counts

    def _mean(self, Xnew):
        if self.mean_function is None:
            return 0.0
        return self.mean_function(Xnew)

    def _Kmm_and_KmmLambda(self):
        iv, kernel = self.inducing_variable, self.kernel
        Kmm = Kuu(iv, kernel, jitter=0.0)  # :236 / :300
        KmmLambda = Kuu(iv, kernel, jitter=0.0, diag_add=self.diag_variance[:, 0])  # add_diagonal fused
        return Kmm, KmmLambda

    # ---- Cholesky versions
    def prior_kl(self):  # :230-248
        Kmm, K = self._Kmm_and_KmmLambda()
        L = torch.linalg.cholesky(K)
        a = torch.cholesky_solve(self.pseudo_u, L)
        quad = ops.dot_all(ops.symm_matmul(Kmm, a.t().contiguous()), a.t().contiguous())
        trace = torch.cholesky_solve(Kmm, L).diagonal().sum().item()
        logdet = (2.0 * torch.log(L.diagonal())).sum().item()
        const = torch.log(self.diag_variance).sum().item()
        return 0.5 * (quad - trace + logdet - const)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):  # :250-276
        assert not full_output_cov
        iv, kernel = self.inducing_variable, self.kernel
        _, K = self._Kmm_and_KmmLambda()
        Kmn = Kuf(iv, kernel, Xnew)
        L = torch.linalg.cholesky(K)
        a = torch.cholesky_solve(self.pseudo_u, L)
        A = torch.linalg.solve_triangular(L, Kmn, upper=False)
        if not full_cov:
            fvar = (kernel.K_diag(Xnew) - ops.colwise_dot(A, A))[:, None]
        else:
            fvar = (kernel.K(Xnew) - A.t() @ A)[None, ...]
        fmu = ops.knm_matvec(kernel.spec(Xnew.shape[1]), Xnew, iv.Z, a)
        return fmu + self._mean(Xnew), fvar

    # ---- shared by both
    def scale(self, batch_size, dtype=None):  # :163-169
        if self.num_data is not None:
            return float(self.num_data) / float(batch_size)
        return 1.0

    def elbo(self, data):  # :125-134
        x, y = data
        kl = self.prior_kl()
        f_mean, f_var = self.predict_f(x, full_cov=False, full_output_cov=False)
        var_exp = self.likelihood.variational_expectations(x, f_mean, f_var, y)
        return var_exp.sum().item() * self.scale(x.shape[0]) - kl

    def maximum_log_likelihood_objective(self, data):  # :122-123
        return self.elbo(data)

    def training_loss(self, data):
        return -self.elbo(data)

    def q_moments(self, full_cov=False):  # :171-173
        return self.predict_f(self.inducing_variable.Z, full_cov=full_cov)

    def predict_f_batched(self, X, batch_size):
        """`batch_posterior_computation` (`cggp/cli_utils.py:426-436`): stream rows in batches."""
        means, variances = [], []
        for s in range(0, X.shape[0], batch_size):
            mu, var = self.predict_f(X[s:s + batch_size])
            means.append(mu)
            variances.append(var)
        return torch.cat(means, 0), torch.cat(variances, 0)


class CGGP(ClusterGP):
    """`cggp/models.py:279-354`.

    `matrix_free=True`: nothing [M, M] is allocated by any method.  Every solve takes the operator
    `KmmLambdaOperator(kernel, Z, diag_variance)` (libmgp applies it by the fused sweep, 8 columns per launch; DESIGN
    4.15) and every product with K_mm is `ops.knm_matvec(spec, Z, Z, .)`; `K_mn [M, B]` of one batch stays dense, as
    the reference holds it.  What returns or needs an [M, M] array is refused with `ValueError`: the exact trace of
    `prior_kl` (`num_probes=None` without `probes`: M right-hand sides), `shared_inverse=True` (the explicit inverse)
    and `logdet_gradient()` (dL/dK itself).

    `wide_solves` (with `matrix_free=True` only; anything but False without it is a `ValueError`) is the `wide`
    argument of every `KmmLambdaOperator` the model makes: False the sweep form, True libmgp's many-column form
    (each kernel value evaluated once per 256 columns and contracted on the fp64 matrix cores: the form for
    `W = CG(K_mm + Lambda, K_mn)`, one column per test row), "auto" the many-column form from
    `conjugate_gradient.WIDE_MIN_COLUMNS` columns and `WIDE_MIN_M` inducing points on.

    `fused_anyd` (False, True or "auto"; with `matrix_free=True` only, anything but False without it is a `ValueError`)
    is the `fused_anyd` argument of every `KmmLambdaOperator` the model makes and the rule of its own K(Z, Z) and
    K(X*, Z) products: at D > 32 in fp64 libmgp's fused any-D sweeps (include/mgp_sweep_anyd.h) instead of kernel
    panels; "auto" follows `conjugate_gradient.fused_anyd_auto`.

    `wide_anyd` (False, True or "auto"; with `matrix_free=True` only, anything but False without it is a `ValueError`)
    is the `wide_anyd` argument of every `KmmLambdaOperator` the model makes: at D > 32 in fp64 the many-column form
    `MGP_OP_KMM_LAMBDA_WIDE_ANYD` (what `wide_solves` is at D <= 32) for `W = CG(K_mm + Lambda, K_mn)`; "auto" follows
    `conjugate_gradient.wide_anyd_auto`.

    `data_term` ("batch", the default and the reference's form, or "trace"; fp64 only) is what `elbo(data)` does with
    the rows of `data`.  "batch" solves `W = CG(K_mm + Lambda, K_mn)` with one column per row to sum the diagonal of
    `K_nm W`.  "trace" takes that sum as a trace, `B variance - tr(A^-1 K_mn K_nm)`, and estimates it with the probes
    of the KL term: `(1/P) sum_p (K_nm s_p) . (K_nm z_p)` with `s_p = A^-1 z_p` the solves `prior_kl` makes anyway, so
    every solve has `1 + P` columns and the rows of `data` enter through one `mgp_knm_matvec` pass on `[a | S | Zp]`;
    nothing [M, B] is formed, for a minibatch or the whole data set.  With `num_probes=None` and no
    `probes` the dense model takes the exact trace from `Q = K_mn K_nm` (`mgp_kmn_knm`) and one M-column solve; the
    matrix-free model refuses that, as above.  "pathwise" takes the likelihood term from `num_samples` pathwise
    posterior samples on `num_bases` random Fourier features, `-(1/2) [sum_sn (y_n - f_sn)^2 / (S s2) + B log(2 pi s2)]`
    (`PathwiseClusterGP`'s estimator with the model's CG and its KL term): one S-column solve whatever B is,
    never negative in its quadratic part, and with `epsilon="matheron"` (the default here; "reference" as in
    `pathwise_epsilon`) its expectation is the "batch" data term up to the random-feature truncation.  The draws come
    from `pathwise_seed`, which advances per call, or are injected as `elbo(data, pathwise=(E, W, xi))`
    (`draw_pathwise`).  Value only: `training.TrainableCGGP` is the differentiable form.

    `rff_anyd` (False, True or "auto"; with `data_term="pathwise"` only, anything but False with another data term is a
    `ValueError`): the prior draw at D > 32 in fp64 by libmgp's fused any-D kernels (MGP_RFF_ANYD,
    include/mgp_pathwise.h) instead of feature panels; "auto" follows `rff.rff_anyd_auto`."""

    def __init__(self, kernel, likelihood, inducing_variable, conjugate_gradient, num_probes=5, matrix_free=False,
                 wide_solves=False, data_term="batch", num_bases=1024, num_samples=5, epsilon="matheron",
                 fused_anyd=False, wide_anyd=False, rff_anyd=False, **kwargs):
        from .rff import check_rff_anyd
        self.rff_anyd = check_rff_anyd(rff_anyd)
        if self.rff_anyd is not False and data_term != "pathwise":
            raise ValueError(f"rff_anyd needs data_term='pathwise': no other data term draws random Fourier features "
                             f"(got data_term={data_term!r})")
        self.wide_solves = check_wide(wide_solves, "wide_solves")
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.wide_anyd = check_wide(wide_anyd, "wide_anyd")
        if self.wide_anyd is not False and not matrix_free:
            raise ValueError("wide_anyd needs matrix_free=True: without it there is no operator to widen")
        if self.fused_anyd is not False and not matrix_free:
            raise ValueError("fused_anyd needs matrix_free=True: without it K_mm is a dense matrix and no sweep runs")
        if self.wide_solves is not False and not matrix_free:
            raise ValueError("wide_solves needs matrix_free=True: without it there is no operator to widen")
        super().__init__(kernel, likelihood, inducing_variable, **kwargs)
        Z = self.inducing_variable.Z
        self.data_term = check_data_term(data_term, Z.dtype, Z.shape[1])
        self.num_bases, self.num_samples, self.epsilon = check_pathwise(num_bases, num_samples, epsilon)
        self.pathwise_seed = 0
        self.conjugate_gradient = conjugate_gradient
        self.num_probes = num_probes
        self.probe_seed = 0
        self.matrix_free = bool(matrix_free)

    def _system(self):
        """(K_mm or None, what the CG solves on, R [r, M] -> R K_mm): the two dense matrices and `ops.symm_matmul`, or
        with `matrix_free` the operator and the K(Z, Z) sweep."""
        if not self.matrix_free:
            Kmm, KmmLambda = self._Kmm_and_KmmLambda()  # :300-301
            return Kmm, KmmLambda, lambda R: ops.symm_matmul(Kmm, R)
        Z = self.inducing_variable.Z
        spec = self.kernel.spec(Z.shape[1])
        op = KmmLambdaOperator(self.kernel, Z, self.diag_variance[:, 0].contiguous(), wide=self.wide_solves,
                               fused_anyd=self.fused_anyd, wide_anyd=self.wide_anyd)
        return None, op, lambda R: anyd_matvec(self.fused_anyd, "knm", spec, Z, Z, R, ops.ROWS, ops.ROWS)

    def prior_kl(self, probes=None):  # :293-322
        if self.matrix_free and self.num_probes is None and probes is None:
            raise ValueError("matrix_free=True needs num_probes (or probes=): the exact trace solves M right-hand sides")
        Kmm, KmmLambda, times_kmm = self._system()
        cg = self.conjugate_gradient
        a = cg(KmmLambda, self.pseudo_u)  # :303
        if self.num_probes is None and probes is None:
            trace = cg(KmmLambda, Kmm).diagonal().sum().item()  # :305-306
        else:
            if probes is None:
                Z = self.inducing_variable.Z
                probes = rademacher((Z.shape[0], self.num_probes), Z.dtype, Z.device, self.probe_seed)
                self.probe_seed += 1
            S = cg(KmmLambda, probes)  # :311
            Kp = times_kmm(probes.t().contiguous())  # (Kmm Zp)^T, :312
            trace = ops.dot_all(S.t().contiguous(), Kp) / probes.shape[1]  # :313-314
        at = a.t().contiguous()
        quad = ops.dot_all(times_kmm(at), at)  # :316-317
        logdet = 0.0  # eval_logdet forward value, :319 -> :46
        const = torch.log(self.diag_variance).sum().item()  # :321
        return 0.5 * (quad - trace + logdet - const)  # :322

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False, _shared=None):  # :324-354
        assert not full_output_cov
        iv, kernel = self.inducing_variable, self.kernel
        cg = self.conjugate_gradient
        if _shared is None:
            _, KmmLambda, _ = self._system()  # :333,337
            a = cg(KmmLambda, self.pseudo_u)  # :339
        else:  # predict_f_batched: the N-free pieces are the same for every batch
            KmmLambda, a = _shared
        Kmn = Kuf(iv, kernel, Xnew)  # :334
        W = cg(KmmLambda, Kmn)  # :340
        if not full_cov:
            fvar = (kernel.K_diag(Xnew) - ops.colwise_dot(Kmn, W))[:, None]  # :343-345
        else:
            fvar = (kernel.K(Xnew) - Kmn.t() @ W)[None, ...]  # :347-349
        fmu = anyd_matvec(self.fused_anyd, "knm", kernel.spec(Xnew.shape[1]), Xnew, iv.Z, a)  # Kmn^T a, :351 (row M1)
        return fmu + self._mean(Xnew), fvar

    def predict_f_batched(self, X, batch_size, shared_inverse=False, inverse_threshold=None, fused_variance=False):
        """`batch_posterior_computation` (`cggp/cli_utils.py:426-436`); (Kmm+Lambda) and its solve
        against pseudo_u do not depend on the batch and are formed once.

        `shared_inverse=True` (build-side option for predicting many rows): instead of one
        B-column CG per batch -- iterations x 2 B M^2 flops each, the dominant cost of the reference's
        prediction -- solve (Kmm+Lambda) Y = I ONCE with the same device CG
        (M right-hand sides) and apply Y to every batch as one GEMM.  For N rows that is
        `iterations x 2 M^3 + 2 N M^2` flops instead of `iterations x 2 N M^2`.  The columns of I are
        solved to `inverse_threshold` (default: the model's threshold squared, so that the product
        with a batch stays inside the per-batch solve's own tolerance).

        `fused_variance` (False, True or "auto"; with `shared_inverse=True` only): True forms the variance term
        k(x, Z) Y k(Z, x) of each batch by one `ops.knm_quadform` (include/mgp_predict.h) -- no [B, M] kernel panel, half
        the matrix-core work -- instead of `ops.k_dense`, `ops.symm_matmul` and a row sum; False is that composition,
        bit for bit what this method computed before the option existed; "auto" follows
        `conjugate_gradient.fused_variance_auto`."""
        check_fused_variance(fused_variance)
        if shared_inverse and self.matrix_free:
            raise ValueError("shared_inverse=True forms the [M, M] inverse; matrix_free=True refuses it "
                             "(pass shared_inverse=False)")
        if fused_variance is True and not shared_inverse:
            raise ValueError("fused_variance=True applies the shared [M, M] inverse: pass shared_inverse=True")
        _, KmmLambda, _ = self._system()
        cg = self.conjugate_gradient
        a = cg(KmmLambda, self.pseudo_u)
        means, variances = [], []
        if not shared_inverse:
            shared = (KmmLambda, a)
            for s in range(0, X.shape[0], batch_size):
                mu, var = self.predict_f(X[s:s + batch_size], _shared=shared)
                means.append(mu)
                variances.append(var)
            return torch.cat(means, 0), torch.cat(variances, 0)
        M = KmmLambda.shape[0]
        thr = inverse_threshold if inverse_threshold is not None else min(cg.error_threshold ** 2, 1e-12)
        tight = ConjugateGradient(thr, cg.preconditioner, cg.max_iterations, cg.max_steps_cycle,
                                  min_float=cg.min_float, check_every=cg.check_every)
        Y = tight(KmmLambda, torch.eye(M, dtype=KmmLambda.dtype, device=KmmLambda.device))
        self.inverse_stats = tight.last_stats
        Y = (0.5 * (Y + Y.t())).contiguous()
        kernel, Z = self.kernel, self.inducing_variable.Z
        spec = kernel.spec(Z.shape[1])
        if use_fused_variance(fused_variance, Y.dtype, Z.shape[1], M):
            for s in range(0, X.shape[0], batch_size):
                xb = X[s:s + batch_size]
                variances.append((kernel.K_diag(xb) - ops.knm_quadform(spec, xb, Z, Y))[:, None])
                means.append(anyd_matvec(self.fused_anyd, "knm", spec, xb, Z, a) + self._mean(xb))
            return torch.cat(means, 0), torch.cat(variances, 0)
        for s in range(0, X.shape[0], batch_size):
            xb = X[s:s + batch_size]
            Knm = ops.k_dense(spec, xb, Z)  # [B, M] = Kmn^T
            Wt = ops.symm_matmul(Y, Knm)  # Kmn^T Y  (Y symmetric)
            variances.append((kernel.K_diag(xb) - (Knm * Wt).sum(dim=1))[:, None])
            means.append(anyd_matvec(self.fused_anyd, "knm", spec, xb, Z, a) + self._mean(xb))
        return torch.cat(means, 0), torch.cat(variances, 0)

    def _elbo_trace(self, data, probes):
        """`elbo` with `data_term="trace"`: the sum of the predictive variances as B variance - tr(A^-1 K_mn K_nm),
        estimated with the probes of the KL term (or exact, from Q = K_mn K_nm, in the dense model without probes)."""
        x, y = data
        exact = self.num_probes is None and probes is None
        if self.matrix_free and exact:
            raise ValueError("matrix_free=True needs num_probes (or probes=): the exact trace solves M right-hand sides")
        Z, cg = self.inducing_variable.Z, self.conjugate_gradient
        spec = self.kernel.spec(Z.shape[1])
        B, s2, variance = x.shape[0], float(self.likelihood.variance), float(self.kernel.variance)
        scale = self.scale(B) if B else 1.0  # without rows the data term is 0 whatever multiplies it
        Kmm, KmmLambda, times_kmm = self._system()
        a = cg(KmmLambda, self.pseudo_u)  # :303 / :339
        at = a.t().contiguous()
        quad = ops.dot_all(times_kmm(at), at)  # :316-317
        const = torch.log(self.diag_variance).sum().item()  # :321
        if exact:
            # tr(A^-1 K_mm) of the KL term and (scale / s2) tr(A^-1 Q) of the data term from one M-column solve
            rhs = Kmm + (scale / s2) * ops.kmn_knm(spec, x, Z) if B else Kmm
            both = cg(KmmLambda, rhs).diagonal().sum().item()
            if B == 0:
                return 0.5 * both - 0.5 * (quad - const)
            fmu = anyd_matvec(self.fused_anyd, "knm", spec, x, Z, a) + self._mean(x)
            resid = (y - fmu).contiguous()
            data_sum = -0.5 * B * math.log(2.0 * math.pi * s2) - 0.5 * (ops.dot_all(resid, resid) + B * variance) / s2
            return scale * data_sum + 0.5 * both - 0.5 * (quad - const)
        if probes is None:
            probes = rademacher((Z.shape[0], self.num_probes), Z.dtype, Z.device, self.probe_seed)
            self.probe_seed += 1
        P = probes.shape[1]
        S = cg(KmmLambda, probes)  # :311
        trace = ops.dot_all(S.t().contiguous(), times_kmm(probes.t().contiguous())) / P  # :312-314
        kl = 0.5 * (quad - trace - const)  # eval_logdet's forward value is 0.0
        if B == 0:
            return -kl
        out = anyd_matvec(self.fused_anyd, "knm", spec, x, Z,
                          torch.cat([a, S, probes], dim=1).contiguous())  # [mu | U | V], [B, 2 P + 1]
        resid = (y - (out[:, :1] + self._mean(x))).contiguous()
        uv = ops.dot_all(out[:, 1:1 + P].contiguous(), out[:, 1 + P:].contiguous()) / P  # ~ tr(A^-1 K_mn K_nm)
        data_sum = -0.5 * B * math.log(2.0 * math.pi * s2) - 0.5 * (ops.dot_all(resid, resid) + B * variance - uv) / s2
        return scale * data_sum - kl

    def _elbo_pathwise(self, data, probes, pathwise):
        """`elbo` with `data_term="pathwise"`: the likelihood term from S pathwise posterior samples, as
        `PathwiseClusterGP.compute_likelihood_term`, the [M, M] solve by the model's CG (S columns)."""
        from . import rff
        x, y = data
        Z, cg, kernel = self.inducing_variable.Z, self.conjugate_gradient, self.kernel
        B, M, D = x.shape[0], Z.shape[0], Z.shape[1]
        S, L = self.num_samples, self.num_bases
        if pathwise is None:
            pathwise = draw_pathwise(kernel.name, D, M, L, S, self.pathwise_seed)
            self.pathwise_seed += 1
        kl = self.prior_kl(probes=probes)
        if B == 0:
            return -kl
        E, W, xi = (torch.as_tensor(t).to(device=Z.device, dtype=Z.dtype) for t in pathwise)
        S, L = W.shape[0], E.shape[0]
        ls = torch.tensor(kernel.spec(D).lengthscales, dtype=Z.dtype, device=Z.device)
        theta = (E / ls[None, :]).contiguous()
        prior = rff.rff_sample(torch.cat([x, Z], dim=0), kernel, L, S, theta=theta, weights=W,
                               rff_anyd=self.rff_anyd)  # [S, B + M]
        lam = self.diag_variance[:, 0]
        eps = pathwise_epsilon(lam, S, self.epsilon, xi=xi)
        rhs = (self.pseudo_u[:, 0][None, :] - prior[:, B:] - eps).t().contiguous()  # [M, S]
        _, KmmLambda, _ = self._system()
        w = cg(KmmLambda, rhs)
        f = prior[:, :B] + anyd_matvec(self.fused_anyd, "knm", kernel.spec(D), x, Z, w.contiguous(), ops.COLS,
                                       ops.ROWS)  # [S, B]
        s2 = float(self.likelihood.variance)
        mean = self._mean(x)
        resid = (y.reshape(1, -1) - (f if self.mean_function is None else f + mean.reshape(1, -1))).contiguous()
        data_sum = -0.5 * (ops.dot_all(resid, resid) / (S * s2) + B * math.log(2.0 * math.pi * s2))
        return self.scale(B) * data_sum - kl

    def elbo(self, data, probes=None, pathwise=None):
        if self.data_term == "trace":
            return self._elbo_trace(data, probes)
        if self.data_term == "pathwise":
            return self._elbo_pathwise(data, probes, pathwise)
        x, y = data
        kl = self.prior_kl(probes=probes)
        f_mean, f_var = self.predict_f(x, full_cov=False, full_output_cov=False)
        var_exp = self.likelihood.variational_expectations(x, f_mean, f_var, y)
        return var_exp.sum().item() * self.scale(x.shape[0]) - kl

    def elbo_over_batches(self, data, batch_size, shared_inverse=True, probes=None):
        """sum_b elbo(batch_b) -- the quantity `make_metrics_callback` accumulates as "train/elbo"
        (`cggp/optimize.py:336-338`) -- without repeating the batch-independent work: the prior KL is
        evaluated once and counted once per batch, and the predictive moments of all rows come from
        `predict_f_batched` (with `shared_inverse`: one M-column CG for the whole data set instead of
        one B-column CG per batch).  With Hutchinson probes the reference draws fresh probes in every
        batch's KL; here the one evaluation stands for all of them.

        With `matrix_free=True` the default `shared_inverse=True` raises `ValueError` (the shared inverse is an [M, M]
        array): pass `shared_inverse=False` there."""
        x, y = data
        if shared_inverse and self.matrix_free:
            raise ValueError("shared_inverse=True forms the [M, M] inverse; matrix_free=True refuses it "
                             "(pass shared_inverse=False)")
        kl = self.prior_kl(probes=probes)
        mu, var = self.predict_f_batched(x, batch_size, shared_inverse=shared_inverse)
        ve = self.likelihood.variational_expectations(x, mu, var, y)
        total, nb = 0.0, 0
        for s in range(0, x.shape[0], batch_size):
            part = ve[s:s + batch_size]
            total += part.sum().item() * self.scale(part.shape[0])
            nb += 1
        return total - nb * kl

    def logdet_gradient(self, df=1.0, probes=None):
        """d/dK of the omitted log|Kmm+Lambda| term (`eval_logdet` backward, row M5)."""
        if self.matrix_free:
            raise ValueError("logdet_gradient() returns the [M, M] array dL/dK; matrix_free=True refuses it "
                             "(TrainableCGGP(matrix_free=True) contracts it with dK/dtheta instead)")
        _, KmmLambda = self._Kmm_and_KmmLambda()
        return eval_logdet_grad(KmmLambda, self.conjugate_gradient, df, self.num_probes, probes,
                                seed=self.probe_seed)


EPSILON_CONVENTIONS = ("reference", "matheron")


def pathwise_epsilon(lambda_diag, num_samples, convention="reference", seed=None, xi=None):
    """[S, M] noise of the pathwise update from standard normals xi [S, M] (drawn from `seed` when not given).

    "reference": lambda * xi, what `tfd.MultivariateNormalDiag(scale_diag=lambda_diag)` draws in the reference
    (`cggp/models.py:404-408`), i.e. covariance Lambda^2.  "matheron": sqrt(lambda) * xi, covariance Lambda, the
    noise Matheron's rule needs for the samples to have `predict_f`'s variance."""
    lam = torch.as_tensor(lambda_diag).reshape(-1)
    if xi is None:
        xi = torch.from_numpy(np.random.default_rng(seed).standard_normal((int(num_samples), lam.shape[0])))
    xi = torch.as_tensor(xi).to(device=lam.device, dtype=lam.dtype)
    if convention == "reference":
        return lam[None, :] * xi
    if convention == "matheron":
        return torch.sqrt(lam)[None, :] * xi
    raise ValueError(f"epsilon must be one of {EPSILON_CONVENTIONS}, got {convention!r}")


class PathwiseClusterGP(ClusterGP):
    """`cggp/models.py:357-420`: the ELBO's likelihood term from pathwise posterior function samples.

    A sample at X is f(X) + K_xz (K_zz + Lambda)^-1 (u - f(Z) - eps), with f one random-Fourier-feature prior draw
    evaluated at X and Z together (one theta and one W, as the reference concatenates them, :397-402).  Nothing of
    size N x M or N x L is formed: the prior comes from `mgp_rff_sample` (one fused sweep for D <= 32, S <= 8), the
    correction K_xz . weights from the multi-column K_nm sweep (`ops.knm_matvec`, R = S).  The [M, M] solve is a
    Cholesky factorisation, as in the `ClusterGP` twin, or -- with `conjugate_gradient=` -- that CG on K_zz + Lambda
    with S columns.

    `epsilon="reference"` (default, drop-in) draws eps with scale_diag = lambda, i.e. covariance Lambda^2, as the
    reference does; `epsilon="matheron"` draws covariance Lambda, for which the sample variance is `predict_f`'s.

    Random draws: numpy PCG64 from `seed` -- theta, then W, then the [S, M] normals of eps.  The values are not
    differentiable: like the reference, which only evaluates this model, `elbo` returns a float and no gradient
    flows through the random-feature term.

    `rff_anyd` (False, True or "auto"): the prior draw at D > 32 in fp64 by libmgp's fused any-D kernels
    (MGP_RFF_ANYD, include/mgp_pathwise.h) instead of feature panels; "auto" follows `rff.rff_anyd_auto`."""

    def __init__(self, kernel, likelihood, inducing_variable, *, conjugate_gradient=None, epsilon="reference",
                 rff_anyd=False, **kwargs):
        from .rff import check_rff_anyd
        self.rff_anyd = check_rff_anyd(rff_anyd)
        super().__init__(kernel, likelihood, inducing_variable, **kwargs)
        if epsilon not in EPSILON_CONVENTIONS:
            raise ValueError(f"epsilon must be one of {EPSILON_CONVENTIONS}, got {epsilon!r}")
        self.conjugate_gradient = conjugate_gradient
        self.epsilon = epsilon

    def elbo(self, data, *, num_bases=1, num_samples=1, seed=None):  # :358-371
        kl = self.prior_kl()
        likelihood = self.compute_likelihood_term(data, num_bases, num_samples, seed=seed)
        x, _ = data
        return likelihood * self.scale(x.shape[0]) - kl

    def compute_likelihood_term(self, data, num_bases, num_samples, *, seed=None):  # :373-388
        x, y = data
        num_data = y.shape[0]
        samples = self.pathwise_samples(x, num_bases, num_samples, seed=seed)  # [S, N, 1]
        noise = self.likelihood.variance
        error_squared = (y[None, ...] - samples) ** 2
        likelihood = error_squared.sum().item() / noise / num_samples
        constant_term = num_data * math.log(2.0 * math.pi * noise)
        return -0.5 * (likelihood + constant_term)

    def pathwise_samples(self, sample_at, num_bases, num_samples, *, seed=None, theta=None, weights=None, xi=None):
        """[S, N, 1] posterior function samples at `sample_at` (:390-420).  `theta` [L, D], `weights` [S, 2L] and
        `xi` [S, M] (standard normals of eps) may be injected; whatever is not is drawn from `seed`."""
        from . import rff

        iv, kernel = self.inducing_variable, self.kernel
        Z = iv.Z
        n, D = sample_at.shape
        lambda_diag = self.diag_variance[:, 0]
        rng = np.random.default_rng(seed)
        if theta is None:
            theta = rff.basis_theta_parameter(kernel, num_bases, rng, dim=D)
        if weights is None:
            weights = rff.rff_weights(num_samples, num_bases, rng)
        prior_at = torch.cat([sample_at, Z], dim=0)  # :397
        prior = rff.rff_sample(prior_at, kernel, num_bases, num_samples, theta=theta, weights=weights,
                               rff_anyd=self.rff_anyd)  # [S, N + M]
        prior_fx, prior_fz = prior[:, :n], prior[:, n:]
        epsilon = pathwise_epsilon(lambda_diag, num_samples, self.epsilon, rng, xi)  # :404-408
        solve_against = self.pseudo_u[:, 0][None, :] - prior_fz - epsilon  # [S, M], :414
        kzz_lambda = Kuu(iv, kernel, jitter=0.0, diag_add=lambda_diag)  # :411-412
        if self.conjugate_gradient is None:
            L = torch.linalg.cholesky(kzz_lambda)  # :415-416
            w = torch.cholesky_solve(solve_against.t().contiguous(), L)  # [M, S]
        else:
            w = self.conjugate_gradient(kzz_lambda, solve_against.t().contiguous())
        correction = ops.knm_matvec(kernel.spec(D), sample_at, Z, w.contiguous(), ops.COLS, ops.ROWS)  # [S, N], :418
        return (prior_fx + correction)[..., None]  # :419


class SGPR:
    """SGPR predictions and bound with the N-sized products done matrix-free (row S1).

    The reference reaches `gpflow.models.SGPR` through `sgpr_class` (`cggp/cli_utils.py:444-446`).
    Its two-Cholesky closed form is restated here in normal-equation form so that the only
    N-sized work is the fused sweeps:
        S = s2 (Kmm + jitter I) + K_mn K_nm,   alpha = S^-1 K_mn y            (CG, matrix-free S)
        mean* = K_*m alpha
        var*  = k_** - K_*m (Kmm+jI)^-1 K_m* + s2 K_*m S^-1 K_m*            (CG, two operators)
    `elbo()` needs log-determinants, so it forms K_mn K_nm explicitly on the matrix cores
    (`ops.kmn_knm`) and factorises the [M,M] result.  Rows of X may be this rank's shard: pass
    `allreduce` (parallel.make_allreduce) and every N-sized reduction is summed over ranks.
    """

    def __init__(self, data, kernel, inducing_variable, noise_variance, conjugate_gradient=None, *,
                 jitter=1e-6, allreduce=None, num_data=None, preconditioner="auto", explicit_rhs=8,
                 kmm_solver="cholesky", fused_anyd=False):
        """`preconditioner`: "auto" (the subsampled normal-equation preconditioner built from
        min(N, 32 M) rows of the data set -- all ranks together), None, or a
        `CGPreconditioner` for the [M,M] system.  `explicit_rhs`: solves on S with at least this
        many right-hand sides form S once on the matrix cores (`ops.kmn_knm`, 2NM^2 flops) and run
        the dense CG on it -- a matrix-free step costs two N x M sweeps per right-hand-side chunk,
        so beyond a handful of columns the explicit matrix is cheaper (0 disables).
        `kmm_solver`: how `K_*m (Kmm+jI)^-1 K_m*` of the predictive variance is formed --
        "cholesky" (GPflow's own `L = chol(Kmm + jitter I)`, one [M,M] factorisation, cached) or
        "cg" (the model's `conjugate_gradient`; Kmm + 1e-6 I is badly conditioned, so this takes
        hundreds of steps).
        `fused_anyd` (False, True or "auto"): handed to the `SgprNormalOperator` and the rule of the model's own
        K_mn y and K_*m alpha products -- at D > 32 in fp64 libmgp's fused any-D sweeps (include/mgp_sweep_anyd.h)
        instead of kernel panels; "auto" follows `conjugate_gradient.fused_anyd_auto`."""
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.X, self.Y = data
        self.kernel = kernel
        self.inducing_variable = inducingpoint_wrapper(inducing_variable)
        self.likelihood = Gaussian(noise_variance)
        self.conjugate_gradient = conjugate_gradient or ConjugateGradient(1e-6)
        self.jitter = float(jitter)
        self.allreduce = allreduce
        if num_data is None:
            # rows of X may be this rank's shard: N of the bound and of the "auto" preconditioner rule
            # is the GLOBAL row count, agreed by one all-reduce (every rank must call the constructor)
            num_data = self.X.shape[0]
            if allreduce is not None:
                t = torch.tensor([float(num_data)], dtype=torch.float64, device=self.X.device)
                allreduce(t)
                num_data = int(round(t.item()))
        self.num_data = num_data
        self.preconditioner = preconditioner
        self.explicit_rhs = int(explicit_rhs)
        if kmm_solver not in ("cholesky", "cg"):
            raise ValueError(f"unknown kmm_solver {kmm_solver!r}")
        self.kmm_solver = kmm_solver
        self.invalidate()

    # ---- caches.  Everything below is a function of (X, Y, Z, kernel and likelihood parameters,
    # jitter); `update_fn` / `multiple_assign` / `assign_inducing_parameters` change those from
    # outside (cggp/cli_utils.py:394-411, paper_cli_uci.py:123-124), so every public method first
    # compares a fingerprint of them and drops the caches when it moved.
    def invalidate(self):
        self._Lmm = None
        self._alpha = None
        self._op = None
        self._cg_S = None
        self._S = None
        self._KK = None
        self._C = None
        self._key = self._fingerprint()
        # keep the fingerprinted tensors alive: id() of a freed tensor can be handed to the next one
        self._key_refs = (self.inducing_variable.Z, self.X, self.Y)

    def _fingerprint(self):
        Z = self.inducing_variable.Z
        k = self.kernel
        return (id(Z), Z._version, tuple(Z.shape), id(self.X), self.X._version, id(self.Y), self.Y._version,
                type(k).__name__, float(k.variance), tuple(float(v) for v in k.lengthscales),
                float(self.likelihood.variance), float(self.jitter), id(self.conjugate_gradient),
                id(self.preconditioner) if not isinstance(self.preconditioner, str) else self.preconditioner)

    def _sync(self):
        if self._fingerprint() != self._key:
            self.invalidate()

    def operator(self):
        self._sync()
        if self._op is None:
            self._op = SgprNormalOperator(self.kernel, self.X, self.inducing_variable.Z,
                                          self.likelihood.variance, jitter=self.jitter,
                                          allreduce=self.allreduce, fused_anyd=self.fused_anyd)
        return self._op

    def solver(self):
        """The CG used on S: the model's `conjugate_gradient` settings plus the preconditioner."""
        self._sync()
        if self._cg_S is None:
            cg, pre = self.conjugate_gradient, self.preconditioner
            if isinstance(pre, str):
                if pre != "auto":
                    raise ValueError(f"unknown preconditioner {pre!r}")
                # Always built (its build contains collectives: no rank may decide otherwise from its
                # own shard).  The sample is min(N, 32 M) rows: a data set smaller than that gives
                # P = S itself, and CG then acts as iterative refinement of the factorised solve --
                # which is what brings the predictive variance to the 1e-6 of the closed form when
                # cond(S) ~ cond(Kmm)^2 leaves the un-preconditioned recurrence stuck at its guard floor
                pre = SubsampledNormalPreconditioner(self.operator())
            if pre is None:
                self._cg_S = cg
            else:
                cycle = cg.max_steps_cycle
                if cycle is None and self.X.dtype != torch.float64:
                    # below fp64 the preconditioned recurrence drifts from the true residual within
                    # ~16 steps; the reference's residual refresh (:71-84) every 4 keeps it honest
                    cycle = 4
                self._cg_S = ConjugateGradient(cg.error_threshold, pre, cg.max_iterations, cycle,
                                               min_float=cg.min_float, check_every=cg.check_every)
        return self._cg_S

    def dense_S(self):
        """S = s2 (Kmm + jitter I) + K_mn K_nm as an [M,M] matrix (formed once, cached)."""
        self._sync()
        if self._S is None:
            self._S = torch.add(self.kmn_knm(), self.operator().Kmm, alpha=self.likelihood.variance)
        return self._S

    def kmn_knm(self):
        """K_mn K_nm [M,M] on the matrix cores, summed over ranks (formed once, cached)."""
        self._sync()
        if self._KK is None:
            Z = self.inducing_variable.Z
            KK = ops.kmn_knm(self.kernel.spec(Z.shape[1]), self.X, Z)
            if self.allreduce is not None:
                self.allreduce(KK.view(-1))
            self._KK = KK
        return self._KK

    def solve_S(self, rhs):
        """S^-1 rhs for rhs [M, R]: matrix-free for a few columns, explicit S beyond `explicit_rhs`."""
        self._sync()
        if self._S is not None or (self.explicit_rhs > 0 and rhs.shape[1] >= self.explicit_rhs):
            return self.solver()(self.dense_S(), rhs)
        return self.solver()(self.operator(), rhs)

    def _Kmn_y(self):
        Z = self.inducing_variable.Z
        b = anyd_matvec(self.fused_anyd, "kmn", self.kernel.spec(Z.shape[1]), self.X, Z, self.Y)  # K_mn y, [M,1]
        if self.allreduce is not None:
            self.allreduce(b.view(-1))
        return b

    def alpha(self):
        self._sync()
        if self._alpha is None:
            self._alpha = self.solve_S(self._Kmn_y())
        return self._alpha

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        assert not full_output_cov
        self._sync()
        iv, kernel = self.inducing_variable, self.kernel
        mean = anyd_matvec(self.fused_anyd, "knm", kernel.spec(Xnew.shape[1]), Xnew, iv.Z, self.alpha())
        Kms = Kuf(iv, kernel, Xnew)
        if self.kmm_solver == "cholesky":
            if self._Lmm is None:
                self._Lmm = torch.linalg.cholesky(self.operator().Kmm)  # Kmm + jitter I
            W1 = torch.cholesky_solve(Kms, self._Lmm)
        else:
            W1 = self.conjugate_gradient(self.operator().Kmm, Kms)
        W2 = self.solve_S(Kms)
        if full_cov:  # GPflow SGPR.predict_f: [1, B, B]
            cov = kernel.K(Xnew) - Kms.t() @ W1 + self.likelihood.variance * (Kms.t() @ W2)
            return mean, cov[None, ...]
        var = kernel.K_diag(Xnew) - ops.colwise_dot(Kms, W1) + self.likelihood.variance * ops.colwise_dot(Kms, W2)
        return mean, var[:, None]

    def variance_matrix(self):
        """C = (Kmm + jitter I)^-1 - s2 S^-1 [M, M], symmetric, so that var* = k_** - K_*m C K_m* (cached).

        Formed without that subtraction, which cancels: with L = chol(Kmm + jitter I),
        AAT = L^-1 (K_mn K_nm) L^-T / s2 and B = I + AAT (the matrices of `elbo`), S = s2 L B L^T and
        C = L^-T (I - B^-1) L^-1 = L^-T (B^-1 AAT) L^-1.  K_mn K_nm is the all-reduced `kmn_knm()`, so the rows of X
        may be this rank's shard."""
        self._sync()
        if self._C is None:
            s2 = self.likelihood.variance
            KK = self.kmn_knm()
            L = torch.linalg.cholesky(self.operator().Kmm)  # Kmm + jitter I
            T1 = torch.linalg.solve_triangular(L, KK, upper=False)
            AAT = torch.linalg.solve_triangular(L, T1.t().contiguous(), upper=False) / s2
            AAT = 0.5 * (AAT + AAT.t())
            B = AAT + torch.eye(KK.shape[0], dtype=KK.dtype, device=KK.device)
            G = torch.cholesky_solve(AAT, torch.linalg.cholesky(B))  # B^-1 AAT
            G = 0.5 * (G + G.t())
            # L^-T G L^-1: two triangular solves from the left, G symmetric
            T2 = torch.linalg.solve_triangular(L.t(), G, upper=True)  # L^-T G
            C = torch.linalg.solve_triangular(L.t(), T2.t().contiguous(), upper=True)  # L^-T (L^-T G)^T
            self._C = (0.5 * (C + C.t())).contiguous()
        return self._C

    def predict_f_batched(self, X, batch_size=None, fused_variance="auto"):
        """(mean [N, P], var [N, 1]) for all rows of X: what `predict_f` returns with `full_cov=False`, without its two
        B-column solves per batch.  The mean is one K_*m alpha sweep over all rows; the variance is
        k_** - K_*m C K_m* with the [M, M] matrix of `variance_matrix()`, in chunks of `batch_size` rows (None: one).

        `fused_variance`: True forms K_*m C K_m* by `ops.knm_quadform` (include/mgp_predict.h: no [B, M] kernel panel,
        the upper triangle of C on the matrix cores), False composes it from `ops.k_dense`, `ops.symm_matmul` and a row
        sum, "auto" follows `conjugate_gradient.fused_variance_auto`."""
        check_fused_variance(fused_variance)
        self._sync()
        kernel, Z = self.kernel, self.inducing_variable.Z
        spec = kernel.spec(Z.shape[1])
        mean = anyd_matvec(self.fused_anyd, "knm", spec, X, Z, self.alpha())
        C = self.variance_matrix()
        fused = use_fused_variance(fused_variance, C.dtype, Z.shape[1], Z.shape[0])
        bs = batch_size or max(X.shape[0], 1)
        variances = []
        for s in range(0, X.shape[0], bs):
            xb = X[s:s + bs]
            if fused:
                quad = ops.knm_quadform(spec, xb, Z, C)
            else:
                Knm = ops.k_dense(spec, xb, Z)  # [B, M]
                quad = (Knm * ops.symm_matmul(C, Knm)).sum(dim=1)
            variances.append((kernel.K_diag(xb) - quad)[:, None])
        var = torch.cat(variances, 0) if variances else mean.new_empty((0, 1))
        return mean, var

    def predict_y(self, Xnew, full_cov=False, full_output_cov=False):
        """`predict_f` plus the noise variance (GPflow `GPModel.predict_y` with a Gaussian likelihood).  It runs
        `predict_f`'s two solves for all of Xnew at once: for many rows use `predict_y_batched`."""
        assert not full_cov and not full_output_cov
        mean, var = self.predict_f(Xnew)
        return mean, var + self.likelihood.variance

    def predict_y_batched(self, X, batch_size=None, fused_variance="auto"):
        """`predict_f_batched` plus the noise variance: the whole-data-set form of `predict_y`."""
        mean, var = self.predict_f_batched(X, batch_size, fused_variance)
        return mean, var + self.likelihood.variance

    def elbo(self):
        """Titsias' collapsed bound, GPflow `SGPR.elbo` (const + logdet + quad + trace)."""
        self._sync()
        iv, kernel = self.inducing_variable, self.kernel
        Z = iv.Z
        s2 = self.likelihood.variance
        N = self.num_data
        KK = self.kmn_knm()  # on the matrix cores; shared with the explicit-S solves
        yy = ops.dot_all(self.Y, self.Y)
        if self.allreduce is not None:
            t = torch.tensor([yy], dtype=torch.float64, device=Z.device)
            self.allreduce(t)
            yy = t.item()
        Kmn_y = self._Kmn_y()
        kuu = Kuu(iv, kernel, jitter=self.jitter)
        L = torch.linalg.cholesky(kuu)
        # A A^T = L^-1 (K_mn K_nm) L^-T / s2
        T1 = torch.linalg.solve_triangular(L, KK, upper=False)
        AAT = torch.linalg.solve_triangular(L, T1.t().contiguous(), upper=False) / s2
        B = AAT + torch.eye(Z.shape[0], dtype=Z.dtype, device=Z.device)
        LB = torch.linalg.cholesky(B)
        Aerr = torch.linalg.solve_triangular(L, Kmn_y, upper=False) / math.sqrt(s2)
        c = torch.linalg.solve_triangular(LB, Aerr, upper=False) / math.sqrt(s2)
        const = -0.5 * N * math.log(2.0 * math.pi)
        logdet = -torch.log(LB.diagonal()).sum().item() - 0.5 * N * math.log(s2)
        quad = -0.5 * yy / s2 + 0.5 * (c * c).sum().item()
        trace = -0.5 * N * kernel.variance / s2 + 0.5 * AAT.diagonal().sum().item()
        return const + logdet + quad + trace


LMLEstimate = namedtuple("LMLEstimate", ["value", "log_det", "data_fit", "std_error", "iterations", "converged"])
LMLEstimate.__doc__ = """`GPR.log_marginal_likelihood_estimate`: value = -1/2 data_fit - 1/2 P log_det - 1/2 N P log(2 pi),
data_fit = sum y^T (K + s2 I)^-1 y, std_error = the spread of the per-probe log-det terms / sqrt(t), iterations and
converged of the one CG solve."""


def _k_torch(kernel, A, B):
    """k(A, B) in plain torch (GPflow's expansion-form distance and profiles): the CPU half of
    `LanczosVarianceCache`, whose GPU half is libmgp's."""
    ls = torch.as_tensor(kernel.lengthscales, dtype=A.dtype, device=A.device)
    a, b = A / ls, B / ls
    r2 = (a * a).sum(-1)[:, None] + (b * b).sum(-1)[None, :] - 2.0 * (a @ b.t())
    if kernel.name == "se":
        return kernel.variance * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-36))
    if kernel.name == "matern12":
        return kernel.variance * torch.exp(-r)
    if kernel.name == "matern32":
        s3 = math.sqrt(3.0)
        return kernel.variance * (1.0 + s3 * r) * torch.exp(-s3 * r)
    s5 = math.sqrt(5.0)
    return kernel.variance * (1.0 + s5 * r + (5.0 / 3.0) * r * r) * torch.exp(-s5 * r)


class LanczosVarianceCache:
    """Predictive variances of exact GP regression for whole test sets from one Lanczos run (Pleiss et al. 2018,
    "LOVE").  k Lanczos steps on Khat = K + s2 I (`cggp.lanczos`, full re-orthogonalisation) give an orthonormal
    Q [k, N] and a tridiagonal T = Q Khat Q^T = C C^T; with R = Q^T C^-T [N, k]

        var(x*) ~= k(x*, x*) - |k(x*, X) R|^2,      cov(X*) ~= k(X*, X*) - (k(X*, X) R)(k(X*, X) R)^T.

    Per test point this costs what the mean costs -- one pass over the kernel values, `mgp_knm_project` on the GPU --
    instead of a CG solve.  It is a Galerkin projection of Khat^-1: it never under-states the variance, it decreases
    monotonically to the exact value as the rank grows (exact at rank N), and it is capped by the prior variance.  It
    is loose where the spectrum of K decays slowly (rough kernels, many input dimensions, short lengthscales).

    `build(gpr)` runs the recurrence on `gpr.operator()` from the normalised first column of Y (`start="y"`) or from
    a caller's vector [N]; `from_tridiagonal(Q, alpha, beta, X)` installs a hand-made basis on any device (CPU
    included: `variance` / `covariance` are plain torch there).  `rank_` holds the rank reached (the recurrence stops
    early when the Krylov space is exhausted)."""

    def __init__(self, rank=128, start="y", breakdown=1e-10):
        self.rank = int(rank)
        if self.rank < 1:
            raise ValueError("rank must be >= 1")
        if not (isinstance(start, torch.Tensor) or start == "y"):
            raise ValueError("start must be 'y' or a vector [N]")
        self.start = start
        self.breakdown = float(breakdown)
        self.rank_ = None
        self.X = self.R = None

    def build(self, gpr):
        from .lanczos import lanczos

        X, Y = gpr.data
        v = Y[:, 0] if isinstance(self.start, str) else self.start.to(device=X.device, dtype=X.dtype).reshape(-1)
        if v.shape[0] != X.shape[0]:
            raise ValueError(f"the start vector has {v.shape[0]} entries, the data {X.shape[0]} rows")
        Q, alpha, beta = lanczos(gpr.operator(), v, self.rank, self.breakdown)
        return self.from_tridiagonal(Q, alpha, beta, X)

    def from_tridiagonal(self, Q, alpha, beta, X=None):
        """Install the basis Q [k, N] with Q Khat Q^T = tridiag(beta, alpha, beta); X [N, D] are the training inputs
        the queries are taken against."""
        k = Q.shape[0]
        if alpha.shape[0] != k or beta.shape[0] != k - 1:
            raise ValueError(f"Q has {k} rows: alpha must be [{k}] and beta [{k - 1}]")
        if X is not None and X.shape[0] != Q.shape[1]:
            raise ValueError(f"Q has n={Q.shape[1]}, X has {X.shape[0]} rows")
        T = torch.diag(alpha) + torch.diag(beta, 1) + torch.diag(beta, -1)
        C = torch.linalg.cholesky(T)
        # R^T = C^-1 Q through the explicit k x k inverse of the triangular factor and one GEMM: a triangular solve
        # with N right-hand sides is not served by the BLAS at N = 2^17 (as PivotedCholeskyPreconditioner.set_factor)
        Cinv = torch.linalg.solve_triangular(C, torch.eye(k, dtype=Q.dtype, device=Q.device), upper=False)
        self.R = (Cinv @ Q).t().contiguous()  # [N, k]
        self.rank_ = k
        if X is not None:
            self.X = X
        return self

    def _project(self, kernel, Xnew, want_proj):
        if self.R is None or self.X is None:
            raise RuntimeError("no basis yet: call build(gpr) or from_tridiagonal(Q, alpha, beta, X)")
        if Xnew.is_cuda:
            return ops.knm_project(kernel.spec(Xnew.shape[1]), Xnew, self.X, self.R, want_proj=want_proj)
        proj = _k_torch(kernel, Xnew, self.X) @ self.R
        return (proj * proj).sum(dim=1), proj

    def variance(self, kernel, Xnew):
        """[B]: k(x*, x*) - |k(x*, X) R|^2."""
        sqnorm, _ = self._project(kernel, Xnew, False)
        return kernel.K_diag(Xnew) - sqnorm

    def covariance(self, kernel, Xnew):
        """[B, B]: k(X*, X*) - (k(X*, X) R)(k(X*, X) R)^T."""
        _, proj = self._project(kernel, Xnew, True)
        Kss = kernel.K(Xnew) if Xnew.is_cuda else _k_torch(kernel, Xnew, Xnew)
        return Kss - proj @ proj.t()


class GPR:
    """Exact GP regression: GPflow `GPR`'s surface (`gpflow.models.GPR(data, kernel, noise_variance)`), the baseline the
    reference builds through `gpr_class` / `create_gpr_model` (`cggp/cli_utils.py:171-184,449-452`) and whose
    `predict_f(x, full_cov=True)` is the ground truth of `paper_condition_wasserstein.py:60-135`.

    Two ways to solve with K + s2 I:
      "cholesky": `mgp_k_dense` forms it, `torch.linalg.cholesky` factors it -- GPflow's own arithmetic;
      "cg":       `KxxNoiseOperator`, matrix-free, through the model's `conjugate_gradient`:
                  alpha = (K + s2 I)^-1 y, mean = k(X*, X) alpha, and the variance solves (K + s2 I) W = K_X*
                  for the test columns in chunks of at most `variance_chunk_bytes` of K_X*.
      "auto":     Cholesky up to `cholesky_max_n` rows, CG above.
    `variance` chooses how the CG path gets predictive variances: "solve" (default) is the per-test-column solve
    above; "lanczos" builds a `LanczosVarianceCache` of rank `variance_rank` once per model state and answers every
    test row from it (var = K_diag - |k(x*, X) R|^2, an upper bound that tightens with the rank; the mean is
    unchanged).  The cache is dropped with alpha and the operator when the kernel, the noise or the data change.  On
    the Cholesky path the option is ignored: the exact variance is cheaper there.
    `fused_anyd` (False, True or "auto") is handed to the `KxxNoiseOperator` and is the rule of the model's own
    k(X*, X) products: at D > 32 in fp64 libmgp's fused any-D sweeps (include/mgp_sweep_anyd.h), not kernel panels.
    `sym_anyd` (False, True or "auto") is handed to the `KxxNoiseOperator` alone: at D > 32 in fp64 the CG path solves
    on `MGP_OP_KXX_NOISE_SYM_ANYD`, each unordered pair of rows once on the fp64 matrix cores.
    `log_marginal_likelihood` needs log|K + s2 I| and exists on the Cholesky path only;
    `log_marginal_likelihood_estimate` is its matrix-free stochastic Lanczos estimate at any N.
    """

    def __init__(self, data, kernel, noise_variance=1.0, conjugate_gradient=None, *, solver="auto",
                 cholesky_max_n=16384, variance_chunk_bytes=256 << 20, variance="solve", variance_rank=128,
                 fused_anyd=False, sym_anyd=False):
        self.fused_anyd = check_fused_anyd(fused_anyd)
        self.sym_anyd = check_sym_anyd(sym_anyd)
        if solver not in ("auto", "cholesky", "cg"):
            raise ValueError(f"unknown solver {solver!r}")
        if variance not in ("solve", "lanczos"):
            raise ValueError(f"unknown variance {variance!r}")
        X, Y = data
        if X.dim() != 2 or Y.dim() != 2 or Y.shape[0] != X.shape[0]:
            raise ValueError(f"data must be (X [N, D], Y [N, P]), got {tuple(X.shape)}, {tuple(Y.shape)}")
        self.data = (X, Y)
        self.kernel = kernel
        self.likelihood = Gaussian(noise_variance)
        self.conjugate_gradient = conjugate_gradient or ConjugateGradient(1e-6)
        self.solver = solver
        self.cholesky_max_n = int(cholesky_max_n)
        self.variance_chunk_bytes = int(variance_chunk_bytes)
        self.variance = variance
        self.variance_rank = int(variance_rank)
        self.invalidate()

    # ---- caches (alpha, the factor, the operator): functions of X, Y, the kernel and the noise, which
    # `multiple_assign` and the training loop change from outside -- dropped when the fingerprint moves (as SGPR)
    def invalidate(self):
        self._L = None
        self._alpha = None
        self._op = None
        self._variance_cache = None
        self._key = self._fingerprint()
        self._key_refs = self.data

    def _fingerprint(self):
        X, Y = self.data
        k = self.kernel
        return (id(X), X._version, tuple(X.shape), id(Y), Y._version, tuple(Y.shape), type(k).__name__,
                float(k.variance), tuple(float(v) for v in k.lengthscales), float(self.likelihood.variance),
                id(self.conjugate_gradient), self.solver, self.cholesky_max_n, self.variance, self.variance_rank)

    def _sync(self):
        if self._fingerprint() != self._key:
            self.invalidate()

    def uses_cholesky(self):
        return self.solver == "cholesky" or (self.solver == "auto" and self.data[0].shape[0] <= self.cholesky_max_n)

    def _spec(self):
        return self.kernel.spec(self.data[0].shape[1])

    def cholesky(self):
        """L = chol(K + s2 I) (GPflow GPR: add_likelihood_noise_cov, then cholesky); formed once, cached."""
        self._sync()
        if self._L is None:
            X = self.data[0]
            self._L = torch.linalg.cholesky(ops.k_dense(self._spec(), X, X, jitter=self.likelihood.variance))
        return self._L

    def operator(self):
        """K + s2 I as a matrix-free operator (`KxxNoiseOperator`)."""
        self._sync()
        if self._op is None:
            self._op = KxxNoiseOperator(self.kernel, self.data[0], self.likelihood.variance,
                                        fused_anyd=self.fused_anyd, sym_anyd=self.sym_anyd)
        return self._op

    def solve(self, rhs):
        """(K + s2 I)^-1 rhs for rhs [N, R]."""
        self._sync()
        if self.uses_cholesky():
            return torch.cholesky_solve(rhs, self.cholesky())
        return self.conjugate_gradient(self.operator(), rhs.contiguous())

    def alpha(self):
        self._sync()
        if self._alpha is None:
            self._alpha = self.solve(self.data[1])
        return self._alpha

    def variance_cache(self):
        """The `LanczosVarianceCache` of `variance="lanczos"` (built once per model state, cached)."""
        self._sync()
        if self._variance_cache is None:
            self._variance_cache = LanczosVarianceCache(self.variance_rank).build(self)
        return self._variance_cache

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """mean [B, P]; variance [B, P] or covariance [P, B, B] (GPflow GPR.predict_f, P = 1 output here)."""
        assert not full_output_cov
        self._sync()
        X, Y = self.data
        spec = self._spec()
        P = Y.shape[1]
        if self.uses_cholesky():
            L = self.cholesky()
            Kmn = ops.k_dense(spec, X, Xnew)  # [N, B]
            A = torch.linalg.solve_triangular(L, Kmn, upper=False)
            v = torch.linalg.solve_triangular(L, Y, upper=False)
            mean = A.t() @ v
            if full_cov:
                cov = ops.k_dense(spec, Xnew, Xnew) - A.t() @ A
                return mean, cov[None, ...].expand(P, -1, -1).contiguous()
            var = self.kernel.K_diag(Xnew) - (A * A).sum(dim=0)
            return mean, var[:, None].expand(-1, P).contiguous()
        mean = anyd_matvec(self.fused_anyd, "knm", spec, Xnew, X, self.alpha())
        if self.variance == "lanczos":
            cache = self.variance_cache()
            if full_cov:
                cov = cache.covariance(self.kernel, Xnew)
                cov = 0.5 * (cov + cov.t())
                return mean, cov[None, ...].expand(P, -1, -1).contiguous()
            var = cache.variance(self.kernel, Xnew)
            return mean, var[:, None].expand(-1, P).contiguous()
        B, N = Xnew.shape[0], X.shape[0]
        step = max(1, min(B, self.variance_chunk_bytes // max(1, N * X.element_size())))
        if full_cov:
            cov = ops.k_dense(spec, Xnew, Xnew)
        else:
            var = self.kernel.K_diag(Xnew).clone()
        for c0 in range(0, B, step):
            xs = Xnew[c0:c0 + step]
            Kc = ops.k_dense(spec, X, xs)  # [N, bc]
            Wc = self.conjugate_gradient(self.operator(), Kc)
            if full_cov:
                # K_*X W = K_*X (K + s2 I)^-1 K_X*
                cov[:, c0:c0 + step] -= anyd_matvec(self.fused_anyd, "knm", spec, Xnew, X, Wc)
            else:
                var[c0:c0 + step] -= ops.colwise_dot(Kc, Wc)
        if full_cov:
            cov = 0.5 * (cov + cov.t())
            return mean, cov[None, ...].expand(P, -1, -1).contiguous()
        return mean, var[:, None].expand(-1, P).contiguous()

    def predict_y(self, Xnew, full_cov=False, full_output_cov=False):
        mean, var = self.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        if full_cov:
            eye = torch.eye(var.shape[-1], dtype=var.dtype, device=var.device)
            return mean, var + self.likelihood.variance * eye
        return mean, var + self.likelihood.variance

    def log_marginal_likelihood(self):
        """log N(y | 0, K + s2 I), GPflow GPR.log_marginal_likelihood (multivariate_normal on the Cholesky factor)."""
        self._sync()
        if not self.uses_cholesky():
            raise NotImplementedError(
                "GPR.log_marginal_likelihood needs log|K + s2 I|, which the CG path does not form; use "
                "log_marginal_likelihood_estimate() (stochastic Lanczos quadrature), solver='cholesky' or raise "
                "cholesky_max_n")
        X, Y = self.data
        L = self.cholesky()
        v = torch.linalg.solve_triangular(L, Y, upper=False)
        N, P = Y.shape
        logdet = torch.log(L.diagonal()).sum().item()
        return -0.5 * N * P * math.log(2.0 * math.pi) - P * logdet - 0.5 * (v * v).sum().item()

    def log_marginal_likelihood_estimate(self, num_probes=15, seed=0, probes=None):
        """Matrix-free estimate of log N(y | 0, K + s2 I), whatever `solver` is set (`LMLEstimate`).

        One CG solve on the `KxxNoiseOperator` with the columns [Y, Z] (t Rademacher probes Z [N, t] drawn from a
        seeded CPU `torch.Generator`, or `probes`), each normalised to unit norm so that the model's `error_threshold`
        acts per column and relative, records its step lengths and direction ratios (`ops.pcg_solve_record`).
        alpha = (K + s2 I)^-1 Y gives the data fit; the probe columns' Lanczos tridiagonals give
        log|K + s2 I| ~= (1/t) sum_i |z_i|^2 e1^T log(T_i) e1 (stochastic Lanczos quadrature, `cggp.slq`).

        When the model's CG carries a `PivotedCholeskyPreconditioner` P the recording solve is preconditioned: the
        probes are `P.sample(t, seed=seed)` (draws from N(0, P)), each probe's weight is z^T P^-1 z and
        log_det = log|P| + the mean of the per-probe terms.  `probes` given by the caller are then taken as draws
        with E[z z^T] = P -- the caller's duty; without the preconditioner they keep E[z z^T] = I."""
        return self._lml_estimate(num_probes, seed, probes)[0]

    def _lml_estimate(self, num_probes=15, seed=0, probes=None, conjugate_gradient=None):
        """(LMLEstimate, alpha [N, P], (K + s2 I)^-1 Z [N, t], Z [N, t]) -- with a `PivotedCholeskyPreconditioner` on
        the CG the last entry is P^-1 Z, the right-hand factor of the gradient's trace term
        E[(Khat^-1 z)^T dK (P^-1 z)] (`training._GPRLmlEstimate`)."""
        self._sync()
        X, Y = self.data
        N, P = Y.shape
        cg = conjugate_gradient or self.conjugate_gradient
        pre = cg.preconditioner if isinstance(cg.preconditioner, PivotedCholeskyPreconditioner) else None
        if pre is not None:
            pre._prepare(self.operator())
        if probes is None:
            if pre is not None:
                probes = pre.sample(int(num_probes), seed=int(seed))
            else:
                gen = torch.Generator().manual_seed(int(seed))
                probes = torch.randint(0, 2, (N, int(num_probes)), generator=gen, dtype=torch.int64) * 2 - 1
        probes = probes.to(device=X.device, dtype=X.dtype)
        if probes.dim() != 2 or probes.shape[0] != N or probes.shape[1] < 1:
            raise ValueError(f"probes must be [N={N}, t >= 1], got {tuple(probes.shape)}")
        t = probes.shape[1]
        B = torch.cat([Y, probes], dim=1).t().contiguous()  # [P + t, N]: the solve's rows are the columns
        norms = torch.linalg.vector_norm(B, dim=1, keepdim=True)
        scale = torch.where(norms > 0, norms, torch.ones_like(norms))
        if pre is None:
            sol, _, stats, coef = ops.pcg_solve_record(
                self.operator(), B / scale, cg.error_threshold, cg.max_iterations, cg.min_float, cg.check_every)
            weights, right, log_det_p = norms[P:, 0] ** 2, probes, 0.0
        else:
            # preconditioned CG is Lanczos on P^-1/2 Khat P^-1/2 started at P^-1/2 z: the quadrature weight of a probe
            # is z^T P^-1 z, and with E[z z^T] = P the mean estimates log|Khat| - log|P|
            sol, _, stats, coef = ops.pcg_solve_record(
                self.operator(), B / scale, cg.error_threshold, cg.max_iterations, cg.min_float, cg.check_every,
                preconditioner=pre)
            PiZ = pre.solve(B[P:])  # [t, N]
            weights, right, log_det_p = (B[P:] * PiZ).sum(dim=1), PiZ.t(), pre.log_det()
        sol = sol * scale
        alpha, W = sol[:P].t(), sol[P:].t()
        quads, _ = slq_log_quadratic(coef[:, P:, :].cpu().numpy(), weights.cpu().numpy(),
                                     cg.error_threshold, cg.min_float)
        log_det = log_det_p + float(np.mean(quads))
        std_error = float(np.std(quads, ddof=1) / math.sqrt(t)) if t > 1 else float("nan")
        data_fit = float((Y * alpha).sum())
        value = -0.5 * data_fit - 0.5 * P * log_det - 0.5 * N * P * math.log(2.0 * math.pi)
        est = LMLEstimate(value, log_det, data_fit, std_error, int(stats.iterations), bool(stats.converged))
        return est, alpha, W, right

    def maximum_log_likelihood_objective(self):
        return self.log_marginal_likelihood()

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()


def gpr_class(train_data, kernel, likelihood, **kwargs):
    """`cggp/cli_utils.py:449-452` (GPflow GPR there)."""
    return GPR(train_data, kernel, noise_variance=likelihood.variance, **kwargs)


def create_gpr_model(train_data, _kernel_fn, **model_kwargs):
    """`cggp/cli_utils.py:171-184`: noise variance 0.1 and the module's `kernel_fn(dim)` (the reference, too, ignores
    its `_kernel_fn` argument)."""
    from .cli_utils import kernel_fn

    dim = train_data[0].shape[-1]
    return GPR(train_data, kernel_fn(dim), noise_variance=0.1, **model_kwargs)


def cdgp_class(kernel, likelihood, iv, error_threshold=1e-6, preconditioner=None, **kwargs):
    """`cggp/cli_utils.py:439-441`.  `preconditioner` (build-side addition): the `CGPreconditioner` of every solve, e.g.
    `PivotedCholeskyPreconditioner()` with `matrix_free=True`."""
    conjugate_gradient = ConjugateGradient(error_threshold, preconditioner=preconditioner)
    return CGGP(kernel, likelihood, iv, conjugate_gradient, **kwargs)


def sgpr_class(train_data, kernel, likelihood, iv, **kwargs):
    """`cggp/cli_utils.py:444-446` (GPflow SGPR there; the CG form here)."""
    return SGPR(train_data, kernel, iv, noise_variance=likelihood.variance, **kwargs)


def rmse_nlpd(model, test_data, batch_size=None, batched=False):
    """Test RMSE / NLPD as `make_metrics_callback` computes them (`cggp/optimize.py:302-309,344-350`).
    `batched=True` predicts all rows by `model.predict_f_batched(x, batch_size)` where the model has one (the pieces
    that do not depend on the rows are formed once); the default loops `predict_f`."""
    x, y = test_data
    bs = batch_size or x.shape[0]
    if batched and hasattr(model, "predict_f_batched") and x.shape[0] > 0:
        mu, var = model.predict_f_batched(x, bs)
        lpd = model.likelihood.predict_log_density(x, mu, var, y).sum().item()
        return math.sqrt(((y - mu) ** 2).sum().item() / x.shape[0]), -lpd / x.shape[0]
    sq, lpd, n = 0.0, 0.0, 0
    for s in range(0, x.shape[0], bs):
        xb, yb = x[s:s + bs], y[s:s + bs]
        mu, var = model.predict_f(xb)
        lpd += model.likelihood.predict_log_density(xb, mu, var, yb).sum().item()
        sq += ((yb - mu) ** 2).sum().item()
        n += xb.shape[0]
    return math.sqrt(sq / n), -lpd / n
