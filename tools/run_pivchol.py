"""Pivoted-Cholesky preconditioner of exact GPR (`mgp_kxx_pivchol`, `mgp_lowrank_apply`, `MGP_PRE_LOWRANK`): build
time, application time, and converged solves / marginal-likelihood evaluations with and without it.

    python tools/run_pivchol.py [--sizes 17,20] [--lml-sizes 17] [--identity-cap 17:0,20:120] [--reps 3]
                                [--out profiles/pivchol_times.json]

SE, fp64, rank 128, noise 0.1, inputs X ~ U(-3, 3)^(N x D), y = sin(sum x) + 0.1 eps; cases D = 2 (lengthscale 1.5),
D = 8 (3.0) and D = 8 (1.5, where a low-rank preconditioner should not pay).  HIP events around synchronised calls; the
identity and the preconditioned form alternate in one process.  `--identity-cap LG:STEPS` bounds the identity solve at
size 2^LG (0 = until converged); a capped solve is reported with converged = false and is a lower bound.  Two
conditions are evaluated per size and written out: the one-column application under 5 % of the one-column operator,
the build under ten one-column operator applications.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import kernels, models, ops  # noqa: E402
from cggp.conjugate_gradient import (ConjugateGradient, EyePreconditioner, KxxNoiseOperator,  # noqa: E402
                                     PivotedCholeskyPreconditioner, _solve_device)

CASES = [(2, 1.5), (8, 3.0), (8, 1.5)]
RANK, S2, THR = 128, 0.1, 1e-8


def timed(fn, reps=1):
    """(median ms by HIP events around a synchronised call, last result)"""
    out, ms = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="17,20")
    ap.add_argument("--lml-sizes", default="17")
    ap.add_argument("--identity-cap", default="17:0,20:120")
    ap.add_argument("--cases-at", default="17:0,1,2;20:0", help="case indices per size")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pivchol_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    caps = {int(a): int(b) for a, b in (kv.split(":") for kv in args.identity_cap.split(","))}
    cases_at = {int(a): [int(i) for i in b.split(",")] for a, b in (kv.split(":") for kv in args.cases_at.split(";"))}
    lml_sizes = {int(s) for s in args.lml_sizes.split(",") if s}
    res = {"device": torch.cuda.get_device_name(0), "kernel": "se", "rank": RANK, "noise": S2, "threshold": THR,
           "probes": 15, "sizes": []}
    for lg in [int(s) for s in args.sizes.split(",")]:
        N = 1 << lg
        size = {"N": N, "cases": []}
        for ci in cases_at.get(lg, [0]):
            D, ls = CASES[ci]
            rng = np.random.default_rng(0)
            X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(dev)
            y = torch.sin(X.sum(dim=1)) + 0.1 * torch.from_numpy(rng.standard_normal(N)).to(dev)
            kern = kernels.SquaredExponential(1.0, [ls] * D)
            op = KxxNoiseOperator(kern, X, S2)
            v1 = torch.from_numpy(rng.standard_normal((1, N))).to(dev)
            v16 = torch.from_numpy(rng.standard_normal((16, N))).to(dev)
            op.rmatmul(v1)  # warm-up (arenas)
            op_ms, _ = timed(lambda: op.rmatmul(v1), args.reps)
            ops.kxx_pivchol(op.spec, X, RANK, 0.0)  # warm-up
            build_ms, (L, piv, diag) = timed(lambda: ops.kxx_pivchol(op.spec, X, RANK, 0.0), args.reps)
            # factor + the k x k Cholesky and B = C^-1 L D^-1 in torch, on a fresh object each time; one untimed call
            # first (the first torch.linalg call of a process loads the solver library's kernels)
            fresh = lambda: PivotedCholeskyPreconditioner(rank=RANK, rel_tol=0.0)
            fresh()._prepare(op)
            setup_ms, _ = timed(lambda: fresh()._prepare(op), args.reps)
            pre = fresh()
            pre._prepare(op)
            ops.lowrank_apply(pre.diag_inv, pre.B, v16)
            ap1_ms, _ = timed(lambda: ops.lowrank_apply(pre.diag_inv, pre.B, v1), args.reps)
            ap16_ms, _ = timed(lambda: ops.lowrank_apply(pre.diag_inv, pre.B, v16), args.reps)
            row = {"D": D, "lengthscale": ls, "operator_1col_ms": op_ms, "build_ms": build_ms,
                   "setup_ms_build_plus_woodbury": setup_ms, "apply_1col_ms": ap1_ms, "apply_16col_ms": ap16_ms,
                   "apply_bytes": 2 * 8 * RANK * N, "apply_1col_GBps": 2 * 8 * RANK * N / ap1_ms / 1e6,
                   "build_bytes_estimate": 4 * RANK * RANK * N, "trace_left": float(diag.sum()) / N,
                   "condition_a_apply_under_5pct_of_operator": ap1_ms < 0.05 * op_ms,
                   "condition_b_build_under_10_operators": build_ms < 10 * op_ms}
            rhs = y[None, :].contiguous()
            cap = caps.get(lg, 0) or N
            id_ms, (x_id, st_id, _) = timed(lambda: _solve_device(op, rhs, None, THR, EyePreconditioner(), cap, cap + 1, 1e-16, 10))
            pc_ms, (x_pc, st_pc, _) = timed(lambda: _solve_device(op, rhs, None, THR, pre, N, N + 1, 1e-16, 10))
            res_id = float(torch.linalg.vector_norm(op.rmatmul(x_id) - rhs))
            res_pc = float(torch.linalg.vector_norm(op.rmatmul(x_pc) - rhs))
            row["solve"] = {"identity_ms": id_ms, "identity_steps": st_id.iterations, "identity_converged": bool(st_id.converged),
                            "identity_residual": res_id, "preconditioned_ms": pc_ms, "preconditioned_steps": st_pc.iterations,
                            "preconditioned_converged": bool(st_pc.converged), "preconditioned_residual": res_pc,
                            "build_plus_preconditioned_ms": setup_ms + pc_ms,
                            "speedup_incl_build": id_ms / (setup_ms + pc_ms)}
            if lg in lml_sizes:
                Y = y[:, None].contiguous()
                mi = models.GPR((X, Y), kern, noise_variance=S2, conjugate_gradient=ConjugateGradient(THR), solver="cg")
                mp = models.GPR((X, Y), kern, noise_variance=S2, solver="cg",
                                conjugate_gradient=ConjugateGradient(THR, preconditioner=PivotedCholeskyPreconditioner(RANK, 0.0)))
                li_ms, ei = timed(lambda: mi.log_marginal_likelihood_estimate(num_probes=15, seed=0))
                mp.invalidate()
                lp_ms, ep = timed(lambda: mp.log_marginal_likelihood_estimate(num_probes=15, seed=0))  # builds the factor
                row["lml"] = {"identity_ms": li_ms, "identity_steps": ei.iterations, "identity_log_det": ei.log_det,
                              "identity_std_error": ei.std_error, "preconditioned_ms_incl_build": lp_ms,
                              "preconditioned_steps": ep.iterations, "preconditioned_log_det": ep.log_det,
                              "preconditioned_std_error": ep.std_error, "value_identity": ei.value,
                              "value_preconditioned": ep.value}
            size["cases"].append(row)
            print(json.dumps(row), flush=True)
            del X, y, L, pre, v1, v16
            torch.cuda.empty_cache()
        res["sizes"].append(size)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # after every size: a later size that runs out of time loses nothing
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
