"""Lanczos variance cache of exact GPR (`mgp_knm_project`, `cggp.lanczos`, `GPR(variance="lanczos")`): query time
against the compositions that give the same result without the fused kernel, build time, today's per-column solve, and
the accuracy of the cache against the rank.

    python tools/run_love.py [--parts query,build,solve,accuracy] [--lg-n 17] [--lg-b 14] [--rank 128] [--rounds 5]
                             [--out profiles/love_times.json]

fp64, noise 0.1, inputs X ~ U(-3, 3)^(N x D), y = sin(sum x) + 0.1 eps; cases (D, lengthscale) = (2, 1.5), (8, 3.0),
kernels SE and Matern-3/2.  HIP events around synchronised calls, one warm-up, the versions of a comparison alternated
round by round within one process, median and spread (min, max) reported.

query:    k(Xs, X) R and its row norms, B = 2^lg-b test rows against N = 2^lg-n: `ops.knm_project` (fused), R in both
          layouts; `ops.k_dense` row panels of 256 MiB + torch.matmul + square-sum; `ops.knm_matvec` in groups of 8
          columns.  Floor: 2 B N r flop at 64 cycles per v_mfma_f64_16x16x4_f64 and SIMD at the 2.4 GHz peak clock.
build:    `rank` Lanczos steps on the operator; the share outside the operator (re-orthogonalisation and the rest).
solve:    `GPR(variance="solve").predict_f` for 64 test rows, once; per-row cost and its extrapolation to B rows.
accuracy: N = 2^14 (Cholesky affordable), 1024 test rows, ranks 32 ... 256: max and median relative excess of the
          variance over the exact one, and the NLPD beside the exact NLPD.
"""

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import kernels, models, ops  # noqa: E402
from cggp.conjugate_gradient import ConjugateGradient  # noqa: E402
from cggp.lanczos import lanczos  # noqa: E402

CASES = [(2, 1.5), (8, 3.0)]
KERNELS = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}
S2 = 0.1


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternated(fns, rounds):
    """{name: {median_ms, min_ms, max_ms}}: one warm-up each, then `rounds` rounds with the versions in turn."""
    for fn in fns.values():
        fn()
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(once(fn)[0])
    return {name: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
            for name, v in ms.items()}


def make(N, D, dev, seed=0):
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(dev)
    y = torch.sin(X.sum(dim=1)) + 0.1 * torch.from_numpy(rng.standard_normal(N)).to(dev)
    return X, y[:, None].contiguous(), rng


def part_query(args, dev, res):
    N, B, r = 1 << args.lg_n, 1 << args.lg_b, args.rank
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    floor_ms = 2.0 * B * N * r / (cus * 4 * 2048 / 64 * 2.4e9) * 1e3
    rows = []
    for D, ls in CASES:
        X, _, rng = make(N, D, dev)
        Xs = torch.from_numpy(rng.uniform(-3.0, 3.0, (B, D))).to(dev)
        R = torch.from_numpy(rng.standard_normal((N, r))).to(dev)
        Rt = R.t().contiguous()
        panel = max(1, (256 << 20) // (8 * N))
        groups = [R[:, c:c + 8].contiguous() for c in range(0, r, 8)]
        for name, cls in KERNELS.items():
            spec = cls(1.0, [ls] * D).spec(D)

            def dense():
                out = torch.empty((B,), dtype=torch.float64, device=dev)
                for c0 in range(0, B, panel):
                    p = ops.k_dense(spec, Xs[c0:c0 + panel], X) @ R
                    out[c0:c0 + panel] = (p * p).sum(dim=1)
                return out

            def sweeps():
                out = torch.zeros((B,), dtype=torch.float64, device=dev)
                for g in groups:
                    p = ops.knm_matvec(spec, Xs, X, g)
                    out += (p * p).sum(dim=1)
                return out

            fns = {"fused_cols": lambda: ops.knm_project(spec, Xs, X, R)[0],
                   "fused_rows": lambda: ops.knm_project(spec, Xs, X, Rt, r_layout=ops.ROWS)[0],
                   "k_dense_matmul": dense, "knm_matvec_groups": sweeps}
            ref = dense()
            err = {k: float(torch.linalg.vector_norm(f() - ref) / torch.linalg.vector_norm(ref)) for k, f in fns.items()}
            row = {"kernel": name, "D": D, "lengthscale": ls, "N": N, "B": B, "r": r, "mfma_floor_ms": floor_ms,
                   "kernel_evaluations": B * N, "times": alternated(fns, args.rounds), "rel_diff_to_k_dense": err}
            row["fused_over_floor"] = row["times"]["fused_cols"]["median_ms"] / floor_ms
            rows.append(row)
            print(json.dumps(row), flush=True)
        del X, Xs, R, Rt, groups
        torch.cuda.empty_cache()
    res["query"] = rows


def part_build(args, dev, res):
    N, r = 1 << args.lg_n, args.rank
    rows = []
    for D, ls in CASES:
        X, Y, rng = make(N, D, dev)
        m = models.GPR((X, Y), kernels.SquaredExponential(1.0, [ls] * D), noise_variance=S2, solver="cg")
        op = m.operator()
        v = Y[:, 0].contiguous()
        op.rmatmul(v[None, :])
        op_ms = float(np.median([once(lambda: op.rmatmul(v[None, :]))[0] for _ in range(5)]))
        lanczos(op, v, 8)
        lz = [once(lambda: lanczos(op, v, r))[0] for _ in range(max(2, args.rounds // 2))]
        cache_ms, cache = once(lambda: models.LanczosVarianceCache(r).build(m))
        row = {"kernel": "se", "D": D, "lengthscale": ls, "N": N, "rank": r, "rank_reached": cache.rank_,
               "operator_1col_ms": op_ms, "lanczos_median_ms": float(np.median(lz)), "lanczos_min_ms": float(min(lz)),
               "lanczos_max_ms": float(max(lz)), "cache_build_ms_incl_factor": cache_ms,
               "share_outside_operator": 1.0 - r * op_ms / float(np.median(lz))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, Y, m, op, cache
        torch.cuda.empty_cache()
    res["build"] = rows


def part_solve(args, dev, res):
    N, B = 1 << args.lg_n, 1 << args.lg_b
    D, ls = CASES[1]
    X, Y, rng = make(N, D, dev)
    Xs = torch.from_numpy(rng.uniform(-3.0, 3.0, (64, D))).to(dev)
    kern = kernels.SquaredExponential(1.0, [ls] * D)
    cg = ConjugateGradient(1e-8, max_iterations=2000)
    m = models.GPR((X, Y), kern, noise_variance=S2, conjugate_gradient=cg, solver="cg")
    m.alpha()  # the mean's solve is common to both paths
    ms, (_, var) = once(lambda: m.predict_f(Xs))
    love = models.GPR((X, Y), kern, noise_variance=S2, conjugate_gradient=cg, solver="cg", variance="lanczos",
                      variance_rank=args.rank)
    love._alpha = m._alpha
    build_ms, _ = once(love.variance_cache)
    q_ms, (_, var_l) = once(lambda: love.predict_f(Xs))
    res["solve"] = {"kernel": "se", "D": D, "lengthscale": ls, "N": N, "rows": 64, "solve_ms_once": ms,
                    "per_row_ms": ms / 64, "extrapolated_to_B_rows_s": ms / 64 * B / 1e3, "B": B,
                    "note": "one run, 64 rows in one batched solve; the figure for B rows is an extrapolation",
                    "lanczos_build_ms": build_ms, "lanczos_query_64_rows_ms": q_ms, "rank": args.rank,
                    "max_rel_excess_of_cache": float(((var_l - var) / var).max()),
                    "min_excess_of_cache": float((var_l - var).min())}
    print(json.dumps(res["solve"]), flush=True)


def part_accuracy(args, dev, res):
    N, B = 1 << 14, 1024
    rows = []
    for D, ls in CASES:
        X, Y, rng = make(N, D, dev)
        Xs = torch.from_numpy(rng.uniform(-3.0, 3.0, (B, D))).to(dev)
        ys = torch.sin(Xs.sum(dim=1, keepdim=True)) + 0.1 * torch.from_numpy(rng.standard_normal((B, 1))).to(dev)
        for name, cls in KERNELS.items():
            kern = cls(1.0, [ls] * D)
            chol = models.GPR((X, Y), kern, noise_variance=S2, solver="cholesky")
            mu, v0 = chol.predict_f(Xs)
            nlpd0 = models.rmse_nlpd(chol, (Xs, ys))[1]
            cg = ConjugateGradient(1e-10, max_iterations=4000)
            for rank in [32, 64, 128, 256]:
                love = models.GPR((X, Y), kern, noise_variance=S2, conjugate_gradient=cg, solver="cg",
                                  variance="lanczos", variance_rank=rank)
                love._alpha = chol.solve(Y)  # the mean is not the subject here
                _, v = love.predict_f(Xs)
                ex = ((v - v0) / v0)[:, 0]
                exy = ((v - v0) / (v0 + S2))[:, 0]
                row = {"kernel": name, "D": D, "lengthscale": ls, "N": N, "rank": rank,
                       "rank_reached": love.variance_cache().rank_, "max_rel_excess_f": float(ex.max()),
                       "median_rel_excess_f": float(ex.median()), "min_excess": float((v - v0).min()),
                       "max_rel_excess_y": float(exy.max()), "median_rel_excess_y": float(exy.median()),
                       "nlpd": models.rmse_nlpd(love, (Xs, ys))[1], "nlpd_exact": nlpd0}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del chol
            torch.cuda.empty_cache()
    res["accuracy"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="query,build,solve,accuracy")
    ap.add_argument("--lg-n", type=int, default=17)
    ap.add_argument("--lg-b", type=int, default=14)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "love_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "noise": S2, "dtype": "float64"}
    for part in args.parts.split(","):
        {"query": part_query, "build": part_build, "solve": part_solve, "accuracy": part_accuracy}[part](args, dev, res)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # after every part: a later part that runs out of time loses nothing
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
