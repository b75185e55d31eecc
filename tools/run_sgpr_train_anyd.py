"""SGPR training above 32 input dimensions (`mgp_kmn_knm_vjp_anyd`, include/mgp_anyd.h): the time of the N-sized
backward against the same gradient built from the entry points that existed before it, and against the forward.

    python tools/run_sgpr_train_anyd.py [--lg-n 18] [--m 4096] [--dims 77,90] [--kernels matern32,se] [--rounds 5]
                                        [--out profiles/sgpr_train_anyd_times.json]
    python tools/run_sgpr_train_anyd.py --profile-child [--lg-n 18] [--m 4096]     (under rocprofv3 --kernel-trace --stats)
    python tools/run_sgpr_train_anyd.py --stats-summary '<dir>/**/*kernel_stats.csv' --out <json>   (adds the split)

fp64, X ~ U(-2, 2)^(N x D), Z a perturbed sample of X, lengthscales sqrt(D) * linspace(0.8, 1.2), random cotangents
Gq [M, M] and Gb [M, 1].  HIP events around synchronised calls, one warm-up, the versions alternated round by round
within one process, median and (min, max) reported: boxes differ by +-5 %, only the in-run ratios count.

forward:      `ops.kmn_knm` + `ops.kmn_matvec` (K_mn K_nm and K_mn y), what `_SGPRElbo.forward` enqueues
vjp, vjp_dz:  `ops.kmn_knm_vjp_anyd` without and with dZ
composed, composed_dz: row panels of 256 MiB of `ops.k_dense`, `torch.matmul` for W = K (Gq + Gq^T) + Y Gb^T,
              `ops.k_dense_vjp` for (dvariance, dl) and `training.k_grad_points` for dZ -- the yardstick
"""

import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import ops, training  # noqa: E402

VAR = 1.2


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


def make(N, M, D, dev, seed=0):
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.uniform(-2.0, 2.0, (N, D))).to(dev)
    Y = (torch.sin(1.5 * X[:, :1]) * torch.cos(X[:, 1:2])).contiguous()
    Z = (X[torch.from_numpy(rng.choice(N, M, replace=False)).to(dev)]
         + 0.01 * torch.from_numpy(rng.standard_normal((M, D))).to(dev)).contiguous()
    Gq = torch.from_numpy(rng.standard_normal((M, M)) / M).to(dev)
    Gb = torch.from_numpy(rng.standard_normal((M, 1))).to(dev)
    return X, Y, Z, Gq, Gb


def composed(name, spec, X, Y, Z, Gq, Gb, need_dz):
    """the same (dvariance, dl, dZ) from k_dense + matmul + k_dense_vjp (+ k_grad_points)"""
    N, M = X.shape[0], Z.shape[0]
    G2 = Gq + Gq.t()
    rows = max(16, (256 << 20) // (8 * M))
    dv, dl = 0.0, np.zeros(spec.D)
    dZ = torch.zeros_like(Z) if need_dz else None
    for i0 in range(0, N, rows):
        Xp = X[i0:i0 + rows]
        W = torch.addmm(Y[i0:i0 + rows] @ Gb.t(), ops.k_dense(spec, Xp, Z), G2)
        v, l = ops.k_dense_vjp(spec, Xp, Z, W)
        dv, dl = dv + v, dl + np.asarray(l)
        if need_dz:
            dZ += training.k_grad_points(name, spec.variance, spec.lengthscales, Xp, Z, W)[1]
    return dv, list(dl), dZ


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def measure(args, dev):
    N, M = 1 << args.lg_n, args.m
    rows = []
    for D in [int(d) for d in args.dims.split(",")]:
        X, Y, Z, Gq, Gb = make(N, M, D, dev)
        for name in args.kernels.split(","):
            spec = ops.KernelSpec(name, VAR, list(np.sqrt(D) * np.linspace(0.8, 1.2, D)), D)
            fns = {"forward": lambda: (ops.kmn_knm(spec, X, Z), ops.kmn_matvec(spec, X, Z, Y)),
                   "vjp": lambda: ops.kmn_knm_vjp_anyd(spec, X, Z, Gq, Y, Gb, need_dZ=False),
                   "vjp_dz": lambda: ops.kmn_knm_vjp_anyd(spec, X, Z, Gq, Y, Gb, need_dZ=True),
                   "composed": lambda: composed(name, spec, X, Y, Z, Gq, Gb, False),
                   "composed_dz": lambda: composed(name, spec, X, Y, Z, Gq, Gb, True)}
            a, b = fns["vjp_dz"](), fns["composed_dz"]()
            row = {"kernel": name, "D": D, "N": N, "M": M, "rounds": args.rounds,
                   "rel_diff_to_composed": {"dvariance": rel(a[0], b[0]), "dl": rel(a[1], b[1]),
                                            "dZ": rel(a[2].cpu().numpy(), b[2].cpu().numpy())},
                   "times": alternated(fns, args.rounds)}
            t = {k: v["median_ms"] for k, v in row["times"].items()}
            row["vjp_over_composed"] = t["vjp"] / t["composed"]
            row["vjp_dz_over_composed_dz"] = t["vjp_dz"] / t["composed_dz"]
            row["vjp_dz_over_forward"] = t["vjp_dz"] / t["forward"]
            row["vjp_over_forward"] = t["vjp"] / t["forward"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def profile_child(args, dev):
    """two calls with dZ at the first dimension and kernel, for a kernel trace"""
    N, M, D = 1 << args.lg_n, args.m, int(args.dims.split(",")[0])
    name = args.kernels.split(",")[0]
    X, Y, Z, Gq, Gb = make(N, M, D, dev)
    spec = ops.KernelSpec(name, VAR, list(np.sqrt(D) * np.linspace(0.8, 1.2, D)), D)
    for _ in range(2):
        ops.kmn_knm_vjp_anyd(spec, X, Z, Gq, Y, Gb, need_dZ=True)
    torch.cuda.synchronize()


def stats_summary(pattern):
    """per-kernel totals of a rocprofv3 --kernel-trace --stats run of --profile-child (two calls)"""
    f = sorted(glob.glob(pattern, recursive=True))[0]
    out = []
    for r in csv.DictReader(open(f)):
        n = r["Name"].split("(anonymous namespace)::")[-1].split("(")[0][:72]
        out.append({"kernel": n, "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                    "percent": float(r["Percentage"])})
    return sorted(out, key=lambda r: -r["total_ms"])[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg-n", type=int, default=18)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--dims", default="77,90")
    ap.add_argument("--kernels", default="matern32,se")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--stats-summary", default=None)
    args = ap.parse_args()
    if args.stats_summary:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        res["kernel_split_two_calls_with_dz"] = stats_summary(args.stats_summary)
        print(json.dumps(res["kernel_split_two_calls_with_dz"], indent=1))
    else:
        dev = torch.device("cuda:0")
        if args.profile_child:
            return profile_child(args, dev)
        res = {"device": torch.cuda.get_device_name(0), "rows": measure(args, dev)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
