"""One SGPR value-and-gradient evaluation (`training.TrainableSGPR` with trainable Z), split into its parts, and the
N-sized VJP (`mgp_kmn_knm_vjp`, csrc/kmn_grad.hip) against the forward contraction (`mgp_kmn_knm`) at the same shape.

    python tools/run_sgpr_train.py [--configs C3,C5] [--reps 2] [--out profiles/sgpr_train_times.json]

C3: N = 2^20, M = 4096, D = 8, SE.  C5: N = 2^20, M = 4096, D = 32, Matern-3/2.  fp64.  Parts: the forward
mgp_kmn_knm (with K_mn y), the [M, M] algebra (bound value + adjoints), the Kmm VJPs (mgp_k_dense_vjp + the Z
expression), mgp_kmn_knm_vjp (with dZ).  Each part is timed on its own between device synchronisations; the best of
`reps` is kept.  Kernel times from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import ops, training  # noqa: E402

CONFIGS = {"C3": (1 << 20, 4096, 8, "se"), "C5": (1 << 20, 4096, 32, "matern32")}


def timed(fn, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgpr_train_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float64", "configs": []}
    for name in args.configs.split(","):
        N, M, D, kind = CONFIGS[name]
        rng = np.random.default_rng(0)
        X = torch.from_numpy(rng.uniform(-1.0, 1.0, (N, D))).to(dev)
        Y = torch.from_numpy(np.sin(3.0 * rng.uniform(-1.0, 1.0, (N, 1)))).to(dev)
        Z = X[torch.from_numpy(rng.choice(N, M, replace=False)).to(dev)].clone()
        ls = [0.5 * np.sqrt(D)] * D
        spec = ops.KernelSpec(kind, 1.0, ls, D)
        Kmm_j = ops.k_dense(spec, Z, Z, jitter=1e-6)
        s2, var = torch.tensor(0.1, dtype=torch.float64, device=dev), torch.tensor(1.0, dtype=torch.float64, device=dev)

        def forward():
            Q = ops.kmn_knm(spec, X, Z)
            b = ops.kmn_matvec(spec, X, Z, Y)
            return Q, b, ops.dot_all(Y, Y)

        t_fwd, (Q, b, yy) = timed(forward, args.reps)
        t_mm, adj = timed(lambda: training.sgpr_bound_adjoints(Kmm_j, Q, b, yy, s2, var, N), args.reps)
        _, Gq, Gb, GK, _, _ = adj
        t_kmm, _ = timed(lambda: (ops.k_dense_vjp(spec, Z, Z, GK),
                                  training.kmm_grad_z(kind, 1.0, ls, Z, GK)), args.reps)
        t_vjp, _ = timed(lambda: ops.kmn_knm_vjp(spec, X, Z, Gq.contiguous(), Y, Gb.contiguous(), need_dZ=True),
                         args.reps)
        t_knm, _ = timed(lambda: ops.kmn_knm(spec, X, Z), args.reps)
        flop = 2.0 * N * M * M
        row = {"config": name, "N": N, "M": M, "D": D, "kernel": kind,
               "forward_kmn_knm_and_kmn_y_ms": t_fwd, "mm_algebra_ms": t_mm, "kmm_vjps_ms": t_kmm,
               "kmn_knm_vjp_ms": t_vjp, "kmn_knm_alone_ms": t_knm,
               "total_ms": t_fwd + t_mm + t_kmm + t_vjp, "vjp_over_kmn_knm": t_vjp / t_knm,
               "vjp_gemm_tflops": flop / (t_vjp * 1e-3) / 1e12}
        print(json.dumps(row), flush=True)
        res["configs"].append(row)
        del Q, b, Gq, Gb, GK, Kmm_j, X, Y, Z
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
