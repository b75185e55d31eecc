"""Symmetric self-product (mgp_kxx_matvec, csrc/kxx.hip) against the plain self-sweep (mgp_knm_matvec(X, X) + s2 V),
timed in the same process, alternating, with HIP events around synchronised work; and one converged GPR CG solve.

    python tools/run_gpr.py [--sizes 15,17,20] [--reps 3] [--out profiles/gpr_times.json]

SE, D = 8, fp64, R in {1, 8}.  The handle runs with MGP_KXX=sym (the symmetric kernel at every size, so the small sizes
measure where the dispatch threshold belongs).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run
of this tool.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

os.environ["MGP_KXX"] = "sym"  # read when the handle is created

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import kernels, ops  # noqa: E402
from cggp.conjugate_gradient import ConjugateGradient, KxxNoiseOperator  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,15,16,17,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-n", type=int, default=1 << 17)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpr_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    D, s2 = 8, 0.1
    rng = np.random.default_rng(0)
    kern = kernels.SquaredExponential(1.0, [1.5] * D)
    spec = kern.spec(D)
    rows = []
    for lg in [int(s) for s in args.sizes.split(",")]:
        N = 1 << lg
        X = torch.from_numpy(rng.standard_normal((N, D))).to(dev)
        for R in (1, 8):
            V = torch.from_numpy(rng.standard_normal((N, R))).to(dev)
            sym = lambda: ops.kxx_matvec(spec, X, s2, V)  # noqa: E731
            plain = lambda: ops.knm_matvec(spec, X, X, V).add_(V, alpha=s2)  # noqa: E731
            reps = args.reps if lg < 20 else max(1, args.reps - 1)
            timed(sym, 1)  # warm-up: code objects, workspace arenas
            timed(plain, 1)
            ts, tp = [], []
            for _ in range(reps):  # alternating
                ts += timed(sym, 1)
                tp += timed(plain, 1)
            err = float(torch.linalg.norm(sym() - plain()) / torch.linalg.norm(plain()))
            pairs_sym = N * (N + 1) / 2  # diagonal tiles are evaluated whole: a few % more at N = 2^15
            row = dict(N=N, R=R, D=D, kind="se", dtype="fp64", sym_ms=ts, plain_ms=tp, sym_ms_median=float(np.median(ts)),
                       plain_ms_median=float(np.median(tp)), ratio=float(np.median(ts) / np.median(tp)),
                       rel_diff=err, ordered_pairs_per_s_plain=N * N / (np.median(tp) * 1e-3),
                       unordered_pairs_per_s_sym=pairs_sym / (np.median(ts) * 1e-3))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del V
        del X
    # one converged GPR solve (alpha = (K + s2 I)^-1 y) through the device CG on MGP_OP_KXX_NOISE
    N = args.solve_n
    X = torch.from_numpy(rng.uniform(-3, 3, (N, D))).to(dev)
    y = torch.sin(X.sum(dim=1, keepdim=True)) + 0.1 * torch.from_numpy(rng.standard_normal((N, 1))).to(dev)
    cg = ConjugateGradient(1e-8, max_iterations=5000)
    op = KxxNoiseOperator(kern, X, s2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol, stats = cg.solve_with_stats(op, y)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    r = y - (ops.knm_matvec(spec, X, X, sol) + s2 * sol)
    solve = dict(N=N, D=D, kind="se", s2=s2, threshold=1e-8, iterations=int(stats[0]), seconds=sec,
                 true_half_residual_sq=float(0.5 * (r * r).sum()))
    print(json.dumps(solve), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), products=rows, gpr_cg_solve=solve)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
