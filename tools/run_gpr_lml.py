"""Matrix-free exact-GPR marginal likelihood: one estimate plus gradient (`TrainableGPR(num_probes=15)`), and the pair
kernel of the hyper-parameter bilinear forms (`mgp_kxx_grad`, csrc/kxx_grad.hip) on its own.

    python tools/run_gpr_lml.py [--sizes 15,17] [--reps 3] [--out profiles/gpr_lml_times.json]

SE, D = 8, fp64, 15 probes (16 columns: y and the probes), noise 0.1, ConjugateGradient(1e-6).  The kernel alone runs
with R = 16; its issue fraction uses the static instruction count per pair of DESIGN 4.11.  Kernel times from a
separate `rocprofv3 --kernel-trace --stats` run of this tool.
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

from cggp import kernels, ops, training  # noqa: E402
from cggp.conjugate_gradient import ConjugateGradient  # noqa: E402

NUM_SIMDS, CLOCK_HZ = 1024, 2.4e9  # MI355X: 256 CUs x 4 SIMDs; one fp64 wave-instruction holds a SIMD 4 cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="15,17")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--instr-per-pair", type=float, default=0.0, help="static fp64 VALU instructions per pair (DESIGN 4.11)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpr_lml_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    D, R = 8, 16
    res = {"device": torch.cuda.get_device_name(0), "D": D, "kernel": "se", "probes": 15, "noise": 0.1,
           "threshold": 1e-6, "sizes": []}
    for lg in [int(s) for s in args.sizes.split(",")]:
        N = 1 << lg
        rng = np.random.default_rng(lg)
        X = torch.from_numpy(rng.standard_normal((N, D))).to(dev)
        Y = torch.sin(X[:, :1]) + 0.3 * torch.from_numpy(rng.standard_normal((N, 1))).to(dev)
        U, V = (torch.from_numpy(rng.standard_normal((N, R))).to(dev) for _ in range(2))
        spec = ops.KernelSpec("se", 1.0, [2.0] * D, D)
        ops.kxx_grad(spec, X, U, V)  # warm-up (arena)
        kt = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.kxx_grad(spec, X, U, V)  # synchronises
            kt.append((time.perf_counter() - t0) * 1e3)
        pairs = N * (N + 1) / 2
        ms = float(np.median(kt))
        row = {"N": N, "kxx_grad_ms": kt, "kxx_grad_median_ms": ms, "pairs": pairs}
        if args.instr_per_pair > 0:
            busy_s = pairs * args.instr_per_pair / 64 * 4 / (NUM_SIMDS * CLOCK_HZ)
            row["instr_per_pair"] = args.instr_per_pair
            row["fp64_issue_fraction"] = busy_s / (ms * 1e-3)
        m = training.TrainableGPR(kernels.SquaredExponential(1.0, [2.0] * D), 0.1, X, Y, num_probes=15,
                                  conjugate_gradient=ConjugateGradient(1e-6))
        ev = []
        for _ in range(args.reps):
            for p in m.parameters():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = m.training_loss()
            t1 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ev.append({"forward_ms": (t1 - t0) * 1e3, "backward_ms": (t2 - t1) * 1e3, "loss": loss.item()})
        est = m.frozen_model().log_marginal_likelihood_estimate(probes=m.probes)
        row.update(evaluations=ev, cg_iterations=est.iterations, converged=est.converged, std_error=est.std_error,
                   ms_per_cg_step=float(np.median([e["forward_ms"] for e in ev])) / max(1, est.iterations))
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
