"""Point gradients of a dense kernel block: `ops.k_dense_vjp_points` (include/mgp_points.h) against the torch route it
replaces (`ops.k_dense_vjp` + `training.k_grad_points`), and one loss + backward of the models that take it.

    python tools/run_kvjp_points.py [--rounds 5] [--out profiles/kvjp_points_times.json]
    python tools/run_kvjp_points.py --step op|cdgp|sgpr       (one step in this process; prints its JSON rows)

fp64, one GPU.  The driver runs every step in a fresh child process under a time limit of its own and stops at the
first one that fails.  In a step: HIP events around synchronised calls, one warm-up of every timed shape, the versions
alternated round by round within the process, median and (min, max) reported: boxes differ by a few per cent, only the
in-run ratios count.  No hardware-counter run is part of this tool.

steps   op     K_mm blocks [M, M] at M = 2048 .. 16384 (A is B) and K_mn blocks [4096, 256], [4096, 1000], for SE at
               D = 8, Matern-3/2 at D = 32 and Matern-3/2 at D = 77: all four outputs from one fused call against
               k_dense_vjp + k_grad_points on the same inputs; the largest difference between the routes relative to
               the largest entry
        cdgp   TrainableCGGP(trainable_inducing=True), dense, batch 1000, SE at D = 8, M = 2048 (the C2 training step)
               and M = 4096: one training_loss(batch).backward() with fused_point_grads off and on
        sgpr   TrainableSGPR(trainable_inducing=True), N = 2^18, M = 4096, SE at D = 8: the same
The "auto" entry of the output is the rule of `conjugate_gradient.fused_point_grads_auto`: the smallest measured block
(in pairs) and the largest measured D such that every measured point inside is at or below 0.9; None when there is none.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

STEP_LIMIT_S = {"op": 420, "cdgp": 240, "sgpr": 240}
CONFIGS = (("se", 8), ("matern32", 32), ("matern32", 77))
KMM = (2048, 4096, 8192, 16384)
KMN = ((4096, 256), (4096, 1000))


def once(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternated(torch, np, fns, rounds):
    """{name: {median_ms, min_ms, max_ms}}: one warm-up each, then `rounds` rounds with the versions in turn."""
    for fn in fns.values():
        fn()
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(once(torch, fn)[0])
    return {name: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
            for name, v in ms.items()}


def run_step(args):
    import numpy as np
    import torch

    from cggp import kernels, ops, training
    from cggp.conjugate_gradient import ConjugateGradient

    dev = torch.device("cuda:0")
    emit = lambda row: print(json.dumps(row), flush=True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())

    if args.step == "op":
        for name, D in CONFIGS:
            ls = [float(np.sqrt(D))] * D
            spec = ops.KernelSpec(name, 1.0, ls, D)
            for na, nb, same in [(M, M, True) for M in KMM] + [(a, b, False) for a, b in KMN]:
                g = torch.Generator().manual_seed(na + nb + D)
                A = torch.randn((na, D), generator=g, dtype=torch.float64).to(dev)
                B = A if same else torch.randn((nb, D), generator=g, dtype=torch.float64).to(dev)
                G = torch.randn((na, nb), generator=g, dtype=torch.float64).to(dev)

                def torch_route():
                    dv, dl = ops.k_dense_vjp(spec, A, B, G)
                    dA, dB = training.k_grad_points(name, 1.0, ls, A, B, G)
                    return dv, dl, dA, dB

                fns = {"fused": lambda: ops.k_dense_vjp_points(spec, A, B, G), "torch": torch_route}
                f, t = fns["fused"](), fns["torch"]()
                times = alternated(torch, np, fns, args.rounds)
                emit({"step": "op", "block": "K_mm" if same else "K_mn", "kernel": name, "D": D, "na": na, "nb": nb,
                      "rounds": args.rounds, "times": times, "fused_ms": times["fused"]["median_ms"],
                      "torch_ms": times["torch"]["median_ms"],
                      "ratio": times["fused"]["median_ms"] / times["torch"]["median_ms"],
                      "rel_diff": {"dvariance": abs(f[0] - t[0]) / abs(t[0]),
                                   "dlengthscales": float(np.max(np.abs(np.subtract(f[1], t[1]))) / np.max(np.abs(t[1]))),
                                   "dA": rel(f[2], t[2]), "dB": rel(f[3], t[3])}})
                del A, B, G, f, t
                torch.cuda.empty_cache()
        return

    g = torch.Generator().manual_seed(5)
    rand = lambda *s: (torch.rand(s, generator=g, dtype=torch.float64) * 6.0 - 3.0).to(dev)
    D = 8
    kern = lambda: kernels.SquaredExponential(variance=1.0, lengthscales=[3.0] * D)
    if args.step == "cdgp":
        B = 1000
        for M in (2048, 4096):
            Z, x = rand(M, D), rand(B, D)
            y = torch.randn((B, 1), generator=g, dtype=torch.float64).to(dev)
            u = torch.randn((M, 1), generator=g, dtype=torch.float64).to(dev)
            counts = torch.full((M, 1), 4.0, dtype=torch.float64, device=dev)
            probes = (2.0 * torch.randint(0, 2, (M, 5), generator=g) - 1.0).to(dtype=torch.float64, device=dev)

            def step(fused):
                m = training.TrainableCGGP(kern(), 0.1, Z, ConjugateGradient(1e-6, max_iterations=50), num_probes=5,
                                           pseudo_u=u, cluster_counts=counts, num_data=4 * M, trainable_inducing=True,
                                           fused_point_grads=fused)

                def run():
                    for p in m.parameters():
                        p.grad = None
                    loss = m.training_loss((x, y), probes=probes)
                    loss.backward()
                    return float(loss.detach()), m.Z.grad.clone()
                return run

            fns = {"torch": step(False), "fused": step(True)}
            (l0, z0), (l1, z1) = fns["torch"](), fns["fused"]()
            times = alternated(torch, np, fns, args.rounds)
            emit({"step": "cdgp", "model": "TrainableCGGP dense, trainable_inducing, data_term=batch", "kernel": "se",
                  "D": D, "M": M, "batch": B, "probes": 5, "cg": "threshold 1e-6, at most 50 steps",
                  "rounds": args.rounds, "times": times, "fused_ms": times["fused"]["median_ms"],
                  "torch_ms": times["torch"]["median_ms"],
                  "ratio": times["fused"]["median_ms"] / times["torch"]["median_ms"],
                  "loss_bit_identical": l0 == l1, "rel_diff_dZ": rel(z1, z0)})
        return
    if args.step == "sgpr":
        N, M = 1 << 18, 4096
        X, Z = rand(N, D), rand(M, D)
        Y = (torch.sin(X[:, :1]) + 0.1 * torch.randn((N, 1), generator=g, dtype=torch.float64).to(dev)).contiguous()

        def step(fused):
            m = training.TrainableSGPR(kern(), 0.1, X, Y, Z, trainable_inducing=True, fused_point_grads=fused)

            def run():
                for p in m.parameters():
                    p.grad = None
                loss = m.training_loss()
                loss.backward()
                return float(loss.detach()), m.Z.grad.clone()
            return run

        fns = {"torch": step(False), "fused": step(True)}
        (l0, z0), (l1, z1) = fns["torch"](), fns["fused"]()
        times = alternated(torch, np, fns, args.rounds)
        emit({"step": "sgpr", "model": "TrainableSGPR, trainable_inducing", "kernel": "se", "D": D, "N": N, "M": M,
              "rounds": args.rounds, "times": times, "fused_ms": times["fused"]["median_ms"],
              "torch_ms": times["torch"]["median_ms"],
              "ratio": times["fused"]["median_ms"] / times["torch"]["median_ms"],
              "loss_bit_identical": l0 == l1, "rel_diff_dZ": rel(z1, z0)})
        return
    raise SystemExit(f"unknown step {args.step!r}")


def auto_rule(op_rows):
    """the largest region {D <= max_d, na nb >= min_pairs} of the measured grid in which every point is <= 0.9"""
    ds = sorted({r["D"] for r in op_rows})
    pairs = sorted({r["na"] * r["nb"] for r in op_rows})
    best = None
    for max_d in ds:
        for min_pairs in pairs:
            inside = [r for r in op_rows if r["D"] <= max_d and r["na"] * r["nb"] >= min_pairs]
            if inside and all(r["ratio"] <= 0.9 for r in inside) and (best is None or len(inside) > best[0]):
                best = (len(inside), min_pairs, max_d)
    return {"min_pairs": best[1] if best else None, "max_d": best[2] if best else None,
            "rule": "fp64 device tensors, D <= max_d and na * nb >= min_pairs: every measured point inside is at or "
                    "below 0.9 of the torch route"}


def drive(args):
    """Every step in a child of its own, each under its time limit; the first failure ends the run."""
    rows, device = [], None
    for step in ("op", "cdgp", "sgpr"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} ran past its limit of {STEP_LIMIT_S[step]} s; nothing more is started")
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {step} failed with {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                if "device" in rec:
                    device = rec["device"]
                else:
                    rows.append(rec)
                    print(line, flush=True)
    op = [r for r in rows if r["step"] == "op"]
    res = {"device": device, "method": f"median of {args.rounds} (min, max kept), versions alternated in one process, HIP events; "
                                       "no hardware-counter run was made",
           "auto": auto_rule(op), "op": op, "models": [r for r in rows if r["step"] != "op"]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.step is None:
        return drive(args)
    import torch
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    run_step(args)


if __name__ == "__main__":
    main()
