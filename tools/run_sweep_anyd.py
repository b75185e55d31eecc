"""The fused any-D sweeps (include/mgp_sweep_anyd.h) against the panel route of the plain names, timed in one run.

    python tools/run_sweep_anyd.py [--lg-n 18] [--m 4096] [--dims 33,48,77,90,128,512] [--kernels se,matern32]
                                   [--columns 1,5,8] [--rounds 5] [--out profiles/sweep_anyd_times.json]
    python tools/run_sweep_anyd.py --step sweeps --dims 77 ...        (one step in this process; prints its JSON rows)

fp64, X ~ U(-2, 2)^(N x D), Z a perturbed sample of X, lengthscales sqrt(D) * linspace(0.8, 1.2).  The driver runs
every step in a fresh child process under a time limit of its own and stops at the first one that fails.  In a step:
HIP events around synchronised calls, one warm-up of every timed shape, the two routes alternated round by round
within the process, median and (min, max) reported: boxes differ by a few per cent, only the in-run ratios count.

steps   sweeps      K_nm V (`knm`) and K_mn W (`kmn`) at N x M, per dimension, kernel and column count:
                    fused = ops.k*_matvec_anyd, panel = ops.k*_matvec (the parent's code), and their largest difference
        kmm_lambda  one (K_mm + Lambda) application at M = 2^14 (operator kinds 6 and 2), 8 right-hand sides
        sgpr_step   one application of the SGPR operator (kinds 5 and 1), one right-hand side: the two sweeps of a CG step
        gpr_matvec  one (K_xx + s2 I) application at N = 2^16, D = 77 (kinds 7 and 3), one right-hand side
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

VAR = 1.2
STEP_LIMIT_S = {"sweeps": 240, "kmm_lambda": 180, "sgpr_step": 180, "gpr_matvec": 180}


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


def finish(row, times):
    row["times"] = times
    row["fused_over_panel"] = times["fused"]["median_ms"] / times["panel"]["median_ms"]
    print(json.dumps(row), flush=True)
    return row


def run_step(args):
    import numpy as np
    import torch

    from cggp import kernels, ops
    from cggp.conjugate_gradient import KmmLambdaOperator, KxxNoiseOperator, SgprNormalOperator

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    N, M = 1 << args.lg_n, args.m
    names = args.kernels.split(",")
    kcls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32, "matern12": kernels.Matern12,
            "matern52": kernels.Matern52}

    def ls_of(D):
        return list(np.sqrt(D) * np.linspace(0.8, 1.2, D))

    def points(n, m, D):
        X = torch.from_numpy(rng.uniform(-2.0, 2.0, (n, D))).to(dev)
        Z = (X[torch.from_numpy(rng.choice(n, m, replace=False)).to(dev)]
             + 0.01 * torch.from_numpy(rng.standard_normal((m, D))).to(dev)).contiguous()
        return X, Z

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    rows = []
    if args.step == "sweeps":
        for D in [int(d) for d in args.dims.split(",")]:
            X, Z = points(N, M, D)
            for name in names:
                spec = ops.KernelSpec(name, VAR, ls_of(D), D)
                for R in [int(r) for r in args.columns.split(",")]:
                    V = torch.from_numpy(rng.standard_normal((M, R))).to(dev)
                    W = torch.from_numpy(rng.standard_normal((N, R)) / np.sqrt(N)).to(dev)
                    for what, fused, panel, arg in (("knm", ops.knm_matvec_anyd, ops.knm_matvec, V),
                                                    ("kmn", ops.kmn_matvec_anyd, ops.kmn_matvec, W)):
                        fns = {"fused": lambda: fused(spec, X, Z, arg), "panel": lambda: panel(spec, X, Z, arg)}
                        row = {"step": "sweeps", "product": what, "kernel": name, "D": D, "N": N, "M": M, "R": R,
                               "rounds": args.rounds, "rel_diff_to_panel": rel(fns["fused"](), fns["panel"]())}
                        rows.append(finish(row, alternated(torch, np, fns, args.rounds)))
    elif args.step == "kmm_lambda":
        Mk, D, Bt = 1 << 14, 77, 8
        _, Z = points(Mk, Mk, D)
        lam = torch.from_numpy(rng.random(Mk) + 0.5).to(dev)
        P = torch.from_numpy(rng.standard_normal((Bt, Mk))).to(dev)
        for name in names:
            kern = kcls[name](VAR, ls_of(D))
            ops_ = {"fused": KmmLambdaOperator(kern, Z, lam, fused_anyd=True), "panel": KmmLambdaOperator(kern, Z, lam)}
            fns = {k: (lambda o=o: o.rmatmul(P)) for k, o in ops_.items()}
            row = {"step": "kmm_lambda", "kernel": name, "D": D, "M": Mk, "R": Bt, "rounds": args.rounds,
                   "rel_diff_to_panel": rel(fns["fused"](), fns["panel"]())}
            rows.append(finish(row, alternated(torch, np, fns, args.rounds)))
    elif args.step == "sgpr_step":
        for D in (77, 90):
            X, Z = points(N, M, D)
            P = torch.from_numpy(rng.standard_normal((1, M))).to(dev)
            for name in names:
                kern = kcls[name](VAR, ls_of(D))
                ops_ = {"fused": SgprNormalOperator(kern, X, Z, 0.1, jitter=1e-6, fused_anyd=True),
                        "panel": SgprNormalOperator(kern, X, Z, 0.1, jitter=1e-6)}
                fns = {k: (lambda o=o: o.rmatmul(P)) for k, o in ops_.items()}
                row = {"step": "sgpr_step", "kernel": name, "D": D, "N": N, "M": M, "R": 1, "rounds": args.rounds,
                       "rel_diff_to_panel": rel(fns["fused"](), fns["panel"]())}
                rows.append(finish(row, alternated(torch, np, fns, args.rounds)))
    elif args.step == "gpr_matvec":
        Ng, D = 1 << 16, 77
        X, _ = points(Ng, 1, D)
        P = torch.from_numpy(rng.standard_normal((1, Ng))).to(dev)
        for name in names:
            kern = kcls[name](VAR, ls_of(D))
            ops_ = {"fused": KxxNoiseOperator(kern, X, 0.1, fused_anyd=True), "panel": KxxNoiseOperator(kern, X, 0.1)}
            fns = {k: (lambda o=o: o.rmatmul(P)) for k, o in ops_.items()}
            row = {"step": "gpr_matvec", "kernel": name, "D": D, "N": Ng, "R": 1, "rounds": args.rounds,
                   "rel_diff_to_panel": rel(fns["fused"](), fns["panel"]())}
            rows.append(finish(row, alternated(torch, np, fns, args.rounds)))
    else:
        raise SystemExit(f"unknown step {args.step!r}")
    return rows


def drive(args):
    """Every step in a child of its own, each under its time limit; the first failure ends the run."""
    common = ["--lg-n", str(args.lg_n), "--m", str(args.m), "--kernels", args.kernels, "--columns", args.columns,
              "--rounds", str(args.rounds)]
    steps = [("sweeps", ["--dims", d]) for d in args.dims.split(",")]
    steps += [(s, []) for s in ("kmm_lambda", "sgpr_step", "gpr_matvec")]
    rows, device = [], None
    for step, extra in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + common + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} {extra} ran past its limit of {STEP_LIMIT_S[step]} s; nothing more is started")
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {step} {extra} failed with {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                if "device" in rec:
                    device = rec["device"]
                else:
                    rows.append(rec)
                    print(line, flush=True)
    res = {"device": device, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg-n", type=int, default=18)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--dims", default="33,48,77,90,128,512")
    ap.add_argument("--kernels", default="se,matern32")
    ap.add_argument("--columns", default="1,5,8")
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
