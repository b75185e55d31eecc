"""The three routes of the matrix-free exact-GPR operator (k(X, X) + s2 I) above 32 dimensions side by side: the plain
kind (`MGP_OP_KXX_NOISE`: kernel panels, csrc/generic.hip), the fused any-D sweep (`MGP_OP_KXX_NOISE_ANYD`, right-hand
sides in passes of 8, 4, 2, 1, csrc/sweep_anyd.hip) and the symmetric form (`MGP_OP_KXX_NOISE_SYM_ANYD`,
csrc/kxx_sym_anyd.hip), and the rule for `conjugate_gradient.sym_anyd_auto` that follows from the table.

    python tools/run_kxx_sym_anyd.py [--parts table,models] [--lg-n 14,16,17] [--dims 33,77,90,128,512]
                                     [--columns 1,5,8,16,32] [--rounds 3] [--row-seconds 0]
                                     [--out profiles/kxx_sym_anyd_times.json]

fp64, X ~ U(-3, 3)^(N x D), s2 = 0.1, lengthscale 3 sqrt(D / 8) in every dimension (r^2 as at the D = 8 configuration
of tools/run_kmm_wide.py); SE and Matern-3/2.  Per (N, D, kernel, columns): one application
(`KxxNoiseOperator.rmatmul`) by each route in one process, one warm-up each, then `--rounds` rounds with the routes
alternated; device events between two synchronisations; best, median and largest time.  `--row-seconds S` (0 = off)
lowers the rounds of a measurement, never below 2, when its warm-up says that `--rounds` of it would take longer than
S; the rounds taken are recorded.  A run merges its rows into `--out` (same N, D, kernel and columns replace), so the
table can be made in pieces.

rule: the regions (largest D, column range, smallest N) such that at EVERY measured point with D up to that one, a
column count in the range and at least that N the symmetric form's best time is at most 0.9 of the best time of the
FASTER of the two existing routes, for both kernels; of those, the one that admits the most measured points (ties: the
larger D, then the smaller N).  None: "auto" equals False.

models: at N = 2^16 and D = 77 (SE), one converged `GPR.solve` (threshold 1e-6) and one
`TrainableGPR(num_probes=15)` loss + backward, each with `sym_anyd=True`, `fused_anyd=True` and the default; one
warm-up and one timed run each.
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

from cggp import kernels  # noqa: E402
from cggp.conjugate_gradient import ConjugateGradient, KxxNoiseOperator  # noqa: E402

KERNELS = [("se", kernels.SquaredExponential), ("matern32", kernels.Matern32)]
ROUTES = {"plain": {}, "anyd": {"fused_anyd": True}, "sym_anyd": {"sym_anyd": True}}
MARGIN = 0.9


def lengthscale(D):
    return 3.0 * float(np.sqrt(D / 8.0))


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternated(fns, rounds, row_seconds):
    """{name: {best_ms, median_ms, max_ms}}, rounds taken: one timed warm-up each, then the routes in turn."""
    warm = sum(once(fn)[0] for fn in fns.values()) * 1e-3
    if row_seconds > 0 and warm * rounds > row_seconds:
        rounds = max(2, int(row_seconds / warm))
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(once(fn)[0])
    out = {name: {"best_ms": float(min(v)), "median_ms": float(np.median(v)), "max_ms": float(max(v))}
           for name, v in ms.items()}
    return out, rounds


def table_rows(args, dev):
    """Yields the rows as they are measured (the caller saves after each: a long run cut short keeps what it has)."""
    for lg in args.lg_n:
        N = 1 << lg
        for D in args.dims:
            for name, cls in KERNELS:
                rng = np.random.default_rng([lg, D])
                X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(dev)
                kern = cls(1.0, [lengthscale(D)] * D)
                ops_ = {r: KxxNoiseOperator(kern, X, 0.1, **kw) for r, kw in ROUTES.items()}
                for Bt in args.columns:
                    t0 = time.time()
                    P = torch.from_numpy(rng.standard_normal((Bt, N))).to(dev)
                    assert [op.kind_for(Bt) for op in ops_.values()] == [3, 7, 9]
                    ref = ops_["anyd"].rmatmul(P)
                    diff = float((ops_["sym_anyd"].rmatmul(P) - ref).abs().max() / ref.abs().max())
                    fns = {r: (lambda op=op: op.rmatmul(P)) for r, op in ops_.items()}
                    t, taken = alternated(fns, args.rounds, args.row_seconds)
                    fastest = min(t["plain"]["best_ms"], t["anyd"]["best_ms"])
                    row = {"kernel": name, "D": D, "lengthscale": lengthscale(D), "N": N, "columns": Bt,
                           "rel_diff_to_anyd": diff, "rounds": taken, "times": t,
                           "sym_anyd_over_plain": t["sym_anyd"]["best_ms"] / t["plain"]["best_ms"],
                           "sym_anyd_over_anyd": t["sym_anyd"]["best_ms"] / t["anyd"]["best_ms"],
                           "sym_anyd_over_fastest": t["sym_anyd"]["best_ms"] / fastest,
                           "row_seconds": time.time() - t0}
                    print(json.dumps(row), flush=True)
                    yield row
                    del P, ref
                del X, ops_
                torch.cuda.empty_cache()


def derive_rule(rows):
    """See the module docstring.  {"valid_regions": [...], "chosen": {"max_d", "min_columns", "max_columns", "N",
    "points"} or None}."""
    dims = sorted({r["D"] for r in rows})
    cols = sorted({r["columns"] for r in rows})
    sizes = sorted({r["N"] for r in rows})
    wins = lambda r: r["sym_anyd_over_fastest"] <= MARGIN
    valid = []
    for max_d in dims:
        for N in sizes:
            for i, lo in enumerate(cols):
                for hi in cols[i:]:
                    pts = [r for r in rows if r["D"] <= max_d and lo <= r["columns"] <= hi and r["N"] >= N]
                    if pts and all(wins(r) for r in pts):
                        valid.append({"max_d": max_d, "min_columns": lo, "max_columns": hi, "N": N, "points": len(pts)})
    chosen = max(valid, key=lambda v: (v["points"], v["max_d"], -v["N"])) if valid else None
    keep = [v for v in valid if not any(w is not v and w["max_d"] >= v["max_d"] and w["N"] <= v["N"]
                                        and w["min_columns"] <= v["min_columns"] and w["max_columns"] >= v["max_columns"]
                                        for w in valid)]
    return {"margin": MARGIN, "valid_regions": keep, "chosen": chosen}


def models_part(args, dev):
    from cggp.models import GPR
    from cggp.training import TrainableGPR
    N, D, s2 = 1 << 16, 77, 0.1
    ls = lengthscale(D)
    rng = np.random.default_rng(7)
    X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(dev)
    y = (torch.sin(X.sum(dim=1) / np.sqrt(D / 8.0)) + 0.1 * torch.from_numpy(rng.standard_normal(N)).to(dev))[:, None].contiguous()
    out = {"N": N, "D": D, "kernel": "se", "lengthscale": ls, "noise_variance": s2, "rounds": 1}
    solve, train = {}, {}
    ref = None
    for route, kw in ROUTES.items():
        kern = kernels.SquaredExponential(1.0, [ls] * D)
        m = GPR((X, y), kern, noise_variance=s2, conjugate_gradient=ConjugateGradient(1e-6, max_iterations=500),
                solver="cg", **kw)
        warm, _ = once(lambda: m.solve(y))
        ms, alpha = once(lambda: m.solve(y))
        ref = alpha if ref is None else ref
        solve[route] = {"warmup_ms": warm, "best_ms": ms, "rel_diff_to_plain": float((alpha - ref).abs().max() / ref.abs().max())}
        print(json.dumps({"GPR.solve": route, **solve[route]}), flush=True)
    for route, kw in ROUTES.items():
        def step():
            t = TrainableGPR(kernels.SquaredExponential(1.0, [ls] * D), s2, X, y, num_probes=15,
                             conjugate_gradient=ConjugateGradient(1e-6, max_iterations=500), **kw)
            loss = t.training_loss()
            loss.backward()
            return float(loss.detach())
        warm, _ = once(step)
        ms, loss = once(step)
        train[route] = {"warmup_ms": warm, "best_ms": ms, "loss": loss}
        print(json.dumps({"TrainableGPR": route, **train[route]}), flush=True)
    for name, t in (("GPR.solve", solve), ("TrainableGPR(num_probes=15) loss + backward", train)):
        out[name] = {"times": t, "sym_anyd_over_anyd": t["sym_anyd"]["best_ms"] / t["anyd"]["best_ms"],
                     "sym_anyd_over_plain": t["sym_anyd"]["best_ms"] / t["plain"]["best_ms"]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="table,models")
    ap.add_argument("--lg-n", type=ints, default=[14, 16, 17])
    ap.add_argument("--dims", type=ints, default=[33, 77, 90, 128, 512])
    ap.add_argument("--columns", type=ints, default=[1, 5, 8, 16, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--row-seconds", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kxx_sym_anyd_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "dtype": "float64",
                "timing": "device events between two device synchronisations; one warm-up per route, routes alternated; "
                          "best of the rounds each measurement records",
                "counters": "no counter run was made"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if "table" in args.parts:
        key = lambda r: (r["N"], r["D"], r["kernel"], r["columns"])
        merged = {key(r): r for r in res.get("rows", [])}
        for row in table_rows(args, dev):
            merged[key(row)] = row
            res["rows"] = [merged[k] for k in sorted(merged)]
            res["rule"] = derive_rule(res["rows"])
            save()
        print(json.dumps(res.get("rule")), flush=True)
    if "models" in args.parts:
        res["models"] = models_part(args, dev)
    save()


if __name__ == "__main__":
    main()
