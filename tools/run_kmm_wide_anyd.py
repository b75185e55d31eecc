"""The three routes of the matrix-free (K_mm + Lambda) operator above 32 dimensions side by side: the plain kind
(`MGP_OP_KMM_LAMBDA`: kernel panels, csrc/generic.hip), the fused any-D sweep (`MGP_OP_KMM_LAMBDA_ANYD`, right-hand sides
in passes of 8, csrc/sweep_anyd.hip) and the many-column form (`MGP_OP_KMM_LAMBDA_WIDE_ANYD`, csrc/kmm_wide_anyd.hip),
and the rule for `conjugate_gradient.wide_anyd_auto` that follows from the table.

    python tools/run_kmm_wide_anyd.py [--parts table,predict] [--lg-m 12,14,16] [--dims 33,77,90,128,512]
                                      [--columns 16,48,64,256] [--rounds 3] [--row-seconds 0]
                                      [--out profiles/kmm_wide_anyd_times.json]

fp64, Z ~ U(-3, 3)^(M x D), lambda ~ U(0.05, 0.15), lengthscale 3 sqrt(D / 8) in every dimension (r^2 as at the D = 8
configuration of tools/run_kmm_wide.py); SE and Matern-3/2.  Per (M, D, kernel, columns): one application
(`KmmLambdaOperator.rmatmul`) by each route in one process, one warm-up each, then `--rounds` rounds with the routes
alternated; device events between two synchronisations; best, median and largest time.  `--row-seconds S` (0 = off)
lowers the rounds of a measurement, never below 2, when its warm-up says that `--rounds` of it would take longer than
S; the rounds taken are recorded.  A run merges its rows into `--out` (same M, D, kernel and columns replace), so the
table can be made in pieces.

rule: the regions (largest D, fewest columns, smallest M) such that at EVERY measured point with D up to that one, at
least that many columns and at least that M the many-column form's best time is at most 0.9 of the best time of the
FASTER of the two existing routes, for both kernels; of those, the one that admits the most measured points (ties: the
larger D, then the smaller M).  None: "auto" equals False.

predict: `CGGP(matrix_free=True).predict_f_batched(shared_inverse=False)` at M = 2^14 and D = 77, 2^12 rows in batches
of 256, CG threshold 1e-6 capped at 50 steps, `wide_anyd` False and True, one warm-up and one timed run each.
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
from cggp.conjugate_gradient import ConjugateGradient, KmmLambdaOperator  # noqa: E402

KERNELS = [("se", kernels.SquaredExponential), ("matern32", kernels.Matern32)]
ROUTES = {"plain": {}, "anyd": {"fused_anyd": True}, "wide_anyd": {"wide_anyd": True}}
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
    for lg in args.lg_m:
        M = 1 << lg
        for D in args.dims:
            for name, cls in KERNELS:
                rng = np.random.default_rng([lg, D])
                Z = torch.from_numpy(rng.uniform(-3.0, 3.0, (M, D))).to(dev)
                lam = torch.from_numpy(rng.uniform(0.05, 0.15, M)).to(dev)
                kern = cls(1.0, [lengthscale(D)] * D)
                ops_ = {r: KmmLambdaOperator(kern, Z, lam, **kw) for r, kw in ROUTES.items()}
                for Bt in args.columns:
                    t0 = time.time()
                    P = torch.from_numpy(rng.standard_normal((Bt, M))).to(dev)
                    assert [op.kind_for(Bt) for op in ops_.values()] == [2, 6, 8]
                    ref = ops_["plain"].rmatmul(P)
                    diff = float((ops_["wide_anyd"].rmatmul(P) - ref).abs().max() / ref.abs().max())
                    fns = {r: (lambda op=op: op.rmatmul(P)) for r, op in ops_.items()}
                    t, taken = alternated(fns, args.rounds, args.row_seconds)
                    fastest = min(t["plain"]["best_ms"], t["anyd"]["best_ms"])
                    row = {"kernel": name, "D": D, "lengthscale": lengthscale(D), "M": M, "columns": Bt,
                           "rel_diff_to_plain": diff, "rounds": taken, "times": t,
                           "wide_anyd_over_plain": t["wide_anyd"]["best_ms"] / t["plain"]["best_ms"],
                           "wide_anyd_over_anyd": t["wide_anyd"]["best_ms"] / t["anyd"]["best_ms"],
                           "wide_anyd_over_fastest": t["wide_anyd"]["best_ms"] / fastest,
                           "row_seconds": time.time() - t0}
                    print(json.dumps(row), flush=True)
                    yield row
                    del P, ref
                del Z, lam, ops_
                torch.cuda.empty_cache()


def derive_rule(rows):
    """See the module docstring.  {"valid_regions": [...], "chosen": {"max_d", "columns", "M", "points"} or None}."""
    dims = sorted({r["D"] for r in rows})
    cols = sorted({r["columns"] for r in rows})
    sizes = sorted({r["M"] for r in rows})
    wins = lambda r: r["wide_anyd_over_fastest"] <= MARGIN
    valid = []
    for max_d in dims:
        for M in sizes:
            for c in cols:
                pts = [r for r in rows if r["D"] <= max_d and r["columns"] >= c and r["M"] >= M]
                if pts and all(wins(r) for r in pts):
                    valid.append({"max_d": max_d, "columns": c, "M": M, "points": len(pts)})
                    break  # the smallest width at this size; wider ones are implied
    chosen = max(valid, key=lambda v: (v["points"], v["max_d"], -v["M"])) if valid else None
    return {"margin": MARGIN, "valid_regions": valid, "chosen": chosen}


def predict_part(args, dev):
    from cggp.models import CGGP
    from cggp.optimize import nearest_centre_statistics
    M, N, rows, batch, D, s2 = 1 << 14, 1 << 16, 1 << 12, 256, 77, 0.1
    ls = lengthscale(D)
    rng = np.random.default_rng(7)
    X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(dev)
    y = (torch.sin(X.sum(dim=1) / np.sqrt(D / 8.0)) + 0.1 * torch.from_numpy(rng.standard_normal(N)).to(dev))[:, None].contiguous()
    Z = X[torch.from_numpy(rng.choice(N, M, replace=False)).to(dev)].contiguous()
    kern = kernels.SquaredExponential(1.0, [ls] * D)
    _, sums, counts = nearest_centre_statistics(kern, Z, (X, y))
    counts = counts.clamp(min=1.0)
    u = (sums / counts)[:, None].contiguous()
    models = {w: CGGP(kern, s2, Z, ConjugateGradient(1e-6, max_iterations=50), num_probes=5, pseudo_u=u,
                      cluster_counts=counts[:, None].contiguous(), num_data=N, matrix_free=True, wide_anyd=w)
              for w in (False, True)}
    xs = X[:rows].contiguous()
    fns = {("wide_anyd" if w else "plain"): (lambda m=m: m.predict_f_batched(xs, batch, shared_inverse=False))
           for w, m in models.items()}
    warm = {name: once(fn) for name, fn in fns.items()}
    (mu_s, var_s), (mu_w, var_w) = warm["plain"][1], warm["wide_anyd"][1]
    t = {name: {"warmup_ms": warm[name][0], "best_ms": once(fn)[0]} for name, fn in fns.items()}
    out = {"M": M, "rows": rows, "batch": batch, "kernel": "se", "D": D, "lengthscale": ls, "threshold": 1e-6,
           "max_iterations": 50, "rounds": 1, "times": t,
           "wide_anyd_over_plain": t["wide_anyd"]["best_ms"] / t["plain"]["best_ms"],
           "mean_abs_diff": float((mu_w - mu_s).abs().max()), "variance_abs_diff": float((var_w - var_s).abs().max())}
    print(json.dumps(out), flush=True)
    return out


def main():
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="table,predict")
    ap.add_argument("--lg-m", type=ints, default=[12, 14, 16])
    ap.add_argument("--dims", type=ints, default=[33, 77, 90, 128, 512])
    ap.add_argument("--columns", type=ints, default=[16, 48, 64, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--row-seconds", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmm_wide_anyd_times.json"))
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
        key = lambda r: (r["M"], r["D"], r["kernel"], r["columns"])
        merged = {key(r): r for r in res.get("rows", [])}
        for row in table_rows(args, dev):
            merged[key(row)] = row
            res["rows"] = [merged[k] for k in sorted(merged)]
            res["rule"] = derive_rule(res["rows"])
            save()
        print(json.dumps(res.get("rule")), flush=True)
    if "predict" in args.parts:
        res["predict_f_batched"] = predict_part(args, dev)
    save()


if __name__ == "__main__":
    main()
