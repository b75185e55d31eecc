"""The random-Fourier-feature prior draw and its backward pass above 32 dimensions: the fused any-D kernels
(MGP_RFF_ANYD, csrc/rff_anyd.hip) beside the routes taken without the flag -- feature panels and a GEMM forward
(`sample_panel_t`, csrc/rff.hip), `training._rff_vjp_panels` backward -- and the rule for `rff.rff_anyd_auto` that
follows from the table.

    python tools/run_rff_anyd.py [--parts kernel,paths] [--ops forward,dtheta,dX] [--dims 77,90,...] [--samples 5,1,8]
                                 [--bases 1024,256,4096] [--lg-n 17,14,20] [--rounds 3] [--row-seconds 0]
                                 [--budget-seconds 0] [--out profiles/rff_anyd_times.json]
    python tools/run_rff_anyd.py --derive          # no GPU: the rule from the rows already in --out

kernel: fp64, X ~ N(0, 1)^(N x D), theta ~ N(0, 1 / D)^(L x D) (phases of order 1), W and the cotangent G standard
normal, scale sqrt(1 / L).  Per (op, N, D, L, S) the old and the new route run in one process: one warm-up each, then
`--rounds` rounds with the routes alternated; device events between two synchronisations; the best time per route,
the slower route's slowest round over its best, and the largest difference of the two results relative to the
largest entry.  The grid is walked in the order given (N outermost, then D, L, S, op), a row is saved as soon as it is
measured and a run merges into `--out`, so the
table can be made in pieces; `--budget-seconds` stops before the next row once that much time is spent, and
`--row-seconds` lowers the rounds of a slow row (never below 1; the rounds taken are recorded).  dX is what the
parent route does for the inducing inputs: `_rff_vjp_panels(want_dX=True)`, which forms dtheta as well.

rule, per op and sample count S: the pairs (largest D, smallest N L) such that at EVERY measured point with that op
and S, D up to that one and N L at least that one the new route's best time is at most 0.9 of the old route's; of
those the one that admits the most measured points (ties: the larger D, then the smaller N L).  None: "auto" equals
False for that op and S.

paths: one `PathwiseClusterGP.pathwise_samples` call and one `TrainableCGGP(data_term="pathwise")` loss + backward at
N = 2^18, M = 4096, L = 1024, S = 5, SE at D = 77 and 90 (lengthscale 3 sqrt(D / 8)), dense and `matrix_free=True`, CG
threshold 1e-6 capped at 50 steps; `rff_anyd` False and True alternated.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

MARGIN = 0.9
OPS = ("forward", "dtheta", "dX")


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternated(fns, rounds, row_seconds):
    """({name: {best_ms, median_ms, max_ms}}, rounds taken, {name: warm-up result})"""
    warm = {name: once(fn) for name, fn in fns.items()}
    spent = sum(w[0] for w in warm.values()) * 1e-3
    if row_seconds > 0 and spent * rounds > row_seconds:
        rounds = max(1, int(row_seconds / spent))
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(once(fn)[0])
    out = {name: {"best_ms": float(min(v)), "median_ms": float(np.median(v)), "max_ms": float(max(v))}
           for name, v in ms.items()}
    return out, rounds, {name: w[1] for name, w in warm.items()}


def compact(t):
    """{name: [best_ms, median_ms, max_ms]}, rounded to 0.1 us: what a row keeps of `alternated`'s times"""
    return {name: [round(v[k], 4) for k in ("best_ms", "median_ms", "max_ms")] for name, v in t.items()}


def ratio(t):
    return round(t["new"][0] / t["old"][0], 4)


# old_ms, new_ms: the best of the rounds; worst_over_best: the larger of the two routes' slowest round / best round
COLUMNS = ["op", "N", "D", "L", "S", "rounds", "old_ms", "new_ms", "worst_over_best", "rel_diff_to_old", "new_over_old"]


def load(path):
    """The document at `path` ({} if there is none), its table rows as dicts"""
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        res = json.load(f)
    res["rows"] = [dict(zip(COLUMNS, r)) for r in res.get("rows", [])]
    res.pop("columns", None)
    return res


def dump(res, f):
    """JSON with one measured row per line; the table rows as arrays in the order of `columns`"""
    head = {k: v for k, v in res.items() if k not in ("rows", "paths")}
    head["columns"] = COLUMNS
    text = json.dumps(head, indent=1)[:-2]
    rows = [[r[c] for c in COLUMNS] for r in res.get("rows", [])]
    for key, lines in (("rows", rows), ("paths", res.get("paths"))):
        if lines:
            text += ',\n "%s": [\n' % key + ",\n".join("  " + json.dumps(r) for r in lines) + "\n ]"
    f.write(text + "\n}\n")


def kernel_rows(args, deadline):
    import torch

    from cggp import ops
    from cggp.training import _rff_vjp_panels
    dev = torch.device("cuda:0")
    for lg in args.lg_n:
        N = 1 << lg
        for D in args.dims:
            g = torch.Generator().manual_seed(1000 * lg + D)
            X = torch.randn((N, D), generator=g, dtype=torch.float64).to(dev)
            for L in args.bases:
                theta = (torch.randn((L, D), generator=g, dtype=torch.float64) / np.sqrt(D)).to(dev)
                scale = float(np.sqrt(1.0 / L))
                for S in args.samples:
                    W = torch.randn((S, 2 * L), generator=g, dtype=torch.float64).to(dev)
                    G = torch.randn((S, N), generator=g, dtype=torch.float64).to(dev)
                    for op in args.ops:
                        if deadline is not None and time.time() > deadline:
                            return
                        if op == "forward":
                            fns = {"old": lambda: ops.rff_sample(X, theta, W, scale),
                                   "new": lambda: ops.rff_sample(X, theta, W, scale, anyd=True)}
                        elif op == "dtheta":
                            fns = {"old": lambda: _rff_vjp_panels(X, theta, W, scale, G)[0],
                                   "new": lambda: ops.rff_sample_vjp(X, theta, W, scale, G, anyd=True)[0]}
                        else:
                            fns = {"old": lambda: _rff_vjp_panels(X, theta, W, scale, G, want_dX=True)[1],
                                   "new": lambda: ops.rff_sample_vjp(X, theta, W, scale, G, want_dtheta=False,
                                                                     want_dX=True, anyd=True)[1]}
                        t, taken, res = alternated(fns, args.rounds, args.row_seconds)
                        diff = float((res["new"] - res["old"]).abs().max() / res["old"].abs().max())
                        del res
                        t = compact(t)
                        row = {"op": op, "N": N, "D": D, "L": L, "S": S, "rounds": taken, "old_ms": t["old"][0],
                               "new_ms": t["new"][0], "worst_over_best": round(max(v[2] / v[0] for v in t.values()), 3),
                               "rel_diff_to_old": float("%.2g" % diff), "new_over_old": ratio(t)}
                        print(json.dumps(row), flush=True)
                        yield row
                    del W, G
                del theta
            del X
            torch.cuda.empty_cache()


def derive_rule(rows):
    """See the module docstring.  {"margin", "regions": {"op S": {"max_d", "min_nl", "points"} or None}}."""
    regions = {}
    for op in OPS:
        for S in sorted({r["S"] for r in rows if r["op"] == op}):
            mine = [r for r in rows if r["op"] == op and r["S"] == S]
            valid = []
            for max_d in sorted({r["D"] for r in mine}):
                for nl in sorted({r["N"] * r["L"] for r in mine}):
                    pts = [r for r in mine if r["D"] <= max_d and r["N"] * r["L"] >= nl]
                    if pts and all(r["new_over_old"] <= MARGIN for r in pts):
                        valid.append({"max_d": max_d, "min_nl": nl, "points": len(pts)})
                        break  # the smallest N L at this D; larger ones are implied
            regions[f"{op} {S}"] = (max(valid, key=lambda v: (v["points"], v["max_d"], -v["min_nl"]))
                                    if valid else None)
    return {"margin": MARGIN, "regions": regions}


def auto_table(rule):
    """`rff.RFF_ANYD_AUTO` as the rule gives it: {(op, S): (max_d, min_nl)}."""
    out = {}
    for key, reg in rule["regions"].items():
        if reg is not None:
            op, S = key.split()
            out[(op, int(S))] = (reg["max_d"], reg["min_nl"])
    return out


def paths_part(args):
    import torch

    import run_cdgp_full as rf
    from cggp import kernels
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import PathwiseClusterGP, rademacher
    from cggp.training import TrainableCGGP
    N, M, L, S = 1 << args.paths_lg_n, 4096, 1024, 5
    rows = []
    for D in (77, 90):
        ls = 3.0 * float(np.sqrt(D / 8.0))
        Z, x, y, u, counts = rf.inputs(N, M, D, 7 + D)
        kern = kernels.SquaredExponential(variance=1.0, lengthscales=[ls] * D)
        gps = {a: PathwiseClusterGP(kern, 0.1, Z, pseudo_u=u, cluster_counts=counts, rff_anyd=a,
                                    conjugate_gradient=ConjugateGradient(1e-6, max_iterations=50))
               for a in (False, True)}
        fns = {("new" if a else "old"): (lambda gp=gp: gp.pathwise_samples(x, L, S, seed=3)) for a, gp in gps.items()}
        t, taken, res = alternated(fns, args.rounds, args.row_seconds)
        t = compact(t)
        row = {"path": "PathwiseClusterGP.pathwise_samples", "D": D, "N": N, "M": M, "L": L, "S": S, "rounds": taken,
               "ms": t, "new_over_old": ratio(t),
               "rel_diff_to_old": float("%.2g" % float((res["new"] - res["old"]).abs().max() / res["old"].abs().max()))}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del res, gps
        probes = rademacher((M, 5), torch.float64, Z.device, 0)
        for mf in (False, True):
            ms = {a: TrainableCGGP(kern, 0.1, Z, ConjugateGradient(1e-6, max_iterations=50), num_probes=5, pseudo_u=u,
                                   cluster_counts=counts, num_data=N, matrix_free=mf, data_term="pathwise",
                                   num_bases=L, num_samples=S, rff_anyd=a) for a in (False, True)}
            draw = tuple(t_.to(Z.device) for t_ in ms[False].draw_pathwise(0))

            def step(m):
                for p in m.parameters():
                    p.grad = None
                loss = m.training_loss((x, y), probes=probes, pathwise=draw)
                loss.backward()
                return float(loss.detach())

            fns = {("new" if a else "old"): (lambda m=m: step(m)) for a, m in ms.items()}
            t, taken, res = alternated(fns, args.rounds, args.row_seconds)
            t = compact(t)
            row = {"path": "TrainableCGGP(data_term='pathwise') loss + backward", "matrix_free": mf, "D": D, "N": N,
                   "M": M, "L": L, "S": S, "rounds": taken, "ms": t, "new_over_old": ratio(t),
                   "loss_rel_diff": float("%.2g" % (abs(res["new"] - res["old"]) / abs(res["old"])))}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del ms
        del Z, x, y, u, counts
        torch.cuda.empty_cache()
    return rows


def main():
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,paths")
    ap.add_argument("--ops", type=lambda s: s.split(","), default=list(OPS))
    ap.add_argument("--dims", type=ints, default=[77, 90, 33, 48, 128, 256, 257, 512])
    ap.add_argument("--samples", type=ints, default=[5, 1, 8])
    ap.add_argument("--bases", type=ints, default=[1024, 256, 4096])
    ap.add_argument("--lg-n", type=ints, default=[17, 14, 20])
    ap.add_argument("--paths-lg-n", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--row-seconds", type=float, default=0.0)
    ap.add_argument("--budget-seconds", type=float, default=0.0)
    ap.add_argument("--derive", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rff_anyd_times.json"))
    args = ap.parse_args()
    res = load(args.out)
    if args.derive:
        rule = derive_rule(res.get("rows", []))
        print(json.dumps(rule, indent=1))
        print("RFF_ANYD_AUTO =", auto_table(rule))
        return
    import torch
    res.update({"device": torch.cuda.get_device_name(0), "dtype": "float64",
                "timing": "device events between two device synchronisations; one warm-up per route, routes "
                          "alternated; best of the rounds each measurement records",
                "old": "the call without MGP_RFF_ANYD: feature panels + GEMM forward, training._rff_vjp_panels backward",
                "counters": "no counter run was made"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            dump(res, f)

    if "kernel" in args.parts:
        deadline = time.time() + args.budget_seconds if args.budget_seconds > 0 else None
        key = lambda r: (r["op"], r["N"], r["D"], r["L"], r["S"])
        merged = {key(r): r for r in res.get("rows", [])}
        for row in kernel_rows(args, deadline):
            merged[key(row)] = row
            res["rows"] = [merged[k] for k in sorted(merged)]
            res["rule"] = derive_rule(res["rows"])
            save()
        print(json.dumps(res.get("rule")), flush=True)
    if "paths" in args.parts:
        res["paths"] = paths_part(args)
    save()


if __name__ == "__main__":
    main()
