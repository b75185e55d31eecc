"""The pivoted-Cholesky preconditioner of matrix-free CDGP, measured: one application of `MGP_PRE_LOWRANK` (kind 5, 16
right-hand sides per group of launches) beside `MGP_PRE_LOWRANK_WIDE` (kind 6, 256 per group on the fp64 matrix cores)
and the rule for `conjugate_gradient.LOWRANK_WIDE_MIN_COLUMNS`, its share of a CG step beside the many-column operator,
`CGGP(matrix_free=True).predict_f_batched` and one `TrainableCGGP` step with and without the preconditioner.

    python tools/run_cdgp_precond.py [--parts apply,step,predict,train] [--lg-n 12,14,16,17]
                                     [--columns 16,24,32,48,64,128,256] [--rounds 5] [--cap 500]
                                     [--out profiles/cdgp_precond_times.json]

apply: rank 128, hand-made (dinv, B).  libmgp exports no entry point for the many-column application, so both kinds are
timed through a CG solve of ZERO steps from x0 = 0: its start-up forms r = b, applies the preconditioner once
(ungated) and makes three small launches and one poll, and never applies the operator.  The same solve with the identity
is the overhead both carry; `apply_ms` = the kind's time minus it, and `mgp_lowrank_apply` called directly is recorded
beside kind 5 as a check of that subtraction.  One warm-up, then `--rounds` rounds with the forms alternated, device
events between two synchronisations, best of the rounds.
rule (fixed before measuring): LOWRANK_WIDE_MIN_COLUMNS is the smallest measured width such that at every measured point
with at least that many columns the many-column form's zero-step solve takes at most 0.9 of kind 5's (overhead
included in both, which favours kind 5); None if no width qualifies.

step: 10 fixed CG steps at M = 2^14 with 256 columns on the many-column operator, identity / kind 5 / kind 6.
predict: `predict_f_batched` on 2^12 rows in batches of 256 at M = 2^14, threshold 1e-6, every solve capped at `--cap`
steps (the cap and the steps of every batch are recorded), SE with D = 2 (lengthscale 1.5) and D = 8 (3.0), rank 128:
identity, kind 5, kind 6; one warm-up on one batch, one timed run each.
train: one `TrainableCGGP(matrix_free=True)` loss and backward pass at M = 2^14, batch 256, D = 2, the same three.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cggp import _hip, kernels, ops  # noqa: E402
from cggp.conjugate_gradient import (ConjugateGradient, EyePreconditioner, KmmLambdaOperator,  # noqa: E402
                                     PivotedCholeskyPreconditioner, _solve_device)

RANK = 128
MARGIN = 0.9
DEV = torch.device("cuda:0")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternated(fns, rounds):
    for fn in fns.values():
        once(fn)
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(once(fn)[0])
    return {name: {"best_ms": float(min(v)), "median_ms": float(np.median(v)), "max_ms": float(max(v))}
            for name, v in ms.items()}


class Hand:
    """(dinv, B) handed to libmgp as the given kind."""

    def __init__(self, dinv, B, kind):
        self.dinv, self.B, self.kind = dinv, B, kind

    def _native_for(self, op, Bt):
        st = _hip.MgpPrecond()
        st.kind, st.diag_inv, st.dense_inv, st.num_blocks = self.kind, self.dinv.data_ptr(), self.B.data_ptr(), self.B.shape[0]
        return st, (self.dinv, self.B)


def system(n, D, ls, seed):
    rng = np.random.default_rng([seed, n, D])
    Z = torch.from_numpy(rng.uniform(-3.0, 3.0, (n, D))).to(DEV)
    lam = torch.from_numpy(0.1 / rng.integers(1, 65, n)).to(DEV)
    return rng, Z, lam, kernels.SquaredExponential(1.0, [ls] * D)


def apply_rows(args):
    for lg in args.lg_n:
        n = 1 << lg
        rng, Z, lam, kern = system(n, 2, 1.5, 0)
        op = KmmLambdaOperator(kern, Z, lam)
        B = torch.from_numpy(0.3 * rng.standard_normal((RANK, n)) / (np.sqrt(n) + np.sqrt(RANK))).to(DEV)
        dinv = torch.from_numpy(0.5 + rng.random(n)).to(DEV)
        pres = {"identity": EyePreconditioner(), "narrow": Hand(dinv, B, _hip.PRE_LOWRANK),
                "wide": Hand(dinv, B, _hip.PRE_LOWRANK_WIDE)}
        for Bt in args.columns:
            R = torch.from_numpy(rng.standard_normal((Bt, n))).to(DEV)
            z = {k: _solve_device(op, R, None, 0.0, p, 1, 2, 1e-16, 10)[0] for k, p in pres.items() if k != "identity"}
            diff = float((z["wide"] - z["narrow"]).abs().max() / z["narrow"].abs().max())
            fns = {k: (lambda p=p: _solve_device(op, R, None, 0.0, p, 0, 1, 1e-16, 10)) for k, p in pres.items()}
            fns["direct_narrow"] = lambda: ops.lowrank_apply(dinv, B, R)
            t = alternated(fns, args.rounds)
            base = t["identity"]["best_ms"]
            row = {"n": n, "rank": RANK, "columns": Bt, "one_step_rel_diff": diff, "zero_step_solve": t,
                   "apply_ms": {k: t[k]["best_ms"] - base for k in ("narrow", "wide")},
                   "wide_over_narrow_solve": t["wide"]["best_ms"] / t["narrow"]["best_ms"]}
            row["wide_over_narrow_apply"] = row["apply_ms"]["wide"] / max(row["apply_ms"]["narrow"], 1e-9)
            print(json.dumps(row), flush=True)
            yield row
            del R
        del Z, lam, B, dinv
        torch.cuda.empty_cache()


def derive_rule(rows):
    cols = sorted({r["columns"] for r in rows})
    wins = lambda r: r["zero_step_solve"]["wide"]["best_ms"] <= MARGIN * r["zero_step_solve"]["narrow"]["best_ms"]
    chosen = None
    for c in cols:
        if all(wins(r) for r in rows if r["columns"] >= c):
            chosen = c
            break
    return {"margin": MARGIN, "points": len(rows), "LOWRANK_WIDE_MIN_COLUMNS": chosen}


def step_part(args):
    n, Bt, steps = 1 << 14, 256, 10
    rng, Z, lam, kern = system(n, 2, 1.5, 1)
    op = KmmLambdaOperator(kern, Z, lam, wide=True)
    B = torch.from_numpy(0.3 * rng.standard_normal((RANK, n)) / (np.sqrt(n) + np.sqrt(RANK))).to(DEV)
    dinv = torch.from_numpy(0.5 + rng.random(n)).to(DEV)
    R = torch.from_numpy(rng.standard_normal((Bt, n))).to(DEV)
    pres = {"identity": EyePreconditioner(), "narrow": Hand(dinv, B, _hip.PRE_LOWRANK),
            "wide": Hand(dinv, B, _hip.PRE_LOWRANK_WIDE)}
    fns = {k: (lambda p=p: _solve_device(op, R, None, 0.0, p, steps, steps + 1, 1e-16, 10)) for k, p in pres.items()}
    t = alternated(fns, args.rounds)
    per = {k: v["best_ms"] / steps for k, v in t.items()}
    out = {"M": n, "columns": Bt, "rank": RANK, "steps": steps, "solve": t, "ms_per_step": per,
           "share_of_step": {k: (per[k] - per["identity"]) / per[k] for k in ("narrow", "wide")}}
    print(json.dumps(out), flush=True)
    return out


class CountingCG(ConjugateGradient):
    """Records (steps, largest 0.5 rz) of every solve."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def solve_with_stats(self, matrix, rhs, initial_solution=None):
        sol, stats = super().solve_with_stats(matrix, rhs, initial_solution)
        self.log.append((int(stats[0]), float(stats[1].max())))
        return sol, stats


def cdgp_problem(D, ls, seed):
    from cggp.optimize import nearest_centre_statistics
    M, N = 1 << 14, 1 << 16
    rng = np.random.default_rng([seed, D])
    X = torch.from_numpy(rng.uniform(-3.0, 3.0, (N, D))).to(DEV)
    y = (torch.sin(X.sum(dim=1)) + 0.1 * torch.from_numpy(rng.standard_normal(N)).to(DEV))[:, None].contiguous()
    Z = X[torch.from_numpy(rng.choice(N, M, replace=False)).to(DEV)].contiguous()
    kern = kernels.SquaredExponential(1.0, [ls] * D)
    _, sums, counts = nearest_centre_statistics(kern, Z, (X, y))
    counts = counts.clamp(min=1.0)
    return X, y, Z, kern, (sums / counts)[:, None].contiguous(), counts[:, None].contiguous()


def variants():
    return {"identity": None, "narrow": PivotedCholeskyPreconditioner(rank=RANK, wide=False),
            "wide": PivotedCholeskyPreconditioner(rank=RANK, wide=True)}


def predict_part(args):
    from cggp.models import CGGP
    rows, batch, thr = 1 << 12, 256, 1e-6
    out = []
    for D, ls in ((2, 1.5), (8, 3.0)):
        X, y, Z, kern, u, counts = cdgp_problem(D, ls, 7)
        xs = X[:rows].contiguous()
        res = {"M": Z.shape[0], "rows": rows, "batch": batch, "kernel": "se", "D": D, "lengthscale": ls, "threshold": thr,
               "cap": args.cap, "rank": RANK, "wide_solves": "auto", "runs": {}}
        ref = None
        for name, pre in variants().items():
            cg = CountingCG(thr, preconditioner=pre, max_iterations=args.cap)
            m = CGGP(kern, 0.1, Z, cg, num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=X.shape[0],
                     matrix_free=True, wide_solves="auto")
            build_ms = 0.0
            if pre is not None:
                _, op, _ = m._system()
                pre._prepare(op)  # warm-up: the first build of a process also starts torch's dense linear algebra
                pre._kmm_key = None
                build_ms, _ = once(lambda: pre._prepare(op))
                pre._kmm_key = None  # the timed run builds it again, as a first call would
            once(lambda: m.predict_f_batched(xs[:batch], batch))
            if pre is not None:
                pre._kmm_key = None
            cg.log.clear()
            ms, (mu, var) = once(lambda: m.predict_f_batched(xs, batch))
            steps = [s for s, _ in cg.log]
            run = {"total_ms": ms, "factor_build_ms": build_ms, "rank_reached": None if pre is None else pre.rank_,
                   "steps_pseudo_u": steps[0], "steps_per_batch": steps[1:], "steps_total": int(sum(steps)),
                   "capped_solves": int(sum(s >= args.cap for s in steps)), "largest_half_rz": max(e for _, e in cg.log)}
            if ref is None:
                ref = (mu, var)
            else:
                run["mean_abs_diff_to_identity"] = float((mu - ref[0]).abs().max())
                run["variance_abs_diff_to_identity"] = float((var - ref[1]).abs().max())
            res["runs"][name] = run
            print(json.dumps({"D": D, name: run}), flush=True)
        out.append(res)
        del X, y, Z
        torch.cuda.empty_cache()
    return out


def train_part(args):
    from cggp.training import TrainableCGGP
    D, ls, batch = 2, 1.5, 256
    X, y, Z, kern, u, counts = cdgp_problem(D, ls, 7)
    data = (X[:batch].contiguous(), y[:batch].contiguous())
    res = {"M": Z.shape[0], "batch": batch, "D": D, "lengthscale": ls, "threshold": 1e-6, "cap": args.cap, "rank": RANK,
           "runs": {}}
    for name, pre in variants().items():
        cg = CountingCG(1e-6, preconditioner=pre, max_iterations=args.cap)
        m = TrainableCGGP(kern, 0.1, Z, cg, num_probes=5, pseudo_u=u, cluster_counts=counts, num_data=X.shape[0],
                          matrix_free=True, wide_solves="auto")

        def step():
            for p in m.parameters():
                p.grad = None
            m.probe_seed = 0
            loss = m.training_loss(data)
            loss.backward()
            return float(loss.detach())

        once(step)
        ms, loss = once(step)
        res["runs"][name] = {"step_ms": ms, "loss": loss}
        print(json.dumps({name: res["runs"][name]}), flush=True)
    return res


def main():
    ints = lambda s: [int(v) for v in s.split(",") if v]
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="apply,step,predict,train")
    ap.add_argument("--lg-n", type=ints, default=[12, 14, 16, 17])
    ap.add_argument("--columns", type=ints, default=[16, 24, 32, 48, 64, 128, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdgp_precond_times.json"))
    args = ap.parse_args()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "dtype": "float64",
                "timing": "device events between two device synchronisations; one warm-up per form, forms alternated; "
                          "best of the rounds (apply, step); one warm-up and one timed run (predict, train)"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if "apply" in args.parts:
        key = lambda r: (r["n"], r["columns"])
        merged = {key(r): r for r in res.get("apply", [])}
        for row in apply_rows(args):
            merged[key(row)] = row
            res["apply"] = [merged[k] for k in sorted(merged)]
            res["rule"] = derive_rule(res["apply"])
            save()
        print(json.dumps(res.get("rule")), flush=True)
    if "step" in args.parts:
        res["cg_step"] = step_part(args)
        save()
    if "predict" in args.parts:
        res["predict_f_batched"] = predict_part(args)
        save()
    if "train" in args.parts:
        res["trainable_step"] = train_part(args)
        save()


if __name__ == "__main__":
    main()
