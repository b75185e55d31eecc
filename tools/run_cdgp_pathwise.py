"""The pathwise CDGP bound: what `mgp_rff_sample_vjp` and `TrainableCGGP(data_term="pathwise")` cost, beside the forward
kernel and beside "trace", and how far one draw is from the exact data term.

    python tools/run_cdgp_pathwise.py [--parts kernel,step,spread] [--out profiles/cdgp_pathwise_times.json]

kernel: N = 2^20 + M rows, M = 4096, L = 1024, S = 5, fp64, for SE at D = 8 (C3) and the frequencies of Matern-3/2 at
D = 32: `mgp_rff_sample`, `mgp_rff_sample_vjp` for dtheta on all rows and for dX on the M rows of Z, in the same run; HIP
events, one warm-up, the median of `--rounds`.

step: one `training_loss(data).backward()` with "pathwise" (S = 5, L = 1024) and with "trace" (P = 5) on the same inputs
(those of tools/run_cdgp_full.py), dense and matrix-free, CG threshold 1e-6 capped at 50 steps; the ratio pathwise /
trace.  Recorded, not asserted.

spread: N = 2^14, M = 1024, SE at D = 8 (lengthscale 3) and Matern-3/2 at D = 4 (lengthscale 2): the data term
(elbo + KL) over 32 draws with S = 5 and S = 15 samples, beside "trace" over 32 draws of P = 5 probes; standard
deviations relative to the exact data term and to its variance part sum_n var_n / (2 s2), both from the exact probe
set sqrt(M) I.  Solves to 1e-10.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import run_cdgp_full as rf  # noqa: E402

CONFIGS = rf.CONFIGS
SPREAD_CONFIGS = {"SE D=8 l=3": ("se", 8, 3.0), "Matern-3/2 D=4 l=2": ("matern32", 4, 2.0)}
KERNELS = lambda: __import__("cggp.kernels", fromlist=["x"])


def model_of(kind, D, ls, Z, pseudo_u, counts, N, matrix_free, data_term, cg, S=5, L=1024):
    from cggp.training import TrainableCGGP
    k = KERNELS()
    cls = {"se": k.SquaredExponential, "matern32": k.Matern32}[kind]
    return TrainableCGGP(cls(variance=1.0, lengthscales=[ls] * D), 0.1, Z, cg, num_probes=5, pseudo_u=pseudo_u,
                         cluster_counts=counts, num_data=N, matrix_free=matrix_free, data_term=data_term,
                         num_bases=L, num_samples=S)


def median_ms(fn, rounds):
    import torch
    fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def kernel_part(args):
    import torch

    from cggp import models, ops
    N, M, L, S = 1 << args.lg_n, args.m, 1024, 5
    rows = []
    for name, (kind, D, ls) in CONFIGS.items():
        Z, x, _, _, _ = rf.inputs(N, M, D, 7 + D)
        pts = torch.cat([x, Z], dim=0).contiguous()
        E, W, _ = models.draw_pathwise(kind, D, M, L, S, 0)
        theta, W = (E / ls).to(pts.device).contiguous(), W.to(pts.device).contiguous()
        scale = float(np.sqrt(1.0 / L))
        G = torch.randn((S, N + M), dtype=torch.float64, device=pts.device)
        Gz = G[:, N:].contiguous()
        fwd, fwd_all = median_ms(lambda: ops.rff_sample(pts, theta, W, scale), args.rounds)
        dth, dth_all = median_ms(lambda: ops.rff_sample_vjp(pts, theta, W, scale, G), args.rounds)
        dz, dz_all = median_ms(lambda: ops.rff_sample_vjp(Z, theta, W, scale, Gz, want_dtheta=False, want_dX=True),
                               args.rounds)
        dxa, dxa_all = median_ms(lambda: ops.rff_sample_vjp(pts, theta, W, scale, G, want_dtheta=False, want_dX=True),
                                 args.rounds)
        row = dict(config=name, kernel=kind, D=D, rows=N + M, M=M, L=L, S=S, forward_ms=fwd, vjp_dtheta_ms=dth,
                   vjp_dz_ms=dz, vjp_dx_all_rows_ms=dxa, dtheta_over_forward=dth / fwd, dx_all_rows_over_forward=dxa / fwd,
                   forward_all_ms=fwd_all, vjp_dtheta_all_ms=dth_all, vjp_dz_all_ms=dz_all, vjp_dx_all_rows_all_ms=dxa_all)
        rows.append(row)
        print(f"{name}: mgp_rff_sample {fwd:.2f} ms; vjp dtheta {dth:.2f} ms ({dth / fwd:.2f}x), dX on all rows "
              f"{dxa:.2f} ms ({dxa / fwd:.2f}x), dZ on {M} rows {dz:.3f} ms", flush=True)
        del Z, x, pts, G
        torch.cuda.empty_cache()
    return rows


def step_part(args):
    import torch

    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    N, M = 1 << args.lg_n, args.m
    rows = []
    for name, (kind, D, ls) in CONFIGS.items():
        Z, x, y, u, counts = rf.inputs(N, M, D, 7 + D)
        probes = rademacher((M, 5), torch.float64, Z.device, 0)
        for mf in (False, True):
            out = {}
            for term in ("trace", "pathwise"):
                m = model_of(kind, D, ls, Z, u, counts, N, mf, term, ConjugateGradient(1e-6, max_iterations=50))
                kw = dict(pathwise=tuple(t.to(Z.device) for t in m.draw_pathwise(0))) if term == "pathwise" else {}

                def step():
                    for p in m.parameters():
                        p.grad = None
                    loss = m.training_loss((x, y), probes=probes, **kw)
                    loss.backward()
                    return float(loss.detach())

                ms, all_ms = median_ms(step, args.rounds)
                out[term] = dict(step_ms=ms, all_step_ms=all_ms, loss=step())
            row = dict(config=name, kernel=kind, D=D, N=N, M=M, P=5, S=5, L=1024, matrix_free=mf,
                       trace_ms=out["trace"]["step_ms"], pathwise_ms=out["pathwise"]["step_ms"],
                       pathwise_over_trace=out["pathwise"]["step_ms"] / out["trace"]["step_ms"], detail=out)
            rows.append(row)
            print(f"{name} {'matrix-free' if mf else 'dense'}: trace {row['trace_ms']:.1f} ms, pathwise "
                  f"{row['pathwise_ms']:.1f} ms, ratio {row['pathwise_over_trace']:.2f}", flush=True)
        del Z, x, y, u, counts
        torch.cuda.empty_cache()
    return rows


def spread_part(args):
    import math

    import torch

    from cggp import ops
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    N, M, draws = 1 << 14, 1024, 32
    rows = []
    for name, (kind, D, ls) in SPREAD_CONFIGS.items():
        Z, x, y, u, counts = rf.inputs(N, M, D, 13)
        cg = ConjugateGradient(1e-10, max_iterations=4 * M)
        exact_probes = float(np.sqrt(M)) * torch.eye(M, dtype=torch.float64, device=Z.device)
        tr = model_of(kind, D, ls, Z, u, counts, N, False, "trace", cg).frozen_model()
        kl = tr.prior_kl(probes=exact_probes)
        exact = tr.elbo((x, y), probes=exact_probes) + kl
        a = cg(tr._system()[1], tr.pseudo_u)
        resid = (y - ops.knm_matvec(tr.kernel.spec(D), x, Z, a)).contiguous()
        s2 = 0.1
        var_part = -(exact + 0.5 * N * math.log(2.0 * math.pi * s2) + 0.5 * ops.dot_all(resid, resid) / s2)
        row = dict(config=name, kernel=kind, D=D, N=N, M=M, draws=draws, exact_data_term=exact,
                   exact_variance_part=var_part, estimators={})

        def record(label, vals):
            vals = np.array(vals)
            sd = float(vals.std(ddof=1))
            row["estimators"][label] = dict(mean=float(vals.mean()), std=sd, std_over_exact=sd / abs(exact),
                                            std_over_variance_part=sd / abs(var_part),
                                            mean_minus_exact_over_variance_part=float((vals.mean() - exact) / abs(var_part)),
                                            min=float(vals.min()), max=float(vals.max()))
            print(f"{name} {label}: {vals.mean():.3f} +- {sd:.3f} (exact {exact:.3f}, variance part {var_part:.3f}): "
                  f"std / variance part {sd / abs(var_part):.3g}", flush=True)

        vals = []
        for s in range(draws):
            pr = rademacher((M, 5), torch.float64, Z.device, 5000 + s)
            vals.append(tr.elbo((x, y), probes=pr) + tr.prior_kl(probes=pr))
        record("trace P=5", vals)
        for S in (5, 15):
            pw = model_of(kind, D, ls, Z, u, counts, N, False, "pathwise", cg, S=S).frozen_model()
            vals = []
            for s in range(draws):
                pw.pathwise_seed = 100 * S + s
                vals.append(pw.elbo((x, y), probes=exact_probes) + kl)
            record(f"pathwise S={S} L=1024", vals)
        rows.append(row)
        del Z, x, y, u, counts
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,step,spread")
    ap.add_argument("--lg-n", type=int, default=20)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdgp_pathwise_times.json"))
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["what"] = ("mgp_rff_sample_vjp beside mgp_rff_sample; TrainableCGGP(data_term=\"pathwise\") beside \"trace\": one "
                   "loss plus backward, HIP events, one warm-up and the median of the rounds; spread of the data term "
                   "over draws; tools/run_cdgp_pathwise.py")
    parts = args.parts.split(",")
    for part, fn in (("kernel", kernel_part), ("step", step_part), ("spread", spread_part)):
        if part in parts:
            doc[part] = fn(args)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # after every part: a later part's failure loses nothing
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
