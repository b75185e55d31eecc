"""The full-data CDGP bound: what `TrainableCGGP(data_term="trace")` costs, against "batch", and how far one draw of
probes is from the exact data term.

    python tools/run_cdgp_full.py [--parts timing,compare,spread,lbfgs] [--out profiles/cdgp_full_times.json]

timing: one `training_loss(data).backward()` at N = 2^20, M = 4096, P = 5, fp64, dense and matrix-free, for SE at D = 8
(lengthscale 3.0; the sizes of C3) and Matern-3/2 at D = 32 (lengthscale 6.0; the kernel of C5); X and Z ~ U(-3, 3)^D,
CG threshold 1e-6 capped at 50 steps.  HIP events around the whole step and, inside it, around every solve (forward
and adjoint: "M-sized") and every `_KnmTimes` forward and backward ("N-sized": `mgp_knm_matvec`, `mgp_kmn_matvec`,
`mgp_kmn_knm_vjp`); the rest is the K_mm products, the log-det node and torch glue.  One warm-up step, then the median
of 5.

compare: "batch" (the code path as it was before `data_term`) and "trace" on the same data at N = 2^14, 2^15, ... while
a "batch" step stays under `--batch-seconds`; SE at D = 8, M = 4096, matrix-free and dense; the ratio batch / trace at
each N.  A recorded measurement, not a pass mark.

spread: N = 2^14, M = 1024, SE at D = 8: the data term `scale sum_n var_exp_n` (elbo + KL, both at the same probes) over
32 Rademacher draws of P = 5 and of P = 15 probes, its standard deviation relative to the exact value, which the probe
set sqrt(M) I gives.  Solves to 1e-10.

lbfgs: N = 20000, M = 200, both kernels, matrix-free: three iterations of `train_using_lbfgs_and_update` (which fixes one
draw of probes for the whole run) with P = 5, 15 and 50, and the loss before and after at those probes and at the exact
probe set: whether the steps lowered the bound or fitted the draw.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

CONFIGS = {"C3": ("se", 8, 3.0), "C5 kernel": ("matern32", 32, 6.0)}


def inputs(N, M, D, seed):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: ((torch.rand(s, generator=g, dtype=torch.float64) * 6.0) - 3.0).to(dev)
    Z, x = u(M, D), u(N, D)
    y = (torch.sin(x[:, :3]).sum(dim=1, keepdim=True) + 0.3 * torch.randn((N, 1), generator=g, dtype=torch.float64).to(dev))
    pseudo_u = torch.sin(Z[:, :3]).sum(dim=1, keepdim=True).contiguous()
    counts = torch.full((M, 1), float(N) / M, dtype=torch.float64, device=dev)
    return Z, x, y.contiguous(), pseudo_u, counts


def model_of(kind, D, ls, Z, pseudo_u, counts, N, matrix_free, data_term, cg):
    from cggp import kernels
    from cggp.training import TrainableCGGP
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32}[kind]
    return TrainableCGGP(cls(variance=1.0, lengthscales=[ls] * D), 0.1, Z, cg, num_probes=5, pseudo_u=pseudo_u,
                         cluster_counts=counts, num_data=N, matrix_free=matrix_free, data_term=data_term)


class Sections:
    """HIP events around chosen calls: wraps functions in place, sums the elapsed time per label after a synchronise"""

    def __init__(self):
        self.spans, self.undo = [], []

    def wrap(self, owner, name, label):
        import torch
        raw = getattr(owner, name)  # a module's function, or a class's staticmethod (an autograd node's forward)

        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = raw(*a, **k)
            e1.record()
            self.spans.append((label, e0, e1))
            return out

        self.undo.append((owner, name, vars(owner)[name]))
        setattr(owner, name, staticmethod(timed) if isinstance(owner, type) else timed)

    def restore(self):
        for owner, name, inner in reversed(self.undo):
            setattr(owner, name, inner)
        self.undo = []

    def collect(self):
        out = {}
        for label, e0, e1 in self.spans:
            out[label] = out.get(label, 0.0) + e0.elapsed_time(e1)
        self.spans = []
        return out


def timed_steps(m, data, probes, rounds, sections=None):
    import torch

    def step():
        for p in m.parameters():
            p.grad = None
        loss = m.training_loss(data, probes=probes)
        loss.backward()
        return float(loss.detach())

    step()  # warm-up: arenas, code objects
    if sections is not None:
        sections.collect()
    total, parts = [], []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        value = step()
        b.record()
        torch.cuda.synchronize()
        total.append(a.elapsed_time(b))
        if sections is not None:
            parts.append(sections.collect())
    assert np.isfinite(value)
    med = lambda v: float(np.median(v))
    out = dict(step_ms=med(total), all_step_ms=total, loss=value)
    if sections is not None:
        for label in sorted({k for p in parts for k in p}):
            out[label + "_ms"] = med([p.get(label, 0.0) for p in parts])
    return out


def timing_part(args):
    import torch

    from cggp import conjugate_gradient as cgm, training
    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    N, M = 1 << args.lg_n, args.m
    sec = Sections()
    # every solve of either model goes through these two (forward and adjoint); the rows through `_KnmTimes`
    sec.wrap(cgm, "_solve_device", "m_sized_solves")
    sec.wrap(training._KnmTimes, "forward", "n_sized_passes")
    sec.wrap(training._KnmTimes, "backward", "n_sized_passes")
    rows = []
    try:
        for name, (kind, D, ls) in CONFIGS.items():
            Z, x, y, u, counts = inputs(N, M, D, 7 + D)
            probes = rademacher((M, 5), torch.float64, Z.device, 0)
            for mf in (False, True):
                m = model_of(kind, D, ls, Z, u, counts, N, mf, "trace", ConjugateGradient(1e-6, max_iterations=50))
                row = dict(config=name, kernel=kind, D=D, N=N, M=M, P=5, matrix_free=mf,
                           **timed_steps(m, (x, y), probes, args.rounds, sec))
                row["other_ms"] = row["step_ms"] - row.get("m_sized_solves_ms", 0.0) - row.get("n_sized_passes_ms", 0.0)
                rows.append(row)
                print(f"{name} {kind} D={D} {'matrix-free' if mf else 'dense'}: step {row['step_ms']:.1f} ms = solves "
                      f"{row['m_sized_solves_ms']:.1f} + N-sized passes {row['n_sized_passes_ms']:.1f} + other "
                      f"{row['other_ms']:.1f}", flush=True)
            del Z, x, y, u, counts
            torch.cuda.empty_cache()
    finally:
        sec.restore()
    return rows


def compare_part(args):
    import torch

    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    kind, D, ls = CONFIGS["C3"]
    M = args.m
    rows = []
    for mf in (True, False):
        for lg in range(14, args.lg_n + 1):
            N = 1 << lg
            Z, x, y, u, counts = inputs(N, M, D, 11)
            probes = rademacher((M, 5), torch.float64, Z.device, 0)
            out = {}
            for term in ("batch", "trace"):
                m = model_of(kind, D, ls, Z, u, counts, N, mf, term, ConjugateGradient(1e-6, max_iterations=50))
                out[term] = timed_steps(m, (x, y), probes, 3)
            row = dict(kernel=kind, D=D, N=N, M=M, P=5, matrix_free=mf, batch_ms=out["batch"]["step_ms"],
                       trace_ms=out["trace"]["step_ms"], batch_over_trace=out["batch"]["step_ms"] / out["trace"]["step_ms"],
                       batch_all_ms=out["batch"]["all_step_ms"], trace_all_ms=out["trace"]["all_step_ms"])
            rows.append(row)
            print(f"{'matrix-free' if mf else 'dense'} N=2^{lg}: batch {row['batch_ms']:.1f} ms, trace "
                  f"{row['trace_ms']:.1f} ms, ratio {row['batch_over_trace']:.1f}", flush=True)
            del Z, x, y, u, counts
            torch.cuda.empty_cache()
            if row["batch_ms"] > 1e3 * args.batch_seconds / 2:  # the next N doubles it
                break
    return rows


def spread_part(args):
    import torch

    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    kind, D, ls = CONFIGS["C3"]
    N, M = 1 << 14, 1024
    Z, x, y, u, counts = inputs(N, M, D, 13)
    m = model_of(kind, D, ls, Z, u, counts, N, False, "trace", ConjugateGradient(1e-10, max_iterations=4 * M))
    frozen = m.frozen_model()

    def data_term(probes):
        return frozen.elbo((x, y), probes=probes) + frozen.prior_kl(probes=probes)

    exact = data_term(float(np.sqrt(M)) * torch.eye(M, dtype=torch.float64, device=Z.device))
    out = dict(kernel=kind, D=D, N=N, M=M, draws=32, exact_data_term=exact, by_probes={})
    for P in (5, 15):
        vals = np.array([data_term(rademacher((M, P), torch.float64, Z.device, 1000 * P + s)) for s in range(32)])
        out["by_probes"][str(P)] = dict(mean=float(vals.mean()), std=float(vals.std(ddof=1)),
                                        std_over_exact=float(vals.std(ddof=1) / abs(exact)),
                                        mean_minus_exact_over_exact=float((vals.mean() - exact) / abs(exact)))
        print(f"P={P}: data term {vals.mean():.4f} +- {vals.std(ddof=1):.4f} over 32 draws, exact {exact:.4f}: "
              f"relative spread {vals.std(ddof=1) / abs(exact):.2e}", flush=True)
    return out


def lbfgs_part(args):
    """Three L-BFGS iterations on the fixed-probe objective, and what they did to the bound itself: the loss at the
    optimiser's probes and at the exact probe set sqrt(M) I, before and after."""
    import torch

    from cggp.conjugate_gradient import ConjugateGradient
    from cggp.models import rademacher
    from cggp.training import train_using_lbfgs_and_update
    N, M = 20000, 200
    rows = []
    for name, (kind, D, ls) in CONFIGS.items():
        Z, x, y, u, counts = inputs(N, M, D, 17)
        exact = float(np.sqrt(M)) * torch.eye(M, dtype=torch.float64, device=Z.device)
        for P in (5, 15, 50):
            m = model_of(kind, D, ls, Z, u, counts, N, True, "trace", ConjugateGradient(1e-12, max_iterations=4 * M))
            m.num_probes = P
            fixed = rademacher((M, P), torch.float64, Z.device, 0)  # what train_using_lbfgs_and_update draws
            value = lambda probes: float(m.training_loss((x, y), probes=probes).detach())
            row = dict(config=name, kernel=kind, D=D, N=N, M=M, P=P, fixed_before=value(fixed), exact_before=value(exact))
            try:
                res = train_using_lbfgs_and_update((x, y), m, 3)
                row.update(iterations=int(res.nit), evaluations=int(res.nfev), fixed_after=value(fixed),
                           exact_after=value(exact), variance=m.kernel.variance_p.value,
                           lengthscales=m.kernel.lengthscales_p.value, noise=m.noise_p.value)
            except (ValueError, RuntimeError) as e:  # the line search left the domain: NaN, then a non-positive value
                row.update(failed=repr(e))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="timing,compare,spread,lbfgs")
    ap.add_argument("--lg-n", type=int, default=20)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-seconds", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdgp_full_times.json"))
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["what"] = ("TrainableCGGP(data_term=\"trace\"): one loss plus backward, HIP events, one warm-up and the median of "
                   "the rounds; against data_term=\"batch\"; spread of the data term over probe draws; "
                   "tools/run_cdgp_full.py")
    parts = args.parts.split(",")
    if "timing" in parts:
        doc["timing"] = timing_part(args)
    if "compare" in parts:
        doc["compare"] = compare_part(args)
    if "spread" in parts:
        doc["spread"] = spread_part(args)
    if "lbfgs" in parts:
        doc["lbfgs"] = lbfgs_part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
