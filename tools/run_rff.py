"""Random Fourier features at C3 size (N = 2^20 + M rows, D = 8, L = 1024, S = 5, fp64): device-event times of the two
routes of mgp_rff_sample (alternated in one process) and of PathwiseClusterGP.pathwise_samples split into prior, solve
and correction; a second mode feeds a rocprofv3 --pmc pass and a third turns its counters into VALU instructions per
(row, basis) pair.

    python tools/run_rff.py --out profiles/rff_c3_times.json           # times (both routes, pathwise stages)
    rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_INSTS_VALU GRBM_GUI_ACTIVE --output-format csv -d <dir> -- \
        python tools/run_rff.py --pmc-child                              # counters only: 3 fused launches
    python tools/run_rff.py --pmc-summary <dir> --times profiles/rff_c3_times.json --out profiles/rff_c3_pmc.json
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd"))

N_C3, M_C3, D, L, S = 1 << 20, 4096, 8, 1024, 5
SIMDS, NOMINAL_HZ = 1024, 2.4e9  # MI355X: 256 CUs x 4 SIMDs; an fp64 VALU instruction of a wave issues in 4 cycles


def inputs(dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(a).to(dev)
    X = t(rng.standard_normal((N_C3 + M_C3, D)))
    th = t(rng.standard_normal((L, D)))
    W = t(rng.standard_normal((S, 2 * L)))
    return X, th, W


def timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def times(args):
    import numpy as np
    import torch
    from cggp import kernels, models, ops, rff
    dev = torch.device("cuda:0")
    X, th, W = inputs(dev)
    scale = math.sqrt(1.0 / L)

    def route(name):
        os.environ["MGP_RFF_ROUTE"] = name
        return ops.rff_sample(X, th, W, scale)

    a, b = route("fused"), route("panel")  # warm-up, and the two routes against each other
    torch.cuda.synchronize()
    diff = float((a - b).abs().max() / b.abs().max())
    fused, panel = [], []
    for _ in range(args.reps):  # alternate the routes
        fused += timed(lambda: route("fused"), 1)
        panel += timed(lambda: route("panel"), 1)
    os.environ.pop("MGP_RFF_ROUTE", None)
    pairs = float(N_C3 + M_C3) * L

    # pathwise_samples at C3: 2^20 sample rows, M = 4096, the same stages as the model runs them
    rng = np.random.default_rng(1)
    Xs = X[:N_C3]
    Z = X[N_C3:]
    counts = torch.from_numpy(rng.integers(50, 400, size=(M_C3, 1)).astype(np.float64)).to(dev)
    u = torch.from_numpy(rng.standard_normal((M_C3, 1))).to(dev)
    kern = kernels.SquaredExponential(variance=1.0, lengthscales=[1.0] * D)
    model = models.PathwiseClusterGP(kern, 25.6, Z, pseudo_u=u, cluster_counts=counts)
    xi = torch.from_numpy(rng.standard_normal((S, M_C3)))
    thc, Wc = th.cpu(), W.cpu()
    full = lambda: model.pathwise_samples(Xs, L, S, theta=thc, weights=Wc, xi=xi)
    full()
    st = {"prior": [], "solve": [], "correction": [], "full": []}
    lam = model.diag_variance[:, 0]
    for _ in range(args.reps):
        st["full"] += timed(full, 1)
        box = {}
        st["prior"] += timed(lambda: box.update(p=rff.rff_sample(X, kern, L, S, theta=th, weights=W)), 1)
        rhs = (u[:, 0][None, :] - box["p"][:, N_C3:] - models.pathwise_epsilon(lam, S, "reference", xi=xi)).t()

        def solve():
            K = kernels.Kuu(model.inducing_variable, kern, diag_add=lam)
            box["w"] = torch.cholesky_solve(rhs.contiguous(), torch.linalg.cholesky(K))
        st["solve"] += timed(solve, 1)
        st["correction"] += timed(lambda: ops.knm_matvec(kern.spec(D), Xs, Z, box["w"], ops.COLS, ops.ROWS), 1)
    med = lambda v: statistics.median(v)
    res = {
        "what": "mgp_rff_sample at C3 size (rows N + M = 2^20 + 4096, D = 8, L = 1024, S = 5, fp64, SE), fused and "
                "panel routes alternated in one process; PathwiseClusterGP.pathwise_samples at C3 (2^20 rows, "
                "M = 4096) and its stages (prior = mgp_rff_sample over X and Z together, solve = K_zz + Lambda and "
                "its Cholesky solve with S columns, correction = K_xz . weights by the multi-column K_nm sweep); "
                "device-event milliseconds, medians over reps",
        "device": torch.cuda.get_device_name(0),
        "reps": args.reps,
        "fused_ms": med(fused), "panel_ms": med(panel), "fused_ms_all": fused, "panel_ms_all": panel,
        "panel_over_fused": med(panel) / med(fused),
        "routes_max_rel_diff": diff,
        "pairs": pairs,
        "fused_ns_per_pair": med(fused) * 1e6 / pairs,
        "pathwise_ms": {k: med(v) for k, v in st.items()},
        "pathwise_ms_all": st,
    }
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def pmc_child(args):
    import torch
    from cggp import ops
    os.environ["MGP_RFF_ROUTE"] = "fused"
    X, th, W = inputs(torch.device("cuda:0"))
    for _ in range(3):
        ops.rff_sample(X, th, W, math.sqrt(1.0 / L))
    torch.cuda.synchronize()


def pmc_summary(args):
    per = {}
    for f in glob.glob(os.path.join(args.pmc_summary, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "rff_fused_kernel" not in row["Kernel_Name"]:
                continue
            d = per.setdefault(row["Dispatch_Id"], {})
            d[row["Counter_Name"]] = d.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    assert per, "no rff_fused_kernel dispatch in the counter files"
    mean = {c: statistics.mean(d[c] for d in per.values()) for c in next(iter(per.values()))}
    pairs = float(N_C3 + M_C3) * L
    res = {"what": "rocprofv3 --pmc (counters only) over tools/run_rff.py --pmc-child: 3 launches of the fused route "
                   "at C3 size (rows 2^20 + 4096, D = 8, L = 1024, S = 5, fp64); means per launch",
           "dispatches": len(per), "counters": mean, "pairs": pairs,
           "valu_instructions_per_pair": mean["SQ_INSTS_VALU"] * 64.0 / pairs,
           "active_valu_quadcycles_per_wave_pair": mean["SQ_ACTIVE_INST_VALU"] / (pairs / 64.0)}
    if "GRBM_GUI_ACTIVE" in mean:  # VALU-busy share of the launch's own cycles (as tools/make_valu_model.py)
        res["valu_busy_fraction"] = mean["SQ_ACTIVE_INST_VALU"] * 4.0 / SIMDS / (mean["GRBM_GUI_ACTIVE"] / 8.0)
    if args.times:
        t = json.load(open(args.times))
        # issue limit: one fp64 VALU instruction per SIMD every 4 cycles at the nominal clock
        floor_ms = pairs / 64.0 * res["valu_instructions_per_pair"] * 4.0 / (SIMDS * NOMINAL_HZ) * 1e3
        res["issue_limit_ms_at_2.4GHz"] = floor_ms
        res["fused_ms"] = t["fused_ms"]
        res["fraction_of_issue_limit"] = floor_ms / t["fused_ms"]
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--pmc-child", action="store_true")
    ap.add_argument("--pmc-summary")
    ap.add_argument("--times")
    a = ap.parse_args()
    if a.pmc_child:
        pmc_child(a)
    elif a.pmc_summary:
        pmc_summary(a)
    else:
        times(a)
