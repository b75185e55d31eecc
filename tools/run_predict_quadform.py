"""Whole-test-set variances: `mgp_knm_quadform` (include/mgp_predict.h) against the composition it replaces, and the
batched prediction of the two sparse models end to end, all legs in one run on one GPU.

    python tools/run_predict_quadform.py [--lg-b 16] [--ms 1024,4096,8192] [--rounds 5] [--lg-n 20] [--m 4096]
                                         [--lg-loop 14] [--out profiles/predict_quadform_times.json]
    python tools/run_predict_quadform.py --step kernel --ms 4096 ...     (one step in this process; prints its JSON rows)

fp64, the synthetic inputs of `cggp.synthetic.make_inputs` (X ~ N(0, I), Z a sample of X, unit lengthscales), the two
kernels of C3 and C5: SE at D = 8 and Matern-3/2 at D = 32.  The driver runs every step in a fresh child process under
a time limit of its own and stops at the first one that fails.  In a step: HIP events around synchronised calls, one
warm-up of every timed shape, the versions alternated round by round within the process, median and (min, max)
reported: boxes differ by a few per cent, only the in-run ratios count.  Every step records the shader clock of a few
profiled sweep launches before and after its timed rounds (`mgp_profile_read_clocks`).

steps   kernel   q = k(Xs, Z) C k(Z, Xs) for B = 2^lg-b rows, per M and kernel: fused = ops.knm_quadform; composition =
                 ops.k_dense + ops.symm_matmul + row sum (what CGGP.predict_f_batched(shared_inverse=True) runs per
                 batch) over batches of 8192 rows and as one batch; the ratio is to the faster of the two; the largest
                 difference between the routes relative to max |q|; the share of the matrix cores' peak the fused call
                 reaches on the flop of the triangular form
        cdgp     CGGP.predict_f_batched(X, 2^16, shared_inverse=True) over 2^lg-n rows at M = --m, SE, D = 8, with
                 fused_variance off and on (each call includes the shared M-column solve, timed on its own as well)
        sgpr     SGPR.predict_f_batched over 2^lg-n rows, fused_variance off and on, against a loop of SGPR.predict_f
                 in batches of 256 over the first 2^lg-loop rows, scaled by 2^(lg-n - lg-loop) (the loop is linear in
                 the rows: every batch runs the same two 256-column solves)
"""

import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")):
    sys.path.insert(0, p)

STEP_LIMIT_S = {"kernel": 300, "cdgp": 300, "sgpr": 390}
CONFIGS = (("se", 8), ("matern32", 32))
# the floor tools/run_love.py uses: v_mfma_f64_16x16x4_f64 (2048 flop) every 64 cycles per SIMD, 4 SIMDs x 256 CUs, 2.4 GHz
MFMA_F64_PEAK_TF = 78.6


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


def shader_clock_mhz(torch, np, dev):
    """Mean shader clock over the sampled workgroups of four profiled one-column sweeps (2^18 x 4096, SE, D = 8)."""
    from cggp import _hip, ops
    rng = np.random.default_rng(7)
    X = torch.from_numpy(rng.standard_normal((1 << 18, 8))).to(dev)
    Z = X[:4096].contiguous()
    v = torch.from_numpy(rng.standard_normal((4096, 1))).to(dev)
    spec = ops.KernelSpec("se", 1.0, [1.0] * 8, 8)
    ops.knm_matvec(spec, X, Z, v)
    hd = _hip.get_handle(dev)
    hd.check(hd.lib.mgp_profile_enable(hd.h, 1))
    for _ in range(4):
        ops.knm_matvec(spec, X, Z, v)
    torch.cuda.synchronize()
    cap = 16 * 16
    mhz = (ctypes.c_double * cap)()
    n = ctypes.c_int64(0)
    ok = hd.lib.mgp_profile_read_clocks(hd.h, mhz, cap, ctypes.byref(n)) == 0 and n.value > 0
    hd.check(hd.lib.mgp_profile_enable(hd.h, 0))
    return float(np.mean(mhz[:min(n.value, cap)])) if ok else None


def run_step(args):
    import numpy as np
    import torch

    from cggp import kernels, ops, synthetic
    from cggp.conjugate_gradient import ConjugateGradient

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    clock0 = shader_clock_mhz(torch, np, dev)

    def emit(row):
        row["shader_clock_mhz_before"] = clock0
        row["shader_clock_mhz_after"] = shader_clock_mhz(torch, np, dev)
        print(json.dumps(row), flush=True)

    if args.step == "kernel":
        B = 1 << args.lg_b
        for name, D in CONFIGS:
            for M in [int(m) for m in args.ms.split(",")]:
                syn = synthetic.make_inputs(B, D, M, need_y=False)
                Xs, Z = t(syn.X), t(syn.Z)
                spec = ops.KernelSpec(name, 1.0, [1.0] * D, D)
                rng = np.random.default_rng([M, D])
                G = t(rng.standard_normal((M, M)))
                C = (G @ G.t() / M + torch.eye(M, dtype=torch.float64, device=dev)).contiguous()
                del G

                def composed(bs):
                    out = []
                    for s in range(0, B, bs):
                        Knm = ops.k_dense(spec, Xs[s:s + bs], Z)
                        out.append((Knm * ops.symm_matmul(C, Knm)).sum(dim=1))
                    return torch.cat(out)

                fns = {"fused": lambda: ops.knm_quadform(spec, Xs, Z, C), "composed_8192": lambda: composed(8192),
                       "composed_one_batch": lambda: composed(B)}
                q1, q0 = fns["fused"](), fns["composed_8192"]()
                times = alternated(torch, np, fns, args.rounds)
                best = min(times["composed_8192"]["median_ms"], times["composed_one_batch"]["median_ms"])
                nJ = (M + 127) // 128
                tri_flop = 2.0 * B * 128 * 128 * nJ * (nJ + 1) / 2  # the walks of the blocks, padded as the kernel runs them
                emit({"step": "kernel", "kernel": name, "D": D, "B": B, "M": M, "rounds": args.rounds, "times": times,
                      "fused_over_composed": times["fused"]["median_ms"] / best,
                      "rel_diff_to_composed": float((q1 - q0).abs().max() / q0.abs().max()),
                      "fused_tflops_on_triangular_flop": tri_flop / (times["fused"]["median_ms"] * 1e-3) / 1e12,
                      "fused_share_of_fp64_matrix_peak": tri_flop / (times["fused"]["median_ms"] * 1e-3) / 1e12 / MFMA_F64_PEAK_TF,
                      "kernel_evaluations_per_row_over_M": (nJ + 1) / 2.0,
                      "c_bytes_streamed_per_row_tile": 8.0 * 128 * 128 * nJ * (nJ + 1) / 2})
                del C, Xs, Z
                torch.cuda.empty_cache()
        return

    N, M, D = 1 << args.lg_n, args.m, 8
    syn = synthetic.make_inputs(N, D, M)
    X, y, Z = t(syn.X), t(syn.y), t(syn.Z)
    kern = kernels.SquaredExponential(variance=syn.variance, lengthscales=syn.lengthscales)
    if args.step == "cdgp":
        from cggp.models import CGGP
        from cggp.optimize import nearest_centre_statistics
        _, sums, counts = nearest_centre_statistics(kern, Z, (X, y), "sqeuclidean", None)
        counts = torch.where(counts != 0, counts, torch.ones_like(counts))
        cgm = ConjugateGradient(1e-6, check_every=25)
        mdl = CGGP(kern, syn.noise_variance, Z, cgm, num_probes=None, pseudo_u=(sums / counts)[:, None],
                   cluster_counts=counts[:, None], num_data=N)
        bs = 1 << 16
        fns = {"composed": lambda: mdl.predict_f_batched(X, bs, shared_inverse=True, fused_variance=False),
               "fused": lambda: mdl.predict_f_batched(X, bs, shared_inverse=True, fused_variance=True)}
        v1, v0 = fns["fused"]()[1], fns["composed"]()[1]
        times = alternated(torch, np, fns, args.rounds)
        _, KL, _ = mdl._system()
        tight = ConjugateGradient(1e-12, cgm.preconditioner, cgm.max_iterations, cgm.max_steps_cycle,
                                  min_float=cgm.min_float, check_every=cgm.check_every)
        eye = torch.eye(M, dtype=torch.float64, device=dev)
        tight(KL, eye)
        solve_ms = float(np.median([once(torch, lambda: tight(KL, eye))[0] for _ in range(args.rounds)]))
        emit({"step": "cdgp", "kernel": "se", "D": D, "rows": N, "M": M, "batch_size": bs, "rounds": args.rounds,
              "times": times,
              "shared_solve_ms_included_in_both": solve_ms,
              "fused_over_composed": times["fused"]["median_ms"] / times["composed"]["median_ms"],
              "fused_over_composed_without_the_solve": (times["fused"]["median_ms"] - solve_ms)
              / (times["composed"]["median_ms"] - solve_ms),
              "max_abs_variance_diff": float((v1 - v0).abs().max())})
        return
    if args.step == "sgpr":
        from cggp.models import SGPR
        mdl = SGPR((X, y), kern, Z, syn.noise_variance, ConjugateGradient(1e-6))
        build_ms = once(torch, lambda: (mdl.alpha(), mdl.variance_matrix()))[0]  # alpha, K_mn K_nm and C: once per model
        bs = 1 << 16
        fns = {"batched_composed": lambda: mdl.predict_f_batched(X, bs, fused_variance=False),
               "batched_fused": lambda: mdl.predict_f_batched(X, bs, fused_variance=True)}
        v1, v0 = fns["batched_fused"]()[1], fns["batched_composed"]()[1]
        times = alternated(torch, np, fns, args.rounds)
        nl = 1 << args.lg_loop

        def loop():
            out = []
            for s in range(0, nl, 256):
                out.append(mdl.predict_f(X[s:s + 256])[1])
            return torch.cat(out)

        vl = loop()  # warm: forms the explicit S and the preconditioner
        loop_ms = [once(torch, loop)[0] for _ in range(args.rounds)]
        loop_med = float(np.median(loop_ms))
        scale = N // nl
        emit({"step": "sgpr", "kernel": "se", "D": D, "rows": N, "M": M, "batch_size": bs, "rounds": args.rounds,
              "times": times,
              "alpha_and_variance_matrix_ms_once": build_ms,
              "predict_f_loop": {"rows_timed": nl, "batch": 256, "rounds": args.rounds, "ms": loop_ms,
                                 "median_ms": loop_med, "scaled_by": scale, "scaled_ms": loop_med * scale,
                                 "scaling": "linear in the rows: every batch of 256 runs the same two 256-column solves"},
              "fused_over_composed": times["batched_fused"]["median_ms"] / times["batched_composed"]["median_ms"],
              "loop_over_batched_fused": loop_med * scale / times["batched_fused"]["median_ms"],
              "loop_over_batched_composed": loop_med * scale / times["batched_composed"]["median_ms"],
              "max_abs_variance_diff_fused_to_composed": float((v1 - v0).abs().max()),
              "max_abs_variance_diff_batched_to_loop": float((v1[:nl] - vl).abs().max())})
        return
    raise SystemExit(f"unknown step {args.step!r}")


def drive(args):
    """Every step in a child of its own, each under its time limit; the first failure ends the run."""
    common = ["--lg-b", str(args.lg_b), "--rounds", str(args.rounds), "--lg-n", str(args.lg_n), "--m", str(args.m),
              "--lg-loop", str(args.lg_loop)]
    steps = [("kernel", ["--ms", m]) for m in args.ms.split(",")] + [("cdgp", []), ("sgpr", [])]
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
    ap.add_argument("--lg-b", type=int, default=16)
    ap.add_argument("--ms", default="1024,4096,8192")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lg-n", type=int, default=20)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--lg-loop", type=int, default=14)
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
