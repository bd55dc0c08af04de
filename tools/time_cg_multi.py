#!/usr/bin/env python3
"""Multi-RHS CG (spmv_hip_csr_cg_multi: k CG recurrences sharing one SpMM per step) against k runs of csr_cg on the
same handle, in one process.

The matrices are the nlpkkt-like (3.5 M rows) and the FEM-shaped fembig (1.23 M rows) stand-ins, made symmetric
positive definite by adding each row's absolute sum + 1 to its diagonal.  For every matrix and every k, after the
card is settled as bench.py does, alternating rounds time one cg_multi(k) run of S steps and k csr_cg runs of S steps
(device time of the loop each, as the library reports it).  Prints per row: us per step of cg_multi, us per step and
right-hand side, k x csr_cg per step, and cg_multi / (k x csr_cg).

--profile K runs only cg_multi at that k (a 2-step warm-up, then one run of S steps) so that a separate
`rocprofv3 --kernel-trace --stats` pass sees the loop's kernels alone; --trace-report DIR then reads that pass's
kernel_stats.csv and splits the time into SpMM, the three vector kernels (mcg_dot_partial, mcg_update_x_r,
mcg_update_p: 11 n k sizeof(T) bytes per step, 2 n k sizeof(T) more for the initial r.r) and the small fold / scalar
kernels, with the vector kernels' bytes / time as a share of 8 TB/s.

usage: time_cg_multi.py [--matrices nlpkkt,fembig] [--ks 1,2,4,8,16] [--steps 20] [--rounds 3] [--out FILE]
       time_cg_multi.py --profile 8 --matrices nlpkkt [--steps 20]
       time_cg_multi.py --trace-report DIR --profile 8 --matrices nlpkkt [--steps 20] [--out FILE]"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402

HBM_PEAK = 8e12
MATRICES = {
    "nlpkkt": ("nlpkkt-like, fp64", lambda: synth.kkt_like()),
    "fembig": ("FEM-shaped (40, 40, 257), fp64", lambda: synth.fem_like((40, 40, 257), 1)),
}
VECTOR_KERNELS = {"mcg_dot_partial": 2, "mcg_update_x_r": 6, "mcg_update_p": 3}  # arrays of n x k moved per call


def make_spd(row_ptr, col, val):
    """symmetric stand-in with one diagonal entry per row -> SPD: each row's absolute sum + 1 onto its diagonal"""
    M = len(row_ptr) - 1
    diag = np.flatnonzero(col == np.repeat(np.arange(M, dtype=np.int32), np.diff(row_ptr)))
    if len(diag) != M:
        raise SystemExit("a row without its diagonal entry")
    val[diag] += np.add.reduceat(np.abs(val), row_ptr[:-1]) + 1.0
    return val


def load(key):
    label, make = MATRICES[key]
    M, row_ptr, col, val = make()
    return label, M, row_ptr, col, make_spd(row_ptr, col, val)


def settle(dev, ms=40.0):
    """Untimed launches for `ms` milliseconds, as bench.py's settle(): the card's transient after an idle stretch."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        dev.time(sp.CSR_AUTO, 0, 20, zero_y=False)


def sweep(args, ks):
    name, cus, _ = sp.device_name()
    lines = [f"device: {name} ({cus} CUs); S = {args.steps} steps per run, medians of {args.rounds} alternating rounds",
             "", "| matrix | k | cg_multi us / step | us / step / rhs | k x csr_cg us / step | cg_multi / (k x csr_cg) |",
             "|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    S = args.steps
    for key in args.matrices.split(","):
        label, M, row_ptr, col, val = load(key)
        rng = np.random.default_rng(7)
        B = rng.uniform(-1, 1, (M, max(ks)))
        with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
            settle(dev)
            multi = {k: [] for k in ks}
            single = []
            b = np.ascontiguousarray(B[:, 0])
            dev.cg(b, 2)                                               # warm-up of both loops' kernels
            for k in ks:
                dev.cg_multi(np.ascontiguousarray(B[:, :k]), 2)
            for _ in range(args.rounds):
                for k in ks:
                    Bk = np.ascontiguousarray(B[:, :k])
                    single.append(dev.cg(b, S)[2])
                    multi[k].append(dev.cg_multi(Bk, S)[3])
                single.append(dev.cg(b, S)[2])
        t_cg = float(np.median(single)) * 1e3 / S                     # us per csr_cg step
        for k in ks:
            t = float(np.median(multi[k])) * 1e3 / S
            row = (f"| {label} (M {M / 1e6:.2f} M, nnz {int(row_ptr[-1]) / 1e6:.1f} M) | {k} | {t:.1f} | {t / k:.1f} | "
                   f"{k * t_cg:.1f} | {t / (k * t_cg):.3f} |")
            lines.append(row)
            print(row, flush=True)
        lines.append(f"(csr_cg alone: {t_cg:.1f} us per step on {label})")
        print(lines[-1], flush=True)
    return lines


def profile(args):
    key = args.matrices.split(",")[0]
    label, M, row_ptr, col, val = load(key)
    B = np.random.default_rng(7).uniform(-1, 1, (M, args.profile))
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        dev.cg_multi(B, 2)
        _, _, _, ms = dev.cg_multi(B, args.steps)
    print(f"{label}: k = {args.profile}, {args.steps} steps in {ms:.3f} ms ({ms * 1e3 / args.steps:.1f} us / step)")


def trace_report(args):
    """kernel_stats.csv of a --profile run under rocprofv3 -> SpMM / vector kernels / small kernels per step"""
    files = sorted(glob.glob(os.path.join(args.trace_report, "**", "*kernel_stats.csv"), recursive=True),
                   key=os.path.getmtime)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {args.trace_report}")
    key = args.matrices.split(",")[0]
    M = {"nlpkkt": synth.KKT_GRID, "fembig": (40, 40, 257)}[key]
    lib = sp.lib()
    n = lib.synth_kkt_rows(*M) if key == "nlpkkt" else lib.synth_fem_rows(*M)
    k, S = args.profile, args.steps
    steps_total = S + 2                                                 # the warm-up run, then the timed one
    vb = 8
    groups = {"spmm": [0, 0.0], "vector": [0, 0.0], "small": [0, 0.0]}
    vec_bytes = 0.0
    rows = []
    for r in csv.DictReader(open(files[-1])):
        name, calls, total = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        hit = next((v for kname, v in VECTOR_KERNELS.items() if kname in name), None)
        if hit is not None:
            g = "vector"
            vec_bytes += calls * hit * n * k * vb
        elif "mcg_" in name or "solver_fold" in name or "solver_rank_sum" in name:   # (the shared fold / rank sum)
            g = "small"
        elif "spmm" in name or k == 1:
            g = "spmm"
        else:
            continue                                                    # upload's own launches
        groups[g][0] += calls
        groups[g][1] += total
        rows.append((g, name.split("(")[0][:70], calls, total / calls / 1e3))
    lines = [f"rocprofv3 --kernel-trace --stats, {os.path.relpath(files[-1], args.trace_report)}: "
             f"k = {k}, n = {n}, {steps_total} steps in all (2 warm-up + {S})", "",
             "| kernel | group | calls | us / call |", "|---|---|---|---|"]
    lines += [f"| `{nm}` | {g} | {c} | {us:.1f} |" for g, nm, c, us in sorted(rows)]
    lines += ["", "| group | us / step | share of the step |", "|---|---|---|"]
    step_total = sum(v[1] for v in groups.values()) / steps_total
    for g, (_, total) in groups.items():
        lines.append(f"| {g} | {total / steps_total / 1e3:.1f} | {total / steps_total / step_total:.2f} |")
    t_vec = groups["vector"][1] * 1e-9
    lines += ["", f"vector kernels: {vec_bytes / 1e9:.2f} GB in {t_vec * 1e3:.2f} ms = {vec_bytes / t_vec / 1e12:.2f} TB/s, "
              f"{vec_bytes / t_vec / HBM_PEAK:.2f} of 8 TB/s (11 n k sizeof(T) per step, 2 n k sizeof(T) per initial r.r)"]
    print("\n".join(lines))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="nlpkkt,fembig")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0, help="k of a single profiled cg_multi run (see above)")
    ap.add_argument("--trace-report", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_report:
        lines = trace_report(args)
    else:
        sp.hip_init(0)
        if args.profile:
            profile(args)
            return
        lines = sweep(args, [int(v) for v in args.ks.split(",")])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
