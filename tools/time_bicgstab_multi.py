#!/usr/bin/env python3
"""BiCGSTAB for k right-hand sides (spmv_hip_csr_bicgstab_multi: k recurrences sharing the two SpMMs of a step and the
k-wide apply) against k runs of spmv_hip_csr_bicgstab / _pbicgstab with the same preconditioner, in one session on one
box, fp64, on the three matrices of time_trsv.py (million, convdiff, fembig).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed
or ran out of time nothing more is started.  Per matrix, after the card is settled as bench.py does, and per
preconditioner (none, Jacobi, block-Jacobi (3), FSAI cap 32, AMG, Chebyshev degree 4):
  - one step: device time of S steps with tol = 0 of bicgstab and of bicgstab_multi for every k, in alternating rounds,
    medians; S is halved while bicgstab stops on its own before S steps (a stopped bicgstab's vector kernels return
    early, which would count as fast steps; bicgstab_multi's stopped columns do not return early);
  - the time to tol = 1e-8 for k = 8 (--tol-matrices, --tol-kinds): one bicgstab_multi solve against the sum of 8
    bicgstab solves, device time, median of three.
Prints markdown, matrix by matrix.

usage: time_bicgstab_multi.py [--matrices million,convdiff,fembig] [--ks 1,2,4,8,16] [--steps 50] [--rounds 3]
       [--tol-matrices convdiff] [--tol-kinds "amg,block_jacobi 3"] [--limit 420] [--out FILE]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KINDS = [("none", None), ("jacobi", dict(kind="jacobi")), ("block_jacobi 3", dict(kind="block_jacobi", block=3)),
         ("fsai cap 32", dict(kind="fsai", cap=32)), ("amg", dict(kind="amg")),
         ("chebyshev 4", dict(kind="chebyshev", degree=4))]
TOL, TOL_K, TOL_ITERS = 1e-8, 8, 3000


def one(key, S, R, ks, tol_kinds, out_path):
    import sparsematrixvectormultiplication_amd as sp
    from time_bicgstab import settle
    from time_trsv import MATRICES

    sp.hip_init(0)
    name, cus, _ = sp.device_name()

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    title, make, _ = MATRICES[key]
    M, rp, col, val = make()
    B = np.random.default_rng(7).uniform(-1, 1, (M, max(max(ks), TOL_K)))
    cols = [np.ascontiguousarray(B[:, j]) for j in range(TOL_K)]
    Bk = {k: np.ascontiguousarray(B[:, :k]) for k in set(ks) | {TOL_K}}
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries")
    emit()
    emit(f"device: {name.strip()} ({cus} CUs)")
    step_rows, tol_rows = [], []
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
        emit(f"SpMV (AUTO) {t_spmv:.1f} us")
        emit()
        for label, kw in KINDS:
            P = dev.preconditioner(**kw) if kw else None
            try:
                steps = S
                while steps > 5 and dev.bicgstab(cols[0], steps, precond=P)[2]["status"] != sp.BICG_RAN_ALL:
                    steps //= 2
                for k in ks:                                           # warm-up of every shape's kernels
                    dev.bicgstab_multi(Bk[k], 2, precond=P)
                single, multi, stopped = [], {k: [] for k in ks}, {k: 0 for k in ks}
                for _ in range(R):
                    for k in ks:
                        single.append(dev.bicgstab(cols[0], steps, precond=P)[3])
                        res = dev.bicgstab_multi(Bk[k], steps, precond=P)
                        multi[k].append(res[3])
                        stopped[k] = int(np.count_nonzero(res[2]["status"] != sp.BICG_RAN_ALL))
                t_one = float(np.median(single)) * 1e3 / steps
                for k in ks:
                    t = float(np.median(multi[k])) * 1e3 / steps
                    note = f" ({stopped[k]} columns stopped early)" if stopped[k] else ""
                    step_rows.append(f"| {label} | {k} | {t:.1f} | {t / k:.1f} | {t_one:.1f} | {k * t_one:.1f} | "
                                     f"{t / (k * t_one):.3f}{note} | {steps} |")
                if label not in tol_kinds:
                    continue
                # to tol = 1e-8, k = TOL_K
                t_multi, t_single = [], []
                for _ in range(3):
                    res = dev.bicgstab_multi(Bk[TOL_K], TOL_ITERS, tol=TOL, precond=P)
                    t_multi.append(res[3])
                    runs = [dev.bicgstab(c, TOL_ITERS, tol=TOL, precond=P) for c in cols]
                    t_single.append(sum(r[3] for r in runs))
                s_multi, s_single = res[2]["steps"], [r[2]["steps"] for r in runs]
                status = sorted(set(res[2]["status"].tolist()) | {r[2]["status"] for r in runs})
                tm, ts = float(np.median(t_multi)), float(np.median(t_single))
                tol_rows.append(f"| {label} | {int(s_multi.min())} .. {int(s_multi.max())} | {min(s_single)} .. "
                                f"{max(s_single)} | {status} | {tm:.2f} ({min(t_multi):.2f} .. {max(t_multi):.2f}) | "
                                f"{ts:.2f} ({min(t_single):.2f} .. {max(t_single):.2f}) | {tm / ts:.3f} |")
            finally:
                if P is not None:
                    P.close()
    emit("| P | k | bicgstab_multi us / step | us / step / rhs | bicgstab us / step | k x bicgstab us / step | "
         "bicgstab_multi / (k x bicgstab) | steps timed |")
    emit("|---|---|---|---|---|---|---|---|")
    for line in step_rows:
        emit(line)
    emit()
    if tol_rows:
        emit(f"| P, to tol {TOL:g}, k = {TOL_K} | bicgstab_multi steps (min .. max over columns) | bicgstab steps | "
             f"statuses seen | bicgstab_multi ms (min .. max of 3) | {TOL_K} bicgstab solves ms (min .. max of 3) | "
             f"bicgstab_multi / {TOL_K} bicgstab |")
        emit("|---|---|---|---|---|---|---|")
        for line in tol_rows:
            emit(line)
        emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tol-matrices", default="convdiff", help="the matrices that also run to tol")
    ap.add_argument("--tol-kinds", default="amg,block_jacobi 3", help="the preconditioners that run to tol there")
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",")]
    if args.one:
        tol_kinds = args.tol_kinds.split(",") if args.one in args.tol_matrices.split(",") else []
        one(args.one, args.steps, args.rounds, ks, tol_kinds, args.out)
        return 0
    head = (f"fp64; one step: device time of up to {args.steps} steps with tol = 0, medians of {args.rounds} alternating "
            f"rounds; to tol {TOL:g}: device time, median of three; everything of a matrix in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--ks", args.ks, "--steps", str(args.steps),
               "--rounds", str(args.rounds), "--tol-matrices", args.tol_matrices, "--tol-kinds", args.tol_kinds]
        cmd += ["--out", args.out] if args.out else []
        try:                     # the child writes its lines itself, as they come
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:      # a fault, an abort or the time limit: nothing more is started on the card
            print(f"{key}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
