#!/usr/bin/env python3
"""MINRES for k right-hand sides (spmv_hip_csr_minres_multi: k recurrences with a shift per column sharing the one SpMM
of a step and the k-wide apply) against k runs of spmv_hip_csr_minres with the same preconditioner, in one session on
one box, on the three matrices of time_trsv.py (million, convdiff, fembig) and the nlpkkt-like KKT matrix.

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed
or ran out of time nothing more is started.  Per matrix, after the card is settled as bench.py does:
  - the stream probe's rate, the SpMV and the SpMM for every k (time_spmm), and from them the expected step: one SpMM
    plus 15 values per row and column at the probe's rate;
  - per preconditioner (none, Jacobi of the copy with |diagonal|): device time of S steps with tol = 0 of minres and of
    minres_multi for every k, in alternating rounds, medians; the vector part of a step is the step minus the SpMM;
  - the time to tol = 1e-8 for k = 8 (--tol-matrices, symmetric matrices only): one minres_multi solve against the sum
    of 8 minres solves, device time, median of three.
The convection-diffusion stencil is not symmetric: MINRES solves nothing on it, its steps cost what they cost on any
matrix of that shape, and only they are timed there.  Prints markdown, matrix by matrix.

usage: time_minres_multi.py [--matrices million,convdiff,fembig,nlpkkt] [--ks 1,2,4,8,16] [--steps 30] [--rounds 3]
       [--dtype fp64|fp32] [--tol-matrices fembig] [--limit 420] [--out FILE]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL, TOL_K, TOL_ITERS = 1e-8, 8, 3000
VALUES_PER_ROW = 15   # the arrays a step's vector kernels read or write beside the product (README)


def matrices():
    from sparsematrixvectormultiplication_amd import synth
    from time_trsv import MATRICES
    out = {key: (title, make) for key, (title, make, _) in MATRICES.items()}
    out["nlpkkt"] = ("nlpkkt-like, symmetric indefinite", lambda: synth.kkt_like())
    return out


def with_abs_diagonal(rp, col, val):
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    out = val.copy()
    pos = np.flatnonzero(col == rows)
    out[pos] = np.abs(out[pos])
    return out


def one(key, S, R, ks, dtype, to_tol, out_path):
    import sparsematrixvectormultiplication_amd as sp
    from time_bicgstab import settle

    sp.hip_init(0)
    name, cus, _ = sp.device_name()

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    title, make = matrices()[key]
    M, rp, col, val = make()
    val = np.ascontiguousarray(val, dtype=dtype)
    vb = np.dtype(dtype).itemsize
    B = np.random.default_rng(7).uniform(-1, 1, (M, max(max(ks), TOL_K))).astype(dtype)
    cols = [np.ascontiguousarray(B[:, j]) for j in range(TOL_K)]
    Bk = {k: np.ascontiguousarray(B[:, :k]) for k in set(ks) | {TOL_K}}
    emit(f"## {key}: {title}, {np.dtype(dtype).name}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries")
    emit()
    emit(f"device: {name.strip()} ({cus} CUs)")
    step_rows, tol_rows = [], []
    with sp.CsrDevice(M, M, rp, col, val) as dev, \
            sp.CsrDevice(M, M, rp, col, with_abs_diagonal(rp, col, val)) as dev_abs:
        settle(dev)
        probe_ms = sp.stream_probe(1 << 30, 3, 10)[0]
        rate = (1 << 30) / (probe_ms * 1e-3)                     # bytes per second
        t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
        t_spmm = {k: float(np.median(dev.time_spmm(k, 3, 30))) * 1e3 for k in ks}
        expect = {k: t_spmm[k] + VALUES_PER_ROW * M * k * vb / rate * 1e6 for k in ks}
        emit(f"stream probe {rate / 1e12:.2f} TB/s; SpMV (AUTO) {t_spmv:.1f} us; SpMM us: "
             + ", ".join(f"k = {k}: {t_spmm[k]:.1f}" for k in ks))
        emit()
        for label, kw in (("none", None), ("jacobi of abs(diag)", dict(kind="jacobi"))):
            P = dev_abs.preconditioner(**kw) if kw else None
            try:
                steps = S
                while steps > 5 and dev.minres(cols[0], steps, precond=P)[2]["status"] != sp.MINRES_RAN_ALL:
                    steps //= 2
                for k in ks:                                           # warm-up of every shape's kernels
                    dev.minres_multi(Bk[k], 2, precond=P)
                single, multi, stopped = [], {k: [] for k in ks}, {k: 0 for k in ks}
                for _ in range(R):
                    for k in ks:
                        single.append(dev.minres(cols[0], steps, precond=P)[3])
                        res = dev.minres_multi(Bk[k], steps, precond=P)
                        multi[k].append(res[3])
                        stopped[k] = int(np.count_nonzero(res[2]["status"] != sp.MINRES_RAN_ALL))
                t_one = float(np.median(single)) * 1e3 / steps
                for k in ks:
                    t = float(np.median(multi[k])) * 1e3 / steps
                    vec = t - t_spmm[k]
                    tbs = VALUES_PER_ROW * M * k * vb / (vec * 1e-6) / 1e12 if vec > 0 else float("nan")
                    note = f" ({stopped[k]} columns stopped early)" if stopped[k] else ""
                    step_rows.append(f"| {label} | {k} | {t:.1f} | {expect[k]:.1f} | {t / expect[k]:.2f} | {t_spmm[k]:.1f} | "
                                     f"{vec:.1f} | {tbs:.2f} | {t_one:.1f} | {k * t_one:.1f} | "
                                     f"{t / (k * t_one):.3f}{note} | {steps} |")
                if not to_tol:
                    continue
                t_multi, t_single = [], []
                for _ in range(3):
                    res = dev.minres_multi(Bk[TOL_K], TOL_ITERS, tol=TOL, precond=P)
                    t_multi.append(res[3])
                    runs = [dev.minres(c, TOL_ITERS, tol=TOL, precond=P) for c in cols]
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
    emit("| P | k | minres_multi us / step | expected us | measured / expected | SpMM us | vector part us | vector part TB/s "
         "(15 values) | minres us / step | k x minres us / step | minres_multi / (k x minres) | steps timed |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for line in step_rows:
        emit(line)
    emit()
    if tol_rows:
        emit(f"| P, to tol {TOL:g}, k = {TOL_K} | minres_multi steps (min .. max over columns) | minres steps | "
             f"statuses seen | minres_multi ms (min .. max of 3) | {TOL_K} minres solves ms (min .. max of 3) | "
             f"minres_multi / {TOL_K} minres |")
        emit("|---|---|---|---|---|---|---|")
        for line in tol_rows:
            emit(line)
        emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig,nlpkkt")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", choices=("fp64", "fp32"), default="fp64")
    ap.add_argument("--tol-matrices", default="fembig", help="the (symmetric) matrices that also run to tol")
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",")]
    dtype = np.float64 if args.dtype == "fp64" else np.float32
    if args.one:
        one(args.one, args.steps, args.rounds, ks, dtype, args.one in args.tol_matrices.split(","), args.out)
        return 0
    head = (f"{args.dtype}; one step: device time of up to {args.steps} steps with tol = 0, medians of {args.rounds} "
            f"alternating rounds; to tol {TOL:g}: device time, median of three; everything of a matrix in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--ks", args.ks, "--steps", str(args.steps),
               "--rounds", str(args.rounds), "--dtype", args.dtype, "--tol-matrices", args.tol_matrices]
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
