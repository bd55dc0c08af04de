#!/usr/bin/env python3
"""LOBPCG (spmv_hip_csr_lobpcg) step by step: what one step costs and where, in one session on one box, fp64.

Matrices: million and fembig of time_trsv.py and the nlpkkt-like KKT stand-in of time_minres.py (time_trsv.py's third
matrix, convdiff, is not symmetric).  Each matrix runs in a child process of its own under its own time limit
(--limit seconds); after a child that failed or ran out of time nothing more is started.  Per matrix, after the card
is settled as bench.py does, and per k:
  - one step: device time of a solve of S steps with tol = 0 over S (it includes the step-0 product and the final
    residual product, spread over the steps), and the host time inside spmv_lobpcg_rr per step;
  - the SpMM: spmv_hip_csr_spmm_time, median;
  - the Jacobi and FSAI applies: wall time of R asynchronous spmv_hip_precond_apply_multi_on calls between two
    synchronisations;
  - the Gram and update passes (nb = 3): wall time of spmv_hip_lobpcg_gram / _update, median of R calls, less the same
    call on 4 rows (each call allocates, transfers its small matrices and waits: the 4-row call is that overhead);
    their bytes (6 resp. 10 arrays of n x k doubles) over that time, next to the box's stream probe;
  - the rest of a step (the residual pass, the small transfers and the two waits per step), by difference.
Then steps and device ms to tol = 1e-8 at k = 8 with no preconditioner, Jacobi and FSAI (skipped for the indefinite
matrix), within --cap steps.  One run; prints markdown.

usage: time_lobpcg.py [--matrices nlpkkt,fembig,million] [--ks 4,8,16] [--steps 20] [--rounds 5] [--cap 400]
       [--limit 420] [--out FILE]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL, TOL_K = 1e-8, 8
STATUS = {0: "ran all", 1: "converged", 2: "breakdown"}


def one(key, S, R, ks, cap, out_path):
    import sparsematrixvectormultiplication_amd as sp
    from sparsematrixvectormultiplication_amd import _native as nat
    from sparsematrixvectormultiplication_amd import synth
    from time_bicgstab import settle
    from time_trsv import MATRICES

    matrices = {"million": MATRICES["million"][:2], "fembig": MATRICES["fembig"][:2],
                "nlpkkt": ("nlpkkt-like, indefinite", lambda: synth.kkt_like())}
    sp.hip_init(0)
    name, cus, _ = sp.device_name()

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert nat.lib().spmv_hip_malloc(C.byref(p), nbytes) == 0, nat.lib().spmv_hip_last_error()
        return p

    def wall(call, reps):
        out = []
        for _ in range(reps):
            sp.hip_sync()
            t = time.perf_counter()
            call()
            sp.hip_sync()
            out.append((time.perf_counter() - t) * 1e6)
        return float(np.median(out))

    title, make = matrices[key]
    M, rp, col, val = make()
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries")
    emit()
    probe = sp.stream_probe()[1]
    emit(f"device: {name.strip()} ({cus} CUs); stream probe {(1 << 30) / probe / 1e9:.2f} TB/s")
    emit()
    rows = []
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        J = dev.preconditioner("jacobi") if key != "nlpkkt" else None
        F = dev.preconditioner("fsai") if key != "nlpkkt" else None
        for k in ks:
            X0 = np.random.default_rng(0).standard_normal((M, k))
            dev.lobpcg(k, 2, X0=X0)                                       # warm-up of this shape's kernels
            res = dev.lobpcg(k, S, X0=X0)
            step, host = res[5] * 1e3 / S, res[4]["host_ms"] * 1e3 / S
            spmm = float(np.median(dev.time_spmm(k, 3, 20))) * 1e3
            nbytes = M * k * 8
            bufs = [dmalloc(nbytes + 128) for _ in range(7)]
            for b in bufs[:6]:
                nat.lib().spmv_hip_memcpy_h2d(b, X0.ctypes.data_as(C.c_void_p), nbytes)
            blocks = [b.value for b in bufs]
            apply_us = {}
            for label, P in (("jacobi", J), ("fsai", F)):
                if P is not None:
                    P.apply_multi_on(blocks[0], blocks[1], k, blocks[6])
                    apply_us[label] = wall(lambda: [P.apply_multi_on(blocks[0], blocks[1], k, blocks[6])
                                                    for _ in range(10)], R) / 10
            Cm = np.random.default_rng(1).uniform(-1, 1, (3 * k, k)) / (3 * k)
            gram = wall(lambda: sp.lobpcg_gram(M, k, 3, blocks[:3], blocks[3:6]), R) - \
                wall(lambda: sp.lobpcg_gram(4, k, 3, blocks[:3], blocks[3:6]), R)
            upd = wall(lambda: sp.lobpcg_update(M, k, 3, blocks[:3], blocks[3:6], Cm, Cm, blocks[0], blocks[2],
                                                blocks[3], blocks[5]), R) - \
                wall(lambda: sp.lobpcg_update(4, k, 3, blocks[:3], blocks[3:6], Cm, Cm, blocks[0], blocks[2], blocks[3],
                                              blocks[5]), R)
            for b in bufs:
                nat.lib().spmv_hip_free(b)
            rest = step - spmm * (1 + 2.0 / S) - gram - upd - host
            ap = " / ".join(f"{apply_us[n]:.0f}" if n in apply_us else "-" for n in ("jacobi", "fsai"))
            rows.append(f"| {k} | {step:.0f} | {spmm:.0f} | {ap} | {gram:.0f} | {6 * nbytes / gram / 1e6:.2f} | {upd:.0f} | "
                        f"{10 * nbytes / upd / 1e6:.2f} | {host:.0f} | {rest:.0f} | {(gram + upd) / spmm:.2f} | "
                        f"{res[4]['restarts']} |")
        emit("| k | step us (no P) | SpMM us | apply us (Jacobi / FSAI) | Gram us | Gram TB/s | update us | update TB/s | "
             "host us | rest us (by difference) | (Gram + update) / SpMM | restarts |")
        emit("|---|---|---|---|---|---|---|---|---|---|---|---|")
        for line in rows:
            emit(line)
        emit()
        emit(f"| P, to tol {TOL:g}, k = {TOL_K}, at most {cap} steps | steps | status | restarts | device ms | host ms | "
             "largest true residual / anorm |")
        emit("|---|---|---|---|---|---|---|")
        X0 = np.random.default_rng(0).standard_normal((M, TOL_K))
        for label, P in (("none", None), ("jacobi", J), ("fsai cap 32", F)):
            if label != "none" and P is None:
                continue
            w, X, th, rh, info, ms = dev.lobpcg(TOL_K, cap, tol=TOL, precond=P, X0=X0)
            emit(f"| {label} | {info['steps']} | {STATUS[info['status']]} | {info['restarts']} | {ms:.1f} | "
                 f"{info['host_ms']:.1f} | {info['resid'].max() / info['anorm']:.2e} |")
        emit()
        for P in (J, F):
            if P is not None:
                P.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="nlpkkt,fembig,million")
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=400)
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",")]
    if args.one:
        one(args.one, args.steps, args.rounds, ks, args.cap, args.out)
        return 0
    head = (f"fp64, one run; one step: device time of {args.steps} steps with tol = 0; passes: medians of {args.rounds} "
            "calls; everything of a matrix in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--ks", args.ks, "--steps", str(args.steps),
               "--rounds", str(args.rounds), "--cap", str(args.cap)] + (["--out", args.out] if args.out else [])
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
