#!/usr/bin/env python3
"""The FSAI preconditioner against Jacobi, block-Jacobi (3) and multicolour ILU(0) in one session on one box, fp64, on
the three matrices of time_trsv.py (million, convdiff, fembig).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed
or ran out of time nothing more is started.  Per matrix, after the card is settled as bench.py does: the handle's SpMV
(CsrDevice.time, median of 100); the FSAI build split and the plans of its two handles (Preconditioner.fsai_info);
one apply of each preconditioner, host time over as many asynchronous calls on device vectors between two
synchronisations as fill --window milliseconds (at least R; launches included), repeated three times, the median reported
with the spread; a solver step (device time of S steps with tol = 0, halved while the solve stops on its own before them, three repeats,
median); and steps and milliseconds to tol 1e-8 (PCG on the symmetric matrices,
right-preconditioned BiCGSTAB on the stencil).  Prints markdown, matrix by matrix.

usage: time_fsai.py [--matrices million,convdiff,fembig] [--steps 200] [--reps 20] [--caps 32] [--window 30]
       [--limit 420] [--out FILE]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def one(key, S, R, caps, window_ms, out_path):
    import sparsematrixvectormultiplication_amd as sp
    from time_bicgstab import settle
    from time_trsv import MATRICES, Vec, us_per_call

    sp.hip_init(0)
    name, cus, _ = sp.device_name()

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    title, make, method = MATRICES[key]
    M, rp, col, val = make()
    b = np.random.default_rng(7).uniform(-1, 1, M)
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries ({method})")
    emit()
    emit(f"device: {name.strip()} ({cus} CUs)")
    med3 = lambda f: sorted(f() for _ in range(3))  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
        solve = (lambda **kw: dev.pcg(b, **kw)) if method == "pcg" else (lambda **kw: dev.bicgstab(b, **kw))
        ms = lambda res: res[4] if method == "pcg" else res[3]        # noqa: E731
        info = lambda res: res[3] if method == "pcg" else res[2]      # noqa: E731

        def step_us(P):
            """(us per step, steps timed): S steps with tol = 0, fewer where the solve stops on its own before them (a
            stopped solve's vector kernels return early, which would count as fast steps)"""
            steps = S
            while steps > 5 and info(solve(iters=steps, precond=P))["status"] != 0:
                steps //= 2
            return med3(lambda: ms(solve(iters=steps, precond=P)) * 1e3 / steps)[1], steps

        t_plain, s_plain = step_us(None)
        emit(f"SpMV (AUTO, {sp.device.CSR_STREAM_KERNELS[dev.info()['stream_kernel']]}) {t_spmv:.1f} us; "
             f"unpreconditioned {method} step {t_plain:.1f} us (over {s_plain} steps)")
        emit()
        kinds = [("jacobi", dict(kind="jacobi")), ("block_jacobi 3", dict(kind="block_jacobi", block=3)),
                 ("ilu0 multicolor", dict(kind="ilu0", ordering="multicolor"))]
        kinds += [(f"fsai cap {c}", dict(kind="fsai", cap=c)) for c in caps]
        d_r, d_z = Vec(b), Vec(np.zeros(M))
        rows, builds = [], []
        for label, kw in kinds:
            with dev.preconditioner(**kw) as P:
                if kw["kind"] == "fsai":
                    f = P.fsai_info()
                    builds.append(f"| {label} | {f['entries'] / 1e6:.2f} | {f['entries'] / int(rp[-1]):.2f} | "
                                  f"{f['truncated_rows']} | {f['widest']} | {sp.device.FSAI_PLANS[f['plan_g']]} / "
                                  f"{sp.device.FSAI_PLANS[f['plan_gt']]} | {f['analysis_us'] / 1e3:.0f} | "
                                  f"{f['build_us'] / 1e3:.0f} | {f['upload_us'] / 1e3:.0f} |")
                call = lambda: P.apply_on(d_r.p.value, d_z.p.value)  # noqa: E731
                reps = max(R, int(np.ceil(window_ms * 1e3 / us_per_call(call, R))))   # a window of window_ms at least
                t_apply = med3(lambda: us_per_call(call, reps))
                t_step, s_step = step_us(P)
                res = solve(iters=3000, tol=1e-8, precond=P)
                t_tol = med3(lambda: ms(solve(iters=3000, tol=1e-8, precond=P)))
            rows.append(f"| {label} | {t_apply[1]:.1f} ({t_apply[0]:.1f} .. {t_apply[2]:.1f}) | {t_apply[1] / t_spmv:.2f} | "
                        f"{t_step:.1f} ({s_step}) | {t_step / t_plain:.2f} | {info(res)['steps']} | {info(res)['status']} | "
                        f"{t_tol[1]:.2f} ({t_tol[0]:.2f} .. {t_tol[2]:.2f}) |")
        d_r.close(), d_z.close()
        emit("| FSAI build | entries of G (M) | / entries of A | rows cut by the cap | largest row | plan of G / G^T | "
             "analysis ms | device build ms | uploads + transpose ms |")
        emit("|---|---|---|---|---|---|---|---|---|")
        for line in builds:
            emit(line)
        emit()
        emit(f"| {method} with | apply us (min .. max of 3) | x SpMV | us / step (steps timed) | / unpreconditioned step | "
             "steps to 1e-8 | status | ms to 1e-8 (min .. max of 3) |")
        emit("|---|---|---|---|---|---|---|---|")
        for line in rows:
            emit(line)
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--caps", default="32")
    ap.add_argument("--window", type=float, default=30.0, help="milliseconds one timed run of applies lasts at least")
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    caps = [int(c) for c in args.caps.split(",")]
    if args.one:
        one(args.one, args.steps, args.reps, caps, args.window, args.out)
        return 0
    head = (f"fp64; applies: host time over windows of at least {args.window:g} ms of asynchronous calls; solver steps: "
            f"device time of up to {args.steps} steps with tol = 0; every figure the median of three repeats in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--steps", str(args.steps), "--reps",
               str(args.reps), "--caps", args.caps, "--window", str(args.window)] + (["--out", args.out] if args.out else [])
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
