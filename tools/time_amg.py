#!/usr/bin/env python3
"""The AMG preconditioner against Jacobi, block-Jacobi (3), FSAI and multicolour ILU(0) in one session on one box, fp64,
on the three matrices of time_trsv.py (million, convdiff, fembig).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed
or ran out of time nothing more is started.  Per matrix, after the card is settled as bench.py does: the handle's SpMV
(CsrDevice.time, median of 100); the AMG build split, levels, operator complexity and launches per apply
(Preconditioner.amg_info), with chain on and off; one apply of each preconditioner, host time over as many
asynchronous calls on device vectors between two synchronisations as fill --window milliseconds (at least R; launches
included), three times, the median with the spread; a solver step (device time of S steps with tol = 0, halved while
the solve stops on its own before them); steps and milliseconds to tol 1e-8 (PCG on the symmetric matrices,
right-preconditioned BiCGSTAB on the stencil); on the symmetric matrices pcg_multi at k = 8 to 1e-8 with Jacobi, FSAI
and AMG; on the million-row matrix lobpcg at k = 8 to 1e-8 within 400 steps with the same three.  Prints markdown.

--max-entries: a matrix with more entries than this (millions) gets no AMG (the host setup forms R A P on one thread);
its table then holds the other kinds alone.

--setup: the AMG build alone, setup="host" against setup="device" on the same handle in the same process: three builds
of each (alternating), the build wall time and the Preconditioner.amg_info() split as the median with the smallest and
largest, the device setup's phases (Preconditioner.amg_setup_info()), and whether the two hold the same bytes (every
level's operators and scalars, and one apply); exit status 1 if they do not.

usage: time_amg.py [--matrices million,convdiff,fembig] [--steps 200] [--reps 20] [--window 30] [--limit 420]
       [--max-entries 200] [--setup] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STATUS = {0: "ran all", 1: "converged", 2: "breakdown"}


def one(key, S, R, window_ms, max_entries, out_path):
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
    with_amg = int(rp[-1]) <= max_entries * 1e6
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
        solve = (lambda **kw: dev.pcg(b, **kw)) if method == "pcg" else (lambda **kw: dev.bicgstab(b, **kw))
        ms = lambda res: res[4] if method == "pcg" else res[3]        # noqa: E731
        info = lambda res: res[3] if method == "pcg" else res[2]      # noqa: E731

        def step_us(P):
            steps = S
            while steps > 5 and info(solve(iters=steps, precond=P))["status"] != 0:
                steps //= 2
            return med3(lambda: ms(solve(iters=steps, precond=P)) * 1e3 / steps)[1], steps

        t_plain, s_plain = step_us(None)
        emit(f"SpMV (AUTO, {sp.device.CSR_STREAM_KERNELS[dev.info()['stream_kernel']]}) {t_spmv:.1f} us; "
             f"unpreconditioned {method} step {t_plain:.1f} us (over {s_plain} steps)")
        emit()
        kinds = [("jacobi", dict(kind="jacobi")), ("block_jacobi 3", dict(kind="block_jacobi", block=3)),
                 ("ilu0 multicolor", dict(kind="ilu0", ordering="multicolor")), ("fsai cap 32", dict(kind="fsai", cap=32))]
        if with_amg:
            kinds += [("amg", dict(kind="amg")), ("amg, chain off", dict(kind="amg", chain=False))]
        else:
            emit(f"no AMG: more than {max_entries:g} M entries")
            emit()
        d_r, d_z = Vec(b), Vec(np.zeros(M))
        rows, builds = [], []
        for label, kw in kinds:
            t0 = time.perf_counter()
            with dev.preconditioner(**kw) as P:
                wall = (time.perf_counter() - t0) * 1e3
                if kw["kind"] == "amg":
                    f = P.amg_info()
                    builds.append(f"| {label} | {f['levels']} | {' '.join(str(r) for r in f['rows'])} | "
                                  f"{f['complexity_x1000'] / 1e3:.3f} | {f['first_chained']} | {f['launches']} | "
                                  f"{'direct' if f['coarsest'] == sp.device.AMG_DIRECT else 'smooth'} | "
                                  f"{f['download_us'] / 1e3:.0f} | {f['setup_us'] / 1e3:.0f} | {f['upload_us'] / 1e3:.0f} | "
                                  f"{wall:.0f} |")
                call = lambda: P.apply_on(d_r.p.value, d_z.p.value)  # noqa: E731
                reps = max(R, int(np.ceil(window_ms * 1e3 / us_per_call(call, R))))
                t_apply = med3(lambda: us_per_call(call, reps))
                t_step, s_step = step_us(P)
                res = solve(iters=3000, tol=1e-8, precond=P)
                t_tol = med3(lambda: ms(solve(iters=3000, tol=1e-8, precond=P)))
            rows.append(f"| {label} | {t_apply[1]:.1f} ({t_apply[0]:.1f} .. {t_apply[2]:.1f}) | {t_apply[1] / t_spmv:.2f} | "
                        f"{t_step:.1f} ({s_step}) | {t_step / t_plain:.2f} | {info(res)['steps']} | {info(res)['status']} | "
                        f"{t_tol[1]:.2f} ({t_tol[0]:.2f} .. {t_tol[2]:.2f}) |")
        d_r.close(), d_z.close()
        if builds:
            emit("| AMG build | levels | rows per level | operator complexity | first chained level | launches per apply | "
                 "coarsest | download + canonical rows ms | host setup ms | uploads ms | build wall ms |")
            emit("|---|---|---|---|---|---|---|---|---|---|---|")
            for line in builds:
                emit(line)
            emit()
        emit(f"| {method} with | apply us (min .. max of 3) | x SpMV | us / step (steps timed) | / unpreconditioned step | "
             "steps to 1e-8 | status | ms to 1e-8 (min .. max of 3) |")
        emit("|---|---|---|---|---|---|---|---|")
        for line in rows:
            emit(line)
        emit()
        wide = [("jacobi", dict(kind="jacobi")), ("fsai cap 32", dict(kind="fsai", cap=32))]
        wide += [("amg", dict(kind="amg"))] if with_amg else []
        if method == "pcg":
            k = 8
            B = np.random.default_rng(8).uniform(-1, 1, (M, k))
            emit(f"| pcg_multi, k = {k}, with | steps to 1e-8 (min .. max over the columns) | ms to 1e-8 (min .. max of 3) | "
                 "ms per column |")
            emit("|---|---|---|---|")
            for label, kw in wide:
                with dev.preconditioner(**kw) as P:
                    res = dev.pcg_multi(B, 3000, tol=1e-8, precond=P)
                    t = med3(lambda: dev.pcg_multi(B, 3000, tol=1e-8, precond=P)[4])
                emit(f"| {label} | {int(res[3]['steps'].min())} .. {int(res[3]['steps'].max())} | {t[1]:.2f} ({t[0]:.2f} .. "
                     f"{t[2]:.2f}) | {t[1] / k:.2f} |")
            emit()
        if key == "million":
            k, cap = 8, 400
            X0 = np.random.default_rng(0).standard_normal((M, k))
            emit(f"| lobpcg, k = {k}, to tol 1e-8, at most {cap} steps, with | steps | status | restarts | device ms | host ms | "
                 "largest true residual / anorm |")
            emit("|---|---|---|---|---|---|---|")
            for label, kw in wide:
                with dev.preconditioner(**kw) as P:
                    w, X, th, rh, li, lms = dev.lobpcg(k, cap, tol=1e-8, precond=P, X0=X0)
                emit(f"| {label} | {li['steps']} | {STATUS[li['status']]} | {li['restarts']} | {lms:.1f} | {li['host_ms']:.1f} | "
                     f"{li['resid'].max() / li['anorm']:.2e} |")
            emit()


def one_setup(key, out_path):
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

    title, make, method = MATRICES[key]
    M, rp, col, val = make()
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries")
    emit()
    emit(f"device: {name.strip()} ({cus} CUs)")
    emit()
    spread = lambda v: f"{sorted(v)[1]:.1f} ({min(v):.1f} .. {max(v):.1f})"  # noqa: E731
    phases = [k for k in sp.device.PRECOND_AMG_SETUP_INFO if k != "setup"]
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        runs = {"host": [], "device": []}
        shape = {}
        for _ in range(3):
            for setup in ("host", "device"):
                t0 = time.perf_counter()
                with dev.preconditioner("amg", setup=setup) as P:
                    wall = (time.perf_counter() - t0) * 1e3
                    f, g = P.amg_info(), P.amg_setup_info()
                    assert g["setup"] == sp.device.AMG_SETUPS[setup]
                    runs[setup].append((wall, f, g))
                    shape[setup] = (f["rows"], f["entries"], f["launches"], f["first_chained"], f["coarsest"])
        same = shape["host"] == shape["device"]
        with dev.preconditioner("amg", setup="host") as Ph, dev.preconditioner("amg", setup="device") as Pd:
            b = np.random.default_rng(7).uniform(-1, 1, M)
            same = same and Ph.apply(b).tobytes() == Pd.apply(b).tobytes()
            for lh, ld in zip(Ph.levels(), Pd.levels()):        # every operator and scalar of every level, byte for byte
                same = same and sorted(lh) == sorted(ld) and all(
                    np.array(u).tobytes() == np.array(v).tobytes()
                    for k in lh for u, v in zip(*[x[k] if isinstance(x[k], tuple) else (x[k],) for x in (lh, ld)]))
        f = runs["host"][0][1]
        emit(f"levels {f['levels']}, rows per level {' '.join(str(r) for r in f['rows'])}, operator complexity "
             f"{f['complexity_x1000'] / 1e3:.3f}; the two setups hold the same bytes (every operator, w, rho and kind of "
             f"every level, and one apply): {'yes' if same else 'NO'}")
        emit()
        emit("| setup | build wall ms (min .. max of 3) | download + canonical rows ms | setup ms | uploads ms |")
        emit("|---|---|---|---|---|")
        for setup in ("host", "device"):
            r = runs[setup]
            emit(f"| {setup} | {spread([w for w, _, _ in r])} | " +
                 " | ".join(spread([f[k] / 1e3 for _, f, _ in r]) for k in ("download_us", "setup_us", "upload_us")) + " |")
        emit()
        emit("| device setup phase | ms (min .. max of 3) |")
        emit("|---|---|")
        for k in phases:
            emit(f"| {k[:-3]} | {spread([g[k] / 1e3 for _, _, g in runs['device']])} |")
        emit(f"| all phases | {spread([sum(g[k] for k in phases) / 1e3 for _, _, g in runs['device']])} |")
        emit()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=float, default=30.0, help="milliseconds one timed run of applies lasts at least")
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--max-entries", type=float, default=200.0, help="millions of entries up to which AMG is built")
    ap.add_argument("--setup", action="store_true", help="time the AMG build alone: host setup against device setup")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        if args.setup:
            return one_setup(args.one, args.out)
        one(args.one, args.steps, args.reps, args.window, args.max_entries, args.out)
        return 0
    if args.setup:
        head = "fp64; three builds of each setup in one process, alternating; the median with the smallest and largest"
    else:
        head = (f"fp64; applies: host time over windows of at least {args.window:g} ms of asynchronous calls; solver steps: "
                f"device time of up to {args.steps} steps with tol = 0; every figure the median of three repeats in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--steps", str(args.steps), "--reps",
               str(args.reps), "--window", str(args.window), "--max-entries", str(args.max_entries)]
        cmd += ["--setup"] if args.setup else []
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
