#!/usr/bin/env python3
"""The Chebyshev polynomial preconditioner at degrees 2, 4 and 8 against Jacobi, block-Jacobi (3), FSAI and AMG in one
session on one box, fp64, on the three matrices of time_trsv.py (million, convdiff, fembig).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed
or ran out of time nothing more is started.  Per matrix, after the card is settled as bench.py does: the handle's SpMV
(CsrDevice.time, median of 100) and the stream probe; the EXPECTATION of an apply of degree m, printed before anything
of the new kind is timed: (m - 1) SpMVs plus m - 1 passes of 7 values a row and one of 4 at the probe's rate; the build
(host clock around preconditioner() and the split of cheb_info); one apply of each preconditioner, host time over as
many asynchronous calls on device vectors between two synchronisations as fill --window milliseconds (at least R;
launches included), repeated three times, the median with the spread; the fused pass by difference,
(apply(8) - apply(2)) / 6 - SpMV, as TB/s of its 7 values a row; steps and milliseconds to tol 1e-8 (PCG on the
symmetric matrices, right-preconditioned BiCGSTAB on the stencil); and on the symmetric matrices pcg_multi with k = 8
at degree 4 against 8 pcg solves of its columns.  Prints markdown, matrix by matrix.

usage: time_chebyshev.py [--matrices million,convdiff,fembig] [--reps 20] [--window 30] [--others jacobi,block,fsai,amg]
       [--limit 420] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEGREES = (2, 4, 8)
OTHERS = {"jacobi": ("jacobi", dict(kind="jacobi")), "block": ("block_jacobi 3", dict(kind="block_jacobi", block=3)),
          "fsai": ("fsai cap 32", dict(kind="fsai", cap=32)), "amg": ("amg", dict(kind="amg"))}


def one(key, R, window_ms, others, out_path):
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
    med3 = lambda f: sorted(f() for _ in range(3))  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        settle(dev)
        t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
        probe = (1 << 30) / (sp.stream_probe()[1] * 1e-3) / 1e12
        emit(f"device: {name.strip()} ({cus} CUs); stream probe {probe:.2f} TB/s; SpMV (AUTO, "
             f"{sp.device.CSR_STREAM_KERNELS[dev.info()['stream_kernel']]}) {t_spmv:.1f} us")
        emit()
        pass7, pass4 = 7 * 8 * M / probe / 1e6, 4 * 8 * M / probe / 1e6
        expect = {m: (m - 1) * (t_spmv + pass7) + pass4 for m in DEGREES}
        emit(f"expected before timing: a pass of 7 values a row {pass7:.1f} us, of 4 values {pass4:.1f} us; an apply of "
             + ", ".join(f"degree {m}: {expect[m]:.1f} us" for m in DEGREES))
        emit()
        solve = (lambda **kw: dev.pcg(b, **kw)) if method == "pcg" else (lambda **kw: dev.bicgstab(b, **kw))
        ms = lambda res: res[4] if method == "pcg" else res[3]        # noqa: E731
        info = lambda res: res[3] if method == "pcg" else res[2]      # noqa: E731
        kinds = [OTHERS[o] for o in others] + [(f"chebyshev {m}", dict(kind="chebyshev", degree=m)) for m in DEGREES]
        d_r, d_z = Vec(b), Vec(np.zeros(M))
        builds, applies = [], {}
        emit(f"| {method} with | apply us (min .. max of 3) | expected us | x SpMV | steps to 1e-8 | status | "
             "ms to 1e-8 (min .. max of 3) | build wall ms |")
        emit("|---|---|---|---|---|---|---|---|")
        for label, kw in kinds:
            t0 = time.perf_counter()
            with dev.preconditioner(**kw) as P:
                wall = (time.perf_counter() - t0) * 1e3
                if kw["kind"] == "chebyshev":
                    c = P.cheb_info()
                    builds.append(f"| {label} | {c['lmin']:.4g} | {c['lmax']:.4g} | {c['gershgorin']:.4g} | {c['products']} | "
                                  f"{sp.device.FSAI_PLANS[c['plan']]} | {c['download_us'] / 1e3:.0f} | "
                                  f"{c['upload_us'] / 1e3:.0f} | {wall:.0f} |")
                call = lambda: P.apply_on(d_r.p.value, d_z.p.value)  # noqa: E731
                reps = max(R, int(np.ceil(window_ms * 1e3 / us_per_call(call, R))))   # a window of window_ms at least
                t_apply = med3(lambda: us_per_call(call, reps))
                applies[label] = t_apply[1]
                res = solve(iters=3000, tol=1e-8, precond=P)
                t_tol = med3(lambda: ms(solve(iters=3000, tol=1e-8, precond=P)))
                want = f"{expect[kw['degree']]:.1f}" if kw["kind"] == "chebyshev" else "-"
                emit(f"| {label} | {t_apply[1]:.1f} ({t_apply[0]:.1f} .. {t_apply[2]:.1f}) | {want} | "
                            f"{t_apply[1] / t_spmv:.2f} | {info(res)['steps']} | {info(res)['status']} | "
                            f"{t_tol[1]:.2f} ({t_tol[0]:.2f} .. {t_tol[2]:.2f}) | {wall:.0f} |")
                if kw["kind"] == "chebyshev" and kw["degree"] == 4 and method == "pcg":
                    B = np.random.default_rng(8).uniform(-1, 1, (M, 8))
                    multi = dev.pcg_multi(B, 3000, tol=1e-8, precond=P)
                    t_multi = med3(lambda: dev.pcg_multi(B, 3000, tol=1e-8, precond=P)[4])
                    singles = [dev.pcg(np.ascontiguousarray(B[:, j]), 3000, tol=1e-8, precond=P) for j in range(8)]
                    t_single = med3(lambda: sum(dev.pcg(np.ascontiguousarray(B[:, j]), 3000, tol=1e-8, precond=P)[4]
                                                for j in range(8)))
                    multi_line = (f"pcg_multi, k = 8, chebyshev 4, to 1e-8: {t_multi[1]:.2f} ms ({t_multi[0]:.2f} .. "
                                  f"{t_multi[2]:.2f}), steps {int(multi[3]['steps'].min())} .. {int(multi[3]['steps'].max())}; "
                                  f"8 pcg solves of the same columns: {t_single[1]:.2f} ms ({t_single[0]:.2f} .. "
                                  f"{t_single[2]:.2f}), steps {min(s[3]['steps'] for s in singles)} .. "
                                  f"{max(s[3]['steps'] for s in singles)}; ratio {t_single[1] / t_multi[1]:.2f}")
        d_r.close(), d_z.close()
        emit()
        emit("| Chebyshev build | lmin | lmax | Gershgorin bound | products per apply | plan of P's upload | download + canonical "
             "rows + bound ms | upload + vectors ms | build wall ms |")
        emit("|---|---|---|---|---|---|---|---|---|")
        for line in builds:
            emit(line)
        emit()
        t_pass = (applies["chebyshev 8"] - applies["chebyshev 2"]) / 6.0 - t_spmv
        emit(f"the fused pass by difference, (apply(8) - apply(2)) / 6 - SpMV: {t_pass:.1f} us, "
             f"{7 * 8 * M / max(t_pass, 1e-3) / 1e6:.2f} TB/s of its 7 values a row against the probe's {probe:.2f} TB/s")
        if method == "pcg":
            emit()
            emit(multi_line)
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=float, default=30.0, help="milliseconds one timed run of applies lasts at least")
    ap.add_argument("--others", default="jacobi,block,fsai,amg", help="the kinds measured beside the new one")
    ap.add_argument("--limit", type=int, default=420, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    others = [o for o in args.others.split(",") if o]
    if args.one:
        one(args.one, args.reps, args.window, others, args.out)
        return 0
    head = (f"fp64; applies: host time over windows of at least {args.window:g} ms of asynchronous calls; times to tol: "
            "device time of the solve; every figure the median of three repeats in one process")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--reps", str(args.reps), "--window",
               str(args.window), "--others", args.others] + (["--out", args.out] if args.out else [])
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
