#!/usr/bin/env python3
"""Preconditioned solvers (spmv_hip_csr_pcg, spmv_hip_csr_pbicgstab) against their unpreconditioned twins, in one
process, on the FEM-shaped fembig stand-in ((40, 40, 257), 1.23 M rows, 78 M entries) with each row's absolute sum + 1
added to its diagonal, fp64.

After the card is settled as bench.py does, alternating rounds time one run of S steps with tol = 0 (no host
synchronisation, every step runs) of: csr_cg, PCG with P = NULL, Jacobi and block-3, BiCGSTAB and right-preconditioned
BiCGSTAB with Jacobi and block-3 (device times as the library reports them), and the build of each preconditioner
(host wall time around the call, which synchronises).  Then the time to tol = 1e-8 of plain CG against Jacobi PCG on a
badly scaled copy S A S (S = 2^u, u uniform in [-8, 8]).  Prints markdown tables.

usage: time_pcg.py [--steps 50] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from time_bicgstab import fembig, settle  # noqa: E402


def build_ms(dev, kind, block, rounds):
    out = []
    for _ in range(rounds):
        t = time.perf_counter()
        P = dev.preconditioner(kind, block)
        out.append((time.perf_counter() - t) * 1e3)
        P.close()
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    S, R = args.steps, args.rounds
    M, row_ptr, col, val = fembig()
    b = np.random.default_rng(7).uniform(-1, 1, M)
    lines = [f"device: {name} ({cus} CUs); fembig fp64, M {M / 1e6:.2f} M, nnz {int(row_ptr[-1]) / 1e6:.1f} M; "
             f"S = {S} steps per run, tol = 0; medians of {R} alternating rounds", ""]
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        settle(dev)
        J = dev.preconditioner("jacobi")
        B3 = dev.preconditioner("block_jacobi", 3)
        runs = {
            "csr_cg": lambda: dev.cg(b, S)[2],
            "pcg, P = NULL": lambda: dev.pcg(b, S)[4],
            "pcg, Jacobi": lambda: dev.pcg(b, S, precond=J)[4],
            "pcg, block-3": lambda: dev.pcg(b, S, precond=B3)[4],
            "bicgstab": lambda: dev.bicgstab(b, S)[3],
            "pbicgstab, Jacobi": lambda: dev.bicgstab(b, S, precond=J)[3],
            "pbicgstab, block-3": lambda: dev.bicgstab(b, S, precond=B3)[3],
        }
        for f in runs.values():                                      # warm-up of every loop's kernels
            f()
        times = {k: [] for k in runs}
        spmv = []
        for _ in range(R):
            for k, f in runs.items():
                times[k].append(f() * 1e3 / S)
            spmv.append(float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
        t = {k: float(np.median(v)) for k, v in times.items()}
        t_s = float(np.median(spmv))
        lines += ["| loop | us / step | / csr_cg step | / unpreconditioned twin |", "|---|---|---|---|"]
        for k, v in t.items():
            twin = t["bicgstab"] if "bicgstab" in k else t["csr_cg"]
            lines.append(f"| {k} | {v:.1f} | {v / t['csr_cg']:.3f} | {v / twin:.3f} |")
        lines += ["", f"SpMV (AUTO): {t_s:.1f} us; csr_cg step - SpMV = {t['csr_cg'] - t_s:.1f} us, Jacobi PCG step - "
                  f"SpMV = {t['pcg, Jacobi'] - t_s:.1f} us (88 and 104 B per row by the byte count: "
                  f"{88 * M / ((t['csr_cg'] - t_s) * 1e-6) / 1e12:.2f} and "
                  f"{104 * M / ((t['pcg, Jacobi'] - t_s) * 1e-6) / 1e12:.2f} TB/s with the small kernels charged)", ""]
        lines += ["| build | ms (host wall, median) |", "|---|---|",
                  f"| Jacobi | {build_ms(dev, 'jacobi', 1, R):.2f} |",
                  f"| block-3 | {build_ms(dev, 'block_jacobi', 3, R):.2f} |",
                  f"| block-32 | {build_ms(dev, 'block_jacobi', 32, R):.2f} |", ""]
        J.close()
        B3.close()
    print("\n".join(lines), flush=True)
    # time to tolerance on S A S
    rng = np.random.default_rng(11)
    s = np.ldexp(1.0, rng.integers(-8, 9, M))
    sval = val * s[np.repeat(np.arange(M), np.diff(row_ptr))] * s[col]
    tol, iters = 1e-8, 20000
    tail = ["| S A S, tol 1e-8 | steps | status | ms |", "|---|---|---|---|"]
    with sp.CsrDevice(M, M, row_ptr, col, sval) as dev:
        settle(dev)
        with dev.preconditioner("jacobi") as J:
            for label, P in (("CG (pcg, P = NULL)", None), ("Jacobi PCG", J)):
                _, _, _, info, ms = dev.pcg(b * s, iters, tol=tol, precond=P)
                tail.append(f"| {label} | {info['steps']} | {info['status']} | {ms:.1f} |")
    print("\n".join(tail), flush=True)
    lines += tail
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
