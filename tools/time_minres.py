#!/usr/bin/env python3
"""MINRES (spmv_hip_csr_minres) steps against the same handle's SpMV, csr_cg step and BiCGSTAB step, in one process.

Three matrices: the nlpkkt-like KKT stand-in as generated (3.5 M rows, symmetric indefinite), the FEM-shaped fembig
stand-in of time_bicgstab.py (1.23 M rows, diagonally dominant, SPD) and the million-row kron(5-point, I_3) + kron(I, C)
matrix of time_trsv.py (SPD).  For each, after the card is settled as bench.py does, alternating rounds time one minres
run of S steps with tol = 0 (no host synchronisation, every step is launched), one csr_cg run and one bicgstab run of S
steps and 100 SpMV launches (device times as the library reports them).  A solver that stops before step S (a
breakdown: its later launches return at once) is marked with the step it stopped at; its time per step is then not a
step's cost.  Prints per matrix: us per MINRES step, that step / one SpMV, the csr_cg and BiCGSTAB steps, and what the
vector work adds to the product: step - SpMV (the three vector kernels, 15 n sizeof(T) bytes, plus the folds and
scalar kernels); bytes / that time is the vector kernels' achieved rate with the small kernels charged to them (a lower
bound).

Then, on fembig: steps and ms to tol = 1e-8 for MINRES against pcg, both plain and with Jacobi.

usage: time_minres.py [--matrices nlpkkt,fembig,million] [--steps 50] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402
from time_bicgstab import HBM_PEAK, fembig, settle  # noqa: E402
from time_trsv import million  # noqa: E402

MATRICES = {
    "nlpkkt": ("nlpkkt-like, indefinite, fp64", lambda: synth.kkt_like()),
    "fembig": ("FEM-shaped (40, 40, 257), SPD, fp64", fembig),
    "million": ("kron(5-point 577 x 577, I_3) + kron(I, C), SPD, fp64", million),
}
STATUS = {sp.MINRES_RAN_ALL: "ran all", sp.MINRES_CONVERGED: "converged", sp.MINRES_BREAKDOWN: "breakdown"}


def stopped(info, S):
    """'' for a run of all S steps, else a note naming the step the device stopped at"""
    steps = int(info["steps"])
    return "" if steps >= S else f" (stopped at step {steps})"


def step_table(args, lines):
    S = args.steps
    lines += ["", "| matrix | SpMV us | MINRES us / step | step / SpMV | csr_cg us / step | BiCGSTAB us / step "
              "| MINRES vector us | csr_cg vector us | MINRES vector TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines[-3:]), flush=True)
    for key in args.matrices.split(","):
        label, make = MATRICES[key]
        M, row_ptr, col, val = make()
        val = np.ascontiguousarray(val, dtype=np.float64)
        b = np.random.default_rng(7).uniform(-1, 1, M)
        with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
            settle(dev)
            info_m = dev.minres(b, S)[2]                                   # warm-up of the loops' kernels
            dev.cg(b, 2)
            info_b = dev.bicgstab(b, S)[2]
            mr, cg, bicg, spmv = [], [], [], []
            for _ in range(args.rounds):
                mr.append(dev.minres(b, S)[3] * 1e3 / S)
                cg.append(dev.cg(b, S)[2] * 1e3 / S)
                bicg.append(dev.bicgstab(b, S)[3] * 1e3 / S)
                spmv.append(float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
        t_m, t_c, t_b, t_s = (float(np.median(v)) for v in (mr, cg, bicg, spmv))
        vec_m, vec_c = t_m - t_s, t_c - t_s
        rate = 15 * M * 8 / (vec_m * 1e-6) / 1e12
        row = (f"| {label} (M {M / 1e6:.2f} M, nnz {int(row_ptr[-1]) / 1e6:.1f} M) | {t_s:.1f} | {t_m:.1f}"
               f"{stopped(info_m, S)} | {t_m / t_s:.3f} | {t_c:.1f} | {t_b:.1f}{stopped(info_b, S)} | {vec_m:.1f} | "
               f"{vec_c:.1f} | {rate:.2f} ({rate * 1e12 / HBM_PEAK:.2f} of 8) |")
        lines.append(row)
        print(row, flush=True)


def solve_table(args, lines):
    tol, budget = 1e-8, 2000
    M, row_ptr, col, val = fembig()
    b = np.random.default_rng(7).uniform(-1, 1, M)
    lines += ["", f"fembig to tol = {tol:g} (budget {budget} steps; medians of {args.rounds} runs)", "",
              "| solver | steps | status | ms | us / step |", "|---|---|---|---|---|"]
    print("\n".join(lines[-4:]), flush=True)
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev, dev.preconditioner("jacobi") as J:
        settle(dev)
        runs = {
            "minres": lambda: dev.minres(b, budget, tol=tol),
            "pcg (plain)": lambda: dev.pcg(b, budget, tol=tol),
            "minres, Jacobi": lambda: dev.minres(b, budget, tol=tol, precond=J),
            "pcg, Jacobi": lambda: dev.pcg(b, budget, tol=tol, precond=J),
        }
        for name, run in runs.items():
            run()
            out = [run() for _ in range(args.rounds)]
            info, ms = out[0][-2], float(np.median([o[-1] for o in out]))
            status = STATUS[info["status"]]                                 # the PCG_* values are the same three
            row = f"| {name} | {info['steps']} | {status} | {ms:.2f} | {ms * 1e3 / max(info['steps'], 1):.1f} |"
            lines.append(row)
            print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="nlpkkt,fembig,million")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    lines = [f"device: {name} ({cus} CUs); S = {args.steps} steps per run, tol = 0; medians of {args.rounds} "
             "alternating rounds"]
    print(lines[0], flush=True)
    step_table(args, lines)
    solve_table(args, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
