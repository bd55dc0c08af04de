#!/usr/bin/env python3
"""GMRES(m) (spmv_hip_csr_gmres) steps against what they should cost, and the time to a tolerance against BiCGSTAB, in
one process, fp64.

Three matrices, those of profiles/trsv_step.md: the million-row kron(5-point, I_3) + kron(I, C) matrix, the 1500 x 1500
convection-diffusion stencil and the FEM-shaped fembig stand-in.

Step table.  Step j of a cycle is one SpMV, plus the CGS2 passes, which read the j + 1 basis vectors four times (twice
for the dots, twice for the updates) and w a few times more.  The expectation is

    SpMV + 4 (j + 1) n 8 bytes / (the stream probe's rate)

The cost of step j is measured as the difference of two one-cycle runs at restart 30, iters = j + 1 and iters = j
(tol = 0; the device time of a run includes the cycle's one read and its close, which the difference removes up to the
close's one more basis vector).  Medians of --rounds alternating rounds after the card is settled as bench.py does.

Solve table.  The convection-diffusion stencil to tol = 1e-8: gmres at restart 30 against bicgstab, without a
preconditioner, with block-Jacobi (3) and with AMG; steps, status, device ms, the true relative residual.

usage: time_gmres.py [--matrices million,convdiff,fembig] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from time_bicgstab import convdiff, fembig, settle  # noqa: E402
from time_trsv import million  # noqa: E402

MATRICES = {
    "million": ("kron(5-point 577 x 577, I_3) + kron(I, C), fp64", million),
    "convdiff": ("convection-diffusion 1500 x 1500, fp64", convdiff),
    "fembig": ("FEM-shaped (40, 40, 257), fp64", fembig),
}
STATUS = {sp.GMRES_RAN_ALL: "ran all", sp.GMRES_CONVERGED: "converged", sp.GMRES_BREAKDOWN: "breakdown"}
RESTART = 30
COLUMNS = (0, 14, 29)


def stream_rate():
    """bytes / s of the read-only stream probe over 1 GiB (its fastest pass)"""
    _, fastest = sp.stream_probe(1 << 30)
    return (1 << 30) / (fastest * 1e-3)


def step_table(args, lines, rate):
    lines += ["", "| matrix | SpMV us | " + " | ".join(f"step j = {j} us | expected us | ratio" for j in COLUMNS) +
              " | us / step over a cycle of 30 |", "|---|---|" + "---|---|---|" * len(COLUMNS) + "---|"]
    print("\n".join(lines[-2:]), flush=True)
    for key in args.matrices.split(","):
        label, make = MATRICES[key]
        M, row_ptr, col, val = make()
        val = np.ascontiguousarray(val, dtype=np.float64)
        b = np.random.default_rng(7).uniform(-1, 1, M)
        with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
            settle(dev)
            lengths = sorted({j + d for j in COLUMNS for d in (0, 1)} | {RESTART})
            for k in lengths:
                if k:
                    dev.gmres(b, k, restart=RESTART)                     # warm-up of every length's launches
            ms = {k: [] for k in lengths}
            spmv = []
            for _ in range(args.rounds):
                for k in lengths:
                    ms[k].append(dev.gmres(b, k, restart=RESTART)[3])
                spmv.append(float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
        med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}      # us
        t_s = float(np.median(spmv))
        cells = []
        for j in COLUMNS:
            got = med[j + 1] - med[j]
            want = t_s + 4 * (j + 1) * M * 8 / rate * 1e6
            cells.append(f"{got:.1f} | {want:.1f} | {got / want:.2f}")
        row = (f"| {label} (M {M / 1e6:.2f} M, nnz {int(row_ptr[-1]) / 1e6:.1f} M) | {t_s:.1f} | " + " | ".join(cells) +
               f" | {med[RESTART] / RESTART:.1f} |")
        lines.append(row)
        print(row, flush=True)


def solve_table(args, lines):
    tol, budget = 1e-8, 4000
    import scipy.sparse as sps
    M, row_ptr, col, val = convdiff()
    a = sps.csr_matrix((val, col, row_ptr), shape=(M, M))
    b = np.random.default_rng(7).uniform(-1, 1, M)
    lines += ["", f"convection-diffusion 1500 x 1500 to tol = {tol:g} (budget {budget} steps; gmres at restart {RESTART}; "
              f"medians of {args.rounds} runs)", "",
              "| preconditioner | solver | steps | status | ms | us / step | true ||b - A x|| / ||b|| |",
              "|---|---|---|---|---|---|---|"]
    print("\n".join(lines[-4:]), flush=True)
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev, dev.preconditioner("block_jacobi", 3) as B3, \
            dev.preconditioner("amg") as A:
        settle(dev)
        for pname, P in (("none", None), ("block-Jacobi (3)", B3), ("AMG", A)):
            for sname, run in (("gmres(30)", lambda: dev.gmres(b, budget, tol=tol, restart=RESTART, precond=P)),
                               ("bicgstab", lambda: dev.bicgstab(b, budget, tol=tol, precond=P))):
                run()
                out = [run() for _ in range(args.rounds)]
                x, info, ms = out[0][0], out[0][2], float(np.median([o[3] for o in out]))
                res = float(np.linalg.norm(b - a @ x) / np.linalg.norm(b))
                row = (f"| {pname} | {sname} | {info['steps']} | {STATUS[min(info['status'], 2)]} | {ms:.2f} | "
                       f"{ms * 1e3 / max(info['steps'], 1):.1f} | {res:.2e} |")
                lines.append(row)
                print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    rate = stream_rate()
    lines = [f"device: {name} ({cus} CUs); restart {RESTART}, tol = 0 for the step table; medians of {args.rounds} "
             f"alternating rounds; stream probe {rate / 1e12:.2f} TB/s"]
    print(lines[0], flush=True)
    step_table(args, lines, rate)
    solve_table(args, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
