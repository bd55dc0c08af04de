#!/usr/bin/env python3
"""BiCGSTAB (spmv_hip_csr_bicgstab) steps against the same handle's SpMV and csr_cg step, in one process.

Two matrices: the FEM-shaped fembig stand-in (1.23 M rows, 78 M entries) with each row's absolute sum + 1 added to its
diagonal, and an unsymmetric 5-point convection-diffusion stencil on a 1500 x 1500 grid (2.25 M rows, 11.2 M entries).
For each, after the card is settled as bench.py does, alternating rounds time one bicgstab run of S steps with tol = 0
(no host synchronisation, every step runs), one csr_cg run of S steps and 100 SpMV launches (device times as the
library reports them).  Prints per matrix: us per BiCGSTAB step, that step / two SpMVs, the csr_cg step, and what the
vector work adds to the products: step - 2 SpMV for BiCGSTAB (the five vector kernels, 18 n sizeof(T) bytes, plus the
folds and scalar kernels) and step - SpMV for csr_cg (11 n sizeof(T)); bytes / that time is the vector kernels'
achieved rate with the small kernels charged to them (a lower bound).

usage: time_bicgstab.py [--matrices fembig,convdiff] [--steps 50] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402

HBM_PEAK = 8e12


def dominant_diagonal(row_ptr, col, val):
    M = len(row_ptr) - 1
    diag = np.flatnonzero(col == np.repeat(np.arange(M, dtype=np.int32), np.diff(row_ptr)))
    if len(diag) != M:
        raise SystemExit("a row without its diagonal entry")
    val[diag] += np.add.reduceat(np.abs(val), row_ptr[:-1]) + 1.0
    return val


def fembig():
    M, row_ptr, col, val = synth.fem_like((40, 40, 257), 1)
    return M, row_ptr, col, dominant_diagonal(row_ptr, col, val)


def convdiff(nx=1500, ny=1500, px=0.4, py=0.2, shift=0.05):
    """5-point convection-diffusion, central differences (cell Peclet numbers px, py), diagonal 4 + shift"""
    n = nx * ny
    i = np.arange(n, dtype=np.int64)
    gx, gy = i % nx, i // nx
    # row i's entries in column order: south, west, centre, east, north (where they exist)
    parts = [(gy > 0, -nx, -1.0 - py), (gx > 0, -1, -1.0 - px), (np.ones(n, bool), 0, 4.0 + shift),
             (gx < nx - 1, 1, -1.0 + px), (gy < ny - 1, nx, -1.0 + py)]
    counts = sum(c.astype(np.int32) for c, _, _ in parts)
    row_ptr = np.zeros(n + 1, np.int32)
    np.cumsum(counts, out=row_ptr[1:])
    col = np.empty(row_ptr[-1], np.int32)
    val = np.empty(row_ptr[-1])
    pos = row_ptr[:-1].astype(np.int64).copy()
    for cond, off, v in parts:
        rows = i[cond]
        col[pos[rows]] = rows + off
        val[pos[rows]] = v
        pos[rows] += 1
    return n, row_ptr, col, val


MATRICES = {
    "fembig": ("FEM-shaped (40, 40, 257), fp64", fembig),
    "convdiff": ("convection-diffusion 1500 x 1500, fp64", convdiff),
}


def settle(dev, ms=40.0):
    """Untimed launches for `ms` milliseconds, as bench.py's settle(): the card's transient after an idle stretch."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        dev.time(sp.CSR_AUTO, 0, 20, zero_y=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="fembig,convdiff")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    S = args.steps
    lines = [f"device: {name} ({cus} CUs); S = {S} steps per run, tol = 0; medians of {args.rounds} alternating rounds",
             "", "| matrix | SpMV us | BiCGSTAB us / step | step / 2 SpMV | csr_cg us / step | BiCGSTAB vector us "
             "| csr_cg vector us | ratio | BiCGSTAB vector TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    for key in args.matrices.split(","):
        label, make = MATRICES[key]
        M, row_ptr, col, val = make()
        b = np.random.default_rng(7).uniform(-1, 1, M)
        with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
            settle(dev)
            dev.bicgstab(b, 2)                                              # warm-up of both loops' kernels
            dev.cg(b, 2)
            bicg, cg, spmv = [], [], []
            for _ in range(args.rounds):
                bicg.append(dev.bicgstab(b, S)[3] * 1e3 / S)
                cg.append(dev.cg(b, S)[2] * 1e3 / S)
                spmv.append(float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
        t_b, t_c, t_s = float(np.median(bicg)), float(np.median(cg)), float(np.median(spmv))
        vec_b, vec_c = t_b - 2 * t_s, t_c - t_s
        rate = 18 * M * 8 / (vec_b * 1e-6) / 1e12
        row = (f"| {label} (M {M / 1e6:.2f} M, nnz {int(row_ptr[-1]) / 1e6:.1f} M) | {t_s:.1f} | {t_b:.1f} | "
               f"{t_b / (2 * t_s):.3f} | {t_c:.1f} | {vec_b:.1f} | {vec_c:.1f} | {vec_b / vec_c:.2f} | "
               f"{rate:.2f} ({rate * 1e12 / HBM_PEAK:.2f} of 8) |")
        lines.append(row)
        print(row, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
