#!/usr/bin/env python3
"""SpMM (Y = A X, k vectors per pass over the matrix) against k separate SpMVs of the same handle, in one process.

For every matrix and every k, alternating rounds time one spmv_hip_csr_spmm call (library-owned X / Y) and k times
the handle's SpMV under CSR_AUTO.  Prints per row: us per call, us per vector, effective GFLOP/s = 2 nnz k / t,
algorithmic bytes = nnz (sizeof(T) + 4) + 4 (M + 1) + k sizeof(T) (N + M) and those bytes / t as a fraction of
8 TB/s, and SpMM time / (k x SpMV time).

--format hll does the same for an HLL slab built on the device from the matrix (spmv_hip_hll_from_csr): one
spmv_hip_hll_spmm call against k times the handle's SpMV under HLL_AUTO.  HLL is fp64 only, so the default matrices
are then the fp64 ones; its algorithmic bytes are priced by padded slots, slots x 12 + 8 (hacks + 1) + 4 hacks +
8 k (N + M), and GFLOP/s still counts 2 nnz k.

usage: time_spmm.py [--format csr|hll] [--matrices nlpkkt,fembig,uniform,powerlaw] [--ks 1,2,4,8,16,32] [--rounds 5]
                    [--out FILE]"""
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


def uniform_random(n, per_row, seed=2026):
    """n x n, `per_row` uniformly random columns per row (sorted; repeats kept as separate entries)."""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, n, (n, per_row), dtype=np.int64)
    col.sort(axis=1)
    row_ptr = (np.arange(n + 1, dtype=np.int64) * per_row).astype(np.int32)
    return n, row_ptr, col.ravel().astype(np.int32), rng.uniform(-1, 1, n * per_row)


MATRICES = {
    # BASELINE config 4's shape at full size (3.5 M rows, ~98 M nnz), fp64
    "nlpkkt": ("nlpkkt-like, fp64", lambda: synth.kkt_like()),
    # the FEM-shaped > 1 GB matrix of tools/tune_csr.py fembig (1.23 M rows, ~92 M nnz), fp64
    "fembig": ("FEM-shaped (40, 40, 257), fp64", lambda: synth.fem_like((40, 40, 257), 1)),
    # uniformly random columns (uniform:2000000:16 of tools/time_tile.py), fp64
    "uniform": ("uniform 2 M x 16, fp64", lambda: uniform_random(2_000_000, 16)),
    # BASELINE config 5's power-law family at 1/16 of its size, fp32
    "powerlaw": ("power-law 2^20 rows, fp32", lambda: synth.powerlaw(1 << 20, 1 << 16, 5)),
}


FP64 = ("nlpkkt", "fembig", "uniform")


def settle(dev, variant, ms=40.0):
    """Untimed launches for `ms` milliseconds, as bench.py's settle(): the card's transient after an idle stretch."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        dev.time(variant, 0, 20, zero_y=False)


def measure(dev, variant, ks, rounds, iters):
    spmm = {k: [] for k in ks}
    spmv = []
    for _ in range(rounds):
        spmv.extend(dev.time(variant, 3, iters, zero_y=False).tolist())
        for k in ks:
            spmm[k].extend(dev.time_spmm(k, 3, iters).tolist())
            spmv.extend(dev.time(variant, 3, iters, zero_y=False).tolist())
    return {k: float(np.median(v)) for k, v in spmm.items()}, float(np.median(spmv))


def handle(fmt, M, N, row_ptr, col, val):
    """The handle under test, its SpMV variant and its algorithmic bytes as a function of k."""
    nnz = int(row_ptr[-1])
    vb = val.dtype.itemsize
    if fmt == "csr":
        return (sp.CsrDevice(M, N, row_ptr, col, val), sp.CSR_AUTO,
                lambda k: nnz * (vb + 4) + 4 * (M + 1) + k * vb * (N + M))
    with sp.CsrDevice(M, N, row_ptr, col, val) as cdev:
        dev = sp.HllDevice.from_csr_device(cdev)
    info = dev.info()
    slots, hacks = info["slots"], info["hacks"]
    return dev, sp.HLL_AUTO, lambda k: slots * 12 + 8 * (hacks + 1) + 4 * hacks + 8 * k * (N + M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=("csr", "hll"), default="csr")
    ap.add_argument("--matrices", default=None)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",")]
    keys = (args.matrices or ",".join(FP64 if args.format == "hll" else MATRICES)).split(",")
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    lines = [f"device: {name} ({cus} CUs); medians of {args.rounds} alternating rounds x {args.iters} launches",
             "", "| matrix | k | us / call | us / vector | GFLOP/s | algo GB | frac of 8 TB/s | vs k SpMVs |",
             "|---|---|---|---|---|---|---|---|"]
    if args.format == "hll":
        lines[0] += "; HLL slabs built on the device, SpMV under HLL_AUTO"
    print("\n".join(lines), flush=True)
    for key in keys:
        label, make = MATRICES[key]
        M, row_ptr, col, val = make()
        N = M
        nnz = int(row_ptr[-1])
        if args.format == "hll" and val.dtype != np.float64:
            raise SystemExit(f"{key}: HLL handles are fp64 only")
        dev, variant, algo_bytes = handle(args.format, M, N, row_ptr, col, val)
        with dev:
            settle(dev, variant)
            t_spmm, t_spmv = measure(dev, variant, ks, args.rounds, args.iters)
        for k in ks:
            t = t_spmm[k] * 1e-3
            algo = algo_bytes(k)
            row = (f"| {label} (nnz {nnz / 1e6:.1f} M) | {k} | {t * 1e6:.1f} | {t * 1e6 / k:.1f} | "
                   f"{2 * nnz * k / t / 1e9:.0f} | {algo / 1e9:.3f} | {algo / t / HBM_PEAK:.2f} | "
                   f"{t_spmm[k] / (k * t_spmv):.3f} (SpMV {t_spmv * 1e3:.1f} us) |")
            lines.append(row)
            print(row, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
