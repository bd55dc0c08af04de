#!/usr/bin/env python3
"""The sparse sum CsrDevice.add on the three matrices of time_trsv.py (million, convdiff, fembig), fp64: A + A^T (through
the merge alone and, for comparison, with method="canonical" on the same canonical input), A + sigma I, and canonical() of
a copy whose rows are shuffled (every row a random permutation of itself; beyond 2^25 entries the rows are reversed
instead, which the output says).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed or
ran out of time nothing more is started.  The card is settled with untimed SpMV launches first.  Per case: one untimed
sum, then --reps timed ones; the wall time of the median one with the library's split (check, canonical, symbolic,
numeric, adopt).  Next to the merge's symbolic + numeric time stand the bytes it must move (col and val of A and of B
read twice, col and val of C written once) priced at the rate spmv_hip_stream_probe measures in the same process, and
scipy on one host thread (where scipy imports): A + B for the sums, sum_duplicates() (which sorts the indices) of the
shuffled copy for canonical().  Its pattern must be C's; the largest value difference over the row's largest is printed.

usage: time_spadd.py [--matrices million,convdiff,fembig] [--reps 3] [--limit 600] [--sigma 0.5] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHUFFLE_MAX = 1 << 25


def shuffled_rows(rp, col, val):
    """every row permuted (a random permutation, or its reversal for a large matrix); returns (col, val, how)"""
    nz = int(rp[-1])
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    if nz <= SHUFFLE_MAX:
        order = np.argsort(rows + np.random.default_rng(4).random(nz), kind="stable")
        how = "rows randomly permuted"
    else:
        order = rp[rows].astype(np.int64) + rp[rows + 1] - 1 - np.arange(nz, dtype=np.int64)
        how = "rows reversed"
    return col[order], val[order], how


def one(key, reps, sigma, out_path):
    try:
        import scipy.sparse as sps
    except ImportError:
        sps = None

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

    title, make, _ = MATRICES[key]
    M, rp, col, val = make()
    nz = int(rp[-1])
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {nz / 1e6:.1f} M entries")
    emit()
    da = sp.CsrDevice(M, M, rp, col, val)
    settle(da)
    nbytes = 1 << 30
    probe_mean, probe_min = sp.stream_probe(nbytes, 3, 10)
    rate = nbytes / (probe_mean * 1e-3)                          # bytes / s
    emit(f"device: {name.strip()} ({cus} CUs); stream probe over 1 GiB: {probe_mean:.3f} ms mean ({probe_min:.3f} min), "
         f"{rate / 1e9:.0f} GB/s")
    emit()
    emit("| case | method | nnz(A) | nnz(B) | nnz(C) | matches | long rows | wall ms (min .. max) | check | canonical | symbolic | "
         "numeric | adopt | merge bytes | at the probe's rate ms | symbolic + numeric / that | scipy ms | scipy / wall | "
         "same pattern | largest value difference / row max |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")

    def case(label, method, call, nza, nzb, ref_call):
        call().close()                                           # untimed: first launches
        runs, keep = [], None
        for k in range(reps):
            sp.hip_sync()
            t0 = time.perf_counter()
            dc = call()
            runs.append(((time.perf_counter() - t0) * 1e3, dc.add_info))
            if k == reps - 1:
                keep = dc
            else:
                dc.close()
        runs.sort(key=lambda r: r[0])
        wall, info = runs[len(runs) // 2]
        ms = info["ms"]
        moved = 2 * (nza + nzb) * 12 + info["nz"] * 12
        at_rate = moved / rate * 1e3
        t_scipy, same, diff = "", "", ""
        if sps is not None and ref_call is not None:
            t0 = time.perf_counter()
            ref = ref_call()
            t_ref = (time.perf_counter() - t0) * 1e3
            ref.sort_indices()
            crp, ccol, cval = keep.download()
            same = bool(np.array_equal(crp, ref.indptr) and np.array_equal(ccol, ref.indices))
            if same and len(cval):
                live = np.flatnonzero(np.diff(crp))
                row_max = np.repeat(np.maximum.reduceat(np.abs(ref.data), crp[live]), np.diff(crp)[live])
                diff = f"{float(np.max(np.abs(cval - ref.data) / np.maximum(row_max, 1e-300))):.1e}"
            t_scipy = f"{t_ref:.0f}"
            ratio = f"{t_ref / wall:.1f}"
        else:
            ratio = ""
        keep.close()
        emit(f"| {label} | {method} | {nza} | {nzb} | {info['nz']} | {info['matches']} | {info['long_rows']} | {wall:.1f} "
             f"({runs[0][0]:.1f} .. {runs[-1][0]:.1f}) | {ms['check']:.2f} | {ms['canonical']:.2f} | {ms['symbolic']:.2f} | "
             f"{ms['numeric']:.2f} | {ms['adopt']:.1f} | {moved} | {at_rate:.2f} | "
             f"{(ms['symbolic'] + ms['numeric']) / at_rate:.1f} | {t_scipy} | {ratio} | {same} | {diff} |")

    if sps is not None:
        sa = sps.csr_matrix((val, col, rp), shape=(M, M))
        sat = sa.T.tocsr()
        eye = sps.identity(M, format="csr")
    with da.transpose() as dt:
        case("A + A^T", "auto (merge)", lambda: da.add(dt), nz, nz, (lambda: sa + sat) if sps else None)
        case("A + A^T", "canonical", lambda: da.add(dt, method="canonical"), nz, nz, None)
    with sp.identity(M) as de:
        case(f"A + {sigma} I", "auto (merge)", lambda: da.add(de, beta=sigma), nz, M, (lambda: sa + sigma * eye) if sps else None)
    scol, sval, how = shuffled_rows(rp, col, val)
    with sp.CsrDevice(M, M, rp, scol, sval) as ds:
        # (a permutation of rows without repeats: canon() is A again).  scipy's side is what canonical() does, on its own
        # copy of the shuffled arrays made before the clock starts: sum_duplicates(), which sorts the indices first
        ss = sps.csr_matrix((sval, scol, rp), shape=(M, M), copy=True) if sps else None

        def scipy_canonical():
            ss.sum_duplicates()
            return ss

        case(f"canonical(), {how}", "auto (product, then merge)", lambda: ds.canonical(), nz, 0, scipy_canonical if sps else None)
    da.close()
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds one matrix may take")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one, args.reps, args.sigma, args.out)
        return 0
    head = (f"fp64; wall time of CsrDevice.add on the host, synchronised, the median of {args.reps} after one untimed sum; the "
            "split is the library's own (host clock around each phase); scipy on one host thread")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--reps", str(args.reps), "--sigma", str(args.sigma)]
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
