#!/usr/bin/env python3
"""The sparse product CsrDevice.matmul on the three matrices of time_trsv.py (million, convdiff, fembig), fp64: A A, then
A P and R (A P) with the P and R of level 0 of sp.amg_plan (the Galerkin product of the AMG setup).

Each matrix runs in a child process of its own under its own time limit (--limit seconds); after a child that failed or
ran out of time nothing more is started.  Per case and tier (auto: the on-chip tier with the global tier for the long
rows; block_products = -1: everything through the global tier): one untimed product, then --reps timed ones; the wall
time of the median one with its split (count, symbolic, numeric, adopt), the products, the blocks, long rows and chunks,
nnz(C) and the bytes C's three arrays hold.  Against that: the same product by scipy on the host (one thread, sorted
indices), whose pattern must be C's and whose values must agree to 1e-12 of the row's largest, and the host setup time
the AMG build of the handle reports (Preconditioner.amg_info), which holds three such products per level.

A case is skipped, and the table says so, when its arrays would not fit in memory: nnz(C) is at most min(products,
M N), and those entries at 12 bytes each plus one chunk of workspace must fit in --mem-share of the card's memory and
(for scipy) of the host's; --max-products bounds the time a case may take the same way.

usage: time_spgemm.py [--matrices million,convdiff,fembig] [--reps 3] [--limit 600] [--max-products 4e9]
       [--mem-share 0.5] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def one(key, reps, max_products, mem_share, out_path):
    import scipy.sparse as sps

    import sparsematrixvectormultiplication_amd as sp
    from time_bicgstab import settle
    from time_trsv import MATRICES

    sp.hip_init(0)
    name, cus, mem = sp.device_name()
    host_mem = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES")

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    title, make, _ = MATRICES[key]
    M, rp, col, val = make()
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries")
    emit()
    emit(f"device: {name.strip()} ({cus} CUs)")
    t0 = time.perf_counter()
    levels = sp.amg_plan(rp, col, val)
    t_plan = (time.perf_counter() - t0) * 1e3
    emit(f"sp.amg_plan on the host: {t_plan:.0f} ms of wall time, {len(levels)} levels, rows "
         f"{' '.join(str(lv['rows']) for lv in levels)}")
    A = (rp, col, val)
    mats = {"A": (M, M, A)}
    if "P" in levels[0]:
        nc = levels[0]["aggregates"]
        mats["P"], mats["R"] = (M, nc, levels[0]["P"]), (nc, M, levels[0]["R"])
    else:
        emit("the plan has a single level: no P and R, A A alone")
    del levels
    to_sps = lambda m: sps.csr_matrix((m[2][2], m[2][1], m[2][0]), shape=(m[0], m[1]))  # noqa: E731
    dev = {k: sp.CsrDevice(m[0], m[1], *m[2]) for k, m in mats.items()}
    settle(dev["A"])
    with dev["A"].preconditioner(kind="amg") as P:
        f = P.amg_info()
    emit(f"AMG build of the handle: host setup {f['setup_us'] / 1e3:.0f} ms (download {f['download_us'] / 1e3:.0f} ms, "
         f"uploads {f['upload_us'] / 1e3:.0f} ms), {f['levels']} levels")
    emit()
    emit("| case | tier | products | blocks | long rows | chunks | nnz(C) | C bytes | wall ms (min .. max) | count | symbolic | "
         "numeric | adopt | scipy ms | scipy / device | same pattern | largest value difference / row max |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")

    def products_of(a, b):
        lens = np.diff(b[2][0].astype(np.int64))
        return int(lens[a[2][1]].sum())

    def case(label, da, db, a, b):
        """rows of the table for da @ db; returns the product as (handle, host triple) or (None, None)"""
        products = products_of(a, b)
        bound = min(products, a[0] * b[1])
        need = bound * 12 + min(products, 1 << 23) * 32 + (a[0] + 1) * 4
        if products > max_products or need > mem_share * min(mem, host_mem):
            emit(f"| {label} | skipped: {products:.3e} products, up to {bound:.3e} entries of C = {need / 2**30:.1f} GiB with the "
                 f"workspace; the limits are {max_products:.1e} products and {mem_share * min(mem, host_mem) / 2**30:.0f} GiB |")
            return None, None
        t0 = time.perf_counter()
        ref = to_sps(a) @ to_sps(b)
        ref.sort_indices()
        t_scipy = (time.perf_counter() - t0) * 1e3
        keep = None
        for tier, bp in (("auto", 0), ("global only", -1)):
            da.matmul(db, block_products=bp).close()             # untimed: first launches, the sort's workspace
            runs = []
            for _ in range(reps):
                sp.hip_sync()
                t0 = time.perf_counter()
                dc = da.matmul(db, block_products=bp)
                runs.append(((time.perf_counter() - t0) * 1e3, dc.matmul_info))
                if keep is None and len(runs) == reps:
                    keep = dc
                else:
                    dc.close()
            runs.sort(key=lambda r: r[0])
            wall, info = runs[len(runs) // 2]
            same, diff = "", ""
            if tier == "auto":
                crp, ccol, cval = keep.download()
                same = bool(np.array_equal(crp, ref.indptr) and np.array_equal(ccol, ref.indices))
                if same and len(cval):
                    live = np.flatnonzero(np.diff(crp))
                    row_max = np.repeat(np.maximum.reduceat(np.abs(ref.data), crp[live]), np.diff(crp)[live])
                    diff = f"{float(np.max(np.abs(cval - ref.data) / np.maximum(row_max, 1e-300))):.1e}"
                host = (crp, ccol, cval)
            ms = info["ms"]
            emit(f"| {label} | {tier} | {info['products']} | {info['blocks']} | {info['long_rows']} | {info['chunks']} | "
                 f"{info['nz']} | {info['nz'] * 12 + (a[0] + 1) * 4} | {wall:.1f} ({runs[0][0]:.1f} .. {runs[-1][0]:.1f}) | "
                 f"{ms['count']:.1f} | {ms['symbolic']:.1f} | {ms['numeric']:.1f} | {ms['adopt']:.1f} | {t_scipy:.0f} | "
                 f"{t_scipy / wall:.1f} | {same} | {diff} |")
        return keep, host

    c, _ = case("A A", dev["A"], dev["A"], mats["A"], mats["A"])
    if c is not None:
        c.close()
    if "P" in mats:
        dap, ap = case("A P", dev["A"], dev["P"], mats["A"], mats["P"])
        if dap is not None:
            c, _ = case("R (A P)", dev["R"], dap, mats["R"], (M, mats["P"][1], ap))
            if c is not None:
                c.close()
            dap.close()
    emit()
    for d in dev.values():
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds one matrix may take")
    ap.add_argument("--max-products", type=float, default=4e9, help="products beyond which a case is skipped")
    ap.add_argument("--mem-share", type=float, default=0.5, help="share of the memory a case's arrays may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one, args.reps, args.max_products, args.mem_share, args.out)
        return 0
    head = (f"fp64; wall time of CsrDevice.matmul on the host, synchronised, the median of {args.reps} after one untimed "
            "product; the split is the library's own (host clock around each phase); scipy on one host thread")
    print(head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--reps", str(args.reps), "--max-products",
               str(args.max_products), "--mem-share", str(args.mem_share)]
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
