#!/usr/bin/env python3
"""Reordering on the device (CsrDevice.permute, CsrDevice.rcm, CsrDevice.reordered) on the three matrices of
time_trsv.py (million, convdiff, fembig) and a 1000 x 1000 5-point grid, fp64, each shuffled by one seeded symmetric
random permutation.

Per matrix, in a child process of its own under its own time limit (after a child that failed or ran out of time nothing
more is started): the SpMV time (CsrDevice.time, median) and the plan of the handle in natural order, shuffled, and
shuffled then reordered("rcm"), all three in the same process; the split of rcm on the shuffled handle (graph,
peripheral, order; levels, chained levels, wide levels, launches) with chain_nodes auto, with chain_nodes = -1 for the
cost of the wide tier, and at the other caps; the split of permute (device build, adopt); sp.rcm_plan (the host definition, one thread)
and scipy.sparse.csgraph.reverse_cuthill_mckee (one thread, where scipy imports) on the shuffled arrays for the ordering
alone, with the bandwidth each reaches.  Wall times are host time around synchronised calls, the median of --reps after
one untimed call.

usage: time_rcm.py [--matrices million,convdiff,fembig,grid1000] [--reps 3] [--limit 900] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EXPECTATION = """\
Expectation, written before the first run: the shuffled handles lose their x-window plans and fall to the gather or
tile kernels at a fraction of the natural-order rate; RCM brings a banded numbering back (bandwidth of the order of the
grid side times the entries per node), the upload's plan search finds an x-window plan again, and the reordered SpMV
should come within a few tens of per cent of the natural-order one, not equal: RCM's bandwidth is about twice a
lexicographic grid numbering's.  The ordering itself is a breadth-first search: about 2000 levels on the grids, each a
launch or a barrier.  With chain_nodes auto (1024) the grids' levels (at most ~1000 to 1700 nodes wide) run mostly
chained in one workgroup, which uses one CU of 256; the wide tier pays about five launches and a 4-byte read per level,
some tens of microseconds, so 2000 wide levels are 0.1 s before any work.  scipy's serial loop does a million-row grid in
roughly 0.1 to 0.3 s.  So the device ordering is expected to be at best level with the host on these graphs, and to lose
wherever the levels are many and narrow; it can only win where levels are few and wide.  If it loses, the host plan
(sp.rcm_plan) stays the way to order and permute() the way to apply."""


def grid1000():
    g = 1000
    idx = np.arange(g * g, dtype=np.int64).reshape(g, g)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    r = np.concatenate([u, v, idx.ravel()])
    c = np.concatenate([v, u, idx.ravel()])
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    rp = np.searchsorted(r, np.arange(g * g + 1)).astype(np.int32)
    val = np.where(r == c, 4.0, -1.0)
    return g * g, rp, c.astype(np.int32), val


def permuted(M, rp, col, val, p):
    """A permuted symmetrically by p (the definition of CsrDevice.permute), rows sorted again"""
    inv = np.empty(M, np.int64)
    inv[p] = np.arange(M)
    lens = np.diff(rp)[p]
    rp_c = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(rp[:-1][p].astype(np.int64) - rp_c[:-1], lens) + np.arange(rp_c[-1])
    rows = np.repeat(np.arange(M, dtype=np.int64), lens)
    c = inv[col[src]]
    order = np.lexsort((c, rows))
    return rp_c.astype(np.int32), c[order].astype(np.int32), np.ascontiguousarray(val[src][order])


def bandwidth(M, rp, col):
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(rp))
    return int(np.abs(rows - col).max()) if len(col) else 0


def one(key, reps, out_path):
    import sparsematrixvectormultiplication_amd as sp
    from sparsematrixvectormultiplication_amd.device import CSR_STREAM_KERNELS
    from time_bicgstab import settle
    from time_trsv import MATRICES

    def emit(line=""):
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    def median_ms(call):
        call()
        runs = []
        for _ in range(reps):
            sp.hip_sync()
            t0 = time.perf_counter()
            res = call()
            runs.append(((time.perf_counter() - t0) * 1e3, res))
        runs.sort(key=lambda r: r[0])
        return runs[len(runs) // 2]

    def plan_of(dev):
        i = dev.info()
        kind = CSR_STREAM_KERNELS[i["stream_kernel"]] if 0 <= i["stream_kernel"] < len(CSR_STREAM_KERNELS) else str(i["stream_kernel"])
        return f"{kind}{' + patterns' if i['pattern_slots'] else ''} ({i['local_blocks']} x-window blocks, {i['tile_blocks']} tile blocks)"

    def spmv_us(dev):
        return float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3

    sp.hip_init(0)
    title, make = ("5-point grid 1000 x 1000", grid1000) if key == "grid1000" else MATRICES[key][:2]
    M, rp, col, val = make()
    nz = int(rp[-1])
    emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {nz / 1e6:.1f} M entries")
    emit()
    p = np.random.default_rng(2024).permutation(M)
    srp, scol, sval = permuted(M, rp, col, val, p)

    with sp.CsrDevice(M, M, rp, col, val) as natural, sp.CsrDevice(M, M, srp, scol, sval) as shuffled:
        settle(natural)
        t_rcm, (perm, info) = median_ms(lambda: shuffled.rcm())
        t_wide, (perm_w, info_w) = median_ms(lambda: shuffled.rcm(chain_nodes=-1))
        assert perm.tobytes() == perm_w.tobytes()
        lo, hi, auto = sp.rcm_chain_nodes()
        caps = []
        for cap in sorted({lo, 256, 1024, hi} - {auto}):
            t_cap, (perm_c, info_c) = median_ms(lambda: shuffled.rcm(chain_nodes=cap))
            assert perm.tobytes() == perm_c.tobytes()
            caps.append((f"chain_nodes {cap}", t_cap, info_c))

        def permute_once():
            out = shuffled.permute(perm, perm)
            ms = out.permute_info["ms"]
            out.close()
            return ms

        t_perm, ms_perm = median_ms(permute_once)
        with shuffled.permute(perm, perm) as re:
            emit("| handle | plan | bandwidth | SpMV us | / natural |")
            emit("|---|---|---|---|---|")
            t_nat = spmv_us(natural)
            for label, dev, bw in (("natural", natural, bandwidth(M, rp, col)), ("shuffled", shuffled, info["bandwidth_before"]),
                                   ("shuffled, then reordered(\"rcm\")", re, info["bandwidth_after"])):
                t = spmv_us(dev)
                emit(f"| {label} | {plan_of(dev)} | {bw} | {t:.1f} | {t / t_nat:.2f} |")
        emit()
        emit("| rcm of the shuffled handle | wall ms | graph | peripheral | order | components | levels | chained | wide | launches | "
             "searches |")
        emit("|---|---|---|---|---|---|---|---|---|---|---|")
        for label, t, i in [(f"chain_nodes auto ({auto})", t_rcm, info), ("chain_nodes -1 (wide tier alone)", t_wide, info_w)] + caps:
            ms = i["ms"]
            emit(f"| {label} | {t:.1f} | {ms['graph']:.1f} | {ms['peripheral']:.1f} | {ms['order']:.1f} | {i['components']} | "
                 f"{i['levels']} | {i['chained_levels']} | {i['wide_levels']} | {i['launches']} | {i['peripheral_searches']} |")
        emit()
        emit(f"permute(perm, perm): {t_perm:.1f} ms wall; device build {ms_perm['device_build']:.2f} ms, adopt (the upload of "
             f"the result) {ms_perm['adopt']:.1f} ms")
        t0 = time.perf_counter()
        host_perm, host_info = sp.rcm_plan(srp, scol, M)
        t_host = (time.perf_counter() - t0) * 1e3
        same = host_perm.tobytes() == perm.tobytes()
        emit(f"sp.rcm_plan on one host thread: {t_host:.1f} ms, bandwidth {host_info['bandwidth_after']}; the device's perm "
             f"is {'the same bytes' if same else 'DIFFERENT'}; device / host = {t_rcm / t_host:.2f}")
        try:
            import scipy.sparse as sps
            from scipy.sparse.csgraph import reverse_cuthill_mckee
            a = sps.csr_matrix((sval, scol, srp), shape=(M, M))
            t0 = time.perf_counter()
            sperm = reverse_cuthill_mckee(a, symmetric_mode=False)
            t_scipy = (time.perf_counter() - t0) * 1e3
            inv = np.empty(M, np.int64)
            inv[sperm] = np.arange(M)
            rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(srp))
            emit(f"scipy reverse_cuthill_mckee (symmetric_mode=False) on one host thread: {t_scipy:.1f} ms, bandwidth "
                 f"{int(np.abs(inv[rows] - inv[scol]).max())}; device / scipy = {t_rcm / t_scipy:.2f}")
        except ImportError:
            emit("scipy does not import here: no scipy column")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig,grid1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds one matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one, args.reps, args.out)
        return 0
    head = (f"fp64; wall times on the host around synchronised calls, the median of {args.reps} after one untimed call; SpMV: "
            "CsrDevice.time, the median of 100 launches")
    print(EXPECTATION + "\n\n" + head, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(EXPECTATION + "\n\n" + head + "\n\n")
    for key in args.matrices.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--reps", str(args.reps)]
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
