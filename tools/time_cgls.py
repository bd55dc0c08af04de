#!/usr/bin/env python3
"""Transposed handles (spmv_hip_csr_transpose) and CGLS steps (spmv_hip_csr_cgls) against the products they run on.

Three matrices: the nlpkkt-like stand-in (3.54 M rows, 97.8 M entries, fp64), the FEM-shaped fembig stand-in of
tools/time_bicgstab.py (1.23 M rows, 96.4 M entries, fp64) and the config-5 power-law matrix (2^24 rows, 2.6e8 entries,
fp32).  For each, after the card is settled as bench.py does:

- the wall time of one transpose, end to end, and the split of a second one into the device build (pairs, sort,
  gather, row pointers) and the upload of the result (its plans and searches), as the library's SPMV_TRACE_UPLOAD
  trace reports them (that run synchronises the device between phases);
- the SpMV time of A and of A^T (AUTO, the median of 100 launches) with the kernel AUTO picked for each;
- a CGLS step (tol = 0, S steps per run, no host synchronisation; the median of alternating rounds) against
  t(A x) + t(A^T x).

usage: time_cgls.py [--matrices nlpkkt,fembig,powerlaw] [--steps 20] [--rounds 5] [--out FILE]"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402

MATRICES = {
    "nlpkkt": ("nlpkkt-like, fp64", lambda: synth.kkt_like()),
    "fembig": ("FEM-shaped (40, 40, 257), fp64", lambda: synth.fem_like((40, 40, 257), 1)),
    "powerlaw": ("power-law 2^24 (config 5), fp32", lambda: synth.powerlaw()),
}
TRACE = re.compile(r"\[upload trace\] (\S+)\s+(.*?)\s+([\d.]+) ms$")


def settle(dev, ms=40.0):
    """Untimed launches for `ms` milliseconds, as bench.py's settle(): the card's transient after an idle stretch."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        dev.time(sp.CSR_AUTO, 0, 20, zero_y=False)


def plan(dev):
    info = dev.info()
    if info["auto_variant"] != sp.CSR_STREAM:
        return {v: k for k, v in sp.CSR_VARIANTS.items()}[info["auto_variant"]]
    name = sp.device.CSR_STREAM_KERNELS[info["stream_kernel"]]
    return name + (" + pattern plan" if info["pattern_slots"] else "")


def timed_transpose(dev):
    t = time.perf_counter()
    dt = dev.transpose()
    sp.hip_sync()
    return dt, time.perf_counter() - t


def traced_transpose(dev):
    """(device build ms, upload ms) of one transpose, from the library's trace on stderr"""
    os.environ["SPMV_TRACE_UPLOAD"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            dt, _ = timed_transpose(dev)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["SPMV_TRACE_UPLOAD"]
        f.seek(0)
        text = f.read().decode(errors="replace")
    dt.close()
    build = upload = 0.0
    for line in text.splitlines():
        m = TRACE.search(line.strip())
        if m and m.group(1) == "csr_transpose":
            build += float(m.group(3))
        elif m and m.group(1) == "csr_upload":
            upload += float(m.group(3))
    return build, upload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="nlpkkt,fembig,powerlaw")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    S = args.steps
    with sp.CsrDevice(4, 3, np.array([0, 1, 2, 3, 3], np.int32), np.array([0, 1, 2], np.int32), np.ones(3)) as tiny:
        tiny.transpose().close()                                        # loads the sort's code objects
    lines = [f"device: {name} ({cus} CUs); CGLS: S = {S} steps per run, tol = 0; medians of {args.rounds} alternating "
             "rounds", "",
             "| matrix | transpose s | device build ms | upload ms | A x us (AUTO) | A^T x us (AUTO) | A^T / A "
             "| CGLS us / step | step / (A x + A^T x) |", "|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    plans = []
    for key in args.matrices.split(","):
        label, make = MATRICES[key]
        M, row_ptr, col, val = make()
        nz = int(row_ptr[-1])
        with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
            del col
            settle(dev)
            dt, wall = timed_transpose(dev)
            build, upload = traced_transpose(dev)
            b = np.random.default_rng(7).uniform(-1, 1, M).astype(dev.dtype)
            settle(dev)
            dev.cgls(b, 2, at=dt)                                       # warm-up of the loop's kernels
            steps, t_a, t_at = [], [], []
            for _ in range(args.rounds):
                _, _, _, info, ms = dev.cgls(b, S, at=dt)
                if info["status"] != sp.CGLS_RAN_ALL:
                    raise SystemExit(f"{label}: CGLS stopped early ({info}); the step time would not be a step's")
                steps.append(ms * 1e3 / S)
                t_a.append(float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
                t_at.append(float(np.median(dt.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3)
            plans.append(f"- {label}: A {plan(dev)}, A^T {plan(dt)}")
            dt.close()
        ts, ta, tat = float(np.median(steps)), float(np.median(t_a)), float(np.median(t_at))
        row = (f"| {label} (M {M / 1e6:.2f} M, nnz {nz / 1e6:.1f} M) | {wall:.3f} | {build:.1f} | {upload:.1f} | "
               f"{ta:.1f} | {tat:.1f} | {tat / ta:.3f} | {ts:.1f} | {ts / (ta + tat):.3f} |")
        lines.append(row)
        print(row, flush=True)
    lines += ["", "Plans AUTO picked:"] + plans
    print("\n".join(lines[-len(plans) - 2:]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
