#!/usr/bin/env python3
"""Value updates against what they replace, in one process, fp64: CsrDevice.update_values against a fresh upload, and
Preconditioner.refresh against a fresh build, on the three matrices of profiles/trsv_step.md (million, convdiff, fembig:
x-window handles) and a power-law stand-in that gets a tile plan.

Per matrix, after the card is settled as bench.py does, medians of three:
  upload          wall time of CsrDevice(...)
  update          from a host array (wall time, it synchronises) and from a device array (update_info()["last_us"],
                  events around the copy and the gathers); the first update's analysis (map_build_us) and the maps' bytes;
                  next to them nz x 8 bytes at the read-only stream probe's rate
  SpMV            CsrDevice.time (median of 100) three times before the first update and three times after the last
  refresh         ILU(0) and SSOR(1.0), natural and multicolour (--precond): wall time of the build, its tri_info() split, the first
                  refresh (with its analysis) and later refreshes
Prints markdown, matrix by matrix.

usage: time_update.py [--matrices million,convdiff,fembig,powerlaw] [--precond 1] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402
from time_bicgstab import convdiff, fembig, settle  # noqa: E402
from time_trsv import Vec, million  # noqa: E402


def powerlaw():
    n, rp, col, val = synth.powerlaw(1 << 22, 1 << 16)
    return n, rp, col, val.astype(np.float64)


MATRICES = {"million": ("kron(5-point 577 x 577, I_3) + kron(I, C)", million, True),
            "convdiff": ("convection-diffusion 1500 x 1500", convdiff, True),
            "fembig": ("FEM-shaped (40, 40, 257)", fembig, True),
            "powerlaw": ("power-law stand-in, 2^22 rows", powerlaw, False)}


def wall_ms(call):
    sp.hip_sync()
    t = time.perf_counter()
    out = call()
    sp.hip_sync()
    return (time.perf_counter() - t) * 1e3, out


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig,powerlaw")
    ap.add_argument("--precond", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    out = open(args.out, "w") if args.out else None

    def emit(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    probe_ms = sp.stream_probe(1 << 30)[0]
    rate = (1 << 30) / (probe_ms * 1e-3)
    emit(f"device: {name.strip()} ({cus} CUs); fp64; medians of three; read-only stream probe {rate / 1e12:.2f} TB/s")
    for key in args.matrices.split(","):
        title, make, square = MATRICES[key]
        M, rp, col, val = make()
        nz = int(rp[-1])
        other = val * np.random.default_rng(3).uniform(0.9, 1.1, nz)    # (a dominant diagonal stays one)
        emit()
        emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {nz / 1e6:.1f} M entries")
        emit()
        uploads = []
        for _ in range(3):
            ms, dev = wall_ms(lambda: sp.CsrDevice(M, M, rp, col, val))
            uploads.append(ms)
            dev.close()
        with sp.CsrDevice(M, M, rp, col, val) as dev:
            info = dev.info()
            settle(dev)
            before = [med(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False)) * 1e3 for _ in range(3)]
            first_ms, _ = wall_ms(lambda: dev.update_values(other))
            ui = dev.update_info()
            host = [wall_ms(lambda v=v: dev.update_values(v))[0] for v in (val, other, val)]
            d_other, d_val = Vec(other), Vec(val)
            device = []
            for d in (d_other, d_val, d_other, d_val):                  # (the first: untimed)
                dev.update_values_on(d.p.value)
                device.append(dev.update_info()["last_us"])
            d_other.close(), d_val.close()
            settle(dev)
            after = [med(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False)) * 1e3 for _ in range(3)]
            plan = {1: "x-window", 3: "tile plan"}.get(info["stream_kernel"], "gather kernels")
            slots = ui["map_bytes"] // 4
            emit(f"plan: {plan}; upload {med(uploads):.0f} ms; nz x 8 bytes at the probe's rate {nz * 8 / rate * 1e6:.0f} us"
                 + (f"; {slots / 1e6:.1f} M mapped slots x 20 bytes at that rate {slots * 20 / rate * 1e6:.0f} us" if slots else ""))
            emit()
            emit("| update | us |")
            emit("|---|---|")
            emit(f"| first (with its analysis), from the host | {first_ms * 1e3:.0f} |")
            emit(f"| the first update's analysis (map_build_us), maps of {ui['map_bytes'] / 1e6:.1f} MB | {ui['map_build_us']:.0f} |")
            emit(f"| later, from the host (wall, synchronises) | {med(host) * 1e3:.0f} |")
            emit(f"| later, from the device (events) | {med(device[1:]):.0f} |")
            emit()
            emit(f"SpMV (AUTO) before the updates: {', '.join(f'{t:.1f}' for t in before)} us; after: "
                 f"{', '.join(f'{t:.1f}' for t in after)} us")
            if not (args.precond and square):
                continue
            emit()
            emit("| preconditioner | build ms | analysis / factorisation / upload ms | first refresh ms | later refresh ms |")
            emit("|---|---|---|---|---|")
            for kind, ordering in (("ilu0", "natural"), ("ilu0", "multicolor"), ("ssor", "natural"), ("ssor", "multicolor")):
                build_ms, P = wall_ms(lambda: dev.preconditioner(kind, ordering=ordering))
                ti = P.tri_info()
                dev.update_values(other)
                first, _ = wall_ms(lambda: P.refresh(dev))
                later = []
                for v in (val, other, val):
                    dev.update_values(v)
                    later.append(wall_ms(lambda: P.refresh(dev))[0])
                P.close()
                emit(f"| {kind} {ordering} | {build_ms:.0f} | {ti['analysis_us'] / 1e3:.0f} / {ti['factor_us'] / 1e3:.0f} / "
                     f"{ti['upload_us'] / 1e3:.0f} | {first:.0f} | {med(later):.1f} |")


if __name__ == "__main__":
    main()
