#!/usr/bin/env python3
"""Sparse triangular solves and the SSOR / ILU(0) preconditioners against the handle's own SpMV, in one process, fp64:
the million-row kron(5-point, I_3) + kron(I, C) matrix of the tests, the 11 M-entry convection-diffusion stencil and
the FEM-shaped fembig stand-in of time_bicgstab.py, each in natural and in multicolour order.

Per matrix, after the card is settled as bench.py does: the handle's SpMV (CsrDevice.time, median); per ordering the
level structure and the build split of ILU(0) (Preconditioner.tri_info), one ILU(0) apply, and one forward and one
backward solve on their own (CsrDevice.triangular; for the multicolour order on a handle of Q A Q^T, permuted here with
the library's own colouring: the triangles of ILU(0)'s factors have its pattern, so the solves cost the same).
Solves and applies are timed on the host around R asynchronous calls on device vectors between two synchronisations,
so a launch-bound schedule is charged its launches.  Then a solver step (S steps, tol = 0) with
ILU(0) and SSOR(1) against the unpreconditioned step, and the time to tol 1e-8 against Jacobi and block-Jacobi (3):
PCG on the symmetric matrices, right-preconditioned BiCGSTAB on the stencil.  Prints markdown, matrix by matrix.

usage: time_trsv.py [--matrices million,convdiff,fembig] [--steps 20] [--reps 20] [--out FILE]"""
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
from time_bicgstab import convdiff, fembig, settle  # noqa: E402


def million():
    import scipy.sparse as sps
    g = 577
    q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((3, 3)))
    c = q @ np.diag([1.0, np.sqrt(1e3), 1e3]) @ q.T / 1e2
    t = sps.diags([-np.ones(g - 1), np.full(g, 2.005), -np.ones(g - 1)], [-1, 0, 1])
    lap = sps.kron(sps.eye(g), t) + sps.kron(t, sps.eye(g))
    a = (sps.kron(lap, sps.eye(3)) + sps.kron(sps.eye(g * g), sps.csr_matrix(c))).tocsr()
    a.sort_indices()
    return a.shape[0], a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


MATRICES = {"million": ("kron(5-point 577 x 577, I_3) + kron(I, C)", million, "pcg"),
            "convdiff": ("convection-diffusion 1500 x 1500", convdiff, "bicgstab"),
            "fembig": ("FEM-shaped (40, 40, 257)", fembig, "pcg")}


def multicolour_permuted(M, rp, col, val):
    """Q A Q^T with the rows in the (colour, row) order of spmv_trsv_colour"""
    import scipy.sparse as sps
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
    colour, order = np.zeros(M + 1, np.int32), np.zeros(M + 1, np.int32)
    assert sp.lib().spmv_trsv_colour(M, ip(rp), ip(col), ip(colour), ip(order)) > 0
    a = sps.csr_matrix((val, col, rp), shape=(M, M))[order[:M]][:, order[:M]].tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


class Vec:
    def __init__(self, host):
        self.p = C.c_void_p()
        assert sp.lib().spmv_hip_malloc(C.byref(self.p), host.nbytes) == 0
        assert sp.lib().spmv_hip_memcpy_h2d(self.p, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0

    def close(self):
        sp.lib().spmv_hip_free(self.p)


def us_per_call(call, reps):
    call()
    sp.hip_sync()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    sp.hip_sync()
    return (time.perf_counter() - t) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="million,convdiff,fembig")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sp.hip_init(0)
    name, cus, _ = sp.device_name()
    S, R = args.steps, args.reps
    out = open(args.out, "w") if args.out else None

    def emit(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"device: {name.strip()} ({cus} CUs); fp64; solves and applies: host time over {R} asynchronous calls; "
         f"solver steps: device time of {S} steps with tol = 0")
    for key in args.matrices.split(","):
        title, make, method = MATRICES[key]
        M, rp, col, val = make()
        b = np.random.default_rng(7).uniform(-1, 1, M)
        emit()
        emit(f"## {key}: {title}, {M / 1e6:.2f} M rows, {int(rp[-1]) / 1e6:.1f} M entries ({method})")
        emit()
        with sp.CsrDevice(M, M, rp, col, val) as dev:
            settle(dev)
            t_spmv = float(np.median(dev.time(sp.CSR_AUTO, 5, 100, zero_y=False))) * 1e3
            solve = (lambda **kw: dev.pcg(b, **kw)) if method == "pcg" else (lambda **kw: dev.bicgstab(b, **kw))
            ms = lambda res: res[4] if method == "pcg" else res[3]        # noqa: E731
            info = lambda res: res[3] if method == "pcg" else res[2]      # noqa: E731
            solve(iters=S)
            t_plain = ms(solve(iters=S)) * 1e3 / S
            emit(f"SpMV (AUTO) {t_spmv:.1f} us; unpreconditioned {method} step {t_plain:.1f} us")
            emit()
            emit("| ordering | levels fwd / bwd | launches fwd / bwd | widest | median | colours | analysis ms | "
                 "factorisation ms | upload ms | forward us (x SpMV) | backward us (x SpMV) | apply us (x SpMV) |")
            emit("|---|---|---|---|---|---|---|---|---|---|---|---|")
            d_r, d_z = Vec(b), Vec(np.zeros(M))
            for ordering in ("natural", "multicolor"):
                with dev.preconditioner("ilu0", ordering=ordering) as P:
                    t = P.tri_info()
                    t_apply = us_per_call(lambda: P.apply_on(d_r.p.value, d_z.p.value), R)
                own = dev if ordering == "natural" else sp.CsrDevice(M, M, *multicolour_permuted(M, rp, col, val))
                with own.triangular(lower=True, unit_diagonal=True) as Tl, own.triangular(lower=False) as Tu:
                    t_f = us_per_call(lambda: Tl.solve_on(d_r.p.value, d_z.p.value), R)
                    t_b = us_per_call(lambda: Tu.solve_on(d_r.p.value, d_z.p.value), R)
                if own is not dev:
                    own.close()
                fwd, bwd = f"{t_f:.0f} ({t_f / t_spmv:.1f})", f"{t_b:.0f} ({t_b / t_spmv:.1f})"
                emit(f"| {ordering} | {t['forward_levels']} / {t['backward_levels']} | {t['forward_launches']} / "
                     f"{t['backward_launches']} | {t['forward_widest']} | {t['forward_median']} | {t['colours']} | "
                     f"{t['analysis_us'] / 1e3:.0f} | {t['factor_us'] / 1e3:.0f} | {t['upload_us'] / 1e3:.0f} | {fwd} | "
                     f"{bwd} | {t_apply:.0f} ({t_apply / t_spmv:.1f}) |")
            d_r.close(), d_z.close()
            emit()
            emit(f"| {method} with | us / step | / unpreconditioned step | steps to 1e-8 | status | ms to 1e-8 |")
            emit("|---|---|---|---|---|---|")
            kinds = [("none", None), ("jacobi", dict(kind="jacobi")), ("block_jacobi 3", dict(kind="block_jacobi", block=3)),
                     ("ilu0 natural", dict(kind="ilu0")), ("ilu0 multicolor", dict(kind="ilu0", ordering="multicolor")),
                     ("ssor(1) natural", dict(kind="ssor")), ("ssor(1) multicolor", dict(kind="ssor", ordering="multicolor"))]
            for label, kw in kinds:
                P = dev.preconditioner(**kw) if kw else None
                solve(iters=2, precond=P)
                t_step = ms(solve(iters=S, precond=P)) * 1e3 / S
                res = solve(iters=3000, tol=1e-8, precond=P)
                emit(f"| {label} | {t_step:.1f} | {t_step / t_plain:.2f} | {info(res)['steps']} | {info(res)['status']} | "
                     f"{ms(res):.1f} |")
                if P:
                    P.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
