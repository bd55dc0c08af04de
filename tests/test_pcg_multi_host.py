"""Preconditioned CG for k right-hand sides without a GPU: the solver and the two k-wide apply entry points are exported,
listed in the version script and bound, the Python methods check their input before any device call, and the new
kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels
from conftest import ROOT

VGPR_BOUND = 64  # the bound the solver kernels sit under (test_precond_host.py)
NEW = ("spmv_hip_csr_pcg_multi", "spmv_hip_precond_apply_multi", "spmv_hip_precond_apply_multi_on")


def test_new_symbols_are_exported_listed_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    version_script = open(os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc", "libspmv_amd.map")).read()
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    for name in NEW:
        assert name in exported and name in sp.EXPORTED_SYMBOLS, name
        assert re.search(rf"^\s*{name};", version_script, re.M), name
        assert re.search(rf"^int {name}\(", header, re.M), name
    L = sp.lib()
    int_p, double_p = C.POINTER(C.c_int), C.POINTER(C.c_double)
    solve = L.spmv_hip_csr_pcg_multi
    assert solve.restype is C.c_int
    assert list(solve.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, int_p, C.c_void_p, C.c_void_p,
                                    double_p, double_p, int_p, int_p, C.POINTER(C.c_float)]
    on = L.spmv_hip_precond_apply_multi_on
    assert on.restype is C.c_int
    assert list(on.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    host = L.spmv_hip_precond_apply_multi
    assert host.restype is C.c_int and list(host.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]


def _handle_without_device(M=6, N=6, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


def _precond_without_device(rows=6, row0=0, dtype=np.float64):
    P = sp.Preconditioner.__new__(sp.Preconditioner)
    sp.device._Handle.__init__(P)
    P.kind, P.block, P.rows, P.row0, P.dtype = sp.PRECOND_JACOBI, 1, rows, row0, dtype
    return P


BAD_ARRAYS = {
    "1-D": np.zeros(6),
    "wrong dtype": np.zeros((6, 2), np.float32),
    "integers": np.zeros((6, 2), np.int64),
    "not C-contiguous": np.zeros((2, 6)).T,
    "a strided view": np.zeros((6, 4))[:, ::2],
    "k = 65": np.zeros((6, 65)),
    "k = 0": np.zeros((6, 0)),
    "wrong rows": np.zeros((5, 2)),
    "3-D": np.zeros((6, 2, 1)),
}


@pytest.mark.parametrize("what", sorted(BAD_ARRAYS))
def test_pcg_multi_rejects_a_bad_B_before_any_device_call(what):
    with pytest.raises(ValueError):
        _handle_without_device().pcg_multi(BAD_ARRAYS[what], 3)


def test_pcg_multi_rejects_bad_iters_tol_and_preconditioners_before_any_device_call():
    dev = _handle_without_device()
    B = np.zeros((6, 2))
    with pytest.raises(ValueError):
        dev.pcg_multi(B, -1)
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.pcg_multi(B, 3, tol=tol)
    for P in ("jacobi", _precond_without_device(rows=5), _precond_without_device(row0=1),
              _precond_without_device(dtype=np.float32)):
        with pytest.raises(ValueError):
            dev.pcg_multi(B, 3, precond=P)
    half = _handle_without_device()
    half.row0, half.row1 = 0, 3   # a row-range handle: P must cover the same rows
    with pytest.raises(ValueError):
        half.pcg_multi(B, 3, precond=_precond_without_device(rows=6))


@pytest.mark.parametrize("what", sorted(BAD_ARRAYS))
def test_apply_multi_rejects_a_bad_R_before_any_device_call(what):
    with pytest.raises(ValueError):
        _precond_without_device().apply_multi(BAD_ARRAYS[what])


@pytest.mark.parametrize("k", [0, 65, -1, 2.5, True])
def test_apply_multi_on_rejects_a_bad_k_before_any_device_call(k):
    with pytest.raises(ValueError):
        _precond_without_device().apply_multi_on(256, 512, k)


def test_entry_points_refuse_null_arguments():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    L = sp.lib()
    buf = (C.c_double * 8)()
    words = (C.c_int * 4)()
    ms = C.c_float(0)
    assert L.spmv_hip_csr_pcg_multi(None, None, 2, 3, 0.0, None, buf, buf, buf, buf, words, words, C.byref(ms)) == -1
    assert L.spmv_hip_precond_apply_multi(None, 2, buf, buf) == -1
    assert L.spmv_hip_precond_apply_multi_on(None, 2, buf, buf, None, None) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_pcg_multi_kernels_compile_for_gfx950_without_scratch():
    kernels = compile_kernels("spmv_pcg_multi.hip")
    for name, v in kernels.items():
        assert v.scratch == 0, f"{name} spills {v.scratch} bytes of scratch ({v.vgprs} VGPRs)"
        assert v.vgprs <= VGPR_BOUND, f"{name}: {v.vgprs} VGPRs > {VGPR_BOUND}"
    # every vector kernel in its lane shapes: fp64 pieces of 2, fp32 pieces of 4, single elements of both
    shapes = r"I(dLi2|fLi4|dLi1|fLi1)E"
    for pattern, count in ((rf"mpcg_start_dots{shapes}Lb[01]EE", 8), (rf"mpcg_update_x_r{shapes}Li[012]EE", 12),
                           (rf"mpc_apply{shapes}Lb[01]EE", 8), (rf"mpcg_dots{shapes}E", 4),
                           (rf"mcg_dot_partial{shapes}E", 4), (rf"mcg_update_p{shapes}E", 4)):
        found = [k for k in kernels if re.search(pattern, k)]
        assert len(found) == count, (pattern, sorted(kernels))
    for name in ("mpcg_start", "mpcg_set_alpha", "mpcg_set_beta", "solver_fold", "solver_rank_sum"):
        assert any(re.search(rf"\d{name}E", k) for k in kernels), (name, sorted(kernels))
    # the two-plane partials reuse cg_multi's staging array behind a barrier: no kernel holds more than that array
    assert max(v.lds for v in kernels.values()) <= (256 // 64) * 64 * 8, {k: v.lds for k, v in kernels.items()}
