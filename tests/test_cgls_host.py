"""Transposed handles and CGLS without a GPU: both C-ABI symbols are exported and bound, the status values match the
header, CsrDevice.cgls checks its input before any device call, the entry points refuse NULL handles, and the new
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

VGPR_BOUND = 64  # as test_bicgstab_host.py: the vector kernels stream


def exported_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_transpose_and_cgls_symbols_are_exported_and_bound():
    exported = exported_symbols()
    for name in ("spmv_hip_csr_transpose", "spmv_hip_csr_cgls"):
        assert name in exported and name in sp.EXPORTED_SYMBOLS, name
    fn = sp.lib().spmv_hip_csr_transpose
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_void_p)]
    fn = sp.lib().spmv_hip_csr_cgls
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 11
    assert fn.argtypes[0] is C.c_void_p and fn.argtypes[1] is C.c_void_p      # m, mt
    assert fn.argtypes[2] is C.c_int                                          # iters
    assert fn.argtypes[3] is C.c_double and fn.argtypes[4] is C.c_double      # tol, damp
    assert fn.argtypes[7] is C.POINTER(C.c_double) and fn.argtypes[8] is C.POINTER(C.c_double)  # histories
    assert fn.argtypes[9] is C.POINTER(C.c_int) and fn.argtypes[10] is C.POINTER(C.c_float)    # info, ms


def test_cgls_status_values_match_the_header():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    for name, value in (("RAN_ALL", 0), ("CONVERGED", 1), ("BREAKDOWN", 2)):
        assert re.search(rf"SPMV_CGLS_{name}\s*=\s*{value}\b", text), name
        assert getattr(sp, f"CGLS_{name}") == value


def _handle_without_device(M=5, N=3, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


@pytest.mark.parametrize("b", [np.zeros(4), np.zeros(3), np.zeros(6), np.zeros((5, 1)), np.zeros(5, dtype=np.float32),
                               np.zeros(5, dtype=np.int64)],
                         ids=["short", "N-long", "long", "2d", "fp32", "int"])
def test_cgls_rejects_wrong_length_or_dtype_before_any_device_call(b):
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.cgls(b, 3)                  # with at=None a transpose would be the first device call


def test_cgls_rejects_bad_scalars_and_transposes_before_any_device_call():
    dev32 = _handle_without_device(dtype=np.float32)
    with pytest.raises(ValueError):
        dev32.cgls(np.zeros(5), 3)
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.cgls(np.zeros(5), -1)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.cgls(np.zeros(5), 3, tol=bad)
        with pytest.raises(ValueError):
            dev.cgls(np.zeros(5), 3, damp=bad)
    with pytest.raises(ValueError):
        dev.cgls(np.zeros(5), 3, at="not a handle")


def test_transpose_and_cgls_refuse_null_handles():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    L = sp.lib()
    out = C.c_void_p()
    assert L.spmv_hip_csr_transpose(None, C.byref(out)) == -1 and out.value is None
    buf = (C.c_double * 8)()
    hist = (C.c_double * 8)()
    info = (C.c_int * 2)()
    ms = C.c_float(0)
    assert L.spmv_hip_csr_cgls(None, None, 3, 0.0, 0.0, buf, buf, hist, hist, info, C.byref(ms)) == -1


def assert_no_scratch(kernels):
    for name, k in kernels.items():
        scratch, vgprs = k.scratch, k.vgprs
        assert scratch == 0, f"{name} spills {scratch} bytes of scratch ({vgprs} VGPRs)"
        assert vgprs <= VGPR_BOUND, f"{name}: {vgprs} VGPRs > {VGPR_BOUND}"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cgls_and_shared_solver_kernels_compile_for_gfx950_without_scratch():
    # with the shared fold (and rank sum) of solver_ops.hpp
    cgls = {k: v for k, v in compile_kernels("spmv_cgls.hip", timeout=900).items() if "cgls_" in k or "solver_" in k}
    # the four vector kernels x {fp64 in 16-byte pieces of 2, fp32 in pieces of 4}
    vector = [k for k in cgls if re.search(r"cgls_(norm2|update_x_r|update_s|update_p)I(dLi2|fLi4)E", k)]
    assert len(vector) == 8, sorted(cgls)
    for name in ("solver_fold", "cgls_start", "cgls_set_alpha", "cgls_set_beta"):
        assert any(name in k for k in cgls), (name, sorted(cgls))
    assert_no_scratch(cgls)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_transpose_kernels_compile_for_gfx950_without_scratch():
    tr = {k: v for k, v in compile_kernels("spmv_transpose.hip", timeout=900).items() if re.search(r"tr_(make_pairs|gather|row_ptr)", k)}
    assert any("tr_make_pairs" in k for k in tr) and any("tr_row_ptr" in k for k in tr), sorted(tr)
    assert sum("tr_gather" in k for k in tr) == 2, sorted(tr)   # fp64 and fp32
    assert_no_scratch(tr)
