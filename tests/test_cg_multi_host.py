"""Multi-RHS CG (k CG recurrences sharing one SpMM per step) without a GPU: the C-ABI is exported and bound,
CsrDevice.cg_multi checks its input before any device call, the entry point refuses a NULL handle, and the vector
kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels


def test_cg_multi_symbol_is_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "spmv_hip_csr_cg_multi" in exported
    assert "spmv_hip_csr_cg_multi" in sp.EXPORTED_SYMBOLS
    fn = sp.lib().spmv_hip_csr_cg_multi
    assert fn.restype is C.c_int
    assert fn.argtypes[3] is C.c_double   # tol


def _handle_without_device(M=5, N=5, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


@pytest.mark.parametrize("B", [np.zeros((4, 2)), np.zeros((5, 0)), np.zeros((5, 65)), np.zeros((5, 2, 1)),
                               np.zeros(3), np.zeros((5, 2), dtype=np.float32), np.zeros(5, dtype=np.int64)],
                         ids=["rows", "k0", "k65", "3d", "short-vector", "fp32", "int"])
def test_cg_multi_rejects_wrong_shape_or_dtype_before_any_device_call(B):
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.cg_multi(B, 3)


def test_cg_multi_rejects_fp64_input_on_an_fp32_handle_and_bad_scalars():
    dev32 = _handle_without_device(dtype=np.float32)
    with pytest.raises(ValueError):
        dev32.cg_multi(np.zeros((5, 3)), 3)
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.cg_multi(np.zeros((5, 3)), -1)
    for tol in (-1e-3, float("nan")):
        with pytest.raises(ValueError):
            dev.cg_multi(np.zeros((5, 3)), 3, tol=tol)


def test_cg_multi_refuses_a_null_handle():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    buf = (C.c_double * 16)()
    hist = (C.c_double * 16)()
    done = (C.c_int * 4)()
    ms = C.c_float(0)
    assert sp.lib().spmv_hip_csr_cg_multi(None, 2, 3, 0.0, None, buf, buf, hist, done, C.byref(ms)) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cg_and_shared_solver_kernels_compile_for_gfx950_without_scratch():
    kernels = {k: (v.scratch, v.vgprs) for k, v in compile_kernels("spmv_cg.hip").items()}
    mcg = {k: v for k, v in kernels.items() if "mcg_" in k or "solver_" in k}
    # {dot_partial, update_x_r, update_p} x {fp64 element, fp64 16-byte, fp32 element, fp32 16-byte}, the three scalar
    # kernels, and the shared fold and rank sum of solver_ops.hpp
    vector = [k for k in mcg if re.search(r"mcg_(dot_partial|update_x_r|update_p)I[df]Li[124]E", k)]
    assert len(vector) == 12, sorted(mcg)
    for name in ("solver_fold", "solver_rank_sum", "mcg_start", "mcg_set_alpha", "mcg_set_beta"):
        assert any(name in k for k in mcg), (name, sorted(mcg))
    for name, (scratch, vgprs) in mcg.items():
        assert scratch == 0, f"{name} spills {scratch} bytes of scratch ({vgprs} VGPRs)"
