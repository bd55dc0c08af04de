"""HLL SpMM (Y = A X for k vectors per pass over the slab) without a GPU: the C-ABI is exported and bound,
HllDevice.spmm checks its input before any device call, the entry points refuse a NULL handle, and the kernels
compile for gfx950 in their own translation unit without scratch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels

HLL_SPMM_SYMBOLS = ("spmv_hip_hll_spmm", "spmv_hip_hll_spmm_on", "spmv_hip_hll_spmm_time")


def test_hll_spmm_symbols_are_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in HLL_SPMM_SYMBOLS:
        assert name in exported, name
        assert name in sp.EXPORTED_SYMBOLS, name
        assert getattr(sp.lib(), name).restype is C.c_int


def _hll_handle_without_device(M=5, N=4):
    dev = sp.HllDevice.__new__(sp.HllDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N = M, N
    return dev


@pytest.mark.parametrize("X", [np.zeros((5, 2)), np.zeros((4, 0)), np.zeros((4, 2, 1)), np.zeros(3),
                               np.zeros((4, 2), dtype=np.float32), np.zeros(4, dtype=np.int64),
                               np.zeros((4, 3), dtype=np.complex128)],
                         ids=["rows", "k0", "3d", "short-vector", "fp32", "int", "complex"])
def test_hll_spmm_rejects_wrong_shape_or_dtype_before_any_device_call(X):
    dev = _hll_handle_without_device()
    with pytest.raises(ValueError):
        dev.spmm(X)


def test_hll_spmm_entry_points_refuse_a_null_handle():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    lib = sp.lib()
    buf = (C.c_double * 16)()
    ms = (C.c_float * 4)()
    assert lib.spmv_hip_hll_spmm_on(None, 2, buf, buf, None) == -1
    assert lib.spmv_hip_hll_spmm(None, 2, buf, buf) == -1
    assert lib.spmv_hip_hll_spmm_time(None, 2, 1, 4, ms) == -1
    assert lib.spmv_hip_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_hll_spmm_kernels_compile_for_gfx950_without_scratch():
    kernels = {k: (v.scratch, v.vgprs) for k, v in compile_kernels("spmv_hll_spmm.hip").items()}
    # 4 column-tile widths x {16-byte, element} loads, for the window and the long-row kernels (fp64 only)
    assert len([k for k in kernels if "hll_spmm_block" in k]) == 8, sorted(kernels)
    assert len([k for k in kernels if "hll_spmm_row" in k]) == 8, sorted(kernels)
    assert not [k for k in kernels if "csr_spmm" in k], sorted(kernels)
    assert len(kernels) == 16, sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name} spills {scratch} bytes of scratch ({vgprs} VGPRs)"
