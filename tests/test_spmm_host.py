"""SpMM (Y = A X for k vectors per pass) without a GPU: the C-ABI is exported and bound, CsrDevice.spmm checks its
input before any device call, the entry points refuse a NULL handle, and the kernels compile for gfx950 without
scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels

SPMM_SYMBOLS = ("spmv_hip_csr_spmm", "spmv_hip_csr_spmm_on", "spmv_hip_csr_spmm_time")


def test_spmm_symbols_are_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in SPMM_SYMBOLS:
        assert name in exported, name
        assert name in sp.EXPORTED_SYMBOLS, name
        assert getattr(sp.lib(), name).restype is C.c_int


def _handle_without_device(M=5, N=4, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


@pytest.mark.parametrize("X", [np.zeros((5, 2)), np.zeros((4, 0)), np.zeros((4, 2, 1)), np.zeros(3),
                               np.zeros((4, 2), dtype=np.float32), np.zeros(4, dtype=np.int64)],
                         ids=["rows", "k0", "3d", "short-vector", "fp32", "int"])
def test_spmm_rejects_wrong_shape_or_dtype_before_any_device_call(X):
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.spmm(X)


def test_spmm_rejects_fp64_input_on_an_fp32_handle():
    dev = _handle_without_device(dtype=np.float32)
    with pytest.raises(ValueError):
        dev.spmm(np.zeros((4, 3)))


def test_spmm_entry_points_refuse_a_null_handle():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    lib = sp.lib()
    buf = (C.c_double * 16)()
    ms = (C.c_float * 4)()
    assert lib.spmv_hip_csr_spmm_on(None, 2, buf, buf, None) == -1
    assert lib.spmv_hip_csr_spmm(None, 2, buf, buf) == -1
    assert lib.spmv_hip_csr_spmm_time(None, 2, 1, 4, ms) == -1
    assert lib.spmv_hip_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_spmm_kernels_compile_for_gfx950_without_scratch():
    kernels = {k: (v.scratch, v.vgprs) for k, v in compile_kernels("spmv_spmm.hip").items()}
    spmm = {k: v for k, v in kernels.items() if "csr_spmm" in k}
    # {fp64, fp32} x 4 column-tile widths x {16-byte, element} loads, for the block and piece kernels; 2 finish kernels
    assert len([k for k in spmm if "csr_spmm_block" in k]) == 16, sorted(spmm)
    assert len([k for k in spmm if "csr_spmm_pieces" in k]) == 16, sorted(spmm)
    assert len([k for k in spmm if "csr_spmm_finish" in k]) == 2, sorted(spmm)
    assert not [k for k in spmm if re.search("csr_tile|tile_expand|csr_stream_local", k)]
    for name, (scratch, vgprs) in spmm.items():
        assert scratch == 0, f"{name} spills {scratch} bytes of scratch ({vgprs} VGPRs)"
