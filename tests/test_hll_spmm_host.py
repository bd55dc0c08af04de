"""HLL SpMM (Y = A X for k vectors per pass over the slab) without a GPU: the C-ABI is exported and bound,
HllDevice.spmm checks its input before any device call, the entry points refuse a NULL handle, and the kernels
compile for gfx950 in their own translation unit without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from conftest import ROOT

HLL_SPMM_SYMBOLS = ("spmv_hip_hll_spmm", "spmv_hip_hll_spmm_on", "spmv_hip_hll_spmm_time")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc", "hip")


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
    tmp = tempfile.mkdtemp(prefix="spmv_hll_spmm_regs_")
    try:
        proc = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-I" + SRC, "-c", os.path.join(SRC, "spmv_hll_spmm.hip"), "-o", os.path.join(tmp, "o.o"),
                               "-save-temps=obj"], capture_output=True, text=True, timeout=600, cwd=tmp)
        assert proc.returncode == 0, proc.stderr[-2000:]
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    # 4 column-tile widths x {16-byte, element} loads, for the window and the long-row kernels (fp64 only)
    assert len([k for k in kernels if "hll_spmm_block" in k]) == 8, sorted(kernels)
    assert len([k for k in kernels if "hll_spmm_row" in k]) == 8, sorted(kernels)
    assert not [k for k in kernels if "csr_spmm" in k], sorted(kernels)
    assert len(kernels) == 16, sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name} spills {scratch} bytes of scratch ({vgprs} VGPRs)"
