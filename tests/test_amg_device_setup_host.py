"""The AMG device setup without a device: its two entry points in the library, the header, the version script and the
binding table, the setup info words, the Python argument checks ahead of any library call, what hipcc makes of its
kernels for gfx950, and the loud failure where no device is present."""
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels
from conftest import ROOT

NEW = {"spmv_hip_csr_precond_build_amg_device": 7, "spmv_hip_precond_amg_setup_info": 2}
CSRC = os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc")


def null_handle():
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)      # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = 5, 5, np.float64
    return dev


def test_new_symbols_are_in_step():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    listed = set(re.findall(r"^\s+(\w+);", open(os.path.join(CSRC, "libspmv_amd.map")).read(), flags=re.M))
    L = sp.lib()
    for name, nargs in NEW.items():
        assert name in exported and name in listed and name in sp.EXPORTED_SYMBOLS, name
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", header)
        assert declared and len(declared.group(1).split(",")) == nargs, name
        assert len(getattr(L, name).argtypes) == nargs, name
    # the parts of the host setup the device setup calls stay inside the library
    assert not {"amg_aggregate", "amg_dense_inverse"} & exported
    assert "amg_aggregate" not in header and "amg_dense_inverse" not in header


def test_setup_info_words_agree():
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    words = int(re.search(r"SPMV_PRECOND_AMG_SETUP_INFO_WORDS\s*=\s*(\d+)", header).group(1))
    assert words == sp.device.PRECOND_AMG_SETUP_INFO_WORDS == len(sp.device.PRECOND_AMG_SETUP_INFO) == 10
    assert sp.device.PRECOND_AMG_SETUP_INFO[0] == "setup" and sp.device.AMG_SETUPS == {"host": 0, "device": 1}
    kernels = open(os.path.join(CSRC, "hip", "spgemm_kernels.hpp")).read()
    assert int(re.search(r"kSgMaxProducts\s*=\s*(\d+)", kernels).group(1)) == sp.device.SPGEMM_MAX_BLOCK_PRODUCTS


def test_python_arguments_are_checked_before_the_library_is_asked():
    dev = null_handle()
    for kw in ({"setup": "gpu"}, {"setup": None}, {"setup": 1}, {"setup": "device", "block_products": 3},
               {"setup": "device", "block_products": 8192}, {"setup": "device", "block_products": 96},
               {"setup": "device", "block_products": True}, {"setup": "device", "block_products": 64.5},
               {"setup": "host", "block_products": 64}, {"block_products": -1},
               {"setup": "device", "theta": 1.0}, {"setup": "device", "coarse_rows": 257},
               {"setup": "device", "max_levels": 0}):
        with pytest.raises(ValueError):
            dev.preconditioner("amg", **kw)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_setup_kernels_do_not_spill_and_the_product_kernels_stay_in_their_unit():
    kernels = compile_kernels("spmv_amg_setup.hip", timeout=900)
    ours = {}
    for name in ("as_row_stats", "as_strong_count", "as_strong_emit", "as_graph", "as_smooth", "as_round", "as_g"):
        found = {k: v for k, v in kernels.items() if name in k}
        assert found, (name, sorted(kernels))
        ours.update(found)
    assert len([k for k in ours if "as_round" in k]) == 2 and len([k for k in ours if "as_g" in k and "as_graph" not in k]) == 2
    for name, k in ours.items():                                 # streams over a level: no LDS, no scratch
        assert k.scratch == 0 and k.lds == 0, f"{name}: {k.scratch} bytes of scratch, {k.lds} of LDS ({k.vgprs} VGPRs)"
    # the products come from spmv_spgemm.hip's core: no second copy of its kernels here
    assert not [k for k in kernels if "sg_" in k or "tr_gather" in k], sorted(kernels)


def test_the_device_setup_fails_loudly_without_a_device():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    dev = null_handle()
    for kw in ({}, {"block_products": 64}, {"block_products": -1}):
        with pytest.raises(sp.SpmvHipError):
            dev.preconditioner("amg", setup="device", **kw)
    out = (sp.device.C.c_int * sp.device.PRECOND_AMG_SETUP_INFO_WORDS)()
    assert sp.lib().spmv_hip_precond_amg_setup_info(None, out) == -1
