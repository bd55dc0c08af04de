"""spmv_hip_csr_add without a GPU: the C-ABI is exported and bound, the tuples match the header's word counts, CsrDevice.add
checks its arguments before any device call, and the definition's canon(A) is the product's A I byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _spadd_ref import canon, identity_csr, random_unsorted
from _spgemm_ref import spgemm_ref
from conftest import ROOT


def test_add_symbol_is_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "spmv_hip_csr_add" in exported
    assert "spmv_hip_csr_add" in sp.EXPORTED_SYMBOLS
    fn = sp.lib().spmv_hip_csr_add
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 10
    assert fn.argtypes[0] is C.c_void_p and fn.argtypes[1] is C.c_double      # a, alpha
    assert fn.argtypes[2] is C.c_void_p and fn.argtypes[3] is C.c_double      # b, beta
    assert all(t is C.c_int for t in fn.argtypes[4:7])                        # method, lanes, long_row
    assert fn.argtypes[7] is C.POINTER(C.c_void_p)                            # out
    assert fn.argtypes[8] is C.POINTER(C.c_longlong)                          # stats
    assert fn.argtypes[9] is C.POINTER(C.c_double)                            # ms


def test_add_tuples_match_the_headers_word_counts():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    doc = text[:text.index("int spmv_hip_csr_add(")]
    doc = doc[doc.rindex("/*"):]
    assert int(re.search(r"stats \((\d+), may be NULL\)", doc).group(1)) == len(sp.ADD_STATS) == 6
    assert int(re.search(r"ms \((\d+), may be NULL\)", doc).group(1)) == len(sp.ADD_MS) == 5
    assert sp.ADD_STATS == ("nz", "matches", "a_canonical", "b_canonical", "long_rows", "max_row_nz")
    assert sp.ADD_MS == ("check", "canonical", "symbolic", "numeric", "adopt")


def _handle_without_device(M=5, N=5, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


def test_add_refuses_a_non_handle():
    dev = _handle_without_device()
    for other in (3.0, np.eye(5), "A"):
        with pytest.raises(TypeError):
            dev.add(other)
        with pytest.raises(TypeError):
            dev + other
        with pytest.raises(TypeError):
            dev - other


@pytest.mark.parametrize("shape", [(4, 5), (5, 4), (6, 6)])
def test_add_refuses_other_shapes_and_dtypes(shape):
    dev = _handle_without_device()
    with pytest.raises(ValueError, match=f"{shape[0]} x {shape[1]}"):
        dev.add(_handle_without_device(*shape))
    with pytest.raises(ValueError, match="float32"):
        dev.add(_handle_without_device(dtype=np.float32))
    with pytest.raises(ValueError):
        dev - _handle_without_device(*shape)


@pytest.mark.parametrize("bad", [dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("-inf")),
                                 dict(beta=float("nan")), dict(method="sort"), dict(method=1), dict(lanes=3), dict(lanes=128),
                                 dict(lanes=-2), dict(long_row=-1), dict(long_row=1 << 31)])
def test_add_refuses_bad_scalars_before_any_device_call(bad):
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.add(_handle_without_device(), **bad)
    with pytest.raises(ValueError):
        dev.add(None, **bad)


def test_add_refuses_a_row_range_handle():
    dev, part = _handle_without_device(), _handle_without_device()
    part.row0, part.row1 = 1, 5
    with pytest.raises(ValueError, match=r"rows \(1, 5\) of 5"):
        dev.add(part)
    with pytest.raises(ValueError):
        part.add(dev)
    with pytest.raises(ValueError):
        part.canonical()
    with pytest.raises(ValueError):
        -part


def test_add_refuses_a_null_handle():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    out = C.c_void_p()
    assert sp.lib().spmv_hip_csr_add(None, 1.0, None, 1.0, 0, 0, 0, C.byref(out), None, None) == -1


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_canon_is_the_products_a_times_identity_byte_for_byte(dtype):
    rng = np.random.default_rng(21)
    for M, N, mean in ((130, 77, 5), (40, 9, 12), (7, 3, 3), (0, 5, 1)):
        a = random_unsorted(rng, M, N, mean, dtype)
        want = spgemm_ref(M, N, a, identity_csr(N, dtype), dtype)
        got = canon(M, N, a, dtype)
        if M > 7:
            assert len(got[1]) < len(a[1]), "no repeated pair in the case"
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
