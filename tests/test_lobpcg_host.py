"""LOBPCG without a GPU: the four entry points are exported, listed in the version script, declared and bound;
CsrDevice.lobpcg checks its input before any device call; spmv_lobpcg_rr (the host Rayleigh-Ritz step) against a numpy
restatement; the kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _lobpcg_ref import rr_ref
from _util import HIPCC, compile_kernels
from conftest import ROOT

NEW = ("spmv_hip_csr_lobpcg", "spmv_lobpcg_rr", "spmv_hip_lobpcg_gram", "spmv_hip_lobpcg_update")


def test_new_symbols_are_exported_listed_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    version_script = open(os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc", "libspmv_amd.map")).read()
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    for name in NEW:
        assert name in exported and name in sp.EXPORTED_SYMBOLS, name
        assert re.search(rf"^\s*{name};", version_script, re.M), name
        assert re.search(rf"^int {name}\(", header, re.M), name
    L = sp.lib()
    int_p, double_p, float_p = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
    ptrs = C.POINTER(C.c_void_p)
    solve = L.spmv_hip_csr_lobpcg
    assert solve.restype is C.c_int
    assert list(solve.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int] + [double_p] * 7 + \
        [int_p, float_p, float_p]
    rr = L.spmv_lobpcg_rr
    assert rr.restype is C.c_int
    assert list(rr.argtypes) == [C.c_int, C.c_int, double_p, double_p, C.c_int, C.c_double, double_p, double_p, double_p,
                                 int_p, int_p]
    gram = L.spmv_hip_lobpcg_gram
    assert gram.restype is C.c_int
    assert list(gram.argtypes) == [C.c_longlong, C.c_int, C.c_int, ptrs, ptrs, double_p, double_p]
    update = L.spmv_hip_lobpcg_update
    assert update.restype is C.c_int
    assert list(update.argtypes) == [C.c_longlong, C.c_int, C.c_int, ptrs, ptrs, double_p, double_p] + [C.c_void_p] * 4


def test_status_values_match_the_header():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    for name, value in (("RAN_ALL", 0), ("CONVERGED", 1), ("BREAKDOWN", 2)):
        assert re.search(rf"SPMV_LOBPCG_{name}\s*=\s*{value}\b", text), name
        assert getattr(sp, f"LOBPCG_{name}") == value


def test_entry_points_refuse_null_arguments():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    L = sp.lib()
    buf = (C.c_double * 64)()
    words = (C.c_int * 4)()
    ms = C.c_float(0)
    assert L.spmv_hip_csr_lobpcg(None, None, 2, 3, 0.0, 0, buf, buf, buf, buf, buf, buf, buf, words, C.byref(ms),
                                 C.byref(ms)) == -1
    assert L.spmv_hip_lobpcg_gram(8, 2, 1, None, None, buf, buf) == -1
    assert L.spmv_hip_lobpcg_update(8, 2, 1, None, None, buf, buf, None, None, None, None) == -1


def test_rr_refuses_bad_arguments():
    L = sp.lib()
    buf = (C.c_double * (48 * 48))()
    kept, restarted = C.c_int(0), C.c_int(0)
    good = (buf, buf, 0, 1e-10, buf, buf, buf, C.byref(kept), C.byref(restarted))
    assert L.spmv_lobpcg_rr(1, 2, *good) in (0, 1)
    for nb, k in ((0, 2), (4, 2), (1, 0), (1, 17)):
        assert L.spmv_lobpcg_rr(nb, k, *good) == -1
    assert L.spmv_lobpcg_rr(1, 2, None, buf, 0, 1e-10, buf, buf, buf, None, None) == -1
    assert L.spmv_lobpcg_rr(1, 2, buf, buf, 0, 1e-10, None, buf, buf, None, None) == -1
    assert L.spmv_lobpcg_rr(1, 2, buf, buf, 0, float("nan"), buf, buf, buf, None, None) == -1


def _handle_without_device(M=64, N=64, dtype=np.float64):
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)  # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = M, N, dtype
    return dev


def _precond_without_device(rows=64, row0=0, dtype=np.float64, kind=sp.PRECOND_JACOBI):
    P = sp.Preconditioner.__new__(sp.Preconditioner)
    sp.device._Handle.__init__(P)
    P.kind, P.block, P.rows, P.row0, P.dtype = kind, 1, rows, row0, dtype
    return P


def test_lobpcg_rejects_bad_handles_before_any_device_call():
    """(A tiles-only handle exists only inside an HLL handle and cannot be reached from Python: the C entry point
    refuses it.  An active communicator needs a device: tests/test_gpu_lobpcg.py.)"""
    with pytest.raises(ValueError):
        _handle_without_device(dtype=np.float32).lobpcg(2, 3)
    with pytest.raises(ValueError):
        _handle_without_device(M=64, N=65).lobpcg(2, 3)
    half = _handle_without_device()
    half.row0, half.row1 = 0, 32
    with pytest.raises(ValueError):
        half.lobpcg(2, 3)


@pytest.mark.parametrize("k", [0, 17, -1, 2.5, True])
def test_lobpcg_rejects_a_bad_k_before_any_device_call(k):
    with pytest.raises(ValueError):
        _handle_without_device().lobpcg(k, 3)


def test_lobpcg_rejects_small_n_bad_iters_tol_and_X0_before_any_device_call():
    for k in (1, 4, 16):
        with pytest.raises(ValueError):
            _handle_without_device(M=4 * k - 1, N=4 * k - 1).lobpcg(k, 3)
    dev = _handle_without_device()
    with pytest.raises(ValueError):
        dev.lobpcg(2, -1)
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.lobpcg(2, 3, tol=tol)
    for X0 in (np.zeros((64, 3)), np.zeros((63, 2)), np.zeros((64, 2), np.float32), np.zeros(64)):
        with pytest.raises(ValueError):
            dev.lobpcg(2, 3, X0=X0)


def test_lobpcg_rejects_an_active_communicator_before_any_device_call(monkeypatch):
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    monkeypatch.setattr(NativeComm, "active", True)
    with pytest.raises(ValueError, match="communicator"):
        _handle_without_device().lobpcg(2, 3)


def test_lobpcg_rejects_bad_preconditioners_before_any_device_call():
    dev = _handle_without_device()
    for P in ("jacobi", _precond_without_device(rows=63), _precond_without_device(row0=1),
              _precond_without_device(dtype=np.float32), _precond_without_device(kind=sp.PRECOND_SSOR),
              _precond_without_device(kind=sp.PRECOND_ILU0)):
        with pytest.raises(ValueError):
            dev.lobpcg(2, 3, precond=P)
    with pytest.raises(ValueError):
        dev.lobpcg(2, 3, precond=_precond_without_device(), largest=True)


# ---------------------------------------------------------------- spmv_lobpcg_rr against numpy
def _grams(k, nb, seed=3, n=200):
    rng = np.random.default_rng(seed + 100 * k + nb)
    S = rng.standard_normal((n, nb * k))
    M = rng.standard_normal((n, n))
    M = M + M.T
    return S, M @ S


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_rr_matches_numpy(k, nb, largest):
    S, AS = _grams(k, nb)
    GB, GA = S.T @ S, S.T @ AS
    rc, theta, Cm, Cp, kept, restarted = sp.lobpcg_rr(GB, GA, nb, k, largest)
    ref_theta = rr_ref(GB, GA, nb, k, largest)[0]
    assert (rc, kept, restarted) == (0, nb * k, 0)
    scale = np.abs(ref_theta).max()
    assert np.abs(theta - ref_theta).max() <= 1e-12 * scale
    order = np.diff(theta)
    assert np.all(order <= 0) if largest else np.all(order >= 0)
    B, A = (GB + GB.T) / 2, (GA + GA.T) / 2
    assert np.abs(Cm.T @ B @ Cm - np.eye(k)).max() <= 1e-10
    assert np.abs(Cm.T @ A @ Cm - np.diag(theta)).max() <= 1e-10 * scale
    assert np.all(Cp[:k] == 0)
    if nb > 1:
        assert np.abs(np.einsum("ij,ij->j", Cp, B @ Cp) - 1).max() <= 1e-12
        # Cp is C without its X rows, rescaled column by column
        ratio = Cp[k:] / Cm[k:]
        assert np.abs(ratio - ratio[0]).max() <= 1e-9 * np.abs(ratio[0]).max()
    else:
        assert np.all(Cp == 0)


@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_rr_restarts_without_p_when_p_copies_w(k):
    S, _ = _grams(k, 3)
    S[:, 2 * k:] = S[:, k:2 * k]
    rng = np.random.default_rng(9)
    M = rng.standard_normal((200, 200))
    AS = (M + M.T) @ S
    GB, GA = S.T @ S, S.T @ AS
    rc, theta, Cm, Cp, kept, restarted = sp.lobpcg_rr(GB, GA, 3, k)
    assert (rc, kept, restarted) == (0, 2 * k, 1)
    assert np.all(Cm[2 * k:] == 0) and np.all(Cp[2 * k:] == 0)
    ref = rr_ref(GB, GA, 3, k)
    assert ref[3:] == (2 * k, 1)
    assert np.abs(theta - ref[0]).max() <= 1e-12 * np.abs(ref[0]).max()


def test_rr_drops_a_zero_column_without_a_nan():
    k = 3
    S, AS = _grams(k, 2)
    S[:, k + 1] = 0
    AS[:, k + 1] = 0
    GB, GA = S.T @ S, S.T @ AS
    rc, theta, Cm, Cp, kept, restarted = sp.lobpcg_rr(GB, GA, 2, k)
    assert (rc, kept, restarted) == (0, 2 * k - 1, 0)
    assert np.isfinite(theta).all() and np.isfinite(Cm).all() and np.isfinite(Cp).all()
    assert np.all(Cm[k + 1] == 0) and np.all(Cp[k + 1] == 0)
    assert np.abs(theta - rr_ref(GB, GA, 2, k)[0]).max() <= 1e-12 * np.abs(theta).max()


def test_rr_two_equal_columns_at_nb_1_keep_fewer_than_k():
    k = 4
    S, AS = _grams(k, 1)
    S[:, 2], AS[:, 2] = S[:, 0], AS[:, 0]
    rc, theta, Cm, Cp, kept, restarted = sp.lobpcg_rr(S.T @ S, S.T @ AS, 1, k)
    assert rc == 1 and kept == k - 1 and restarted == 0


@pytest.mark.parametrize("where", ["GB", "GA"])
def test_rr_reports_a_nan_entry_as_a_breakdown(where):
    S, AS = _grams(3, 2)
    GB, GA = S.T @ S, S.T @ AS
    (GB if where == "GB" else GA)[1, 4] = np.nan
    rc, theta, Cm, Cp, kept, restarted = sp.lobpcg_rr(GB, GA, 2, 3)
    assert rc == 1 and kept == 0
    assert np.isfinite(theta).all() and np.isfinite(Cm).all() and np.isfinite(Cp).all()


# ---------------------------------------------------------------- the kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lobpcg_kernels_compile_for_gfx950_without_scratch():
    kernels = compile_kernels("spmv_lobpcg.hip")
    for name, v in kernels.items():
        assert v.scratch == 0, f"{name} spills {v.scratch} bytes of scratch ({v.vgprs} VGPRs)"
    for mt in (1, 2, 3):
        found = [k for k in kernels if re.search(rf"lob_gramILi{mt}EE", k)]
        assert len(found) == 1, (mt, sorted(kernels))
        assert kernels[found[0]].lds == 4 * 256 * 8   # 4 waves x one tile of 256 doubles
    for nb in (1, 2, 3):
        for kp in (4, 8, 16):
            found = [k for k in kernels if re.search(rf"lob_updateILi{nb}ELi{kp}ELb[01]EE", k)]
            assert len(found) == 2, (nb, kp, sorted(kernels))   # single elements and 16-byte pieces
            for name in found:
                assert kernels[name].lds == nb * kp * kp * 16   # the {C, Cp} pairs, at most 12 KB
    assert len([k for k in kernels if re.search(r"lob_residualILi[12]EE", k)]) == 2
    for name in ("lob_row_abs_max", "lob_max", "solver_fold"):
        assert any(re.search(rf"\d{name}E", k) for k in kernels), (name, sorted(kernels))
    assert max(v.lds for v in kernels.values()) <= 12 * 1024, {k: v.lds for k, v in kernels.items()}
