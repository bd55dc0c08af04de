"""BiCGSTAB for k right-hand sides without a GPU: the solver is exported, listed in the version script, declared and
bound, the Python method checks its input before any device call, the kernels compile for gfx950 in every lane shape
without scratch, and the restated loop (tests/_bicgstab_multi_ref.py) is bicgstab_ref at k = 1 and gives the listed
fates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _bicgstab_multi_ref import (FATES_ITERS, FATES_TOL, bicgstab_multi_ref, fates_case, fates_expected)
from _util import HIPCC, compile_kernels
from conftest import ROOT
from test_gpu_bicgstab import bicgstab_ref
from test_pcg_multi_host import BAD_ARRAYS, _handle_without_device, _precond_without_device

VGPR_BOUND = 64  # the bound the solver kernels sit under (test_precond_host.py)
NAME = "spmv_hip_csr_bicgstab_multi"


def test_the_symbol_is_exported_listed_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    version_script = open(os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc", "libspmv_amd.map")).read()
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert NAME in exported and NAME in sp.EXPORTED_SYMBOLS
    assert re.search(rf"^\s*{NAME};", version_script, re.M)
    assert re.search(rf"^int {NAME}\(", header, re.M)
    int_p, double_p = C.POINTER(C.c_int), C.POINTER(C.c_double)
    solve = getattr(sp.lib(), NAME)
    assert solve.restype is C.c_int
    assert list(solve.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, int_p, C.c_void_p, C.c_void_p,
                                    double_p, int_p, int_p, int_p, C.POINTER(C.c_float)]


@pytest.mark.parametrize("what", sorted(BAD_ARRAYS))
def test_bicgstab_multi_rejects_a_bad_B_before_any_device_call(what):
    with pytest.raises(ValueError):
        _handle_without_device().bicgstab_multi(BAD_ARRAYS[what], 3)


def test_bicgstab_multi_rejects_bad_iters_tol_and_preconditioners_before_any_device_call():
    dev = _handle_without_device()
    B = np.zeros((6, 2))
    with pytest.raises(ValueError):
        dev.bicgstab_multi(B, -1)
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.bicgstab_multi(B, 3, tol=tol)
    for P in ("jacobi", _precond_without_device(rows=5), _precond_without_device(row0=1),
              _precond_without_device(dtype=np.float32)):
        with pytest.raises(ValueError):
            dev.bicgstab_multi(B, 3, precond=P)


def test_the_entry_point_refuses_null_arguments():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    buf = (C.c_double * 8)()
    words = (C.c_int * 4)()
    ms = C.c_float(0)
    solve = getattr(sp.lib(), NAME)
    assert solve(None, None, 2, 3, 0.0, None, buf, buf, buf, words, words, words, C.byref(ms)) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_bicgstab_multi_kernels_compile_for_gfx950_without_scratch():
    kernels = compile_kernels("spmv_bicgstab_multi.hip")
    for name, v in kernels.items():
        assert v.scratch == 0, f"{name} spills {v.scratch} bytes of scratch ({v.vgprs} VGPRs)"
        assert v.vgprs <= VGPR_BOUND, f"{name}: {v.vgprs} VGPRs > {VGPR_BOUND}"
    # every vector kernel in its four lane shapes: fp64 pieces of 2, fp32 pieces of 4, single elements of both
    shapes = r"I(dLi2|fLi4|dLi1|fLi1)E"
    for pattern, count in ((rf"mbcg_update_s{shapes}Li[012]EE", 12), (rf"mbcg_dot2{shapes}E", 4),
                           (rf"mbcg_update_x_r{shapes}Lb[01]EE", 8), (rf"mbcg_update_p{shapes}Li[012]EE", 12),
                           (rf"mcg_dot_partial{shapes}E", 4)):
        found = [k for k in kernels if re.search(pattern, k)]
        assert len(found) == count, (pattern, sorted(kernels))
    for name in ("mbcg_start", "mbcg_set_alpha", "mbcg_check_s", "mbcg_set_omega", "mbcg_set_beta", "solver_fold",
                 "solver_rank_sum"):
        assert any(re.search(rf"\d{name}E", k) for k in kernels), (name, sorted(kernels))
    # the two-plane partials reuse cg_multi's staging array behind a barrier: no kernel holds more than that array
    assert max(v.lds for v in kernels.values()) <= (256 // 64) * 64 * 8, {k: v.lds for k, v in kernels.items()}


def _dense_columns(A):
    """the k-wide product of the restated loop, column by column through A @ x: bicgstab_ref's own product"""
    return lambda X: np.stack([A @ np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], axis=1)


@pytest.mark.parametrize("tol", [0.0, 1e-9])
def test_the_restated_loop_with_k1_and_no_apply_is_bicgstab_ref_bit_for_bit(tol):
    rng = np.random.default_rng(31)
    n = 80
    A = rng.uniform(-1, 1, (n, n)) * (rng.uniform(0, 1, (n, n)) < 0.1) + 5.0 * np.eye(n)
    for b in (rng.uniform(-1, 1, n), np.zeros(n)):
        x_ref, h_ref, info_ref = bicgstab_ref(lambda v: A @ v, b, 30, tol)
        for apply in (None, lambda R: R.copy()):
            X, H, info = bicgstab_multi_ref(_dense_columns(A), apply, b[:, None], 30, tol)
            assert X.shape == (n, 1) and H.shape == (31, 1)
            assert X[:, 0].tobytes() == x_ref.tobytes() and H[:, 0].tobytes() == h_ref.tobytes()
            assert {k: int(v[0]) for k, v in info.items()} == info_ref
    # and in the three small systems of the one-wide test that stop early
    for A, b in (([[0.0, 1.0], [1.0, 0.0]], [1.0, 0.0]), ([[-1.0, 0.0, 2.0], [-1.0, -1.0, 2.0], [0.0, 0.0, 1.0]], [0.0, 1.0, 1.0]),
                 ([[4.0, 1.0], [0.0, 3.0]], [1.0, 0.0])):
        A, b = np.asarray(A), np.asarray(b)
        x_ref, h_ref, info_ref = bicgstab_ref(lambda v: A @ v, b, 6, tol)
        X, H, info = bicgstab_multi_ref(_dense_columns(A), None, b[:, None], 6, tol)
        assert X[:, 0].tobytes() == x_ref.tobytes() and H[:, 0].tobytes() == h_ref.tobytes()
        assert {k: int(v[0]) for k, v in info.items()} == info_ref


@pytest.mark.parametrize("tol", [0.0, FATES_TOL])
def test_the_fates_case_gives_the_listed_fates_on_the_cpu(tol):
    A, B = fates_case()
    X, H, info = bicgstab_multi_ref(_dense_columns(A), None, B, FATES_ITERS, tol)
    steps, status, half = fates_expected(tol)
    assert info["steps"].tolist() == steps and info["status"].tolist() == status and info["half_step"].tolist() == half
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(H))
    # every column is its own bicgstab_ref run, bit for bit: nothing crosses between columns
    for j in range(B.shape[1]):
        x_ref, h_ref, info_ref = bicgstab_ref(lambda v: A @ v, B[:, j].copy(), FATES_ITERS, tol)
        assert X[:, j].tobytes() == x_ref.tobytes() and H[:, j].tobytes() == h_ref.tobytes(), j
        assert (steps[j], status[j], half[j]) == (info_ref["steps"], info_ref["status"], info_ref["half_step"]), j
    # 8 times the right-hand side: 8 times x and 64 times the history, exactly
    assert np.array_equal(X[:, 5], 8.0 * X[:, 3]) and np.array_equal(H[:, 5], 64.0 * H[:, 3])
    # the restated loop scales exactly by powers of two with an apply as well
    dinv = 1.0 / np.diag(A + np.eye(len(A)) * (np.diag(A) == 0))
    jacobi = lambda R: dinv[:, None] * R  # noqa: E731
    Xp, Hp, infop = bicgstab_multi_ref(_dense_columns(A), jacobi, B[:, [3, 5]], FATES_ITERS, tol)
    assert np.array_equal(Xp[:, 1], 8.0 * Xp[:, 0]) and np.array_equal(Hp[:, 1], 64.0 * Hp[:, 0])
    assert infop["steps"][0] == infop["steps"][1]
