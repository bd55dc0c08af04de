"""MINRES for k right-hand sides without a GPU: the solver is exported, listed in the version script, declared and
bound, the Python method checks its input before any device call, and the restated loop (tests/_minres_multi_ref.py) is
minres_ref at k = 1 bit for bit and gives the known answers: a diagonal matrix in as many steps as it has distinct
eigenvalues, an eigenvector in one, b_j = 0 in none, a 2 x 2 indefinite matrix in two, a shift per column as the plain
loop on A - shift_j I, and scipy's minres on an SPD band."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _minres_multi_ref import columns_product, minres_multi_ref
from conftest import ROOT
from test_gpu_minres import minres_ref, spd_banded
from test_pcg_multi_host import BAD_ARRAYS, _handle_without_device, _precond_without_device

NAME = "spmv_hip_csr_minres_multi"


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
    assert list(solve.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, double_p, int_p, C.c_void_p,
                                    C.c_void_p, double_p, int_p, int_p, C.POINTER(C.c_float)]


@pytest.mark.parametrize("what", sorted(BAD_ARRAYS))
def test_minres_multi_rejects_a_bad_B_before_any_device_call(what):
    with pytest.raises(ValueError):
        _handle_without_device().minres_multi(BAD_ARRAYS[what], 3)


def test_minres_multi_rejects_bad_iters_tol_shifts_and_preconditioners_before_any_device_call():
    dev = _handle_without_device()
    B = np.zeros((6, 2))
    with pytest.raises(ValueError):
        dev.minres_multi(B, -1)
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.minres_multi(B, 3, tol=tol)
    for shift in (float("nan"), float("inf"), [0.0, float("nan")], [0.0], [0.0, 1.0, 2.0], [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            dev.minres_multi(B, 3, shift=shift)
    for P in ("jacobi", _precond_without_device(rows=5), _precond_without_device(row0=1),
              _precond_without_device(dtype=np.float32)):
        with pytest.raises(ValueError):
            dev.minres_multi(B, 3, precond=P)


def test_the_entry_point_refuses_null_arguments():
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present; the no-device behaviour is checked on CPU hosts")
    buf = (C.c_double * 8)()
    words = (C.c_int * 4)()
    ms = C.c_float(0)
    solve = getattr(sp.lib(), NAME)
    assert solve(None, None, 2, 3, 0.0, None, None, buf, buf, buf, words, words, C.byref(ms)) == -1


# ---------------------------------------------------------------- the restated loop on cases with known answers
def dense(A):
    A = np.asarray(A, dtype=np.float64)
    return columns_product(lambda u: A @ u)


@pytest.mark.parametrize("tol", [0.0, 1e-9])
def test_the_restated_loop_with_k1_is_minres_ref_bit_for_bit(tol):
    rng = np.random.default_rng(41)
    n = 60
    A = rng.uniform(-1, 1, (n, n)) * (rng.uniform(0, 1, (n, n)) < 0.1)
    A = A + A.T + np.diag(3.0 * rng.choice([-1.0, 1.0], n))
    inv = 1.0 / np.abs(np.diag(A))
    for b in (rng.uniform(-1, 1, n), np.zeros(n)):
        for shift in (0.0, 0.3):
            for minv1, minvk in ((None, None), (lambda r: r * inv, lambda R: R * inv[:, None])):
                x_ref, h_ref, info_ref = minres_ref(lambda u: A @ u, b, 40, tol, shift=shift, minv=minv1)
                X, H, info = minres_multi_ref(dense(A), b[:, None], 40, tol, shift=shift, minv=minvk)
                assert X.shape == (n, 1) and H.shape == (41, 1)
                assert X[:, 0].tobytes() == x_ref.tobytes() and H[:, 0].tobytes() == h_ref.tobytes()
                assert {key: int(val[0]) for key, val in info.items()} == info_ref


def test_a_diagonal_matrix_is_solved_in_as_many_steps_as_it_has_distinct_eigenvalues():
    d = np.tile([2.0, -1.0, 0.5, -4.0], 6)
    n = len(d)
    rng = np.random.default_rng(42)
    B = rng.uniform(-1, 1, (n, 3))
    B[:, 1] = np.where(np.isin(d, (2.0, -1.0)), B[:, 1], 0.0)       # two of the four eigenspaces
    B[:, 2] = np.where(d == 0.5, B[:, 2], 0.0)                      # an eigenvector: one
    X, H, info = minres_multi_ref(dense(np.diag(d)), B, 6, tol=1e-12)
    assert info["steps"].tolist() == [4, 2, 1] and info["status"].tolist() == [sp.MINRES_CONVERGED] * 3
    assert np.max(np.abs(X - B / d[:, None])) <= 1e-13
    assert np.all(np.diff(H, axis=0) <= 0.0) and np.all(H[-1] <= 1e-24 * H[0])
    # the history repeats after a column's stop
    assert np.all(H[2:, 1] == H[2, 1]) and np.all(H[1:, 2] == H[1, 2])


@pytest.mark.parametrize("tol", [0.0, 1e-6])
def test_an_eigenvector_converges_at_step_1_and_a_zero_column_at_step_0(tol):
    d = np.array([2.0, -1.0, 0.5, -4.0, 8.0])
    B = np.zeros((5, 4))
    B[3, 0] = -0.5                       # an eigenvector whose every operation is exact
    B[:, 2] = [1.0, 1.0, 1.0, 1.0, 1.0]  # an ordinary column
    B[1, 3] = 4.0
    X, H, info = minres_multi_ref(dense(np.diag(d)), B, 3, tol)
    assert info["steps"].tolist()[:2] == [1, 0] and info["steps"][3] == 1
    assert info["status"].tolist()[:2] == [sp.MINRES_CONVERGED] * 2 and info["status"][3] == sp.MINRES_CONVERGED
    assert H[1:, 0].tolist() == [0.0] * 3 and H[:, 1].tolist() == [0.0] * 4 and H[1:, 3].tolist() == [0.0] * 3
    assert X[:, 0].tolist() == [0.0, 0.0, 0.0, 0.125, 0.0] and X[:, 1].tolist() == [0.0] * 5
    assert X[:, 3].tolist() == [0.0, -4.0, 0.0, 0.0, 0.0]
    assert info["steps"][2] == 3 and H[3, 2] < H[0, 2]


def test_a_two_by_two_indefinite_matrix():
    A = np.array([[0.0, 1.0], [1.0, 0.0]])                # eigenvalues +-1
    B = np.array([[1.0, 3.0], [0.0, 4.0]])
    X, H, info = minres_multi_ref(dense(A), B, 4)
    # b = e_1: alfa = 0 at both steps, the first step leaves x = 0 and the residual where it was, the second solves
    assert H[:, 0].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0] and X[:, 0].tolist() == [0.0, 1.0]
    assert (info["steps"][0], info["status"][0]) == (2, sp.MINRES_CONVERGED)
    assert np.max(np.abs(X[:, 1] - np.array([4.0, 3.0]))) <= 1e-14 and H[2, 1] <= 1e-28 * H[0, 1]
    # a shift that makes A - shift I singular on the Krylov space: A - I has the null vector (1, 1); b = (1, -1) is an
    # eigenvector for -2
    X, H, info = minres_multi_ref(dense(A), np.array([[1.0], [-1.0]]), 3, tol=1e-12, shift=1.0)
    assert np.max(np.abs(X[:, 0] - np.array([-0.5, 0.5]))) <= 1e-15
    assert (info["steps"][0], info["status"][0]) == (1, sp.MINRES_CONVERGED)


def test_a_shift_per_column_is_the_plain_loop_on_the_shifted_matrix():
    rng = np.random.default_rng(43)
    n, k = 50, 4
    A = rng.uniform(-1, 1, (n, n)) * (rng.uniform(0, 1, (n, n)) < 0.15)
    A = A + A.T + np.diag(4.0 * rng.choice([-1.0, 1.0], n))
    B = rng.uniform(-1, 1, (n, k))
    shifts = np.array([0.0, 0.3, -0.2, 1.5])
    X, H, info = minres_multi_ref(dense(A), B, 8, shift=shifts)
    for j in range(k):
        As = A - shifts[j] * np.eye(n)
        x, h, info_j = minres_ref(lambda u: As @ u, B[:, j].copy(), 8)
        assert (info["steps"][j], info["status"][j]) == (info_j["steps"], info_j["status"])
        # A v - shift v against (A - shift I) v: a rounding per entry and step, amplified by a few steps of Lanczos
        assert np.max(np.abs(X[:, j] - x)) <= 1e-12 * np.max(np.abs(x)), j
        assert np.max(np.abs(H[:, j] - h)) <= 1e-12 * h[0], j
    # a scalar shift is that shift for every column
    Xs, Hs, _ = minres_multi_ref(dense(A), B, 8, shift=0.3)
    X3, H3, _ = minres_multi_ref(dense(A), B, 8, shift=[0.3] * k)
    assert Xs.tobytes() == X3.tobytes() and Hs.tobytes() == H3.tobytes()
    assert Xs[:, 1].tobytes() == X[:, 1].tobytes()


def test_the_restated_loop_agrees_with_scipy_on_an_spd_band():
    import scipy.sparse as sps
    from scipy.sparse.linalg import minres as scipy_minres
    n, k = 400, 3
    rng = np.random.default_rng(44)
    rp, col, val = spd_banded(rng, n, 5, 12)
    a = sps.csr_matrix((val, col, rp), shape=(n, n))
    B = rng.uniform(-1, 1, (n, k))
    shifts = np.array([0.0, 0.25, -0.5])
    X, H, info = minres_multi_ref(columns_product(lambda u: a @ u), B, 300, tol=1e-12, shift=shifts)
    assert info["status"].tolist() == [sp.MINRES_CONVERGED] * k
    for j in range(k):
        try:
            xs, _ = scipy_minres(a, B[:, j], rtol=1e-12, maxiter=300, shift=shifts[j])
        except TypeError:                                   # an older scipy spells it tol
            xs, _ = scipy_minres(a, B[:, j], tol=1e-12, maxiter=300, shift=shifts[j])
        assert np.max(np.abs(xs - X[:, j])) <= 1e-9 * np.max(np.abs(xs)), j
        r = B[:, j] - (a @ X[:, j] - shifts[j] * X[:, j])
        assert float(r @ r) <= 4.0 * H[-1, j] + 1e-24 * H[0, j]


def test_a_stopped_column_still_rides_and_keeps_its_vectors():
    """the products and applies see every column at every step; a NaN column stays a breakdown at step 0 with x = 0 and
    changes no other column's bits"""
    rng = np.random.default_rng(45)
    n = 30
    A = rng.uniform(-1, 1, (n, n))
    A = A + A.T
    B = rng.uniform(-1, 1, (n, 4))
    B[:, 1] = 0.0
    bad = B.copy()
    bad[7, 1] = np.nan
    widths = []
    spmm = lambda V: (widths.append(V.shape[1]), dense(A)(V))[1]  # noqa: E731
    X0, H0, info0 = minres_multi_ref(spmm, B, 6)
    X1, H1, info1 = minres_multi_ref(dense(A), bad, 6)
    assert widths == [4] * 6
    assert (info0["steps"][1], info0["status"][1]) == (0, sp.MINRES_CONVERGED)
    assert (info1["steps"][1], info1["status"][1]) == (0, sp.MINRES_BREAKDOWN)
    assert np.all(X1[:, 1] == 0.0) and np.all(np.isnan(H1[:, 1]))
    others = [0, 2, 3]
    assert X0[:, others].tobytes() == X1[:, others].tobytes() and H0[:, others].tobytes() == H1[:, others].tobytes()
    # M = D^-1 of an indefinite diagonal: r.M^-1 r < 0 is a breakdown at step 0
    d = np.where(np.arange(n) % 2 == 0, 1.0, -3.0)
    Xn, Hn, infon = minres_multi_ref(dense(np.diag(d)), np.ones((n, 2)), 4, minv=lambda R: R / d[:, None])
    assert infon["steps"].tolist() == [0, 0] and infon["status"].tolist() == [sp.MINRES_BREAKDOWN] * 2
    assert np.all(Xn == 0.0)
