"""spmv_hip_csr_minres_multi on the GPU: k independent MINRES recurrences with a shift per column that share one SpMM a
step, against the restated loop (tests/_minres_multi_ref.py, pinned by tests/test_minres_multi_host.py) and against
minres column by column; the lane shapes and grid edges; the bit identities the fixed reduction order promises; every
fate in one call; a NaN or Inf that stays in its column; the per-column stop; a KKT matrix; refused calls.

Lanczos amplifies rounding differences exponentially, so x and the history are compared entry by entry only after a few
steps (5 on the banded matrices, 1 to 3 at the edge sizes); longer runs are held to properties, as in test_gpu_minres.py.

The pointwise tolerances follow test_gpu_minres.py: 16 times the restated loop's own rounding, and at least 4 eps of
the dtype.  That rounding is measured on the CPU by `python tests/test_gpu_minres_multi.py`: the largest difference over
the columns (x relative to its column's max |x|, history entries relative to the column's first) between the restated
loop as the handle computes it (fp64: over oracle.csr_serial; fp32: values, B and every stored vector rounded to fp32,
dots in fp64) and the same loop, unrounded, over a long-double product.  The preconditioners of the measurement are the CPU
restatements the other tests pin (1 / |d|, numpy inverses of the 3 x 3 blocks, fsai_ref, _amg_ref.cycle,
_cheb_ref.apply); on the device the restated loop runs over the preconditioner's own k-wide apply.

    case (k = 4, 5 steps, shifts 0, 0.3, -0.2, 0)        measured     tolerance
    banded n = 6000, no M, fp64                          2.448e-15    3.917e-14
    banded n = 6000, no M, fp32                          2.963e-07    4.741e-06
    banded n = 6000, Jacobi of |diag|, fp64              4.658e-16    7.453e-15
    banded n = 6000, Jacobi of |diag|, fp32              1.845e-07    2.952e-06
    banded n = 6000, block-Jacobi(3) of |diag|, fp64     6.885e-16    1.102e-14
    banded n = 6000, block-Jacobi(3) of |diag|, fp32     2.050e-07    3.280e-06
    SPD band n = 2000, FSAI, fp64                        5.943e-16    9.509e-15
    SPD band n = 2000, FSAI, fp32                        2.572e-07    4.115e-06
    SPD band n = 2000, AMG, fp64                         5.942e-16    9.507e-15
    SPD band n = 2000, AMG, fp32                         2.429e-07    3.886e-06
    SPD band n = 2000, Chebyshev degree 4, fp64          1.142e-15    1.827e-14
    SPD band n = 2000, Chebyshev degree 4, fp32          2.681e-07    4.290e-06
    tridiagonal, every size and k, 1 to 3 steps, fp64    4.255e-14    6.808e-13   (n = 257, k = 64, 1 steps)
    tridiagonal, every size and k, 1 to 3 steps, fp32    1.600e-05    2.560e-04   (n = 3, k = 64, 1 steps)
The edge-size maxima are large for one step because x_1 is proportional to alfa = v.A v, a sum that nearly cancels on
a matrix whose diagonal signs alternate; the restated loop itself is no more exact than that there.

(A tiles-only handle exists only inside an HLL handle and cannot be reached from Python: that refusal of the C entry
point has no test here, as in test_gpu_bicgstab_multi.py.  n * k beyond int range needs a handle of more than 33
million rows: its refusal is a line before any allocation and has no test here either.)"""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from _minres_multi_ref import columns_product, minres_multi_ref
from test_gpu_bicgstab_multi import precond_of, rows_per_workgroup
from test_gpu_minres import (KKT_FACTOR, KKT_STEPS, LD, N, alternating_tridiagonal, banded_problem, diagonal_positions,
                             kkt_problem, product, spd_banded, to_csr, true_rr, with_abs_diagonal)

pytestmark = pytest.mark.gpu

K_MCG_BLOCKS = 2048    # cg_multi_kernels.hpp
DTYPES = [np.float64, np.float32]
SHIFTS = np.array([0.0, 0.3, -0.2, 0.0])
STEPS = 5
N_SPD = 2000
ALL_KINDS = ["none", "jacobi", "block3", "fsai", "amg", "cheb4_default"]   # of test_gpu_bicgstab_multi.KINDS

# Measured on the CPU (`python tests/test_gpu_minres_multi.py`): the restated loop's own rounding per case, see the
# module docstring; the tolerance is 16 times it and at least 4 eps.
MEASURED = {
    ("banded", "none", "float64"): 2.448e-15,   # x 2.448e-15, history 8.955e-17
    ("banded", "none", "float32"): 2.963e-07,   # x 2.963e-07, history 9.531e-09
    ("banded", "jacobi", "float64"): 4.658e-16,   # x 4.658e-16, history 6.240e-17
    ("banded", "jacobi", "float32"): 1.845e-07,   # x 1.845e-07, history 1.884e-09
    ("banded", "block3", "float64"): 6.885e-16,   # x 6.885e-16, history 6.365e-17
    ("banded", "block3", "float32"): 2.050e-07,   # x 2.050e-07, history 2.213e-09
    ("spd", "fsai", "float64"): 5.943e-16,   # x 5.943e-16, history 4.349e-22
    ("spd", "fsai", "float32"): 2.572e-07,   # x 2.572e-07, history 3.721e-09
    ("spd", "amg", "float64"): 5.942e-16,   # x 5.942e-16, history 4.155e-18
    ("spd", "amg", "float32"): 2.429e-07,   # x 2.429e-07, history 3.384e-09
    ("spd", "cheb4_default", "float64"): 1.142e-15,   # x 1.142e-15, history 3.410e-17
    ("spd", "cheb4_default", "float32"): 2.681e-07,   # x 2.681e-07, history 3.614e-09
    ("sizes", "float64"): 4.255e-14,   # n = 257, k = 64, 1 steps, x 4.255e-14, history 3.587e-16
    ("sizes", "float32"): 1.600e-05,   # n = 3, k = 64, 1 steps, x 1.600e-05, history 5.086e-08
}


def tolerance(matrix, kind, dtype):
    return max(16.0 * MEASURED[matrix, kind, np.dtype(dtype).name], 4.0 * float(np.finfo(dtype).eps))


def sizes_tolerance(dtype):
    return max(16.0 * MEASURED["sizes", np.dtype(dtype).name], 4.0 * float(np.finfo(dtype).eps))


def rd_of(dtype):
    return lambda u: np.asarray(u).astype(dtype).astype(np.float64)


def device_apply(P, dtype):
    """the restated loop's M^-1: the preconditioner's own k-wide apply on arrays rounded to the handle's dtype"""
    return lambda R: P.apply_multi(np.ascontiguousarray(np.asarray(R).astype(dtype))).astype(np.float64)


def differences(X, H, X_ref, H_ref):
    """(max over the columns of max |x - x_ref| / max |x_ref|, of max |h - h_ref| / h_ref[0]) in long double"""
    dx = dh = 0.0
    for j in range(X_ref.shape[1]):
        x_ref, h_ref = np.asarray(X_ref[:, j]).astype(LD), np.asarray(H_ref[:, j]).astype(LD)
        scale = np.max(np.abs(x_ref))
        if scale > 0:
            dx = max(dx, float(np.max(np.abs(np.asarray(X[:, j]).astype(LD) - x_ref)) / scale))
        if h_ref[0] > 0:
            dh = max(dh, float(np.max(np.abs(np.asarray(H[:, j]).astype(LD) - h_ref)) / h_ref[0]))
    return dx, dh


def check_pointwise(got, ref, tol, what, with_info=True):
    X, H, info = got
    X_ref, H_ref, info_ref = ref
    if with_info:
        for key in ("steps", "status"):
            assert np.array_equal(info[key], info_ref[key]), (what, key, info, info_ref)
    dx, dh = differences(X, H, X_ref, H_ref)
    print(f"{what}: x {dx:.3e} hist {dh:.3e} (tolerance {tol:.3e})")
    assert dx <= tol and dh <= tol, (what, dx, dh, tol)


def same_run(one, two):
    return (one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
            and all(np.array_equal(one[2][key], two[2][key]) for key in ("steps", "status")))


def banded_columns(oracle, k=4):
    """(row_ptr, col, val, B): the banded indefinite matrix of test_gpu_minres.py (seed 909, n = 6000); columns 0 and 1
    are its right-hand side b, the rest are products with further random vectors"""
    row_ptr, col, val, _, b = banded_problem(oracle)
    rng = np.random.default_rng(910)
    cols = [b, b] + [oracle.csr_serial(row_ptr, col, val, rng.uniform(-1, 1, N)) for _ in range(k - 2)]
    return row_ptr, col, val, np.ascontiguousarray(np.stack(cols[:k], axis=1))


def spd_columns(oracle, k=4):
    rng = np.random.default_rng(31)
    row_ptr, col, val = spd_banded(rng, N_SPD, 5, 40)
    B = np.stack([oracle.csr_serial(row_ptr, col, val, rng.uniform(-1, 1, N_SPD)) for _ in range(k)], axis=1)
    return row_ptr, col, val, np.ascontiguousarray(B)


@pytest.fixture(scope="module")
def banded(oracle):
    return banded_columns(oracle)


@pytest.fixture(scope="module")
def spd(oracle):
    return spd_columns(oracle)


# ---------------------------------------------------------------- 1. against the restated loop, column by column
def check_against_the_loop_and_minres(oracle, problem, n, kind, dtype, matrix, val_of_precond=None):
    row_ptr, col, val, B64 = problem
    rd = rd_of(dtype)
    B = np.ascontiguousarray(B64.astype(dtype))
    vals = val.astype(dtype)
    serial = columns_product(lambda u: oracle.csr_serial(row_ptr, col, vals.astype(np.float64), u))
    tol = tolerance(matrix, kind, dtype)
    what = f"{matrix} {kind} {np.dtype(dtype).name}"
    pval = vals if val_of_precond is None else val_of_precond.astype(dtype)
    with sp.CsrDevice(n, n, row_ptr, col, vals) as dev, sp.CsrDevice(n, n, row_ptr, col, pval) as dev_p:
        with precond_of(dev_p, kind) as P:
            X, H, info, ms = dev.minres_multi(B, STEPS, shift=SHIFTS, precond=P)
            assert X.shape == (n, 4) and X.dtype == dtype and H.shape == (STEPS + 1, 4) and ms > 0
            assert info["steps"].tolist() == [STEPS] * 4 and info["status"].tolist() == [sp.MINRES_RAN_ALL] * 4
            minv = None if P is None else device_apply(P, dtype)
            ref = minres_multi_ref(serial, B.astype(np.float64), STEPS, shift=SHIFTS, minv=minv, rd=rd)
            check_pointwise((X, H, info), ref, tol, what + " vs the restated loop")
            one = [dev.minres(np.ascontiguousarray(B[:, j]), STEPS, shift=float(SHIFTS[j]), precond=P) for j in range(4)]
            assert all(o[2] == {"steps": STEPS, "status": sp.MINRES_RAN_ALL} for o in one)
            X_one = np.stack([o[0] for o in one], axis=1)
            H_one = np.stack([o[1] for o in one], axis=1)
            check_pointwise((X, H, info), (X_one, H_one, None), tol, what + " vs minres", with_info=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["none", "jacobi", "block3"])
def test_matches_the_restated_loop_and_minres_on_the_indefinite_band(gpu, oracle, banded, kind, dtype):
    """k = 4, 5 steps, shifts (0, 0.3, -0.2, 0); Jacobi and block-Jacobi(3) are those of the copy with |diagonal|"""
    row_ptr, col, val, _ = banded
    check_against_the_loop_and_minres(oracle, banded, N, kind, dtype, "banded",
                                      val_of_precond=None if kind == "none" else with_abs_diagonal(row_ptr, col, val))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["fsai", "amg", "cheb4_default"])
def test_matches_the_restated_loop_and_minres_on_an_spd_band(gpu, oracle, spd, kind, dtype):
    check_against_the_loop_and_minres(oracle, spd, N_SPD, kind, dtype, "spd")


# ---------------------------------------------------------------- 2. lane shapes and row edges
def sizes_columns(n, k, dtype):
    rp, col, val = alternating_tridiagonal(n)
    B = np.random.default_rng([n, k, 12]).uniform(-1, 1, (n, k)).astype(dtype)
    return rp, col, val.astype(dtype), np.ascontiguousarray(B)


def sizes_shifts(k):
    return 0.125 * (np.arange(k) % 3 - 1)


LANE_CASES = [(np.float64, k) for k in (1, 2, 3, 6, 8, 63, 64)] + [(np.float32, k) for k in (1, 4, 5, 64)]
LANE_SIZES = (1, 2, 3, 5, 63, 64, 65, 257, 1025)


def check_steps_at_a_size(n, k, dtype, steps=(1, 2, 3)):
    """against the restated loop over a long-double product, as test_gpu_minres.py does at these sizes.  x and the
    history are compared, not the status: where the Krylov space is exhausted (n <= 3) the last residual is 0 in one
    order of rounding and 1e-33 in another, and tol = 0 converges only at exactly 0."""
    rp, col, val, B = sizes_columns(n, k, dtype)
    A = columns_product(product(rp, col, val))
    shifts = sizes_shifts(k)
    tol = sizes_tolerance(dtype)
    with sp.CsrDevice(n, n, rp, col, val) as dev:
        for iters in steps:
            X, H, info, _ = dev.minres_multi(B, iters, shift=shifts)
            assert X.dtype == dtype and X.shape == (n, k) and H.shape == (iters + 1, k)
            ref = minres_multi_ref(A, B, iters, shift=shifts)
            check_pointwise((X, H, info), ref, tol, f"n={n} k={k} {np.dtype(dtype).name} {iters} steps", with_info=False)
            assert np.all((info["steps"] == iters) | (info["status"] == sp.MINRES_CONVERGED)), info


@pytest.mark.parametrize("dtype,k", LANE_CASES)
def test_lane_shapes_and_row_edges(gpu, dtype, k):
    """V = 2 (fp64, even k) and 4 (fp32, k a multiple of 4), V = 1, idle column lanes (k / V no power of two) and the
    widest k; n from 1 to past a workgroup's pass"""
    for n in LANE_SIZES:
        check_steps_at_a_size(n, k, dtype)


@pytest.mark.parametrize("k,groups,extra", [(64, 128, 1), (63, 91, -1)])
def test_grid_stride_at_many_workgroups(gpu, k, groups, extra):
    """fp64; k = 64 is 32 column lanes and kBlock >> 5 rows per workgroup: one row more than 128 workgroups' worth.
    k = 63 is single elements, 64 column lanes and kBlock >> 6 rows per workgroup: 91 workgroups' worth minus one."""
    n = groups * rows_per_workgroup(k, np.float64) + extra
    check_steps_at_a_size(n, k, np.float64, steps=(2,))


def test_grid_stride_past_the_workgroup_cap(gpu):
    """k = 64, fp64: the cap of kMcgBlocks workgroups is reached at 2048 x 8 rows; three rows more and some lanes take a
    second row"""
    n = K_MCG_BLOCKS * rows_per_workgroup(64, np.float64) + 3
    check_steps_at_a_size(n, 64, np.float64, steps=(2,))


# ---------------------------------------------------------------- 3. bit identities
def identity_problem(kind, banded, spd):
    """the matrix a kind is symmetric positive definite on, six columns (2 = 0, 3 = 2^7 x 1) and their shifts"""
    row_ptr, col, val, B_all = spd if kind in ("fsai", "amg", "cheb4_default") else banded
    n = len(row_ptr) - 1
    rng = np.random.default_rng(77)
    B = np.ascontiguousarray(np.concatenate([B_all, rng.uniform(-1, 1, (n, 2))], axis=1))
    B[:, 2] = B[:, 0]
    B[:, 3] = 2.0 ** 7 * B[:, 1]
    shifts = np.array([0.0, 0.3, 0.0, 0.3, -0.2, 0.1])
    pval = val if kind in ("none", "fsai", "amg", "cheb4_default") else with_abs_diagonal(row_ptr, col, val)
    return n, row_ptr, col, val, pval, B, shifts


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_bit_identities(gpu, banded, spd, kind):
    """Two calls give the same bytes; permuting B's columns with the shifts permutes everything; equal columns with
    equal shifts give equal bytes; (none, Jacobi, block-Jacobi, FSAI: every operation is a product, a sum, a quotient or
    a square root of an even power, in which a power of two moves through exactly) a column 2^7 times another gives 2^7
    times its x and 4^7 times its history; a single-rank communicator changes nothing; an `iters` 50 times larger
    changes nothing after every column has stopped."""
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    n, row_ptr, col, val, pval, B, shifts = identity_problem(kind, banded, spd)
    perm = np.array([4, 0, 5, 2, 1, 3])
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev, sp.CsrDevice(n, n, row_ptr, col, pval) as dev_p, \
            precond_of(dev_p, kind) as P:
        for iters, tol in ((8, 0.0), (400, 1e-4)):
            run = dev.minres_multi(B, iters, tol=tol, shift=shifts, precond=P)
            assert same_run(run, dev.minres_multi(B, iters, tol=tol, shift=shifts, precond=P)), (kind, tol)
            X, H, info, _ = run
            Xp, Hp, infop, _ = dev.minres_multi(np.ascontiguousarray(B[:, perm]), iters, tol=tol, shift=shifts[perm],
                                                precond=P)
            assert Xp.tobytes() == np.ascontiguousarray(X[:, perm]).tobytes(), (kind, tol)
            assert Hp.tobytes() == np.ascontiguousarray(H[:, perm]).tobytes(), (kind, tol)
            for key in ("steps", "status"):
                assert np.array_equal(infop[key], info[key][perm]), (kind, tol, key)
            assert np.array_equal(X[:, 2], X[:, 0]) and np.array_equal(H[:, 2], H[:, 0]), (kind, tol)
            assert all(info[key][2] == info[key][0] for key in info)
            if kind in ("none", "jacobi", "block3", "fsai"):
                assert np.array_equal(X[:, 3], 2.0 ** 7 * X[:, 1]), (kind, tol)
                assert np.array_equal(H[:, 3], 4.0 ** 7 * H[:, 1]), (kind, tol)
                assert all(info[key][3] == info[key][1] for key in info)
            comm = NativeComm(0, 1, lambda ident: ident)
            try:
                again = dev.minres_multi(B, iters, tol=tol, shift=shifts, precond=P, bounds=np.array([0, n], np.int32))
                assert same_run(run, again), (kind, tol)
            finally:
                comm.close()
            if tol > 0:
                assert np.all(info["status"] == sp.MINRES_CONVERGED) and info["steps"].max() < iters, (kind, info)
                big = dev.minres_multi(B, 50 * iters, tol=tol, shift=shifts, precond=P)
                assert big[0].tobytes() == X.tobytes() and big[1][: iters + 1].tobytes() == H.tobytes()
                assert np.all(big[1][iters:] == H[-1]) and all(np.array_equal(big[2][key], info[key]) for key in info)


# ---------------------------------------------------------------- 4. every fate in one call
def fates_case():
    """(row_ptr, col, val, B): a decoupled 1 x 1 block [[-4]] above the alternating tridiagonal matrix of 40 rows.
    Columns: zeros; e_0 / 2, an eigenvector whose every operation is exact; an ordinary column; one with a NaN; one
    with an Inf."""
    import scipy.sparse as sps
    rp, col, val = alternating_tridiagonal(40)
    a = sps.block_diag([sps.csr_matrix([[-4.0]]), sps.csr_matrix((val, col, rp), shape=(40, 40))]).tocsr()
    n = 41
    rng = np.random.default_rng(4)
    B = np.zeros((n, 5))
    B[0, 1] = 0.5
    B[1:, 2] = rng.uniform(-1, 1, 40)
    B[1:, 3] = rng.uniform(-1, 1, 40)
    B[1:, 4] = rng.uniform(-1, 1, 40)
    B[a.diagonal() < 0.0, 2] *= 4.0      # r.D^-1 r < 0 for this column, whatever the draw
    B[17, 3] = np.nan
    B[23, 4] = np.inf
    return n, *to_csr(a), B


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_every_fate_in_one_call(gpu, dtype):
    n, rp, col, val, B = fates_case()
    B = B.astype(dtype)
    B_zeroed = B.copy()
    B_zeroed[:, 3:] = 0.0
    iters = 6
    conv, ran, broke = sp.MINRES_CONVERGED, sp.MINRES_RAN_ALL, sp.MINRES_BREAKDOWN
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev:
        for tol in (0.0, 1e-30):
            X, H, info, _ = dev.minres_multi(B, iters, tol=tol)
            assert info["steps"].tolist() == [0, 1, iters, 0, 0], (tol, info)
            assert info["status"].tolist() == [conv, conv, ran, broke, broke], (tol, info)
            assert not np.any(np.isnan(X)) and np.all(X[:, [0, 3, 4]] == 0.0)
            assert np.all(H[:, 0] == 0.0) and H[0, 1] == 0.25 and np.all(H[1:, 1] == 0.0)
            assert X[0, 1] == dtype(-0.125) and np.all(X[1:, 1] == 0.0)
            assert np.all(np.diff(H[:, 2]) <= 0.0) and H[-1, 2] < H[0, 2]
            assert not np.any(np.isfinite(H[:, 3])) and not np.any(np.isfinite(H[:, 4]))
            clean = dev.minres_multi(B_zeroed, iters, tol=tol)
            assert clean[2]["steps"].tolist() == [0, 1, iters, 0, 0]
            assert clean[2]["status"].tolist() == [conv, conv, ran, conv, conv]
            assert np.ascontiguousarray(X[:, :3]).tobytes() == np.ascontiguousarray(clean[0][:, :3]).tobytes(), tol
            assert np.ascontiguousarray(H[:, :3]).tobytes() == np.ascontiguousarray(clean[1][:, :3]).tobytes(), tol
        # Jacobi of the indefinite matrix itself has entries of both signs: r.M^-1 r < 0 (columns 1 and 2) or not
        # finite (3 and 4) refuses it at step 0
        with dev.preconditioner("jacobi") as bad:
            X, H, info, _ = dev.minres_multi(B, iters, precond=bad)
            assert H[0, 1] < 0.0 and H[0, 2] < 0.0, H[0]
            assert info["steps"].tolist() == [0] * 5 and info["status"].tolist() == [conv] + [broke] * 4, info
            assert np.all(X == 0.0)


@pytest.mark.parametrize("kind", ["none", "jacobi", "amg", "cheb4_default"])
def test_a_nan_or_inf_in_one_column_of_B_stays_in_that_column(gpu, banded, spd, kind):
    """Column j breaks down at step 0 with x_j = 0; every other column's outputs are, byte for byte, those of the same
    call with column j of B set to zeros."""
    n, row_ptr, col, val, pval, B_all, shifts = identity_problem(kind, banded, spd)
    k, j = 5, 2
    B = np.ascontiguousarray(B_all[:, :k])
    B[:, j] = B_all[:, 5]
    B_zero = B.copy()
    B_zero[:, j] = 0.0
    others = [c for c in range(k) if c != j]
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev, sp.CsrDevice(n, n, row_ptr, col, pval) as dev_p, \
            precond_of(dev_p, kind) as P:
        X0, H0, info0, _ = dev.minres_multi(B_zero, 5, shift=shifts[:k], precond=P)
        assert info0["steps"][j] == 0 and info0["status"][j] == sp.MINRES_CONVERGED
        for poison in (np.nan, np.inf):
            B_bad = B.copy()
            B_bad[1234, j] = poison
            X, H, info, _ = dev.minres_multi(B_bad, 5, shift=shifts[:k], precond=P)
            assert info["status"][j] == sp.MINRES_BREAKDOWN and info["steps"][j] == 0, (kind, poison, info)
            assert np.all(X[:, j] == 0.0), (kind, poison)
            assert np.ascontiguousarray(X[:, others]).tobytes() == np.ascontiguousarray(X0[:, others]).tobytes(), (kind, poison)
            assert np.ascontiguousarray(H[:, others]).tobytes() == np.ascontiguousarray(H0[:, others]).tobytes(), (kind, poison)
            for key in ("steps", "status"):
                assert np.array_equal(info[key][others], info0[key][others]), (kind, poison, key)


# ---------------------------------------------------------------- 5. columns stop on their own
REF_STEPS = (251, 284, 251)   # the CPU reference to tol = 1e-10: module docstring of test_gpu_minres.py


def test_columns_stop_on_their_own_and_the_loop_ends_early(gpu, oracle, banded):
    """tol = 1e-10, shifts (0, 0.3, 0), column 2 = 2^-3 x column 0: each column's step count is within 2 of the CPU
    reference's, every status is CONVERGED, the loop ends before its budget, no history ever grows, and the true
    residual meets the recorded one by the line of test_minres_converges_where_cg_breaks_down."""
    row_ptr, col, val, B_all = banded
    B = np.ascontiguousarray(np.stack([B_all[:, 0], B_all[:, 1], 0.125 * B_all[:, 0]], axis=1))
    shifts = np.array([0.0, 0.3, 0.0])
    iters, tol = 500, 1e-10
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        X, H, info, ms = dev.minres_multi(B, iters, tol=tol, shift=shifts)
        steps = info["steps"]
        print("steps", steps.tolist(), "reference", REF_STEPS)
        assert info["status"].tolist() == [sp.MINRES_CONVERGED] * 3, info
        assert np.all(np.abs(steps - np.array(REF_STEPS)) <= 2), (info, REF_STEPS)
        assert steps[2] == steps[0] and np.array_equal(X[:, 2], 0.125 * X[:, 0])
        assert np.all(np.diff(H, axis=0) <= 0.0)
        for j in range(3):
            t = int(steps[j])
            assert H[t, j] <= tol * tol * H[0, j] and np.all(H[1:t, j] > tol * tol * H[0, j]), j
            assert np.all(H[t:, j] == H[t, j]), j                               # the history repeats after the stop
            rr = true_rr(oracle, row_ptr, col, val, B[:, j], X[:, j], shift=shifts[j])
            assert rr <= 4.0 * H[-1, j] + 1e-24 * H[0, j], (j, rr, H[-1, j], H[0, j])
        # the loop ended early: a budget just past the last stop gives the same bytes, and the long one costs no more
        # than a few polls' worth
        short = int(steps.max()) + 1
        Xs, Hs, infos, ms_short = dev.minres_multi(B, short, tol=tol, shift=shifts)
        assert Xs.tobytes() == X.tobytes() and Hs.tobytes() == H[: short + 1].tobytes()
        assert all(np.array_equal(infos[key], info[key]) for key in info)
        assert ms < 2.0 * ms_short + 2.0, (ms, ms_short)
        # a column's x is the tol = 0 iterate of its stopping step
        for j in (0, 1):
            Xt, Ht, _, _ = dev.minres_multi(B, int(steps[j]), shift=shifts)
            assert Xt[:, j].tobytes() == X[:, j].tobytes() and Ht[:, j].tobytes() == H[: steps[j] + 1, j].tobytes(), j


# ---------------------------------------------------------------- 6. a KKT matrix
def test_minres_multi_on_a_kkt_matrix(gpu, oracle):
    M, row_ptr, col, val, b = kkt_problem()
    rng = np.random.default_rng(22)
    B = np.ascontiguousarray(np.stack([b] + [rng.uniform(-1, 1, M) for _ in range(3)], axis=1))
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        X, H, info, _ = dev.minres_multi(B, KKT_STEPS)
        assert info["steps"].tolist() == [KKT_STEPS] * 4 and info["status"].tolist() == [sp.MINRES_RAN_ALL] * 4
        assert np.all(np.isfinite(X)) and np.all(np.diff(H, axis=0) <= 0.0)
        for j in range(4):
            rr = true_rr(oracle, row_ptr, col, val, B[:, j], X[:, j])
            print(f"kkt column {j}: true rr / hist[-1] - 1 = {rr / H[-1, j] - 1.0:.3e}")
            assert abs(rr / H[-1, j] - 1.0) <= KKT_FACTOR, (j, rr, H[-1, j])
        _, _, _, info_cg, _ = dev.pcg_multi(B, KKT_STEPS)
        assert info_cg["status"].tolist() == [sp.PCG_BREAKDOWN] * 4, info_cg


# ---------------------------------------------------------------- 7. refusals
def raw_minres_multi(dev, P, k, B, iters=2, tol=0.0, shift=None):
    """past the Python checks, into the library"""
    kk = max(k, 1)
    X, H = np.zeros((B.shape[0], kk)), np.zeros((max(iters, 0) + 1, kk))
    words = [np.zeros(kk, np.int32) for _ in range(2)]
    ms = C.c_float(0)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64).ctypes.data_as(nat.c_double_p)
    rc = sp.lib().spmv_hip_csr_minres_multi(dev.h, None if P is None else P.h, k, iters, tol, sh, None,
                                            B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                            H.ctypes.data_as(nat.c_double_p), *(w.ctypes.data_as(nat.c_int_p) for w in words),
                                            C.byref(ms))
    sp.device._check(rc, "spmv_hip_csr_minres_multi")


def refused(text, *args, **kw):
    with pytest.raises(sp.SpmvHipError) as e:
        raw_minres_multi(*args, **kw)
    assert text in str(e.value), (str(e.value), text)


def test_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, B_all = banded
    rng = np.random.default_rng(5)
    B = np.ascontiguousarray(B_all[:, :3])
    what = "csr_minres_multi"
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, \
            sp.CsrDevice(N, N, row_ptr, col, with_abs_diagonal(row_ptr, col, val)) as dev_abs, \
            dev_abs.preconditioner("jacobi") as jac:
        good = dev.minres_multi(B, 5, shift=SHIFTS[:3], precond=jac)

        def still_works(after):
            assert same_run(good, dev.minres_multi(B, 5, shift=SHIFTS[:3], precond=jac)), after

        for kind in ("ssor", "ilu0"):
            with dev_abs.preconditioner(kind) as tri:
                refused(f"{what}: an SSOR or ILU(0) preconditioner is two triangular solves, and those take one "
                        "right-hand side", dev, tri, 3, B)
            still_works(kind)
        refused(f"{what}: k = 0, must be in [1, 64]", dev, jac, 0, B)
        refused(f"{what}: k = 65, must be in [1, 64]", dev, jac, 65, np.zeros((N, 65)))
        still_works("k")
        refused(f"{what}: iters = -1, must be >= 0", dev, None, 3, B, iters=-1)
        for bad, text in ((-1.0, "-1"), (float("nan"), "nan"), (float("inf"), "inf")):
            refused(f"{what}: tol = {text}, must be finite and >= 0", dev, None, 3, B, tol=bad)
        still_works("iters and tol")
        for bad, text in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
            refused(f"{what}: shift[1] = {text}, must be finite", dev, None, 3, B, shift=[0.0, bad, 0.0])
        still_works("a bad shift")
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            refused(f"{what}: needs a square matrix (50 x 60)", rect, None, 2, np.ones((50, 2)))
        still_works("a non-square handle")
        with sp.CsrDevice(N, N, row_ptr, col, val, 0, N // 2) as half:          # rows [0, N/2) and no communicator
            refused(f"{what}: a handle of rows [0, {N // 2}) needs a communicator", half, None, 3, B)
        still_works("a row-range handle")
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            refused(f"{what}: a communicator exists, the row bounds are required", dev, None, 3, B)
        finally:
            comm.close()
        still_works("a communicator without bounds")
        rp3, col3, val3 = alternating_tridiagonal(500)
        with sp.CsrDevice(500, 500, rp3, col3, np.abs(val3)) as small, \
                sp.CsrDevice(N, N, row_ptr, col, np.abs(val).astype(np.float32)) as dev32:
            for other, why in ((small, "another size"), (dev32, "another dtype")):
                with other.preconditioner("jacobi") as P_other:
                    refused(f"{what}: the preconditioner covers rows", dev, P_other, 3, B)
                    with pytest.raises(ValueError):
                        dev.minres_multi(B, 2, precond=P_other)
                still_works(why)
        # every output but the time is optional, and so are the shifts
        ms = C.c_float(0)
        assert sp.lib().spmv_hip_csr_minres_multi(dev.h, jac.h, 3, 5, 0.0, None, None, B.ctypes.data_as(C.c_void_p), None,
                                                  None, None, None, C.byref(ms)) == 0 and ms.value > 0
        still_works("a call without outputs")


# ---------------------------------------------------------------- the CPU measurements behind MEASURED
def cpu_preconditioner(kind, row_ptr, col, val, dtype):
    """M^-1 for an n x k array as the CPU restatements compute it, every stored vector rounded to dtype"""
    import scipy.sparse as sps
    n = len(row_ptr) - 1
    rd = rd_of(dtype)
    v = rd(val)
    a = sps.csr_matrix((v, col, row_ptr), shape=(n, n))
    if kind == "none":
        return None
    if kind == "jacobi":
        inv = rd(1.0 / v[diagonal_positions(row_ptr, col)])
        return lambda R: R * inv[:, None]
    if kind == "block3":
        dense_blocks = [np.linalg.inv(a[i:min(i + 3, n), i:min(i + 3, n)].toarray()) for i in range(0, n, 3)]
        inv = sps.block_diag(dense_blocks).tocsr()
        inv.data = rd(inv.data)
        return lambda R: inv @ R
    if kind == "fsai":
        from test_fsai_host import fsai_ref, host_plan
        from test_trsv_host import canonical
        g_ptr, g_col, _, _, _ = host_plan(n, row_ptr, col, v, 32)
        g = sps.csr_matrix((rd(fsai_ref(canonical(row_ptr, col, v), g_ptr, g_col)), g_col, g_ptr), shape=(n, n))
        gt = g.T.tocsr()
        return lambda R: gt @ rd(g @ R)
    if kind == "amg":
        import _amg_ref
        levels = _amg_ref.build(a)
        return lambda R: _amg_ref.cycle(levels, np.asarray(R, dtype=np.float64), dtype=dtype)
    if kind == "cheb4_default":
        import _cheb_ref
        lmin, lmax = _cheb_ref.interval(a)
        g = _cheb_ref.inverse_diagonal(a, dtype)
        return lambda R: _cheb_ref.apply(a, g, R, 4, lmin, lmax, dtype)
    raise ValueError(kind)


def measure():
    from oracle.oracle import Oracle
    oracle = Oracle()
    for matrix, problem, kinds in (("banded", banded_columns(oracle), ("none", "jacobi", "block3")),
                                   ("spd", spd_columns(oracle), ("fsai", "amg", "cheb4_default"))):
        row_ptr, col, val, B = problem
        pval = with_abs_diagonal(row_ptr, col, val) if matrix == "banded" else val
        for kind in kinds:
            for dtype in DTYPES:
                # the loop as a handle of dtype computes it against the unrounded loop over a long-double product
                rd = rd_of(dtype)
                vals = rd(val)
                serial = columns_product(lambda u: oracle.csr_serial(row_ptr, col, vals, u))
                long = columns_product(product(row_ptr, col, val))
                minv = cpu_preconditioner(kind, row_ptr, col, pval, dtype)
                minv64 = cpu_preconditioner(kind, row_ptr, col, pval, np.float64)
                X, H, info = minres_multi_ref(serial, rd(B), STEPS, shift=SHIFTS, minv=minv, rd=rd)
                Xl, Hl, _ = minres_multi_ref(long, B, STEPS, shift=SHIFTS, minv=minv64)
                assert info["steps"].tolist() == [STEPS] * 4, (matrix, kind, info)
                d = differences(X, H, Xl, Hl)
                print(f'    ("{matrix}", "{kind}", "{np.dtype(dtype).name}"): {max(d):.3e},   # x {d[0]:.3e}, '
                      f"history {d[1]:.3e}")
    worst = {}
    cases = [(dtype, k, n, (1, 2, 3)) for dtype, k in LANE_CASES for n in LANE_SIZES]
    cases += [(np.float64, 64, 128 * rows_per_workgroup(64, np.float64) + 1, (2,)),
              (np.float64, 63, 91 * rows_per_workgroup(63, np.float64) - 1, (2,)),
              (np.float64, 64, K_MCG_BLOCKS * rows_per_workgroup(64, np.float64) + 3, (2,))]
    for dtype, k, n, steps in cases:
        rd = rd_of(dtype)
        rp, col, val, B = sizes_columns(n, k, dtype)
        for iters in steps:
            X, H, _ = minres_multi_ref(columns_product(product(rp, col, val, np.float64)), B, iters, shift=sizes_shifts(k),
                                       rd=rd)
            Xl, Hl, _ = minres_multi_ref(columns_product(product(rp, col, val)), B, iters, shift=sizes_shifts(k))
            d = differences(X, H, Xl, Hl)
            name = np.dtype(dtype).name
            if max(d) > worst.get(name, (0.0,))[0]:
                worst[name] = (max(d), n, k, iters, d)
    for name, (m, n, k, iters, d) in worst.items():
        print(f'    ("sizes", "{name}"): {m:.3e},   # n = {n}, k = {k}, {iters} steps, x {d[0]:.3e}, history {d[1]:.3e}')
    row_ptr, col, val, B = banded_columns(oracle)
    Bs = np.ascontiguousarray(np.stack([B[:, 0], B[:, 1], 0.125 * B[:, 0]], axis=1))
    serial = columns_product(lambda u: oracle.csr_serial(row_ptr, col, val, u))
    _, H, info = minres_multi_ref(serial, Bs, 500, tol=1e-10, shift=[0.0, 0.3, 0.0])
    print(f"    banded to tol 1e-10, shifts (0, 0.3, 0): {info}, nonincreasing {bool(np.all(np.diff(H, axis=0) <= 0))}")


if __name__ == "__main__":
    measure()
