"""spmv_hip_csr_bicgstab_multi on the GPU: k independent right-preconditioned BiCGSTAB recurrences that share the two
SpMMs of a step, against the restated loop (tests/_bicgstab_multi_ref.py) over the device's own SpMM and k-wide apply and
against bicgstab column by column; the lane shapes and grid edges; the bit identities the fixed reduction order promises;
every fate in one call; a NaN or Inf that stays in its column; the per-column stop; step counts with AMG and Chebyshev;
refused calls.

(A tiles-only handle exists only inside an HLL handle and cannot be reached from Python: that refusal of the C entry
point has no test here, as in test_lobpcg_host.py.)"""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from _bicgstab_multi_ref import (FATES_ITERS, FATES_N, FATES_TOL, bicgstab_multi_ref, fates_case, fates_expected)
from test_gpu_bicgstab import convection_diffusion, csr_of, nonsym_banded

pytestmark = pytest.mark.gpu

K_MCG_BLOCKS, K_BLOCK = 2048, 256    # cg_multi_kernels.hpp, spmv_internal.hpp
N = 6000
KINDS = {"none": None, "jacobi": dict(kind="jacobi"), "block3": dict(kind="block_jacobi", block=3),
         "fsai": dict(kind="fsai"), "amg": dict(kind="amg"),
         # for `banded` below: the entries of D^-1 A off the diagonal are uniform in about +-0.36, 7 a row, so its spectrum
         # lies in a disc of radius about 0.55 around 1.  The default interval [lmax / 30, lmax] of the Gershgorin bound
         # (about 2.3) is far wider than that: its degree-4 polynomial is large off the real axis and BiCGSTAB diverges
         # with it, one-wide and k-wide alike.  [0.4, 1.6] encloses the disc's real extent; the polynomial's residual on the
         # ellipse through 1 +- 0.55 i with these foci is below 0.7.
         "cheb4": dict(kind="chebyshev", degree=4, lmin=0.4, lmax=1.6),
         "cheb4_default": dict(kind="chebyshev", degree=4)}
ALL_KINDS = ["none", "jacobi", "block3", "fsai", "amg", "cheb4"]


class precond_of:
    """with precond_of(dev, name) as P: P is a Preconditioner or None"""

    def __init__(self, dev, name):
        self.P = None if KINDS[name] is None else dev.preconditioner(**KINDS[name])

    def __enter__(self):
        return self.P

    def __exit__(self, *exc):
        if self.P is not None:
            self.P.close()


def device_ops(dev, P):
    """the restated loop's operators: the device's own SpMM and k-wide apply, on arrays rounded to the handle's dtype"""
    cast = lambda X: np.ascontiguousarray(np.asarray(X).astype(dev.dtype))  # noqa: E731
    spmm = lambda X: dev.spmm(cast(X)).astype(np.float64)  # noqa: E731
    apply = None if P is None else (lambda R: P.apply_multi(cast(R)).astype(np.float64))
    return spmm, apply


def rows_per_workgroup(k, dtype):
    v = 16 // np.dtype(dtype).itemsize
    if k * np.dtype(dtype).itemsize % 16:
        v = 1
    cl = 0
    while (1 << cl) * v < k:
        cl += 1
    return K_BLOCK >> cl


def assert_columns_close(X, X_ref, rtol, what):
    for j in range(X_ref.shape[1]):
        scale = np.max(np.abs(X_ref[:, j]))
        err = np.max(np.abs(np.asarray(X[:, j], dtype=np.float64) - X_ref[:, j]))
        assert err <= rtol * scale, f"{what}: column {j}: {err:.3e} > {rtol} * {scale:.3e}"


def assert_meets_the_one_wide_tolerances(X, H, X_ref, H_ref, dtype, what):
    """the lines tests/test_gpu_bicgstab.py holds bicgstab to: fp64 1e-10 on x and on the history; fp32 1e-4 on x, 1e-6
    on h[0] and h[-1] <= 4 h_ref[-1] + 1e-10 h_ref[0]"""
    worst = np.max(np.abs(H - H_ref) / H_ref[0])
    print(f"{what}: worst |h - h_ref| / h_ref[0] = {worst:.3e}, h[-1] / h_ref[-1] in "
          f"[{np.min(H[-1] / H_ref[-1]):.4f}, {np.max(H[-1] / H_ref[-1]):.4f}]")
    if np.dtype(dtype) == np.float64:
        assert_columns_close(X, X_ref, 1e-10, what)
        assert np.all(np.abs(H - H_ref) <= 1e-10 * H_ref), what
    else:
        assert_columns_close(X, X_ref, 1e-4, what)
        assert np.all(np.abs(H[0] - H_ref[0]) <= 1e-6 * H_ref[0]), what
        assert np.all(H[-1] <= 4.0 * H_ref[-1] + 1e-10 * H_ref[0]), what


def same_run(one, two):
    return (one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
            and all(np.array_equal(one[2][key], two[2][key]) for key in ("steps", "status", "half_step")))


@pytest.fixture(scope="module")
def banded(oracle):
    rng = np.random.default_rng(909)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.5)
    X_true = rng.uniform(-1, 1, (N, 8))
    B = np.stack([oracle.csr_serial(row_ptr, col, val, X_true[:, j]) for j in range(8)], axis=1)
    return row_ptr, col, val, X_true, B


# ---------------------------------------------------------------- 1. against the restated loop
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_matches_the_restated_loop_and_bicgstab_column_by_column(gpu, oracle, banded, kind, dtype):
    """5 steps, tol = 0: every column's x and history within the one-wide test's tolerances of the restated loop over
    dev.spmm and P.apply_multi, and of dev.bicgstab on that column.  Then to tol = 1e-8 (fp64): the true residual
    through the oracle is the recorded one, |b_j - A x_j|^2 <= 4 h[-1, j] + 1e-24 h[0, j]; an fp32 recurrence leaves
    the true residual at the rounding of x, so that line is fp64's, as in the one-wide test."""
    row_ptr, col, val, _, B_all = banded
    k = 5
    B = np.ascontiguousarray(B_all[:, :k].astype(dtype))
    what = f"{kind} {np.dtype(dtype).name}"
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(dtype)) as dev, precond_of(dev, kind) as P:
        X, H, info, ms = dev.bicgstab_multi(B, 5, precond=P)
        assert X.shape == (N, k) and X.dtype == dtype and H.shape == (6, k) and ms > 0
        assert info["steps"].tolist() == [5] * k and info["status"].tolist() == [sp.BICG_RAN_ALL] * k
        assert info["half_step"].tolist() == [0] * k
        spmm, apply = device_ops(dev, P)
        X_ref, H_ref, info_ref = bicgstab_multi_ref(spmm, apply, B, 5)
        assert info_ref["steps"].tolist() == [5] * k
        assert_meets_the_one_wide_tolerances(X, H, X_ref, H_ref, dtype, what + " vs the restated loop")
        one = [dev.bicgstab(np.ascontiguousarray(B[:, j]), 5, precond=P) for j in range(k)]
        X_one = np.stack([o[0] for o in one], axis=1).astype(np.float64)
        H_one = np.stack([o[1] for o in one], axis=1)
        assert all(o[2] == {"steps": 5, "status": sp.BICG_RAN_ALL, "half_step": 0} for o in one)
        assert_meets_the_one_wide_tolerances(X, H, X_one, H_one, dtype, what + " vs bicgstab")
        if np.dtype(dtype) == np.float64:
            tol = 1e-8
            X, H, info, _ = dev.bicgstab_multi(B, 400, tol=tol, precond=P)
            # a column ends as bicgstab ends on it
            ends = [dev.bicgstab(np.ascontiguousarray(B[:, j]), 400, tol=tol, precond=P)[2] for j in range(k)]
            print(f"{what}: tol = {tol}: {info}; bicgstab: {[(e['steps'], e['status']) for e in ends]}")
            assert info["status"].tolist() == [e["status"] for e in ends], (what, info, ends)
            assert info["status"].tolist() == [sp.BICG_CONVERGED] * k, (what, info)
            for j in range(k):
                r = B[:, j] - oracle.csr_serial(row_ptr, col, val, np.ascontiguousarray(X[:, j]))
                rr = float(r @ r)
                assert H[-1, j] <= tol * tol * H[0, j]
                print(f"{what}: column {j}: true r.r {rr:.3e}, recorded {H[-1, j]:.3e}, h[0] {H[0, j]:.3e}")
                assert rr <= 4.0 * H[-1, j] + 1e-24 * H[0, j], (what, j, rr, H[-1, j], H[0, j])


# ---------------------------------------------------------------- 2. lane shapes and edges
def scaled_identity_plus_band(rng, n):
    """4 I plus three entries a row, uniform in +-1/3, within four columns of the diagonal, as CSR: nonsymmetric, its
    field of values within 1 of 4"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), 3)
    c = np.clip(r + rng.integers(-4, 5, len(r)), 0, n - 1)
    a = sps.csr_matrix((rng.uniform(-1, 1, len(r)) / 3.0, (r, c)), shape=(n, n)) + 4.0 * sps.identity(n)
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def check_three_steps(dev, P, B, dtype, what, fates=True):
    """3 steps against the restated loop.  fp64: x to 1e-10 of its column's largest entry, the history to 1e-10 h[0]; fp32: the one-wide test's fp32 line, 1e-4 on x, 1e-6 on h[0] and
    h[-1] <= 4 h_ref[-1] + 1e-10 h_ref[0] (one rounding of every stored vector a step, 6e-8 each, amplified by a well-conditioned
    matrix: the one-wide test's line for x).  The two loops differ by the order of the sums and by fused
    multiply-adds, a few units in the last place of fp64 per operation; once a column's residual is down at that
    rounding (n <= 3: the Krylov space is exhausted inside the three steps) the history holds noise in both loops, which
    the bound relative to h[0] admits and one relative to h[t] would not.  The matrices are 4 I plus a small band
    (scaled_identity_plus_band): on nonsym_banded one column in a few hundred passes a near-breakdown (r^.v cancels to
    1e-3 of its terms), its history jumps by up to 1e5 for a step, and the order of a sum decides the tenth digit of an
    fp64 history and the fourth of an fp32 x.  Here no column's history rises above h[0] (checked on the CPU)."""
    X, H, info, _ = dev.bicgstab_multi(B, 3, precond=P)
    spmm, apply = device_ops(dev, P)
    X_ref, H_ref, info_ref = bicgstab_multi_ref(spmm, apply, B, 3)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(H)), what
    if np.dtype(dtype) == np.float64:
        assert_columns_close(X, X_ref, 1e-10, what)
        assert np.all(H_ref <= H_ref[0]), what
        assert np.all(np.abs(H - H_ref) <= 1e-10 * H_ref[0]), (what, float(np.max(np.abs(H - H_ref) / H_ref[0])))
    else:
        assert_columns_close(X, X_ref, 1e-4, what)
        assert np.all(np.abs(H[0] - H_ref[0]) <= 1e-6 * H_ref[0]), what
        assert np.all(H[-1] <= 4.0 * H_ref[-1] + 1e-10 * H_ref[0]), (what, H[-1].tolist(), H_ref[-1].tolist())
    if fates:
        for key in ("steps", "status", "half_step"):
            assert np.array_equal(info[key], info_ref[key]), (what, key, info, info_ref)


@pytest.mark.parametrize("dtype,k", [(np.float64, k) for k in (1, 2, 3, 6, 8, 63, 64)]
                         + [(np.float32, k) for k in (4, 6, 12, 64)])
def test_lane_shapes_and_row_edges(gpu, dtype, k):
    """V = 2 (fp64, even k) and 4 (fp32, k a multiple of 4), V = 1, idle column lanes (k / V no power of two) and the
    widest k; n at 1, 2, around a wavefront and one row either side of a workgroup's pass.  Past n = 3 the fates must
    agree too."""
    rows = rows_per_workgroup(k, dtype)
    for n in sorted({1, 2, 63, 64, 65, rows - 1, rows + 1}):
        rng = np.random.default_rng([n, k])
        row_ptr, col, val = scaled_identity_plus_band(rng, n)
        B = rng.uniform(-1, 1, (n, k)).astype(dtype)
        with sp.CsrDevice(n, n, row_ptr, col, val.astype(dtype)) as dev:
            for kind in ("none", "jacobi", "block3"):
                with precond_of(dev, kind) as P:
                    check_three_steps(dev, P, B, dtype, f"{np.dtype(dtype).name} k={k} n={n} {kind}", fates=n > 3)


@pytest.mark.parametrize("k,g", [(64, 129), (63, 91)])
def test_grid_stride_past_the_workgroup_cap(gpu, k, g):
    """fp64 on a g x g convection-diffusion grid.  k = 64 is 32 column lanes and 8 rows per workgroup: the cap of 2048
    workgroups is reached at 16384 rows, at 16641 some lanes take a second row.  k = 63 is single elements, 64 column
    lanes and 4 rows per workgroup: the cap is reached at 8192 rows, 8281 is past it."""
    n = g * g
    assert n > K_MCG_BLOCKS * rows_per_workgroup(k, np.float64) and n <= 17000
    row_ptr, col, val = convection_diffusion(g, g, 0.4, 0.2, 0.05)
    B = np.random.default_rng(g).uniform(-1, 1, (n, k))
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev:
        for kind in ("none", "jacobi"):
            with precond_of(dev, kind) as P:
                check_three_steps(dev, P, B, np.float64, f"k={k} n={n} {kind}")


# ---------------------------------------------------------------- 3. bit identities
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_bit_identities(gpu, banded, kind):
    """Two calls give the same bytes; permuting B's columns permutes everything; equal columns give equal bytes; and
    (none, Jacobi, block-Jacobi, FSAI: every operation is a product, a sum or a quotient, in which a power of two moves
    through exactly) a column 2^e times another gives 2^e times its x and 4^e times its history."""
    row_ptr, col, val, _, B_all = banded
    B = np.ascontiguousarray(B_all[:, :6])
    B[:, 2] = B[:, 0]
    B[:, 3] = 8.0 * B[:, 1]
    B[:, 4] = 0.25 * B[:, 1]
    perm = np.array([4, 0, 5, 2, 1, 3])
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, precond_of(dev, kind) as P:
        for iters, tol in ((8, 0.0), (60, 1e-6)):
            run = dev.bicgstab_multi(B, iters, tol=tol, precond=P)
            assert same_run(run, dev.bicgstab_multi(B, iters, tol=tol, precond=P)), (kind, tol)
            X, H, info, _ = run
            Xp, Hp, infop, _ = dev.bicgstab_multi(np.ascontiguousarray(B[:, perm]), iters, tol=tol, precond=P)
            assert Xp.tobytes() == np.ascontiguousarray(X[:, perm]).tobytes(), (kind, tol)
            assert Hp.tobytes() == np.ascontiguousarray(H[:, perm]).tobytes(), (kind, tol)
            for key in ("steps", "status", "half_step"):
                assert np.array_equal(infop[key], info[key][perm]), (kind, tol, key)
            assert np.array_equal(X[:, 2], X[:, 0]) and np.array_equal(H[:, 2], H[:, 0]), (kind, tol)
            assert all(info[key][2] == info[key][0] for key in info)
            if kind in ("none", "jacobi", "block3", "fsai"):
                for j, e in ((3, 3), (4, -2)):
                    assert np.array_equal(X[:, j], 2.0 ** e * X[:, 1]), (kind, tol, e)
                    assert np.array_equal(H[:, j], 4.0 ** e * H[:, 1]), (kind, tol, e)
                    assert all(info[key][j] == info[key][1] for key in info)


def test_single_rank_communicator_gives_the_same_bits(gpu, banded):
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, _, B_all = banded
    cases = ((3, 8, 0.0), (8, 8, 0.0), (8, 60, 1e-6))
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, precond_of(dev, "jacobi") as J, precond_of(dev, "fsai") as F:
        plain = {(i, c): dev.bicgstab_multi(np.ascontiguousarray(B_all[:, :c[0]]), c[1], tol=c[2], precond=P)
                 for i, P in enumerate((None, J, F)) for c in cases}
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            bounds = np.array([0, N], np.int32)
            for (i, c), run in plain.items():
                again = dev.bicgstab_multi(np.ascontiguousarray(B_all[:, :c[0]]), c[1], tol=c[2],
                                           precond=(None, J, F)[i], bounds=bounds)
                assert same_run(run, again), (i, c)
            with pytest.raises(sp.SpmvHipError, match="bounds"):
                dev.bicgstab_multi(np.ascontiguousarray(B_all[:, :2]), 2)   # a communicator needs them
        finally:
            comm.close()


# ---------------------------------------------------------------- 4. fates in one call
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_fate_in_one_call(gpu, dtype):
    """A half step, both breakdowns, a zero column and two columns that iterate, in one call: status, steps and
    half_step are the restated loop's for tol = 0 and tol = 1e-10, the columns whose every value is exact match it bit
    for bit, and all of X is finite."""
    A, B = fates_case()
    n, row_ptr, col, val = csr_of(A)
    assert n == FATES_N
    dense = lambda X: np.stack([A @ np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], axis=1)  # noqa: E731
    with sp.CsrDevice(n, n, row_ptr, col, val.astype(dtype)) as dev:
        for tol in (0.0, FATES_TOL):
            X, H, info, _ = dev.bicgstab_multi(B.astype(dtype), FATES_ITERS, tol=tol)
            X_ref, H_ref, _ = bicgstab_multi_ref(dense, None, B, FATES_ITERS, tol)
            steps, status, half = fates_expected(tol)
            print(f"{np.dtype(dtype).name} tol={tol}: {info}; column 3: h / h[0] = {(H[:, 3] / H[0, 3]).tolist()}")
            assert info["status"].tolist() == status and info["steps"].tolist() == steps, (tol, info)
            assert info["half_step"].tolist() == half, (tol, info)
            assert np.all(np.isfinite(X)) and np.all(np.isfinite(H))
            for j in (0, 1, 2, 4):
                assert X[:, j].tobytes() == X_ref[:, j].astype(dtype).tobytes(), (tol, j)
                assert H[:, j].tobytes() == H_ref[:, j].tobytes(), (tol, j)
            assert np.array_equal(X[:, 5], dtype(8.0) * X[:, 3]) and np.array_equal(H[:, 5], 64.0 * H[:, 3])


# ---------------------------------------------------------------- 5. isolation
@pytest.mark.parametrize("kind", ["none", "jacobi", "amg", "cheb4"])
def test_a_nan_or_inf_in_one_column_of_B_stays_in_that_column(gpu, banded, kind):
    """Column j ends in a breakdown with a finite x; every other column's outputs are, byte for byte, those of the same
    call with column j of B set to zeros."""
    row_ptr, col, val, _, B_all = banded
    k, j = 5, 2
    B = np.ascontiguousarray(B_all[:, :k])
    B_zero = B.copy()
    B_zero[:, j] = 0.0
    others = [c for c in range(k) if c != j]
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, precond_of(dev, kind) as P:
        X0, H0, info0, _ = dev.bicgstab_multi(B_zero, 5, precond=P)
        assert info0["steps"][j] == 0 and info0["status"][j] == sp.BICG_CONVERGED
        for poison in (np.nan, np.inf):
            B_bad = B.copy()
            B_bad[1234, j] = poison
            X, H, info, _ = dev.bicgstab_multi(B_bad, 5, precond=P)
            assert info["status"][j] in (sp.BICG_BREAKDOWN_RHO, sp.BICG_BREAKDOWN_OMEGA), (kind, poison, info)
            assert np.all(np.isfinite(X[:, j])), (kind, poison)
            assert np.ascontiguousarray(X[:, others]).tobytes() == np.ascontiguousarray(X0[:, others]).tobytes(), (kind, poison)
            assert np.ascontiguousarray(H[:, others]).tobytes() == np.ascontiguousarray(H0[:, others]).tobytes(), (kind, poison)
            for key in ("steps", "status", "half_step"):
                assert np.array_equal(info[key][others], info0[key][others]), (kind, poison, key)


# ---------------------------------------------------------------- 6. stopping
def test_columns_stop_on_their_own_and_the_loop_ends_early(gpu, oracle):
    """A smooth right-hand side next to random ones, tol = 1e-8: each column's history is the tol = 0 run's up to its
    stop and repeats after it, its x is the tol = 0 iterate of that step, and a budget 20 times larger costs no more."""
    rng = np.random.default_rng(77)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.3)
    smooth = oracle.csr_serial(row_ptr, col, val, np.ones(N))
    B = np.ascontiguousarray(np.stack([smooth, rng.uniform(-1, 1, N), 1e-3 * smooth + rng.uniform(-1, 1, N),
                                       np.sin(np.arange(N) / 500.0)], axis=1))
    k = B.shape[1]
    tol = 1e-8
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        first = dev.bicgstab_multi(B, 300, tol=tol)
        steps = first[2]["steps"]
        iters = int(steps.max()) + 1
        assert np.all(first[2]["status"] == sp.BICG_CONVERGED) and 1 <= steps.min() and iters < 300, first[2]
        X, H, info, ms = dev.bicgstab_multi(B, iters, tol=tol)
        assert same_run((X, H, info), (first[0], first[1][: iters + 1], first[2]))
        assert np.all(first[1][iters:] == first[1][iters])
        print("steps", steps.tolist(), "half", info["half_step"].tolist())
        X0, H0, info0, _ = dev.bicgstab_multi(B, iters)                       # tol = 0
        assert info0["steps"].tolist() == [iters] * k
        for j in range(k):
            t = int(steps[j])
            assert H[t, j] <= tol * tol * H[0, j] and np.all(H[1:t, j] > tol * tol * H[0, j]), j
            assert np.all(H[t:, j] == H[t, j]), j
            upto = t if info["half_step"][j] else t + 1
            assert H[:upto, j].tobytes() == H0[:upto, j].tobytes(), j
            if not info["half_step"][j]:
                Xt, _, _, _ = dev.bicgstab_multi(B, t)                        # tol = 0, stopped at that step
                assert Xt[:, j].tobytes() == X[:, j].tobytes(), j
        big = dev.bicgstab_multi(B, 20 * iters, tol=tol)
        assert big[0].tobytes() == X.tobytes() and big[1][: iters + 1].tobytes() == H.tobytes()
        assert np.all(big[1][iters:] == H[-1]) and all(np.array_equal(big[2][key], info[key]) for key in info)
        assert big[3] < 5.0 * ms + 2.0, (big[3], ms)


# ---------------------------------------------------------------- 7. step counts
@pytest.mark.parametrize("kind", ["amg", "cheb4_default"])
def test_step_counts_on_convection_diffusion(gpu, kind):
    """The 40 x 40 convection-diffusion stencil to tol = 1e-8, k = 4: every column converges in the restated loop's count
    +- 1, and that count is below a third of the unpreconditioned one."""
    import _amg_ref
    a = _amg_ref.convection_diffusion(40)
    n, row_ptr, col, val = csr_of(a.toarray())
    B = np.random.default_rng(40).uniform(-1, 1, (n, 4))
    tol = 1e-8
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev, precond_of(dev, kind) as P:
        X, H, info, _ = dev.bicgstab_multi(B, 400, tol=tol, precond=P)
        plain = dev.bicgstab_multi(B, 400, tol=tol)[2]
        _, _, info_ref = bicgstab_multi_ref(*device_ops(dev, P), B, 400, tol)
        print(kind, "steps", info["steps"].tolist(), "restated", info_ref["steps"].tolist(), "plain", plain["steps"].tolist())
        assert info["status"].tolist() == [sp.BICG_CONVERGED] * 4 and plain["status"].tolist() == [sp.BICG_CONVERGED] * 4
        assert info_ref["status"].tolist() == [sp.BICG_CONVERGED] * 4
        assert np.all(np.abs(info["steps"] - info_ref["steps"]) <= 1), (info, info_ref)
        assert np.all(3 * info["steps"] < plain["steps"]), (info, plain)
        assert np.all(H[-1] <= tol * tol * H[0]) and np.all(np.isfinite(X))


# ---------------------------------------------------------------- 8. refusals
def raw_bicgstab_multi(dev, P, k, B, iters=2):
    """past the Python checks, into the library"""
    kk = max(k, 1)
    X, H = np.zeros((B.shape[0], kk)), np.zeros((iters + 1, kk))
    words = [np.zeros(kk, np.int32) for _ in range(3)]
    ms = C.c_float(0)
    rc = sp.lib().spmv_hip_csr_bicgstab_multi(dev.h, None if P is None else P.h, k, iters, 0.0, None,
                                              B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                              H.ctypes.data_as(nat.c_double_p), *(w.ctypes.data_as(nat.c_int_p) for w in words),
                                              C.byref(ms))
    sp.device._check(rc, "spmv_hip_csr_bicgstab_multi")


def test_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    row_ptr, col, val, _, B_all = banded
    rng = np.random.default_rng(5)
    B = np.ascontiguousarray(B_all[:, :3])
    x = rng.uniform(-1, 1, N)
    y_ref = oracle.csr_serial(row_ptr, col, val, x)
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, precond_of(dev, "jacobi") as jac:
        good = dev.bicgstab_multi(B, 5, precond=jac)

        def still_works(after):
            assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref)), after
            assert same_run(good, dev.bicgstab_multi(B, 5, precond=jac)), after

        for kind in ("ssor", "ilu0"):
            with dev.preconditioner(kind) as tri:
                with pytest.raises(sp.SpmvHipError, match="one right-hand side"):
                    dev.bicgstab_multi(B, 3, precond=tri)
            still_works(kind)
        with pytest.raises(sp.SpmvHipError, match="k = 0"):
            raw_bicgstab_multi(dev, jac, 0, B)
        still_works("k = 0")
        with pytest.raises(sp.SpmvHipError, match="k = 65"):
            raw_bicgstab_multi(dev, jac, 65, np.zeros((N, 65)))
        still_works("k = 65")
        for bad in (-1.0, float("nan"), float("inf")):
            ms = C.c_float(0)
            assert sp.lib().spmv_hip_csr_bicgstab_multi(dev.h, None, 3, 2, bad, None, B.ctypes.data_as(C.c_void_p), None,
                                                        None, None, None, None, C.byref(ms)) == -1
            assert b"tol" in sp.lib().spmv_hip_last_error()
        still_works("a bad tol")
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(sp.SpmvHipError, match="square"):
                rect.bicgstab_multi(np.ones((50, 2)), 2)
        still_works("a non-square handle")
        small_rp, small_col, small_val = nonsym_banded(rng, 500, 5, 20, 0.5)
        with sp.CsrDevice(500, 500, small_rp, small_col, small_val) as small, \
                sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
            for other, what in ((small, "another size"), (dev32, "another dtype")):
                with other.preconditioner("jacobi") as P_other:
                    with pytest.raises(sp.SpmvHipError, match="the preconditioner covers rows"):
                        raw_bicgstab_multi(dev, P_other, 3, B)
                still_works(what)
        # every output but the time is optional
        ms = C.c_float(0)
        assert sp.lib().spmv_hip_csr_bicgstab_multi(dev.h, jac.h, 3, 5, 0.0, None, B.ctypes.data_as(C.c_void_p), None, None,
                                                    None, None, None, C.byref(ms)) == 0 and ms.value > 0
        still_works("a call without outputs")
