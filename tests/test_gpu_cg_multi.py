"""spmv_hip_csr_cg_multi on the GPU: k independent CG recurrences (one alpha and one beta per column) that share one
SpMM per step, against a per-column numpy loop over the oracle's serial product, plus the bit-level identities the
fixed reduction order promises, the freeze rule of tol, fp32, a single-rank communicator, refused calls and a
FEM-shaped matrix of about a million rows."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat

pytestmark = pytest.mark.gpu


def spd_banded(rng, n, per_row, band):
    """symmetric, strictly diagonally dominant (hence positive definite) banded matrix as CSR"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-band, band + 1, len(r)), 0, n - 1)
    b = sps.csr_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n))
    a = b + b.T
    a = a + sps.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0)
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def make_spd(row_ptr, col, val):
    """a symmetric matrix with one diagonal entry per row -> SPD: each row's absolute sum + 1 added to its diagonal"""
    M = len(row_ptr) - 1
    rows = np.repeat(np.arange(M), np.diff(row_ptr))
    diag = np.flatnonzero(col == rows)
    assert len(diag) == M
    val = val.copy()
    val[diag] += np.add.reduceat(np.abs(val), row_ptr[:-1]) + 1.0
    return val


def cg_with(spmv, b, iters):
    """the textbook loop spmv_hip_csr_cg runs, with a given product; returns (x, r.r history)"""
    x = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rs = float(r @ r)
    hist = [rs]
    for _ in range(iters):
        q = spmv(p)
        alpha = rs / float(p @ q)
        x += alpha * p
        r -= alpha * q
        rs_new = float(r @ r)
        p = r + (rs_new / rs) * p
        rs = rs_new
        hist.append(rs)
    return x, np.array(hist)


def cg_columns(oracle, row_ptr, col, val, B, iters):
    """the reference: cg_with on every column of B -> (X, hist (iters + 1) x k)"""
    out = [cg_with(lambda v: oracle.csr_serial(row_ptr, col, val, v), np.array(B[:, j], dtype=np.float64), iters)
           for j in range(B.shape[1])]
    return np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1)


def products(oracle, row_ptr, col, val, X):
    return np.stack([oracle.csr_serial(row_ptr, col, val, X[:, j]) for j in range(X.shape[1])], axis=1)


def assert_columns_close(X, X_ref, rtol, what):
    for j in range(X.shape[1]):
        scale = np.max(np.abs(X_ref[:, j]))
        err = np.max(np.abs(X[:, j] - X_ref[:, j]))
        assert err <= rtol * scale, f"{what}: column {j}: {err:.3e} > {rtol} * {scale:.3e}"


def assert_true_residual(oracle, row_ptr, col, val, B, X, hist):
    """the recurrence's residual is the true one: |b_j - A x_j|^2 <= 4 rs_j"""
    R = B - products(oracle, row_ptr, col, val, np.asarray(X, dtype=np.float64))
    for j in range(B.shape[1]):
        rr = float(R[:, j] @ R[:, j])
        assert rr <= 4.0 * hist[-1, j] + 1e-20 * hist[0, j], f"column {j}: true {rr:.3e} vs recorded {hist[-1, j]:.3e}"


N = 6000


@pytest.fixture(scope="module")
def banded(oracle):
    rng = np.random.default_rng(808)
    row_ptr, col, val = spd_banded(rng, N, 7, 60)
    X_true = rng.uniform(-1, 1, (N, 40))
    B = products(oracle, row_ptr, col, val, X_true)
    return row_ptr, col, val, X_true, B


@pytest.mark.parametrize("k", [2, 3, 8, 40])
def test_cg_multi_matches_the_per_column_reference_loop(gpu, oracle, banded, k):
    """k = 3: element loads; k = 2, 8: 16-byte loads; k = 40 crosses the SpMM's 32-column tile."""
    row_ptr, col, val, X_true, B_all = banded
    B, xt = np.ascontiguousarray(B_all[:, :k]), X_true[:, :k]
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        X5, h5, done5, _ = dev.cg_multi(B, 5)
        X_ref5, h_ref5 = cg_columns(oracle, row_ptr, col, val, B, 5)
        assert X5.shape == (N, k) and h5.shape == (6, k) and done5.tolist() == [5] * k
        assert_columns_close(X5, X_ref5, 1e-10, "5 steps")
        assert np.all(np.abs(h5 - h_ref5) <= 1e-10 * h_ref5[0])
        iters = 25
        X, h, done, ms = dev.cg_multi(B, iters)
        X_ref, h_ref = cg_columns(oracle, row_ptr, col, val, B, iters)
        assert ms > 0 and done.tolist() == [iters] * k
        assert np.all(np.abs(h[0] - h_ref[0]) <= 1e-13 * h_ref[0])
        assert_columns_close(X, X_ref, 1e-7, "25 steps")
        assert np.all(np.abs(h - h_ref) <= 1e-8 * h_ref[0] + 1e-4 * h_ref)
        assert np.all(h_ref[-1] < 1e-6 * h_ref[0])                      # the reference itself converges
        assert_columns_close(X, xt, 1e-3, "towards x_true")
        assert_true_residual(oracle, row_ptr, col, val, B, X, h)


def test_cg_multi_bit_identities(gpu, banded):
    """k = 1 is csr_cg bit for bit (fp64 and fp32); two calls agree; permuting B's columns permutes X and the history;
    equal columns give equal columns; a zero column stays exactly zero and harms no other column."""
    row_ptr, col, val, _, B_all = banded
    iters = 25
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        b = np.ascontiguousarray(B_all[:, 0])
        x1, h1, _ = dev.cg(b, iters)
        X, h, done, _ = dev.cg_multi(b, iters)                      # a vector: k = 1
        assert X.shape == (N, 1) and h.shape == (iters + 1, 1) and done.tolist() == [iters]
        assert X[:, 0].tobytes() == x1.tobytes() and h[:, 0].tobytes() == h1.tobytes()

        B = np.ascontiguousarray(B_all[:, :8])
        X, h, done, _ = dev.cg_multi(B, iters)
        X2, h2, done2, _ = dev.cg_multi(B, iters)
        assert X2.tobytes() == X.tobytes() and h2.tobytes() == h.tobytes() and np.array_equal(done2, done)
        perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
        Xp, hp, _, _ = dev.cg_multi(np.ascontiguousarray(B[:, perm]), iters)
        assert Xp.tobytes() == np.ascontiguousarray(X[:, perm]).tobytes()
        assert hp.tobytes() == np.ascontiguousarray(h[:, perm]).tobytes()
        for k in (3, 6):                                            # element path, and 16-byte pieces with idle lanes
            Bp = np.ascontiguousarray(B[:, :k][:, ::-1])
            Xr, hr, _, _ = dev.cg_multi(Bp, iters)
            Xk, hk, _, _ = dev.cg_multi(np.ascontiguousarray(B[:, :k]), iters)
            assert Xr.tobytes() == np.ascontiguousarray(Xk[:, ::-1]).tobytes()
            assert hr.tobytes() == np.ascontiguousarray(hk[:, ::-1]).tobytes()

        Be = B.copy()
        Be[:, 4] = Be[:, 1]
        Be[:, 2] = 0.0
        Xe, he, de, _ = dev.cg_multi(Be, iters)
        assert Xe[:, 4].tobytes() == Xe[:, 1].tobytes() and he[:, 4].tobytes() == he[:, 1].tobytes()
        assert np.all(Xe[:, 2] == 0.0) and np.all(he[:, 2] == 0.0) and de[2] == 0
        assert np.all(np.isfinite(Xe)) and np.all(np.isfinite(he))
        assert de.tolist() == [iters, iters, 0, iters, iters, iters, iters, iters]
        others = [0, 1, 3, 5, 6, 7]
        assert Xe[:, others].tobytes() == np.ascontiguousarray(X[:, others]).tobytes()

    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        b32 = B_all[:, 0].astype(np.float32)
        x1, h1, _ = dev32.cg(b32, iters)
        X, h, _, _ = dev32.cg_multi(b32, iters)
        assert X[:, 0].tobytes() == x1.tobytes() and h[:, 0].tobytes() == h1.tobytes()


def test_cg_multi_tol_freezes_columns_and_stops_early(gpu, oracle, banded):
    """Columns of very different difficulty (eigenvectors of A converge in one or two steps) freeze at different steps;
    a frozen column is exactly the tol = 0 run stopped at its step, its history then repeats; once all are frozen the
    loop ends, so a far larger step budget costs no more."""
    import scipy.sparse as sps
    from scipy.sparse.linalg import eigsh
    row_ptr, col, val, _, B_all = banded
    A = sps.csr_matrix((val, col, row_ptr), shape=(N, N))
    _, vecs = eigsh(A, k=2, which="LA", tol=1e-14, v0=np.ones(N))
    B = np.ascontiguousarray(np.column_stack([B_all[:, 0], vecs[:, 0], 1e-8 * B_all[:, 1], vecs[:, 0] + vecs[:, 1],
                                              B_all[:, 2]]))
    tol = 1e-8
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        iters = 200
        X, h, done, ms = dev.cg_multi(B, iters, tol=tol)
        assert h.shape == (iters + 1, 5)
        assert np.all(h[-1] <= tol * tol * h[0]), (h[-1], h[0])
        assert np.all((done >= 1) & (done < iters)), done
        assert done[1] <= 2 and done[3] <= 3 and done[0] > done[3], done
        assert len(set(done.tolist())) >= 3, done
        for j in range(B.shape[1]):
            t = int(done[j])
            assert np.all(h[t:, j] == h[t, j])                       # frozen: the history repeats
            assert h[t, j] <= tol * tol * h[0, j] and np.all(h[1:t, j] > tol * tol * h[0, j])
            X0, h0, d0, _ = dev.cg_multi(B, t)                      # tol = 0, stopped at that column's step
            assert d0.tolist() == [t] * B.shape[1]
            assert X0[:, j].tobytes() == X[:, j].tobytes(), j
            assert h0[:, j].tobytes() == h[: t + 1, j].tobytes(), j
        assert_true_residual(oracle, row_ptr, col, val, B, X, h)
        # a budget 50 times larger: the loop stops at the same step (one device word read every 16 steps)
        X_big, h_big, done_big, ms_big = dev.cg_multi(B, 50 * iters, tol=tol)
        assert X_big.tobytes() == X.tobytes() and np.array_equal(done_big, done)
        assert h_big[: iters + 1].tobytes() == h.tobytes() and np.all(h_big[iters:] == h[-1])
        assert ms_big < 5.0 * ms + 2.0, (ms_big, ms)


def test_cg_multi_fp32_handle(gpu, oracle, banded):
    """fp32 data, k = 4 (16-byte pieces): within 1e-4 of the fp64 reference after 6 steps."""
    row_ptr, col, val, _, B_all = banded
    B = np.ascontiguousarray(B_all[:, :4])
    X_ref, _ = cg_columns(oracle, row_ptr, col, val, B, 6)
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        X, h, done, _ = dev32.cg_multi(B.astype(np.float32), 6)
    assert X.dtype == np.float32 and done.tolist() == [6] * 4
    assert_columns_close(X.astype(np.float64), X_ref, 1e-4, "fp32")


def test_cg_multi_single_rank_communicator_gives_the_same_bits(gpu, banded):
    """bounds = [0, n] with a communicator: all-gatherv of P with bounds scaled by k, the k dot products all-gathered
    and added in rank order -- the bits of the run without one."""
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, _, B_all = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        plain = {k: dev.cg_multi(np.ascontiguousarray(B_all[:, :k]), 25) for k in (3, 8)}
        plain_tol = dev.cg_multi(np.ascontiguousarray(B_all[:, :8]), 40, tol=1e-6)
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            bounds = np.array([0, N], np.int32)
            for k, (X, h, done, _) in plain.items():
                Xg, hg, dg, _ = dev.cg_multi(np.ascontiguousarray(B_all[:, :k]), 25, bounds=bounds)
                assert Xg.tobytes() == X.tobytes() and hg.tobytes() == h.tobytes() and np.array_equal(dg, done)
            Xg, hg, dg, _ = dev.cg_multi(np.ascontiguousarray(B_all[:, :8]), 40, tol=1e-6, bounds=bounds)
            assert Xg.tobytes() == plain_tol[0].tobytes() and hg.tobytes() == plain_tol[1].tobytes()
            assert np.array_equal(dg, plain_tol[2])
            with pytest.raises(RuntimeError, match="bounds"):
                dev.cg_multi(np.ascontiguousarray(B_all[:, :2]), 2)  # a communicator needs the row bounds
        finally:
            comm.close()


def test_cg_multi_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    row_ptr, col, val, _, B_all = banded
    rng = np.random.default_rng(5)
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        B = np.ascontiguousarray(B_all[:, :3])
        X = np.zeros((N, 65))
        hist = np.zeros((3, 65))
        done = np.zeros(65, dtype=np.int32)
        ms = C.c_float(0)
        L = sp.lib()
        for k in (0, 65):                     # past the Python checks, into the library
            rc = L.spmv_hip_csr_cg_multi(dev.h, k, 2, 0.0, None, X.ctypes.data_as(C.c_void_p),
                                         X.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                         done.ctypes.data_as(nat.c_int_p), C.byref(ms))
            assert rc == -1 and b"k =" in L.spmv_hip_last_error()
        for bad in (np.zeros((N - 1, 3)), np.zeros((N, 0)), np.zeros((N, 65))):
            with pytest.raises(ValueError):
                dev.cg_multi(bad, 2)
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(RuntimeError, match="square"):
                rect.cg_multi(np.ones((50, 2)), 2)
        # and the handle still computes
        x = rng.uniform(-1, 1, N)
        y_ref = oracle.csr_serial(row_ptr, col, val, x)
        assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref))
        Xs = rng.uniform(-1, 1, (N, 5))
        Y_ref = products(oracle, row_ptr, col, val, Xs)
        assert np.max(np.abs(dev.spmm(Xs) - Y_ref)) <= 1e-10 * np.max(np.abs(Y_ref))
        X5, _, _, _ = dev.cg_multi(B, 5)
        X_ref5, _ = cg_columns(oracle, row_ptr, col, val, B, 5)
        assert_columns_close(X5, X_ref5, 1e-10, "after refusals")


def test_cg_multi_fem_million_rows(gpu, oracle):
    """A FEM-shaped SPD matrix of about 10^6 rows (78 M entries), k = 8, 10 steps."""
    from sparsematrixvectormultiplication_amd import synth
    M, row_ptr, col, val = synth.fem_like((36, 36, 257), 1)
    val = make_spd(row_ptr, col, val)
    rng = np.random.default_rng(36)
    B = rng.uniform(-1, 1, (M, 8))
    iters = 10
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        X, h, done, ms = dev.cg_multi(B, iters)
    assert ms > 0 and done.tolist() == [iters] * 8
    X_ref, h_ref = cg_columns(oracle, row_ptr, col, val, B, iters)
    assert_columns_close(X, X_ref, 1e-8, "fem")
    assert np.all(np.abs(h - h_ref) <= 1e-8 * h_ref[0] + 1e-6 * h_ref)
    assert_true_residual(oracle, row_ptr, col, val, B, X, h)
