"""spmv_hip_csr_bicgstab on the GPU: BiCGSTAB for a nonsymmetric A against a numpy loop of exactly the documented
algorithm over the oracle's serial product, plus reproducibility, the tol stop, half-step convergence, both
breakdowns, a single-rank communicator, refused calls and an unsymmetric convection-diffusion matrix of a million
rows."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat

pytestmark = pytest.mark.gpu


def bicgstab_ref(spmv, b, iters, tol=0.0):
    """The loop spmv_hip_csr_bicgstab runs (include/spmv_hip.h), in fp64 with a given product; returns
    (x, r.r history [iters + 1], info)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    rh = b.copy()
    p = b.copy()
    rho, rr0 = float(rh @ r), float(r @ r)
    hist = [rr0]
    info = {"steps": iters, "status": sp.BICG_RAN_ALL, "half_step": 0}
    tol2 = tol * tol
    if rr0 == 0.0:
        return x, np.full(iters + 1, rr0), {"steps": 0, "status": sp.BICG_CONVERGED, "half_step": 0}
    for k in range(1, iters + 1):
        v = spmv(p)
        rv = float(rh @ v)
        if rv == 0.0 or not np.isfinite(rv):
            info.update(steps=k - 1, status=sp.BICG_BREAKDOWN_RHO)
            break
        alpha = rho / rv
        s = r - alpha * v
        ss = float(s @ s)
        if ss <= tol2 * rr0:
            x = x + alpha * p
            r = s
            hist.append(ss)
            info.update(steps=k, status=sp.BICG_CONVERGED, half_step=1)
            break
        t = spmv(s)
        ts, tt = float(t @ s), float(t @ t)
        omega = ts / tt if tt != 0.0 else np.inf
        if tt == 0.0 or ts == 0.0 or not (np.isfinite(ts) and np.isfinite(tt) and np.isfinite(omega)):
            info.update(steps=k - 1, status=sp.BICG_BREAKDOWN_OMEGA)
            break
        x = x + (alpha * p + omega * s)
        r = s - omega * t
        rho_new, rr = float(rh @ r), float(r @ r)
        hist.append(rr)
        if rr <= tol2 * rr0:
            info.update(steps=k, status=sp.BICG_CONVERGED)
            break
        if rho_new == 0.0 or not np.isfinite(rho_new):
            info.update(steps=k, status=sp.BICG_BREAKDOWN_RHO)
            break
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
    hist += [hist[-1]] * (iters + 1 - len(hist))
    return x, np.array(hist), info


def nonsym_banded(rng, n, per_row, band, dominance):
    """unsymmetric banded matrix, diagonal = dominance x the row's absolute sum + 1, as CSR"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-band, band + 1, len(r)), 0, n - 1)
    a = sps.csr_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n))
    a = a + sps.diags(dominance * np.asarray(abs(a).sum(axis=1)).ravel() + 1.0)
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def convection_diffusion(nx, ny, px, py, shift):
    """5-point convection-diffusion on an nx x ny grid (central differences, cell Peclet numbers px, py), diagonal
    4 + shift: unsymmetric"""
    import scipy.sparse as sps
    n = nx * ny
    i = np.arange(n)
    gx, gy = i % nx, i // nx
    rows, cols, vals = [i], [i], [np.full(n, 4.0 + shift)]
    for cond, off, val in ((gx > 0, -1, -1.0 - px), (gx < nx - 1, 1, -1.0 + px),
                           (gy > 0, -nx, -1.0 - py), (gy < ny - 1, nx, -1.0 + py)):
        rows.append(i[cond])
        cols.append(i[cond] + off)
        vals.append(np.full(int(cond.sum()), val))
    a = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def csr_of(dense):
    import scipy.sparse as sps
    a = sps.csr_matrix(np.asarray(dense, dtype=np.float64))
    a.sort_indices()
    return a.shape[0], a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def assert_close(x, x_ref, rtol, what):
    scale = np.max(np.abs(x_ref))
    err = np.max(np.abs(np.asarray(x, dtype=np.float64) - x_ref))
    assert err <= rtol * scale, f"{what}: {err:.3e} > {rtol} * {scale:.3e}"


def true_rr(oracle, row_ptr, col, val, b, x):
    r = np.asarray(b, dtype=np.float64) - oracle.csr_serial(row_ptr, col, val, np.asarray(x, dtype=np.float64))
    return float(r @ r)


N = 6000


@pytest.fixture(scope="module")
def banded(oracle):
    rng = np.random.default_rng(909)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.5)
    x_true = rng.uniform(-1, 1, N)
    b = oracle.csr_serial(row_ptr, col, val, x_true)
    return row_ptr, col, val, x_true, b


def test_bicgstab_matches_the_reference_loop_fp64(gpu, oracle, banded):
    row_ptr, col, val, x_true, b = banded
    spmv = lambda v: oracle.csr_serial(row_ptr, col, val, v)  # noqa: E731
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x5, h5, info5, _ = dev.bicgstab(b, 5)
        x_ref5, h_ref5, info_ref5 = bicgstab_ref(spmv, b, 5)
        assert info5 == info_ref5 == {"steps": 5, "status": sp.BICG_RAN_ALL, "half_step": 0}
        assert x5.dtype == np.float64 and h5.shape == (6,)
        assert_close(x5, x_ref5, 1e-10, "5 steps")
        assert np.all(np.abs(h5 - h_ref5) <= 1e-10 * h_ref5)
        iters = 25
        x, h, info, ms = dev.bicgstab(b, iters)
        x_ref, h_ref, info_ref = bicgstab_ref(spmv, b, iters)
        assert ms > 0 and info == info_ref == {"steps": iters, "status": sp.BICG_RAN_ALL, "half_step": 0}
        assert abs(h[0] - h_ref[0]) <= 1e-13 * h_ref[0]
        assert_close(x, x_ref, 1e-7, "25 steps")
        assert np.all(np.abs(h - h_ref) <= 1e-8 * h_ref[0] + 1e-4 * h_ref)
        assert h_ref[-1] < 1e-16 * h_ref[0]                                 # the reference itself converges
        assert true_rr(oracle, row_ptr, col, val, b, x) <= 4.0 * h[-1] + 1e-24 * h[0]
        assert_close(x, x_true, 1e-8, "towards x_true")
        # another product than AUTO's plan: the same loop
        xw, hw, infow, _ = dev.bicgstab(b, 5, variant=sp.CSR_WAVE_ROW)
        assert infow == info5
        assert_close(xw, x_ref5, 1e-10, "wave_row, 5 steps")


def test_bicgstab_fp32_handle(gpu, oracle, banded):
    row_ptr, col, val, x_true, b = banded
    x_ref, h_ref, _ = bicgstab_ref(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, 6)
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        x, h, info, _ = dev32.bicgstab(b.astype(np.float32), 6)
    assert x.dtype == np.float32 and info == {"steps": 6, "status": sp.BICG_RAN_ALL, "half_step": 0}
    assert np.all(np.isfinite(x))
    assert_close(x, x_ref, 1e-4, "fp32")
    assert abs(h[0] - h_ref[0]) <= 1e-6 * h_ref[0]
    assert h[-1] <= 4.0 * h_ref[-1] + 1e-10 * h_ref[0]


def test_bicgstab_is_bit_reproducible(gpu, banded):
    row_ptr, col, val, _, b = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x1, h1, i1, _ = dev.bicgstab(b, 25)
        x2, h2, i2, _ = dev.bicgstab(b, 25)
    assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes() and i1 == i2
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        b32 = b.astype(np.float32)
        x1, h1, _, _ = dev32.bicgstab(b32, 12)
        x2, h2, _, _ = dev32.bicgstab(b32, 12)
    assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes()


def test_bicgstab_tol_stops_early(gpu, oracle):
    """A harder matrix: tol = 1e-8 stops well before the budget; the history is the tol = 0 run's up to the stop and
    repeats after it; x is the tol = 0 iterate of that step; a 50 times larger budget costs no more."""
    rng = np.random.default_rng(77)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.3)
    b = rng.uniform(-1, 1, N)
    tol, iters = 1e-8, 300
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x, h, info, ms = dev.bicgstab(b, iters, tol=tol)
        t = info["steps"]
        assert info["status"] == sp.BICG_CONVERGED and 1 <= t < iters, info
        assert h[t] <= tol * tol * h[0] and np.all(h[1:t] > tol * tol * h[0])
        assert np.all(h[t:] == h[t])
        x0, h0, info0, _ = dev.bicgstab(b, t)                             # tol = 0, stopped at that step
        assert info0["steps"] == t and info0["status"] == sp.BICG_RAN_ALL
        if info["half_step"]:
            assert h0[:t].tobytes() == h[:t].tobytes()
        else:
            assert h0.tobytes() == h[: t + 1].tobytes()
            assert x0.tobytes() == x.tobytes()
        _, _, info_ref = bicgstab_ref(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, iters, tol)
        assert info_ref["status"] == sp.BICG_CONVERGED and abs(info_ref["steps"] - t) <= 2, (info_ref, info)
        assert true_rr(oracle, row_ptr, col, val, b, x) <= 4.0 * h[-1] + 1e-24 * h[0]
        x_big, h_big, info_big, ms_big = dev.bicgstab(b, 50 * iters, tol=tol)
        assert x_big.tobytes() == x.tobytes() and info_big == info
        assert h_big[: iters + 1].tobytes() == h.tobytes() and np.all(h_big[iters:] == h[-1])
        assert ms_big < 5.0 * ms + 2.0, (ms_big, ms)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bicgstab_half_step_convergence(gpu, dtype):
    """First column 4 e1, b = e1: s = r - (1/4) 4 e1 = 0 exactly at step 1, so x = b / 4 at the half step."""
    rng = np.random.default_rng(4)
    n = 50
    dense = rng.uniform(-1, 1, (n, n)) * (rng.uniform(0, 1, (n, n)) < 0.2) + 6.0 * np.eye(n)
    dense[:, 0] = 0.0
    dense[0, 0] = 4.0
    M, row_ptr, col, val = csr_of(dense)
    b = np.zeros(n, dtype=dtype)
    b[0] = 1.0
    with sp.CsrDevice(M, M, row_ptr, col, val.astype(dtype)) as dev:
        for tol in (0.0, 1e-6):
            x, h, info, _ = dev.bicgstab(b, 10, tol=tol)
            assert info == {"steps": 1, "status": sp.BICG_CONVERGED, "half_step": 1}, info
            assert np.array_equal(x, b / 4)
            assert h[0] == 1.0 and np.all(h[1:] == 0.0)
        x, h, info, _ = dev.bicgstab(np.zeros(n, dtype=dtype), 4)          # b = 0: converged at step 0
        assert info == {"steps": 0, "status": sp.BICG_CONVERGED, "half_step": 0}
        assert np.all(x == 0.0) and np.all(h == 0.0)


def test_bicgstab_breakdowns(gpu):
    # r^.v = 0 at step 1: A = [[0, 1], [1, 0]], b = e1
    M, row_ptr, col, val = csr_of([[0.0, 1.0], [1.0, 0.0]])
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        for tol in (0.0, 1e-3):
            x, h, info, _ = dev.bicgstab(np.array([1.0, 0.0]), 6, tol=tol)
            assert info == {"steps": 0, "status": sp.BICG_BREAKDOWN_RHO, "half_step": 0}
            assert np.all(x == 0.0) and np.all(np.isfinite(x)) and np.all(h == 1.0)
    # t.s = 0 at step 2, after a full step 1 (small integers: every value is exact; a small numpy search found it)
    A = [[-1.0, 0.0, 2.0], [-1.0, -1.0, 2.0], [0.0, 0.0, 1.0]]
    b = np.array([0.0, 1.0, 1.0])
    x_ref, h_ref, info_ref = bicgstab_ref(lambda v: np.asarray(A) @ v, b, 5)
    assert info_ref == {"steps": 1, "status": sp.BICG_BREAKDOWN_OMEGA, "half_step": 0}
    M, row_ptr, col, val = csr_of(A)
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        x, h, info, _ = dev.bicgstab(b, 5)
        assert info == info_ref
        assert x.tobytes() == x_ref.tobytes() and h.tobytes() == h_ref.tobytes()
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(h))
    with sp.CsrDevice(M, M, row_ptr, col, val.astype(np.float32)) as dev32:
        x, h, info, _ = dev32.bicgstab(b.astype(np.float32), 5)
        assert info == info_ref and np.array_equal(x, x_ref.astype(np.float32)) and np.array_equal(h, h_ref)


def test_bicgstab_single_rank_communicator_gives_the_same_bits(gpu, banded):
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, _, b = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        plain = dev.bicgstab(b, 25)
        plain_tol = dev.bicgstab(b, 200, tol=1e-10)
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            bounds = np.array([0, N], np.int32)
            x, h, info, _ = dev.bicgstab(b, 25, bounds=bounds)
            assert x.tobytes() == plain[0].tobytes() and h.tobytes() == plain[1].tobytes() and info == plain[2]
            x, h, info, _ = dev.bicgstab(b, 200, tol=1e-10, bounds=bounds)
            assert x.tobytes() == plain_tol[0].tobytes() and h.tobytes() == plain_tol[1].tobytes()
            assert info == plain_tol[2]
            with pytest.raises(RuntimeError, match="bounds"):
                dev.bicgstab(b, 2)                                          # a communicator needs the row bounds
        finally:
            comm.close()


def test_bicgstab_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    row_ptr, col, val, _, b = banded
    rng = np.random.default_rng(5)
    L = sp.lib()
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x = np.zeros(N)
        hist = np.zeros(8)
        info = np.zeros(3, dtype=np.int32)
        ms = C.c_float(0)

        def call(iters, tol):
            return L.spmv_hip_csr_bicgstab(dev.h, sp.CSR_AUTO, iters, tol, None, b.ctypes.data_as(C.c_void_p),
                                           x.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                           info.ctypes.data_as(nat.c_int_p), C.byref(ms))
        # past the Python checks, into the library
        assert call(-1, 0.0) == -1 and b"iters" in L.spmv_hip_last_error()
        for tol in (-1.0, float("nan"), float("inf")):
            assert call(2, tol) == -1 and b"tol" in L.spmv_hip_last_error()
        with pytest.raises(ValueError):
            dev.bicgstab(b, -1)
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(RuntimeError, match="square"):
                rect.bicgstab(np.ones(50), 2)
        with sp.CsrDevice(N, N, row_ptr, col, val, 0, N // 2) as half:   # rows [0, N/2) and no communicator
            with pytest.raises(RuntimeError, match="communicator"):
                half.bicgstab(b, 2)
        # and the handle still computes
        xs = rng.uniform(-1, 1, N)
        y_ref = oracle.csr_serial(row_ptr, col, val, xs)
        assert np.max(np.abs(dev.spmv(xs) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref))
        x5, _, info5, _ = dev.bicgstab(b, 5)
        x_ref5, _, _ = bicgstab_ref(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, 5)
        assert info5["steps"] == 5
        assert_close(x5, x_ref5, 1e-10, "after refusals")


def test_bicgstab_convection_diffusion_million_rows(gpu, oracle):
    """Unsymmetric 5-point convection-diffusion on a 1000 x 1000 grid (10^6 rows, 5 M entries) through AUTO, tol 1e-8:
    it converges well inside the budget and the true residual agrees with the recorded one."""
    row_ptr, col, val = convection_diffusion(1000, 1000, 0.4, 0.2, 0.05)
    M = len(row_ptr) - 1
    b = np.random.default_rng(3).uniform(-1, 1, M)
    tol, iters = 1e-8, 2000
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        x, h, info, ms = dev.bicgstab(b, iters, tol=tol)
    assert info["status"] == sp.BICG_CONVERGED and 0 < info["steps"] < iters, info
    assert ms > 0 and np.all(np.isfinite(x))
    assert h[-1] <= tol * tol * h[0]
    rr = true_rr(oracle, row_ptr, col, val, b, x)
    assert rr <= 4.0 * h[-1] + 1e-20 * h[0], (rr, h[-1], h[0])
