"""spmv_hip_csr_gmres on the GPU: the two Gram-Schmidt passes alone, exactly, at every edge size; the solve against the
numpy restatement of the documented loop (tests/_gmres_ref.py, pinned by tests/test_gmres_host.py) over the oracle's
serial product; bit reproducibility, the stop rules, the exact cases BiCGSTAB cannot solve, power-of-two scaling, every
preconditioner kind, the sizes of the whole solve, and the refused calls."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat

import _amg_ref
from _gmres_ref import gmres_ref
from test_gmres_host import OMEGA_A, OMEGA_B, PERMUTATION, SHIFT
from test_gpu_amg import device_of
from test_gpu_bicgstab import assert_close, convection_diffusion, csr_of, nonsym_banded, true_rr

pytestmark = pytest.mark.gpu

K_BLOCK = 256          # kBlock: csr_kernels.hpp
K_GM_BLOCKS = 1024     # kGmBlocks: gmres_kernels.hpp
N = 6000


def piece(dtype):
    return 16 // np.dtype(dtype).itemsize


def past_the_grid_cap(dtype):
    """one row past the rows one trip of the passes' (and the solver's) grid covers"""
    return K_GM_BLOCKS * K_BLOCK * piece(dtype) + 1


class DevArray:
    """A device copy of a host array of any dtype."""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a)
        self.p = C.c_void_p()
        assert nat.lib().spmv_hip_malloc(C.byref(self.p), max(self.host.nbytes, 16)) == 0
        if self.host.nbytes:
            assert nat.lib().spmv_hip_memcpy_h2d(self.p, self.host.ctypes.data_as(C.c_void_p), self.host.nbytes) == 0

    @property
    def addr(self):
        return self.p.value

    def get(self):
        out = np.empty_like(self.host)
        if out.nbytes:
            assert nat.lib().spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes) == 0
        return out

    def free(self):
        nat.lib().spmv_hip_free(self.p)


# ---------------------------------------------------------------- 1. the passes, exactly
def pass_sizes(dtype):
    v = piece(dtype)
    return sorted({1, v - 1, v, v + 1, 63, 64, 65, 255, 256, 257, 1000, past_the_grid_cap(dtype)})


PASS_CASES = [(dt, n) for dt in (np.float64, np.float32) for n in pass_sizes(dt)]


@pytest.mark.parametrize("dtype,n", PASS_CASES, ids=[f"{np.dtype(d).name}-{n}" for d, n in PASS_CASES])
def test_passes_are_exact_on_small_integers(gpu, dtype, n):
    """Basis and w in [-3, 3], the update's h in [-2, 2]: every sum is exact in any order, so the dots, the updated w
    and w.w equal numpy's integer results bit for bit.  The ld - n elements behind every basis vector hold NaN in one
    run and 0 in the other: they are never read."""
    v = piece(dtype)
    vb = np.dtype(dtype).itemsize
    big = n > 100000
    dots_nvec = [1, 9] if big else [1, 7, 8, 9, 64]
    update_nvec = [1, 9] if big else [1, 8, 9]
    most = max(dots_nvec)
    ld = (n + v - 1) // v * v + v                                     # whole pieces and a tail of at least one piece
    rng = np.random.default_rng(n)
    basis = rng.integers(-3, 4, (most, n))
    w = rng.integers(-3, 4, n)
    d_w = DevArray(w.astype(dtype))
    d_basis = []
    try:
        for tail in (np.nan, 0.0):
            padded = np.full((most, ld), tail, dtype=dtype)
            padded[:, :n] = basis
            d_basis.append(DevArray(padded))
        for nvec in dots_nvec:
            want = (basis[:nvec] @ w).astype(np.float64)
            for d_v in d_basis:
                got = sp.gmres_dots(d_v.addr, ld, nvec, d_w.addr, n, vb)
                assert got.tobytes() == want.tobytes(), (n, nvec, got[:4], want[:4])
        for nvec in update_nvec:
            h = rng.integers(-2, 3, nvec)
            new_w = w - h @ basis[:nvec]
            assert np.max(np.abs(new_w)) < 2 ** 24
            for d_v in d_basis:
                d_out = DevArray(w.astype(dtype))
                try:
                    ww = sp.gmres_update(d_v.addr, ld, nvec, h.astype(np.float64), d_out.addr, n, vb)
                    assert d_out.get().tobytes() == new_w.astype(dtype).tobytes(), (n, nvec)
                    assert ww == float(new_w @ new_w), (n, nvec, ww)
                    assert sp.gmres_update(d_v.addr, ld, nvec, np.zeros(nvec), d_out.addr, n, vb, want_ww=False) is None
                    assert d_out.get().tobytes() == new_w.astype(dtype).tobytes()
                finally:
                    d_out.free()
    finally:
        for d in d_basis + [d_w]:
            d.free()


def test_passes_refuse_bad_arguments(gpu):
    d = DevArray(np.zeros(64))
    try:
        for args, word in (((0, 8, 1, d.addr, 8, 8), "bad arguments"), ((d.addr, 8, 1, 0, 8, 8), "bad arguments"),
                           ((d.addr, 8, 0, d.addr, 8, 8), "nvec"), ((d.addr, 8, 65, d.addr, 8, 8), "nvec"),
                           ((d.addr, 7, 1, d.addr, 8, 8), "ld"), ((d.addr, 9, 1, d.addr, 8, 8), "16 bytes"),
                           ((d.addr, 10, 1, d.addr, 8, 4), "16 bytes"), ((d.addr + 8, 8, 1, d.addr, 8, 8), "aligned"),
                           ((d.addr, 8, 1, d.addr, 8, 2), "value_bytes")):
            with pytest.raises(RuntimeError, match=word):
                sp.gmres_dots(*args)
            d_V, ld, nvec, d_w, n, vb = args
            with pytest.raises(RuntimeError, match=word):
                sp.gmres_update(d_V, ld, nvec, np.zeros(max(nvec, 0)), d_w, n, vb)
        assert nat.lib().spmv_hip_gmres_dots(C.c_void_p(d.addr), 8, 1, C.c_void_p(d.addr), 8, 8, None) == -1
        assert nat.lib().spmv_hip_gmres_update(C.c_void_p(d.addr), 8, 1, None, C.c_void_p(d.addr), 8, 8, None) == -1
        assert sp.gmres_dots(d.addr, 8, 1, d.addr, 8, 8).tobytes() == np.zeros(1).tobytes()
    finally:
        d.free()


# ---------------------------------------------------------------- 2 - 4. against the restated loop; bits
@pytest.fixture(scope="module")
def banded(oracle):
    """the fixture of test_gpu_bicgstab.py, with the restated loop's runs computed once"""
    rng = np.random.default_rng(909)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.5)
    x_true = rng.uniform(-1, 1, N)
    b = oracle.csr_serial(row_ptr, col, val, x_true)
    spmv = lambda v: oracle.csr_serial(row_ptr, col, val, v)  # noqa: E731
    refs = {(iters, restart): gmres_ref(spmv, b, iters, restart=restart) for iters, restart in ((5, 30), (25, 10), (6, 30))}
    return row_ptr, col, val, b, refs


def test_gmres_matches_the_restated_loop_fp64(gpu, oracle, banded):
    """test_gpu_bicgstab.py's tolerances for the same comparison of its loop; the order of the dot products alone moves
    the restated loop by 1.0e-15 of max |x| and 7.9e-15 of the history at 5 steps, 6.7e-16 and 2.9e-12 at 25
    (tests/test_gmres_host.py), a hundred times below every bound here."""
    row_ptr, col, val, b, refs = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x5, h5, info5, ms = dev.gmres(b, 5, restart=30)
        x_ref5, h_ref5, info_ref5 = refs[5, 30]
        assert ms > 0 and info5 == info_ref5 == {"steps": 5, "status": sp.GMRES_RAN_ALL, "cycles": 1}
        assert x5.dtype == np.float64 and h5.shape == (6,)
        print(f"5 steps: x {np.max(np.abs(x5 - x_ref5)) / np.max(np.abs(x_ref5)):.3e}, "
              f"hist {np.max(np.abs(h5 - h_ref5) / h_ref5):.3e}")
        assert_close(x5, x_ref5, 1e-10, "5 steps")
        assert np.all(np.abs(h5 - h_ref5) <= 1e-10 * h_ref5)
        x, h, info, _ = dev.gmres(b, 25, restart=10)
        x_ref, h_ref, info_ref = refs[25, 10]
        assert info == info_ref == {"steps": 25, "status": sp.GMRES_RAN_ALL, "cycles": 3}
        print(f"25 steps: x {np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)):.3e}, "
              f"hist {np.max(np.abs(h - h_ref) / (1e-8 * h_ref[0] + 1e-4 * h_ref)):.3e} of its bound")
        assert_close(x, x_ref, 1e-7, "25 steps")
        assert np.all(np.abs(h - h_ref) <= 1e-8 * h_ref[0] + 1e-4 * h_ref)
        assert true_rr(oracle, row_ptr, col, val, b, x) <= 4.0 * h[-1] + 1e-24 * h[0]
        # another product than AUTO's plan: the same loop
        xw, hw, infow, _ = dev.gmres(b, 5, restart=30, variant=sp.CSR_WAVE_ROW)
        assert infow == info5
        assert_close(xw, x_ref5, 1e-10, "wave_row, 5 steps")
        assert np.all(np.abs(hw - h_ref5) <= 1e-10 * h_ref5)


def test_gmres_fp32_handle(gpu, banded):
    row_ptr, col, val, b, refs = banded
    x_ref, h_ref, _ = refs[6, 30]
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        x, h, info, _ = dev32.gmres(b.astype(np.float32), 6)
    assert x.dtype == np.float32 and info == {"steps": 6, "status": sp.GMRES_RAN_ALL, "cycles": 1}
    assert np.all(np.isfinite(x))
    assert_close(x, x_ref, 1e-4, "fp32")
    assert abs(h[0] - h_ref[0]) <= 1e-6 * h_ref[0]
    assert h[-1] <= 4.0 * h_ref[-1] + 1e-10 * h_ref[0]


def unit_diagonal(row_ptr, col, val):
    """the rows scaled so that the diagonal is exactly 1: Jacobi's D^-1 r is r"""
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    diag = rows == col
    d = np.zeros(len(row_ptr) - 1)
    d[rows[diag]] = val[diag]
    unit = val / d[rows]
    unit[diag] = 1.0
    return unit


def test_gmres_bits(gpu, banded):
    row_ptr, col, val, b, _ = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x1, h1, i1, _ = dev.gmres(b, 25, restart=10)
        x2, h2, i2, _ = dev.gmres(b, 25, restart=10)
        assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes() and i1 == i2
        # a dot product's order depends on n alone: a wider basis that is never filled changes nothing
        x8, h8, i8, _ = dev.gmres(b, 8, restart=8)
        x30, h30, i30, _ = dev.gmres(b, 8, restart=30)
        assert x8.tobytes() == x30.tobytes() and h8.tobytes() == h30.tobytes() and i8 == i30
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        b32 = b.astype(np.float32)
        x1, h1, _, _ = dev32.gmres(b32, 12, restart=5)
        x2, h2, _, _ = dev32.gmres(b32, 12, restart=5)
        assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes()
    with sp.CsrDevice(N, N, row_ptr, col, unit_diagonal(row_ptr, col, val)) as dev, dev.preconditioner("jacobi") as J:
        plain = dev.gmres(b, 25, restart=10)
        jac = dev.gmres(b, 25, restart=10, precond=J)
        assert plain[0].tobytes() == jac[0].tobytes() and plain[1].tobytes() == jac[1].tobytes() and plain[2] == jac[2]


# ---------------------------------------------------------------- 5. the stop rules
def test_gmres_stop_rules(gpu, oracle):
    rng = np.random.default_rng(77)
    row_ptr, col, val = nonsym_banded(rng, N, 7, 60, 0.3)
    b = rng.uniform(-1, 1, N)
    tol, iters, restart = 1e-8, 300, 20
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x, h, info, ms = dev.gmres(b, iters, tol=tol, restart=restart)
        t = info["steps"]
        assert info["status"] == sp.GMRES_CONVERGED and 1 <= t < iters, info
        assert info["cycles"] == -(-t // restart)
        assert h[t] <= tol * tol * h[0] and np.all(h[1:t] > tol * tol * h[0])
        assert np.all(h[t:] == h[t])
        i = np.arange(len(h) - 1)
        inside = i % restart != 0
        assert np.all(h[1:][inside] <= h[:-1][inside])                    # exact: |s| <= 1
        _, _, info_ref = gmres_ref(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, iters, tol, restart)
        assert info_ref["status"] == sp.GMRES_CONVERGED and abs(info_ref["steps"] - t) <= 2, (info_ref, info)
        assert true_rr(oracle, row_ptr, col, val, b, x) <= 4.0 * h[-1] + 1e-24 * h[0]
        x_big, h_big, info_big, _ = dev.gmres(b, 50 * iters, tol=tol, restart=restart)
        assert x_big.tobytes() == x.tobytes() and info_big == info
        assert h_big[: iters + 1].tobytes() == h.tobytes() and np.all(h_big[iters:] == h[-1])


# ---------------------------------------------------------------- 6. the exact cases of the host test
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gmres_exact_cases(gpu, dtype):
    def solve(a, b, iters, **kw):
        m, row_ptr, col, val = csr_of(a)
        with sp.CsrDevice(m, m, row_ptr, col, val.astype(dtype)) as dev:
            return dev.gmres(np.asarray(b, dtype=dtype), iters, **kw)[:3]
    # the permutation BiCGSTAB leaves at step 0 with BREAKDOWN_RHO
    x, h, info = solve(PERMUTATION, [1.0, 0.0], 6, restart=4)
    assert info == {"steps": 2, "status": sp.GMRES_CONVERGED, "cycles": 1}
    assert np.array_equal(x, [0.0, 1.0]) and np.array_equal(h, [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    b = np.ones(4)
    x, h, info = solve(4.0 * np.eye(4), b, 3, restart=5)
    assert info == {"steps": 1, "status": sp.GMRES_CONVERGED, "cycles": 1}
    assert h[0] == 4.0 and np.all(h[1:] == 0.0) and np.array_equal(x, b / 4)
    x, h, info = solve(4.0 * np.eye(4), np.zeros(4), 3)
    assert info == {"steps": 0, "status": sp.GMRES_CONVERGED, "cycles": 0} and np.all(x == 0.0) and np.all(h == 0.0)
    x, h, info = solve(4.0 * np.eye(4), b, 0)
    assert info == {"steps": 0, "status": sp.GMRES_RAN_ALL, "cycles": 1} and np.all(x == 0.0) and np.array_equal(h, [4.0])
    for tol in (0.0, 1e-3):
        x, h, info = solve(SHIFT, [1.0, 0.0, 0.0], 5, restart=4, tol=tol)
        assert info == {"steps": 0, "status": sp.GMRES_BREAKDOWN, "cycles": 1}
        assert np.all(x == 0.0) and np.all(h == 1.0)
        x, h, info = solve(SHIFT, [0.0, 0.0, 1.0], 5, restart=4, tol=tol)
        assert info == {"steps": 2, "status": sp.GMRES_BREAKDOWN, "cycles": 1}
        assert np.all(x == 0.0) and np.all(h == 1.0)
    if dtype == np.float64:
        # the matrix BiCGSTAB leaves at step 1 with BREAKDOWN_OMEGA
        x, h, info = solve(OMEGA_A, OMEGA_B, 6, restart=3, tol=1e-12)
        assert info == {"steps": 3, "status": sp.GMRES_CONVERGED, "cycles": 1}
        assert np.max(np.abs(x - [2.0, -1.0, 1.0])) <= 1e-12
        x, h, info = solve(4.0 * np.eye(4), [1.0, np.nan, 0.0, 0.0], 3)
        assert info == {"steps": 0, "status": sp.GMRES_BREAKDOWN, "cycles": 0} and np.all(x == 0.0)


# ---------------------------------------------------------------- 7. scaling
def test_gmres_power_of_two_scaling(gpu, banded):
    row_ptr, col, val, b, _ = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev, dev.preconditioner("jacobi") as J:
        for P in (None, J):
            x, h, info, _ = dev.gmres(b, 25, restart=10, precond=P)
            xs, hs, infos, _ = dev.gmres(b * 2.0 ** 7, 25, restart=10, precond=P)
            assert info == infos
            assert xs.tobytes() == (x * 2.0 ** 7).tobytes() and hs.tobytes() == (h * 4.0 ** 7).tobytes()


# ---------------------------------------------------------------- 8. every kind
def kind_case(kind):
    """(row_ptr, col, val, b, preconditioner arguments): the nonsymmetric system on which the kind's own test file runs
    bicgstab with it"""
    if kind in ("jacobi", "block_jacobi"):                                # test_gpu_precond.py
        rng = np.random.default_rng(31)
        rp, col, val = nonsym_banded(rng, 4000, 7, 40, 0.3)
        return rp, col, val, rng.uniform(-1, 1, 4000), {"block": 3 if kind == "block_jacobi" else 1}
    if kind in ("ilu0", "ssor"):                                          # test_gpu_trsv.py
        rp, col, val = nonsym_banded(np.random.default_rng(31), 4000, 7, 40, 0.3)
        return rp, col, val, np.random.default_rng(31).uniform(-1, 1, 4000), {"omega": 1.0}
    if kind == "fsai":                                                    # test_gpu_fsai.py
        rp, col, val = convection_diffusion(64, 64, 0.4, 0.2, 0.005)
        return rp, col, val, np.random.default_rng(31).uniform(-1, 1, 64 * 64), {}
    a = _amg_ref.convection_diffusion(40).tocsr()                         # test_gpu_amg.py, test_gpu_chebyshev.py
    a.sort_indices()
    rp, col, val = a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)
    if kind == "amg":
        return rp, col, val, np.random.default_rng(40).standard_normal(a.shape[0]), {}
    return rp, col, val, np.random.default_rng(0).uniform(-1, 1, a.shape[0]), {"degree": 4}


@pytest.mark.parametrize("kind", ["jacobi", "block_jacobi", "ssor", "ilu0", "fsai", "amg", "chebyshev"])
def test_gmres_with_every_kind(gpu, oracle, kind):
    """5 steps against the restated loop with the device's own apply standing in for M^-1 (so the loop is what is
    tested), at the tolerances of the unpreconditioned comparison; tol 1e-8 converges with the true residual the
    recurrence promises."""
    rp, col, val, b, kw = kind_case(kind)
    n = len(b)
    with sp.CsrDevice(n, n, rp, col, val) as dev, dev.preconditioner(kind, **kw) as P:
        x, h, info, _ = dev.gmres(b, 5, restart=30, precond=P)
        x_ref, h_ref, info_ref = gmres_ref(lambda v: oracle.csr_serial(rp, col, val, v), b, 5, restart=30, minv=P.apply)
        assert info == info_ref == {"steps": 5, "status": sp.GMRES_RAN_ALL, "cycles": 1}
        print(f"{kind}: x {np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)):.3e}, hist {np.max(np.abs(h - h_ref) / h_ref):.3e}")
        assert_close(x, x_ref, 1e-10, f"{kind}, 5 steps")
        assert np.all(np.abs(h - h_ref) <= 1e-10 * h_ref)
        x, h, info, _ = dev.gmres(b, 600, tol=1e-8, restart=30, precond=P)
        assert info["status"] == sp.GMRES_CONVERGED and 0 < info["steps"] < 600, info
        assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * h[-1] + 1e-24 * h[0]


# ---------------------------------------------------------------- 9. sizes of the whole solve
def tridiagonal(n):
    import scipy.sparse as sps
    a = sps.diags([np.full(max(n - 1, 0), -1.5), np.full(n, 4.0), np.full(max(n - 1, 0), -0.5)], [-1, 0, 1], shape=(n, n), format="csr")
    a.sort_indices()
    return a


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_gmres_sizes(gpu, n):
    a = tridiagonal(n)
    b = np.random.default_rng(n).uniform(-1, 1, n)
    with device_of(a) as dev:
        x, h, info, _ = dev.gmres(b, n + 5, tol=1e-12, restart=64)
    assert info["status"] == sp.GMRES_CONVERGED, info
    assert n > 3 or info["steps"] <= n, info
    assert_close(x, np.linalg.solve(a.toarray(), b), 1e-10, f"n = {n}")


def test_gmres_one_row_past_the_grid_cap(gpu):
    n = past_the_grid_cap(np.float64)
    a = tridiagonal(n)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    x_ref, h_ref, info_ref = gmres_ref(lambda v: a @ v, b, 3, restart=4)
    with device_of(a) as dev:
        x, h, info, _ = dev.gmres(b, 3, restart=4)
    assert info == info_ref == {"steps": 3, "status": sp.GMRES_RAN_ALL, "cycles": 1}
    assert_close(x, x_ref, 1e-10, "past the grid cap")
    assert np.all(np.abs(h - h_ref) <= 1e-10 * h_ref)


# ---------------------------------------------------------------- 10. refusals
def test_gmres_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    """(A tiles-only handle exists only inside an HLL handle and cannot be reached from Python: that refusal of the C
    entry point is not reachable here.)"""
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, b, refs = banded
    rng = np.random.default_rng(5)
    L = sp.lib()
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x = np.zeros(N)
        hist = np.zeros(8)
        info = np.zeros(3, dtype=np.int32)
        ms = C.c_float(0)

        def call(h=None, P=None, restart=30, iters=2, tol=0.0, rhs=b):
            return L.spmv_hip_csr_gmres(dev.h if h is None else h, P, sp.CSR_AUTO, restart, iters, tol,
                                        None if rhs is None else rhs.ctypes.data_as(C.c_void_p),
                                        x.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                        info.ctypes.data_as(nat.c_int_p), C.byref(ms))
        xs = rng.uniform(-1, 1, N)
        y_ref = oracle.csr_serial(row_ptr, col, val, xs)

        def still_works():
            assert np.max(np.abs(dev.spmv(xs) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref))
        # past the Python checks, into the library
        for restart in (0, -1, 65):
            assert call(restart=restart) == -1 and b"restart" in L.spmv_hip_last_error()
            with pytest.raises(ValueError, match="restart"):
                dev.gmres(b, 2, restart=restart)
            still_works()
        assert call(iters=-1) == -1 and b"iters" in L.spmv_hip_last_error()
        still_works()
        for tol in (-1.0, float("nan"), float("inf")):
            assert call(tol=tol) == -1 and b"tol" in L.spmv_hip_last_error()
            with pytest.raises(ValueError, match="tol"):
                dev.gmres(b, 2, tol=tol)
            still_works()
        with pytest.raises(ValueError, match="iters"):
            dev.gmres(b, -1)
        assert call(rhs=None) == -1 and b"bad arguments" in L.spmv_hip_last_error()
        still_works()
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(RuntimeError, match="square"):
                rect.gmres(np.ones(50), 2)
        still_works()
        with sp.CsrDevice(N, N, row_ptr, col, val, 0, N // 2) as half:     # rows [0, N/2)
            with pytest.raises(RuntimeError, match="not the whole matrix"):
                half.gmres(b, 2)
            assert call(h=half.h) == -1 and b"not the whole matrix" in L.spmv_hip_last_error()
            # a preconditioner of other rows, in the words pcg uses
            with half.preconditioner("jacobi") as Ph:
                assert call(P=Ph.h) == -1 and b"the preconditioner covers rows" in L.spmv_hip_last_error()
                with pytest.raises(ValueError, match="the preconditioner covers rows"):
                    dev.gmres(b, 2, precond=Ph)
            still_works()
        with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32, dev32.preconditioner("jacobi") as P32:
            assert call(P=P32.h) == -1 and b"the preconditioner covers rows" in L.spmv_hip_last_error()
            with pytest.raises(ValueError, match="the preconditioner holds"):
                dev.gmres(b, 2, precond=P32)
        still_works()
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            with pytest.raises(RuntimeError, match="a communicator is active"):
                dev.gmres(b, 2)
            assert call() == -1 and b"a communicator is active" in L.spmv_hip_last_error()
        finally:
            comm.close()
        # and the handle still computes
        still_works()
        x5, _, info5, _ = dev.gmres(b, 5)
        assert info5["steps"] == 5
        assert_close(x5, refs[5, 30][0], 1e-10, "after refusals")
