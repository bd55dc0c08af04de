"""The Chebyshev polynomial preconditioner on the GPU (CsrDevice.preconditioner("chebyshev")): degree 1 bit for bit, the
apply against its restatement within an entry-wise running bound (_cheb_ref.apply_with_bound) that tells a 1 % larger
lmax apart, the grid edges of the one-wide and the k-wide pass, the bit identities, every solver that takes it, an
indefinite M as a breakdown, and the whole text of every refusal."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import _amg_ref
import _cheb_ref as ref
import sparsematrixvectormultiplication_amd as sp
from test_gpu_amg import apply_on_device, device_of, shuffled_with_repeats
from test_gpu_lobpcg import assert_eigenpairs
from test_gpu_pcg_multi import DeviceBuffer
from test_gpu_precond import csr
from test_trsv_host import canonical

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


def held(a, dtype):
    """a with its values as a handle of dtype holds them, in fp64"""
    a = sps.csr_matrix(a)
    return sps.csr_matrix((a.data.astype(dtype).astype(np.float64), a.indices, a.indptr), shape=a.shape)


def assert_within_the_running_bound(z, a, r, degree, dtype, what, lmax=None, lmin=None):
    """|device - restatement| <= bound entry by entry on the block a (fp64 values as the device holds them); the same
    comparison with an lmax 1 % larger must fail somewhere (degree > 1: degree 1 is held bit for bit elsewhere)"""
    g = ref.inverse_diagonal(a, dtype)
    lo, hi = ref.interval(a, lmax, lmin)
    r64 = np.asarray(r, dtype=np.float64)
    z_ref, bound = ref.apply_with_bound(a, g, r64, degree, lo, hi, dtype)
    err = np.abs(z.astype(np.float64) - z_ref)
    print(f"{what}: max |z - ref| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, max bound / max |z| = "
          f"{np.max(bound) / np.max(np.abs(z_ref)):.2e}")
    assert np.all(np.isfinite(z)) and np.all(err <= bound), (what, int(np.argmax(err - bound)))
    off_ref, off_bound = ref.apply_with_bound(a, g, r64, degree, lo, 1.01 * hi, dtype)
    assert np.any(np.abs(z.astype(np.float64) - off_ref) > off_bound), f"{what}: the bound does not discriminate"


# ---------------------------------------------------------------- 1. degree 1 is exact
@DTYPES
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
def test_degree_one_is_exact(gpu, dtype, n):
    rng = np.random.default_rng(n)
    a = sps.diags([-rng.uniform(0.1, 1.0, n - 1), rng.uniform(2.5, 4.0, n), -rng.uniform(0.1, 1.0, n - 1)], [-1, 0, 1],
                  format="csr") if n > 1 else sps.csr_matrix(np.array([[2.5]]))
    r = rng.uniform(-1, 1, n).astype(dtype)
    with device_of(a, dtype) as dev, dev.preconditioner("chebyshev", degree=1) as P:
        assert P.info() == {"kind": sp.PRECOND_CHEBYSHEV, "block": 1, "rows": n, "row0": 0,
                            "value_bytes": np.dtype(dtype).itemsize}
        a_held = held(a, dtype)
        info = P.cheb_info()
        assert info["degree"] == 1 and info["products"] == 0 and info["lmax"] == info["gershgorin"] == ref.gershgorin(a_held)
        assert info["lmin"] == info["lmax"] / 30.0
        g = (1.0 / a_held.diagonal()).astype(dtype)
        _, b = sp.chebyshev_coefficients(1, info["lmin"], info["lmax"])
        want = (b[0] * (g.astype(np.float64) * r.astype(np.float64))).astype(dtype)
        assert P.apply(r).tobytes() == want.tobytes()
        R = rng.uniform(-1, 1, (n, 3)).astype(dtype)
        want3 = (b[0] * (g.astype(np.float64)[:, None] * R.astype(np.float64))).astype(dtype)
        assert P.apply_multi(R).tobytes() == want3.tobytes()


# ---------------------------------------------------------------- 2. the apply against the restatement
def band():
    return _amg_ref.spd_band(300, 4, 1)


@DTYPES
@pytest.mark.parametrize("degree", [2, 3, 4, 7])
@pytest.mark.parametrize("name", ["grid_33x31", "band_300", "shuffled_with_repeats", "row_range"])
def test_apply_against_the_restatement(gpu, name, degree, dtype):
    rng = np.random.default_rng(17)
    what = f"{name} degree {degree} {np.dtype(dtype).name}"
    if name == "grid_33x31":
        a = _amg_ref.laplacian(33, 31)
        dev, block = device_of(a, dtype), held(a, dtype)
    elif name == "band_300":
        a = band()
        dev, block = device_of(a, dtype), held(a, dtype)
    elif name == "shuffled_with_repeats":
        a = band()
        rp, col, val = shuffled_with_repeats(a)
        val = val.astype(dtype)
        dev, block = sp.CsrDevice(300, 300, rp, col, val), canonical(rp, col, val.astype(np.float64), 0, 300)
    else:
        m, rp, col, val = csr(band())
        val = val.astype(dtype)
        dev, block = sp.CsrDevice(m, m, rp, col, val, 100, 220), canonical(rp, col, val.astype(np.float64), 100, 120)
    n = block.shape[0]
    r = rng.uniform(-1, 1, n).astype(dtype)
    with dev, dev.preconditioner("chebyshev", degree=degree) as P:
        info = P.cheb_info()
        assert info["lmax"] == info["gershgorin"] == ref.gershgorin(block) and info["lmin"] == info["lmax"] / 30.0, what
        assert info["degree"] == degree and info["products"] == degree - 1 and 0 <= info["plan"] <= 3
        assert info["download_us"] >= 0 and info["upload_us"] > 0
        if name == "row_range":
            assert (P.row0, P.rows) == (100, 120)
        z = P.apply(r)
        assert z.dtype == dtype
        assert_within_the_running_bound(z, block, r, degree, dtype, what)
    if name == "band_300" and degree == 4:     # explicit bounds are taken as given, and reported beside the bound
        with device_of(band(), dtype) as dev2, dev2.preconditioner("chebyshev", lmax=1.7, lmin=0.2) as P2:
            info = P2.cheb_info()
            assert (info["lmin"], info["lmax"], info["gershgorin"]) == (0.2, 1.7, ref.gershgorin(block))
            assert_within_the_running_bound(P2.apply(r), block, r, 4, dtype, what + " explicit", lmax=1.7, lmin=0.2)


# ---------------------------------------------------------------- 3. grid edges
def tridiagonal(n):
    i = np.arange(n)
    return sps.diags([-(0.3 + 0.1 * (i[1:] % 5)), 2.5 + 0.25 * (i % 7), -(0.2 + 0.1 * (i[1:] % 3))], [-1, 0, 1], format="csr")


def test_one_wide_grid_edge(gpu):
    """2 * 2048 * 256 + 5 rows in fp64: more pieces than the capped grid's lanes, so lanes take a second trip, and the
    last piece is cut"""
    n = 2 * 2048 * 256 + 5
    a = tridiagonal(n)
    r = np.random.default_rng(5).uniform(-1, 1, n)
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=3) as P:
        z = P.apply(r)
        assert_within_the_running_bound(z, a, r, 3, np.float64, "one wide, grid edge")
        assert P.apply(r).tobytes() == z.tobytes()


@pytest.mark.parametrize("n,k,dtype", [(2048 * 64 + 3, 3, np.float64), (300, 8, np.float32), (300, 5, np.float64)],
                         ids=["k3_grid_cap", "k8_f32", "k5_f64"])
def test_k_wide_grid_edges(gpu, n, k, dtype):
    """k = 3: V = 1, four column lanes of which one idles, 64 rows per workgroup and one row more than the capped grid
    takes in a pass; k = 8 fp32: two whole pieces per row; k = 5 fp64: no pieces"""
    a = tridiagonal(n) if n > 300 else band()
    R = np.random.default_rng(k).uniform(-1, 1, (n, k)).astype(dtype)
    with device_of(a, dtype) as dev, dev.preconditioner("chebyshev", degree=3) as P:
        Z = P.apply_multi(R)
        assert_within_the_running_bound(Z, held(a, dtype), R, 3, dtype, f"k = {k}, n = {n}")
        for j in (0, k - 1):     # a column is the one-wide apply up to the bound of either; the values do not depend on k
            zj = P.apply(np.ascontiguousarray(R[:, j]))
            _, bound = ref.apply_with_bound(held(a, dtype), ref.inverse_diagonal(held(a, dtype), dtype),
                                            R[:, j].astype(np.float64), 3, *ref.interval(held(a, dtype)), dtype)
            assert np.all(np.abs(zj.astype(np.float64) - Z[:, j]) <= 2 * bound)


# ---------------------------------------------------------------- 4. bit identities
@DTYPES
def test_bit_identities(gpu, dtype):
    a = _amg_ref.laplacian(33, 31)
    n = a.shape[0]
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, n).astype(dtype)
    L = sp.lib()
    with device_of(a, dtype) as dev, dev.preconditioner("chebyshev") as P, dev.preconditioner("chebyshev") as P2:
        z = P.apply(b)
        assert P.apply(b).tobytes() == z.tobytes() and P2.apply(b).tobytes() == z.tobytes()      # two applies, two builds
        assert P.apply_multi(b.reshape(n, 1)).tobytes() == z.tobytes()                           # k = 1
        assert apply_on_device(P, b.reshape(n, 1), 1).tobytes() == z.tobytes()                   # ... on the device
        with DeviceBuffer(b.nbytes + 128) as d_r, DeviceBuffer(b.nbytes + 128) as d_z:           # apply_on
            assert L.spmv_hip_memcpy_h2d(C.c_void_p(d_r), b.ctypes.data_as(C.c_void_p), b.nbytes) == 0
            P.apply_on(d_r, d_z)
            sp.hip_sync()
            out = np.zeros_like(b)
            assert L.spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(d_z), b.nbytes) == 0
            assert out.tobytes() == z.tobytes()
            # r and z one value off a 16-byte boundary: single values instead of pieces, the same bits
            off = np.dtype(dtype).itemsize
            assert L.spmv_hip_memcpy_h2d(C.c_void_p(d_r + off), b.ctypes.data_as(C.c_void_p), b.nbytes) == 0
            P.apply_on(d_r + off, d_z + off)
            sp.hip_sync()
            assert L.spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(d_z + off), b.nbytes) == 0
            assert out.tobytes() == z.tobytes()
        for k in (2, 3, 8):
            R = rng.uniform(-1, 1, (n, k)).astype(dtype)
            Z = P.apply_multi(R)
            perm = rng.permutation(k)
            assert P.apply_multi(np.ascontiguousarray(R[:, perm])).tobytes() == np.ascontiguousarray(Z[:, perm]).tobytes()
            wb = P.work_bytes(k)
            assert wb == 3 * ((max(n * k * np.dtype(dtype).itemsize, 16) + 127) // 128 * 128 + 128)
            assert apply_on_device(P, R, k).tobytes() == Z.tobytes()      # in a buffer of exactly work_bytes(k)
            for poison in (np.nan, np.inf):                                # reaches no other column
                bad = R.copy()
                bad[n // 2, k // 2] = poison
                Zb = P.apply_multi(bad)
                keep = np.arange(k) != k // 2
                assert Zb[:, keep].tobytes() == Z[:, keep].tobytes() and not np.all(np.isfinite(Zb[:, k // 2]))
        x, hrr, hrz, info, _ = dev.pcg(b, 6, precond=P)
        X, rr, rz, infom, _ = dev.pcg_multi(b.reshape(n, 1), 6, precond=P)                       # k = 1: pcg bit for bit
        assert X[:, 0].tobytes() == x.tobytes() and rr[:, 0].tobytes() == hrr.tobytes() and rz[:, 0].tobytes() == hrz.tobytes()
        assert infom["steps"][0] == info["steps"] and infom["status"][0] == info["status"]
    dev = device_of(a, dtype)
    P = dev.preconditioner("chebyshev")
    R = rng.uniform(-1, 1, (n, 3)).astype(dtype)
    z, Z = P.apply(b), P.apply_multi(R)
    dev.close()                                                           # P works after the handle is closed
    assert P.apply(b).tobytes() == z.tobytes() and P.apply_multi(R).tobytes() == Z.tobytes()
    P.close()


# ---------------------------------------------------------------- 5. solvers
@pytest.fixture(scope="module")
def grid64():
    a = _amg_ref.laplacian(64, 64)
    return a, np.random.default_rng(0).uniform(-1, 1, a.shape[0])


def test_pcg_and_minres_on_the_grid(gpu, grid64):
    a, b = grid64
    tol = 1e-8
    want, want_jacobi = ref.pcg_steps(a, b, 4, tol), ref.pcg_steps(a, b, 0, tol)
    assert (want, want_jacobi) == (52, 193)
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=4) as P, dev.preconditioner("jacobi") as J:
        x, hrr, hrz, info, _ = dev.pcg(b, 500, tol=tol, precond=P)
        jacobi = dev.pcg(b, 2000, tol=tol, precond=J)[3]
        print("pcg steps: chebyshev(4)", info, "restated", want, "jacobi", jacobi)
        assert info["status"] == jacobi["status"] == sp.PCG_CONVERGED
        assert abs(info["steps"] - want) <= 1 and 3 * info["steps"] <= jacobi["steps"]
        assert np.linalg.norm(b - a @ x) <= 10 * tol * np.linalg.norm(b)
        xm, hm, infom, _ = dev.minres(b, 500, tol=tol, precond=P)
        assert infom["status"] == sp.MINRES_CONVERGED and infom["steps"] <= 2 * info["steps"], infom
        assert np.linalg.norm(b - a @ xm) <= 100 * tol * np.linalg.norm(b)


def test_bicgstab_on_convection_diffusion(gpu):
    a = _amg_ref.convection_diffusion(40)
    b = np.random.default_rng(0).uniform(-1, 1, a.shape[0])
    tol = 1e-8
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=4) as P, dev.preconditioner("jacobi") as J:
        x, hist, info, _ = dev.bicgstab(b, 1000, tol=tol, precond=P)
        jacobi = dev.bicgstab(b, 2000, tol=tol, precond=J)[2]
        print("bicgstab steps: chebyshev(4)", info, "jacobi", jacobi)
        assert info["status"] == sp.BICG_CONVERGED and jacobi["status"] == sp.BICG_CONVERGED
        assert 2 * info["steps"] <= jacobi["steps"]
        assert np.linalg.norm(b - a @ x) <= 100 * tol * np.linalg.norm(b)


def test_lobpcg_with_chebyshev(gpu):
    a = _amg_ref.laplacian(48, 48)
    ev = np.linalg.eigvalsh(a.toarray())
    tol, k = 1e-8, 4
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=4) as P, dev.preconditioner("jacobi") as J:
        w, X, th, rh, info, ms = dev.lobpcg(k, 500, tol=tol, precond=P)
        assert info["status"] == sp.LOBPCG_CONVERGED, info
        assert_eigenpairs(a, ev, w, X, info, tol)
        jacobi = dev.lobpcg(k, 2000, tol=tol, precond=J)[4]
        print("lobpcg steps: chebyshev(4)", info["steps"], "jacobi", jacobi["steps"])
        assert jacobi["status"] == sp.LOBPCG_CONVERGED and 3 * info["steps"] <= jacobi["steps"]


def test_pcg_multi_agrees_with_pcg_column_by_column(gpu, grid64):
    a, _ = grid64
    n = a.shape[0]
    B = np.random.default_rng(3).uniform(-1, 1, (n, 3))
    tol = 1e-8
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=4) as P:
        X, rr, rz, info, _ = dev.pcg_multi(B, 500, tol=tol, precond=P)
        for j in range(3):
            x, _, _, one, _ = dev.pcg(np.ascontiguousarray(B[:, j]), 500, tol=tol, precond=P)
            assert info["status"][j] == one["status"] == sp.PCG_CONVERGED and abs(int(info["steps"][j]) - one["steps"]) <= 1
            assert np.linalg.norm(B[:, j] - a @ X[:, j]) <= 10 * tol * np.linalg.norm(B[:, j])


# ---------------------------------------------------------------- 6. an indefinite M is a breakdown, not a NaN
def test_an_indefinite_polynomial_is_a_breakdown(gpu):
    a = _amg_ref.laplacian(16, 16)
    n = a.shape[0]
    i, j = np.divmod(np.arange(n), 16)
    b = (-1.0) ** (i + j)
    lo, hi = ref.interval(a, lmax=0.6)
    rz0 = b @ ref.apply(a, ref.inverse_diagonal(a, np.float64), b, 2, lo, hi)
    assert abs(rz0 + 1560.0) < 0.05                   # r.z < 0 at step 0: M is indefinite
    with device_of(a) as dev, dev.preconditioner("chebyshev", degree=2, lmax=0.6) as P, \
            dev.preconditioner("chebyshev", degree=2) as good:
        x, hrr, hrz, info, _ = dev.pcg(b, 20, tol=1e-8, precond=P)
        assert info["status"] == sp.PCG_BREAKDOWN and info["steps"] == 0, info
        assert np.all(x == 0.0) and np.all(np.isfinite(x))
        assert abs(hrz[0] - rz0) <= 1e-9 * abs(rz0)
        # the handle and P work afterwards
        assert np.max(np.abs(dev.spmv(b) - a @ b)) <= 1e-12 * np.max(np.abs(a @ b))
        assert_within_the_running_bound(P.apply(b), a, b, 2, np.float64, "after the breakdown", lmax=0.6)
        assert dev.pcg(b, 200, tol=1e-8, precond=good)[3]["status"] == sp.PCG_CONVERGED


# ---------------------------------------------------------------- 7. refusals, the whole text
def raw_build(dev, degree=4, lmin=0.0, lmax=0.0, ratio=30.0):
    out = C.c_void_p()
    rc = sp.lib().spmv_hip_csr_precond_build_chebyshev(dev.h, degree, lmin, lmax, ratio, C.byref(out))
    assert (rc == 0) == bool(out)
    if out:
        sp.lib().spmv_hip_precond_free(out)
    return rc, sp.lib().spmv_hip_last_error().decode()


def test_refusals_leave_the_handle_working(gpu):
    a = band()
    n, rp, col, val = csr(a)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    what = "csr_precond_build_chebyshev"
    with device_of(a) as dev:
        def still_works(after):
            assert np.max(np.abs(dev.spmv(x) - a @ x)) <= 1e-12 * np.max(np.abs(a @ x)), after
            assert raw_build(dev)[0] == 0, after

        for kw, text in (({"degree": 0}, f"{what}: degree = 0, must be in [1, 32]"),
                         ({"degree": 33}, f"{what}: degree = 33, must be in [1, 32]"),
                         ({"ratio": 1.0}, f"{what}: ratio = 1, must be finite and > 1"),
                         ({"ratio": float("nan")}, f"{what}: ratio = nan, must be finite and > 1"),
                         ({"lmax": -1.0}, f"{what}: lmax = -1, must be finite and >= 0 (0: the Gershgorin bound)"),
                         ({"lmax": float("inf")}, f"{what}: lmax = inf, must be finite and >= 0 (0: the Gershgorin bound)"),
                         ({"lmin": -0.5}, f"{what}: lmin = -0.5, must be finite and >= 0 (0: lmax / ratio)"),
                         ({"lmin": float("inf")}, f"{what}: lmin = inf, must be finite and >= 0 (0: lmax / ratio)"),
                         ({"lmin": 1.5, "lmax": 1.5}, f"{what}: lmin = 1.5, lmax = 1.5: lmin must be below lmax"),
                         ({"lmin": 4.0}, f"{what}: lmin = 4, lmax = {ref.gershgorin(a):g}: lmin must be below lmax")):
            rc, msg = raw_build(dev, **kw)
            assert rc == -1 and msg == text, (kw, msg)
            still_works(text)
        with dev.preconditioner("chebyshev") as P:
            with pytest.raises(sp.SpmvHipError) as e:
                P.factors()
            assert str(e.value) == "spmv_hip_precond_factors: precond_factors: kind 7 has no factors"
            for method, text in ((P.amg_info, "spmv_hip_precond_amg_info: precond_amg_info: kind 7 is not AMG"),
                                 (P.fsai_info, "spmv_hip_precond_fsai_info: precond_fsai_info: kind 7 is not FSAI"),
                                 (P.tri_info, "spmv_hip_precond_tri_info: precond_tri_info: kind 7 is not made of "
                                              "triangular solves")):
                with pytest.raises(sp.SpmvHipError) as e:
                    method()
                assert str(e.value) == text
            R = rng.uniform(-1, 1, (n, 3))
            with DeviceBuffer(R.nbytes + 128) as d_r, DeviceBuffer(R.nbytes + 128) as d_z:
                with pytest.raises(sp.SpmvHipError) as e:
                    P.apply_multi_on(d_r, d_z, 3)
                assert str(e.value) == ("spmv_hip_precond_apply_multi_on: precond_apply_multi_on: a CHEBYSHEV apply "
                                        "needs d_work (spmv_hip_precond_work_bytes: its three arrays)")
            still_works("the other kinds' readers")
        with dev.preconditioner("jacobi") as J:
            with pytest.raises(sp.SpmvHipError) as e:
                J.cheb_info()
            assert str(e.value) == "spmv_hip_precond_cheb_info: precond_cheb_info: kind 1 is not CHEBYSHEV"
    # a zero, a negative, an infinite and a missing diagonal at row 5 of a row-range handle: the local and the global row
    rows_of = lambda rp: np.repeat(np.arange(len(rp) - 1), np.diff(rp))  # noqa: E731
    for value in (0.0, -2.0, np.inf, None):
        bad = a.tolil()
        bad[105, 105] = 7.0 if value in (None, 0.0) else value
        m, rp, col, val = csr(sps.csr_matrix(bad))
        at = (rows_of(rp) == 105) & (col == 105)
        assert np.count_nonzero(at) == 1
        if value == 0.0:
            val[at] = 0.0                                   # a stored zero
        if value is None:                                   # the entry (105, 105) dropped
            rp = np.concatenate([[0], np.cumsum(np.bincount(rows_of(rp)[~at], minlength=m))]).astype(np.int32)
            col, val = col[~at], val[~at]
        with sp.CsrDevice(m, m, rp, col, val, 100, 220) as part:
            rc, msg = raw_build(part)
            text = f"{what}: row 5 (global row 105) has no diagonal entry" if value is None else \
                f"{what}: row 5 (global row 105): the diagonal is not positive or not finite"
            assert rc == -1 and msg == text, msg
            own = np.setdiff1d(np.arange(100, 220), [105])
            y_ref = sps.csr_matrix((np.where(np.isfinite(val), val, 0.0), col, rp), shape=(m, m)) @ x
            assert np.max(np.abs(part.spmv(x)[own] - y_ref[own])) <= 1e-12 * np.max(np.abs(y_ref))
    m2, rp2 = 10, np.arange(0, 4 * 10 + 1, 4, dtype=np.int32)
    with sp.CsrDevice(m2, 12, rp2, rng.integers(0, 12, 40).astype(np.int32), rng.uniform(1, 2, 40)) as rect:
        rc, msg = raw_build(rect)
        assert rc == -1 and msg == f"{what}: needs a square matrix (10 x 12)", msg
        assert np.all(np.isfinite(rect.spmv(rng.uniform(-1, 1, 12))))
