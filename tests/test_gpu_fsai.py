"""The FSAI preconditioner on the GPU (CsrDevice.preconditioner("fsai")): an exact gate, the factors against a long
double CPU FSAI and against their defining properties, long rows, the apply against long double products on the
returned factors, both solvers against the reference loops of test_gpu_precond.py with M^-1 made of those factors,
lifetimes, row ranges and refusals."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import U32, U64, gamma
from test_fsai_host import fsai_ref, pattern_ref
from test_gpu_bicgstab import assert_close, convection_diffusion, true_rr
from test_gpu_precond import csr, pbicgstab_ref, pcg_ref
from test_gpu_trsv import CASES, _hip, dominant, spd_grid  # noqa: F401 (spd_grid: a fixture)
from test_trsv_host import canonical, grid5

pytestmark = pytest.mark.gpu

LD = np.longdouble
SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 41)   # |S_i| before the cap: every lane width, each boundary, above the cap


def sized(n, sizes, seed):
    """dominant(): row i has min(i, sizes[i % len(sizes)] - 1) entries below the diagonal and a few above it (which
    FSAI does not read)"""
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    a = sps.lil_matrix((n, n))
    for i in range(n):
        k = min(i, sizes[i % len(sizes)] - 1)
        if k:
            a[i, rng.choice(i, k, replace=False)] = rng.uniform(-1, 1, k)
        if i + 1 < n:
            a[i, rng.choice(np.arange(i + 1, n), min(2, n - 1 - i), replace=False)] = rng.uniform(-1, 1, min(2, n - 1 - i))
        a[i, i] = 1.0
    return dominant(a, rng)


def scipy_of(tri, n, real=np.float64):
    import scipy.sparse as sps
    rp, col, val = tri
    return sps.csr_matrix((val.astype(real), col, rp), shape=(n, n))


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def product_ld(rp, col, val, x):
    """(A x, |A| |x|) row by row in long double"""
    y, ay = np.zeros(len(rp) - 1, LD), np.zeros(len(rp) - 1, LD)
    prod = np.asarray(val).astype(LD) * np.asarray(x).astype(LD)[col]
    np.add.at(y, rows_of(rp), prod)
    np.add.at(ay, rows_of(rp), np.abs(prod))
    return y, ay


def minv_of(Gf, Uf, n, ld=False):
    """r -> G^T (G r) from the returned factors, in fp64 (scipy) or in long double"""
    if not ld:
        G, Gt = scipy_of(Gf, n), scipy_of(Uf, n)
        return lambda r: Gt @ (G @ np.asarray(r, np.float64))
    return lambda r: product_ld(*Uf, product_ld(*Gf, r)[0])[0].astype(np.float64)


def symmetric_lower(a):
    """A~: the symmetric matrix whose lower triangle is a's"""
    import scipy.sparse as sps
    low = sps.tril(a, 0, format="csr")
    return (low + sps.tril(a, -1, format="csr").T).tocsr()


def check_factors(M, rp, col, val, cap, dtype, what, row0=0, rows=None, P=None):
    """G against the long double FSAI of the canonical block, entry by entry, within 16 d + eps / 2 relative, d the
    largest relative difference between the same loops in plain fp64 and in long double (printed); G^T the bit-exact
    transpose; the pattern that of the restated rule; and the defining properties on the returned factors within the
    same relative bound carried through the products.  Returns (d, the largest error over the bound)."""
    n = M if rows is None else rows
    val = np.asarray(val).astype(dtype)
    a = canonical(rp, col, val, row0, n)
    g_ptr, g_col, _, counts = pattern_ref(a, cap)
    if P is None:
        with sp.CsrDevice(M, M, rp, col, val, row0, row0 + n) as dev, dev.preconditioner("fsai", cap=cap) as Q:
            Gf, Uf, info = *Q.factors(), Q.fsai_info()
    else:
        Gf, Uf, info = *P.factors(), P.fsai_info()
    assert np.array_equal(Gf[0], g_ptr) and np.array_equal(Gf[1], g_col), what
    assert Gf[2].dtype == dtype and Uf[2].dtype == dtype
    assert (info["cap"], info["entries"], info["truncated_rows"], info["widest"]) == (cap,) + counts[:3], (what, info)
    G = scipy_of(Gf, n)
    Gt = G.T.tocsr()
    Gt.sort_indices()
    assert np.array_equal(Uf[0], Gt.indptr) and np.array_equal(Uf[1], Gt.indices), what
    assert Uf[2].tobytes() == Gt.data.astype(dtype).tobytes(), f"{what}: G^T is not the bit-exact transpose"
    ref, plain = fsai_ref(a, g_ptr, g_col, LD), fsai_ref(a, g_ptr, g_col, np.float64)
    assert np.all(np.isfinite(ref.astype(np.float64))), f"{what}: the reference breaks down"
    nz = ref != 0
    d = float(np.max(np.abs(plain[nz].astype(LD) - ref[nz]) / np.abs(ref[nz]), initial=0.0))
    tau = LD(16.0 * d + 0.5 * np.finfo(dtype).eps)
    err = np.abs(Gf[2].astype(LD) - ref)
    worst = float(np.max(err[nz] / (tau * np.abs(ref[nz])), initial=0.0))
    assert np.all(err <= tau * np.abs(ref)), (what, d, worst)
    # the defining properties: (G A~)_ij = 0 for j in S_i, j != i, and diag(G A~ G^T) = 1, in long double on the
    # returned G; a relative error tau of every entry of G moves (G A~)_ij by tau (|G| |A~|)_ij at most
    at = symmetric_lower(a)
    ga = (scipy_of(Gf, n, LD) @ at.astype(LD)).tocsr()
    aga = (abs(scipy_of(Gf, n, LD)) @ abs(at).astype(LD)).tocsr()
    r = rows_of(g_ptr)
    got = np.asarray(ga[r, g_col]).ravel()
    scale = np.asarray(aga[r, g_col]).ravel()
    off = g_col != r
    prop = float(np.max(np.abs(got[off]) / (tau * scale[off]), initial=0.0))
    assert np.all(np.abs(got[off]) <= tau * scale[off]), (what, prop)
    gv = Gf[2].astype(LD)
    dg, adg = np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(dg, r, got * gv)
    np.add.at(adg, r, scale * np.abs(gv))
    assert np.all(np.abs(dg - 1) <= 2 * tau * adg), (what, float(np.max(np.abs(dg - 1) / (2 * tau * adg))))
    print(f"{what} {np.dtype(dtype)}: fp64 against long double d = {d:.2e}; GPU error / bound = {worst:.3f}, "
          f"(G A~)_ij / bound = {prop:.3f}")
    return d, worst


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_on_scaled_two_by_two_blocks_and_on_a_diagonal(gpu, dtype):
    """blocks 4^k [[4, 2], [2, 2]]: C = 2^k [[2, 0], [1, 1]], G = 2^-k [[1/2, 0], [-1/2, 1]] and G^T G = A^-1, all
    exact; apply of small integers is the exact solve bit for bit.  A diagonal matrix 4^k gives Jacobi's bytes."""
    import scipy.sparse as sps
    nb = 67
    k = np.random.default_rng(1).integers(-6, 7, nb)
    a = sps.block_diag([np.array([[4.0, 2.0], [2.0, 2.0]]) * 4.0 ** int(e) for e in k]).tocsr()
    M, rp, col, val = csr(a)
    r = np.random.default_rng(2).integers(-8, 9, M).astype(dtype)
    with sp.CsrDevice(M, M, rp, col, val.astype(dtype)) as dev, dev.preconditioner("fsai") as P:
        assert P.info() == {"kind": sp.PRECOND_FSAI, "block": 1, "rows": M, "row0": 0,
                            "value_bytes": np.dtype(dtype).itemsize}
        (grp, gcol, gval), (urp, ucol, uval) = P.factors()
        z = P.apply(r)
        assert P.fsai_info()["widest"] == 2 and P.fsai_info()["truncated_rows"] == 0
    s = np.repeat(2.0 ** -k.astype(np.float64), 3)
    assert list(grp) == [0] + [v for b in range(nb) for v in (3 * b + 1, 3 * b + 3)]
    assert list(gcol) == [v for b in range(nb) for v in (2 * b, 2 * b, 2 * b + 1)]
    assert gval.tobytes() == (np.tile([0.5, -0.5, 1.0], nb) * s).astype(dtype).tobytes()
    assert list(ucol) == [v for b in range(nb) for v in (2 * b, 2 * b + 1, 2 * b + 1)]
    assert uval.tobytes() == (np.tile([0.5, -0.5, 1.0], nb) * s).astype(dtype).tobytes()
    z_exact = np.linalg.solve(a.toarray(), r.astype(np.float64))          # dyadic rationals: exact in either dtype
    assert np.array_equal((scipy_of((grp, gcol, gval), M).T @ scipy_of((grp, gcol, gval), M)).toarray(),
                          np.linalg.inv(a.toarray()))
    assert (z + 0.0).tobytes() == (z_exact.astype(dtype) + 0.0).tobytes()          # (+ 0.0: -0 and +0 are one number)
    n = 130
    d = (4.0 ** np.random.default_rng(3).integers(-5, 6, n)).astype(dtype)
    rp, col = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    r = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)
    with sp.CsrDevice(n, n, rp, col, d) as dev, dev.preconditioner("fsai", cap=1) as P, \
            dev.preconditioner("fsai") as P32, dev.preconditioner("jacobi") as J:
        assert P.apply(r).tobytes() == J.apply(r).tobytes() == P32.apply(r).tobytes()
        assert P.factors()[0][2].tobytes() == (1.0 / np.sqrt(d.astype(np.float64))).astype(dtype).tobytes()


# ---------------------------------------------------------------- the factors
FACTOR_CASES = {"1 row": (1, SIZES), "2 rows": (2, SIZES), "63 rows": (63, SIZES), "64 rows": (64, SIZES),
                "65 rows": (65, SIZES), "150 rows, every width": (150, SIZES),
                "65 rows of 32": (97, (32,)), "33 rows of 16 and of 17": (98, (16, 17)), "70 rows of 3": (72, (3,))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(FACTOR_CASES))
def test_factors_match_the_long_double_fsai(gpu, name, dtype):
    """Row sizes 1, 2, 3, 4, 5, 8, 9, 16, 17, 32 and 41 (cut to the cap), in matrices of 1, 2, 63, 64, 65 and 150 rows,
    and whole classes of one lane width whose last workgroup is partly filled.  Tolerance per entry, relative:
    16 d + eps / 2 with d the largest relative difference between the reference loops in plain fp64 and in long double.
    Measured on the MI355X: d = 3.2e-18 (1 row) to 3.4e-14 over the mixed cases and 3.2e-12 for the 65 rows of 32; the
    GPU's error is at most 0.47 of the bound in fp64 and 0.97 of it in fp32, where eps / 2, the rounding to the dtype
    itself, is nearly all of the bound; (G A~)_ij on the pattern at most 0.03 (fp64) and 0.74 (fp32) of its bound."""
    n, sizes = FACTOR_CASES[name]
    M, rp, col, val = sized(n, sizes, 100 + n)
    check_factors(M, rp, col, val, 32, dtype, name)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cap", [32, 2])
def test_factors_of_the_five_point_grid(gpu, cap, dtype):
    """grid5(24, 0.05), the capped pattern too.  Measured: d = 5.2e-17 (fp64 data) and 3.5e-16 (fp32 data), the GPU's
    error 0.055 and 0.39 of the bound."""
    M, rp, col, val = csr(grid5(24, 0.05))
    check_factors(M, rp, col, val, cap, dtype, f"grid5 cap {cap}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_long_rows_keep_their_largest_entries(gpu, dtype):
    """rows of about 4000 entries: the cap keeps the 31 largest below the diagonal, and the local matrices are gathered
    by searches in rows that long.  Measured: d = 7.6e-16 and 1.0e-15, the GPU's error 0.054 (fp64) and 0.99 (fp32) of
    the bound."""
    M, rp, col, val = CASES["long rows"]
    a = canonical(rp, col, val.astype(dtype), 0, M)
    g_ptr, g_col, _, counts = pattern_ref(a, 32)
    assert counts[1] >= 2 and counts[2] == 32
    for i in (5997, 5998):
        low = np.flatnonzero(a.indices[a.indptr[i]:a.indptr[i + 1]] < i)
        kept = g_col[g_ptr[i]:g_ptr[i + 1] - 1]
        assert len(low) > 3000 and len(kept) == 31
        mags = np.abs(a.data[a.indptr[i]:a.indptr[i + 1]][low])
        assert np.min(np.abs(np.asarray(a[i, kept].todense()))) >= np.sort(mags)[-31]
    check_factors(M, rp, col, val, 32, dtype, "long rows")


# ---------------------------------------------------------------- the apply
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["150 rows, every width", "grid", "long rows"])
def test_apply_is_the_two_products_on_the_returned_factors(gpu, name, dtype):
    """t = G r and z = G^T t against long double products on the returned factors, row by row.  Each product is held
    to the row-wise bound of the SpMV tests (fp64: 1e-10 sum |a_ij x_j|; fp32: (gamma32(n_i) + gamma64(n_i)) sum
    |a_ij x_j|), taken at the t the device computed from; the second carries the first's bound through |G^T|."""
    M, rp, col, val = sized(150, SIZES, 250) if name.startswith("150") else CASES[name]
    val = val.astype(dtype)
    r = np.random.default_rng(6).uniform(-1, 1, M).astype(dtype)
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("fsai") as P:
        z = P.apply(r)
        Gf, Uf = P.factors()
        assert P.apply(r).tobytes() == z.tobytes()
        with dev.preconditioner("fsai") as P2:                       # two builds: the same bytes
            assert all(u.tobytes() == v.tobytes() for f, g in zip(P2.factors(), (Gf, Uf)) for u, v in zip(f, g))
            assert P2.apply(r).tobytes() == z.tobytes()

    def bound(rp_, sums):
        n = np.diff(rp_.astype(np.int64))
        if dtype == np.float64:
            return LD(1e-10) * sums
        return (gamma(n, U32) + gamma(n, U64)).astype(LD) * sums * (1.0 + 4.0 * gamma(n + 2, U64))
    t_ref, at = product_ld(*Gf, r)
    e1 = bound(Gf[0], at)
    z_ref, az = product_ld(*Uf, t_ref)
    # |z - G^T t_ref| <= bound at the device's t (within e1 of t_ref: |t| <= |t_ref| + e1) + |G^T| e1
    carried = product_ld(Uf[0], Uf[1], np.abs(Uf[2]), e1)[0]
    e2 = bound(Uf[0], az + carried) + carried
    err = np.abs(z.astype(LD) - z_ref)
    print(f"{name} {np.dtype(dtype)}: max error / bound = {float(np.max(err / np.maximum(e2, LD(1e-4000)))):.3e}")
    assert z.dtype == dtype and np.all(np.isfinite(z)) and np.all(err <= e2), float(np.max(err / e2))


def test_apply_on_a_second_stream_between_sentinels(gpu):
    M, rp, col, val = csr(grid5(40, 0.05))
    r = np.random.default_rng(9).uniform(-1, 1, M)
    L, hip = sp.lib(), _hip()
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("fsai") as P:
        z = P.apply(r)
        pad = 256                                     # doubles of sentinel on either side; r and z stay 128-byte aligned
        buf = np.full(2 * pad + M, -77.25)
        stream, dr, dz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        assert L.spmv_hip_malloc(C.byref(dr), buf.nbytes) == 0 and L.spmv_hip_malloc(C.byref(dz), buf.nbytes) == 0
        assert L.spmv_hip_memcpy_h2d(dz, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
        buf[pad:pad + M] = r
        assert L.spmv_hip_memcpy_h2d(dr, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
        P.apply_on(dr.value + 8 * pad, dz.value + 8 * pad, stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        got, src = np.empty_like(buf), np.empty_like(buf)
        assert L.spmv_hip_memcpy_d2h(got.ctypes.data_as(C.c_void_p), dz, buf.nbytes) == 0
        assert L.spmv_hip_memcpy_d2h(src.ctypes.data_as(C.c_void_p), dr, buf.nbytes) == 0
        assert got[pad:pad + M].tobytes() == z.tobytes()
        assert np.all(got[:pad] == -77.25) and np.all(got[pad + M:] == -77.25) and src.tobytes() == buf.tobytes()
        hip.hipStreamDestroy(stream), L.spmv_hip_free(dr), L.spmv_hip_free(dz)


# ---------------------------------------------------------------- in the solvers
def cpu_runs_differ(run, minv64, minv_ld):
    """the reference loop with M^-1 in fp64 and in long double: (largest |x - x'| / max |x|, largest history
    difference / first entry)"""
    a, b = run(minv64), run(minv_ld)
    return (float(np.max(np.abs(a[0] - b[0])) / np.max(np.abs(a[0]))),
            max(float(np.max(np.abs(u - v)) / u[0]) for u, v in zip(a[1:-1], b[1:-1])))


def test_pcg_matches_the_reference_loop(gpu, oracle, spd_grid):  # noqa: F811
    """spd_grid of test_gpu_trsv.py, the block-Jacobi tolerances (5 steps 1e-10, 25 steps 1e-7), M^-1 of the reference
    loop made of the returned factors.  The loop run twice on the CPU, M^-1 in fp64 and in long double, differs by
    2.4e-16 of max |x| and 2.8e-14 of the first r.r or r.z at 5 steps, 3.8e-16 and 2.8e-14 at 25 (measured, printed and
    asserted below a tenth of the tolerance), so both tolerances stay."""
    M, rp, col, val, b = spd_grid
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("fsai") as P:
        Gf, Uf = P.factors()
        minv = minv_of(Gf, Uf, M)
        for iters, rtol in ((5, 1e-10), (25, 1e-7)):
            dx, dh = cpu_runs_differ(lambda mv: pcg_ref(spmv, mv, b, iters), minv, minv_of(Gf, Uf, M, ld=True))
            print(f"pcg {iters} steps: the two CPU runs differ by {dx:.2e} of max |x|, {dh:.2e} of the first r.r")
            assert dx <= rtol / 10 and dh <= rtol / 10
            x, hrr, hrz, info, ms = dev.pcg(b, iters, precond=P)
            x_ref, hrr_ref, hrz_ref, info_ref = pcg_ref(spmv, minv, b, iters)
            assert info == info_ref == {"steps": iters, "status": sp.PCG_RAN_ALL} and ms > 0
            assert_close(x, x_ref, rtol, f"fsai {iters} steps")
            assert np.all(np.abs(hrz - hrz_ref) <= rtol * hrz_ref[0] + 1e-6 * hrz_ref)
            assert np.all(np.abs(hrr - hrr_ref) <= rtol * hrr_ref[0] + 1e-6 * hrr_ref)
        assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * hrr[-1] + 1e-20 * hrr[0]
        again = dev.pcg(b, 25, precond=P)
        assert again[0].tobytes() == x.tobytes() and again[1].tobytes() == hrr.tobytes()


def test_pbicgstab_matches_the_reference_loop(gpu, oracle):
    """convection_diffusion(64, 64, 0.4, 0.2, 0.005) with the (steps, x tolerance, history tolerance) triples and the
    history expression of the block-Jacobi test.  The two CPU runs differ by 3.0e-15 of max |x| and 2.8e-14 of the
    first r.r at 5 steps, 1.0e-12 and 2.8e-14 at 20 (measured, printed, asserted below a tenth of the tolerances)."""
    g = 64
    rp, col, val = convection_diffusion(g, g, 0.4, 0.2, 0.005)
    M = g * g
    b = np.random.default_rng(31).uniform(-1, 1, M)
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("fsai") as P:
        Gf, Uf = P.factors()
        minv = minv_of(Gf, Uf, M)
        for iters, rtol, htol in ((5, 1e-10, 1e-8), (20, 1e-7, 1e-4)):
            dx, dh = cpu_runs_differ(lambda mv: pbicgstab_ref(spmv, mv, b, iters), minv, minv_of(Gf, Uf, M, ld=True))
            print(f"bicgstab {iters} steps: the two CPU runs differ by {dx:.2e} of max |x|, {dh:.2e} of the first r.r")
            assert dx <= rtol / 10 and dh <= htol * 1e-4 / 10
            x, h, info, ms = dev.bicgstab(b, iters, precond=P)
            x_ref, h_ref, info_ref = pbicgstab_ref(spmv, minv, b, iters)
            assert info == info_ref, (info, info_ref)
            assert_close(x, x_ref, rtol, f"fsai {iters} steps")
            assert np.all(np.abs(h - h_ref) <= htol * (h_ref[0] * 1e-4 + h_ref))
        again = dev.bicgstab(b, 20, precond=P)
        assert again[0].tobytes() == x.tobytes() and again[1].tobytes() == h.tobytes()


def test_convergence_beats_jacobi(gpu, oracle):
    """tol 1e-8 on grid5(64, 0.005) (PCG) and convection_diffusion(64, 64, 0.4, 0.2, 0.005) (BiCGSTAB): converged,
    within one step of the reference loop, the true residual as the recurrence says, and FSAI takes strictly fewer steps
    than Jacobi (the reference loops alone: 95 against 179 and 56 against 94)."""
    g, tol = 64, 1e-8
    b = np.random.default_rng(3).uniform(-1, 1, g * g)
    M, rp, col, val = csr(grid5(g, 0.005))
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("jacobi") as J, dev.preconditioner("fsai") as P:
        jacobi = dev.pcg(b, 2000, tol=tol, precond=J)[3]["steps"]
        x, hrr, _, info, _ = dev.pcg(b, 2000, tol=tol, precond=P)
        info_ref = pcg_ref(spmv, minv_of(*P.factors(), M), b, 2000, tol)[3]
    print("pcg steps: fsai", info, "reference", info_ref, "jacobi", jacobi)
    assert info["status"] == sp.PCG_CONVERGED and abs(info["steps"] - info_ref["steps"]) <= 1, (info, info_ref)
    assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * hrr[-1] + 1e-20 * hrr[0]
    assert info["steps"] < jacobi
    rp, col, val = convection_diffusion(g, g, 0.4, 0.2, 0.005)
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("jacobi") as J, dev.preconditioner("fsai") as P:
        jacobi = dev.bicgstab(b, 2000, tol=tol, precond=J)[2]["steps"]
        x, h, info, _ = dev.bicgstab(b, 2000, tol=tol, precond=P)
        info_ref = pbicgstab_ref(spmv, minv_of(*P.factors(), M), b, 2000, tol)[2]
    print("bicgstab steps: fsai", info, "reference", info_ref, "jacobi", jacobi)
    assert info["status"] == sp.BICG_CONVERGED and abs(info["steps"] - info_ref["steps"]) <= 1, (info, info_ref)
    assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * h[-1] + 1e-20 * h[0]
    assert info["steps"] < jacobi


def test_solver_identities(gpu, spd_grid):  # noqa: F811
    """tol > 0 and tol = 0 agree up to the stop, after which x no longer changes and the histories repeat; a P of other
    rows or dtype is refused; fp32 runs"""
    M, rp, col, val, b = spd_grid
    tol, iters = 1e-6, 500
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("fsai") as P:
        x, hrr, hrz, info, _ = dev.pcg(b, iters, tol=tol, precond=P)
        t = info["steps"]
        assert info["status"] == sp.PCG_CONVERGED and 1 <= t < iters
        assert hrr[t] <= tol * tol * hrr[0] and np.all(hrr[1:t] > tol * tol * hrr[0])
        assert np.all(hrr[t:] == hrr[t]) and np.all(hrz[t:] == hrz[t])
        x0, hrr0, _, info0, _ = dev.pcg(b, t, precond=P)
        assert info0 == {"steps": t, "status": sp.PCG_RAN_ALL}
        assert x0.tobytes() == x.tobytes() and hrr0.tobytes() == hrr[:t + 1].tobytes()
        xb, hb, infob, _ = dev.bicgstab(b, iters, tol=tol, precond=P)
        xb0, hb0, infob0, _ = dev.bicgstab(b, infob["steps"], precond=P)
        tb = infob["steps"]
        assert infob["status"] == sp.BICG_CONVERGED and hb0[:tb].tobytes() == hb[:tb].tobytes() and np.all(hb[tb:] == hb[tb])
        if not infob["half_step"]:                       # (a half step's last entry is s.s, and x stops half way)
            assert xb0.tobytes() == xb.tobytes() and hb0[tb] == hb[tb]
        # tol = 0 launches every step: after the stop the applies go on and x stays
        xl, hl, _, infol, _ = dev.pcg(b, t + 40, tol=tol, precond=P)
        xz, hz, _, infoz, _ = dev.pcg(b, t + 40, precond=P)
        assert xl.tobytes() == x.tobytes() and hl[:t + 1].tobytes() == hz[:t + 1].tobytes() and infol["steps"] == t
        with sp.CsrDevice(M, M, rp, col, val, 0, 1200) as half, half.preconditioner("fsai") as Ph:
            assert Ph.rows == 1200
            for method in (dev.pcg, dev.bicgstab):
                with pytest.raises(ValueError):
                    method(b, 2, precond=Ph)
            out = np.zeros(M)
            assert sp.lib().spmv_hip_csr_pcg(dev.h, Ph.h, 0, 2, 0.0, None, b.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p), None, None, None, None) == -1
        with sp.CsrDevice(M, M, rp, col, val.astype(np.float32)) as d32, d32.preconditioner("fsai") as P32:
            with pytest.raises(ValueError):
                dev.pcg(b, 2, precond=P32)
            x32, h32, _, info32, _ = d32.pcg(b.astype(np.float32), 6, precond=P32)
            assert x32.dtype == np.float32 and info32["steps"] == 6 and np.all(np.isfinite(x32))
            xb32, hb32, infob32, _ = d32.bicgstab(b.astype(np.float32), 6, precond=P32)
            assert xb32.dtype == np.float32 and np.all(np.isfinite(xb32)) and np.all(np.isfinite(hb32))


# ---------------------------------------------------------------- lifetimes, row ranges, refusals
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lifetime_and_row_ranges(gpu, dtype):
    M, rp, col, val = CASES["banded"]
    val = val.astype(dtype)
    r = np.random.default_rng(9).uniform(-1, 1, M).astype(dtype)
    dev = sp.CsrDevice(M, M, rp, col, val)
    P = dev.preconditioner("fsai", cap=8)
    z, f = P.apply(r), P.factors()
    dev.close()                                          # P outlives its handle
    assert P.apply(r).tobytes() == z.tobytes()
    assert all(u.tobytes() == v.tobytes() for a, b in zip(P.factors(), f) for u, v in zip(a, b))
    P.close()
    # a row-range handle builds the FSAI of its own diagonal block: the bytes of that block uploaded on its own
    r0, r1 = 1200, 3700
    Mb, rpb, colb, valb = csr(canonical(rp, col, val, r0, r1 - r0))
    with sp.CsrDevice(M, M, rp, col, val, r0, r1) as part, part.preconditioner("fsai", cap=8) as Pp, \
            sp.CsrDevice(Mb, Mb, rpb, colb, valb.astype(dtype)) as own, own.preconditioner("fsai", cap=8) as Po:
        assert Pp.info()["row0"] == r0 and Pp.rows == r1 - r0 and Pp.fsai_info()["widest"] == 8
        assert all(u.tobytes() == v.tobytes() for a, b in zip(Pp.factors(), Po.factors()) for u, v in zip(a, b))
        assert Pp.apply(r[r0:r1]).tobytes() == Po.apply(r[r0:r1]).tobytes()
        check_factors(M, rp, col, val, 8, dtype, "rows [1200, 3700)", r0, r1 - r0, Pp)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_refused_builds_name_the_row_and_leave_the_handle_working(gpu, oracle, dtype):
    import scipy.sparse as sps
    L = sp.lib()
    rng = np.random.default_rng(8)
    n = 70
    base = sps.lil_matrix(sps.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, -1.0)], [-1, 0, 1]))
    indefinite = base.copy()
    indefinite[41, 41], indefinite[41, 40], indefinite[40, 41] = 1.0, 2.0, 2.0      # [[4, 2], [2, 1]] at rows 40, 41
    missing = base.copy()
    missing[23, 23] = 0.0                                                          # lil drops the entry
    cases = [(csr(sps.csr_matrix(np.array([[1.0, 2.0], [2.0, 1.0]]))), 32, "row 1"), (csr(indefinite), 32, "row 41"),
             (csr(missing), 32, "row 23"), (csr(base), 0, "cap = 0"), (csr(base), 33, "cap = 33")]
    for (M, rp, col, val), cap, where in cases:
        val = val.astype(dtype)
        with sp.CsrDevice(M, M, rp, col, val) as dev:
            out = C.c_void_p()
            assert L.spmv_hip_csr_precond_build_fsai(dev.h, cap, C.byref(out)) == -1
            assert not out and where.encode() in L.spmv_hip_last_error(), L.spmv_hip_last_error()
            x = rng.uniform(-1, 1, M).astype(dtype)
            y_ref = oracle.csr_serial(rp, col, val.astype(np.float64), x.astype(np.float64))
            assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-5 * np.max(np.abs(y_ref))     # the handle still multiplies
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        with pytest.raises(ValueError):
            dev.preconditioner("fsai", cap=33)
    rp = np.arange(0, 4 * 10 + 1, 4, dtype=np.int32)
    with sp.CsrDevice(10, 12, rp, rng.integers(0, 12, 40).astype(np.int32), rng.uniform(1, 2, 40).astype(dtype)) as rect:
        with pytest.raises(sp.SpmvHipError, match="square"):
            rect.preconditioner("fsai")
