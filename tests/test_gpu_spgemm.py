"""CsrDevice.matmul on the GPU against the definition (tests/_spgemm_ref.py), bit for bit: the golden cases times their
transposes, random rectangular matrices through both tiers at several caps, the block and chunk edges, cancellation,
non-finite values, the AMG host plan's Galerkin product, the result as an ordinary handle, the refusals and the stats."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _spgemm_ref import row_products, spgemm_ref, transpose_ref
from _util import assert_parity
from conftest import GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu


def assert_same_arrays(got, want, what):
    for name, g, w in zip(("row_ptr", "col", "val"), got, want):
        assert g.dtype == w.dtype, f"{what} {name}: {g.dtype} vs {w.dtype}"
        assert g.shape == w.shape, f"{what} {name}: {g.shape} vs {w.shape}"
        if g.tobytes() != w.tobytes():
            bits = {4: np.uint32, 8: np.uint64}[g.itemsize]
            bad = np.flatnonzero(np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits))
            raise AssertionError(f"{what} {name}: {bad.size} of {g.size} differ, first at {bad[0]}: "
                                 f"{g[bad[0]]!r} vs {w[bad[0]]!r}")


def csr(M, N, rows):
    """(row_ptr, col, val) from a list of rows of (column, value) pairs, in the order given"""
    rp = np.zeros(M + 1, dtype=np.int32)
    col, val = [], []
    for i, row in enumerate(rows):
        col += [c for c, _ in row]
        val += [v for _, v in row]
        rp[i + 1] = len(col)
    assert len(rows) == M and all(0 <= c < N for c in col)
    return rp, np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


def upload(M, N, m, dtype=np.float64):
    return sp.CsrDevice(M, N, m[0], m[1], m[2].astype(dtype))


def check_product(da, db, ref, what, **caps):
    """da.matmul(db) against ref; returns the downloaded arrays and the stats"""
    with da.matmul(db, **caps) as dc:
        assert (dc.M, dc.N, dc.dtype) == (da.M, db.N, da.dtype), what
        info = dc.info()
        assert (info["M_total"], info["M_local"], info["N"], info["nz"]) == (da.M, da.M, db.N, len(ref[1])), what
        got = dc.download()
        assert_same_arrays(got, ref, what)
        assert dc.matmul_info["nz"] == len(ref[1]) and set(dc.matmul_info["ms"]) == set(sp.MATMUL_MS)
        return got, dc.matmul_info


def expected_stats(a, b, ref, block_products, chunk_products):
    """the stats by the host plan and the definition"""
    products = row_products(a, b)
    cap = {0: 4096, -1: 0}.get(block_products, block_products)
    block_row, long_rows = sp.spgemm_plan(products, block_products)
    blocks = block_rows = 0
    for r0, r1 in zip(block_row[:-1], block_row[1:]):
        own = [r for r in range(r0, r1) if products[r] <= cap]
        if products[own].sum() > 0:
            blocks, block_rows = blocks + 1, block_rows + len(own)
    chunk_cap, chunks, held = chunk_products or 1 << 23, 0, 0
    for r in long_rows:
        if chunks == 0 or held + products[r] > chunk_cap:
            chunks, held = chunks + 1, 0
        held += products[r]
    return dict(products=int(products.sum()), nz=len(ref[1]), blocks=blocks, block_rows=block_rows,
                long_rows=len(long_rows), chunks=chunks, max_row_products=int(products.max(initial=0)),
                max_row_nz=int(np.diff(ref[0]).max(initial=0)))


def assert_stats(info, a, b, ref, block_products=0, chunk_products=0):
    want = expected_stats(a, b, ref, block_products, chunk_products)
    assert {k: info[k] for k in want} == want


# ---- golden cases: A A^T
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_times_its_transpose_is_the_definition(gpu, name, dtype):
    g = load_golden(name)
    M, N = int(g["M"]), int(g["N"])
    a = (g["row_ptr"], g["col_idx"], g["values"].astype(dtype))
    at = transpose_ref(M, N, *a)
    ref = spgemm_ref(M, M, a, at, dtype)
    with sp.CsrDevice(M, N, *a) as da, da.transpose() as dt:
        assert_same_arrays(dt.download(), at, name + " A^T")
        _, info = check_product(da, dt, ref, name)
        assert_stats(info, a, at, ref)


# ---- random rectangular matrices, both tiers, every cap against the definition and against each other
def random_unsorted(rng, M, N, mean, dtype):
    """unsorted rows, repeated (row, column) pairs, empty rows and columns; values with full mantissas: a * b + c fused
    into one operation rounds differently from the product and the sum rounded one after the other, so a contracted
    multiply-add in the kernels changes the bits of these sums"""
    lens = rng.poisson(mean, M)
    lens[rng.random(M) < 0.15] = 0
    live = np.flatnonzero(rng.random(N) < 0.8)                   # the other columns stay empty
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = live[rng.integers(0, len(live), rp[-1])].astype(np.int32)
    dup = np.flatnonzero(rng.random(rp[-1]) < 0.2)
    dup = dup[dup > 0]
    col[dup] = col[dup - 1]                                      # repeats (where both fall into one row)
    val = (rng.uniform(1, 2, rp[-1]) * rng.choice([-1.0, 1.0], rp[-1])).astype(dtype)
    return rp, col, val


@pytest.fixture(scope="module")
def rect():
    out = {}
    for dtype in (np.float64, np.float32):
        rng = np.random.default_rng(77)
        a = random_unsorted(rng, 130, 77, 5, dtype)
        b = random_unsorted(rng, 77, 201, 6, dtype)
        out[np.dtype(dtype)] = (a, b, spgemm_ref(130, 201, a, b, dtype))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_rectangular_through_both_tiers(gpu, rect, dtype):
    a, b, ref = rect[np.dtype(dtype)]
    assert np.any(np.diff(a[0]) == 0) and np.any(np.diff(b[0]) == 0)
    assert np.any(np.diff(ref[0]) < row_products(a, b)), "no sum of several products in the case"
    seen = set()
    with sp.CsrDevice(130, 77, *a) as da, sp.CsrDevice(77, 201, *b) as db:
        for bp in (0, 64, 256, -1):
            for cp in (0, 64, 300):
                got, info = check_product(da, db, ref, f"rect bp={bp} cp={cp}", block_products=bp, chunk_products=cp)
                assert_stats(info, a, b, ref, bp, cp)
                seen.add(b"".join(x.tobytes() for x in got))
    assert len(seen) == 1, "the tiers disagree with each other"


# ---- block edges at block_products = 64
def laplacian_2d(n):
    rows = []
    for i in range(n):
        for j in range(n):
            row = [(i * n + j, 4.0)]
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= i + di < n and 0 <= j + dj < n:
                    row.append(((i + di) * n + j + dj, -1.0))
            rows.append(sorted(row))
    return csr(n * n, n * n, rows)


def test_block_edges_laplacian_squared(gpu):
    a = laplacian_2d(12)
    ref = spgemm_ref(144, 144, a, a, np.float64)
    assert row_products(a, a).max() == 25
    with upload(144, 144, a) as da:
        _, info = check_product(da, da, ref, "laplacian^2", block_products=64)
        assert_stats(info, a, a, ref, 64)
        assert info["blocks"] > 40 and info["long_rows"] == 0


def edge_matrix(rng):
    """A (rows as product counts through a B whose row j holds j + 1 entries): one row of exactly 64 products, the next 65
    (long), a block that sums to exactly 64, one to 63, 5000 empty rows between nonempty ones, a last block of one row"""
    K, N = 70, 90
    b_rows = [[(int(c), float(v)) for c, v in zip(rng.choice(N, j + 1, replace=False), rng.uniform(1, 2, j + 1))]
              for j in range(K)]
    b = csr(K, N, b_rows)

    def row(*lens):                                              # an A row whose B rows have these lengths
        return [(ln - 1, float(rng.uniform(1, 2))) for ln in lens]

    rows = [row(64), row(65), row(30, 20), row(14), row(40, 10), row(13), row(3)]
    rows += [[] for _ in range(5000)]
    rows += [row(5, 5, 7), row(60), row(33)]
    a = csr(len(rows), K, rows)
    return a, b, len(rows), K, N


def test_block_edges_exact_caps_long_row_and_row_cap(gpu):
    rng = np.random.default_rng(5)
    a, b, M, K, N = edge_matrix(rng)
    products = row_products(a, b)
    assert products[:7].tolist() == [64, 65, 50, 14, 50, 13, 3] and products[-3:].tolist() == [17, 60, 33]
    block_row, long_rows = sp.spgemm_plan(products, 64)
    assert long_rows.tolist() == [1]
    # [64, 65 long] [50 + 14 = 64] [50 + 13 = 63] [3 + the row cap's worth of empty rows] [... 17] [60] [33]
    assert block_row.tolist() == [0, 2, 4, 6, 6 + 4096, M - 2, M - 1, M]
    ref = spgemm_ref(M, N, a, b, np.float64)
    with upload(M, K, a) as da, upload(K, N, b) as db:
        _, info = check_product(da, db, ref, "edges", block_products=64)
        assert_stats(info, a, b, ref, 64)
        assert (info["blocks"], info["long_rows"], info["chunks"]) == (7, 1, 1)
        _, info = check_product(da, db, ref, "edges auto")
        assert_stats(info, a, b, ref)


# ---- chunk edges at chunk_products = 64
def test_chunk_edges(gpu):
    rng = np.random.default_rng(6)
    K, N = 12, 500
    b_rows = [[(int(c), float(v)) for c, v in zip(rng.integers(0, N, 25), rng.uniform(1, 2, 25))] for _ in range(K)]
    b = csr(K, N, b_rows)
    a = csr(3, K, [[(j, float(rng.uniform(1, 2))) for j in range(K)], [], [(3, 1.5)]])   # 300 products, 0, 25
    ref = spgemm_ref(3, N, a, b, np.float64)
    with upload(3, K, a) as da, upload(K, N, b) as db:
        _, info = check_product(da, db, ref, "a long row larger than the chunk", block_products=64, chunk_products=64)
        assert (info["max_row_products"], info["long_rows"], info["chunks"], info["blocks"]) == (300, 1, 1, 1)
        assert_stats(info, a, b, ref, 64, 64)
    b = csr(3, 60, [[(int(c), float(rng.uniform(1, 2))) for c in rng.integers(0, 60, n)] for n in (40, 30, 20)])
    a = csr(4, 3, [[(0, 2.5)], [(1, -1.25)], [], [(2, 3.0)]])
    ref = spgemm_ref(4, 60, a, b, np.float64)
    with upload(4, 3, a) as da, upload(3, 60, b) as db:
        _, info = check_product(da, db, ref, "three long rows in two chunks", block_products=-1, chunk_products=64)
        assert (info["long_rows"], info["chunks"], info["blocks"]) == (3, 2, 0)   # 40 | 30 + 20
        assert_stats(info, a, b, ref, -1, 64)


@pytest.mark.parametrize("block_products", [0, -1])
def test_cancellation_stays_in_the_pattern(gpu, block_products):
    a = csr(1, 2, [[(0, 1.0), (1, -1.0)]])
    b = csr(2, 2, [[(0, 2.0), (1, 3.0)], [(0, 2.0), (1, 3.0)]])
    with upload(1, 2, a) as da, upload(2, 2, b) as db, da.matmul(db, block_products=block_products) as dc:
        rp, col, val = dc.download()
        assert rp.tolist() == [0, 2] and col.tolist() == [0, 1]
        assert val.tobytes() == np.zeros(2).tobytes()


# ---- the identity the product exists for: the AMG host plan's own products
@pytest.mark.parametrize("block_products", [0, -1])
def test_galerkin_product_is_the_amg_host_plan_bit_for_bit(gpu, block_products):
    """If this fails on values only, a fused operation or a changed order of additions is the cause, not a tolerance."""
    a = laplacian_2d(24)
    n = 24 * 24
    levels = sp.amg_plan(*a)
    assert len(levels) >= 2
    A, P, R, T = (levels[0][k] for k in ("A", "P", "R", "T"))
    nc = levels[0]["aggregates"]
    with upload(n, n, A) as dA, upload(n, nc, P) as dP, upload(nc, n, R) as dR, upload(n, nc, T) as dT:
        with dA.matmul(dP, block_products=block_products) as dAP, dR.matmul(dAP, block_products=block_products) as dC:
            assert_same_arrays(dC.download(), levels[1]["A"], "R (A P) against level 1's A")
        with dA.matmul(dT, block_products=block_products) as dAT:
            rp, col, _ = dAT.download()
            assert rp.tobytes() == P[0].tobytes() and col.tobytes() == P[1].tobytes()


# ---- the result is an ordinary handle
def test_the_result_is_an_ordinary_handle(gpu, oracle, rect):
    a, b, ref = rect[np.dtype(np.float64)]
    rng = np.random.default_rng(3)
    xa, x = rng.uniform(-1, 1, 77), rng.uniform(-1, 1, 201)
    da, db = sp.CsrDevice(130, 77, *a), sp.CsrDevice(77, 201, *b)
    ya, a0, b0 = da.spmv(xa), da.download(), db.download()
    dc = da.matmul(db)
    dc2 = da @ db
    first = dc.download()
    assert_same_arrays(dc2.download(), first, "two calls")
    dc2.close()
    assert_same_arrays(da.download(), a0, "A after the product")
    assert_same_arrays(db.download(), b0, "B after the product")
    assert da.spmv(xa).tobytes() == ya.tobytes()
    assert da.__matmul__(3.0) is NotImplemented
    da.close()
    db.close()                                                   # A and B go first: C still multiplies
    assert_parity(dc.spmv(x), oracle.csr_serial(*ref, x), *ref, x, what="C x")
    with dc.transpose() as dct:
        assert_same_arrays(dct.download(), transpose_ref(130, 201, *ref), "C^T")
        with dc.matmul(dct) as dcc:
            assert_same_arrays(dcc.download(), spgemm_ref(130, 130, ref, transpose_ref(130, 201, *ref), np.float64), "C C^T")
    sq = laplacian_2d(5)
    with upload(25, 25, sq) as ds, ds.matmul(ds) as d2, d2.matmul(d2) as d4:
        r2 = spgemm_ref(25, 25, sq, sq, np.float64)
        assert_same_arrays(d4.download(), spgemm_ref(25, 25, r2, r2, np.float64), "C.matmul(C)")
    dc.close()


# ---- refusals: each leaves the handles usable
def test_refusals_leave_the_handles_usable(gpu, rect):
    a, b, ref = rect[np.dtype(np.float64)]
    L = sp.lib()
    with sp.CsrDevice(130, 77, *a) as da, sp.CsrDevice(77, 201, *b) as db:
        def refused(x, y, words, **caps):
            with pytest.raises(sp.SpmvHipError) as err:
                x.matmul(y, **caps)
            assert all(w in str(err.value) for w in words), str(err.value)
            check_product(da, db, ref, "after a refusal")

        refused(db, da, ("77 x 201", "130 x 77"))                # inner dimensions
        with sp.CsrDevice(77, 201, b[0], b[1], b[2].astype(np.float32)) as db32:
            refused(da, db32, ("8-byte", "4-byte"))
        with sp.CsrDevice(130, 77, *a, 0, 65) as half:
            refused(half, db, ("rows [0, 65) of 130",))
        with sp.CsrDevice(77, 201, *b, 10, 77) as half:
            refused(da, half, ("rows [10, 77) of 77",))
        refused(da, db, ("block_products = 100",), block_products=100)
        refused(da, db, ("chunk_products = 5",), chunk_products=5)
        assert L.spmv_hip_csr_spgemm(da.h, db.h, 0, 0, None, None, None) == -1
        assert b"out is NULL" in L.spmv_hip_last_error()
        out = C.c_void_p()
        assert L.spmv_hip_csr_spgemm(None, db.h, 0, 0, C.byref(out), None, None) == -1 and out.value is None
        check_product(da, db, ref, "after the raw refusals")
        with pytest.raises(TypeError):
            da.matmul(np.eye(3))


# ---- non-finite values get no special treatment
@pytest.mark.parametrize("block_products", [0, -1])
def test_non_finite_values_reach_exactly_the_sums_that_contain_them(gpu, rect, block_products):
    """A NaN in A and an infinity in B: the entries of C whose sums contain neither keep their bytes, the others have the
    definition's class (NaN, +Inf, -Inf; which NaN a processor makes of Inf - Inf or 0 * Inf is its own business)."""
    a, b, clean = rect[np.dtype(np.float64)]
    va, vb = a[2].copy(), b[2].copy()
    e_nan = len(va) // 3
    nan_row = int(np.searchsorted(a[0], e_nan, side="right")) - 1
    # the infinity goes into a row of B that the last row of A outside the NaN's row reads
    e_inf = max(e for e in range(len(va)) if not a[0][nan_row] <= e < a[0][nan_row + 1] and b[0][a[1][e] + 1] > b[0][a[1][e]])
    va[e_nan], vb[b[0][a[1][e_inf]]] = np.nan, np.inf
    pa, pb = (a[0], a[1], va), (b[0], b[1], vb)
    with np.errstate(invalid="ignore"):
        ref = spgemm_ref(130, 201, pa, pb, np.float64)
    touched = ~np.isfinite(ref[2])
    assert 0 < touched.sum() < len(touched) and np.isnan(ref[2]).any() and np.isinf(ref[2]).any()
    assert ref[2][~touched].tobytes() == clean[2][~touched].tobytes()
    with sp.CsrDevice(130, 77, *pa) as da, sp.CsrDevice(77, 201, *pb) as db:
        with da.matmul(db, block_products=block_products) as dc:
            rp, col, val = dc.download()
    assert rp.tobytes() == ref[0].tobytes() and col.tobytes() == ref[1].tobytes()
    assert val[~touched].tobytes() == ref[2][~touched].tobytes()
    assert np.array_equal(np.isnan(val), np.isnan(ref[2]))
    assert np.array_equal(val[np.isinf(ref[2])], ref[2][np.isinf(ref[2])])
