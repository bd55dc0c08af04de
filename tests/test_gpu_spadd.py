"""CsrDevice.add on the GPU against the definition (tests/_spadd_ref.py), bit for bit, in fp64 and fp32: the golden cases,
random rectangular matrices through every method, the kernel edges at every lane width and around the long-row limit,
exact algebra with the product, the result as an ordinary handle, non-finite values, the refusals and the stats.
Three refusals of the C entry point are not provoked here: more than 2^31 - 1 - kPad entries in C and a failed allocation
(neither fits a test of a few seconds), and a tiles-only handle, which exists only inside an HLL handle and which no
entry point hands out (the product's tests cannot reach one either)."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _spadd_ref import canon, identity_csr, random_sorted, random_unsorted, spadd_ref
from _spgemm_ref import spgemm_ref, transpose_ref
from _util import assert_parity, assert_parity_f32
from conftest import GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
NO_LONG = 1 << 30                                                # a long_row no row reaches: the long tier switched off


def assert_same_arrays(got, want, what):
    for name, g, w in zip(("row_ptr", "col", "val"), got, want):
        assert g.dtype == w.dtype, f"{what} {name}: {g.dtype} vs {w.dtype}"
        assert g.shape == w.shape, f"{what} {name}: {g.shape} vs {w.shape}"
        if g.tobytes() != w.tobytes():
            bits = {4: np.uint32, 8: np.uint64}[g.itemsize]
            bad = np.flatnonzero(np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits))
            raise AssertionError(f"{what} {name}: {bad.size} of {g.size} differ, first at {bad[0]}: "
                                 f"{g[bad[0]]!r} vs {w[bad[0]]!r}")


def csr(M, N, rows, dtype=np.float64):
    """(row_ptr, col, val) from a list of rows of (column, value) pairs, in the order given"""
    rp = np.zeros(M + 1, dtype=np.int32)
    col, val = [], []
    for i, row in enumerate(rows):
        col += [c for c, _ in row]
        val += [v for _, v in row]
        rp[i + 1] = len(col)
    assert len(rows) == M and all(0 <= c < N for c in col)
    return rp, np.array(col, dtype=np.int32), np.array(val, dtype=np.float64).astype(dtype)


def upload(M, N, m):
    return sp.CsrDevice(M, N, m[0], m[1], m[2])


def is_canonical(m):
    rp, col, _ = m
    return all(np.all(np.diff(col[rp[i]:rp[i + 1]]) > 0) for i in range(len(rp) - 1))


def check_add(da, db, ref, what, alpha=1.0, beta=1.0, **kw):
    """da.add(db) against ref = spadd_ref(...); returns the downloaded arrays and add_info"""
    want, matches, combined = ref
    with da.add(db, alpha, beta, **kw) as dc:
        assert (dc.M, dc.N, dc.dtype) == (da.M, da.N, da.dtype), what
        info = dc.info()
        assert (info["M_total"], info["M_local"], info["N"], info["nz"], info["row0"]) == (da.M, da.M, da.N, len(want[1]), 0), what
        got = dc.download()
        assert_same_arrays(got, want, what)
        st = dc.add_info
        assert set(st) == set(sp.ADD_STATS) | {"ms"} and tuple(st["ms"]) == sp.ADD_MS, what
        assert (st["nz"], st["matches"]) == (len(want[1]), matches), (what, st)
        assert st["max_row_nz"] == int(np.diff(want[0]).max(initial=0)), (what, st)
        if kw.get("long_row"):
            assert st["long_rows"] == int((combined >= kw["long_row"]).sum()), (what, st)
        return got, st


# ---- golden cases
def mantissa_values(rng, n, dtype):
    return (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_sums_are_the_definition(gpu, name, dtype):
    """A + A^T (square cases; a rectangular case is refused with both shapes), A - A, and 1.5 A - 0.25 B on A's pattern
    and its mirror image (columns reversed, so B's rows descend) with values of full mantissa: a multiply-add contracted
    into one operation changes the bits of these sums"""
    g = load_golden(name)
    M, N = int(g["M"]), int(g["N"])
    a = (g["row_ptr"], g["col_idx"], g["values"].astype(dtype))
    with upload(M, N, a) as da:
        with da.transpose() as dt:
            if M == N:
                check_add(da, dt, spadd_ref(M, N, a, transpose_ref(M, N, *a), dtype), name + " A + A^T")
            else:
                with pytest.raises(ValueError, match=f"{M} x {N}.*{N} x {M}"):
                    da + dt
        ref = spadd_ref(M, N, a, a, dtype, 1.0, -1.0)
        ca = canon(M, N, a, dtype)
        assert ref[0][0].tobytes() == ca[0].tobytes() and ref[0][1].tobytes() == ca[1].tobytes()
        assert ref[0][2].tobytes() == np.zeros(len(ca[1]), dtype).tobytes() or not np.all(np.isfinite(ca[2]))
        with da - da as dz:
            assert_same_arrays(dz.download(), ref[0], name + " A - A")
    rng = np.random.default_rng(len(name))
    am = (a[0], a[1], mantissa_values(rng, len(a[1]), dtype))
    bm = (a[0], (N - 1 - a[1]).astype(np.int32), mantissa_values(rng, len(a[1]), dtype))
    with upload(M, N, am) as da, upload(M, N, bm) as db:
        check_add(da, db, spadd_ref(M, N, am, bm, dtype, 1.5, -0.25), name + " 1.5 A - 0.25 B", 1.5, -0.25)


# ---- random rectangular matrices: unsorted rows, repeated pairs, empty rows and columns
@pytest.fixture(scope="module")
def rect():
    out = {}
    for dtype in DTYPES:
        rng = np.random.default_rng(77)
        a = random_unsorted(rng, 130, 77, 5, dtype)
        b = random_unsorted(rng, 130, 77, 6, dtype)
        out[np.dtype(dtype)] = (a, b, spadd_ref(130, 77, a, b, dtype, 1.5, -0.25))
    return out


@pytest.fixture(scope="module")
def tidy():
    out = {}
    for dtype in DTYPES:
        rng = np.random.default_rng(78)
        a = random_sorted(rng, 333, 90, 7, dtype)
        b = random_sorted(rng, 333, 90, 9, dtype)
        out[np.dtype(dtype)] = (a, b, spadd_ref(333, 90, a, b, dtype, 1.5, -0.25))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_unsorted_through_auto_and_canonical(gpu, rect, dtype):
    a, b, ref = rect[np.dtype(dtype)]
    assert np.any(np.diff(a[0]) == 0) and not is_canonical(a) and not is_canonical(b)
    assert 0 < ref[1] < len(ref[0][1]) and ref[2].sum() < len(a[1]) + len(b[1]), "no match or no repeated pair in the case"
    seen = set()
    with upload(130, 77, a) as da, upload(130, 77, b) as db:
        for method in ("auto", "canonical"):
            for lanes in (0, 1, 16):
                got, st = check_add(da, db, ref, f"rect {method} lanes={lanes}", 1.5, -0.25, method=method, lanes=lanes)
                assert (st["a_canonical"], st["b_canonical"]) == (0, 0)
                seen.add(b"".join(x.tobytes() for x in got))
        with pytest.raises(sp.SpmvHipError, match="A is not canonical"):
            da.add(db, method="merge")
    assert len(seen) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_sorted_operands_give_the_same_bytes_through_every_method(gpu, rect, tidy, dtype):
    a, b, ref = tidy[np.dtype(dtype)]
    assert is_canonical(a) and is_canonical(b)
    seen = set()
    with upload(333, 90, a) as da, upload(333, 90, b) as db:
        for method in ("merge", "auto", "canonical"):
            got, st = check_add(da, db, ref, f"sorted {method}", 1.5, -0.25, method=method)
            assert (st["a_canonical"], st["b_canonical"]) == (1, 1)
            seen.add(b"".join(x.tobytes() for x in got))
        first = got
        with da.add(db, 1.5, -0.25) as again:
            assert_same_arrays(again.download(), first, "two calls")
    assert len(seen) == 1
    # one operand unsorted: found as such, canonicalised alone; merge-only names it and its first offending row
    u = rect[np.dtype(dtype)][0]
    t = random_sorted(np.random.default_rng(5), 130, 77, 6, dtype)
    bad = next(i for i in range(130) if np.any(np.diff(u[1][u[0][i]:u[0][i + 1]]) <= 0))
    with upload(130, 77, t) as dt, upload(130, 77, u) as du:
        _, st = check_add(dt, du, spadd_ref(130, 77, t, u, dtype), "sorted + unsorted")
        assert (st["a_canonical"], st["b_canonical"]) == (1, 0)
        _, st = check_add(du, dt, spadd_ref(130, 77, u, t, dtype), "unsorted + sorted")
        assert (st["a_canonical"], st["b_canonical"]) == (0, 1)
        with pytest.raises(sp.SpmvHipError, match=f"B is not canonical: row {bad} "):
            dt.add(du, method="merge")
        with pytest.raises(sp.SpmvHipError, match=f"A is not canonical: row {bad} "):
            du.add(dt, method="merge")


@pytest.mark.parametrize("dtype", DTYPES)
def test_canonical_is_a_times_the_identity(gpu, rect, tidy, dtype):
    for M, N, a in ((130, 77, rect[np.dtype(dtype)][0]), (333, 90, tidy[np.dtype(dtype)][0])):
        want = spgemm_ref(M, N, a, identity_csr(N, dtype), dtype)
        with upload(M, N, a) as da, da.canonical() as dc, sp.identity(N, dtype) as eye, da.matmul(eye) as dp:
            assert_same_arrays(dc.download(), want, "canonical()")
            assert_same_arrays(dp.download(), want, "A @ I")
            assert dc.add_info["matches"] == 0 and dc.add_info["b_canonical"] == 1
        with upload(M, N, a) as da, -da as dn:
            assert_same_arrays(dn.download(), (want[0], want[1], -want[2]), "-A")


# ---- kernel edges at every lane width
def edge_pair(lanes, dtype):
    """rows around the lane width, every kind of match, the first and the last column, and random rows up to an M that
    is no multiple of the rows of a workgroup (256 / lanes) and fills more than two workgroups"""
    rng = np.random.default_rng(100 + lanes)
    N = 200
    val = lambda: float(rng.uniform(1, 2) * rng.choice([-1.0, 1.0]))       # noqa: E731
    row = lambda cols: [(int(c), val()) for c in cols]                     # noqa: E731
    pick = lambda n: np.sort(rng.choice(N, n, replace=False))              # noqa: E731
    ra, rb = [], []
    for total in (lanes - 1, lanes, lanes + 1):                            # combined lengths around the lane width
        for la in sorted({0, total // 2, total}):
            cols = pick(total) if total else np.zeros(0, dtype=np.int64)
            mine = rng.permutation(total)[:la]
            ra.append(row(np.sort(cols[mine])))
            rb.append(row(np.delete(cols, mine)))
    for n in (1, lanes, lanes + 1, 2 * lanes + 3):
        cols = pick(n)
        ra.append(row(cols)), rb.append(row(cols))                         # every column matched
        others = pick(min(n + 2, N))
        ra.append(row(cols)), rb.append(row(np.setdiff1d(others, cols)))   # none matched
        more = pick(n + 3)
        lo, hi = np.concatenate([[0], more[more > 0]]), np.concatenate([more[more < N - 1], [N - 1]])
        ra.append(row(lo)), rb.append(row(np.concatenate([[0], np.setdiff1d(pick(n), lo)])))            # the first only
        ra.append(row(hi)), rb.append(row(np.concatenate([np.setdiff1d(pick(n), hi), [N - 1]])))        # the last only
    ra.append(row([0])), rb.append(row([N - 1]))
    ra.append(row([N - 1])), rb.append(row([0]))
    ra.append(row([0, N - 1])), rb.append(row([0, N - 1]))
    while len(ra) < 2 * (256 // lanes) + 3 or len(ra) % (256 // lanes) == 0:
        ra.append(row(pick(int(rng.integers(0, 12))))), rb.append(row(pick(int(rng.integers(0, 12)))))
    M = len(ra)
    return M, N, csr(M, N, ra, dtype), csr(M, N, rb, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_rows_at_the_lane_width_and_every_kind_of_match(gpu, lanes, dtype):
    M, N, a, b = edge_pair(lanes, dtype)
    assert M % (256 // lanes) != 0 and M > 256 // lanes and is_canonical(a) and is_canonical(b)
    ref = spadd_ref(M, N, a, b, dtype, 1.5, -0.25)
    assert {lanes - 1, lanes, lanes + 1} <= set(ref[2].tolist())
    with upload(M, N, a) as da, upload(M, N, b) as db:
        got, st = check_add(da, db, ref, f"edges lanes={lanes}", 1.5, -0.25, method="merge", lanes=lanes, long_row=NO_LONG)
        assert st["long_rows"] == 0
        again, _ = check_add(da, db, ref, f"edges lanes={lanes}, long rows from {lanes}", 1.5, -0.25, lanes=lanes,
                             long_row=max(lanes, 2))
        assert_same_arrays(again, got, "both tiers")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_and_empty_shapes_at_every_lane_width(gpu, dtype):
    one = csr(1, 1, [[(0, 1.25)]], dtype)
    cases = [("N = 1", 3, 1, csr(3, 1, [[(0, 1.5)], [], [(0, -2.5)]], dtype), csr(3, 1, [[(0, 0.75)], [(0, 3.5)], []], dtype)),
             ("M = 0", 0, 5, csr(0, 5, [], dtype), csr(0, 5, [], dtype)),
             ("M = 1", 1, 1, one, one),
             ("A empty", 4, 6, csr(4, 6, [[]] * 4, dtype), csr(4, 6, [[(1, 2.0)], [], [(0, 1.0), (5, -1.0)], []], dtype)),
             ("B empty", 4, 6, csr(4, 6, [[(1, 2.0)], [], [(0, 1.0), (5, -1.0)], []], dtype), csr(4, 6, [[]] * 4, dtype)),
             ("both empty", 4, 6, csr(4, 6, [[]] * 4, dtype), csr(4, 6, [[]] * 4, dtype))]
    for what, M, N, a, b in cases:
        ref, ref1 = spadd_ref(M, N, a, b, dtype, 1.5, -0.25), spadd_ref(M, N, a, None, dtype, 1.5)
        with upload(M, N, a) as da, upload(M, N, b) as db:
            for lanes in (0, 1, 2, 4, 8, 16, 32, 64):
                check_add(da, db, ref, f"{what} lanes={lanes}", 1.5, -0.25, lanes=lanes)
            check_add(da, db, ref, f"{what} long_row=1", 1.5, -0.25, long_row=1)
            check_add(da, db, ref, f"{what} canonical", 1.5, -0.25, method="canonical")
            check_add(da, None, ref1, f"{what} alone", 1.5)


@pytest.fixture(scope="module")
def long_case():
    """rows of 63, 64 and 65 combined entries, one of a few thousand, among short ones: N = 5000"""
    out = {}
    for dtype in DTYPES:
        rng = np.random.default_rng(9)
        N = 5000
        val = lambda n: (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).tolist()   # noqa: E731
        ra, rb = [], []
        for la, lb in ((30, 33), (64, 0), (1, 64), (2100, 1900), (0, 63), (40, 40), (300, 1)):
            k = min(la, lb) // 2                                                     # the columns both rows hold
            union = rng.choice(N, la + lb - k, replace=False)
            ca, cb = np.sort(union[:la]), np.sort(union[la - k:])
            ra.append(list(zip(ca.tolist(), val(len(ca))))), rb.append(list(zip(cb.tolist(), val(len(cb)))))
            ra.append([(7, 1.5)]), rb.append([(7, -2.5), (9, 1.25)])
        a, b = csr(len(ra), N, ra, dtype), csr(len(rb), N, rb, dtype)
        out[np.dtype(dtype)] = (len(ra), N, a, b, spadd_ref(len(ra), N, a, b, dtype, 1.5, -0.25))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_rows_give_the_bytes_of_the_lane_tier(gpu, long_case, dtype):
    M, N, a, b, ref = long_case[np.dtype(dtype)]
    assert {63, 64, 65} <= set(ref[2].tolist()) and ref[2].max() > 3000 and 0 < ref[1]
    with upload(M, N, a) as da, upload(M, N, b) as db:
        off, st = check_add(da, db, ref, "long tier off", 1.5, -0.25, long_row=NO_LONG)
        assert st["long_rows"] == 0
        for lanes in (0, 1, 64):
            on, st = check_add(da, db, ref, f"long rows from 64, lanes={lanes}", 1.5, -0.25, long_row=64, lanes=lanes)
            assert st["long_rows"] == int((ref[2] >= 64).sum()) >= 5
            assert_same_arrays(on, off, "the long tier against the lane tier")
        auto, st = check_add(da, db, ref, "auto", 1.5, -0.25)
        assert st["long_rows"] == 1                                  # (auto: 256 at the least; the row of 4000)
        assert_same_arrays(auto, off, "auto against the lane tier")


# ---- exact algebra: small positive integers, every sum exact in the dtype (and never a zero whose sign could differ)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_algebra_with_the_product(gpu, dtype):
    rng = np.random.default_rng(31)
    ints = lambda m: (m[0], m[1], rng.integers(1, 9, len(m[1])).astype(dtype))   # noqa: E731
    a, b = ints(random_unsorted(rng, 90, 60, 5, dtype)), ints(random_unsorted(rng, 90, 60, 4, dtype))
    cm = ints(random_unsorted(rng, 60, 45, 3, dtype))
    with upload(90, 60, a) as da, upload(90, 60, b) as db, upload(60, 45, cm) as dc:
        with da + db as dab, dab @ dc as left, da @ dc as dac, db @ dc as dbc, dac + dbc as right:
            assert_same_arrays(left.download(), right.download(), "(A + B) C against A C + B C")
            assert left.info()["nz"] > 0
        with da + da as twice, da.add(None, alpha=2.0) as doubled:
            assert_same_arrays(twice.download(), doubled.download(), "A + A against 2 A")
            assert twice.add_info["matches"] == doubled.add_info["nz"]
        with da + db as dab, dab - db as back:
            rp, col, val = back.download()
            ca, cb = canon(90, 60, a, dtype), canon(90, 60, b, dtype)
            want = spadd_ref(90, 60, ca, (cb[0], cb[1], np.zeros(len(cb[1]), dtype)), dtype)[0]
            assert_same_arrays((rp, col, val), want, "(A + B) - B against canon(A) on the union")
            assert np.count_nonzero(val) == len(ca[1]) < len(val)


# ---- the result is an ordinary handle
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_result_is_an_ordinary_handle(gpu, oracle, rect, dtype):
    a, b, _ = rect[np.dtype(dtype)]
    ref = spadd_ref(130, 77, a, b, dtype)[0]
    rng = np.random.default_rng(3)
    x, X = rng.uniform(-1, 1, 77).astype(dtype), rng.uniform(-1, 1, (77, 3)).astype(dtype)
    da, db = upload(130, 77, a), upload(130, 77, b)
    a0, b0 = da.download(), db.download()
    dc = da + db
    assert_same_arrays(da.download(), a0, "A after the sum")
    assert_same_arrays(db.download(), b0, "B after the sum")
    assert da.__add__(3.0) is NotImplemented and da.__sub__(np.eye(3)) is NotImplemented
    with pytest.raises(TypeError):
        da + 3.0
    da.close()
    db.close()                                                   # A and B go first: C still multiplies
    info = dc.info()
    assert (info["M_total"], info["M_local"], info["N"], info["nz"], info["row0"]) == (130, 130, 77, len(ref[1]), 0)
    assert info["value_bytes"] == np.dtype(dtype).itemsize
    assert_same_arrays(dc.download(), ref, "C after A and B are gone")

    def parity(y, xv, what):
        if dtype == np.float64:
            assert_parity(y, oracle.csr_serial(*ref, xv), *ref, xv, what=what)
        else:
            assert_parity_f32(y, oracle.csr_f32_accum64(*ref, xv), *ref, xv, what=what)

    parity(dc.spmv(x), x, "C x")
    Y = dc.spmm(X)
    for k in range(3):
        parity(np.ascontiguousarray(Y[:, k]), np.ascontiguousarray(X[:, k]), f"C X[:, {k}]")
    with dc.transpose() as dct:
        assert_same_arrays(dct.download(), transpose_ref(130, 77, *ref), "C^T")
    dc.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi_of_a_shifted_matrix(gpu, dtype):
    """what minres' shift could not give: the preconditioner of A + sigma I itself"""
    n, sigma = 300, 0.375
    a = random_sorted(np.random.default_rng(12), n, n, 6, dtype)
    ref = spadd_ref(n, n, a, identity_csr(n, dtype), dtype, 1.0, sigma)[0]
    diag = np.array([ref[2][ref[0][i]:ref[0][i + 1]][ref[1][ref[0][i]:ref[0][i + 1]] == i][0] for i in range(n)])
    assert diag.dtype == dtype and np.all(diag != 0)
    with upload(n, n, a) as da, sp.identity(n, dtype) as eye, da.add(eye, beta=sigma) as shifted:
        assert_same_arrays(shifted.download(), ref, "A + sigma I")
        with shifted.transpose() as st:
            assert_same_arrays(st.download(), transpose_ref(n, n, *ref), "(A + sigma I)^T")
        with shifted.preconditioner("jacobi") as P:
            z = P.apply(np.ones(n, dtype))
            assert z.tobytes() == (1.0 / diag.astype(np.float64)).astype(dtype).tobytes()


# ---- non-finite values get no special treatment
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_values_reach_exactly_the_entries_that_contain_them(gpu, rect, tidy, dtype):
    """A NaN and an infinity in single entries of A and of B (A sorted: the merge alone; B unsorted: through the product
    first).  The entries whose formula contains neither keep their bytes; the others have the definition's class (which
    NaN a processor makes of Inf - Inf or 0 * Inf is its own business)."""
    a = random_sorted(np.random.default_rng(14), 130, 77, 6, dtype)
    b = rect[np.dtype(dtype)][1]
    clean = spadd_ref(130, 77, a, b, dtype, 1.5, -0.25)[0]
    va, vb = a[2].copy(), b[2].copy()
    va[len(va) // 3], va[2 * len(va) // 3] = np.nan, np.inf
    vb[len(vb) // 4], vb[len(vb) // 2] = -np.inf, np.nan
    pa, pb = (a[0], a[1], va), (b[0], b[1], vb)
    ref = spadd_ref(130, 77, pa, pb, dtype, 1.5, -0.25)[0]
    touched = ~np.isfinite(ref[2])
    assert 2 <= touched.sum() <= 4 and np.isnan(ref[2]).any() and np.isinf(ref[2]).any()
    assert ref[2][~touched].tobytes() == clean[2][~touched].tobytes()
    with upload(130, 77, pa) as da, upload(130, 77, pb) as db:
        with da.add(db, 1.5, -0.25) as dc:
            rp, col, val = dc.download()
        assert rp.tobytes() == ref[0].tobytes() and col.tobytes() == ref[1].tobytes()
        assert val[~touched].tobytes() == ref[2][~touched].tobytes()
        assert np.array_equal(np.isnan(val), np.isnan(ref[2]))
        assert np.array_equal(val[np.isinf(ref[2])], ref[2][np.isinf(ref[2])])
        # alpha = 0 gets no shortcut: 0 * Inf and 0 * NaN are NaN at A's two entries, and B's own stay what they are
        zero = spadd_ref(130, 77, pa, pb, dtype, 0.0, 1.0)[0]
        plain = spadd_ref(130, 77, a, pb, dtype, 0.0, 1.0)[0]
        differs = np.flatnonzero(np.isnan(zero[2]) & ~np.isnan(plain[2]))
        assert len(differs) == 2
        with da.add(db, 0.0, 1.0) as dz:
            rp, col, val = dz.download()
        assert rp.tobytes() == zero[0].tobytes() and col.tobytes() == zero[1].tobytes()
        assert np.array_equal(np.isnan(val), np.isnan(zero[2]))
        keep = ~np.isnan(zero[2])
        assert val[keep].tobytes() == zero[2][keep].tobytes() == plain[2][keep].tobytes()


# ---- the C entry point's refusals: each leaves the handles usable
def test_refusals_leave_the_handles_usable(gpu, rect, tidy):
    a, b, ref = rect[np.dtype(np.float64)]
    t = tidy[np.dtype(np.float64)][0]
    L = sp.lib()
    bad_row = next(i for i in range(130) if np.any(np.diff(a[1][a[0][i]:a[0][i + 1]]) <= 0))
    with upload(130, 77, a) as da, upload(130, 77, b) as db:
        def refused(x, y, words, alpha=1.0, beta=1.0, method=0, lanes=0, long_row=0):
            out = C.c_void_p()
            rc = L.spmv_hip_csr_add(x, alpha, y, beta, method, lanes, long_row, C.byref(out), None, None)
            msg = L.spmv_hip_last_error().decode()
            assert rc == -1 and out.value is None, words
            assert all(w in msg for w in words), msg
            check_add(da, db, ref, "after a refusal", 1.5, -0.25)

        with upload(333, 90, t) as dt:
            refused(da.h, dt.h, ("130 x 77", "333 x 90"))
        with upload(77, 130, transpose_ref(130, 77, *a)) as dat:
            refused(da.h, dat.h, ("130 x 77", "77 x 130"))
        with sp.CsrDevice(130, 77, b[0], b[1], b[2].astype(np.float32)) as db32:
            refused(da.h, db32.h, ("8-byte", "4-byte"))
        with sp.CsrDevice(130, 77, *a, 0, 65) as half:
            refused(half.h, db.h, ("A", "rows [0, 65) of 130"))
        with sp.CsrDevice(130, 77, *b, 10, 130) as half:
            refused(da.h, half.h, ("B", "rows [10, 130) of 130"))
        refused(da.h, db.h, ("alpha = nan",), alpha=float("nan"))
        refused(da.h, db.h, ("beta = inf",), beta=float("inf"))
        refused(da.h, None, ("alpha = -inf",), alpha=float("-inf"))
        refused(da.h, db.h, ("method = 3",), method=3)
        refused(da.h, db.h, ("method = -1",), method=-1)
        refused(da.h, db.h, ("lanes = 3",), lanes=3)
        refused(da.h, db.h, ("lanes = 128",), lanes=128)
        refused(da.h, db.h, ("long_row = -1",), long_row=-1)
        refused(da.h, db.h, ("A is not canonical", f"row {bad_row} "), method=1)
        refused(None, db.h, ("NULL handle",))
        assert L.spmv_hip_csr_add(da.h, 1.0, db.h, 1.0, 0, 0, 0, None, None, None) == -1
        assert b"out is NULL" in L.spmv_hip_last_error()
        check_add(da, db, ref, "after the raw refusals", 1.5, -0.25)
        # the same handle twice is a sum like any other
        check_add(da, da, spadd_ref(130, 77, a, a, np.float64, 1.5, -0.25), "a == b", 1.5, -0.25)
        with pytest.raises(TypeError):
            da.add(np.eye(3))
