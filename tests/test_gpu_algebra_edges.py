"""CsrDevice.matmul, .add and .transpose beyond the first trip of every kernel loop, bit for bit against the definitions
(spgemm_ref, spadd_ref, transpose_ref) in fp64 and fp32: rows of A wider than one 256-entry tile of the expansion, runs of
equal keys longer than a batch of 256 sorted positions and runs that start at a batch edge, a full on-chip block (4096
rows, 4096 products, the 4096 / 4097 split), the global tier's sort width at chunks of 1 to 5 rows and N at powers of two,
more blocks and more long rows than the product's grids hold, more rows than one trip of sg_count, more long rows than
sa_merge_long has workgroups, and a transpose of more rows than tr_make_pairs has waves with rows wider than a wave's trip.
Each case asserts from matmul_info / add_info that the tier it aims at was taken, and the knob settings of a case must give
identical bytes.  The constructions are in tests/_algebra_cases.py; tests/test_algebra_refs_host.py holds them to their
plans without a GPU.

Measured on an MI355X: the 26 cases of this file take 1.3 s together (pytest's wall time, the device's start included).
The slowest calls are the sum (0.09 s per dtype, the reference loop over 4396 rows included), the product of 2^21 + 70
rows (0.06 s per cap; matmul_info's split: count 0.6 ms, symbolic 8.5 ms, numeric 0.3 ms, adopt 8.0 ms) and the rows
wider than a tile (0.06 s, eight knob settings); the 65742-row products take 0.02 to 0.04 s (symbolic 0.6 to 1.0 ms,
numeric 0.4 to 0.8 ms, adopt 0.8 ms) and the transpose of 4 * 2^20 + 70 rows 0.03 s.

Each path was shown to be reached by one value-only break in a copy of the kernels (no index, count or offset changed),
the file run once per break: negating the products of the expansion's tiles after the first fails cases 1, 2 and 3
(in the global tier alone: 1 and 2); negating the strided trips of sg_block fails 5 "blocks", of sg_expand 5 "one-chunk",
of sa_merge_long 6; dropping the last addition of a run longer than 256 fails 2 and 3 (on chip and, broken alone, in
sg_row_compress); giving the second trip of tr_make_pairs' grid the value of the row's first entry fails the tall
transpose, and giving a row's second trip of 64 entries the value 64 entries back fails both transposes.  sg_count and
sg_row_heads only count: the constructions and the asserted stats are their evidence."""
import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
import _algebra_cases as ac
from _algebra_cases import as_dtype, assert_same_arrays
from _spadd_ref import spadd_ref
from _spgemm_ref import row_products, spgemm_ref, transpose_ref
from _util import assert_parity, assert_parity_f32

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
NO_LONG = 1 << 30                                                # a long_row no row reaches: the long tier switched off


def upload(M, N, m):
    return sp.CsrDevice(M, N, m[0], m[1], m[2])


def check_product(da, db, ref, products, what, bp=0, cp=0):
    """da.matmul(db) against ref and the stats against the host plan; returns (the downloaded bytes, the stats)"""
    with da.matmul(db, block_products=bp, chunk_products=cp) as dc:
        assert (dc.M, dc.N, dc.dtype) == (da.M, db.N, da.dtype), what
        info = dc.info()
        assert (info["M_total"], info["M_local"], info["N"], info["nz"]) == (da.M, da.M, db.N, len(ref[1])), what
        got = dc.download()
        assert_same_arrays(got, ref, what)
        st = dc.matmul_info
    want, _ = ac.plan_stats(products, ref[0], bp, cp)
    assert {k: st[k] for k in want} == want, what
    return b"".join(x.tobytes() for x in got), st


def small_product_case(case, dtype):
    M, K, N, a, b = case
    a, b = as_dtype(a, dtype), as_dtype(b, dtype)
    return M, K, N, a, b, spgemm_ref(M, N, a, b, dtype), row_products(a, b)


# ---- 1. rows wider than one tile
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_rows_wider_than_one_tile(gpu, dtype):
    M, K, N, a, b, ref, products = small_product_case(ac.wide_rows_case(), dtype)
    assert products[0] <= 4096, "row 0 must stay on chip at block_products = 0"
    assert products[:4].sum() > 1024 and products[:4].max() <= 1024 and products[:4].min() > 64
    seen = set()
    with upload(M, K, a) as da, upload(K, N, b) as db:
        for bp in (0, 1024, 64, -1):
            for cp in (0, 64):
                got, st = check_product(da, db, ref, products, f"wide rows bp={bp} cp={cp}", bp, cp)
                seen.add(got)
                if bp == 0:
                    assert (st["blocks"], st["long_rows"], st["chunks"]) == (1, 0, 0)
                elif bp == 1024:
                    assert st["blocks"] >= 3 and st["long_rows"] == 0, "rows 0 to 3 on chip, in more than one block"
                elif bp == 64:                                   # (cp = 64: rows 0 to 3 are larger than a chunk, one each)
                    assert (st["long_rows"], st["chunks"]) == (4, 4 if cp else 1) and st["blocks"] >= 1
                else:
                    assert st["long_rows"] == int((products > 0).sum()) > 30 and st["blocks"] == 0
                    assert st["chunks"] == 1 if cp == 0 else 4 < st["chunks"] < st["long_rows"]
                assert st["max_row_products"] == products.max()
    assert len(seen) == 1, "the tiers disagree with each other"


# ---- 2. long runs and batch edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_long_runs_and_runs_at_batch_edges(gpu, dtype):
    M, K, N, a, b, ref, products = small_product_case(ac.long_runs_case(), dtype)
    assert products.tolist() == [1200, 80, 856, 168, 855] and np.diff(ref[0]).tolist() == [601, 41, 302, 85, 302]
    seen = set()
    with upload(M, K, a) as da, upload(K, N, b) as db:
        got, st = check_product(da, db, ref, products, "long runs on chip", 0)
        assert (st["blocks"], st["block_rows"], st["long_rows"], st["max_row_products"]) == (1, 5, 0, 1200)
        seen.add(got)
        got, st = check_product(da, db, ref, products, "long runs through the global tier", -1)
        assert (st["blocks"], st["long_rows"], st["chunks"], st["max_row_nz"]) == (0, 5, 1, 601)
        seen.add(got)
        got, st = check_product(da, db, ref, products, "long runs, a chunk per row", -1, 64)
        assert (st["long_rows"], st["chunks"]) == (5, 5)
        seen.add(got)
    assert len(seen) == 1, "the tiers disagree with each other"


# ---- 3. a full block
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_full_block_and_the_4096_4097_split(gpu, dtype):
    M, K, N, a, b, ref, products = small_product_case(ac.full_block_case(), dtype)
    block_row, long_rows = sp.spgemm_plan(products, 0)
    assert long_rows.tolist() == [4098] and block_row.tolist() == [0, 4096, 4097, 4099, 4099 + 4095, M]
    assert products[4096:4099].tolist() == [4096, 4096, 4097]
    assert np.diff(ref[0])[4096:4099].tolist() == [4096, 1, 4097]
    with upload(M, K, a) as da, upload(K, N, b) as db:
        on_chip, st = check_product(da, db, ref, products, "full block on chip", 0)
        assert (st["blocks"], st["block_rows"], st["long_rows"], st["chunks"]) == (5, M - 1, 1, 1)
        assert (st["max_row_products"], st["max_row_nz"]) == (4097, 4097)
        glob, st = check_product(da, db, ref, products, "full block through the global tier", -1)
        assert (st["blocks"], st["long_rows"], st["chunks"]) == (0, M, 1)
    assert on_chip == glob, "the tiers disagree with each other"


# ---- 4. the sort width of the global tier
@pytest.mark.parametrize("N, dtype", [(N, d) for N in ac.SORT_WIDTH_NS for d in DTYPES if N < 1 << 20 or d == np.float64],
                         ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
def test_product_sort_width_at_chunks_of_one_to_five_rows(gpu, N, dtype):
    M, K, N, a, b, ref, products = small_product_case(ac.sort_width_case(N), dtype)
    want, chunk_rows = ac.plan_stats(products, ref[0], -1, ac.SORT_WIDTH_CHUNK)
    assert chunk_rows == [1, 2, 3, 4, 5]
    with upload(M, K, a) as da, upload(K, N, b) as db:
        chunked, st = check_product(da, db, ref, products, f"N={N}, chunks of 1 to 5 rows", -1, ac.SORT_WIDTH_CHUNK)
        assert (st["chunks"], st["long_rows"], st["blocks"]) == (5, 15, 0)
        whole, st = check_product(da, db, ref, products, f"N={N}, one chunk of 15 rows", -1, 0)
        assert (st["chunks"], st["long_rows"]) == (1, 15)
        on_chip, st = check_product(da, db, ref, products, f"N={N}, on chip", 0)
        assert (st["chunks"], st["long_rows"], st["blocks"]) == (0, 0, 1)
    assert chunked == whole == on_chip


# ---- 5. grid strides (fp64; the references are tiled and expanded, never a loop over all rows)
@pytest.fixture(scope="module")
def block_stride():
    M, K, N, a, b, ref = ac.block_stride_case()
    ref = ref(np.float64)
    return M, K, N, a, b, ref, row_products(a, b)


@pytest.fixture(scope="module")
def seen():
    """the downloaded bytes of a case's earlier knob settings, by case: every later setting must give the same"""
    return {}


def same_as_before(seen, case, got, what):
    assert seen.setdefault(case, got) == got, f"{what}: other bytes than an earlier knob setting of the case"


@pytest.mark.parametrize("bp, cp", [(64, 0), (-1, 0), (-1, 1 << 20)], ids=["blocks", "one-chunk", "chunks"])
def test_product_more_blocks_and_long_rows_than_the_grid(gpu, block_stride, seen, bp, cp):
    M, K, N, a, b, ref, products = block_stride
    assert M > 65536 and products.min() >= 33 and products.max() <= 64   # kSgMaxGrid; a block per row at bp = 64
    with upload(M, K, a) as da, upload(K, N, b) as db:
        got, st = check_product(da, db, ref, products, f"grid stride bp={bp} cp={cp}", bp, cp)
        same_as_before(seen, "block stride", got, f"bp={bp} cp={cp}")
        print(f"bp={bp} cp={cp}: ms = {st['ms']}")
    if bp == 64:
        assert (st["blocks"], st["block_rows"], st["long_rows"]) == (M, M, 0)
    elif cp == 0:
        assert (st["blocks"], st["long_rows"], st["chunks"]) == (0, M, 1)
    else:
        assert (st["blocks"], st["long_rows"]) == (0, M) and st["chunks"] >= 3
        assert M // st["chunks"] > 10000


@pytest.mark.parametrize("bp", [0, 64])
def test_product_more_rows_than_one_trip_of_the_count(gpu, seen, bp):
    M, K, N, a, b, ref, rows = ac.count_stride_case()
    ref, products = ref(np.float64), row_products(a, b)
    boundary = 65536 * 32                                        # kSgMaxGrid * (kBlock / kSgCountLanes)
    assert M == boundary + 70 and products[boundary + 3] > 64 and (products[boundary:] > 0).sum() > 40
    with upload(M, K, a) as da, upload(K, N, b) as db:
        got, st = check_product(da, db, ref, products, f"count stride bp={bp}", bp)
        same_as_before(seen, "count stride", got, f"bp={bp}")
        print(f"bp={bp}: ms = {st['ms']}")
    assert st["products"] == products.sum() and st["max_row_products"] == products.max() == products[boundary + 3]
    assert st["long_rows"] == (0 if bp == 0 else int((products > 64).sum())) and st["blocks"] > 0


# ---- 6. the sum: more long rows than sa_merge_long's grid
@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_with_more_long_rows_than_the_long_grid(gpu, dtype):
    M, N, a, b = ac.sum_case()
    a, b = as_dtype(a, dtype), as_dtype(b, dtype)
    want, matches, combined = spadd_ref(M, N, a, b, dtype, 1.5, -0.25)
    assert M > 4096 and combined.min() >= 2 and 0 < matches             # kSaLongGrid
    with upload(M, N, a) as da, upload(M, N, b) as db:
        def run(**kw):
            with da.add(db, 1.5, -0.25, method="merge", **kw) as dc:
                got, st = dc.download(), dc.add_info
            assert_same_arrays(got, want, f"sum {kw}")
            assert (st["nz"], st["matches"], st["a_canonical"], st["b_canonical"]) == (len(want[1]), matches, 1, 1)
            return b"".join(x.tobytes() for x in got), st

        off, st = run(long_row=NO_LONG)
        assert st["long_rows"] == 0
        for lanes in (1, 8):
            on, st = run(long_row=2, lanes=lanes)
            assert st["long_rows"] == M
            assert on == off, "the long tier against the lane tier"


# ---- 7. the transpose
@pytest.fixture(scope="module")
def tall():
    M, N, m = ac.transpose_case()
    return M, N, m, transpose_ref(M, N, *m)


@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_with_more_rows_than_the_grid_and_wide_rows(gpu, tall, dtype):
    M, N, m, (rp_t, col_t, val_t) = tall
    assert M == 4 * (1 << 20) + 70                               # kTrMaxGrid * (kBlock / 64) rows in one trip of the grid
    with upload(M, N, as_dtype(m, dtype)) as dev, dev.transpose() as dt:
        assert (dt.M, dt.N, dt.dtype) == (N, M, dtype)
        info = dt.info()
        assert (info["M_total"], info["N"], info["nz"]) == (N, M, len(m[1]))
        assert_same_arrays(dt.download(), (rp_t, col_t, val_t.astype(dtype)), "tall transpose")


@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_rows_of_64_65_and_129_entries(gpu, oracle, dtype):
    M, N, m = ac.transpose_case(boundary=230, sparse_rows=150)
    m = as_dtype(m, dtype)
    assert (M, N) == (300, 300) and {64, 65, 129} <= set(np.diff(m[0]).tolist())
    rp_t, col_t, val_t = transpose_ref(M, N, *m)
    with upload(M, N, m) as dev, dev.transpose() as dt:
        info = dt.info()
        assert (info["M_total"], info["N"], info["nz"]) == (N, M, len(m[1]))
        assert_same_arrays(dt.download(), (rp_t, col_t, val_t), "wide rows")
        x = np.random.default_rng(7).uniform(-1, 1, dt.N).astype(dtype)
        y = dt.spmv(x)
        if dtype == np.float32:
            assert_parity_f32(y, oracle.csr_f32_accum64(rp_t, col_t, val_t, x), rp_t, col_t, val_t, x, "wide rows A^T x")
        else:
            assert_parity(y, oracle.csr_serial(rp_t, col_t, val_t, x), rp_t, col_t, val_t, x, what="wide rows A^T x")
