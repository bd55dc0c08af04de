"""The operands of tests/test_gpu_algebra_edges.py (the product, the sum and the transpose beyond one tile and one grid),
their references, and the plan each case is written for.  Every construction is a plain function of its sizes, so
tests/test_algebra_refs_host.py can check, without a GPU, that the constructions give the plans they aim at and that the
tiled and expanded references of the large cases equal the plain loops at a reduced size.

Values have full mantissas (uniform(1, 2) with random signs): a changed order of additions or a fused multiply-add
changes bits.  Matrices are (row_ptr, col, val) triples with fp64 values; as_dtype rounds them for an fp32 run."""
import numpy as np

import sparsematrixvectormultiplication_amd as sp
from _spgemm_ref import spgemm_ref


# ---- small tools
def mantissa(rng, n):
    return rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)


def pack(N, col_rows, rng):
    """(row_ptr, col, val) from a list of column arrays, in the order given, with values of full mantissa"""
    lens = np.array([len(c) for c in col_rows], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.asarray(c, dtype=np.int64) for c in col_rows] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    assert col.size == 0 or (0 <= col.min() and col.max() < N)
    return rp, col, mantissa(rng, len(col))


def as_dtype(m, dtype):
    return m[0], m[1], m[2].astype(dtype)


def tile_csr(m, rows):
    """the rows of m repeated in a cycle until there are `rows` of them (np.tile: no loop over rows)"""
    rp, col, val = m
    reps = -(-rows // (len(rp) - 1))
    lens = np.tile(np.diff(rp.astype(np.int64)), reps)[:rows]
    n = int(lens.sum())                                          # whole cycles, then a prefix of the rows = of the entries
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.tile(col, reps)[:n], np.tile(val, reps)[:n]


def stack_csr(top, bottom):
    """the rows of top, then the rows of bottom"""
    rp = np.concatenate([top[0].astype(np.int64), top[0][-1] + bottom[0][1:].astype(np.int64)]).astype(np.int32)
    return rp, np.concatenate([top[1], bottom[1]]), np.concatenate([top[2], bottom[2]])


def expand_rows(m, rows, M):
    """m's rows placed at the (ascending) row numbers `rows` of a matrix of M rows that is empty elsewhere"""
    lens = np.zeros(M, dtype=np.int64)
    lens[rows] = np.diff(m[0].astype(np.int64))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), m[1], m[2]


def sorted_product_columns(a, b, i):
    """the columns of row i's products, sorted: position p is what the head loops see at p"""
    cols = [b[1][b[0][j]:b[0][j + 1]] for j in a[1][a[0][i]:a[0][i + 1]]]
    return np.sort(np.concatenate(cols + [np.zeros(0, dtype=np.int32)]), kind="stable")


def plan_stats(products, ref_row_ptr, block_products=0, chunk_products=0):
    """(matmul_info's stats by the host plan and the reference, the long rows of every chunk), vectorised over the rows:
    the launcher's rules (a block's long row is not its own; a block without products is not launched; a chunk takes
    whole rows while they fit)"""
    products = np.asarray(products, dtype=np.int64)
    cap = {0: 4096, -1: 0}.get(block_products, block_products)
    block_row, long_rows = sp.spgemm_plan(products, block_products)
    cum = np.concatenate([[0], np.cumsum(np.where(products <= cap, products, 0))])
    P = cum[block_row[1:]] - cum[block_row[:-1]]
    nrows = np.diff(block_row) - (products[block_row[1:] - 1] > cap)
    chunk_cap, chunk_rows, held = chunk_products or 1 << 23, [], 0
    for p in products[long_rows].tolist():
        if not chunk_rows or held + p > chunk_cap:
            chunk_rows.append(0)
            held = 0
        chunk_rows[-1] += 1
        held += p
    stats = dict(products=int(products.sum()), nz=int(ref_row_ptr[-1]), blocks=int((P > 0).sum()),
                 block_rows=int(nrows[P > 0].sum()), long_rows=len(long_rows), chunks=len(chunk_rows),
                 max_row_products=int(products.max(initial=0)),
                 max_row_nz=int(np.diff(np.asarray(ref_row_ptr, dtype=np.int64)).max(initial=0)))
    return stats, chunk_rows


# ---- 1. rows of A wider than one 256-entry tile of the expansion (kBlock = 256)
def wide_rows_case():
    """(M, K, N, a, b).  B: K = 700 rows, lengths 0 1 2 3 4 cycling over rows 0..255, rows 256..511 empty, 1 0 2 cycling
    over rows 512..699.  A: row 0 = columns 0..699 in order (three tiles: the middle one without a product, the last
    partial), rows of 257 (all on nonempty B rows), exactly 256 and 255 entries, an empty row, then short rows of 0 to 9
    entries, cut so that entry 1536 = 6 * 256 opens a row behind an empty one"""
    rng = np.random.default_rng(101)
    K, N = 700, 97
    lens = np.zeros(K, dtype=np.int64)
    lens[:256] = np.arange(256) % 5
    lens[512:] = np.array([1, 0, 2])[np.arange(K - 512) % 3]
    b_cols = []
    for n in lens:
        c = rng.integers(0, N, n)
        if n >= 3 and rng.random() < 0.5:
            c[-1] = c[0]                                         # a repeated column inside the row
        b_cols.append(c)
    b = pack(N, b_cols, rng)
    rows = [np.arange(K), rng.choice(np.flatnonzero(lens > 0), 257, replace=False), rng.integers(0, K, 256),
            rng.integers(0, K, 255), np.zeros(0, dtype=np.int64)]
    need = 6 * 256 - sum(len(r) for r in rows)                   # entries up to the tile boundary
    short = [rng.integers(0, K, int(n)) for n in rng.integers(0, 10, 45)]
    for i, r in enumerate(short):
        if len(r) >= need:
            short[i] = r[:need]
            short.insert(i + 1, np.zeros(0, dtype=np.int64))
            break
        need -= len(r)
    rows += short
    return len(rows), K, N, pack(K, rows, rng), b


# ---- 2. runs of equal keys longer than a batch of 256 sorted positions, and runs that start at a batch edge
def long_runs_case():
    """(M, K, N, a, b).  B rows 0..599 hold column 7 and one other column each, distinct per row (six of them below 7);
    rows 600..799 hold column 3 once, rows 800..849 twice.  A: row 0 reads rows 0..599 (C(0, 7) = 600 products in entry
    order, P = 1200); row 2 has column 3 at the sorted positions 0..255 and a run of 300 on column 7 from position 256;
    row 4 the same with 255.  Rows 1 and 3 are fillers of 80 and 168 products: in the one block of the on-chip tier row 2
    then starts at position 1280 = 5 * 256 and row 4 at 2304 = 9 * 256"""
    rng = np.random.default_rng(102)
    N = 610
    other = rng.permutation(np.concatenate([[0, 1, 2, 4, 5, 6], np.arange(8, 8 + 594)]))
    b_cols = [([7, o] if rng.random() < 0.5 else [o, 7]) for o in other]
    b_cols += [[3]] * 200 + [[3, 3]] * 50
    K = len(b_cols)
    b = pack(N, b_cols, rng)
    above = np.flatnonzero(other > 7)                            # their other column sorts behind column 7

    def threes_then_sevens(threes):
        singles = 600 + rng.choice(200, threes - 100, replace=False)
        return rng.permutation(np.concatenate([singles, np.arange(800, 850), rng.choice(above, 300, replace=False)]))

    rows = [rng.permutation(600), rng.choice(above, 40, replace=False), threes_then_sevens(256),
            rng.choice(above, 84, replace=False), threes_then_sevens(255)]
    return len(rows), K, N, pack(K, rows, rng), b


# ---- 3. a full block of the on-chip tier: 4096 rows, 4096 products (kSgMaxRows, kSgMaxProducts)
FULL = 4096


def full_block_case():
    """(M, K, N, a, b).  Rows 0..4095 of A: one product each (one block, P = 4096, local row 4095 in a key); row 4096:
    4096 products on 4096 distinct columns; row 4097: 4096 products on one column; row 4098: 4097 products (long); then
    4095 rows of one product and a row of two, which no longer fits their block"""
    rng = np.random.default_rng(103)
    N = 4200
    spread = rng.permutation(FULL).reshape(64, 64)
    b_cols = list(spread) + [[11] * 64] * 64 + [[N - 1]] + [[int(c)] for c in rng.integers(0, N, 50)]
    K = len(b_cols)
    b = pack(N, b_cols, rng)
    one = lambda: [129 + int(rng.integers(0, 50))]               # noqa: E731
    rows = [one() for _ in range(FULL)]
    rows += [rng.permutation(64), 64 + rng.permutation(64), rng.permutation(np.concatenate([np.arange(64), [128]]))]
    rows += [one() for _ in range(FULL - 1)] + [one() + one()]
    return len(rows), K, N, pack(K, rows, rng), b


# ---- 4. the global tier's sort width: col_bits + bits_for(rows of the chunk)
SORT_WIDTH_NS = [1, 2, 256, 257, (1 << 20) + 1]
SORT_WIDTH_CHUNK = 120                                           # chunk_products: chunks of 1, 2, 3, 4 and 5 long rows


def bits_for(n):
    """bits that hold 0 .. n - 1, at least one (the launcher's bits_for)"""
    bits = 1
    while (1 << bits) < n:
        bits += 1
    return bits


def sort_width_case(N):
    """(M, K, N, a, b).  B's row j holds j + 1 entries (K = 15, 120 in all) on the columns 0, N - 1, 2^(b - 1) - 1 and
    2^(b - 1) (b = bits_for(N)) and a few others.  A's long rows have 120 / r products in the chunk of r rows, r = 1..5,
    and all rows of a chunk read the same B rows with values of their own: rows k, k + 2 and k + 4 of a chunk share their
    columns, so a sort one bit short interleaves them.  Empty rows lie between the chunks."""
    rng = np.random.default_rng(104 + N % 1000)
    K, b = 15, bits_for(N)
    special = sorted({0, N - 1, (1 << (b - 1)) - 1, 1 << (b - 1)} & set(range(N)))
    pool = np.array(special + [int(c) for c in rng.integers(0, N, 3)])
    b_cols = [np.where(rng.random(j + 1) < 0.8, rng.choice(special, j + 1), rng.choice(pool, j + 1)) for j in range(K)]
    b_cols[K - 1][:len(special)] = special                       # every special column is there
    bm = pack(N, b_cols, rng)
    rows = []
    for r in range(1, 6):
        want, pick = SORT_WIDTH_CHUNK // r, []
        for j in range(K - 1, -1, -1):                           # B rows whose lengths 15, 14, .. 1 sum to `want`
            if j + 1 <= want:
                pick.append(j)
                want -= j + 1
        assert want == 0
        rows += [rng.permutation(pick) for _ in range(r)] + [np.zeros(0, dtype=np.int64)]
    return len(rows), K, N, pack(K, rows, rng), bm


# ---- 5. grid strides
SG_MAX_GRID = 65536                                              # kSgMaxGrid: workgroups of sg_block, sg_expand, sg_row_*
SG_COUNT_ROWS = 256 // 8                                         # kBlock / kSgCountLanes: rows of a workgroup of sg_count


def block_stride_case(periodic=SG_MAX_GRID, tail=206):
    """(M, K, N, a, b, ref(dtype)).  B: K = 9, N = 61, rows of 8 to 12 entries.  A: `periodic` rows that repeat 7 patterns
    of 4 to 6 entries, then `tail` random rows; every row has 33 to 64 products, so each is a block of its own at
    block_products = 64.  ref: spgemm_ref on the 7 patterns, tiled, and on the tail"""
    rng = np.random.default_rng(105)
    K, N = 9, 61
    lens = rng.integers(8, 13, K)
    b = pack(N, [rng.integers(0, N, n) for n in lens], rng)

    def row():
        while True:
            c = rng.integers(0, K, int(rng.integers(4, 7)))
            if 33 <= lens[c].sum() <= 64:
                return c

    pat, last = pack(K, [row() for _ in range(7)], rng), pack(K, [row() for _ in range(tail)], rng)
    a = stack_csr(tile_csr(pat, periodic), last)

    def ref(dtype):
        bd = as_dtype(b, dtype)
        return stack_csr(tile_csr(spgemm_ref(7, N, as_dtype(pat, dtype), bd, dtype), periodic),
                         spgemm_ref(tail, N, as_dtype(last, dtype), bd, dtype))

    return periodic + tail, K, N, a, b, ref


def count_stride_case(boundary=SG_MAX_GRID * SG_COUNT_ROWS, beyond=70, below=240, above=56):
    """(M, K, N, a, b, ref(dtype), rows).  A: M = boundary + beyond rows (boundary = the rows one trip of sg_count's grid
    takes), K = 40 columns, about 300 nonempty rows on both sides of the boundary, rows 5, boundary - 1, boundary and
    M - 1 among them; row boundary + 3 has more than 64 products.  ref: spgemm_ref on the nonempty rows alone, row_ptr
    expanded by a cumulative sum"""
    rng = np.random.default_rng(106)
    M, K, N = boundary + beyond, 40, 53
    lens = rng.integers(0, 9, K)
    b = pack(N, [rng.integers(0, N, n) for n in lens], rng)
    rows = np.unique(np.concatenate([[5, boundary - 1, boundary, boundary + 3, M - 1], rng.choice(boundary, below, replace=False),
                                     boundary + rng.choice(beyond, above, replace=False)]))
    a_rows = [rng.integers(0, K, int(n)) for n in rng.integers(1, 7, len(rows))]
    a_rows[int(np.searchsorted(rows, boundary + 3))] = rng.permutation(np.argsort(lens)[-12:])   # 12 rows of 6 entries or more
    small = pack(K, a_rows, rng)

    def ref(dtype):
        return expand_rows(spgemm_ref(len(rows), N, as_dtype(small, dtype), as_dtype(b, dtype), dtype), rows, M)

    return M, K, N, expand_rows(small, rows, M), b, ref, rows


# ---- 6. the sum: more long rows than sa_merge_long has workgroups
SA_LONG_GRID = 4096                                              # kSaLongGrid


def sum_case(M=SA_LONG_GRID + 300, N=500):
    """(M, N, a, b): canonical operands, every row with at least 2 combined entries and up to 40, every kind of match
    (all, none, the first column only, the last only, A's row empty, B's row empty, a random share)"""
    rng = np.random.default_rng(107)
    ra, rb = [], []
    for i in range(M):
        kind = i % 8 if i < 64 or rng.random() < 0.3 else 7
        u = np.sort(rng.choice(N, int(rng.integers(3, 21 if kind < 6 else 25)), replace=False))
        where = rng.integers(0, 2, len(u))                       # 0: A's, 1: B's
        where[:2] = [0, 1]                                       # (neither side empty where both are meant to hold some)
        if kind == 0:
            ca, cb = u, u
        elif kind == 1:
            ca, cb = u[where == 0], u[where == 1]
        elif kind == 2:
            ca, cb = np.union1d(u[:1], u[1:][where[1:] == 0]), np.union1d(u[:1], u[1:][where[1:] == 1])
        elif kind == 3:
            ca, cb = np.union1d(u[-1:], u[:-1][where[:-1] == 0]), np.union1d(u[-1:], u[:-1][where[:-1] == 1])
        elif kind == 4:
            ca, cb = u[:0], u
        elif kind == 5:
            ca, cb = u, u[:0]
        else:
            both = rng.random(len(u)) < 0.4
            ca, cb = u[both | (where == 0)], u[both | (where == 1)]
        ra.append(ca)
        rb.append(cb)
    return M, N, pack(N, ra, rng), pack(N, rb, rng)


# ---- 7. the transpose: rows wider than a wave's trip of 64 entries, and more rows than tr_make_pairs has waves
TR_GRID_ROWS = 4 << 20                                           # kTrMaxGrid * (kBlock / 64): rows of one trip of the grid


def transpose_case(boundary=TR_GRID_ROWS, sparse_rows=200_000, N=300):
    """(M, N, (row_ptr, col, val)).  M = boundary + 70; `sparse_rows` random rows below the boundary hold 1 to 5 entries,
    all of the last 70 rows hold some: row `boundary` 64, row M - 40 65 and row M - 1 129, unsorted with repeats"""
    rng = np.random.default_rng(108)
    M = boundary + 70
    lens = np.zeros(M, dtype=np.int64)
    lens[rng.choice(boundary, sparse_rows, replace=False)] = rng.integers(1, 6, sparse_rows)
    lens[boundary:] = rng.integers(1, 6, 70)
    lens[[boundary, M - 40, M - 1]] = [64, 65, 129]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return M, N, (rp, rng.integers(0, N, int(rp[-1])).astype(np.int32), mantissa(rng, int(rp[-1])))


def assert_same_arrays(got, want, what):
    for name, g, w in zip(("row_ptr", "col", "val"), got, want):
        assert g.dtype == w.dtype, f"{what} {name}: {g.dtype} vs {w.dtype}"
        assert g.shape == w.shape, f"{what} {name}: {g.shape} vs {w.shape}"
        if g.tobytes() != w.tobytes():
            bits = {4: np.uint32, 8: np.uint64}[g.itemsize]
            bad = np.flatnonzero(np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits))
            raise AssertionError(f"{what} {name}: {bad.size} of {g.size} differ, first at {bad[0]}: "
                                 f"{g[bad[0]]!r} vs {w[bad[0]]!r}")
