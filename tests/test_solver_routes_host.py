"""The matrices, values and CPU measurements behind test_gpu_solver_routes.py (every solver's steps on every SpMV route),
and what can be checked about them without a GPU.

Matrices (square, fixed seeds): a strict upper pattern U as U + U^T plus a full diagonal, columns sorted.
    band+arrow   n = 9001: a band of half-width 150, about 13 off-diagonal entries per row, three arrow rows (and
                 columns) of 2045, 2046 and 8193 stored entries -- one short of, at, and past the long-row limit
                 cap - 3 of the stages 2048 and 8192 -- and about 2 % of rows that hold their diagonal alone
    short        n = 20011: Poisson(1.2) uniformly placed entries per row of U (mean row 3.4, many diagonal-only rows):
                 csr_stream_short's regime, nz < M cap / 256
    tile         n = 60000: U's columns normally scattered around the diagonal (sigma 2500), about 4 per row: the
                 symmetric version of test_gpu_scaling.tile_cases' "packed"
    tile+stray   the same with 0.4 % of U's entries moved to uniform columns (the packed plan's remainder)
    tile+arrow   the same with three arrow rows of 5000 stored entries (the long-row tier / split rows)
    rect         the 7001 x 2 000 003 "gather passes" matrix of tile_cases, for CGLS alone
Values on a pattern (d_i: the off-diagonal entries of row i):
    lap     off-diagonal -1, diagonal 4 + d_i: every row sums to 4
    spd     off-diagonal SPD_SCALE u_ij / sqrt(d_i d_j), u symmetric and uniform in [-1, 1]; diagonal 1 + the row's
            off-diagonal absolute sum: eigenvalues within [1, 1 + 2 max_i R_i] by Gershgorin
    indef   spd with the diagonal negated on odd rows
    nonsym  spd's construction with independent values at (i, j) and (j, i)

MEASURED (test_gpu_solver_routes.py) is taken here, on the CPU, against the reference alone: the long-double loop
against the same recurrence in the handle's dtype with every product rounded and every row summed in that dtype, once
in entry order and once in reverse entry order (summed_product below, put in place of test_gpu_solver_sizes.product
for rounded_loop and handed to minres_ref)."""
import contextlib
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import sparsematrixvectormultiplication_amd as sp
import test_gpu_solver_sizes as sizes
from test_gpu_minres import minres_ref
from test_gpu_scaling import scattered, stray
from test_gpu_solver_sizes import differences, reference, rounded_loop

LD = np.longdouble
DTYPES = [np.float64, np.float32]
STEPS = sizes.STEPS

ARROWS = {"band+arrow": ((4500, 7, 8990), (2045, 2046, 8193)), "tile+arrow": ((11, 30000, 59990), (5000, 5000, 5000))}
SQUARE = ("band+arrow", "short", "tile", "tile+stray", "tile+arrow")
SPD_SCALE = 0.5        # R_i <= 0.5 sqrt(d_i) max_j d_j^-1/2: at most 7.8 on the arrow rows, a Gershgorin bound below 32
C_EXACT = 3            # b = 3 x 1 of the exact gate
C_COLUMNS = (3, 1, 2, 4, 5, 6, 7, 8)     # cg_multi's columns c_j x 1


# ---------------------------------------------------------------- patterns
def symmetric(n, ui, uj):
    """(row_ptr, col) of U + U^T + I for the pairs (ui, uj), whichever way round and however often they occur"""
    ui, uj = np.asarray(ui, np.int64), np.asarray(uj, np.int64)
    keep = ui != uj
    d = np.arange(n)
    i, j = np.concatenate([ui[keep], uj[keep], d]), np.concatenate([uj[keep], ui[keep], d])
    a = sps.csr_matrix((np.ones(len(i)), (i, j)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def pairs_of(rp, col):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    up = col > rows
    return rows[up], col[up].astype(np.int64)


def with_arrows(rng, n, rp, col, rows, totals, banned=None, spans=None):
    """the symmetric pattern with rows (and columns) `rows` brought to exactly `totals` stored entries: new partners are
    drawn among the columns the row does not hold yet, outside `rows` and outside `banned` (a mask), and within
    `spans` columns of the row where that is given"""
    ui, uj = pairs_of(rp, col)
    free = np.ones(n, bool) if banned is None else ~banned
    free[list(rows)] = False
    for k, (r, total) in enumerate(zip(rows, totals)):
        have = col[rp[r]:rp[r + 1]]
        cand = free.copy()
        cand[have] = False
        if spans is not None and spans[k]:
            cand[:max(r - spans[k], 0)] = False
            cand[r + spans[k] + 1:] = False
        new = rng.choice(np.flatnonzero(cand), total - len(have), replace=False)
        ui, uj = np.concatenate([ui, np.full(len(new), r)]), np.concatenate([uj, new])
    return symmetric(n, ui, uj)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(M, N, row_ptr, col) of one of the matrices above"""
    if name == "band+arrow":
        rng = np.random.default_rng(2101)
        n = 9001
        rows, totals = ARROWS[name]
        lone = rng.random(n) < 0.02
        lone[list(rows)] = False
        ui = np.repeat(np.arange(n), rng.poisson(6.5, n))
        uj = ui + rng.integers(1, 151, len(ui))
        keep = uj < n
        ui, uj = ui[keep], uj[keep]
        keep = ~lone[ui] & ~lone[uj]
        rp, col = symmetric(n, ui[keep], uj[keep])
        # the row of 2045 is no long row at the stage of 2048: it sits in an x-window block, which lists at most 256
        # lines of x (4096 fp64 values), so its partners stay within 1600 columns of it
        return (n, n) + with_arrows(rng, n, rp, col, rows, totals, banned=lone, spans=(1600, 0, 0))
    if name == "short":
        rng = np.random.default_rng(2102)
        n = 20011
        ui = np.repeat(np.arange(n), rng.poisson(1.2, n))
        return (n, n) + symmetric(n, ui, rng.integers(0, n, len(ui)))
    if name in ("tile", "tile+stray", "tile+arrow"):
        rng = np.random.default_rng(2103)
        n = 60000
        rp, col = scattered(rng, n, n, 4, sigma=2500)
        if name == "tile+stray":
            col = stray(rng, rp, col, n, 0.004)
        ui = np.repeat(np.arange(n), np.diff(rp))
        keep = (col > 0) & (col < n - 1)      # (scattered() clips at the edges: columns 0 and n - 1 would become long rows)
        rp, col = symmetric(n, ui[keep], col[keep])
        if name == "tile+arrow":
            rp, col = with_arrows(rng, n, rp, col, *ARROWS[name])
        return (n, n) + (rp, col)
    if name == "rect":
        M, N = 7001, 2_000_003
        return (M, N) + scattered(np.random.default_rng(105), M, N, 18)   # tile_cases' first draw
    raise KeyError(name)


# ---------------------------------------------------------------- values
@functools.lru_cache(maxsize=None)
def values(name, kind):
    """fp64 values of `kind` on the pattern of matrix(name) (rect: uniform in [-1, 1])"""
    M, N, rp, col = matrix(name)
    rng = np.random.default_rng([SQUARE.index(name) if name in SQUARE else 9, ["lap", "spd", "indef", "nonsym"].index(kind)])
    if name == "rect":
        return rng.uniform(-1, 1, len(col))
    rows = np.repeat(np.arange(M), np.diff(rp))
    off = rows != col
    deg = (np.diff(rp) - 1).astype(np.float64)
    if kind == "lap":
        return np.where(off, -1.0, 4.0 + deg[rows])
    if kind == "nonsym":
        u = rng.uniform(-1, 1, len(col))
    else:   # one value per unordered pair
        key = np.minimum(rows, col).astype(np.int64) * M + np.maximum(rows, col)
        _, inv = np.unique(key, return_inverse=True)
        u = rng.uniform(-1, 1, int(inv.max()) + 1)[inv]
    val = np.zeros(len(col))
    val[off] = SPD_SCALE * u[off] / np.sqrt(deg[rows[off]] * deg[col[off]])
    radius = np.bincount(rows, weights=np.abs(val), minlength=M)
    diag = 1.0 + radius
    if kind == "indef":
        diag[1::2] *= -1.0
    val[~off] = diag
    return val


def held(name, kind, dtype):
    """the values as a handle of dtype holds them"""
    return values(name, kind).astype(dtype)


def rhs(n, dtype, seed, k=None):
    rng = np.random.default_rng([n, seed, 31])
    return rng.uniform(-1, 1, n if k is None else (n, k)).astype(dtype)


def diagonal(name, kind, dtype):
    M, _, rp, col = matrix(name)
    rows = np.repeat(np.arange(M), np.diff(rp))
    return held(name, kind, dtype)[rows == col].astype(np.float64)


# ---------------------------------------------------------------- the reference with in-row summation in the dtype
def summed_product(rp, col, val, dtype, reverse=False):
    """v -> A v as fp64 values, every product rounded to dtype and every row summed in dtype one entry after the other,
    in entry order or in reverse entry order"""
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    vals = np.asarray(val).astype(dtype)
    is_short = lens <= 64          # (the few longer rows: one at a time)
    groups = [np.flatnonzero(is_short & (lens > p)) for p in range(int(lens[is_short].max(initial=0)))]
    long_rows = np.flatnonzero(~is_short)

    def apply(v):
        prod = vals * np.asarray(v).astype(dtype)[col]
        y = np.zeros(len(lens), dtype)
        for p, rows in enumerate(groups):
            at = rp[rows + 1] - 1 - p if reverse else rp[rows] + p
            y[rows] = y[rows] + prod[at]
        for r in long_rows:
            seg = prod[rp[r]:rp[r + 1]]
            y[r] = np.cumsum(seg[::-1] if reverse else seg, dtype=dtype)[-1]
        return y.astype(np.float64)
    return apply


@contextlib.contextmanager
def product_summed_in(dtype, reverse):
    """rounded_loop (test_gpu_solver_sizes.py) over summed_product instead of its once-rounded fp64 product"""
    keep = sizes.product
    sizes.product = lambda rp, col, val, acc=None: summed_product(rp, col, val, dtype, reverse)
    try:
        yield
    finally:
        sizes.product = keep


SOLVERS = ("cg", "pcg", "pcg_jacobi", "minres", "minres_indef", "bicgstab", "pbicgstab", "cgls", "cg_multi", "pcg_multi")
KIND_OF = {"cg": "spd", "pcg": "spd", "pcg_jacobi": "spd", "minres": "spd", "minres_indef": "indef", "bicgstab": "nonsym",
           "pbicgstab": "nonsym", "cgls": "nonsym", "cg_multi": "spd", "pcg_multi": "spd"}
KIND_OF["minres_lap"] = "lap"     # one MINRES step on lap with b = C_EXACT x 1: see measured_cases
K_MULTI = {"cg_multi": 8, "pcg_multi": 8}
# (cg_multi runs k = 2, 8 and 3: the first columns of the same B, so the eight columns' figures cover them)


def problem(solver, name, dtype):
    """test_gpu_solver_sizes.problem's tuple (M, N, row_ptr, col, val in dtype, b, Jacobi's stored inverse or None)"""
    M, N, rp, col = matrix(name)
    kind = "nonsym" if name == "rect" else KIND_OF[solver]
    val = held(name, kind, dtype)
    b = np.full(M, C_EXACT, dtype) if solver == "minres_lap" else rhs(M, dtype, 5, K_MULTI.get(solver))
    inv = None
    if solver in ("pcg_jacobi", "pbicgstab", "pcg_multi"):
        inv = (1.0 / diagonal(name, kind, dtype)).astype(dtype)
    return M, N, rp, col, val, b, inv


SIZES_NAME = {"pcg_jacobi": "pcg", "minres_indef": "minres", "minres_lap": "minres"}


def loop(solver, prob, iters, dtype=None, reverse=False):
    """(x, the histories) after iters steps: the long-double loops of the other solver tests (dtype None), or the same
    recurrences with every stored vector rounded to dtype and every row summed in dtype"""
    M, N, rp, col, val, b, inv = prob
    base = SIZES_NAME.get(solver, solver)
    rd = None if dtype is None else (lambda v: np.asarray(v).astype(dtype).astype(np.float64))
    if base == "minres":
        A = sizes.product(rp, col, val, LD) if dtype is None else summed_product(rp, col, val, dtype, reverse)
        x, h, _ = minres_ref(A, b.astype(np.float64), iters, rd=rd)
        return x, [h]
    if base == "pcg_multi":
        out = [loop("pcg_jacobi", (M, N, rp, col, val, np.ascontiguousarray(b[:, j]), inv), iters, dtype, reverse)
               for j in range(b.shape[1])]
        return np.stack([o[0] for o in out], axis=1), [np.stack([o[1][i] for o in out], axis=1) for i in (0, 1)]
    if dtype is None:
        return reference(base, prob, iters)
    with product_summed_in(dtype, reverse):
        return rounded_loop(base, prob, iters, rd)


def measure(solver, name, dtype):
    """the largest difference, over the step counts and the two orders, between the long-double loop and the loop in
    dtype: (the figure, steps, order, x's share, the histories' share)"""
    prob = problem(solver, name, dtype)
    worst = (0.0, 0, "", 0.0, 0.0)
    for iters in ((1,) if solver == "minres_lap" else STEPS):   # (its residual vanishes: a second step divides by rounding)
        ref = loop(solver, prob, iters)
        for reverse in (False, True):
            dx, dh = differences(loop(solver, prob, iters, dtype, reverse), ref)
            if max(dx, dh) > worst[0]:
                worst = (max(dx, dh), iters, "reverse" if reverse else "entry", dx, dh)
    return worst


def measured_cases():
    """(solver, matrix) of every MEASURED entry.  minres_lap: MINRES's first vector is b / |b|, no representable number,
    so on lap its product rounds ((4 + d) v and d subtractions of v) and x = b / 4 holds to that rounding only -- unlike
    the other solvers of the exact gate, whose first product is of b itself"""
    for name in SQUARE:
        for solver in SOLVERS + ("minres_lap",):
            yield solver, name
    yield "cgls", "rect"


# ---------------------------------------------------------------- the builders' invariants
def gershgorin(M, rp, col, val):
    rows = np.repeat(np.arange(M), np.diff(rp))
    d = val[rows == col]
    radius = np.bincount(rows, weights=np.abs(val), minlength=M) - np.abs(d)
    return d, radius


@pytest.mark.parametrize("name", SQUARE)
def test_patterns_are_what_the_routes_need(name):
    M, N, rp, col = matrix(name)
    rows = np.repeat(np.arange(M), np.diff(rp))
    lens = np.diff(rp)
    assert M == N and np.all(np.diff(col)[np.diff(rows) == 0] > 0), "sorted, distinct columns"
    assert np.all(sps.csr_matrix((np.ones(len(col)), col, rp), shape=(M, N)).diagonal() == 1), "a full diagonal"
    a = sps.csr_matrix((np.ones(len(col)), col, rp), shape=(M, N))
    assert (a != a.T).nnz == 0, "a symmetric pattern"
    assert len(col) <= 600_000
    if name in ARROWS:
        where, totals = ARROWS[name]
        assert lens[list(where)].tolist() == list(totals)
        assert np.sort(lens)[-4] < 64, "the arrow rows are the only long ones"
    if name == "band+arrow":
        assert 0.01 * M < (lens == 1).sum() < 0.03 * M
        assert [int((lens > cap - 3).sum()) for cap in (2048, 8192)] == [2, 1]
        inner = np.abs(col.astype(np.int64) - rows) <= 150
        assert np.all(inner | np.isin(rows, where) | np.isin(col, where)), "a band of half-width 150 and the arrows"
        first = col[rp[where[0]]:rp[where[0] + 1]]
        assert (first.max() >> 4) - (first.min() >> 4) < 256, "the row of 2045 fits one x-window block's line list"
        assert 12 < (lens.sum() - 2 * sum(totals)) / M < 15
    if name == "short":
        assert 3.2 < lens.mean() < 3.6 and (lens == 1).sum() > 0.05 * M
        assert len(col) < M * (2048 // 256), "csr_stream_short's regime at the stage of 2048"
        assert lens.max() <= max(64, 8 * lens.mean()), "AUTO's lane-group kernel (spmv_csr.hip: no skewed rows)"
    if name.startswith("tile"):
        assert 8 <= np.median(lens) <= 10, "about 4 entries per row of U"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", SQUARE)
def test_values_are_symmetric_where_claimed_and_strictly_dominant(name, dtype):
    M, N, rp, col = matrix(name)
    for kind in ("lap", "spd", "indef", "nonsym"):
        val = held(name, kind, dtype).astype(np.float64)
        a = sps.csr_matrix((val, col, rp), shape=(M, N))
        assert ((a != a.T).nnz == 0) == (kind != "nonsym"), (kind, "symmetry")
        d, radius = gershgorin(M, rp, col, val)
        assert np.all(np.abs(d) > radius), (kind, "strict diagonal dominance")
        if kind == "lap":
            deg = np.diff(rp) - 1
            assert np.all(val[val < 0] == -1.0) and np.all(d == 4 + deg) and np.all(a @ np.ones(M) == 4.0)
            for c in C_COLUMNS:   # every partial sum of a row and the dot products of one step are integers below 2^24
                assert (4 + 2 * int(deg.max())) * 4 * c < 2 ** 24 and 4 * M * c * c < 2 ** 24
        if kind == "spd":
            assert np.all(d > 0)
            bound = float(np.max(d + radius) / np.min(d - radius))
            assert bound <= 32.0, (name, bound)
        if kind == "indef":
            assert np.all(d[1::2] < 0) and np.all(d[0::2] > 0)


# ---------------------------------------------------------------- what the CPU can say about the plans
def test_stream_plans_decided_on_the_host():
    """spmv_hip_csr_plan_check rebuilds upload's blocks: band+arrow gets x-window blocks and keeps the arrow rows as
    long rows; short gets neither"""
    for vb in (8, 4):
        M, N, rp, col = matrix("band+arrow")
        st = sp.csr_plan_check(M, N, rp, col, vb)
        assert st["local_blocks"] > 0 and st["long_rows"] > 0, st
        M, N, rp, col = matrix("short")
        st = sp.csr_plan_check(M, N, rp, col, vb)
        assert st["local_blocks"] == 0 and st["long_rows"] == 0, st


TILE_KNOBS = {
    "tile-packed": ("tile", dict(stream_tile=1, tile_rows=2048, stream_local=0)),
    "tile-remainder": ("tile+stray", dict(stream_tile=1, tile_rows=2048, stream_local=0)),
    # (tile_density = 0: no window is dense enough to stage.  At the default, one entry per 4 columns, every square
    # matrix of up to 600 000 entries stages most of its passes, uniformly scattered columns included.)
    "tile-gather": ("tile", dict(stream_tile=1, tile_rows=1024, tile_pack=0, tile_expand=0, tile_density=0, stream_local=0)),
    "tile-expanded": ("tile", dict(stream_tile=1, tile_rows=1024, tile_expand=1, tile_lmax=4096, tile_density=0, tile_pack=0,
                                   stream_local=0)),
    "tile-long": ("tile+arrow", dict(stream_tile=1, tile_rows=512, tile_lmax=700, tile_long=2, stream_local=0)),
    "tile-split": ("tile+arrow", dict(stream_tile=1, tile_rows=512, tile_lmax=700, tile_long=0, stream_local=0)),
}


@pytest.mark.parametrize("route", sorted(TILE_KNOBS))
def test_tile_plans_decided_on_the_host(route):
    """spmv_hip_csr_tile_auto_plan under each tile route's upload knobs: tiles, packed or not as the route needs, the
    rows beyond tile_lmax kept out of the ordinary tiles; spmv_hip_csr_tile_plan_check on the same block height."""
    name, knobs = TILE_KNOBS[route]
    M, N, rp, col = matrix(name)
    lens = np.diff(rp)
    for vb in (8, 4):
        with sp.tuning(**knobs):
            st = sp.csr_tile_auto_plan(M, N, rp, col, vb)
        assert st["tiles"] == 1 and st["rows_per_block"] == knobs["tile_rows"], st
        assert st["packed"] == int(route in ("tile-packed", "tile-remainder")), st
        lmax = knobs.get("tile_lmax", 1536)
        in_tiles = int(lens[lens <= lmax].sum())
        if st["packed"]:   # (what sits in windows too sparse for a pass is left to the remainder kernel)
            assert 0 < in_tiles - st["entries"] <= 0.04 * in_tiles, st
        else:
            assert st["entries"] == in_tiles, st
        assert (st["long_items"] > 0) == (route == "tile-long"), st
        chk = sp.csr_tile_plan_check(M, N, rp, col, vb, knobs["tile_rows"], lmax=lmax)
        assert chk["split_rows"] == int((lens > lmax).sum()) == 3 * (name == "tile+arrow") and chk["entries"] == in_tiles, chk


# ---------------------------------------------------------------- MEASURED, recomputed
@pytest.mark.parametrize("name", SQUARE + ("rect",))
def test_recorded_fp32_measurements_cover_the_recomputed_ones(name):
    """Every fp32 entry of test_gpu_solver_routes.MEASURED, taken again: none may exceed what is recorded (the table
    holds four digits, as printed)."""
    from test_gpu_solver_routes import MEASURED
    for solver, mname in measured_cases():
        if mname != name:
            continue
        got = float(f"{measure(solver, name, np.float32)[0]:.3e}")
        assert got <= MEASURED[(solver, "float32", name)], (solver, name, got, MEASURED[(solver, "float32", name)])
