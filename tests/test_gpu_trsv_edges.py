"""The kernels of trsv_kernels.hpp (trsv_rows under trsv_level and trsv_chain, ilu0_row under ilu0_level and ilu0_chain)
at their own edges: every lane-group width G in {1, 2, 4, 8, 16, 32} and the rule that picks it, rows either side of the
long-row length (128), levels either side of the chain limits (256 rows, 4096 entries), levels past the grid caps, SSOR
and ILU(0) applies with wide groups and wavefront rows, and ILU(0) on rows wider than a wavefront.

The matrices are built level by level (test_trsv_host.layered): the rows of a level are neighbours, level 0 holds the
empty rows, a row of level l reads a run of earlier rows that ends in level l - 1.  Levels, lengths, the launch plan and
the expected lanes per row are therefore known by construction; up to a few thousand rows the per-row restatements
(levels_ref) are run as well.  The upper triangle of every matrix is the mirror image of its lower one.

References, none of them measured: the row-wise residual bound of test_gpu_trsv.py for every solve; unit triangles
with entries in {-1, 1} and integer right-hand sides solved in Python integers, every partial sum below 2^53 (2^24), for
the exact gates; tri_apply_bound for the applies; pattern equality and |(LU - A)_ij| <= (k_i + 2) eps (|L||U|)_ij for
ILU(0), and on dense integer blocks, where ILU(0) is LU and every intermediate is an integer, the factors bit for bit.

Each test prints what info() / tri_info() reported (lines that start with "edges:")."""
import functools

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from test_gpu_bicgstab import nonsym_banded
from test_gpu_solver_sizes import tri_apply_bound
from test_gpu_trsv import assert_row_residual, csr, dominant, order_of, permuted, scipy_factor, triangle
from test_trsv_host import (CHAIN_EDGES, both_sides, canonical, lanes_ref, layered, levels_ref, mirrored, plan_ref,
                            rows_of)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
DTYPE_IDS = ["fp64", "fp32"]
WIDTHS = [1, 2, 4, 8, 16, 32]
K_BLOCK = 256          # kBlock
K_TRSV_BLOCKS = 2048   # kTrsvBlocks: the grid cap of trsv_level and ilu0_level
PER_ROW_LOOPS = 6000   # rows up to which levels_ref (a Python loop over the rows) is run next to the construction


def report(what, **values):
    print(f"edges: {what}: " + ", ".join(f"{k} = {v}" for k, v in values.items()))


# ---------------------------------------------------------------- matrices by construction
def width_lengths(G, sizes, rng):
    """lengths for layered(): levels of sizes[l] rows, the lengths of the rows past level 0 drawn from
    {1, G - 1, G, G + 1, 2 G + 1, 127} (0 is level 0 itself), clipped to the rows a level can read, with weights
    exp(theta length) and theta set so that the mean over ALL short rows, the empty ones included, is the middle of the
    interval in which tri_upload picks G; every length occurs at least once per 125 rows of a level"""
    target = {1: 1.2, 2: 3.0, 4: 6.0, 8: 12.0, 16: 24.0, 32: 48.0}[G]
    n = sum(sizes)
    mu = target * n / (n - sizes[0])
    lengths, start = [np.zeros(sizes[0], np.int64)], sizes[0]
    for size in sizes[1:]:
        v = np.unique(np.minimum([k for k in (1, G - 1, G, G + 1, 2 * G + 1, 127) if k >= 1], start))
        reps = size // 125                       # every length this often, whatever the weights
        rest = size - reps * len(v)
        want = (mu * size - reps * v.sum()) / rest
        lo, hi = -80.0, 80.0
        for _ in range(80):
            theta = 0.5 * (lo + hi)
            p = np.exp(theta * (v - v.max()) / 127.0)
            p /= p.sum()
            lo, hi = (theta, hi) if p @ v < want else (lo, theta)
        k = np.concatenate([np.tile(v, reps), rng.choice(v, rest, p=p)])
        rng.shuffle(k)
        lengths.append(k.astype(np.int64))
        start += size
    return lengths


def width_level_sizes(G):
    """three levels; one of them takes its rows from {1, 64 / G - 1, 64 / G + 1, 256 / G + 1, 1000}: a wave with groups
    that have no row, a chained level of several passes (256 / G + 1 rows of G lanes), a wide level.  The other two have
    1000 rows: the rows of a level can only be as long as there are rows before them, and the empty level 0 counts in
    the mean, so a small first level would keep every G above 2 out of reach."""
    for i, x in enumerate(sorted({1, 64 // G - 1, 64 // G + 1, 256 // G + 1, 1000} - {0})):
        yield (1000, x, 1000) if i % 2 == 0 else (1000, 1000, x)


def with_long_rows(lengths, rng, longs=(128, 129, 150, 300)):
    """a few rows of every level past the first made long"""
    out = [lengths[0]]
    for k in lengths[1:]:
        k = k.copy()
        k[rng.choice(len(k), len(longs), replace=False)] = longs
        out.append(k)
    return out


def case_lengths():
    """name -> (lengths, seed)"""
    cases = {}
    for G in WIDTHS:
        for sizes in width_level_sizes(G):
            cases[f"G{G} {sizes[1]}x{sizes[2]}"] = (width_lengths(G, sizes, np.random.default_rng(100 + G)), 200 + G)
        # the rule's own edges: a mean of exactly 2 G picks G, one entry more picks 2 G
        if G < 32:
            cases[f"mean {2 * G}"] = ([np.zeros(128, np.int64), np.full(128, 4 * G)], 300 + G)
            cases[f"mean {2 * G} + 1 entry"] = ([np.zeros(128, np.int64), rows_of((127, 4 * G), (1, 4 * G + 1))],
                                                300 + G)
    # ---- the long-row split: a level of long rows only, of short rows only, of both; each wide and narrow
    longs = (128, 129, 191, 192, 193, 1000)
    split = {"long wide": rows_of(*[(3, k) for k in longs]),
             "long narrow": rows_of(*[(1, k) for k in longs]),
             "long narrow 32x128": rows_of((32, 128)),
             "short wide": rows_of((100, 127), (100, 1), (100, 64)),
             "short narrow": rows_of((10, 127), (10, 1), (12, 64)),
             "both wide": rows_of((150, 127), (3, 128), (150, 5), (1, 1000), (2, 129), (1, 191), (1, 192), (1, 193)),
             "both narrow": rows_of((8, 127), (1, 128), (5, 3), (1, 1000), (1, 129), (1, 191), (1, 192), (1, 193))}
    names = list(split)
    for i, name in enumerate(names):             # the level after it: the next kind, so every pair of neighbours occurs
        cases[name] = ([np.zeros(1100, np.int64), split[name], split[names[(i + 1) % len(names)]]], 400 + i)
    # ---- the chain limits
    cases["rows 256 | 257"] = ([np.zeros(300, np.int64), rows_of((256, 4)), rows_of((257, 4)), rows_of((256, 4)),
                                rows_of((10, 2))], 500)
    cases["entries 4096 | 4097"] = ([np.zeros(300, np.int64), rows_of((64, 64)), rows_of((63, 64), (1, 65)),
                                    rows_of((64, 64))], 501)
    cases["narrow narrow wide narrow narrow"] = ([np.zeros(10, np.int64), rows_of((20, 3)), rows_of((300, 7)),
                                                 rows_of((30, 5)), rows_of((40, 9))], 502)
    cases["G32 256 rows chained"] = ([np.zeros(200, np.int64), rows_of((600, 100)), rows_of((256, 16))], 503)
    cases["G16 256 rows chained"] = ([np.zeros(200, np.int64), rows_of((600, 40)), rows_of((256, 16)),
                                     rows_of((256, 16))], 504)
    cases["chain edges"] = (CHAIN_EDGES, 505)
    # ---- the grid caps
    rng = np.random.default_rng(600)
    cases["cap 17000 rows G32"] = ([np.zeros(200, np.int64), rng.integers(40, 81, 17000)], 601)
    cases["cap 530000 rows G1"] = ([np.zeros(100, np.int64), rng.integers(1, 3, 530000)], 602)
    cases["cap 8300 long rows"] = ([np.zeros(200, np.int64), np.full(8300, 128)], 603)
    # ---- the applies
    for G in (16, 32):
        rng = np.random.default_rng(700 + G)
        cases[f"apply G{G}"] = (with_long_rows(width_lengths(G, (400, 400, 400), rng), rng), 710 + G)
    return cases


LENGTHS = case_lengths()
PLANS = {"rows 256 | 257": [[0, 0, 1], [1, 1, 2], [0, 2, 3], [1, 3, 5]],
         "entries 4096 | 4097": [[0, 0, 1], [1, 1, 2], [0, 2, 3], [1, 3, 4]],
         "narrow narrow wide narrow narrow": [[1, 0, 2], [0, 2, 3], [1, 3, 5]],
         "G32 256 rows chained": [[1, 0, 1], [0, 1, 2], [1, 2, 3]],
         "G16 256 rows chained": [[1, 0, 1], [0, 1, 2], [1, 2, 4]]}
LANES = {"G32 256 rows chained": 32, "G16 256 rows chained": 16, "cap 17000 rows G32": 32, "cap 530000 rows G1": 1,
         "cap 8300 long rows": 1, "apply G16": 16, "apply G32": 32,
         **{f"G{G} {s[1]}x{s[2]}": G for G in WIDTHS for s in width_level_sizes(G)},
         **{f"mean {2 * G}": G for G in WIDTHS[:-1]}, **{f"mean {2 * G} + 1 entry": 2 * G for G in WIDTHS[:-1]}}


@functools.lru_cache(maxsize=2)
def built(name):
    """(M, rp, col, val) in fp64: both_sides(lengths) with uniform values and `dominant` scaling"""
    lengths, seed = LENGTHS[name]
    rng = np.random.default_rng(seed)
    a = both_sides(lengths, rng)
    a.data = rng.uniform(0.1, 1.0, a.nnz) * rng.choice([-1.0, 1.0], a.nnz)
    return dominant(a, rng)


def built_levels(name, lower):
    """level of every row, from the construction alone"""
    sizes = [len(k) for k in LENGTHS[name][0]]
    level = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    return level if lower else level[::-1].copy()


def check_solves(name, dtype, twice=False):
    """lower and upper, unit and non-unit: the row bound on every row, info() against the construction and plan_ref"""
    M, rp, col, val = built(name)
    lengths = LENGTHS[name][0]
    val = val.astype(dtype)
    b = np.random.default_rng(5).uniform(-1, 1, M).astype(dtype)
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        for lower in (True, False):
            t, d = triangle(rp, col, val, dtype, lower)
            level = built_levels(name, lower)
            assert t.nnz == sum(int(k.sum()) for k in lengths)
            assert sorted(np.diff(t.indptr).tolist()) == sorted(np.concatenate(lengths).tolist())
            if M <= PER_ROW_LOOPS:
                assert np.array_equal(levels_ref(t, lower), level), name
            plan = plan_ref(t, level)
            assert name not in PLANS or plan == PLANS[name], (name, plan)
            assert name not in LANES or lanes_ref(t) == LANES[name], (name, lanes_ref(t))
            for unit in (False, True):
                what = f"{name} {np.dtype(dtype)} lower={lower} unit={unit}"
                with dev.triangular(lower=lower, unit_diagonal=unit) as T:
                    x = T.solve(b)
                    info = T.info()
                    if twice:
                        assert T.solve(b).tobytes() == x.tobytes(), what
                assert x.dtype == dtype and x.shape == (M,)
                assert_row_residual(t, None if unit else d, b, x, dtype, what)
                assert info["lanes_per_row"] == lanes_ref(t), (what, info)
                assert info["levels"] == len(lengths) and info["launches"] == len(plan), (what, info, plan)
                assert info["widest"] == max(len(k) for k in lengths) and info["entries"] == t.nnz, (what, info)
                assert info["rows"] == M and info["value_bytes"] == np.dtype(dtype).itemsize
            report(f"{name} {np.dtype(dtype)} lower={lower}", lanes_per_row=info["lanes_per_row"],
                   levels=info["levels"], launches=info["launches"], widest=info["widest"], entries=info["entries"],
                   kernels="".join("c" if k[0] else "l" for k in plan))
    return plan


# ---------------------------------------------------------------- 1. every lane-group width and the rule that picks it
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", [n for n in LENGTHS if n.startswith("G") and "chained" not in n])
def test_every_lane_group_width(gpu, name, dtype):
    """Three levels, lengths from {1, G - 1, G, G + 1, 2 G + 1, 127}, lanes_per_row == G (LANES), the row bound on
    every row.  The level of 256 / G + 1 rows is chained for G >= 2 and takes two passes of the workgroup."""
    plan = check_solves(name, dtype)
    G, sizes = LANES[name], [len(k) for k in LENGTHS[name][0]]
    if G >= 2 and 256 // G + 1 in sizes:
        l = sizes.index(256 // G + 1)
        assert any(k == 1 and l0 <= l < l1 for k, l0, l1 in plan) and sizes[l] * G > K_BLOCK, (name, plan)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", [n for n in LENGTHS if n.startswith("mean")])
def test_the_rule_that_picks_the_width_at_its_edges(gpu, name, dtype):
    """256 short rows, 128 of them empty: a mean of exactly 2, 4, 8, 16, 32 gives G = 1, 2, 4, 8, 16 (2 G < mean is
    false), one entry more in total gives 2, 4, 8, 16, 32"""
    check_solves(name, dtype)


def int_solve(t, b, lower):
    """(x, peak) of the unit triangle I + t in Python integers; peak = max_i |b_i| + sum_j |t_ij x_j| bounds every
    partial sum of every row in any order of addition"""
    n = t.shape[0]
    x, peak = [0] * n, 0
    rp, col, val = t.indptr.tolist(), t.indices.tolist(), [int(v) for v in t.data]
    bi = [int(v) for v in b]
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        terms = [val[e] * x[col[e]] for e in range(rp[i], rp[i + 1])]
        x[i] = bi[i] - sum(terms)
        peak = max(peak, abs(bi[i]) + sum(abs(v) for v in terms))
    return x, peak


def check_integer_gate(lengths, seed, dtype, lanes, what):
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    s = layered(lengths, rng)
    s.data = rng.choice([-1.0, 1.0], s.nnz)
    M, rp, col, val = csr(s + mirrored(s) + sps.eye(s.shape[0]))
    b = rng.integers(-100, 101, M)
    limit = 2 ** (53 if dtype == np.float64 else 24)
    with sp.CsrDevice(M, M, rp, col, val.astype(dtype)) as dev:
        for lower in (True, False):
            t = s if lower else mirrored(s)
            assert set(np.unique(t.data).tolist()) == {-1.0, 1.0}
            x_ref, peak = int_solve(t, b, lower)
            assert isinstance(peak, int) and peak < limit, (what, peak)
            with dev.triangular(lower=lower, unit_diagonal=True) as T:
                x = T.solve(b.astype(dtype))
                info = T.info()
            assert (info["lanes_per_row"], info["levels"]) == (lanes, len(lengths)), (what, info)
            assert x.tobytes() == np.array(x_ref, dtype=dtype).tobytes(), (what, lower)
            report(f"{what} {np.dtype(dtype)} lower={lower}", lanes_per_row=info["lanes_per_row"],
                   levels=info["levels"], launches=info["launches"], peak=peak)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("G", WIDTHS)
def test_rows_of_about_one_group_are_exact_on_small_integers(gpu, G, dtype):
    """Unit triangles, entries in {-1, 1}, three levels, rows of exactly G - 1, G, G + 1 and 2 G + 1 entries (G = 1:
    the row of no entries is a row of level 0), |b| <= 100: |x| <= 100 (1 + 65 * 66) at most, every partial sum below
    2^24 (asserted in Python integers), so x is the integer solution bit for bit.  2 G + 1 empty rows, then 12 and 4
    times as many rows: the mean short row stays in G's interval and lanes_per_row == G."""
    w = 2 * G + 1
    row = np.array([k for k in (G - 1, G, G + 1, 2 * G + 1) if k >= 1])
    lengths = [np.zeros(w, np.int64), np.resize(row, 12 * w), np.resize(row, 4 * w)]
    check_integer_gate(lengths, 40 + G, dtype, G, f"integer gate G{G}")


# ---------------------------------------------------------------- 2. the long-row split
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", ["long wide", "long narrow", "long narrow 32x128", "short wide", "short narrow",
                                  "both wide", "both narrow"])
def test_long_row_split(gpu, name, dtype):
    """Rows of 127 entries (G lanes) and of 128, 129, 191, 192, 193 and 1000 (a wavefront each): a level of long rows
    only (level_split at its start), of short rows only (at its end), of both; each where the level is wide (trsv_level)
    and where it is narrow (trsv_chain).  The level after it is the next of these kinds."""
    plan = check_solves(name, dtype)
    kinds = [k for k, l0, l1 in plan for _ in range(l0, l1)]
    assert kinds[0] == 0 and kinds[1] == (0 if "wide" in name else 1), (name, plan)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_either_side_of_the_long_length_are_exact_on_small_integers(gpu, dtype):
    """the integer gate with rows of 127, 128, 129 and 200 entries in two levels over 256 empty rows:
    |x| <= 100 (1 + 200 * 201), below 2^24"""
    level = rows_of((2, 127), (2, 128), (2, 129), (2, 200), (2, 1))
    check_integer_gate([np.zeros(256, np.int64), level, level[::-1].copy()], 47, dtype, 1, "integer gate long rows")


# ---------------------------------------------------------------- 3. the chain limits on the device
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", ["rows 256 | 257", "entries 4096 | 4097", "narrow narrow wide narrow narrow",
                                  "G32 256 rows chained", "G16 256 rows chained", "chain edges"])
def test_chain_limits(gpu, name, dtype):
    """A level of exactly 256 rows (4096 entries) is chained, its neighbour of 257 rows (4097 entries) is a launch of
    its own; narrow, narrow, wide, narrow, narrow is three launches; 256 rows at G = 32 are 32 passes of the workgroup's
    8 groups inside one chained level; CHAIN_EDGES of test_trsv_host.py holds both limits and a chained level of 32 long
    rows.  launches == len(plan_ref) == len(PLANS[name]), x within the row bound."""
    plan = check_solves(name, dtype)
    if name == "narrow narrow wide narrow narrow":
        assert len(plan) == 3
    if name == "chain edges":
        assert len(plan) == 9 and plan[6] == [1, 6, 7]


# ---------------------------------------------------------------- 4. the grid caps
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", ["cap 17000 rows G32", "cap 530000 rows G1", "cap 8300 long rows"])
def test_levels_past_the_grid_cap(gpu, name, dtype):
    """One level that needs more workgroups than kTrsvBlocks, so trsv_level's stride loop makes a second trip: 17 000
    rows of 32 lanes, 530 000 rows of one lane, 8 300 rows of a wavefront.  The row bound on every row, and two solves
    give the same bytes."""
    rows = len(LENGTHS[name][0][1])
    lanes = 64 if "long" in name else LANES[name]
    assert rows * lanes > K_TRSV_BLOCKS * K_BLOCK
    plan = check_solves(name, dtype, twice=True)
    assert plan[-1][0] == 0


# ---------------------------------------------------------------- 5. SSOR and ILU(0) applies at these widths
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind,omega,ordering", [("ssor", 1.3, "natural"), ("ssor", 1.3, "multicolor"),
                                                 ("ilu0", 1.0, "natural"), ("ilu0", 1.0, "multicolor")])
@pytest.mark.parametrize("name", ["apply G16", "apply G32"])
def test_applies_with_wide_groups_and_long_rows(gpu, name, kind, omega, ordering, dtype):
    """z against long double substitution on the returned factors within tri_apply_bound, on 1200 rows in three levels
    whose triangles pick G = 16 / G = 32 in the natural order and hold rows of 128, 129, 150 and 300 entries: the SCALED
    backward solve, and with the multicolour order the brow / xrow maps, with wide groups and wavefront rows."""
    import scipy.sparse as sps
    M, rp, col, val = built(name)
    val = val.astype(dtype)
    a = canonical(rp, col, val)
    for t in (sps.tril(a, -1).tocsr(), sps.triu(a, 1).tocsr()):
        assert lanes_ref(t) == LANES[name] and np.max(np.diff(t.indptr)) == 300
    r = np.random.default_rng(4).uniform(-1, 1, M).astype(dtype)
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner(kind, omega=omega, ordering=ordering) as P:
        z = P.apply(r)
        Lf, Uf = P.factors()
        tinfo = P.tri_info()
        assert P.apply(r).tobytes() == z.tobytes()
    assert z.dtype == dtype and z.shape == (M,)
    order = order_of(rp, col, val, ordering)
    z_ref, fz, order = tri_apply_bound(Lf, Uf, M, kind, omega, order, r, dtype)
    err = np.abs(z[order].astype(np.longdouble) - z_ref).astype(np.float64)
    lanes = [lanes_ref(side(permuted(scipy_factor(f, M), order), k).tocsr())
             for f, side, k in ((Lf, sps.tril, -1), (Uf, sps.triu, 1))]
    report(f"{name} {kind} {ordering} {np.dtype(dtype)}", lanes_by_the_rule=lanes,
           **{k: tinfo[k] for k in ("forward_levels", "forward_launches", "backward_levels", "backward_launches",
                                    "colours")},
           error_over_bound=f"{np.max(err / fz):.3f}")
    assert np.all(np.isfinite(z)) and np.all(err <= fz), (name, kind, ordering, float(np.max(err / fz)))
    if ordering == "natural":
        assert lanes == [LANES[name]] * 2 and tinfo["forward_levels"] == tinfo["backward_levels"] == 3


# ---------------------------------------------------------------- 6. ILU(0) on wide rows
def assert_ilu0_factors(a, Lf, Uf, dtype, what):
    """natural order: L and U have exactly the pattern of a's lower / upper part, L's diagonal is exactly 1, and
    |(L U - A)_ij| <= (k_i + 2) eps (|L| |U|)_ij on a's pattern (the check of
    test_gpu_trsv.test_ilu0_factors_reproduce_a_on_its_pattern)"""
    import scipy.sparse as sps
    M = a.shape[0]
    Lm, Um = scipy_factor(Lf, M), scipy_factor(Uf, M)
    Lm.sort_indices(), Um.sort_indices()
    lo, up = sps.tril(a, 0, format="csr"), sps.triu(a, 0, format="csr")
    assert np.array_equal(Lm.indptr, lo.indptr) and np.array_equal(Lm.indices, lo.indices), what
    assert np.array_equal(Um.indptr, up.indptr) and np.array_equal(Um.indices, up.indices), what
    assert np.all(Lm.diagonal() == 1.0) and Lf[2].dtype == dtype and Uf[2].dtype == dtype
    lu, alu = (Lm @ Um).tocsr(), (abs(Lm) @ abs(Um)).tocsr()
    rows = np.repeat(np.arange(M), np.diff(a.indptr))
    diff = np.abs(np.asarray(lu[rows, a.indices]).ravel() - a.data)
    bound = (np.diff(a.indptr)[rows] + 2) * np.finfo(dtype).eps * np.asarray(alu[rows, a.indices]).ravel()
    print(f"{what}: max (LU - A) / bound = {np.max(diff / bound):.3f}")
    assert np.all(np.isfinite(Lf[2])) and np.all(np.isfinite(Uf[2])), what
    assert np.all(diff <= bound), (what, float(np.max(diff / bound)))


def integer_blocks(s, blocks, seed, signs, zero_pivots=()):
    """(L0, U0, A) as (blocks, s, s) fp64 arrays of integers, A = L0 U0 per block.  L0 is unit lower, U0 upper, their
    off-diagonal entries in {-1, 1}, U0's diagonal in {+-2, +-4} (0 at place 70 of the blocks in zero_pivots).
    signs "row-column": L0 = S E S and U0 = S F V with S, V random sign diagonals and E, F the triangles of ones, so
    A = S (E F) V has the entries +-(i + 1) above and +-(j + d_j) on and below the diagonal: no zero, as asserted.
    signs "free": every sign is drawn on its own; A then has zeros, which are stored like every other position.
    Either way every Schur complement entry is a partial sum of sum_m l_im u_mj, at most s + 3 in size, and
    w_ik / u_kk = l_ik exactly (u_kk a power of two): the factorisation is exact in fp64 and in fp32's 2^24."""
    rng = np.random.default_rng(seed)
    d = rng.choice([2.0, 4.0], (blocks, s))
    for blk in zero_pivots:
        d[blk, 70] = 0.0
    eye = np.eye(s)
    if signs == "row-column":
        sg, v = rng.choice([-1.0, 1.0], (blocks, s)), rng.choice([-1.0, 1.0], (blocks, s))
        L0 = sg[:, :, None] * np.tril(np.ones((s, s)))[None] * sg[:, None, :]
        U0 = sg[:, :, None] * (np.triu(np.ones((s, s)), 1)[None] + eye[None] * d[:, None, :]) * v[:, None, :]
    else:
        L0 = np.tril(rng.choice([-1.0, 1.0], (blocks, s, s)), -1) + eye[None]
        U0 = (np.triu(rng.choice([-1.0, 1.0], (blocks, s, s)), 1)
              + eye[None] * (d * rng.choice([-1.0, 1.0], (blocks, s)))[:, None, :])
    A = L0 @ U0
    assert int(np.max(np.abs(L0) @ np.abs(U0))) < 2 ** 24 and np.all(A == np.rint(A))
    assert signs == "free" or np.all(A != 0.0)
    return L0, U0, A


def block_csr(A, mask):
    """CSR of the block-diagonal matrix with the positions of mask (s x s, bool) stored in every block, zeros too"""
    blocks, s, _ = A.shape
    r, c = np.nonzero(mask)
    per_row = np.bincount(r, minlength=s)
    rp = np.concatenate([[0], np.cumsum(np.tile(per_row, blocks))]).astype(np.int32)
    col = (c[None, :] + s * np.arange(blocks)[:, None]).ravel().astype(np.int32)
    return rp, col, np.ascontiguousarray(A[:, mask].ravel())


BLOCK_SHAPES = [(1, 3), (2, 3), (63, 3), (64, 3), (65, 3), (66, 3), (129, 3), (200, 3), (66, 300), (3, 8300)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("signs", ["row-column", "free"])
@pytest.mark.parametrize("s,blocks", BLOCK_SHAPES, ids=[f"{s}x{b}" for s, b in BLOCK_SHAPES])
def test_ilu0_of_dense_integer_blocks_is_their_lu_bit_for_bit(gpu, s, blocks, signs, dtype):
    """On a block-diagonal matrix with every block position stored ILU(0) is LU, and on integer_blocks() every step of
    it is exact: factors() equals (L0, U0) byte for byte.  Three blocks: the levels are narrow, one ilu0_chain launch;
    rows of up to 199 pivots and 199 entries right of a pivot (the lanes' f += 64 loop makes up to four trips).
    300 blocks of 66: every level has 300 rows, ilu0_level.  8 300 blocks of 3: past ilu0_level's grid cap of
    2048 x 4 rows."""
    import scipy.sparse as sps
    L0, U0, A = integer_blocks(s, blocks, 1000 + s, signs)
    full = np.ones((s, s), bool)
    n = s * blocks
    rp, col, val = block_csr(A, full)
    srp, scol, sval = block_csr(A, np.tril(full, -1))
    strict = sps.csr_matrix((sval, scol, srp), shape=(n, n))
    plan = plan_ref(strict, np.tile(np.arange(1, s + 1), blocks))
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev, dev.preconditioner("ilu0", ordering="natural") as P:
        Lf, Uf = P.factors()
        tinfo = P.tri_info()
    report(f"ilu0 blocks {s} x {blocks} {signs} {np.dtype(dtype)}", forward_levels=tinfo["forward_levels"],
           forward_launches=tinfo["forward_launches"], kernels="".join("c" if k[0] else "l" for k in plan))
    assert tinfo["forward_levels"] == s and tinfo["forward_launches"] == len(plan), (tinfo, plan)
    if blocks == 3:
        assert plan == [[1, 0, s]] and tinfo["forward_launches"] == 1
    else:
        assert all(k == 0 for k, _, _ in plan) and blocks > (K_BLOCK if s == 66 else K_TRSV_BLOCKS * K_BLOCK // 64)
    for (frp, fcol, fval), F, mask in ((Lf, L0, np.tril(full)), (Uf, U0, np.triu(full))):
        erp, ecol, evals = block_csr(F, mask)
        assert np.array_equal(frp, erp) and np.array_equal(fcol, ecol)
        assert fval.dtype == dtype and fval.tobytes() == evals.astype(dtype).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("blocks,zero_pivots", [(3, (2,)), (3, (1, 2)), (300, (250, 40))])
def test_ilu0_refuses_a_zero_pivot_inside_a_wide_row(gpu, blocks, zero_pivots, dtype):
    """Dense integer blocks of 130 with U0's diagonal zero at place 70 of some blocks (A itself has no zero entry): the
    factorisation is exact, the pivot of that row is exactly 0, and the build is refused naming the lowest such global
    row, under ilu0_chain (3 blocks) and ilu0_level (300 blocks).  The handle multiplies afterwards, exactly: integer x,
    |x| <= 8, row sums below 2^24."""
    s = 130
    L0, U0, A = integer_blocks(s, blocks, 77, "row-column", zero_pivots)
    n, row = s * blocks, s * min(zero_pivots) + 70
    rp, col, val = block_csr(A, np.ones((s, s), bool))
    x = np.random.default_rng(3).integers(-8, 9, n).astype(np.float64)
    y_ref = (A @ x.reshape(blocks, s, 1)).ravel()
    assert np.max(np.abs(A).sum(axis=2)) * 8 < 2 ** 24
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev:
        with pytest.raises(sp.SpmvHipError, match=rf"row {row} \(global row {row}\).*pivot"):
            dev.preconditioner("ilu0", ordering="natural")
        y = dev.spmv(x.astype(dtype))
        assert np.array_equal(y.astype(np.float64), y_ref)
        with dev.preconditioner("ssor") as P:            # a build that does not factor still works
            assert P.tri_info()["forward_levels"] == s


def wide_band(dtype):
    """nonsym_banded with 200 draws per row over a band of +-150 (about 140 distinct entries per row, n = 1500),
    diagonal 1.1 x the row's absolute sum + 1; values rounded to dtype"""
    rp, col, val = nonsym_banded(np.random.default_rng(61), 1500, 200, 150, 1.1)
    return rp, col, val.astype(dtype)


def shuffled_and_split(rp, col, val, rng):
    """the same matrix with every row's entries in random order and a fifth of them split into two or three entries of
    the same (row, column): v / 2, v / 2 or v / 2, v / 4, v / 4, whose sum is v exactly in any order"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    pieces = rng.choice([1, 2, 3], len(col), p=[0.8, 0.1, 0.1])
    r2, c2 = np.repeat(rows, pieces), np.repeat(col, pieces)
    first = np.concatenate([[0], np.cumsum(pieces)[:-1]])
    j = np.arange(len(r2)) - np.repeat(first, pieces)
    np2 = np.repeat(pieces, pieces)
    factor = np.where(np2 == 1, 1.0, np.where(j == 0, 0.5, np.where(np2 == 2, 0.5, 0.25)))
    v2 = (np.repeat(val, pieces) * factor).astype(val.dtype)
    order = np.lexsort((rng.random(len(r2)), r2))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=len(rp) - 1))]).astype(np.int32)
    return rp2, c2[order].astype(np.int32), np.ascontiguousarray(v2[order])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ilu0_of_a_wide_band(gpu, dtype):
    """About 140 entries per row, about 70 pivots per row, pivot rows whose entries are often missing from row i (the
    bisection misses): pattern equality and the (k_i + 2) eps bound on the returned factors, and the same bytes from the
    same matrix uploaded with shuffled rows and entries split into repeated (row, column) pairs."""
    rp, col, val = wide_band(dtype)
    M = len(rp) - 1
    a = canonical(rp, col, val)
    per_row = np.diff(a.indptr)
    assert 130 <= per_row.mean() <= 160 and per_row.max() > 2 * 64
    rp2, col2, val2 = shuffled_and_split(rp, col, val, np.random.default_rng(62))
    a2 = canonical(rp2, col2, val2)
    assert len(col2) > 1.25 * len(col)
    assert np.array_equal(a2.indices, a.indices) and a2.data.tobytes() == a.data.tobytes()
    got = []
    for r, c, v in ((rp, col, val), (rp2, col2, val2)):
        with sp.CsrDevice(M, M, r, c, v) as dev, dev.preconditioner("ilu0", ordering="natural") as P:
            got.append(P.factors())
            tinfo = P.tri_info()
    report(f"ilu0 wide band {np.dtype(dtype)}", entries_per_row=f"{per_row.mean():.1f}",
           **{k: tinfo[k] for k in ("forward_levels", "forward_launches", "entries_l", "entries_u")})
    assert_ilu0_factors(a, *got[0], dtype, f"wide band {np.dtype(dtype)}")
    assert tinfo["entries_l"] + tinfo["entries_u"] == a.nnz + M
    for f, g in zip(got[0], got[1]):
        assert all(u.tobytes() == w.tobytes() for u, w in zip(f, g))
