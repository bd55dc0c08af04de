"""Preconditioner.refresh and TriangularSolver.refresh: new values, the symbolic work kept.

For each kind that can be refreshed -- jacobi, block_jacobi (block 3), ssor (omega 1.2), ilu0 in the natural and in the
multicolour order -- and both dtypes: P is built on values A, the handle is updated to B, P.refresh(handle), and P is held
to a P built afresh on an upload of B, byte for byte: factors() where the kind has them, apply(r) for a uniform and a
wide-range r, info() / tri_info() without the microsecond fields, five solver steps with it.  Then back to A through a
second refresh, which runs on the maps the first one built.

The matrices are the smallest that reach each launch kind of spmv_trsv.hip: a 40 x 40 convection-diffusion grid in natural
order (every level narrow: the chain kernels), a 64 x 64 grid in the multicolour order (two levels of 2048 rows: the level
kernels), an arrow matrix of 300 rows with a dense last row and column (a row beyond the 128-entry wavefront threshold),
the symmetric positive definite fem-like target of test_gpu_adopted_handles.py, the grid with its rows shuffled and a tenth
of its entries split into two repeats, and a row-range handle of the grid, which keeps its diagonal block only.

The refusals: values with a zero pivot in row 17 (the message's words are those of a build on the same values, and P
still applies as before), a handle of another pattern, a handle of the other dtype, the kinds that depend on the values
(fsai, amg, chebyshev), and a refresh that works after a refused one."""
import re

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import wide_range
from test_gpu_adopted_handles import same_results, spd_target

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = {
    "jacobi": dict(kind="jacobi"),
    "block_jacobi": dict(kind="block_jacobi", block=3),
    "ssor": dict(kind="ssor", omega=1.2),
    "ilu0": dict(kind="ilu0"),
    "ilu0-multicolor": dict(kind="ilu0", ordering="multicolor"),
}
TRI = ("ssor", "ilu0", "ilu0-multicolor")


# ---------------------------------------------------------------- matrices: (M, rp, col), square, every diagonal stored
def grid(nx, ny):
    """the 5-point stencil's pattern on an nx x ny grid, rows ascending"""
    idx = np.arange(nx * ny).reshape(ny, nx)
    rows, cols = [idx.ravel()], [idx.ravel()]
    for a, b in ((idx[:, 1:], idx[:, :-1]), (idx[1:, :], idx[:-1, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
    return from_coo(nx * ny, np.concatenate(rows), np.concatenate(cols))


def from_coo(M, rows, cols):
    order = np.lexsort((cols, rows))
    rp = np.zeros(M + 1, dtype=np.int64)
    np.add.at(rp, rows + 1, 1)
    return M, np.cumsum(rp).astype(np.int32), cols[order].astype(np.int32)


def arrow(n):
    """a diagonal with a dense last row and column"""
    k = np.arange(n - 1)
    last = np.full(n - 1, n - 1)
    return from_coo(n, np.concatenate([np.arange(n), k, last]), np.concatenate([np.arange(n), last, k]))


def shuffled_with_repeats(M, rp, col, seed=3):
    """a tenth of the entries stored twice (their value is then the sum of two stored halves), every row's entries in a
    random order"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M), np.diff(rp))
    twice = rng.random(len(col)) < 0.1
    rows, cols = np.concatenate([rows, rows[twice]]), np.concatenate([col, col[twice]])
    order = np.lexsort((rng.random(len(cols)), rows))
    out = np.zeros(M + 1, dtype=np.int64)
    np.add.at(out, rows + 1, 1)
    return M, np.cumsum(out).astype(np.int32), cols[order].astype(np.int32)


def spd_pattern():
    M, _, rp, col, _ = spd_target(np.float64)
    return M, rp, col


def values(M, rp, col, seed, dtype, symmetric=False):
    """a draw on the pattern with a diagonal that dominates its row (convection-diffusion like: the two sides of the
    diagonal differ unless symmetric)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M), np.diff(rp))
    if symmetric:
        lo, hi = np.minimum(rows, col).astype(np.int64), np.maximum(rows, col).astype(np.int64)
        val = -np.abs(np.sin((lo * 7919 + hi * 104729 + seed) * 0.37)) - 0.05
    else:
        val = rng.uniform(-1, 1, len(col)) - 0.3 * (col > rows)
    diag = rows == col
    val[diag] = 0.0
    sums = np.zeros(M)
    np.add.at(sums, rows, np.abs(val))
    val[diag] = (sums[rows[diag]] + 1.0 + (0.0 if symmetric else 1.0) * rng.random(int(diag.sum()))) / np.maximum(
        np.bincount(rows[diag], minlength=M)[rows[diag]], 1)
    return val.astype(dtype)


MATRICES = {
    "grid 40x40": lambda: grid(40, 40),
    "grid 64x64": lambda: grid(64, 64),
    "arrow 300": lambda: arrow(300),
    "fem-like spd": spd_pattern,
    "grid 40x40, shuffled, repeats": lambda: shuffled_with_repeats(*grid(40, 40)),
}
_PATTERNS = {}


def pattern(name):
    if name not in _PATTERNS:
        _PATTERNS[name] = MATRICES[name]()
    return _PATTERNS[name]


# ---------------------------------------------------------------- what is compared
def without_times(info):
    return {k: v for k, v in info.items() if not k.endswith("_us")}


def seen(P, name, dev=None, solver=None, b=None):
    """everything a refreshed P and a freshly built one are compared by"""
    rng = np.random.default_rng(17)
    out = {"info": without_times(P.info())}
    if name in TRI:
        out["tri_info"] = without_times(P.tri_info())
        out["factors"] = P.factors()
    for k, r in enumerate((rng.uniform(-1, 1, P.rows).astype(P.dtype), wide_range(rng, P.rows, P.dtype))):
        out[f"apply {k}"] = P.apply(r)
    if solver == "pcg":
        out["pcg"] = dev.pcg(b, 5, precond=P)[:4]
    elif solver == "bicgstab":
        out["bicgstab"] = dev.bicgstab(b, 5, precond=P)[:3]
    return out


CASES = [(m, k) for m in MATRICES for k in KINDS]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("matrix,name", CASES)
def test_refreshed_preconditioner_is_the_fresh_build(gpu, matrix, name, dtype):
    M, rp, col = pattern(matrix)
    spd = matrix == "fem-like spd"
    A, B = values(M, rp, col, 1, dtype, spd), values(M, rp, col, 2, dtype, spd)
    b = np.random.default_rng(23).uniform(-1, 1, M).astype(dtype)
    solver = "pcg" if spd else "bicgstab"
    what = f"{matrix} {name} {np.dtype(dtype).name}"
    with sp.CsrDevice(M, M, rp, col, A) as dev, sp.CsrDevice(M, M, rp, col, B) as at_b, sp.CsrDevice(M, M, rp, col, A) as at_a:
        with dev.preconditioner(**KINDS[name]) as P:
            if name == "ilu0-multicolor" and matrix == "grid 64x64":
                assert P.tri_info()["forward_widest"] == 2048 and P.tri_info()["colours"] == 2, P.tri_info()
            if name == "ilu0" and matrix == "grid 40x40":
                assert P.tri_info()["forward_levels"] == 79 > P.tri_info()["forward_launches"], P.tri_info()
            dev.update_values(B)
            P.refresh(dev)
            with at_b.preconditioner(**KINDS[name]) as Q:
                same_results(seen(P, name, dev, solver, b), seen(Q, name, at_b, solver, b), what + ", A -> B")
            dev.update_values(A)
            P.refresh(dev)                                         # on the first refresh's maps
            with at_a.preconditioner(**KINDS[name]) as Q:
                same_results(seen(P, name, dev, solver, b), seen(Q, name, at_a, solver, b), what + ", back to A")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(KINDS))
def test_refresh_on_a_row_range_handle(gpu, name, dtype):
    """rows [r0, r1) of the grid: P covers the diagonal block only, entries in other columns feed nothing"""
    M, rp, col = pattern("grid 40x40")
    A, B = values(M, rp, col, 1, dtype), values(M, rp, col, 2, dtype)
    r0, r1 = 403, 1208
    e0, e1 = int(rp[r0]), int(rp[r1])
    with sp.CsrDevice(M, M, rp, col, A, r0, r1) as dev, sp.CsrDevice(M, M, rp, col, B, r0, r1) as at_b:
        with dev.preconditioner(**KINDS[name]) as P:
            assert P.rows == r1 - r0 and P.row0 == r0
            dev.update_values(B[e0:e1])
            P.refresh(dev)
            with at_b.preconditioner(**KINDS[name]) as Q:
                same_results(seen(P, name), seen(Q, name), f"rows [{r0}, {r1}) {name} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("matrix", ["grid 40x40, shuffled, repeats", "grid 64x64", "arrow 300"])
def test_refreshed_triangular_solver_is_the_fresh_build(gpu, matrix, unit, lower, dtype):
    M, rp, col = pattern(matrix)
    A, B = values(M, rp, col, 1, dtype), values(M, rp, col, 2, dtype)
    b = wide_range(np.random.default_rng(29), M, dtype)
    with sp.CsrDevice(M, M, rp, col, A) as dev, sp.CsrDevice(M, M, rp, col, B) as at_b, sp.CsrDevice(M, M, rp, col, A) as at_a:
        with dev.triangular(lower=lower, unit_diagonal=unit) as S:
            for new, twin in ((B, at_b), (A, at_a)):               # (the second refresh: on the first one's maps)
                dev.update_values(new)
                S.refresh(dev)
                with twin.triangular(lower=lower, unit_diagonal=unit) as fresh:
                    assert without_times(S.info()) == without_times(fresh.info())
                    assert S.solve(b).tobytes() == fresh.solve(b).tobytes(), (matrix, unit, lower, np.dtype(dtype).name)
            # a zero diagonal in row 17: refused in the build's words unless the diagonal is not read; S as it was
            before = S.solve(b)
            bad = B.copy()
            bad[(np.repeat(np.arange(M), np.diff(rp)) == 17) & (col == 17)] = 0
            dev.update_values(bad)
            if unit:
                S.refresh(dev)
            else:
                with pytest.raises(sp.SpmvHipError) as refresh_error:
                    S.refresh(dev)
                with pytest.raises(sp.SpmvHipError) as build_error:
                    dev.triangular(lower=lower, unit_diagonal=unit)
                assert words(refresh_error.value) == words(build_error.value) and "row 17 " in words(build_error.value)
                assert S.solve(b).tobytes() == before.tobytes()
                dev.update_values(B)
                S.refresh(dev)                                     # a refresh after a refused one


@pytest.mark.parametrize("lower", [True, False])
def test_triangular_solver_keeps_its_pattern_check_behind_a_refused_first_refresh(gpu, lower):
    M, rp, col = pattern("grid 40x40, shuffled, repeats")
    A = values(M, rp, col, 1, np.float64)
    b = wide_range(np.random.default_rng(29), M, np.float64)
    bad = A.copy()
    bad[(np.repeat(np.arange(M), np.diff(rp)) == 17) & (col == 17)] = 0
    M2, rp2, col2 = grid(32, 50)
    with sp.CsrDevice(M, M, rp, col, A) as dev, sp.CsrDevice(M2, M2, rp2, col2, values(M2, rp2, col2, 1, np.float64)) as other:
        with dev.triangular(lower=lower) as S:
            before = S.solve(b)
            dev.update_values(bad)
            with pytest.raises(sp.SpmvHipError, match="trsv_refresh: row 17 "):
                S.refresh(dev)
            with pytest.raises(sp.SpmvHipError, match="pattern"):
                S.refresh(other)
            assert S.solve(b).tobytes() == before.tobytes()
            dev.update_values(A)
            S.refresh(dev)
            assert S.solve(b).tobytes() == before.tobytes()


def words(error):
    """a refusal from its row (or block) on: what a build and a refresh share, behind the entry points' names"""
    return re.search(r"(row|block) \d+.*", str(error), flags=re.S).group(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(KINDS))
def test_refused_refresh_leaves_the_preconditioner_as_it_was(gpu, name, dtype):
    M, rp, col = pattern("grid 40x40, shuffled, repeats")
    A, B = values(M, rp, col, 1, dtype), values(M, rp, col, 2, dtype)
    rows = np.repeat(np.arange(M), np.diff(rp))
    bad = B.copy()
    bad[rows == 17] = 0                                            # row 17 of zeros: a zero diagonal, a zero pivot
    other_dtype = np.float32 if dtype == np.float64 else np.float64
    M2, rp2, col2 = grid(32, 50)                                   # the same shape, another pattern
    col_moved = col.copy()                                         # row 100's entries in column 140 moved to column 141
    row100 = col_moved[rp[100]:rp[101]]
    assert np.any(row100 == 140) and not np.any(row100 == 141)
    row100[row100 == 140] = 141
    with sp.CsrDevice(M, M, rp, col, A) as dev, sp.CsrDevice(M, M, rp, col, B) as at_b:
        with dev.preconditioner(**KINDS[name]) as P:
            at_a = seen(P, name)
            # a first refresh that is refused
            dev.update_values(bad)
            with pytest.raises(sp.SpmvHipError) as refresh_error:
                P.refresh(dev)
            with pytest.raises(sp.SpmvHipError) as build_error:
                dev.preconditioner(**KINDS[name])
            assert words(refresh_error.value) == words(build_error.value), (str(refresh_error.value), str(build_error.value))
            assert ("block 5 " if name == "block_jacobi" else "row 17 ") in words(build_error.value), str(build_error.value)
            same_results(seen(P, name), at_a, f"{name}: after the refused refresh")
            # ... and a refresh that works after it
            dev.update_values(B)
            P.refresh(dev)
            with at_b.preconditioner(**KINDS[name]) as Q:
                want = seen(Q, name)
            same_results(seen(P, name), want, f"{name}: a refresh after a refused one")
            # a refused refresh on the maps
            dev.update_values(bad)
            with pytest.raises(sp.SpmvHipError) as again:
                P.refresh(dev)
            assert words(again.value) == words(build_error.value)
            same_results(seen(P, name), want, f"{name}: after the second refused refresh")
            # another pattern, the other dtype
            with sp.CsrDevice(M2, M2, rp2, col2, values(M2, rp2, col2, 1, dtype)) as other:
                with pytest.raises(sp.SpmvHipError, match="pattern"):
                    P.refresh(other)
            # ... with the same rows and the same number of entries, one column moved: only the digest can tell
            with sp.CsrDevice(M, M, rp, col_moved, B) as other:
                assert other.info()["nz"] == dev.info()["nz"]
                with pytest.raises(sp.SpmvHipError, match="pattern"):
                    P.refresh(other)
            with sp.CsrDevice(M, M, rp, col, B.astype(other_dtype)) as other:
                with pytest.raises(sp.SpmvHipError, match="byte values"):
                    P.refresh(other)
            with sp.CsrDevice(M, M, rp, col, B, 0, M - 5) as other:
                with pytest.raises(sp.SpmvHipError, match="rows"):
                    P.refresh(other)
            same_results(seen(P, name), want, f"{name}: after the refusals")
        if name in TRI:
            # a FIRST refresh from a handle of another pattern: held to the triangles P stores
            dev.update_values(A)
            with dev.preconditioner(**KINDS[name]) as P:
                with sp.CsrDevice(M2, M2, rp2, col2, values(M2, rp2, col2, 1, dtype)) as other:
                    with pytest.raises(sp.SpmvHipError, match="pattern"):
                        P.refresh(other)
                dev.update_values(B)
                P.refresh(dev)
                same_results(seen(P, name), want, f"{name}: a first refresh after one from another pattern")
            # A first refresh that the NUMBERS refuse has made its maps: the pattern check must outlive the refusal.  A
            # handle of another pattern -- fewer entries, or as many -- is then refused, not gathered from.
            dev.update_values(A)
            with dev.preconditioner(**KINDS[name]) as P:
                dev.update_values(bad)
                with pytest.raises(sp.SpmvHipError, match="row 17 "):
                    P.refresh(dev)
                for cols2, what in (((M2, rp2, col2), "fewer entries"), ((M, rp, col_moved), "as many entries")):
                    Mo, rpo, colo = cols2
                    with sp.CsrDevice(Mo, Mo, rpo, colo, values(Mo, rpo, colo, 1, dtype)) as other:
                        with pytest.raises(sp.SpmvHipError, match="pattern"):
                            P.refresh(other)
                same_results(seen(P, name), at_a, f"{name}: after a refused first refresh and two foreign patterns")
                dev.update_values(B)
                P.refresh(dev)
                same_results(seen(P, name), want, f"{name}: a refresh after all of them")


@pytest.mark.parametrize("kind", ["fsai", "amg", "chebyshev"])
def test_kinds_that_depend_on_the_values_are_refused(gpu, kind):
    tgt = spd_target(np.float64)
    r = np.random.default_rng(3).uniform(-1, 1, tgt[0])
    with sp.CsrDevice(*tgt) as dev:
        with dev.preconditioner(kind) as P:
            before = P.apply(r)
            with pytest.raises(sp.SpmvHipError, match="depends on the values.*[Bb]uild it again"):
                P.refresh(dev)
            assert P.apply(r).tobytes() == before.tobytes()
