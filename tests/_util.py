"""Shared helpers for the parity tests."""
import hashlib
import json
import os

import numpy as np

# BASELINE.json north_star: "within 1e-10 relative error (fp64)" against the
# reference's serial CSR result.  A re-ordered summation (lane-strided partial
# sums + butterfly, and FMA contraction on the GPU) cannot reproduce the serial
# left-to-right sum bit for bit, and for rows whose exact sum cancels to ~0
# (Laplacians / KKT blocks with x = 1) an element-wise relative error is
# unbounded, so the gate is ("Tolerance vs summation order"):
#   norm-wise:  max|y - y_ref| <= 1e-10 * max|y_ref|
#   row-wise:   |y_i - y_ref_i| <= 1e-10 * sum_j |a_ij x_j|
FP64_RTOL = 1e-10
FP32_NORMWISE_RTOL = 1e-5  # config 5 (fp32 data) against the fp64-accumulated oracle


def row_abs_sums(row_ptr, col_idx, values, x):
    p = np.abs(values * x[col_idx])
    out = np.zeros(len(row_ptr) - 1)
    nonempty = np.flatnonzero(np.diff(row_ptr) > 0)
    if len(nonempty):
        out[nonempty] = np.add.reduceat(p, row_ptr[nonempty])
    return out


def assert_parity(y, y_ref, row_ptr, col_idx, values, x, rtol=FP64_RTOL, what=""):
    y = np.asarray(y, dtype=np.float64)
    y_ref = np.asarray(y_ref, dtype=np.float64)
    assert y.shape == y_ref.shape, f"{what}: shape {y.shape} vs {y_ref.shape}"
    if y.size == 0:
        return
    assert np.all(np.isfinite(y)), f"{what}: non-finite result"
    d = np.abs(y - y_ref)
    scale = np.max(np.abs(y_ref))
    assert d.max() <= rtol * scale + 0.0 or scale == 0 and d.max() == 0, \
        f"{what}: norm-wise {d.max() / max(scale, 1e-300):.3e} > {rtol}"
    bound = rtol * row_abs_sums(np.asarray(row_ptr), np.asarray(col_idx),
                                np.asarray(values, dtype=np.float64),
                                np.asarray(x, dtype=np.float64))
    bad = np.flatnonzero(d > bound)
    assert bad.size == 0, (f"{what}: {bad.size} rows beyond {rtol} * sum|a_ij x_j|; first row "
                           f"{bad[0]}: |d| = {d[bad[0]]:.3e}, bound = {bound[bad[0]]:.3e}")


def random_csr(rng, M, N, mean_row, max_row=None, empty_frac=0.0, dtype=np.float64):
    """Random CSR with sorted, distinct columns per row."""
    max_row = min(N, max_row or max(1, 4 * mean_row))
    lens = np.minimum(rng.poisson(mean_row, M), max_row).astype(np.int64)
    lens[rng.random(M) < empty_frac] = 0
    row_ptr = np.zeros(M + 1, dtype=np.int32)
    np.cumsum(lens, out=row_ptr[1:])
    col = np.empty(row_ptr[-1], dtype=np.int32)
    for r in range(M):
        if lens[r]:
            col[row_ptr[r]:row_ptr[r + 1]] = np.sort(rng.choice(N, lens[r], replace=False))
    val = rng.uniform(-1, 1, row_ptr[-1]).astype(dtype)
    return row_ptr, col, val


def coo_from_csr(row_ptr, col, val, rng=None):
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int32), np.diff(row_ptr))
    if rng is not None:
        order = rng.permutation(len(rows))
        return rows[order], col[order], val[order]
    return rows, col, val


def banded_csr(rng, M, N, mean_row, band, empty_frac=0.0, dtype=np.float64, far_frac=0.0):
    """Random CSR whose columns stay within `band` of the diagonal (plus, for far_frac of the
    rows, one cluster far away), sorted and distinct per row: few x lines per row block."""
    lens = np.minimum(rng.poisson(mean_row, M), min(N, 2 * band)).astype(np.int64)
    lens[rng.random(M) < empty_frac] = 0
    row_ptr = np.zeros(M + 1, dtype=np.int32)
    np.cumsum(lens, out=row_ptr[1:])
    col = np.empty(row_ptr[-1], dtype=np.int32)
    for r in range(M):
        n = lens[r]
        if not n:
            continue
        centre = int(r * (N - 1) / max(M - 1, 1))
        lo = max(0, min(centre - band, N - 2 * band))
        cand = np.arange(lo, min(N, lo + 2 * band))
        c = rng.choice(cand, n, replace=False)
        if far_frac and rng.random() < far_frac:
            k = max(1, n // 4)
            c[:k] = (c[:k] + N // 2) % N
            c = np.unique(c)
            c = np.concatenate([c, rng.choice(np.setdiff1d(cand, c), n - len(c), replace=False)]) if len(c) < n else c
        col[row_ptr[r]:row_ptr[r + 1]] = np.sort(c)
    val = rng.uniform(-1, 1, row_ptr[-1]).astype(dtype)
    return row_ptr, col, val


# ---- the inputs of the checks against the reference's own code.  tests/golden/make_golden.py runs
# the compiled reference on exactly these inputs and stores what it computed in REFERENCE_DIGESTS
# (SHA-256 of each output array's bytes, scalars as they are), so the tests need no reference tree.
REFERENCE_DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")


def digest(a):
    """SHA-256 of an array's bytes: equal digests <=> bit-identical arrays."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def reference_digests(section):
    with open(REFERENCE_DIGESTS) as f:
        return json.load(f)[section]


def random_mtx_trials(directory):
    """Seeded random matrices written as .mtx (some symmetric, entries in shuffled order, empty
    rows) with one x each: yields (trial, path, M, N, x)."""
    rng = np.random.default_rng(11)
    for trial, (M, N, mean, sym) in enumerate([(150, 150, 6, True), (333, 211, 11, False),
                                               (64, 64, 2, True), (1000, 1000, 27, False)]):
        row_ptr, col, val = random_csr(rng, M, N, mean, empty_frac=0.1)
        r, c, v = coo_from_csr(row_ptr, col, val, rng)
        if sym:
            keep = c <= r
            r, c, v = r[keep], c[keep], v[keep]
        path = os.path.join(str(directory), f"m{trial}.mtx")
        with open(path, "w") as f:
            f.write(f"%%MatrixMarket matrix coordinate real {'symmetric' if sym else 'general'}\n")
            f.write(f"{M} {N} {len(r)}\n")
            for k in range(len(r)):
                f.write(f"{r[k] + 1} {c[k] + 1} {float(v[k])!r}\n")
        yield trial, path, M, N, rng.uniform(-1, 1, N)


def sort_row_inputs():
    """Seeded rows for sort_row, many repeated keys: yields (n, cols, vals)."""
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 64, 500, 12000):
        for _ in range(4):
            cols = rng.integers(0, max(2, n // 3), n).astype(np.int32)
            vals = rng.uniform(-1, 1, n)
            yield n, cols, vals


def difference_metrics_inputs():
    """A seeded result vector and a perturbed copy, differences over eleven decades."""
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, 5000)
    b = a + rng.uniform(-1, 1, 5000) * 10.0 ** rng.integers(-12, -1, 5000)
    return a, b


def write_free_form_mtx(path, M, N, rows, cols, vals, field, symmetry, ragged=False):
    """Write a .mtx; ragged: legal free-form layout (tabs, blank lines, two entries on one line,
    an entry split over lines)."""
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate {field} {symmetry}\n% big file for the parallel parser\n")
        f.write(f"{M} {N} {len(rows)}\n")
        lines = []
        for k in range(len(rows)):
            if field == "pattern":
                lines.append(f"{rows[k] + 1} {cols[k] + 1}")
            else:
                lines.append(f"{rows[k] + 1} {cols[k] + 1} {float(vals[k])!r}")
        if ragged:
            out = []
            for k, ln in enumerate(lines):
                sel = k % 7
                if sel == 0:
                    out.append(ln.replace(" ", "\t") + "\n\n")
                elif sel == 1:
                    out.append(ln + "   ")       # next entry continues on the same line
                elif sel == 2:
                    out.append(ln.replace(" ", "\n", 1) + "\n")
                else:
                    out.append("  " + ln + " \r\n")
            f.write("".join(out))
        else:
            f.write("\n".join(lines) + "\n")


PARSER_CASES = [("real", "symmetric", False), ("pattern", "general", False), ("real", "general", True)]


def write_parser_case(path, field, symmetry, ragged):
    """A seeded file over 1 MiB (large enough for the parallel parser): 150 000 entries with
    values over forty decades."""
    rng = np.random.default_rng(42)
    M, N, nnz = 50000, 60000 if symmetry == "general" else 50000, 150000
    rows = rng.integers(0, M, nnz)
    cols = rng.integers(0, N, nnz)
    if symmetry == "symmetric":
        rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    vals = rng.uniform(-1, 1, nnz) * 10.0 ** rng.integers(-20, 20, nnz)
    write_free_form_mtx(path, M, N, rows, cols, vals, field, symmetry, ragged)


def parser_case_key(field, symmetry, ragged):
    return f"{field}-{symmetry}{'-ragged' if ragged else ''}"
