"""Shared helpers for the parity tests."""
import collections
import hashlib
import json
import os
import re
import shutil
import subprocess
import tempfile

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


# ---- the exact fp32 row gate.  fp32 x fp32 products are exact in fp64, so the oracle (csr_f32_accum64) is the exact
# row sum up to its own fp64 summation error.  A kernel's fp32 result -- any summation tree, with or without FMA,
# partial sums added later -- holds the standard order-independent bound (Higham, Accuracy and Stability of Numerical
# Algorithms, 2nd ed., section 4.2):
#   |y_i - ref_i| <= (gamma32(n_i) + gamma64(n_i)) * sum_j |a_ij x_j|,  gamma(n) = n u / (1 - n u)
# with n_i the entries of row i, u32 = 2^-24, u64 = 2^-53.  Rigorous while no product underflows and nothing
# overflows; the helper asserts that of its inputs.  An empty row (or one whose products are all 0) must be exactly 0.
U32, U64 = 2.0 ** -24, 2.0 ** -53
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)   # 2^-126
F32_MAX = float(np.finfo(np.float32).max)


def gamma(n, u):
    n = np.asarray(n, dtype=np.float64)
    return n * u / (1.0 - n * u)


def f32_row_bound(row_ptr, col_idx, values, x):
    """Per-row bound of the fp32 gate (the inputs checked: finite, no subnormal fp32 product, no overflow)."""
    values = np.asarray(values)
    x = np.asarray(x)
    assert values.dtype == np.float32 and x.dtype == np.float32, "the fp32 gate takes fp32 data"
    assert np.all(np.isfinite(values)) and np.all(np.isfinite(x)), "fp32 gate: non-finite input"
    from oracle.oracle import Oracle
    sums, smallest = _oracle(Oracle).f32_row_abs_sums(row_ptr, col_idx, values, x)
    assert smallest == 0.0 or smallest >= F32_MIN_NORMAL, \
        f"fp32 gate: a product |a_ij x_j| = {smallest:.3e} is subnormal in fp32; the bound does not hold"
    assert sums.size == 0 or sums.max() * (1.0 + 2.0 ** -10) < F32_MAX, "fp32 gate: a row sum overflows fp32"
    n = np.diff(np.asarray(row_ptr, dtype=np.int64))
    # (sums is itself an fp64 sum of n terms and |y - ref| is rounded once more: the last factor covers both)
    return (gamma(n, U32) + gamma(n, U64)) * sums * (1.0 + 4.0 * gamma(n + 2, U64))


_ORACLE = []


def _oracle(cls):
    if not _ORACLE:
        _ORACLE.append(cls())
    return _ORACLE[0]


def assert_parity_f32(y, y_ref, row_ptr, col_idx, values, x, what=""):
    """Every row of an fp32 result against the fp64-accumulated oracle (y_ref = oracle.csr_f32_accum64), within the
    rigorous fp32 summation bound above; results finite."""
    y = np.asarray(y)
    y_ref = np.asarray(y_ref, dtype=np.float64)
    assert y.shape == y_ref.shape, f"{what}: shape {y.shape} vs {y_ref.shape}"
    assert len(row_ptr) == y.size + 1, f"{what}: row_ptr has {len(row_ptr)} entries for {y.size} rows"
    if y.size == 0:
        return
    assert np.all(np.isfinite(y)), f"{what}: non-finite result in row {np.flatnonzero(~np.isfinite(y))[0]}"
    bound = f32_row_bound(row_ptr, col_idx, values, x)
    d = np.abs(y.astype(np.float64) - y_ref)
    bad = np.flatnonzero(d > bound)
    assert bad.size == 0, (f"{what}: {bad.size} rows beyond the fp32 summation bound; first row {bad[0]} "
                           f"({int(row_ptr[bad[0] + 1]) - int(row_ptr[bad[0]])} entries): y = {float(y[bad[0]])!r}, "
                           f"ref = {y_ref[bad[0]]!r}, |d| = {d[bad[0]]:.3e}, bound = {bound[bad[0]]:.3e}")


# ---- wide-range data and power-of-two scaling.  Every kernel's result is a fixed sequence of adds that depends on the
# matrix structure only, so with D_r, D_c diagonal matrices of +-2^e (exact in IEEE arithmetic while nothing under- or
# overflows, whatever the order of the adds and whether they are fused):  y(D_r A D_c^-1, D_c x) == D_r y(A, x), bit
# for bit.  A term from the wrong row or the wrong column breaks that however small it is.
WIDE_EXP = {np.dtype(np.float32): 40, np.dtype(np.float64): 300}


CHUNK = 1 << 24   # (entries per step: the full-size matrices hold 2.6e8)


def wide_range(rng, n, dtype):
    """n values with random signs and magnitudes spread over [2^-8, 1]."""
    out = np.empty(n, dtype=dtype)
    for s in range(0, n, CHUNK):
        m = min(CHUNK, n - s)
        mag = np.exp2(-8.0 * rng.random(m))
        out[s:s + m] = np.where(rng.random(m) < 0.5, -mag, mag)
    return out


def scaling(rng, M, N, dtype):
    """(d_r, d_c): random +-2^e for every row and column, e within WIDE_EXP of the dtype."""
    e = WIDE_EXP[np.dtype(dtype)]
    dr = np.ldexp(np.where(rng.random(M) < 0.5, -1.0, 1.0), rng.integers(-e, e + 1, M))
    dc = np.ldexp(np.where(rng.random(N) < 0.5, -1.0, 1.0), rng.integers(-e, e + 1, N))
    return dr, dc


def scaled_copy(row_ptr, col_idx, values, x, dr, dc):
    """(D_r A D_c^-1 values, D_c x) in the data's dtype; asserts every entry stays a normal number (which makes the
    scaling exact) and that the scaling is undone exactly."""
    values = np.asarray(values)
    dtype = values.dtype
    tiny, big = np.finfo(dtype).tiny, np.finfo(dtype).max / 2.0 ** 20
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    v = np.empty_like(values)
    r0 = 0
    while r0 < len(row_ptr) - 1:          # whole rows, about CHUNK entries at a time
        r1 = max(r0 + 1, int(np.searchsorted(row_ptr, row_ptr[r0] + CHUNK, side="right")) - 1)
        r1 = min(r1, len(row_ptr) - 1)
        e0, e1 = int(row_ptr[r0]), int(row_ptr[r1])
        f = dr[np.repeat(np.arange(r0, r1), np.diff(row_ptr[r0:r1 + 1]))] / dc[col_idx[e0:e1]]
        a = values[e0:e1].astype(np.float64)
        out = (a * f).astype(dtype)
        m = np.abs(out)
        assert np.all(np.isfinite(out)) and np.all((m >= tiny) & (m <= big)), "scaled values leave the normal range"
        assert np.array_equal(out.astype(np.float64) / f, a), "the scaling of the values is not exact"
        v[e0:e1] = out
        r0 = r1
    xs = (np.asarray(x, dtype=np.float64) * dc).astype(dtype)
    m = np.abs(xs)
    assert np.all(np.isfinite(xs)) and np.all((m >= tiny) & (m <= big)), "scaled x leaves the normal range"
    assert np.array_equal(xs.astype(np.float64) / dc, np.asarray(x, dtype=np.float64)), "the scaling of x is not exact"
    return v, xs


def scale_rows(y, dr):
    """D_r y in y's dtype (exact: power-of-two factors, asserted to stay within the normal range or exactly 0)."""
    y = np.asarray(y)
    out = (y.astype(np.float64) * dr.reshape((-1,) + (1,) * (y.ndim - 1))).astype(y.dtype)
    m = np.abs(out)
    assert np.all(np.isfinite(out)) and np.all((m == 0) | (m >= np.finfo(y.dtype).tiny)), "D_r y leaves the normal range"
    return out


def assert_same_numbers(a, b, what=""):
    """a == b element by element (+0 equals -0), no NaN anywhere."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    assert not np.isnan(a).any() and not np.isnan(b).any(), f"{what}: NaN"
    bad = np.flatnonzero((a != b).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} elements differ; first at flat index {bad[0]}: "
                           f"{a.reshape(-1)[bad[0]]!r} vs {b.reshape(-1)[bad[0]]!r}")


# ---- poison: what 0 x something hides.  A NaN or an infinity in x (or in a stored value) must reach exactly the rows
# that store an entry reading it, and change no bit of any other row: no kernel has atomics and no launch decision
# reads values, so a row's sequence of adds is fixed by the structure.  Judged against the structure and the serial
# oracle only.
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(y_clean, y_poisoned, rows, what):
    bad = rows[_bits(y_clean)[rows] != _bits(y_poisoned)[rows]]
    assert bad.size == 0, (f"{what}: {bad.size} rows that read nothing poisoned changed bits; first row {bad[0]}: "
                           f"{y_clean[bad[0]]!r} -> {y_poisoned[bad[0]]!r}")


def rows_reading(row_ptr, col, columns_mask):
    """Mask of the rows that store an entry in a column of columns_mask."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    hit = np.concatenate([[0], np.cumsum(columns_mask[np.asarray(col)], dtype=np.int64)])
    return hit[row_ptr[1:]] > hit[row_ptr[:-1]]


def assert_poison_x(y_clean, y_poisoned, row_ptr, col, val, x_poisoned, oracle_y, what=""):
    """y_poisoned = A x_poisoned against y_clean (the same handle and variant on the same x with finite values in the
    poisoned places) and oracle_y (the serial fp64 oracle on x_poisoned).  A row that stores no entry in a non-finite
    column keeps y_clean's bits; a row that stores one has the oracle's class (NaN, +Inf or -Inf), which does not
    depend on the order of the adds while finite partial sums cannot overflow: values and finite x within [-1, 1]."""
    y_clean, y_poisoned, oracle_y = np.asarray(y_clean), np.asarray(y_poisoned), np.asarray(oracle_y, dtype=np.float64)
    val, x_poisoned = np.asarray(val), np.asarray(x_poisoned)
    M = len(row_ptr) - 1
    assert y_clean.shape == y_poisoned.shape == oracle_y.shape == (M,), f"{what}: shapes"
    assert y_clean.dtype == y_poisoned.dtype, f"{what}: {y_clean.dtype} vs {y_poisoned.dtype}"
    poisoned = ~np.isfinite(x_poisoned)
    assert np.all(np.isfinite(val)) and (val.size == 0 or np.abs(val).max() <= 1), f"{what}: values beyond [-1, 1]"
    assert np.abs(x_poisoned[~poisoned]).max(initial=0) <= 1, f"{what}: finite x beyond [-1, 1]"
    touched = rows_reading(row_ptr, col, poisoned)
    assert not np.isfinite(oracle_y[touched]).any() and np.isfinite(oracle_y[~touched]).all(), \
        f"{what}: the oracle disagrees with the structure about which rows read a poisoned column"
    _same_bits(y_clean, y_poisoned, np.flatnonzero(~touched), what)
    y = y_poisoned.astype(np.float64)
    for name, want, got in (("NaN", np.isnan(oracle_y), np.isnan(y)), ("+Inf", oracle_y == np.inf, y == np.inf),
                            ("-Inf", oracle_y == -np.inf, y == -np.inf)):
        bad = np.flatnonzero(touched & (want != got))
        assert bad.size == 0, (f"{what}: {bad.size} rows that read a poisoned column are not {name} where the oracle "
                               f"is (or are where it is not); first row {bad[0]}: {y_poisoned[bad[0]]!r}, oracle "
                               f"{oracle_y[bad[0]]!r}")


def assert_poison_values(y_clean, y_poisoned, poisoned_rows, what=""):
    """Exactly the rows holding a NaN stored value are NaN; every other row keeps the clean handle's bits."""
    y_clean, y_poisoned = np.asarray(y_clean), np.asarray(y_poisoned)
    assert y_clean.shape == y_poisoned.shape and y_clean.dtype == y_poisoned.dtype, f"{what}: shapes"
    mask = np.zeros(len(y_clean), dtype=bool)
    mask[np.asarray(poisoned_rows, dtype=np.int64)] = True
    bad = np.flatnonzero(mask & ~np.isnan(y_poisoned))
    assert bad.size == 0, f"{what}: row {bad[0]} holds a NaN value and is {y_poisoned[bad[0]]!r}"
    assert np.isfinite(y_clean).all(), f"{what}: the clean result is not finite"
    _same_bits(y_clean, y_poisoned, np.flatnonzero(~mask), what)


def assert_guard_bands(buffer_bytes_before, buffer_bytes_after, what=""):
    """The bytes around a caller's y are what they were."""
    a = np.frombuffer(bytes(buffer_bytes_before), dtype=np.uint8)
    b = np.frombuffer(bytes(buffer_bytes_after), dtype=np.uint8)
    assert a.size == b.size and a.size > 0, f"{what}: guard bands of {a.size} and {b.size} bytes"
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (f"{what}: {bad.size} guard bytes changed; first at byte {bad[0]}: "
                           f"{a[bad[0]]:#04x} -> {b[bad[0]]:#04x}")


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


# ---- what the compiler made of a translation unit: every kernel's static LDS, scratch and VGPRs from the code
# object's metadata (the gfx950 assembly that -save-temps keeps)
HIPCC = "/opt/rocm/bin/hipcc"
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SRC = os.path.join(_ROOT, "sparsematrixvectormultiplication_amd", "csrc", "hip")
Kernel = collections.namedtuple("Kernel", "lds scratch vgprs")


def compile_kernels(source, timeout=600):
    """{mangled kernel name: Kernel(lds, scratch, vgprs)} of csrc/hip/<source> compiled for gfx950."""
    tmp = tempfile.mkdtemp(prefix="spmv_isa_")
    try:
        proc = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950",
                               "-I" + os.path.join(_ROOT, "include"),
                               "-I" + HIP_SRC, "-c", os.path.join(HIP_SRC, source), "-o", os.path.join(tmp, "o.o"),
                               "-save-temps=obj"], capture_output=True, text=True, timeout=timeout, cwd=tmp)
        assert proc.returncode == 0, proc.stderr[-2000:]
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(2)] = Kernel(int(m.group(1)), int(m.group(3)), int(m.group(4)))
    return kernels
