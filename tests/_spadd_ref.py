"""The definition of C = alpha A + beta B the device sum is held to (include/spmv_hip.h), as plain loops over numpy
scalars: canon(X) adds a row's repeated (row, column) pairs in entry order in double and rounds once to the dtype; the
sum is formed on the union of the canonical patterns, every product and every sum one rounded IEEE double operation,
rounded once to the dtype.  Written for the tests' small matrices, not for speed."""
import numpy as np


def canon(M, N, a, dtype):
    """(row_ptr, col, val) of canon(A): ascending columns without repeats; a is a (row_ptr, col, val) triple"""
    rp, ca, va = a
    va = np.asarray(va).astype(np.float64)      # exact for fp32 data
    row_ptr = np.zeros(M + 1, dtype=np.int32)
    cols, vals = [], []
    for i in range(M):
        acc = {}
        for e in range(int(rp[i]), int(rp[i + 1])):
            c = int(ca[e])
            assert 0 <= c < N
            acc[c] = va[e] if c not in acc else acc[c] + va[e]   # np.float64 + np.float64: one rounded sum
        for c in sorted(acc):
            cols.append(c)
            vals.append(acc[c])
        row_ptr[i + 1] = len(cols)
    return row_ptr, np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64).astype(dtype)


def spadd_ref(M, N, a, b, dtype, alpha=1.0, beta=1.0):
    """((row_ptr, col, val) of alpha A + beta B (b = None: alpha canon(A)), the number of entries in both patterns, the
    rows' combined lengths len canon(A)_i + len canon(B)_i)"""
    alpha, beta = np.float64(alpha), np.float64(beta)
    ra, ca, va = canon(M, N, a, dtype)
    rb, cb, vb = canon(M, N, b, dtype) if b is not None else (np.zeros(M + 1, dtype=np.int32), ca[:0], va[:0])
    va, vb = va.astype(np.float64), vb.astype(np.float64)
    row_ptr = np.zeros(M + 1, dtype=np.int32)
    cols, vals, matches = [], [], 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(M):
            row = {int(ca[e]): alpha * va[e] for e in range(int(ra[i]), int(ra[i + 1]))}      # one rounded product
            for f in range(int(rb[i]), int(rb[i + 1])):
                c, p = int(cb[f]), beta * vb[f]
                if c in row:
                    row[c], matches = row[c] + p, matches + 1                                 # one rounded sum
                else:
                    row[c] = p
            for c in sorted(row):
                cols.append(c)
                vals.append(row[c])
            row_ptr[i + 1] = len(cols)
    combined = np.diff(ra.astype(np.int64)) + np.diff(rb.astype(np.int64))
    return (row_ptr, np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64).astype(dtype)), matches, combined


def identity_csr(n, dtype):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, dtype=dtype)


def random_unsorted(rng, M, N, mean, dtype):
    """the generator of test_gpu_spgemm.py, restated: unsorted rows, repeated (row, column) pairs, empty rows and columns;
    values with full mantissas, so a contracted multiply-add changes the bits of the sums"""
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


def random_sorted(rng, M, N, mean, dtype, values="mantissa"):
    """sorted rows without repeats, some empty; values of full mantissa, or small integers (sums exact in the dtype)"""
    lens = np.minimum(rng.poisson(mean, M), N)
    lens[rng.random(M) < 0.15] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens] + [np.zeros(0, dtype=np.int64)])
    if values == "mantissa":
        val = rng.uniform(1, 2, rp[-1]) * rng.choice([-1.0, 1.0], rp[-1])
    else:
        val = rng.integers(-8, 9, rp[-1]).astype(np.float64)
    return rp, col.astype(np.int32), val.astype(dtype)
