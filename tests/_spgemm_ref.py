"""The definition of C = A B the device product is held to (include/spmv_hip.h), as a plain loop over numpy scalars:
every product and every sum is one rounded IEEE double operation, taken in entry order; the row's columns ascend; each
value is rounded once to the dtype.  Written for the tests' small matrices, not for speed."""
import numpy as np


def spgemm_ref(M, N, a, b, dtype):
    """(row_ptr, col, val) of C = A B; a and b are (row_ptr, col, val) triples, A with M rows, B with N columns."""
    rpa, ca, va = a
    rpb, cb, vb = b
    va = np.asarray(va).astype(np.float64)      # exact for fp32 data
    vb = np.asarray(vb).astype(np.float64)
    row_ptr = np.zeros(M + 1, dtype=np.int32)
    cols, vals = [], []
    for i in range(M):
        acc = {}
        for e in range(int(rpa[i]), int(rpa[i + 1])):
            j, av = int(ca[e]), va[e]
            for f in range(int(rpb[j]), int(rpb[j + 1])):
                c = int(cb[f])
                p = av * vb[f]                    # np.float64 * np.float64: one rounded product
                acc[c] = p if c not in acc else acc[c] + p
        for c in sorted(acc):
            cols.append(c)
            vals.append(acc[c])
        row_ptr[i + 1] = len(cols)
    return row_ptr, np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64).astype(dtype)


def row_products(a, b):
    """products[i] = the sum over row i's entries of the length of B's row colA[e] (what the plan is made from)"""
    rpa, ca, _ = a
    lens = np.diff(np.asarray(b[0], dtype=np.int64))
    per_entry = lens[np.asarray(ca, dtype=np.int64)] if len(ca) else np.zeros(0, dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(per_entry)])
    rpa = np.asarray(rpa, dtype=np.int64)
    return (cum[rpa[1:]] - cum[rpa[:-1]]).astype(np.int64)


def transpose_ref(M, N, row_ptr, col, val):
    """(row_ptr, col, val) of A^T: a stable sort of the entries by column (what CsrDevice.transpose gives)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col)
    rows = np.repeat(np.arange(M, dtype=np.int32), np.diff(row_ptr))
    order = np.argsort(col, kind="stable")
    counts = np.bincount(col, minlength=N) if len(col) else np.zeros(N, dtype=np.int64)
    rp_t = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), np.asarray(val)[order]
