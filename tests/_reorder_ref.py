"""The definitions of CsrDevice.permute and of the reverse Cuthill-McKee ordering (include/spmv_hip.h), restated in
numpy and plain Python: what the host plan (sp.rcm_plan) and the device builds are held to, byte for byte."""
import numpy as np


def inverse(perm):
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


def permute_ref(M, N, rp, col, val, row_perm=None, col_perm=None):
    """C[i, j] = A[row_perm[i], col_perm[j]]: row i of C is row row_perm[i] of A, entry by entry, each value bit for
    bit, each column c replaced by the j with col_perm[j] == c.  Nothing sorted, nothing combined."""
    rp = np.asarray(rp, dtype=np.int64)
    p = np.arange(M, dtype=np.int64) if row_perm is None else np.asarray(row_perm, dtype=np.int64)
    inv_q = np.arange(N, dtype=np.int64) if col_perm is None else inverse(col_perm)
    lens = (rp[1:] - rp[:-1])[p] if M else np.zeros(0, np.int64)
    rp_c = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(lens, out=rp_c[1:])
    # source entry of every entry of C: the start of its row in A plus its place in the row
    src = np.repeat(rp[:-1][p] - rp_c[:-1], lens) + np.arange(int(rp_c[-1]))
    return rp_c.astype(np.int32), inv_q[np.asarray(col)[src]].astype(np.int32), np.asarray(val)[src]


def graph_of(n, rp, col):
    """Neighbour lists (ascending index) of G: u ~ v iff u != v and A stores (u, v) or (v, u)."""
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), rp[1:] - rp[:-1])
    off = rows != col
    u = np.concatenate([rows[off], col[off]])
    v = np.concatenate([col[off], rows[off]])
    pairs = np.unique(u * max(n, 1) + v)
    u, v = pairs // max(n, 1), pairs % max(n, 1)
    start = np.searchsorted(u, np.arange(n + 1))
    return [v[start[i]:start[i + 1]].tolist() for i in range(n)]


def rcm_ref(n, rp, col, peripheral=2):
    """perm of the definition: the serial loop, line for line."""
    adj = graph_of(n, rp, col)
    deg = [len(a) for a in adj]
    key = lambda v: (deg[v], v)  # noqa: E731
    by_key = sorted(range(n), key=key)
    visited = [False] * n
    seq = []

    def search(s):  # (number of levels, the last level) of a breadth-first search from s over unvisited nodes
        seen = {s}
        level, depth = [s], 0
        while level:
            last, depth = level, depth + 1
            level = []
            for u in last:
                for w in adj[u]:
                    if not visited[w] and w not in seen:
                        seen.add(w)
                        level.append(w)
        return depth, last

    cursor = 0
    while cursor < n:
        s = by_key[cursor]
        if visited[s]:
            cursor += 1
            continue
        if deg[s] and peripheral > 0:
            depth_s, last = search(s)
            for _ in range(peripheral):
                t = min(last, key=key)
                depth_t, last_t = search(t)
                if depth_t <= depth_s:
                    break
                s, depth_s, last = t, depth_t, last_t
        head = len(seq)
        seq.append(s)
        visited[s] = True
        while head < len(seq):
            v = seq[head]
            head += 1
            for w in sorted((w for w in adj[v] if not visited[w]), key=key):
                visited[w] = True
                seq.append(w)
    return np.asarray(seq[::-1], dtype=np.int32)


def bandwidth(n, rp, col, perm=None):
    """max |i - j| over the stored entries; with perm, of the matrix renumbered by it: max |inv[i] - inv[j]|."""
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    if not len(col):
        return 0
    rows = np.repeat(np.arange(n, dtype=np.int64), rp[1:] - rp[:-1])
    if perm is not None:
        inv = inverse(perm)
        rows, col = inv[rows], inv[col]
    return int(np.abs(rows - col).max())


# ------------------------------------------------------------------ the graphs both test files walk
def csr_of_edges(n, edges, symmetric=True, diagonal=False):
    """CSR pattern (row_ptr, col) with canonical rows from an edge list."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    u, v = e[:, 0], e[:, 1]
    if symmetric:
        u, v = np.concatenate([u, v]), np.concatenate([v, u])
    if diagonal:
        u, v = np.concatenate([u, np.arange(n)]), np.concatenate([v, np.arange(n)])
    pairs = np.unique(u * max(n, 1) + v)
    u, v = pairs // max(n, 1), pairs % max(n, 1)
    rp = np.searchsorted(u, np.arange(n + 1)).astype(np.int32)
    return rp, v.astype(np.int32)


def grid_edges(nx, ny, nz=1):
    idx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    e = [np.stack([idx[:, :, :-1].ravel(), idx[:, :, 1:].ravel()], 1),
         np.stack([idx[:, :-1, :].ravel(), idx[:, 1:, :].ravel()], 1),
         np.stack([idx[:-1, :, :].ravel(), idx[1:, :, :].ravel()], 1)]
    return np.concatenate(e)


def shuffled(n, rp, col, seed):
    """The pattern renumbered by one seeded symmetric random permutation, rows canonical again."""
    p = np.random.default_rng(seed).permutation(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    inv = inverse(p)
    return csr_of_edges(n, np.stack([inv[rows], inv[np.asarray(col)]], 1), symmetric=False)


def rcm_graphs():
    """name -> (n, row_ptr, col): the list of the issue, small enough for the serial Python loop."""
    rng = np.random.default_rng(20)
    g = {}
    g["path"] = (40, *csr_of_edges(40, [(i, i + 1) for i in range(39)]))
    g["star"] = (33, *csr_of_edges(33, [(0, i) for i in range(1, 33)]))
    g["ring"] = (50, *csr_of_edges(50, [(i, (i + 1) % 50) for i in range(50)], diagonal=True))
    g["grid_1xn"] = (70, *csr_of_edges(70, grid_edges(70, 1), diagonal=True))
    g["grid_gxg"] = (40 * 40, *csr_of_edges(1600, grid_edges(40, 40), diagonal=True))
    g["k70"] = (70, *csr_of_edges(70, [(i, j) for i in range(70) for j in range(i)]))
    g["binary_tree"] = (1023, *csr_of_edges(1023, [((i - 1) // 2, i) for i in range(1, 1023)], diagonal=True))
    g["grid_3d"] = (9 * 8 * 7, *csr_of_edges(504, grid_edges(9, 8, 7), diagonal=True))
    for k, (n, m) in enumerate(((200, 300), (500, 2500), (301, 310))):
        g[f"random_{k}"] = (n, *csr_of_edges(n, rng.integers(0, n, (m, 2))))
    g["nonsymmetric"] = (300, *csr_of_edges(300, rng.integers(0, 300, (700, 2)), symmetric=False))
    # unsorted rows with repeats: every row's entries twice over, in a random order
    n, rp, col = g["random_0"]
    rows = np.repeat(np.arange(n), np.diff(rp))
    order = rng.permutation(2 * len(col))
    r2, c2 = np.concatenate([rows, rows])[order], np.concatenate([col, col])[order]
    by_row = np.argsort(r2, kind="stable")
    g["unsorted_repeats"] = (n, np.searchsorted(r2[by_row], np.arange(n + 1)).astype(np.int32), c2[by_row].astype(np.int32))
    # three components, isolated rows with and without a diagonal among them
    e = np.concatenate([grid_edges(6, 5) + 3, rng.integers(40, 90, (120, 2)), [(95, 96), (96, 97)]])
    g["components_isolated"] = (100, *csr_of_edges(100, np.concatenate([e, [(0, 0), (35, 35), (99, 99)]])))
    g["diagonal_only"] = (17, np.arange(18, dtype=np.int32), np.arange(17, dtype=np.int32))
    g["n1"] = (1, np.array([0, 1], np.int32), np.array([0], np.int32))
    g["n1_empty"] = (1, np.array([0, 0], np.int32), np.zeros(0, np.int32))
    g["no_entries"] = (12, np.zeros(13, np.int32), np.zeros(0, np.int32))
    return g


def spd_band(n, band, per_row, seed, dtype=np.float64):
    """A symmetric, strictly diagonally dominant (so positive definite) band: every row draws per_row // 2 columns within
    `band` below the diagonal, the pattern is mirrored, off-diagonal values are negative and the diagonal is one more
    than the row's absolute sum.  Canonical rows.  Returns (row_ptr, col, val)."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n, dtype=np.int64), per_row // 2)
    cols = rows - rng.integers(1, band + 1, rows.size)
    keep = cols >= 0
    rp, col = csr_of_edges(n, np.stack([rows[keep], cols[keep]], 1), diagonal=True)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    # one value per unordered pair, so that the matrix is symmetric: a hash of (min, max)
    lo, hi = np.minimum(r, col), np.maximum(r, col)
    val = -(((lo * 2654435761 + hi * 40503) % 1000) + 1) / 1000.0
    diag = r == col
    val[diag] = 0.0
    val[diag] = 1.0 - np.add.reduceat(val, rp[:-1].astype(np.int64))
    return rp, col, val.astype(dtype)


# The banded case (the GPU suite runs the same arrays end to end): 20000 rows, columns within 150 of the diagonal, about
# 22 entries per row.  On the CPU the host plan gives 219 x-window blocks in natural order, 0 after the shuffle and 219
# again after rcm_plan (bandwidth 311).  The same held at 8000 rows / band 40; the larger size is the one whose device
# upload tests/test_gpu_spmm.py already relies on for an x-window plan.
BAND_N, BAND_WIDTH, BAND_PER_ROW, BAND_SEED, SHUFFLE_SEED = 20000, 150, 22, 7, 1


def banded_case():
    """(natural, shuffled): (row_ptr, col, val) of the SPD band and of its seeded symmetric shuffle"""
    rp, col, val = spd_band(BAND_N, BAND_WIDTH, BAND_PER_ROW, BAND_SEED)
    p = np.random.default_rng(SHUFFLE_SEED).permutation(BAND_N)
    return (rp, col, val), permute_ref(BAND_N, BAND_N, rp, col, val, p, p)
