"""The smoothed-aggregation AMG preconditioner restated in numpy / scipy: the setup rule by rule (include/spmv_hip.h),
the V(1,1) cycle, the same cycle with an entry-wise running error bound, and the small solvers the tests count steps
with.  test_amg_host.py holds the host setup against it, test_gpu_amg.py the device."""
import numpy as np
import scipy.sparse as sps

NOT_COARSEST, DIRECT, SMOOTH = 0, 1, 2


# ---------------------------------------------------------------- matrices
def laplacian(gx, gy, ax=1.0, ay=1.0):
    """The 5-point stencil on a gx x gy grid (row = x * gy + y): -ax to the x neighbours, -ay to the y neighbours,
    2 (ax + ay) on the diagonal; sorted CSR."""
    tx = sps.diags([-ax * np.ones(gx - 1), 2 * ax * np.ones(gx), -ax * np.ones(gx - 1)], [-1, 0, 1])
    ty = sps.diags([-ay * np.ones(gy - 1), 2 * ay * np.ones(gy), -ay * np.ones(gy - 1)], [-1, 0, 1])
    a = sps.csr_matrix(sps.kron(tx, sps.identity(gy)) + sps.kron(sps.identity(gx), ty))
    a.sort_indices()
    return a


def with_isolated_rows(a, extra, seed=0):
    """a with `extra` rows that hold a diagonal entry alone scattered in (a symmetric permutation of diag(a, D))."""
    n = a.shape[0]
    rng = np.random.default_rng(seed)
    big = sps.block_diag([a, sps.diags(rng.uniform(0.5, 3.0, extra))], format="csr")
    perm = rng.permutation(n + extra)
    out = sps.csr_matrix(big[perm][:, perm])
    out.sort_indices()
    return out


def spd_band(n, half, seed=0):
    """A symmetric, strictly diagonally dominant random band matrix of n rows (so SPD), about half the band stored."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in range(max(0, i - half), i):
            if rng.random() < 0.5:
                v = -rng.uniform(0.1, 1.0)
                rows += [i, j]
                cols += [j, i]
                vals += [v, v]
    a = sps.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a = sps.csr_matrix(a + sps.diags(np.asarray(abs(a).sum(axis=1)).ravel() * 1.05 + 0.1))
    a.sort_indices()
    return a


def convection_diffusion(g, beta=0.4):
    """A nonsymmetric 5-point stencil on g x g: the Laplacian with the x couplings -1 -+ beta (upwind-free central
    convection, diagonally dominant for |beta| < 1)."""
    a = laplacian(g, g).tolil()
    for x in range(g):
        for y in range(g):
            i = x * g + y
            if x > 0:
                a[i, i - g] = -1.0 - beta
            if x < g - 1:
                a[i, i + g] = -1.0 + beta
    a = sps.csr_matrix(a)
    a.sort_indices()
    return a


def csr_of(triple, shape):
    rp, col, val = triple
    return sps.csr_matrix((np.asarray(val, dtype=np.float64), col, rp), shape=shape)


# ---------------------------------------------------------------- the setup
def ones_of(m):
    m = sps.csr_matrix(m)
    return sps.csr_matrix((np.ones(len(m.indices)), m.indices, m.indptr), shape=m.shape)


def structural_product(a, b):
    """a @ b on the STRUCTURAL pattern (scipy drops an entry whose sum cancels to 0; the setup keeps it), sorted"""
    pat = sps.csr_matrix(ones_of(a) @ ones_of(b))
    pat.sort_indices()
    c = sps.csr_matrix(a @ b)
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    vals = np.asarray(c[rows, pat.indices]).ravel() if len(rows) else np.zeros(0)
    return sps.csr_matrix((vals, pat.indices, pat.indptr), shape=pat.shape)


def strength_neighbours(a, d, theta):
    """the symmetrised strength graph as ascending neighbour lists"""
    n = a.shape[0]
    nb = [set() for _ in range(n)]
    for i in range(n):
        for e in range(a.indptr[i], a.indptr[i + 1]):
            j, v = int(a.indices[e]), a.data[e]
            if j != i and v != 0.0 and abs(v) >= theta * np.sqrt(d[i] * d[j]):
                nb[i].add(j)
                nb[j].add(i)
    return [sorted(s) for s in nb]


def aggregate(nb):
    n = len(nb)
    agg = [-1] * n
    na = 0
    for i in range(n):  # (a)
        if nb[i] and agg[i] < 0 and all(agg[j] < 0 for j in nb[i]):
            agg[i] = na
            for j in nb[i]:
                agg[j] = na
            na += 1
    after_a = list(agg)
    for i in range(n):  # (b)
        if agg[i] < 0:
            for j in nb[i]:
                if after_a[j] >= 0:
                    agg[i] = after_a[j]
                    break
    for i in range(n):  # (c)
        if agg[i] < 0 and nb[i]:
            agg[i] = na
            for j in nb[i]:
                if agg[j] < 0:
                    agg[j] = na
            na += 1
    return np.array(agg, dtype=np.int64), na


def level_step(a, theta):
    """one level of the setup on the canonical fp64 matrix a: w, rho, and -- when the level were not the coarsest --
    agg, na, T, P, R and the next matrix (None when aggregation stalls)"""
    n = a.shape[0]
    d = a.diagonal()
    rho = 0.0
    for i in range(n):
        s = 0.0
        for v in a.data[a.indptr[i]:a.indptr[i + 1]]:
            s += abs(v)
        rho = max(rho, s / d[i])
    w = 4.0 / (3.0 * rho)
    agg, na = aggregate(strength_neighbours(a, d, theta))
    out = {"w": w, "rho": rho, "agg": agg, "na": na, "d": d}
    if na == 0 or 10 * na > 9 * n:
        return out
    rows = np.nonzero(agg >= 0)[0]
    t = sps.csr_matrix((np.ones(len(rows)), (rows, agg[rows])), shape=(n, na))
    at = structural_product(a, t)  # a sum that cancels stays
    p = at.copy()
    row_of = np.repeat(np.arange(n), np.diff(at.indptr))
    p.data = (at.indices == agg[row_of]).astype(np.float64) - (w / d)[row_of] * at.data
    r = sps.csr_matrix(p.T)
    r.sort_indices()
    nxt = structural_product(r, structural_product(a, p))
    out.update(T=t, P=p, R=r, next=nxt)
    return out


def build(a, theta=0.08, coarse_rows=64, max_levels=16):
    """the whole hierarchy: a list of {"A", "w", "rho", "kind", and "P", "R" or "inv"}"""
    levels = []
    while True:
        n = a.shape[0]
        if n <= coarse_rows:
            step = level_step_scalars(a)
            levels.append({"A": a, "w": step[0], "rho": step[1], "kind": DIRECT, "inv": np.linalg.inv(a.toarray())})
            return levels
        if len(levels) + 1 == max_levels:
            step = level_step_scalars(a)
            levels.append({"A": a, "w": step[0], "rho": step[1], "kind": SMOOTH})
            return levels
        s = level_step(a, theta)
        if "P" not in s:
            levels.append({"A": a, "w": s["w"], "rho": s["rho"], "kind": SMOOTH})
            return levels
        levels.append({"A": a, "w": s["w"], "rho": s["rho"], "kind": NOT_COARSEST, "P": s["P"], "R": s["R"], "agg": s["agg"]})
        a = s["next"]


def level_step_scalars(a):
    rho = float(np.max(np.asarray(abs(a).sum(axis=1)).ravel() / a.diagonal()))
    return 4.0 / (3.0 * rho), rho


def from_reader(levels):
    """the levels a reader returned (sp.amg_plan, Preconditioner.levels()) as scipy matrices in fp64"""
    out = []
    for lv in levels:
        n = lv["rows"]
        e = {"A": csr_of(lv["A"], (n, n)), "w": lv["w"], "rho": lv["rho"], "kind": lv["kind"]}
        if lv["kind"] == NOT_COARSEST:
            e["P"] = csr_of(lv["P"], (n, lv["aggregates"]))
            e["R"] = csr_of(lv["R"], (lv["aggregates"], n))
        elif lv["kind"] == DIRECT:
            e["inv"] = csr_of(lv["inv"], (n, n)).toarray()
        out.append(e)
    return out


# ---------------------------------------------------------------- the cycle
def cycle(levels, b, l=0, dtype=np.float64):
    """one V(1,1) cycle on b (n_l values, or n_l x k); every vector rounded once to dtype when it is stored"""
    lv = levels[l]
    a = lv["A"]
    rnd = lambda v: np.asarray(v, dtype=np.float64).astype(dtype).astype(np.float64)  # noqa: E731
    if lv["kind"] == DIRECT:
        return rnd(lv["inv"] @ b)
    g = lv["w"] / a.diagonal()
    if b.ndim == 2:
        g = g[:, None]
    x = rnd(g * b)
    if lv["kind"] == NOT_COARSEST:
        r = rnd(b - a @ x)
        e = cycle(levels, rnd(lv["R"] @ r), l + 1, dtype)
        x = rnd(x + lv["P"] @ e)
    return rnd(x + g * (b - a @ x))


def longest(m):
    return int(np.max(np.diff(sps.csr_matrix(m).indptr))) if m.shape[0] else 0


def cycle_with_bound(levels, b, dtype, l=0, eb=None):
    """(z, bound): the cycle in fp64 on b and a bound on |device - z| entry by entry.  Every pass out = f(inputs) adds
    to the inputs' bounds carried through |f| its own rounding: the pass evaluated on absolute values, times
    (2 k + 6) eps with k the operator's longest row -- k products and k additions in double, the few operations of the
    row's formula and the store to dtype on the device (each at most eps / 2 relative, eps of dtype), and as much again
    for this fp64 restatement."""
    eps = float(np.finfo(dtype).eps)
    lv = levels[l]
    a = lv["A"]
    aa = abs(a)
    eb = np.zeros_like(b) if eb is None else eb
    if lv["kind"] == DIRECT:
        inv = lv["inv"]
        return inv @ b, abs(inv) @ eb + (2 * a.shape[0] + 6) * eps * (abs(inv) @ (abs(b) + eb))
    g = lv["w"] / a.diagonal()
    if b.ndim == 2:
        g = g[:, None]
    ka = longest(a)
    x = g * b
    ex = g * eb + 6 * eps * g * (abs(b) + eb)
    if lv["kind"] == NOT_COARSEST:
        p, r_ = lv["P"], lv["R"]
        res = b - a @ x
        eres = eb + aa @ ex + (2 * ka + 6) * eps * (abs(b) + eb + aa @ (abs(x) + ex))
        bc = r_ @ res
        ebc = abs(r_) @ eres + (2 * longest(r_) + 6) * eps * (abs(r_) @ (abs(res) + eres))
        e, ee = cycle_with_bound(levels, bc, dtype, l + 1, ebc)
        x2 = x + p @ e
        ex = ex + abs(p) @ ee + (2 * longest(p) + 6) * eps * (abs(x) + ex + abs(p) @ (abs(e) + ee))
        x = x2
    z = x + g * (b - a @ x)
    ez = ex + g * (eb + aa @ ex) + (2 * ka + 6) * eps * (abs(x) + ex + g * (abs(b) + eb + aa @ (abs(x) + ex)))
    return z, ez


def dense_m(levels, n):
    """the cycle as a dense matrix M (column j = cycle(e_j))"""
    return cycle(levels, np.eye(n))


# ---------------------------------------------------------------- solvers that count steps
def pcg_steps(a, b, apply, tol, maxit=5000):
    """preconditioned CG from x0 = 0 to r.r <= tol^2 r0.r0; returns (steps, x)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = apply(r)
    p = z.copy()
    rz = r @ z
    rr0 = r @ r
    for t in range(1, maxit + 1):
        q = a @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = apply(r)
        rz_new = r @ z
        if r @ r <= tol * tol * rr0:
            return t, x
        p = z + (rz_new / rz) * p
        rz = rz_new
    return maxit, x
