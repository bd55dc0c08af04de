"""The iterated methods (cg, cg_multi, pcg, bicgstab / pbicgstab, cgls) and the Jacobi, block-Jacobi, SSOR and ILU(0)
applies at the sizes where their vector kernels change path: one, two and three rows, rows that leave a cut 16-byte
piece, one row either side of a wavefront (64), a workgroup (256) and its multiples, and the first size past each
solver's grid cap, where the lanes' stride loop makes its second trip.

Three kinds of check.  (1) Exact integer gates: integer right-hand sides small enough that every partial sum is exact in
the handle's dtype, on A = I or a power-of-two diagonal, so no order of addition can change a bit and the expected
values come from integer arithmetic; a row counted twice or dropped changes the first history entry.  (2) One, two and
three steps against the reference loops of the other solver tests run over a long-double product, within 16 times the
reference's own rounding (measured on the CPU: `python tests/test_gpu_solver_sizes.py` prints the table below).
(3) The applies against long-double substitution and per-block solves within the bounds test_gpu_trsv.py and
test_gpu_precond.py derive, and apply_on / solve_on on a second stream with r / z placed at a 16-byte boundary and one
element past it, between sentinel values.

First size at which the lanes' stride loop makes a second trip (cap x kBlock x V + 1 rows; cg_multi: cap x rows per
workgroup + 1, rows per workgroup = kBlock / 2^cl, 2^cl the next power of two >= k / V, V = 16 / sizeof(T) when a row
of k values is whole 16-byte pieces, else 1):
    cg, pcg, cg_multi at k = 1 (cap 512, V = 1)            131 073
    bicgstab, pbicgstab, cgls (cap 2048)                 1 048 577 (fp64)    2 097 153 (fp32)
    cg_multi k = 8 (cap 2048)                              131 073 (fp64, 64 rows per workgroup)
                                                           262 145 (fp32, 128 rows per workgroup)
"""
import math

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from test_gpu_bicgstab import bicgstab_ref, true_rr
from test_gpu_cg_multi import cg_with
from test_gpu_cgls import cgls_ref
from test_gpu_hll_spmm import DeviceBuffer
from test_gpu_precond import block_minv, csr, dense_blocks, pbicgstab_ref, pcg_ref
from test_gpu_trsv import _hip, comparison, dominant, order_of, solve_ld, tri_parts

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = [np.float64, np.float32]

K_BLOCK = 256          # kBlock: csr_kernels.hpp
K_NORM_BLOCKS = 512    # kNormBlocks: solver_ops.hpp (csr_cg, csr_pcg, cg_multi at k = 1)
K_BCG_BLOCKS = 2048    # kBcgBlocks: bicgstab_kernels.hpp
K_CGLS_BLOCKS = 2048   # kCglsBlocks: cgls_kernels.hpp
K_MCG_BLOCKS = 2048    # kMcgBlocks: cg_multi_kernels.hpp (k > 1)

SMALL = [1, 2, 3, 5, 7, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025]
MCG_KS = (2, 3, 8)     # 16-byte pieces (fp64: 2, 8; fp32: 8) and single elements (3; fp32: 2)
MCG_EDGE_K = 8


def piece(dtype):
    """V: values of one 16-byte piece"""
    return 16 // np.dtype(dtype).itemsize


def mcg_rows_per_workgroup(k, dtype):
    """mcg_run in spmv_cg.hip: V = a piece when a row of k values is whole pieces, else 1; 2^cl column lanes"""
    v = piece(dtype) if k * np.dtype(dtype).itemsize % 16 == 0 else 1
    cl = 0
    while (1 << cl) * v < k:
        cl += 1
    return K_BLOCK >> cl


CG_EDGE = K_NORM_BLOCKS * K_BLOCK + 1


def bcg_edge(dtype):
    return K_BCG_BLOCKS * K_BLOCK * piece(dtype) + 1


def cgls_edge(dtype):
    return K_CGLS_BLOCKS * K_BLOCK * piece(dtype) + 1


def mcg_edge(dtype):
    return K_MCG_BLOCKS * mcg_rows_per_workgroup(MCG_EDGE_K, dtype) + 1


assert CG_EDGE == 131073 and bcg_edge(np.float64) == cgls_edge(np.float64) == 1048577
assert bcg_edge(np.float32) == cgls_edge(np.float32) == 2097153
assert mcg_edge(np.float64) == 131073 and mcg_edge(np.float32) == 262145


# ---------------------------------------------------------------- matrices
def identity(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)


def pow2_diagonal(n):
    """d_i in {1/2, 1, 2}"""
    d = np.ldexp(1.0, np.arange(n) % 3 - 1)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d


def stacked_identity(n):
    """(n + 3) x n: the identity on three rows without entries"""
    rp = np.concatenate([np.arange(n + 1), np.full(3, n)]).astype(np.int32)
    return rp, np.arange(n, dtype=np.int32), np.ones(n)


def sym_tridiagonal(n, seed=0):
    """SPD: diagonal uniform in [1, 2], off-diagonal entries +-1/4 (n < 3: the diagonal alone)"""
    import scipy.sparse as sps
    rng = np.random.default_rng([n, seed, 1])
    d = rng.uniform(1.0, 2.0, n)
    if n < 3:
        return csr(sps.diags(d).tocsr())[1:]
    off = 0.25 * rng.choice([-1.0, 1.0], n - 1)
    return csr(sps.diags([off, d, off], [-1, 0, 1]).tocsr())[1:]


def nonsym_tridiagonal(n, seed=0):
    """nonsymmetric: every row's off-diagonal absolute sum is 1/2, diagonal uniform in [1, 2] (n < 3: the diagonal)"""
    import scipy.sparse as sps
    rng = np.random.default_rng([n, seed, 2])
    if n < 3:
        return csr(sps.diags(rng.uniform(1.0, 2.0, n)).tocsr())[1:]
    return dominant(sps.diags([rng.uniform(-1, 1, n - 1), np.ones(n), rng.uniform(-1, 1, n - 1)], [-1, 0, 1]), rng,
                    scale=0.5)[1:]


def rect_banded(n, seed=0):
    """(n + 3) x n: (i, i) uniform in [1, 2], (i + 1, i) and (i + 3, i) = +-1/4 (n < 3: the diagonal on three rows
    without entries)"""
    import scipy.sparse as sps
    rng = np.random.default_rng([n, seed, 3])
    i = np.arange(n)
    d = rng.uniform(1.0, 2.0, n)
    if n < 3:
        a = sps.csr_matrix((d, (i, i)), shape=(n + 3, n))
    else:
        a = sps.csr_matrix((np.concatenate([d, 0.25 * rng.choice([-1.0, 1.0], 2 * n)]),
                            (np.concatenate([i, i + 1, i + 3]), np.concatenate([i, i, i]))), shape=(n + 3, n))
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def transposed(M, N, rp, col, val):
    import scipy.sparse as sps
    t = sps.csr_matrix((val, col, rp), shape=(M, N)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(np.int32), t.indices.astype(np.int32), np.ascontiguousarray(t.data)


def product(rp, col, val, acc=LD):
    """v -> A v with the products and each row's sum (entry order) in `acc`; rows without entries give 0"""
    vals = np.asarray(val).astype(acc)
    empty = np.diff(rp) == 0

    def apply(v):
        prod = np.append(vals * np.asarray(v).astype(acc)[col], acc(0))
        y = np.add.reduceat(prod, rp[:-1]) if len(rp) > 1 else np.zeros(0, acc)
        y[empty] = 0
        return y
    return apply


def diagonal_of(rp, col, val):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    d = np.zeros(len(rp) - 1)
    d[rows[col == rows]] = np.asarray(val, np.float64)[col == rows]
    return d


def stored_inverse(rp, col, val, dtype):
    """Jacobi's stored values: 1.0 / d in fp64, rounded once to dtype"""
    return (1.0 / diagonal_of(rp, col, val)).astype(dtype)


# ---------------------------------------------------------------- exact integer gates
EXACT_BELOW = {np.dtype(np.float64): 2 ** 53, np.dtype(np.float32): 2 ** 24}


def int_rhs(n, dtype, seed, scale=1):
    """n nonzero integers with scale x sum b^2 below 2^53 (fp64) or 2^24 (fp32): |b_i| <= isqrt(limit / (scale n)),
    at most 1000"""
    bmax = min(1000, math.isqrt((EXACT_BELOW[np.dtype(dtype)] - 1) // (scale * n)))
    assert bmax >= 1
    rng = np.random.default_rng([n, seed])
    return (rng.integers(1, bmax + 1, n) * rng.choice([-1, 1], n)).astype(np.int64)


def sumsq(b):
    return int(np.sum(b * b))


def check_x(x, expect, dtype, what):
    assert x.dtype == dtype and x.shape == expect.shape, (what, x.dtype, x.shape)
    assert x.tobytes() == expect.astype(dtype).tobytes(), what


def exact_cg_and_pcg(n, dtype):
    """A = I: alpha = 1, x = b, r = 0"""
    rp, col, val = identity(n)
    bi = int_rhs(n, dtype, 1)
    b, rr0 = bi.astype(dtype), float(sumsq(bi))
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev:
        x, h, _ = dev.cg(b, 2)
        assert h.tolist() == [rr0, 0.0, 0.0], ("cg", n, h.tolist(), rr0)
        check_x(x, b, dtype, f"cg n={n}")
        x, rr, rz, info, _ = dev.pcg(b, 2)
        assert rr.tolist() == [rr0, 0.0, 0.0] and rz.tolist() == [rr0, 0.0, 0.0], ("pcg", n, rr.tolist(), rz.tolist())
        assert info == {"steps": 1, "status": sp.PCG_CONVERGED}
        check_x(x, b, dtype, f"pcg n={n}")


def exact_cg_multi(n, dtype, ks):
    """A = I, a different integer b in each of the k columns"""
    rp, col, val = identity(n)
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev:
        for k in ks:
            Bi = np.stack([int_rhs(n, dtype, 10 + 7 * k + j) for j in range(k)], axis=1)
            B = np.ascontiguousarray(Bi.astype(dtype))
            X, h, done, _ = dev.cg_multi(B, 2)
            expect = [float(sumsq(Bi[:, j])) for j in range(k)]
            assert h.shape == (3, k) and h[0].tolist() == expect, ("cg_multi", n, k, h[0].tolist(), expect)
            assert np.all(h[1:] == 0.0) and done.tolist() == [1] * k, ("cg_multi", n, k, h[1:].tolist(), done)
            check_x(X, B, dtype, f"cg_multi n={n} k={k}")


def exact_jacobi(n, dtype):
    """A = D = diag(2^e), Jacobi: z = b / d, q = D z = b, alpha = 1, x = b / d; every value a multiple of 1/2"""
    rp, col, d = pow2_diagonal(n)
    bi = int_rhs(n, dtype, 2, scale=4)
    b, rr0 = bi.astype(dtype), float(sumsq(bi))
    rz0 = int(np.sum(bi * bi * np.array([4, 2, 1])[np.arange(n) % 3])) / 2.0      # sum b^2 / d
    with sp.CsrDevice(n, n, rp, col, d.astype(dtype)) as dev, dev.preconditioner("jacobi") as J:
        x, rr, rz, info, _ = dev.pcg(b, 2, precond=J)
        assert rr.tolist() == [rr0, 0.0, 0.0] and rz.tolist() == [rz0, 0.0, 0.0], ("pcg", n, rr.tolist(), rz.tolist())
        assert info == {"steps": 1, "status": sp.PCG_CONVERGED}
        check_x(x, bi / d, dtype, f"pcg jacobi n={n}")
        x, h, info, _ = dev.bicgstab(b, 2, precond=J)
        x_ref, h_ref, info_ref = pbicgstab_ref(lambda v: d * v, lambda v: v / d, bi.astype(np.float64), 2)
        assert info == info_ref and h[0] == rr0 and h.tobytes() == h_ref.tobytes(), ("pbicgstab", n, info, h.tolist())
        check_x(x, x_ref, dtype, f"pbicgstab jacobi n={n}")


def exact_bicgstab(n, dtype):
    """A = I: s = 0 at the first half step; the stop, the steps and x are the reference loop's"""
    rp, col, val = identity(n)
    bi = int_rhs(n, dtype, 3)
    b = bi.astype(dtype)
    with sp.CsrDevice(n, n, rp, col, val.astype(dtype)) as dev:
        x, h, info, _ = dev.bicgstab(b, 2)
    x_ref, h_ref, info_ref = bicgstab_ref(lambda v: v.copy(), bi.astype(np.float64), 2)
    assert info == info_ref and h[0] == float(sumsq(bi)) and h.tobytes() == h_ref.tobytes(), (n, info, h.tolist())
    check_x(x, x_ref, dtype, f"bicgstab n={n}")


def exact_cgls(n, dtype):
    """A = I_n on three empty rows: s = b[:n], alpha = 1, x = b[:n], r = (0, b[n:]), s = 0"""
    rp, col, val = stacked_identity(n)
    bi = int_rhs(n + 3, dtype, 4)
    b = bi.astype(dtype)
    with sp.CsrDevice(n + 3, n, rp, col, val.astype(dtype)) as dev, dev.transpose() as dt:
        x, ss, rr, info, _ = dev.cgls(b, 2, at=dt)
    assert ss.tolist() == [float(sumsq(bi[:n])), 0.0, 0.0], (n, ss.tolist())
    tail = float(sumsq(bi[n:]))
    assert rr.tolist() == [float(sumsq(bi)), tail, tail], (n, rr.tolist())
    assert info == {"steps": 1, "status": sp.CGLS_CONVERGED}
    check_x(x, b[:n], dtype, f"cgls n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SMALL)
def test_exact_integer_gates(gpu, n, dtype):
    """The first history entry of every solver is sum b_i^2 (r.z: sum b_i^2 / d_i, s.s: over the columns) bit for bit,
    one step closes in integers (x = b or b / d, the next entry exactly 0), and x has n entries of the handle's dtype."""
    exact_cg_and_pcg(n, dtype)
    exact_cg_multi(n, dtype, MCG_KS)
    exact_jacobi(n, dtype)
    exact_bicgstab(n, dtype)
    exact_cgls(n, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("family", ["cg_pcg", "cg_multi", "bicgstab", "cgls"])
def test_exact_integer_gates_at_the_grid_cap(gpu, family, dtype):
    """The same gates one row past each family's grid cap: the lanes' stride loop makes its second trip."""
    if family == "cg_pcg":
        exact_cg_and_pcg(CG_EDGE, dtype)
        exact_jacobi(CG_EDGE, dtype)
    elif family == "cg_multi":
        exact_cg_multi(mcg_edge(dtype), dtype, (MCG_EDGE_K,))
    elif family == "bicgstab":
        exact_bicgstab(bcg_edge(dtype), dtype)
        exact_jacobi(bcg_edge(dtype), dtype)
    else:
        exact_cgls(cgls_edge(dtype), dtype)


# ---------------------------------------------------------------- step-level agreement
# Largest difference between the reference loop run in the handle's dtype (vectors rounded to dtype after every
# update, dot products in fp64 as the kernels do) and the same loop over the long-double product, over all sizes of
# SMALL and, for fp64, the cap sizes; x relative to max |x|, history entries relative to the first one.  Printed by
# `python tests/test_gpu_solver_sizes.py`; the tolerance is 16 times it, and at least 4 eps.
MEASURED = {
    ("cg", "float64"): 7.323e-16,         # n = 1025, 1 step                  -> tolerance 1.172e-14
    ("cg_multi", "float64"): 5.501e-16,   # n = 511, 1 step                   -> tolerance 8.801e-15
    ("pcg", "float64"): 3.323e-16,        # n = 131073, 2 steps               -> tolerance 5.317e-15
    ("bicgstab", "float64"): 3.473e-16,   # n = 7, 3 steps                    -> tolerance 5.557e-15
    ("pbicgstab", "float64"): 8.612e-12,  # n = 1048577, 2 steps (history)    -> tolerance 1.378e-10
    ("cgls", "float64"): 5.705e-16,       # n = 1048577, 2 steps              -> tolerance 9.128e-15
    ("cg", "float32"): 9.333e-08,         # n = 64, 2 steps                   -> tolerance 1.493e-06
    ("cg_multi", "float32"): 1.085e-07,   # n = 511, 3 steps                  -> tolerance 1.735e-06
    ("pcg", "float32"): 8.496e-08,        # n = 511, 3 steps                  -> tolerance 1.359e-06
    ("bicgstab", "float32"): 1.326e-07,   # n = 3, 2 steps                    -> tolerance 2.121e-06
    ("pbicgstab", "float32"): 6.706e-07,  # n = 511, 2 steps                  -> tolerance 1.073e-05
    ("cgls", "float32"): 1.367e-07,       # n = 65, 2 steps                   -> tolerance 2.187e-06
}
STEPS = (1, 2, 3)


def tolerance(solver, dtype):
    return max(16.0 * MEASURED[(solver, np.dtype(dtype).name)], 4.0 * float(np.finfo(dtype).eps))


def rhs(n, dtype, seed):
    return np.random.default_rng([n, seed, 9]).uniform(-1, 1, n).astype(dtype)


def problem(solver, n, dtype):
    """(M, N, row_ptr, col, val rounded to dtype, b, minv in long double or None) of one solver at one size"""
    if solver in ("cg", "cg_multi", "pcg"):
        rp, col, val = sym_tridiagonal(n)
    elif solver in ("bicgstab", "pbicgstab"):
        rp, col, val = nonsym_tridiagonal(n)
    else:
        rp, col, val = rect_banded(n)
    val = val.astype(dtype)
    M = len(rp) - 1
    if solver == "cg_multi":
        b = np.ascontiguousarray(np.stack([rhs(M, dtype, 20 + j) for j in range(max(MCG_KS))], axis=1))
    else:
        b = rhs(M, dtype, 5)
    inv = stored_inverse(rp, col, val, dtype) if solver in ("pcg", "pbicgstab") else None
    return M, n, rp, col, val, b, inv


def cg_loop(A, b, iters):
    """cg_with; where its residual vanishes exactly (p.q = 0 at the next step: a division by zero in that loop) the
    iterate stays and the history repeats, which is what csr_cg documents (alpha = 0 when p.q = 0)"""
    for t in range(iters, -1, -1):
        try:
            x, h = cg_with(A, b, t)
        except ZeroDivisionError:
            continue
        return x, np.concatenate([h, np.full(iters - t, h[-1])])


def reference(solver, prob, iters, acc=LD, rd=None):
    """(x, the histories) after `iters` steps: the reference loops of the other solver tests over a product in `acc`
    (rd None), or the same recurrences with every stored vector rounded by rd (the handle's dtype)"""
    if rd is not None:
        return rounded_loop(solver, prob, iters, rd)
    M, N, rp, col, val, b, inv = prob
    A = product(rp, col, val, acc)
    minv = None if inv is None else (lambda r: np.asarray(r).astype(acc) * inv.astype(acc))
    if solver == "cg":
        x, h = cg_loop(A, b.astype(acc), iters)
        return x, [h]
    if solver == "cg_multi":
        out = [cg_loop(A, b[:, j].astype(acc), iters) for j in range(b.shape[1])]
        return np.stack([o[0] for o in out], axis=1), [np.stack([o[1] for o in out], axis=1)]
    if solver == "pcg":
        x, hrr, hrz, _ = pcg_ref(A, minv, b, iters)
        return x, [hrr, hrz]
    if solver == "bicgstab":
        x, h, _ = bicgstab_ref(A, b, iters)
        return x, [h]
    if solver == "pbicgstab":
        x, h, _ = pbicgstab_ref(A, minv, b, iters)
        return x, [h]
    AT = product(*transposed(M, N, rp, col, val), acc)
    x, ss, rr, _ = cgls_ref(A, AT, N, b, iters)
    return x, [ss, rr]


def rounded_loop(solver, prob, iters, rd):
    """The recurrences of the reference loops with every stored vector (products, preconditioned vectors and updates)
    rounded to the handle's dtype by rd and the dot products in fp64: what a solve in that dtype computes, up to the
    order of its sums.  A zero denominator ends the loop (the history repeats)."""
    M, N, rp, col, val, b, inv = prob
    A64 = product(rp, col, val, np.float64)
    A = lambda v: rd(A64(v))  # noqa: E731
    minv = (lambda r: r.copy()) if inv is None else (lambda r: rd(r * inv.astype(np.float64)))
    dot = lambda u, v: float(u @ v)  # noqa: E731
    pad = lambda h: np.array(h + [h[-1]] * (iters + 1 - len(h)))  # noqa: E731
    if solver == "cg_multi":
        out = [rounded_loop("cg", (M, N, rp, col, val, b[:, j], None), iters, rd) for j in range(b.shape[1])]
        return np.stack([o[0] for o in out], axis=1), [np.stack([o[1][0] for o in out], axis=1)]
    b = b.astype(np.float64)
    if solver in ("cg", "pcg"):
        x, r = np.zeros(M), b.copy()
        z = minv(r)
        p = z.copy()
        rz = dot(r, z)
        hrr, hrz = [dot(r, r)], [rz]
        for _ in range(iters):
            q = A(p)
            pq = dot(p, q)
            if pq == 0.0 or rz == 0.0:
                break
            alpha = rz / pq
            x, r = rd(x + alpha * p), rd(r - alpha * q)
            z = minv(r)
            rz_new = dot(r, z)
            hrr.append(dot(r, r))
            hrz.append(rz_new)
            p = rd(z + (rz_new / rz) * p)
            rz = rz_new
        return x, ([pad(hrr)] if solver == "cg" else [pad(hrr), pad(hrz)])
    if solver in ("bicgstab", "pbicgstab"):
        x, r, rh, p = np.zeros(M), b.copy(), b.copy(), b.copy()
        rho = dot(rh, r)
        hist = [dot(r, r)]
        for _ in range(iters):
            ph = minv(p)
            v = A(ph)
            rv = dot(rh, v)
            if rv == 0.0:
                break
            alpha = rho / rv
            s = rd(r - alpha * v)
            if dot(s, s) == 0.0:             # the half-step stop of tol = 0
                x = rd(x + alpha * ph)
                hist.append(0.0)
                break
            sh = minv(s)
            t = A(sh)
            ts, tt = dot(t, s), dot(t, t)
            if ts == 0.0 or tt == 0.0:
                break
            omega = ts / tt
            x, r = rd(x + (alpha * ph + omega * sh)), rd(s - omega * t)
            rho_new = dot(rh, r)
            hist.append(dot(r, r))
            if rho_new == 0.0:
                break
            p = rd(r + (rho_new / rho) * (alpha / omega) * (p - omega * v))
            rho = rho_new
        return x, [pad(hist)]
    AT64 = product(*transposed(M, N, rp, col, val), np.float64)
    x, r = np.zeros(N), b.copy()
    s = rd(AT64(r))
    p = s.copy()
    gamma = dot(s, s)
    ss, rr = [gamma], [dot(r, r)]
    for _ in range(iters):
        q = A(p)
        delta = dot(q, q)
        if delta == 0.0 or gamma == 0.0:
            break
        alpha = gamma / delta
        x, r = rd(x + alpha * p), rd(r - alpha * q)
        s = rd(AT64(r))
        g = dot(s, s)
        ss.append(g)
        rr.append(dot(r, r))
        p = rd(s + (g / gamma) * p)
        gamma = g
    return x, [pad(ss), pad(rr)]


def differences(got, ref):
    """(max |x - x_ref| / max |x_ref|, max over the histories of max |h - h_ref| / h_ref[0]), in long double"""
    (x, hists), (x_ref, hists_ref) = got, ref
    x_ref = np.asarray(x_ref).astype(LD)
    dx = float(np.max(np.abs(np.asarray(x).astype(LD) - x_ref)) / np.max(np.abs(x_ref)))
    dh = max(float(np.max(np.abs(h.astype(LD) - h_ref.astype(LD)) / np.abs(h_ref[0].astype(LD))))
             for h, h_ref in zip(hists, hists_ref))
    return dx, dh


def solve(solver, dev, at, P, b, iters):
    """(x, the histories) of one device solve"""
    if solver == "cg":
        x, h, _ = dev.cg(b, iters)
        return x, [h]
    if solver == "cg_multi":
        X, h, _, _ = dev.cg_multi(b, iters)
        return X, [h]
    if solver == "pcg":
        x, rr, rz, _, _ = dev.pcg(b, iters, precond=P)
        return x, [rr, rz]
    if solver in ("bicgstab", "pbicgstab"):
        x, h, _, _ = dev.bicgstab(b, iters, precond=P)
        return x, [h]
    x, ss, rr, _, _ = dev.cgls(b, iters, at=at)
    return x, [ss, rr]


def same_bits(one, two):
    return one[0].tobytes() == two[0].tobytes() and all(u.tobytes() == v.tobytes() for u, v in zip(one[1], two[1]))


def check_steps(oracle, solver, n, dtype):
    prob = problem(solver, n, dtype)
    M, N, rp, col, val, b, inv = prob
    tol = tolerance(solver, dtype)
    with sp.CsrDevice(M, N, rp, col, val) as dev:
        at = dev.transpose() if solver == "cgls" else None
        P = dev.preconditioner("jacobi") if inv is not None else None
        try:
            for k in (MCG_KS if solver == "cg_multi" else (None,)):
                bk = b if k is None else np.ascontiguousarray(b[:, :k])
                pk = prob if k is None else (M, N, rp, col, val, bk, inv)
                for iters in STEPS:
                    got = solve(solver, dev, at, P, bk, iters)
                    assert got[0].dtype == dtype and got[0].shape == ((N,) if k is None else (N, k))
                    dx, dh = differences(got, reference(solver, pk, iters))
                    print(f"{solver} n={n} {np.dtype(dtype).name} k={k} {iters} steps: x {dx:.3e} hist {dh:.3e} "
                          f"(tolerance {tol:.3e})")
                    assert dx <= tol and dh <= tol, (solver, n, k, iters, dx, dh, tol)
                assert same_bits(got, solve(solver, dev, at, P, bk, STEPS[-1])), (solver, n, k, "two calls")
            # the documented identities, and the recorded residual against the true one
            if solver == "cg":
                x, h, _ = dev.cg(b, 3)
                X, hm, _, _ = dev.cg_multi(b, 3)
                assert X[:, 0].tobytes() == x.tobytes() and hm[:, 0].tobytes() == h.tobytes(), (n, "cg_multi k = 1")
                xp, rr, rz, _, _ = dev.pcg(b, 3)
                assert xp.tobytes() == x.tobytes(), (n, "pcg without a preconditioner")
                assert rr.tobytes() == h.tobytes() and rz.tobytes() == rr.tobytes(), (n, rr, rz, h)
            if solver == "bicgstab":
                x, h, info, _ = dev.bicgstab(b, 3, precond=None)
                x2, h2, info2, _ = dev.bicgstab(b, 3)
                assert x.tobytes() == x2.tobytes() and h.tobytes() == h2.tobytes() and info == info2
            if solver in ("cg", "bicgstab"):
                # b - A x against the recurrence's r: each of the 3 steps rounds x, r and two products of values of
                # size at most |b| + |A| |x| <= 6 |b| (|A| <= 2.5, |A^-1| <= 2 by diagonal dominance): well within
                # 100 eps |b| in the 2-norm
                x, h = got[0], got[1][0]
                b64 = b.astype(np.float64)
                rr_true = true_rr(oracle, rp, col, val.astype(np.float64), b64, x)
                eps = float(np.finfo(dtype).eps)
                assert abs(math.sqrt(rr_true) - math.sqrt(h[-1])) <= 100.0 * eps * math.sqrt(h[0]), (n, rr_true, h[-1])
        finally:
            for obj in (P, at):
                if obj is not None:
                    obj.close()


SOLVERS = ["cg", "cg_multi", "pcg", "bicgstab", "pbicgstab", "cgls"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SMALL)
def test_one_two_and_three_steps_match_the_long_double_loop(gpu, oracle, n, dtype):
    """Every solver, 1, 2 and 3 steps with tol = 0 on a diagonally dominant tridiagonal matrix (nonsymmetric for
    BiCGSTAB, (n + 3) x n banded for CGLS; n < 3: diagonal) with b uniform in [-1, 1]: x and every history entry against
    the reference loops over a long-double product, within tolerance(); two calls give the same bits, cg_multi at k = 1
    and pcg without a preconditioner give cg's bits, bicgstab(precond=None) is the plain call.

    Measured reference rounding -> tolerance (MEASURED holds the size and step of each maximum):
        fp64  cg 7.3e-16 -> 1.2e-14   cg_multi 5.5e-16 -> 8.8e-15   pcg 3.3e-16 -> 5.3e-15
              bicgstab 3.5e-16 -> 5.6e-15   pbicgstab 8.6e-12 -> 1.4e-10   cgls 5.7e-16 -> 9.1e-15
        fp32  cg 9.3e-08 -> 1.5e-06   cg_multi 1.1e-07 -> 1.7e-06   pcg 8.5e-08 -> 1.4e-06
              bicgstab 1.3e-07 -> 2.1e-06   pbicgstab 6.7e-07 -> 1.1e-05   cgls 1.4e-07 -> 2.2e-06
    """
    for solver in SOLVERS:
        check_steps(oracle, solver, n, dtype)


def cap_cases():
    yield "cg", CG_EDGE
    yield "pcg", CG_EDGE
    yield "cg_multi", mcg_edge(np.float64)
    yield "bicgstab", bcg_edge(np.float64)
    yield "pbicgstab", bcg_edge(np.float64)
    yield "cgls", cgls_edge(np.float64)


@pytest.mark.parametrize("solver,n", list(cap_cases()), ids=lambda v: str(v))
def test_steps_at_the_grid_cap_fp64(gpu, oracle, solver, n):
    """The same one row past each solver's grid cap (fp64), where the stride loop makes its second trip."""
    check_steps(oracle, solver, n, np.float64)


# ---------------------------------------------------------------- the applies
def tri_apply_bound(Lf, Uf, n, kind, omega, order, r, dtype):
    """(z_ref in the solve order, the entry-wise bound fz, the order): long double substitution on the returned factors
    and the forward bound of test_gpu_trsv.test_apply_is_the_two_solves_on_the_returned_factors, term for term"""
    from scipy.sparse.linalg import spsolve_triangular
    Lm, Um, w, order = tri_parts(Lf, Uf, n, kind, omega, order)
    y = solve_ld(Lm, r[order], True)
    z_ref = solve_ld(Um, w * y, False)
    c = (max(int(np.max(np.diff(Lm.indptr))), int(np.max(np.diff(Um.indptr)))) + 4) * np.finfo(dtype).eps
    fy = spsolve_triangular(comparison(Lm), c * (abs(Lm) @ np.abs(y).astype(np.float64)), lower=True)
    fz = 1.1 * spsolve_triangular(comparison(Um), c * (abs(Um) @ np.abs(z_ref).astype(np.float64)) + np.abs(w) * fy,
                                  lower=False)
    return z_ref, fz, order


TRI_KINDS = [("ssor", 1.0, "natural"), ("ssor", 1.5, "multicolor"), ("ilu0", 1.0, "natural"),
             ("ilu0", 1.0, "multicolor")]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SMALL)
def test_applies_match_long_double_solves(gpu, n, dtype):
    """Jacobi is r times the rounded inverse bit for bit; block-Jacobi with blocks of 3 and 32 (n < block and a short
    last block both occur) agrees with per-block solves within test_gpu_precond.py's 1e-12 per block (fp64: the only
    dtype that bound is derived for); SSOR and ILU(0) in both orderings meet test_gpu_trsv.py's entry-wise bound
    against long double substitution on factors()."""
    rp, col, val = nonsym_tridiagonal(n)
    val = val.astype(dtype)
    r = rhs(n, dtype, 6)
    with sp.CsrDevice(n, n, rp, col, val) as dev:
        with dev.preconditioner("jacobi") as J:
            z = J.apply(r)
            inv = stored_inverse(rp, col, val, dtype).astype(np.float64)
            assert z.dtype == dtype and z.shape == (n,)
            assert z.tobytes() == (inv * r.astype(np.float64)).astype(dtype).tobytes()
        if dtype == np.float64:
            for blk in (3, 32):
                blocks = dense_blocks(rp, col, val, blk)
                z_ref = block_minv(blocks)(r)
                with dev.preconditioner("block_jacobi", blk) as P:
                    z = P.apply(r)
                assert z.dtype == dtype and z.shape == (n,)
                k0 = 0
                for d in blocks:
                    zr, zb = z_ref[k0:k0 + len(d)], z[k0:k0 + len(d)]
                    assert np.max(np.abs(zb - zr)) <= 1e-12 * np.max(np.abs(zr)), (n, blk, k0)
                    k0 += len(d)
        for kind, omega, ordering in TRI_KINDS:
            with dev.preconditioner(kind, omega=omega, ordering=ordering) as P:
                z = P.apply(r)
                Lf, Uf = P.factors()
                assert P.apply(r).tobytes() == z.tobytes()
            assert z.dtype == dtype and z.shape == (n,)
            z_ref, fz, order = tri_apply_bound(Lf, Uf, n, kind, omega, order_of(rp, col, val, ordering), r, dtype)
            err = np.abs(z[order].astype(LD) - z_ref).astype(np.float64)
            assert np.all(err <= fz), (n, kind, ordering, float(np.max(err / fz)))


SENTINEL = -777.0


def placed(n, dtype, shift):
    """element offsets of r and z in one buffer, each `shift` elements past a 16-byte boundary with at least one piece
    of sentinels on either side, and the buffer's length (a whole number of 8-byte words)"""
    v = piece(dtype)
    r_off = 2 * v + shift
    z_off = ((r_off + n + v) // v + 2) * v + shift
    total = (z_off + n + 2 * v + 1) // 2 * 2
    return r_off, z_off, total


def run_on_stream(call, n, dtype, r, shift, hip, stream):
    """call(d_r, d_z, stream) with r and z placed in one sentinel-filled device buffer -> (z, the buffer is otherwise
    unchanged)"""
    item = np.dtype(dtype).itemsize
    r_off, z_off, total = placed(n, dtype, shift)
    host = np.full(total, SENTINEL, dtype)
    host[r_off:r_off + n] = r
    with DeviceBuffer(total * item) as buf:
        buf.upload(host)
        assert (buf.at() + (r_off - shift) * item) % 16 == 0 and (buf.at() + (z_off - shift) * item) % 16 == 0
        call(buf.at(r_off * item), buf.at(z_off * item), stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        back = buf.download(total * item // 8).view(dtype)
    z = back[z_off:z_off + n].copy()
    back[z_off:z_off + n] = SENTINEL
    untouched = back.tobytes() == host.tobytes()
    return z, untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", [5, 257, 1025])
def test_apply_on_and_solve_on_at_element_aligned_addresses(gpu, n, dtype):
    """Preconditioner.apply_on and TriangularSolver.solve_on on a second stream with r / b and z / x inside one larger
    device buffer, at a 16-byte boundary and one element past it: both give apply's / solve's bits and change nothing
    around z / x; an address that is not a multiple of the element size is refused and the object keeps working."""
    import ctypes as C
    rp, col, val = nonsym_tridiagonal(n)
    val = val.astype(dtype)
    r = rhs(n, dtype, 7)
    item = np.dtype(dtype).itemsize
    hip = _hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        with sp.CsrDevice(n, n, rp, col, val) as dev:
            makers = [lambda: dev.preconditioner("jacobi"), lambda: dev.preconditioner("block_jacobi", 3),
                      lambda: dev.preconditioner("block_jacobi", 32), lambda: dev.preconditioner("ssor", omega=1.5),
                      lambda: dev.preconditioner("ilu0", ordering="multicolor"),
                      lambda: dev.triangular(lower=True), lambda: dev.triangular(lower=False, unit_diagonal=True)]
            for make in makers:
                with make() as obj:
                    tri = isinstance(obj, sp.TriangularSolver)
                    host_call, on = (obj.solve, obj.solve_on) if tri else (obj.apply, obj.apply_on)
                    z_host = host_call(r)
                    for shift in (0, 1):
                        z, untouched = run_on_stream(on, n, dtype, r, shift, hip, stream)
                        assert z.tobytes() == z_host.tobytes(), (type(obj).__name__, n, shift)
                        assert untouched, (type(obj).__name__, n, shift, "wrote outside z")
                    with DeviceBuffer(2 * (n + 4) * item) as buf:
                        d_r, d_z = buf.at(), buf.at((n + 4) * item)
                        for bad_r, bad_z in ((d_r + item // 2, d_z), (d_r, d_z + item // 2)):
                            with pytest.raises(sp.SpmvHipError, match=f"must be aligned to {item} bytes"):
                                on(bad_r, bad_z, stream.value)
                    assert host_call(r).tobytes() == z_host.tobytes()
    finally:
        hip.hipStreamDestroy(stream)


# ---------------------------------------------------------------- the CPU measurement behind MEASURED
def measure():
    worst = {}
    for dtype in DTYPES:
        rd = lambda v, t=dtype: np.asarray(v).astype(t).astype(np.float64)  # noqa: E731
        cases = [(s, n) for s in SOLVERS for n in SMALL] + (list(cap_cases()) if dtype == np.float64 else [])
        for solver, n in cases:
            prob = problem(solver, n, dtype)
            for iters in STEPS:
                dx, dh = differences(reference(solver, prob, iters, rd=rd), reference(solver, prob, iters))
                key = (solver, np.dtype(dtype).name)
                if max(dx, dh) > worst.get(key, (0.0,))[0]:
                    worst[key] = (max(dx, dh), n, iters, dx, dh)
    for key, (w, n, iters, dx, dh) in worst.items():
        print(f"    {key!r}: {w:.3e},   # n = {n}, {iters} steps (x {dx:.3e}, history {dh:.3e}); "
              f"tolerance {max(16 * w, 4 * float(np.finfo(key[1]).eps)):.3e}")


if __name__ == "__main__":
    measure()
