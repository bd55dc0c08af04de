"""The Chebyshev polynomial preconditioner restated in numpy (include/spmv_hip.h): the coefficient loop, the Gershgorin
bound, the apply with every stored vector rounded to the handle's dtype, and the same apply in fp64 with an entry-wise
running error bound.  test_cheb_host.py holds the host side against it, test_gpu_chebyshev.py the device."""
import numpy as np
import scipy.sparse as sps

import _amg_ref

RATIO = 30.0


def coefficients(degree, lmin, lmax):
    """(a, b) of the loop, every line one rounded fp64 operation in the order written"""
    lmin, lmax = np.float64(lmin), np.float64(lmax)
    theta = (lmax + lmin) / np.float64(2.0)
    delta = (lmax - lmin) / np.float64(2.0)
    sigma = theta / delta
    rho = np.float64(1.0) / sigma
    a, b = np.zeros(degree), np.zeros(degree)
    b[0] = np.float64(1.0) / theta
    for j in range(1, degree):
        nxt = np.float64(1.0) / (np.float64(2.0) * sigma - rho)
        a[j] = nxt * rho
        b[j] = (np.float64(2.0) * nxt) / delta
        rho = nxt
    return a, b


def gershgorin(a):
    """max_i (sum_j |a_ij|) / a_ii of a canonical fp64 matrix, every row's sum in stored order"""
    a = sps.csr_matrix(a)
    n = a.shape[0]
    length = np.diff(a.indptr)
    total = np.zeros(n)
    for p in range(int(length.max()) if n else 0):
        rows = np.nonzero(length > p)[0]
        total[rows] = total[rows] + np.abs(a.data[a.indptr[rows] + p])
    return float(np.max(total / a.diagonal()))


def interval(a, lmax=None, lmin=None, ratio=RATIO):
    """(lmin, lmax) as the build picks them"""
    lmax = gershgorin(a) if lmax is None else float(lmax)
    return (lmax / ratio if lmin is None else float(lmin)), lmax


def inverse_diagonal(a, dtype):
    """g = T(1 / a_ii) as fp64 values"""
    return (1.0 / sps.csr_matrix(a).diagonal()).astype(dtype).astype(np.float64)


def apply(a, g, r, degree, lmin, lmax, dtype=np.float64):
    """z = p(D^-1 A) D^-1 r for r of n values or n x k; every stored vector rounded once to dtype"""
    ca, cb = coefficients(degree, lmin, lmax)
    rnd = lambda v: np.asarray(v, dtype=np.float64).astype(dtype).astype(np.float64)  # noqa: E731
    r = np.asarray(r, dtype=np.float64)
    gg = g[:, None] if r.ndim == 2 else g
    d = rnd(cb[0] * (gg * r))
    z = d
    for j in range(1, degree):
        q = rnd(a @ z)
        d = rnd(ca[j] * d + cb[j] * (gg * (r - q)))
        z = rnd(z + d)
    return z


def apply_with_bound(a, g, r, degree, lmin, lmax, dtype):
    """(z, bound): the apply in fp64 without the roundings and a bound on |device - z| entry by entry, built as
    _amg_ref.cycle_with_bound builds its own.  Every pass out = f(inputs) adds to its inputs' bounds, carried through
    the pass on absolute values, its own rounding: the pass evaluated on absolute values times (2 ka + 6) eps for the
    product (ka = A's longest row: ka products and ka additions in double, the store to dtype, and as much again for
    this restatement) and 6 eps for a vector pass (its few operations in double and the store, and as much again)."""
    eps = float(np.finfo(dtype).eps)
    ca, cb = coefficients(degree, lmin, lmax)
    r = np.asarray(r, dtype=np.float64)
    gg = g[:, None] if r.ndim == 2 else g
    aa = abs(sps.csr_matrix(a))
    ka = _amg_ref.longest(a)
    d = cb[0] * (gg * r)
    ed = 6 * eps * np.abs(d)
    z, ez = d, ed
    for j in range(1, degree):
        q = a @ z
        absq = aa @ (np.abs(z) + ez)
        eq = aa @ ez + (2 * ka + 6) * eps * absq
        absd = abs(ca[j]) * (np.abs(d) + ed) + abs(cb[j]) * (gg * (np.abs(r) + absq + eq))
        d, ed = ca[j] * d + cb[j] * (gg * (r - q)), abs(ca[j]) * ed + abs(cb[j]) * (gg * eq) + 6 * eps * absd
        z, ez = z + d, ez + ed + 6 * eps * (np.abs(z) + ez + np.abs(d) + ed)
    return z, ez


def residual_polynomial(t, degree, lmin, lmax):
    """1 - t p(t) by the restatement on the 1 x 1 matrix [t] with unit diagonal scaling (g = 1, r = 1)"""
    one = np.ones(1)
    return 1.0 - t * apply(sps.csr_matrix(np.array([[t]])), one, one, degree, lmin, lmax)[0]


def chebyshev_t(m, x):
    """T_m(x) by the three-term recurrence"""
    t0, t1 = 1.0, x
    if m == 0:
        return t0
    for _ in range(m - 1):
        t0, t1 = t1, 2.0 * x * t1 - t0
    return t1


def pcg_steps(a, b, degree, tol, lmax=None, lmin=None, ratio=RATIO, maxit=5000):
    """steps of _amg_ref.pcg_steps with the polynomial of `degree` (0: Jacobi) as the preconditioner"""
    g = inverse_diagonal(a, np.float64)
    lo, hi = interval(a, lmax, lmin, ratio)
    prec = (lambda r: g * r) if degree == 0 else (lambda r: apply(a, g, r, degree, lo, hi))
    return _amg_ref.pcg_steps(a, b, prec, tol, maxit)[0]
