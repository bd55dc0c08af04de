"""spmv_hip_csr_minres on the GPU: MINRES for a symmetric indefinite A against a numpy loop of exactly the documented
algorithm (include/spmv_hip.h) over the oracle's serial product.

Lanczos amplifies rounding differences exponentially, so x and the history are compared entry by entry with the
reference only after a few steps (5 and 10 on the banded matrix, 1 to 3 at the edge sizes); longer runs are held to
properties: the status, the step count within 2 of the reference's, a history that never grows, the true residual
against the recorded one, the distance to x_true.

The pointwise tolerances are 16 times the reference's own rounding, and at least 4 eps of the dtype (the convention of
tolerance() in test_gpu_solver_sizes.py).  The reference's rounding is measured on the CPU by
`python tests/test_gpu_minres.py`: the largest difference (x relative to max |x|, history entries relative to the first)
between the reference loop as the handle computes it (fp64: over oracle.csr_serial; fp32: values, b and every stored
vector rounded to fp32, dots in fp64) and the same loop over a long-double product:

    case                                               measured     tolerance
    banded n = 6000, fp64, 5 steps                     1.060e-15    1.696e-14
    banded n = 6000, fp64, 10 steps                    1.021e-13    1.634e-12
    banded n = 6000, fp64, 5 steps, shift 0.3          7.011e-16    1.122e-14
    banded n = 6000, fp64, 5 steps, M = |diag A|       3.679e-16    5.886e-15
    banded n = 6000, fp32, 6 steps                     1.500e-07    2.400e-06
    tridiagonal, all sizes, 1 to 3 steps, fp64         3.958e-13    6.333e-12   (n = 256, 1 step)
    tridiagonal, all sizes, 1 to 3 steps, fp32         1.543e-05    2.469e-04   (n = 256, 1 step)
The edge-size maxima are large for one step because x_1 is proportional to alfa = v.A v, a sum that nearly cancels on
a matrix whose diagonal signs alternate; the reference itself is no more exact than that there.

The banded matrix (seed 909) on the CPU: 3000 eigenvalues of each sign, |lambda| in [0.49, 17.4]; the reference's
hist[40] equals the true ||b - A x||^2 to 6.7e-15; its history never grows; it reaches tol = 1e-10 in 251 steps (178
with M = |diag A|, 284 with shift = 0.3) and agrees with scipy's minres to 3.2e-7; textbook CG meets p.q <= 0 at
step 1.
"""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from sparsematrixvectormultiplication_amd import synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = [np.float64, np.float32]
K_BLOCK, K_MR_BLOCKS = 256, 2048   # kBlock: csr_kernels.hpp; kMrBlocks: minres_kernels.hpp


def minres_ref(spmv, b, iters, tol=0.0, shift=0.0, minv=None, rd=None):
    """The loop spmv_hip_csr_minres runs (include/spmv_hip.h) with a given product and M^-1 apply (None: no
    preconditioner), scalars in fp64; rd (optional) rounds every stored vector, as a handle of that dtype does.
    Returns (x, history [iters + 1], info)."""
    rd = rd or (lambda u: u)
    fin = np.isfinite
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r1 = b.copy()
    r2 = b.copy()
    y = rd(minv(r2)) if minv else r2
    with np.errstate(all="ignore"):
        bb0 = float(r2 @ y)
        if not fin(bb0) or bb0 < 0.0:
            return x, np.full(iters + 1, bb0), {"steps": 0, "status": sp.MINRES_BREAKDOWN}
        if bb0 == 0.0:
            return x, np.full(iters + 1, bb0), {"steps": 0, "status": sp.MINRES_CONVERGED}
        beta = float(np.sqrt(bb0))
        phibar = beta
        oldb = dbar = epsln = 0.0
        cs, sn = -1.0, 0.0
        w = np.zeros_like(b)
        w2 = np.zeros_like(b)
        hist = [bb0]
        info = {"steps": iters, "status": sp.MINRES_RAN_ALL}
        tol2 = tol * tol
        for k in range(1, iters + 1):
            v = rd(y / beta)
            t = spmv(v) - shift * v
            if k >= 2:
                t = t - (beta / oldb) * r1
            t = rd(t)
            alfa = float(v @ t)
            c2 = alfa / beta
            if not (fin(alfa) and fin(c2)):
                info.update(steps=k - 1, status=sp.MINRES_BREAKDOWN)
                break
            t = rd(t - c2 * r2)
            r1, r2 = r2, t
            y = rd(minv(r2)) if minv else r2
            bb = float(r2 @ y)
            new_beta = float(np.sqrt(bb))
            oldeps = epsln
            delta = cs * dbar + sn * alfa
            gbar = sn * dbar - cs * alfa
            new_epsln = sn * new_beta
            new_dbar = -cs * new_beta
            gamma = float(np.sqrt(gbar * gbar + new_beta * new_beta))
            new_cs, new_sn = (gbar / gamma, new_beta / gamma) if gamma != 0.0 else (np.nan, np.nan)
            phi, new_phibar = new_cs * phibar, new_sn * phibar
            c1, rr = new_beta / beta, new_phibar * new_phibar
            if not bb >= 0.0 or gamma == 0.0 or not all(fin(s) for s in (bb, delta, new_epsln, new_dbar, gamma, phi,
                                                                          new_phibar, c1, rr)):
                info.update(steps=k - 1, status=sp.MINRES_BREAKDOWN)
                break
            oldb, beta, epsln, dbar, cs, sn, phibar = beta, new_beta, new_epsln, new_dbar, new_cs, new_sn, new_phibar
            w1, w2 = w2, w
            w = rd(((v - oldeps * w1) - delta * w2) / gamma)
            x = rd(x + phi * w)
            hist.append(rr)
            if rr <= tol2 * bb0:
                info.update(steps=k, status=sp.MINRES_CONVERGED)
                break
    hist += [hist[-1]] * (iters + 1 - len(hist))
    return x, np.array(hist, dtype=np.float64), info


def cg_breaks_down_at(spmv, b, iters):
    """The step at which textbook CG from x0 = 0 meets p.q <= 0 (None: it does not within iters)"""
    r = np.asarray(b, dtype=np.float64).copy()
    p = r.copy()
    rr = float(r @ r)
    for k in range(1, iters + 1):
        q = spmv(p)
        pq = float(p @ q)
        if pq <= 0.0:
            return k
        alpha = rr / pq
        r = r - alpha * q
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
    return None


# ---------------------------------------------------------------- matrices
def to_csr(a):
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data, dtype=np.float64)


def sym_indefinite_banded(rng, n, per_row, band):
    """per_row draws per row in a band of +-band, the strict upper triangle kept and symmetrised, diagonal
    +-(0.5 sum |a_ij| + 1) with the sign drawn per row: symmetric and indefinite"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-band, band + 1, len(r)), 0, n - 1)
    a = sps.csr_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n))
    u = sps.triu(a, 1)
    s = (u + u.T).tocsr()
    sign = rng.choice([-1.0, 1.0], n)
    return to_csr(s + sps.diags(sign * (0.5 * np.asarray(abs(s).sum(axis=1)).ravel() + 1.0)))


def spd_banded(rng, n, per_row, band):
    """the spd_banded shape of test_gpu_pcg_multi.py: symmetric, strictly diagonally dominant"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-band, band + 1, len(r)), 0, n - 1)
    b = sps.csr_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n))
    a = b + b.T
    return to_csr(a + sps.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0))


def alternating_tridiagonal(n):
    """symmetric, diagonally dominant, indefinite: diagonal (-1)^i d_i with d_i uniform in [1, 2], off-diagonal
    entries +-1/4 (n < 3: the diagonal alone)"""
    import scipy.sparse as sps
    rng = np.random.default_rng([n, 11])
    d = rng.uniform(1.0, 2.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    if n < 3:
        return to_csr(sps.diags(d))
    off = 0.25 * rng.choice([-1.0, 1.0], n - 1)
    return to_csr(sps.diags([off, d, off], [-1, 0, 1]))


def diagonal_positions(row_ptr, col):
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    return np.flatnonzero(col == rows)


def product(rp, col, val, acc=LD):
    """v -> A v with the products and each row's sum (entry order) in `acc` (every row has an entry)"""
    vals = np.asarray(val).astype(acc)
    return lambda v: np.add.reduceat(vals * np.asarray(v).astype(acc)[col], rp[:-1])


def differences(got, ref):
    """(max |x - x_ref| / max |x_ref|, max |h - h_ref| / h_ref[0]) in long double"""
    (x, h), (x_ref, h_ref) = got, ref
    x_ref, h_ref = np.asarray(x_ref).astype(LD), np.asarray(h_ref).astype(LD)
    scale = np.max(np.abs(x_ref))
    dx = float(np.max(np.abs(np.asarray(x).astype(LD) - x_ref)) / scale) if scale > 0 else 0.0
    dh = float(np.max(np.abs(np.asarray(h).astype(LD) - h_ref)) / np.abs(h_ref[0]))
    return dx, dh


def true_rr(oracle, row_ptr, col, val, b, x, shift=0.0):
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(b, dtype=np.float64) - (oracle.csr_serial(row_ptr, col, val, x) - shift * x)
    return float(r @ r)


# Measured on the CPU (`python tests/test_gpu_minres.py`): the reference's own rounding per case, see the module
# docstring; the tolerance is 16 times it and at least 4 eps.
MEASURED = {
    ("banded", "float64", 5): 1.060e-15,    # x 1.060e-15, history 4.477e-17
    ("banded", "float64", 10): 1.021e-13,   # x 1.021e-13, history 5.037e-17
    ("shift", "float64", 5): 7.011e-16,     # x 7.011e-16, history 4.477e-17
    ("jacobi", "float64", 5): 3.679e-16,    # x 3.679e-16, history 0
    ("banded", "float32", 6): 1.500e-07,    # x 1.500e-07, history 9.107e-09
    ("sizes", "float64"): 3.958e-13,        # n = 256, 1 step, x 3.958e-13, history 0
    ("sizes", "float32"): 1.543e-05,        # n = 256, 1 step, x 1.543e-05, history 1.624e-12
}


def tolerance(*key):
    return max(16.0 * MEASURED[key], 4.0 * float(np.finfo(key[1]).eps))


N = 6000
SHIFT = 0.3
SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025]
STEPS = (1, 2, 3)


def banded_problem(oracle):
    rng = np.random.default_rng(909)
    row_ptr, col, val = sym_indefinite_banded(rng, N, 7, 60)
    x_true = rng.uniform(-1, 1, N)
    b = oracle.csr_serial(row_ptr, col, val, x_true)
    return row_ptr, col, val, x_true, b


@pytest.fixture(scope="module")
def banded(oracle):
    return banded_problem(oracle)


@pytest.fixture(scope="module")
def refs(oracle, banded):
    """The reference runs several tests share, computed once: name -> (x, hist, info)"""
    row_ptr, col, val, _, b = banded
    spmv = lambda v: oracle.csr_serial(row_ptr, col, val, v)  # noqa: E731
    inv = abs_jacobi_inverse(row_ptr, col, val)
    minv = lambda r: r * inv  # noqa: E731
    out = {("plain", k): minres_ref(spmv, b, k) for k in (5, 6, 10)}
    out["plain", "tol"] = minres_ref(spmv, b, 400, tol=1e-10)
    out["shift", 5] = minres_ref(spmv, b, 5, shift=SHIFT)
    out["shift", "tol"] = minres_ref(spmv, b, 500, tol=1e-10, shift=SHIFT)
    out["jacobi", 5] = minres_ref(spmv, b, 5, minv=minv)
    out["jacobi", "tol"] = minres_ref(spmv, b, 400, tol=1e-10, minv=minv)
    return out


def abs_jacobi_inverse(row_ptr, col, val):
    """Jacobi's stored values for the copy of the matrix with |diagonal|: 1.0 / |d|"""
    return 1.0 / np.abs(val[diagonal_positions(row_ptr, col)])


def with_abs_diagonal(row_ptr, col, val):
    out = val.copy()
    pos = diagonal_positions(row_ptr, col)
    out[pos] = np.abs(out[pos])
    return out


def check_pointwise(got, ref, tol, what, with_info=True):
    x, h, info = got
    x_ref, h_ref, info_ref = ref
    assert not with_info or info == info_ref, (what, info, info_ref)
    dx, dh = differences((x, h), (x_ref, h_ref))
    print(f"{what}: x {dx:.3e} hist {dh:.3e} (tolerance {tol:.3e})")
    assert dx <= tol and dh <= tol, (what, dx, dh, tol)


# ---------------------------------------------------------------- the banded indefinite matrix
def test_minres_matches_the_reference_loop_fp64(gpu, banded, refs):
    row_ptr, col, val, _, b = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        for k in (5, 10):
            x, h, info, ms = dev.minres(b, k)
            assert x.dtype == np.float64 and h.shape == (k + 1,) and ms > 0
            assert info == {"steps": k, "status": sp.MINRES_RAN_ALL}
            check_pointwise((x, h, info), refs["plain", k], tolerance("banded", "float64", k), f"{k} steps")
            assert abs(h[0] - refs["plain", k][1][0]) <= 1e-13 * refs["plain", k][1][0]
        # another product than AUTO's plan: the same loop
        xw, hw, infow, _ = dev.minres(b, 5, variant=sp.CSR_WAVE_ROW)
        check_pointwise((xw, hw, infow), refs["plain", 5], tolerance("banded", "float64", 5), "wave_row, 5 steps")


def test_minres_converges_where_cg_breaks_down(gpu, oracle, banded, refs):
    """tol = 1e-10 on the indefinite matrix; on the same handle pcg stops with PCG_BREAKDOWN (the CPU loop meets
    p.q <= 0 at step 1: b.A b < 0): the reason for the solver."""
    row_ptr, col, val, x_true, b = banded
    _, h_ref, info_ref = refs["plain", "tol"]
    assert info_ref["status"] == sp.MINRES_CONVERGED
    assert cg_breaks_down_at(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, 50) == 1
    iters, tol = 400, 1e-10
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x, h, info, _ = dev.minres(b, iters, tol=tol)
        t = info["steps"]
        assert info["status"] == sp.MINRES_CONVERGED and abs(t - info_ref["steps"]) <= 2, (info, info_ref)
        assert np.all(np.diff(h) <= 0.0)
        assert h[t] <= tol * tol * h[0] and np.all(h[1:t] > tol * tol * h[0])
        assert np.all(h[t:] == h[t])                                      # the history repeats after the stop
        rr = true_rr(oracle, row_ptr, col, val, b, x)
        assert rr <= 4.0 * h[-1] + 1e-24 * h[0], (rr, h[-1], h[0])
        assert np.max(np.abs(x - x_true)) <= 1e-8 * np.max(np.abs(x_true))
        # tol = 0 over a longer budget: the stop only at exactly 0, the same iterates up to step t
        x0, h0, info0, _ = dev.minres(b, t)
        assert info0 == {"steps": t, "status": sp.MINRES_RAN_ALL}
        assert h0.tobytes() == h[: t + 1].tobytes() and x0.tobytes() == x.tobytes()
        _, _, _, info_cg, _ = dev.pcg(b, 50)
        assert info_cg["status"] == sp.PCG_BREAKDOWN, info_cg


def test_minres_fp32_handle(gpu, banded, refs):
    row_ptr, col, val, _, b = banded
    x_ref, h_ref, _ = refs["plain", 6]
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        x, h, info, _ = dev32.minres(b.astype(np.float32), 6)
    assert x.dtype == np.float32 and info == {"steps": 6, "status": sp.MINRES_RAN_ALL}
    assert np.all(np.isfinite(x))
    check_pointwise((x, h, info), refs["plain", 6], tolerance("banded", "float32", 6), "fp32, 6 steps")
    assert abs(h[0] - h_ref[0]) <= 1e-6 * h_ref[0]


def test_minres_is_bit_reproducible(gpu, banded):
    row_ptr, col, val, _, b = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x1, h1, i1, _ = dev.minres(b, 25)
        x2, h2, i2, _ = dev.minres(b, 25)
    assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes() and i1 == i2
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
        b32 = b.astype(np.float32)
        x1, h1, _, _ = dev32.minres(b32, 12)
        x2, h2, _, _ = dev32.minres(b32, 12)
    assert x1.tobytes() == x2.tobytes() and h1.tobytes() == h2.tobytes()


def test_minres_single_rank_communicator_gives_the_same_bits(gpu, banded):
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, _, b = banded
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        plain = dev.minres(b, 25)
        plain_tol = dev.minres(b, 400, tol=1e-10)
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            bounds = np.array([0, N], np.int32)
            x, h, info, _ = dev.minres(b, 25, bounds=bounds)
            assert x.tobytes() == plain[0].tobytes() and h.tobytes() == plain[1].tobytes() and info == plain[2]
            x, h, info, _ = dev.minres(b, 400, tol=1e-10, bounds=bounds)
            assert x.tobytes() == plain_tol[0].tobytes() and h.tobytes() == plain_tol[1].tobytes()
            assert info == plain_tol[2]
            with pytest.raises(RuntimeError, match="bounds"):
                dev.minres(b, 2)                                            # a communicator needs the row bounds
        finally:
            comm.close()


def test_minres_shift(gpu, oracle, banded, refs):
    row_ptr, col, val, _, b = banded
    _, _, info_ref = refs["shift", "tol"]
    assert info_ref["status"] == sp.MINRES_CONVERGED
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        x, h, info, _ = dev.minres(b, 5, shift=SHIFT)
        check_pointwise((x, h, info), refs["shift", 5], tolerance("shift", "float64", 5), "shift, 5 steps")
        x, h, info, _ = dev.minres(b, 500, tol=1e-10, shift=SHIFT)
        assert info["status"] == sp.MINRES_CONVERGED and abs(info["steps"] - info_ref["steps"]) <= 2, (info, info_ref)
        assert np.all(np.diff(h) <= 0.0)
        rr = true_rr(oracle, row_ptr, col, val, b, x, shift=SHIFT)          # against A - 0.3 I
        assert rr <= 4.0 * h[-1] + 1e-24 * h[0], (rr, h[-1], h[0])


def test_minres_jacobi_of_the_absolute_diagonal(gpu, oracle, banded, refs):
    """M = |diag A| (SPD), taken from a copy of the matrix with |diagonal|: 5 steps against the reference with minv,
    fewer steps to tol = 1e-10 than the plain run.  The Jacobi preconditioner of the indefinite matrix itself has
    negative entries: MINRES_BREAKDOWN, x finite.  precond=None is the plain call."""
    row_ptr, col, val, _, b = banded
    inv = abs_jacobi_inverse(row_ptr, col, val)
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        with sp.CsrDevice(N, N, row_ptr, col, with_abs_diagonal(row_ptr, col, val)) as dev_abs:
            J = dev_abs.preconditioner("jacobi")
        with J:
            assert J.apply(b).tobytes() == (b * inv).tobytes()
            x, h, info, _ = dev.minres(b, 5, precond=J)
            check_pointwise((x, h, info), refs["jacobi", 5], tolerance("jacobi", "float64", 5), "Jacobi, 5 steps")
            x, h, info, _ = dev.minres(b, 400, tol=1e-10, precond=J)
            plain = dev.minres(b, 400, tol=1e-10)
            assert info["status"] == sp.MINRES_CONVERGED and plain[2]["status"] == sp.MINRES_CONVERGED
            assert info["steps"] < plain[2]["steps"], (info, plain[2])
            assert abs(info["steps"] - refs["jacobi", "tol"][2]["steps"]) <= 2
            assert np.all(np.diff(h) <= 0.0)
            r = b - oracle.csr_serial(row_ptr, col, val, x)                 # the history is r.M^-1 r
            rmr = float(r @ (r * inv))
            assert rmr <= 4.0 * h[-1] + 1e-24 * h[0], (rmr, h[-1], h[0])
        with dev.preconditioner("jacobi") as bad:                           # 1 / d with d of both signs
            x, h, info, _ = dev.minres(b, 20, precond=bad)
            assert info["status"] == sp.MINRES_BREAKDOWN, info
            assert np.all(np.isfinite(x))
            x_ref, h_ref, info_ref = minres_ref(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, 20,
                                                minv=lambda r: r / val[diagonal_positions(row_ptr, col)])
            assert info == info_ref, (info, info_ref)
        a = dev.minres(b, 7, precond=None)
        c = dev.minres(b, 7)
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes() and a[2] == c[2]


@pytest.mark.parametrize("kind", ["block_jacobi", "ssor", "ilu0", "fsai"])
def test_minres_preconditioned_on_an_spd_matrix(gpu, oracle, kind):
    """Block-Jacobi(3), SSOR, ILU(0) and FSAI on an SPD banded matrix: each converges to tol = 1e-8 in no more steps
    than the plain run, and the true residual in the norm the history records (r.M^-1 r, through the
    preconditioner's own apply) meets the bound of the plain runs."""
    n = 4000
    rng = np.random.default_rng(31)
    row_ptr, col, val = spd_banded(rng, n, 5, 40)
    b = oracle.csr_serial(row_ptr, col, val, rng.uniform(-1, 1, n))
    tol = 1e-8
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev:
        xp, hp, infop, _ = dev.minres(b, 200, tol=tol)
        assert infop["status"] == sp.MINRES_CONVERGED
        rr = true_rr(oracle, row_ptr, col, val, b, xp)
        assert rr <= 4.0 * hp[-1] + 1e-24 * hp[0], (rr, hp[-1], hp[0])
        P = dev.preconditioner("block_jacobi", 3) if kind == "block_jacobi" else dev.preconditioner(kind)
        with P:
            x, h, info, _ = dev.minres(b, 200, tol=tol, precond=P)
            assert info["status"] == sp.MINRES_CONVERGED and info["steps"] <= infop["steps"], (kind, info, infop)
            assert np.all(np.diff(h) <= 0.0) and h[-1] <= tol * tol * h[0]
            r = b - oracle.csr_serial(row_ptr, col, val, x)
            rmr = float(r @ P.apply(r))
            assert rmr <= 4.0 * h[-1] + 1e-24 * h[0], (kind, rmr, h[-1], h[0])
            assert np.max(np.abs(x - xp)) <= 1e-6 * np.max(np.abs(xp))


# ---------------------------------------------------------------- sizes
def sizes_problem(n, dtype):
    rp, col, val = alternating_tridiagonal(n)
    val = val.astype(dtype)
    b = np.random.default_rng([n, 12]).uniform(-1, 1, n).astype(dtype)
    return rp, col, val, b


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_minres_one_two_and_three_steps_at_the_edge_sizes(gpu, n, dtype):
    """1, 2 and 3 steps on an indefinite tridiagonal matrix (n < 3: diagonal) against the reference over a long-double
    product.  x and the history are compared, not the status: where the Krylov space is exhausted (n <= 3) the last
    residual is 0 in one order of rounding and 1e-33 in another, and tol = 0 converges only at exactly 0.
    n = 1 with |b| a power of two: every operation but the one division is exact, so x = b / a exactly after one step,
    the history ends at 0 and the step converges."""
    rp, col, val, b = sizes_problem(n, dtype)
    A = product(rp, col, val)
    tol = tolerance("sizes", np.dtype(dtype).name)
    with sp.CsrDevice(n, n, rp, col, val) as dev:
        for iters in STEPS:
            x, h, info, _ = dev.minres(b, iters)
            assert x.dtype == dtype and x.shape == (n,) and h.shape == (iters + 1,)
            x_ref, h_ref, info_ref = minres_ref(A, b, iters)
            check_pointwise((x, h, info), (x_ref, h_ref, info_ref), tol, f"n={n} {np.dtype(dtype).name} {iters} steps",
                            with_info=False)
            assert info["steps"] == iters or info["status"] == sp.MINRES_CONVERGED, info
        if n == 1:
            b1 = np.array([-0.5], dtype=dtype)
            x, h, info, _ = dev.minres(b1, 1)
            assert x[0] == b1[0] / val[0] and h[1] == 0.0 and info == {"steps": 1, "status": sp.MINRES_CONVERGED}


def cap_problem(dtype):
    """(n, d, b): a diagonal matrix of alternating signs, three rows past the grid cap's kMrBlocks x kBlock pieces"""
    n = K_MR_BLOCKS * K_BLOCK * (16 // np.dtype(dtype).itemsize) + 3
    d = (np.random.default_rng(13).uniform(1.0, 2.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)).astype(dtype)
    return n, d, np.random.default_rng(14).uniform(-1, 1, n).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_minres_past_the_grid_cap(gpu, dtype):
    """n = 2048 x 256 x V + 3 rows of a diagonal matrix, 2 steps: the lanes' stride loop makes its second trip"""
    n, d, b = cap_problem(dtype)
    rp, col = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    dl = d.astype(LD)
    with sp.CsrDevice(n, n, rp, col, d) as dev:
        x, h, info, _ = dev.minres(b, 2)
    ref = minres_ref(lambda u: dl * np.asarray(u).astype(LD), b, 2)
    check_pointwise((x, h, info), ref, tolerance("sizes", np.dtype(dtype).name), f"n={n} {np.dtype(dtype).name}")


# ---------------------------------------------------------------- stops and breakdowns
def test_minres_stops_and_breakdowns(gpu):
    import scipy.sparse as sps
    d = np.tile([2.0, -1.0, 0.5], 10)
    rp, col, val = to_csr(sps.diags(d))
    n = len(d)
    with sp.CsrDevice(n, n, rp, col, val) as dev:
        x, h, info, _ = dev.minres(np.zeros(n), 4)                          # b = 0: converged at step 0
        assert info == {"steps": 0, "status": sp.MINRES_CONVERGED}
        assert np.all(x == 0.0) and np.all(h == 0.0)
        b = np.ones(n)
        b[7] = np.nan
        for tol in (0.0, 1e-3):
            x, h, info, _ = dev.minres(b, 6, tol=tol)
            assert info == {"steps": 0, "status": sp.MINRES_BREAKDOWN}
            assert not np.any(np.isnan(x)) and np.all(x == 0.0)
        b = np.ones(n)                                                      # three distinct eigenvalues: three steps
        x, h, info, _ = dev.minres(b, 3)
        assert h[3] <= 1e-24 * h[0], h
        assert np.max(np.abs(x - b / d)) <= 1e-14 * np.max(np.abs(b / d))
        assert np.all(np.diff(h) <= 0.0)
        x8, h8, info8, _ = dev.minres(b, 8, tol=1e-9)                       # stops at step 3; the history repeats
        assert info8 == {"steps": 3, "status": sp.MINRES_CONVERGED}
        assert x8.tobytes() == x.tobytes() and np.all(h8[3:] == h[3])


def test_minres_refused_calls_leave_the_handle_usable(gpu, banded):
    row_ptr, col, val, _, b = banded
    rng = np.random.default_rng(5)
    L = sp.lib()
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        good = dev.minres(b, 5)
        x = np.zeros(N)
        hist = np.zeros(8)
        info = np.zeros(2, dtype=np.int32)
        ms = C.c_float(0)

        def call(P, iters, tol, shift):
            return L.spmv_hip_csr_minres(dev.h, P, sp.CSR_AUTO, iters, tol, shift, None, b.ctypes.data_as(C.c_void_p),
                                         x.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                         info.ctypes.data_as(nat.c_int_p), C.byref(ms))

        def still_good():
            again = dev.minres(b, 5)
            assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
            assert again[2] == good[2]
        # past the Python checks, into the library
        assert call(None, -1, 0.0, 0.0) == -1 and b"iters" in L.spmv_hip_last_error()
        for tol in (-1.0, float("nan"), float("inf")):
            assert call(None, 2, tol, 0.0) == -1 and b"tol" in L.spmv_hip_last_error()
        for shift in (float("nan"), float("inf")):
            assert call(None, 2, 0.0, shift) == -1 and b"shift" in L.spmv_hip_last_error()
        still_good()
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(RuntimeError, match="square"):
                rect.minres(np.ones(50), 2)
        still_good()
        with sp.CsrDevice(N, N, row_ptr, col, val, 0, N // 2) as half:     # rows [0, N/2) and no communicator
            with pytest.raises(RuntimeError, match="communicator"):
                half.minres(b, 2)
        rp3, col3, val3 = alternating_tridiagonal(100)
        with sp.CsrDevice(100, 100, rp3, col3, np.abs(val3)) as small, small.preconditioner("jacobi") as other_size:
            with pytest.raises(ValueError):
                dev.minres(b, 2, precond=other_size)
            assert call(other_size.h, 2, 0.0, 0.0) == -1 and b"preconditioner" in L.spmv_hip_last_error()
        still_good()
        with sp.CsrDevice(N, N, row_ptr, col, np.abs(val).astype(np.float32)) as dev32, \
                dev32.preconditioner("jacobi") as other_dtype:
            with pytest.raises(ValueError):
                dev.minres(b, 2, precond=other_dtype)
            assert call(other_dtype.h, 2, 0.0, 0.0) == -1 and b"preconditioner" in L.spmv_hip_last_error()
        still_good()


# ---------------------------------------------------------------- a KKT matrix
KKT_GRID, KKT_STEPS = (8, 8, 8), 50
# On the CPU (`python tests/test_gpu_minres.py`): after 50 steps of the reference loop on this matrix (1024 rows,
# hist[-1] = 3.9e-2 hist[0], a history that never grows) the true ||b - A x||^2 over the recorded hist[-1] is off 1 by
# KKT_REF_DEVIATION (8.9e-16 over a long-double product); the device run is held to 16 times that.  Textbook CG meets
# p.q <= 0 at step 1 on it.
KKT_REF_DEVIATION = 1.221e-15
KKT_FACTOR = 16.0 * KKT_REF_DEVIATION


def kkt_problem():
    M, row_ptr, col, val = synth.kkt_like(KKT_GRID)
    b = np.random.default_rng(21).uniform(-1, 1, M)
    return M, row_ptr, col, np.ascontiguousarray(val, dtype=np.float64), b


def test_minres_on_a_kkt_matrix(gpu, oracle):
    M, row_ptr, col, val, b = kkt_problem()
    with sp.CsrDevice(M, M, row_ptr, col, val) as dev:
        x, h, info, _ = dev.minres(b, KKT_STEPS)
        assert info == {"steps": KKT_STEPS, "status": sp.MINRES_RAN_ALL}
        assert np.all(np.isfinite(x)) and np.all(np.diff(h) <= 0.0)
        rr = true_rr(oracle, row_ptr, col, val, b, x)
        print(f"kkt: true rr / hist[-1] = {rr / h[-1]:.6f}, hist[-1] / hist[0] = {h[-1] / h[0]:.3e}")
        assert abs(rr / h[-1] - 1.0) <= KKT_FACTOR, (rr, h[-1])
        assert cg_breaks_down_at(lambda v: oracle.csr_serial(row_ptr, col, val, v), b, KKT_STEPS) == 1
        _, _, _, info_cg, _ = dev.pcg(b, KKT_STEPS)
        assert info_cg["status"] == sp.PCG_BREAKDOWN, info_cg


# ---------------------------------------------------------------- the CPU measurements behind MEASURED
def measure():
    from oracle.oracle import Oracle
    oracle = Oracle()
    row_ptr, col, val, x_true, b = banded_problem(oracle)
    serial = lambda v: oracle.csr_serial(row_ptr, col, val, v)  # noqa: E731
    long = product(row_ptr, col, val)
    inv = abs_jacobi_inverse(row_ptr, col, val)
    minv = lambda r: r * inv  # noqa: E731
    import scipy.sparse as sps
    a = sps.csr_matrix((val, col, row_ptr), shape=(N, N))
    if N <= 6000:
        ev = np.linalg.eigvalsh(a.toarray())
        print(f"eigenvalues: {np.sum(ev < 0)} negative, {np.sum(ev > 0)} positive, |ev| in "
              f"[{np.min(np.abs(ev)):.3f}, {np.max(np.abs(ev)):.3f}]")
    print("CG breaks down at step", cg_breaks_down_at(serial, b, 50))
    for name, kw in (("banded", {}), ("shift", {"shift": SHIFT}), ("jacobi", {"minv": minv})):
        for k in (5, 10):
            d = differences(minres_ref(serial, b, k, **kw)[:2], minres_ref(long, b, k, **kw)[:2])
            print(f'    ("{name}", "float64", {k}): {max(d):.3e},   # x {d[0]:.3e}, history {d[1]:.3e}')
        x, h, info = minres_ref(serial, b, 500, tol=1e-10, **kw)
        rr = true_rr(oracle, row_ptr, col, val, b, x, kw.get("shift", 0.0))
        print(f"    {name}: tol 1e-10 in {info}, nonincreasing {bool(np.all(np.diff(h) <= 0))}, true rr / hist[-1] "
              f"{rr / h[-1]:.4f}, |x - x_true| {np.max(np.abs(x - x_true)):.2e}")
    x, h, _ = minres_ref(serial, b, 40)
    rr = true_rr(oracle, row_ptr, col, val, b, x)
    print(f"    hist[40] against the true residual: {abs(rr / h[-1] - 1):.2e}")
    try:
        from scipy.sparse.linalg import minres as scipy_minres
        xs, _ = scipy_minres(a, b, rtol=1e-10, maxiter=500)
        x, _, _ = minres_ref(serial, b, 500, tol=1e-10)
        print(f"    against scipy's minres: {np.max(np.abs(xs - x)) / np.max(np.abs(x)):.2e}")
    except Exception as e:  # noqa: BLE001
        print("    scipy's minres:", e)
    rd32 = lambda v: np.asarray(v).astype(np.float32).astype(np.float64)  # noqa: E731
    serial32 = lambda v: oracle.csr_serial(row_ptr, col, rd32(val), v)  # noqa: E731
    d = differences(minres_ref(serial32, rd32(b), 6, rd=rd32)[:2], minres_ref(long, b, 6)[:2])
    print(f'    ("banded", "float32", 6): {max(d):.3e},   # x {d[0]:.3e}, history {d[1]:.3e}')
    for dtype in DTYPES:
        rd = lambda v, t=dtype: np.asarray(v).astype(t).astype(np.float64)  # noqa: E731
        worst = (0.0,)
        for n in SIZES:
            rp, c, v, bb = sizes_problem(n, dtype)
            for iters in STEPS:
                d = differences(minres_ref(product(rp, c, v, np.float64), bb, iters, rd=rd)[:2],
                                minres_ref(product(rp, c, v), bb, iters)[:2])
                if max(d) > worst[0]:
                    worst = (max(d), n, iters, d)
        n, dd, bb = cap_problem(dtype)
        d64, dl = dd.astype(np.float64), dd.astype(LD)
        d = differences(minres_ref(lambda u: d64 * u, bb, 2, rd=rd)[:2],
                        minres_ref(lambda u: dl * np.asarray(u).astype(LD), bb, 2)[:2])
        print(f"    cap {np.dtype(dtype).name} n = {n}, 2 steps: x {d[0]:.3e}, history {d[1]:.3e}")
        if max(d) > worst[0]:
            worst = (max(d), n, 2, d)
        print(f'    ("sizes", "{np.dtype(dtype).name}"): {worst[0]:.3e},   # n = {worst[1]}, {worst[2]} steps, '
              f"x {worst[3][0]:.3e}, history {worst[3][1]:.3e}")
    M, rp, c, v, bk = kkt_problem()
    kserial = lambda u: oracle.csr_serial(rp, c, v, u)  # noqa: E731
    x, h, info = minres_ref(kserial, bk, KKT_STEPS)
    xl, hl, _ = minres_ref(product(rp, c, v), bk, KKT_STEPS)
    rr, rrl = true_rr(oracle, rp, c, v, bk, x), true_rr(oracle, rp, c, v, bk, xl)
    print(f"    kkt {KKT_GRID}: M {M}, {info}, hist[-1] / hist[0] {h[-1] / h[0]:.3e}, nonincreasing "
          f"{bool(np.all(np.diff(h) <= 0))}, true rr / hist[-1] - 1: serial {rr / h[-1] - 1:.3e}, long double "
          f"{float(rrl / hl[-1]) - 1:.3e}; CG breaks down at {cg_breaks_down_at(kserial, bk, KKT_STEPS)}")


if __name__ == "__main__":
    measure()
