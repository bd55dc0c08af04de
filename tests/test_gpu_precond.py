"""Jacobi and block-Jacobi preconditioners on the GPU, preconditioned CG (spmv_hip_csr_pcg) and right-preconditioned
BiCGSTAB (spmv_hip_csr_pbicgstab): the apply against numpy (bit for bit for Jacobi), refused builds, lifetimes and
row-range handles, both solvers against numpy loops of exactly the documented algorithms over the oracle's serial
product, the identities with csr_cg / csr_bicgstab, power-of-two scaling invariance, convergence where scaling or
strong in-node coupling hurts plain CG, the stop rules and a matrix of a million rows."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from test_gpu_bicgstab import assert_close, nonsym_banded, true_rr

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- reference loops and matrices
def pcg_ref(spmv, minv, b, iters, tol=0.0):
    """The loop spmv_hip_csr_pcg runs (include/spmv_hip.h), in fp64; minv None = identity.  Returns
    (x, r.r history, r.z history, info)."""
    minv = minv or (lambda v: v.copy())
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    z = minv(r)
    p = z.copy()
    rz, rr0 = float(r @ z), float(r @ r)
    hrr, hrz = [rr0], [rz]
    info = {"steps": iters, "status": sp.PCG_RAN_ALL}
    if rr0 == 0.0:
        info = {"steps": 0, "status": sp.PCG_CONVERGED}
    elif not rz > 0.0:
        info = {"steps": 0, "status": sp.PCG_BREAKDOWN}
    else:
        for k in range(1, iters + 1):
            q = spmv(p)
            pq = float(p @ q)
            if not pq > 0.0 or not np.isfinite(rz / pq):
                info = {"steps": k - 1, "status": sp.PCG_BREAKDOWN}
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = minv(r)
            rz_new, rr = float(r @ z), float(r @ r)
            hrr.append(rr)
            hrz.append(rz_new)
            if rr <= tol * tol * rr0:
                info = {"steps": k, "status": sp.PCG_CONVERGED}
                break
            if not rz_new > 0.0:
                info = {"steps": k, "status": sp.PCG_BREAKDOWN}
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
    hrr += [hrr[-1]] * (iters + 1 - len(hrr))
    hrz += [hrz[-1]] * (iters + 1 - len(hrz))
    return x, np.array(hrr), np.array(hrz), info


def pbicgstab_ref(spmv, minv, b, iters, tol=0.0):
    """The loop spmv_hip_csr_pbicgstab runs: BiCGSTAB on A M^-1 with x moving along p^ = M^-1 p and s^ = M^-1 s."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r, rh, p = b.copy(), b.copy(), b.copy()
    rho, rr0 = float(rh @ r), float(r @ r)
    hist = [rr0]
    info = {"steps": iters, "status": sp.BICG_RAN_ALL, "half_step": 0}
    tol2 = tol * tol
    if rr0 == 0.0:
        return x, np.full(iters + 1, rr0), {"steps": 0, "status": sp.BICG_CONVERGED, "half_step": 0}
    for k in range(1, iters + 1):
        ph = minv(p)
        v = spmv(ph)
        rv = float(rh @ v)
        if rv == 0.0 or not np.isfinite(rv):
            info.update(steps=k - 1, status=sp.BICG_BREAKDOWN_RHO)
            break
        alpha = rho / rv
        s = r - alpha * v
        ss = float(s @ s)
        if ss <= tol2 * rr0:
            x = x + alpha * ph
            hist.append(ss)
            info.update(steps=k, status=sp.BICG_CONVERGED, half_step=1)
            break
        sh = minv(s)
        t = spmv(sh)
        ts, tt = float(t @ s), float(t @ t)
        omega = ts / tt if tt != 0.0 else np.inf
        if tt == 0.0 or ts == 0.0 or not (np.isfinite(ts) and np.isfinite(tt) and np.isfinite(omega)):
            info.update(steps=k - 1, status=sp.BICG_BREAKDOWN_OMEGA)
            break
        x = x + (alpha * ph + omega * sh)
        r = s - omega * t
        rho_new, rr = float(rh @ r), float(r @ r)
        hist.append(rr)
        if rr <= tol2 * rr0:
            info.update(steps=k, status=sp.BICG_CONVERGED)
            break
        if rho_new == 0.0 or not np.isfinite(rho_new):
            info.update(steps=k, status=sp.BICG_BREAKDOWN_RHO)
            break
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
    hist += [hist[-1]] * (iters + 1 - len(hist))
    return x, np.array(hist), info


def csr(a):
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.shape[0], a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def block3(cond=1e4, seed=1):
    """a 3 x 3 SPD block of condition number `cond`"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q @ np.diag([1.0, np.sqrt(cond), cond]) @ q.T


def kron_spd(nodes, shift, c):
    """kron(tridiag(-1, 2 + shift, -1), C): SPD, 3 unknowns per node, strong coupling inside a node"""
    import scipy.sparse as sps
    t = sps.diags([-np.ones(nodes - 1), np.full(nodes, 2.0 + shift), -np.ones(nodes - 1)], [-1, 0, 1])
    return csr(sps.kron(t, sps.csr_matrix(c)))


def dense_blocks(row_ptr, col, val, b, row0=0, rows=None):
    """the fp64 diagonal blocks of rows [row0, row0 + rows), entries added in entry order"""
    rows = len(row_ptr) - 1 - row0 if rows is None else rows
    out = []
    for k0 in range(0, rows, b):
        bk = min(b, rows - k0)
        d = np.zeros((bk, bk))
        for i in range(bk):
            g = row0 + k0 + i
            for e in range(row_ptr[g], row_ptr[g + 1]):
                c = col[e] - (row0 + k0)
                if 0 <= c < bk:
                    d[i, c] = d[i, c] + float(val[e])
        out.append(d)
    return out


def block_minv(blocks):
    """z = M^-1 r by batched np.linalg.solve over the blocks (the last one may be shorter)"""
    b = len(blocks[0])
    full = np.array([d for d in blocks if len(d) == b])
    last = blocks[-1] if len(blocks[-1]) != b else None
    nf = len(full) * b

    def apply(r):
        z = np.empty_like(r)
        z[:nf] = np.linalg.solve(full, r[:nf].reshape(-1, b, 1)).reshape(-1)
        if last is not None:
            z[nf:] = np.linalg.solve(last, r[nf:])
        return z
    return apply


def jacobi_minv(row_ptr, col, val):
    d = np.array([blk[0, 0] for blk in dense_blocks(row_ptr, col, val, 1)])
    return lambda r: r / d


N = 3000


@pytest.fixture(scope="module")
def spd():
    """kron SPD with badly scaled rows and columns (S A S, S = 2^u, u in [-4, 4]): CG is slow, Jacobi undoes S"""
    M, rp, col, val = kron_spd(N // 3, 0.05, block3(1e2))
    rng = np.random.default_rng(21)
    s = np.ldexp(1.0, rng.integers(-4, 5, M))
    val = val * s[np.repeat(np.arange(M), np.diff(rp))] * s[col]
    b = rng.uniform(-1, 1, M)
    return M, rp, col, val, b


# ---------------------------------------------------------------- the preconditioner itself
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jacobi_apply_is_r_times_the_rounded_inverse_bit_for_bit(gpu, dtype):
    rng = np.random.default_rng(3)
    n = 700
    rows, cols, vals = [], [], []
    for i in range(n):                       # the diagonal in one, two or three pieces, among off-diagonal entries
        parts = 1 + i % 3
        for c in sorted(set(rng.integers(0, n, 4).tolist()) - {i}) + [i] * parts:
            rows.append(i)
            cols.append(c)
            vals.append(rng.uniform(0.5, 2.0) if c == i else rng.uniform(-1, 1))
    order = np.lexsort((np.arange(len(rows)), np.array(rows)))  # keep each row's entry order
    rows, cols, vals = np.array(rows)[order], np.array(cols, np.int32)[order], np.array(vals)[order].astype(dtype)
    rp = np.zeros(n + 1, np.int32)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    d = np.zeros(n)
    for e in range(len(rows)):               # the in-order fp64 sum of each row's diagonal pieces
        if cols[e] == rows[e]:
            d[rows[e]] = d[rows[e]] + float(vals[e])
    r = rng.uniform(-1, 1, n).astype(dtype)
    with sp.CsrDevice(n, n, rp, cols, vals) as dev:
        with dev.preconditioner("jacobi") as P:
            assert P.info() == {"kind": sp.PRECOND_JACOBI, "block": 1, "rows": n, "row0": 0,
                                "value_bytes": np.dtype(dtype).itemsize}
            z = P.apply(r)
            inv = (1.0 / d).astype(dtype).astype(np.float64)
            assert z.dtype == dtype and z.tobytes() == (inv * r.astype(np.float64)).astype(dtype).tobytes()
            with dev.preconditioner("block_jacobi", 1) as P1:    # BLOCK_JACOBI with b = 1: JACOBI's bytes
                assert P1.apply(r).tobytes() == z.tobytes()
                e = np.zeros(n, dtype)
                e[5] = 1
                assert P1.apply(e).tobytes() == P.apply(e).tobytes()
            with dev.preconditioner("jacobi") as P2:             # two builds: the same bytes
                assert P2.apply(r).tobytes() == z.tobytes()


@pytest.mark.parametrize("b", [1, 2, 3, 4, 7, 16, 32])
def test_block_jacobi_apply_matches_per_block_solves(gpu, b):
    import scipy.sparse as sps
    rng = np.random.default_rng(b)
    n = 301                                    # a short last block for every b > 1
    a = sps.random(n, n, density=0.05, random_state=rng, format="csr")
    a = a + sps.block_diag([rng.uniform(-1, 1, (min(b, n - k), min(b, n - k))) for k in range(0, n, b)])
    a = a + sps.diags(np.full(n, 4.0))
    M, rp, col, val = csr(a)
    blocks = dense_blocks(rp, col, val, b)
    r = rng.uniform(-1, 1, n)
    z_ref = block_minv(blocks)(r)
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("block_jacobi", b) as P:
        z = P.apply(r)
    k0 = 0
    for d in blocks:
        zr, zb = z_ref[k0:k0 + len(d)], z[k0:k0 + len(d)]
        assert np.max(np.abs(zb - zr)) <= 1e-12 * np.max(np.abs(zr)), (b, k0)
        k0 += len(d)


def test_refused_builds_leave_no_handle_and_the_handle_works(gpu, oracle):
    import scipy.sparse as sps
    rng = np.random.default_rng(8)
    n = 64
    base = sps.random(n, n, density=0.1, random_state=rng, format="lil")
    for i in range(n):
        base[i, i] = 3.0
    cases = []
    M, rp, col, val = csr(base)
    val = val.copy()
    val[rp[17] + int(np.flatnonzero(col[rp[17]:rp[18]] == 17)[0])] = 0.0    # a stored zero on the diagonal
    cases.append(("jacobi", 1, (M, rp, col, val), "row 17"))
    a = base.copy()
    a[23, 23] = 0.0                                      # lil drops the entry: row 23 without its diagonal
    cases.append(("jacobi", 1, csr(a), "row 23"))
    cases.append(("block_jacobi", 4, csr(a), "row 23"))
    a = base.copy()
    a[8:10, 8:10] = np.ones((2, 2))                      # block 4 of size 2 singular
    cases.append(("block_jacobi", 2, csr(a), "block 4"))
    L = sp.lib()
    for kind, b, (M, rp, col, val), where in cases:
        with sp.CsrDevice(M, M, rp, col, val) as dev:
            out = C.c_void_p()
            assert L.spmv_hip_csr_precond_build(dev.h, sp.PRECOND_JACOBI if kind == "jacobi" else
                                                sp.PRECOND_BLOCK_JACOBI, b, C.byref(out)) == -1
            assert not out and where.encode() in L.spmv_hip_last_error(), L.spmv_hip_last_error()
            with pytest.raises(sp.SpmvHipError):
                dev.preconditioner(kind, b)
            x = rng.uniform(-1, 1, M)
            y_ref = oracle.csr_serial(rp, col, val, x)
            assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-12 * np.max(np.abs(y_ref))
    rp = np.arange(0, 4 * 10 + 1, 4, dtype=np.int32)
    with sp.CsrDevice(10, 12, rp, rng.integers(0, 12, 40).astype(np.int32), rng.uniform(1, 2, 40)) as rect:
        with pytest.raises(sp.SpmvHipError, match="square"):
            rect.preconditioner("jacobi")


def test_precond_outlives_its_handle_and_row_ranges_give_slices(gpu, spd):
    M, rp, col, val, b = spd
    r = np.random.default_rng(2).uniform(-1, 1, M)
    dev = sp.CsrDevice(M, M, rp, col, val)
    P = dev.preconditioner("block_jacobi", 3)
    J = dev.preconditioner("jacobi")
    z, zj = P.apply(r), J.apply(r)
    dev.close()
    assert P.apply(r).tobytes() == z.tobytes() and J.apply(r).tobytes() == zj.tobytes()
    for r0, r1 in ((0, 1200), (1200, M), (600, 2400)):   # multiples of 3
        with sp.CsrDevice(M, M, rp, col, val, r0, r1) as half, half.preconditioner("block_jacobi", 3) as Ph:
            assert Ph.info()["row0"] == r0 and Ph.rows == r1 - r0
            assert Ph.apply(r[r0:r1]).tobytes() == z[r0:r1].tobytes()
            with pytest.raises(ValueError):
                half.pcg(b, 2, precond=P)                 # P of the whole handle: other rows
    P.close()
    J.close()


# ---------------------------------------------------------------- PCG
@pytest.mark.parametrize("kind,blk", [("jacobi", 1), ("block_jacobi", 3)])
def test_pcg_matches_the_reference_loop(gpu, oracle, spd, kind, blk):
    M, rp, col, val, b = spd
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    minv = block_minv(dense_blocks(rp, col, val, blk))
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner(kind, blk) as P:
        for iters, rtol in ((5, 1e-10), (25, 1e-7)):
            x, hrr, hrz, info, ms = dev.pcg(b, iters, precond=P)
            x_ref, hrr_ref, hrz_ref, info_ref = pcg_ref(spmv, minv, b, iters)
            assert info == info_ref == {"steps": iters, "status": sp.PCG_RAN_ALL} and ms > 0
            assert_close(x, x_ref, rtol, f"{kind} {iters} steps")
            assert np.all(np.abs(hrz - hrz_ref) <= rtol * hrz_ref[0] + 1e-6 * hrz_ref)
            assert np.all(np.abs(hrr - hrr_ref) <= rtol * hrr_ref[0] + 1e-6 * hrr_ref)
        assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * hrr[-1] + 1e-20 * hrr[0]
    with sp.CsrDevice(M, M, rp, col, val.astype(np.float32)) as d32, d32.preconditioner(kind, blk) as P32:
        x, hrr, _, info, _ = d32.pcg(b.astype(np.float32), 6, precond=P32)
    x_ref, hrr_ref, _, _ = pcg_ref(spmv, minv, b, 6)
    assert x.dtype == np.float32 and info["steps"] == 6 and np.all(np.isfinite(x))
    assert_close(x, x_ref, 1e-3, f"{kind} fp32")
    assert abs(hrr[0] - hrr_ref[0]) <= 1e-6 * hrr_ref[0]


def test_pcg_identities(gpu, spd):
    """P = NULL is csr_cg; Jacobi on a unit diagonal is P = NULL; two calls and a single-rank communicator agree."""
    M, rp, col, val, b = spd
    iters = 30
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        x_cg, h_cg, _ = dev.cg(b, iters)
        x, hrr, hrz, info, _ = dev.pcg(b, iters)
        assert info == {"steps": iters, "status": sp.PCG_RAN_ALL}
        assert x.tobytes() == x_cg.tobytes() and hrr.tobytes() == h_cg.tobytes() and hrz.tobytes() == hrr.tobytes()
        x2, hrr2, hrz2, info2, _ = dev.pcg(b, iters)
        assert x2.tobytes() == x.tobytes() and hrr2.tobytes() == hrr.tobytes() and info2 == info
        with dev.preconditioner("block_jacobi", 3) as P:
            a1 = dev.pcg(b, iters, precond=P)
            a2 = dev.pcg(b, iters, precond=P)
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a1[:3], a2[:3])) and a1[3] == a2[3]
        from sparsematrixvectormultiplication_amd.distributed import NativeComm
        with dev.preconditioner("jacobi") as J:
            plain = dev.pcg(b, iters, precond=J)
            plain_tol = dev.pcg(b, 400, tol=1e-9, precond=J)
            comm = NativeComm(0, 1, lambda ident: ident)
            try:
                bounds = np.array([0, M], np.int32)
                got = dev.pcg(b, iters, precond=J, bounds=bounds)
                assert all(u.tobytes() == v.tobytes() for u, v in zip(got[:3], plain[:3])) and got[3] == plain[3]
                got = dev.pcg(b, 400, tol=1e-9, precond=J, bounds=bounds)
                assert all(u.tobytes() == v.tobytes() for u, v in zip(got[:3], plain_tol[:3]))
                assert got[3] == plain_tol[3]
            finally:
                comm.close()
    # unit diagonal: D^-1 r = r exactly
    d = np.zeros(M)
    e_diag = np.flatnonzero(col == np.repeat(np.arange(M), np.diff(rp)))
    d[np.repeat(np.arange(M), np.diff(rp))[e_diag]] = val[e_diag]
    s = 1.0 / np.sqrt(d)
    unit = val * s[np.repeat(np.arange(M), np.diff(rp))] * s[col]
    unit[e_diag] = 1.0
    with sp.CsrDevice(M, M, rp, col, unit) as dev, dev.preconditioner("jacobi") as J:
        a = dev.pcg(b, iters)
        c = dev.pcg(b, iters, precond=J)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a[:3], c[:3])) and a[3] == c[3]


@pytest.mark.parametrize("kind,blk", [("jacobi", 1), ("block_jacobi", 3)])
def test_pcg_scaling_invariance(gpu, spd, kind, blk):
    """(S A S, S b) with power-of-two S (constant on each block): x' = x / s and the r.z history, bit for bit."""
    M, rp, col, val, b = spd
    rng = np.random.default_rng(5)
    s = np.repeat(np.ldexp(1.0, rng.integers(-6, 7, M // blk + 1)), blk)[:M]
    rows = np.repeat(np.arange(M), np.diff(rp))
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner(kind, blk) as P:
        x, _, hrz, info, _ = dev.pcg(b, 20, precond=P, variant=sp.CSR_WAVE_ROW)
    with sp.CsrDevice(M, M, rp, col, val * s[rows] * s[col]) as dev, dev.preconditioner(kind, blk) as P:
        xs, _, hrzs, infos, _ = dev.pcg(b * s, 20, precond=P, variant=sp.CSR_WAVE_ROW)
    assert info == infos
    assert xs.tobytes() == (x / s).tobytes() and hrzs.tobytes() == hrz.tobytes()


def test_pcg_convergence(gpu, oracle, spd):
    """Badly scaled: Jacobi PCG reaches tol in the reference's step count (+-1) where plain CG has not.
    kron(tridiag + shift, C) with cond(C) = 1e4: block-3 needs fewer steps than Jacobi."""
    tol = 1e-8
    M, rp, col, val, b = spd
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("jacobi") as J:
        x, hrr, _, info, _ = dev.pcg(b, 3000, tol=tol, precond=J)
        _, _, _, info_ref = pcg_ref(spmv, jacobi_minv(rp, col, val), b, 3000, tol)
        t = info["steps"]
        assert info["status"] == sp.PCG_CONVERGED and abs(t - info_ref["steps"]) <= 1, (info, info_ref)
        _, hrr0, _, info0, _ = dev.pcg(b, t, tol=tol)
        assert info0["status"] == sp.PCG_RAN_ALL and hrr0[t] > tol * tol * hrr0[0]
    M, rp, col, val = kron_spd(1000, 1.0, block3(1e4))
    b = np.random.default_rng(6).uniform(-1, 1, M)
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    steps = {}
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        for kind, blk, minv in (("jacobi", 1, jacobi_minv(rp, col, val)),
                                ("block_jacobi", 3, block_minv(dense_blocks(rp, col, val, 3)))):
            with dev.preconditioner(kind, blk) as P:
                x, hrr, _, info, _ = dev.pcg(b, 5000, tol=tol, precond=P)
            _, _, _, info_ref = pcg_ref(spmv, minv, b, 5000, tol)
            assert info["status"] == sp.PCG_CONVERGED and abs(info["steps"] - info_ref["steps"]) <= 1, (kind, info,
                                                                                                         info_ref)
            assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * hrr[-1] + 1e-20 * hrr[0]
            steps[kind] = info["steps"]
    assert steps["block_jacobi"] < steps["jacobi"], steps


def test_pcg_stops(gpu, spd):
    M, rp, col, val, b = spd
    tol, iters = 1e-6, 500
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("block_jacobi", 3) as P:
        x, hrr, hrz, info, ms = dev.pcg(b, iters, tol=tol, precond=P)
        t = info["steps"]
        assert info["status"] == sp.PCG_CONVERGED and 1 <= t < iters
        assert hrr[t] <= tol * tol * hrr[0] and np.all(hrr[1:t] > tol * tol * hrr[0])
        assert np.all(hrr[t:] == hrr[t]) and np.all(hrz[t:] == hrz[t])
        x0, hrr0, hrz0, info0, _ = dev.pcg(b, t, precond=P)
        assert info0 == {"steps": t, "status": sp.PCG_RAN_ALL}
        assert x0.tobytes() == x.tobytes() and hrr0.tobytes() == hrr[:t + 1].tobytes()
        x_big, hrr_big, _, info_big, _ = dev.pcg(b, 20 * iters, tol=tol, precond=P)   # tol = 0 after a stop: x kept
        assert x_big.tobytes() == x.tobytes() and info_big == info
        x_z, hrr_z, hrz_z, info_z, _ = dev.pcg(np.zeros(M), 4, precond=P)           # b = 0: converged at step 0
        assert info_z == {"steps": 0, "status": sp.PCG_CONVERGED}
        assert np.all(x_z == 0.0) and np.all(hrr_z == 0.0) and np.all(hrz_z == 0.0)
    # indefinite: p.q < 0 at step 1 (no step taken)
    rp2, col2 = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    with sp.CsrDevice(2, 2, rp2, col2, np.array([1.0, -3.0])) as dev:
        for tol in (0.0, 1e-3):
            x, hrr, _, info, _ = dev.pcg(np.array([1.0, 1.0]), 5, tol=tol)
            assert info == {"steps": 0, "status": sp.PCG_BREAKDOWN} and np.all(x == 0.0) and np.all(hrr == 2.0)
    # [[1, 2], [2, 1]] (eigenvalues 3, -1), b = e1: one full step, then p.q = -12 < 0; x stays the step-1 iterate
    import scipy.sparse as sps
    M, rp2, col2, val2 = csr(sps.csr_matrix([[1.0, 2.0], [2.0, 1.0]]))
    with sp.CsrDevice(M, M, rp2, col2, val2) as dev, dev.preconditioner("jacobi") as J:
        x, _, _, info, _ = dev.pcg(np.array([1.0, 0.0]), 5, precond=J)
        assert info == {"steps": 1, "status": sp.PCG_BREAKDOWN} and x.tolist() == [1.0, 0.0]


# ---------------------------------------------------------------- right-preconditioned BiCGSTAB
NB = 4000


@pytest.fixture(scope="module")
def nonsym(oracle):
    rng = np.random.default_rng(31)
    rp, col, val = nonsym_banded(rng, NB, 7, 40, 0.3)
    b = rng.uniform(-1, 1, NB)
    return rp, col, val, b


@pytest.mark.parametrize("kind,blk", [("jacobi", 1), ("block_jacobi", 3)])
def test_pbicgstab_matches_the_reference_loop(gpu, oracle, nonsym, kind, blk):
    rp, col, val, b = nonsym
    spmv = lambda v: oracle.csr_serial(rp, col, val, v)  # noqa: E731
    minv = block_minv(dense_blocks(rp, col, val, blk))
    with sp.CsrDevice(NB, NB, rp, col, val) as dev, dev.preconditioner(kind, blk) as P:
        for iters, rtol, htol in ((5, 1e-10, 1e-8), (20, 1e-7, 1e-4)):
            x, h, info, _ = dev.bicgstab(b, iters, precond=P)
            x_ref, h_ref, info_ref = pbicgstab_ref(spmv, minv, b, iters)
            assert info == info_ref, (info, info_ref)
            assert_close(x, x_ref, rtol, f"{kind} {iters}")
            assert np.all(np.abs(h - h_ref) <= htol * (h_ref[0] * 1e-4 + h_ref))
        x, h, info, _ = dev.bicgstab(b, 400, tol=1e-9, precond=P)
        assert info["status"] == sp.BICG_CONVERGED
        assert true_rr(oracle, rp, col, val, b, x) <= 4.0 * h[-1] + 1e-22 * h[0]


def test_pbicgstab_identities_and_column_scaling(gpu, nonsym):
    rp, col, val, b = nonsym
    L = sp.lib()
    with sp.CsrDevice(NB, NB, rp, col, val) as dev:
        x, h, info, _ = dev.bicgstab(b, 25)
        xn, hn = np.zeros(NB), np.zeros(26)
        inf = np.zeros(3, np.int32)
        ms = C.c_float(0)
        assert L.spmv_hip_csr_pbicgstab(dev.h, None, sp.CSR_AUTO, 25, 0.0, None, b.ctypes.data_as(C.c_void_p),
                                        xn.ctypes.data_as(C.c_void_p), hn.ctypes.data_as(nat.c_double_p),
                                        inf.ctypes.data_as(nat.c_int_p), C.byref(ms)) == 0
        assert xn.tobytes() == x.tobytes() and hn.tobytes() == h.tobytes() and list(inf) == list(info.values())
    cs = np.ldexp(1.0, np.random.default_rng(9).integers(-6, 7, NB))
    out = []
    for v in (val, val * cs[col]):
        with sp.CsrDevice(NB, NB, rp, col, v) as dev, dev.preconditioner("jacobi") as J:
            out.append(dev.bicgstab(b, 20, precond=J, variant=sp.CSR_WAVE_ROW))
    (x, h, info, _), (xc, hc, infoc, _) = out
    assert info == infoc and hc.tobytes() == h.tobytes() and xc.tobytes() == (x / cs).tobytes()


def test_pbicgstab_half_step_and_breakdowns(gpu):
    import scipy.sparse as sps
    rng = np.random.default_rng(4)
    n = 50
    dense = rng.uniform(-1, 1, (n, n)) * (rng.uniform(0, 1, (n, n)) < 0.2) + 6.0 * np.eye(n)
    dense[:, 0] = 0.0
    dense[0, 0] = 4.0
    b = np.zeros(n)
    b[0] = 1.0
    cases = [(dense, b, {"steps": 1, "status": sp.BICG_CONVERGED, "half_step": 1}),
             (np.array([[2.0, -6.0], [2.0, 2.0]]), np.array([1.0, 1.0]),                  # r^.(A D^-1 b) = 0
              {"steps": 0, "status": sp.BICG_BREAKDOWN_RHO, "half_step": 0})]
    for a, rhs, expect in cases:
        M, rp, col, val = csr(sps.csr_matrix(a))
        minv = jacobi_minv(rp, col, val)
        x_ref, h_ref, info_ref = pbicgstab_ref(lambda v: a @ v, minv, rhs, 6)
        assert info_ref == expect
        with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("jacobi") as J:
            for tol in (0.0, 1e-6):
                x, h, info, _ = dev.bicgstab(rhs, 6, tol=tol, precond=J)
                assert info == expect and np.all(np.isfinite(x))
                if np.any(x_ref):
                    assert_close(x, x_ref, 1e-12, "small case")
                else:
                    assert np.all(x == 0.0)
    # t.s = 0 at step 2 of csr_bicgstab's test matrix: the reference loop decides what preconditioned BiCGSTAB reports
    a = np.array([[-1.0, 0.0, 2.0], [-1.0, -1.0, 2.0], [0.0, 0.0, 1.0]])
    rhs = np.array([0.0, 1.0, 1.0])
    M, rp, col, val = csr(sps.csr_matrix(a))
    _, _, info_ref = pbicgstab_ref(lambda v: a @ v, jacobi_minv(rp, col, val), rhs, 5)
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("jacobi") as J:
        x, _, info, _ = dev.bicgstab(rhs, 5, precond=J)
    assert info == info_ref and np.all(np.isfinite(x))


# ---------------------------------------------------------------- a million rows
def test_block3_million_rows_through_both_solvers(gpu, oracle):
    """kron(5-point Laplacian, I_3) + kron(I, C): 577^2 nodes x 3 unknowns (10^6 rows, 7 M entries), SPD with strong
    in-node coupling; block-3 PCG and block-3 BiCGSTAB converge and the true residual matches the recurrence."""
    import scipy.sparse as sps
    g = 577
    t = sps.diags([-np.ones(g - 1), np.full(g, 2.005), -np.ones(g - 1)], [-1, 0, 1])
    lap = sps.kron(sps.eye(g), t) + sps.kron(t, sps.eye(g))
    a = sps.kron(lap, sps.eye(3)) + sps.kron(sps.eye(g * g), sps.csr_matrix(block3(1e3) / 1e2))
    M, rp, col, val = csr(a)
    b = np.random.default_rng(12).uniform(-1, 1, M)
    tol = 1e-8
    with sp.CsrDevice(M, M, rp, col, val) as dev, dev.preconditioner("block_jacobi", 3) as P:
        x, hrr, _, info, ms = dev.pcg(b, 4000, tol=tol, precond=P)
        assert info["status"] == sp.PCG_CONVERGED and 0 < info["steps"] < 4000 and ms > 0, info
        rr = true_rr(oracle, rp, col, val, b, x)
        assert rr <= 4.0 * hrr[-1] + 1e-20 * hrr[0], (rr, hrr[-1])
        x, h, info, _ = dev.bicgstab(b, 4000, tol=tol, precond=P)
        assert info["status"] == sp.BICG_CONVERGED and 0 < info["steps"] < 4000, info
        rr = true_rr(oracle, rp, col, val, b, x)
        assert rr <= 4.0 * h[-1] + 1e-20 * h[0], (rr, h[-1])
