"""spmv_hip_csr_lobpcg on the GPU: the two dense passes alone (Gram and update) against numpy at every lane, tile and
grid edge, then the solver against eigvalsh, against a numpy restatement of the documented loop step by step, with
every k-wide preconditioner, and at its edges.

Bounds.  A Gram entry and an update entry are sums of n (of m) products: whatever the order of the adds and whether
they are fused, |computed - exact| <= gamma_n sum |s| |t| with gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy
and Stability of Numerical Algorithms, section 3.1).  The reference is summed in long double (64-bit mantissa: its own
error is 2^-11 of the bound) up to 4099 rows; beyond, numpy's fp64 product, whose blocked sums err far below gamma_n at
n > 10^5.  The solver's bounds: true residual <= 2 tol anorm (the factor 2 caps the recurrence's drift; the restatement
stays within 1.001), |w - eigvalsh| <= 2 tol anorm (for a symmetric matrix an eigenvalue lies within the residual norm
of every Ritz value with a unit vector), max |X^T X - I| <= 48 eps / sqrt(drop) (the restatement stays below 1e-14)."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from _lobpcg_ref import BREAKDOWN, CONVERGED, DROP, RAN_ALL, lap, lobpcg_ref, scaled_lap
from _util import U64, gamma

pytestmark = pytest.mark.gpu

GRAM_ROWS, GRAM_CAP = 16, 512       # lob_gram: rows per workgroup pass, kLobGramBlocks
UPDATE_ROWS, UPDATE_CAP = 256, 256  # lob_update: rows per workgroup pass, kLobUpdateBlocks
N_BIG = 2 * max(GRAM_ROWS * GRAM_CAP, UPDATE_ROWS * UPDATE_CAP) + 5   # every lane of both kernels strides
SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 4099, N_BIG]
KS = [1, 2, 3, 5, 8, 11, 16]
GUARD = 256


class DevBuf:
    """A device buffer holding `a` (fp64), then `guard` NaNs."""

    def __init__(self, a, guard=0):
        self.host = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel(), np.full(guard, np.nan)])
        self.p = C.c_void_p()
        assert nat.lib().spmv_hip_malloc(C.byref(self.p), max(self.host.nbytes, 8)) == 0
        if self.host.nbytes:
            assert nat.lib().spmv_hip_memcpy_h2d(self.p, self.host.ctypes.data_as(C.c_void_p), self.host.nbytes) == 0

    @property
    def addr(self):
        return self.p.value

    def get(self):
        out = np.empty_like(self.host)
        if out.nbytes:
            assert nat.lib().spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes) == 0
        return out

    def free(self):
        nat.lib().spmv_hip_free(self.p)


def basis(n, k, nb):
    """S and AS (n x nb k) with a distinct value per (row, column): a wrong accumulator row or a wrong block shows"""
    i = np.arange(n, dtype=np.float64)[:, None]
    c = np.arange(nb * k, dtype=np.float64)[None, :]
    S = ((i % 1009) * 0.37 + c + 1.0) * 1e-2
    AS = (i % 997) * 0.11 - c * 0.5 + 0.25
    return S, AS


def exact_product(Lm, Rm, long_double=True):
    if long_double:
        return (Lm.astype(np.longdouble) @ Rm.astype(np.longdouble)).astype(np.float64)
    return Lm @ Rm


def blocks(M, k, nb, guard=0):
    return [DevBuf(M[:, b * k:(b + 1) * k], guard) for b in range(nb)]


def addrs(bufs):
    return [b.addr for b in bufs] + [0] * (3 - len(bufs))


@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("k", KS)
def test_gram_pass_matches_numpy_within_the_summation_bound(gpu, k, nb):
    for n in SIZES:
        S, AS = basis(n, k, nb)
        dS, dAS = blocks(S, k, nb), blocks(AS, k, nb)
        try:
            GB, GA = sp.lobpcg_gram(n, k, nb, addrs(dS), addrs(dAS))
            GB2, GA2 = sp.lobpcg_gram(n, k, nb, addrs(dS), addrs(dAS))
        finally:
            for b in dS + dAS:
                b.free()
        assert np.array_equal(GB, GB2) and np.array_equal(GA, GA2), f"n = {n}: two calls differ"
        g = float(gamma(n, U64))
        for name, got, right in (("G_B", GB, S), ("G_A", GA, AS)):
            ref = exact_product(S.T, right, n <= 4099)
            bound = g * (np.abs(S).T @ np.abs(right)) * (1 + 2.0 ** -10)
            bad = np.argwhere(~(np.abs(got - ref) <= bound))
            assert bad.size == 0, (f"n = {n}, k = {k}, nb = {nb}: {name}{tuple(bad[0])} = {got[tuple(bad[0])]!r}, "
                                   f"reference {ref[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3e}")


def coefficients(k, nb, seed=4):
    rng = np.random.default_rng(seed + 10 * k + nb)
    return rng.uniform(-1, 1, (nb * k, k)), rng.uniform(-1, 1, (nb * k, k))


@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("k", KS)
def test_update_pass_matches_numpy_within_the_summation_bound(gpu, k, nb):
    Cm, Cp = coefficients(k, nb)
    g = float(gamma(nb * k, U64))
    rng = np.random.default_rng(1)
    for n in SIZES:
        S, AS = basis(n, k, nb)
        dS, dAS = blocks(S, k, nb), blocks(AS, k, nb)
        outs = [DevBuf(np.zeros((n, k))) for _ in range(4)]
        try:
            results = []
            for _ in range(2):
                sp.lobpcg_update(n, k, nb, addrs(dS), addrs(dAS), Cm, Cp, *[o.addr for o in outs])
                results.append([o.get().reshape(n, k) for o in outs])
        finally:
            for b in dS + dAS + outs:
                b.free()
        for a, b in zip(*results):
            assert np.array_equal(a, b), f"n = {n}: two calls differ"
        # beyond 4099 rows the long double reference is taken on the head, the tail and 3000 rows in between
        rows = np.arange(n) if n <= 4099 else np.unique(np.concatenate([np.arange(600), np.arange(n - 600, n),
                                                                        rng.integers(0, n, 3000)]))
        for name, got, left, coef in (("X", results[0][0], S, Cm), ("P", results[0][1], S, Cp),
                                      ("AX", results[0][2], AS, Cm), ("AP", results[0][3], AS, Cp)):
            assert np.isfinite(got).all(), f"n = {n}: {name} is not finite"
            ref = exact_product(left[rows], coef)
            bound = g * (np.abs(left[rows]) @ np.abs(coef)) * (1 + 2.0 ** -10)
            bad = np.argwhere(~(np.abs(got[rows] - ref) <= bound))
            assert bad.size == 0, (f"n = {n}, k = {k}, nb = {nb}: {name}[{rows[bad[0][0]]}, {bad[0][1]}] = "
                                   f"{got[rows][tuple(bad[0])]!r}, reference {ref[tuple(bad[0])]!r}")
            if n > 4099:   # every row against fp64 numpy, whose own sum of m products may err by gamma_m as well
                full = 2 * g * (np.abs(left) @ np.abs(coef))
                assert np.all(np.abs(got - left @ coef) <= full), f"n = {n}, k = {k}, nb = {nb}: {name}"


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_dense_passes_leave_guards_and_unused_blocks_alone(gpu, nb):
    """Every buffer carries 256 NaNs behind it and the unused block pointers are NULL: the results are finite and equal
    to the unguarded run bit for bit, and after an in-place update the NaNs are where they were."""
    for n in (1, 5, 65, 4099):
        for k in (1, 3, 8, 11, 16):
            S, AS = basis(n, k, nb)
            Cm, Cp = coefficients(k, nb)
            plain_S, plain_AS = blocks(S, k, nb), blocks(AS, k, nb)
            plain_out = [DevBuf(np.zeros((n, k))) for _ in range(4)]
            dS, dAS = blocks(S, k, nb, GUARD), blocks(AS, k, nb, GUARD)
            # the update runs in place where the solver runs it: X and AX are block 0, P and AP block 2 (a buffer of
            # their own while nb < 3)
            extra = [DevBuf(np.zeros((n, k)), GUARD) for _ in range(2)]
            try:
                want = sp.lobpcg_gram(n, k, nb, addrs(plain_S), addrs(plain_AS))
                got = sp.lobpcg_gram(n, k, nb, addrs(dS), addrs(dAS))
                for a, b in zip(want, got):
                    assert np.isfinite(b).all() and np.array_equal(a, b), (n, k, nb)
                sp.lobpcg_update(n, k, nb, addrs(plain_S), addrs(plain_AS), Cm, Cp, *[o.addr for o in plain_out])
                outs = [dS[0], dS[2] if nb == 3 else extra[0], dAS[0], dAS[2] if nb == 3 else extra[1]]
                sp.lobpcg_update(n, k, nb, addrs(dS), addrs(dAS), Cm, Cp, *[o.addr for o in outs])
                for o, plain in zip(outs, plain_out):
                    after = o.get()
                    assert np.isfinite(after[:n * k]).all(), (n, k, nb)
                    assert np.array_equal(after[:n * k], plain.get()), (n, k, nb)
                for b in dS + dAS + extra:
                    tail = b.get()[n * k:]
                    assert np.array_equal(tail.view(np.uint64), b.host[n * k:].view(np.uint64)), (n, k, nb)
                if nb >= 2:   # W and AW are inputs only
                    assert np.array_equal(dS[1].get()[:n * k], dS[1].host[:n * k])
                    assert np.array_equal(dAS[1].get()[:n * k], dAS[1].host[:n * k])
            finally:
                for b in plain_S + plain_AS + plain_out + dS + dAS + extra:
                    b.free()


# ---------------------------------------------------------------- the solver
def device_of(A):
    return sp.CsrDevice(A.shape[0], A.shape[1], A.indptr.astype(np.int32), A.indices.astype(np.int32),
                        np.ascontiguousarray(A.data, dtype=np.float64))


_SPECTRA = {}


def spectrum(key, A):
    if key not in _SPECTRA:
        _SPECTRA[key] = np.linalg.eigvalsh(A.toarray())
    return _SPECTRA[key]


def assert_eigenpairs(A, ev, w, X, info, tol, largest=False):
    k = len(w)
    anorm = float(abs(A).sum(axis=1).max())
    assert abs(info["anorm"] - anorm) <= 1e-13 * anorm
    true = np.linalg.norm(A @ X - X * w, axis=0)
    want = ev[::-1][:k] if largest else ev[:k]
    print(f"k = {k}: steps {info['steps']}, max residual {true.max():.3e}, eigenvalue error "
          f"{np.abs(w - want).max():.3e}, |X^T X - I| {np.abs(X.T @ X - np.eye(k)).max():.3e}")
    assert np.all(true <= 2 * tol * anorm), true
    assert np.all(np.abs(w - want) <= 2 * tol * anorm), (w, want)
    assert np.abs(X.T @ X - np.eye(k)).max() <= 48 * np.finfo(float).eps / np.sqrt(DROP)
    assert np.all(np.abs(info["resid"] - true) <= 0.01 * true + 1e-3 * tol * anorm), (info["resid"], true)
    assert np.all(np.diff(w) <= 0) if largest else np.all(np.diff(w) >= 0)


@pytest.mark.parametrize("grid,k,tol,iters,largest", [((24, 31), 4, 1e-9, 300, False), ((12, 13), 1, 1e-10, 300, False),
                                                      ((12, 13), 5, 1e-10, 300, False), ((40, 53), 16, 1e-9, 400, False),
                                                      ((24, 31), 3, 1e-9, 600, True)])
def test_lobpcg_converges_to_the_extreme_eigenpairs(gpu, grid, k, tol, iters, largest):
    A = lap(*grid)
    ev = spectrum(grid, A)
    with device_of(A) as dev:
        w, X, th, rh, info, ms = dev.lobpcg(k, iters, tol=tol, largest=largest)
    assert info["status"] == CONVERGED and 0 < info["steps"] < iters and ms > 0 and info["host_ms"] > 0, info
    assert th.shape == rh.shape == (iters + 1, k) and X.shape == (A.shape[0], k)
    assert_eigenpairs(A, ev, w, X, info, tol, largest)
    # the recurrence's last residual is the true one, and after the stop both histories repeat their last row
    s = info["steps"]
    assert np.all(np.abs(rh[s] - info["resid"]) <= 0.01 * info["resid"] + 1e-3 * tol * info["anorm"])
    assert np.all(th[s:] == th[s]) and np.all(rh[s:] == rh[s]) and np.array_equal(th[s], w)


def test_lobpcg_k16_on_n64_runs_all_its_steps(gpu):
    A = lap(8, 8)
    with device_of(A) as dev:
        w, X, th, rh, info, ms = dev.lobpcg(16, 20)
    assert info["status"] == RAN_ALL and info["steps"] == 20, info
    assert np.isfinite(w).all() and np.isfinite(X).all() and np.isfinite(th).all() and np.isfinite(rh).all()
    assert np.all(np.diff(th, axis=0) <= 1e-10 * info["anorm"]), np.diff(th, axis=0).max()
    assert 16 <= info["min_basis"] <= 48


@pytest.mark.parametrize("grid", [(24, 31), (300, 301)])
@pytest.mark.parametrize("k", [4, 8])
def test_lobpcg_follows_the_numpy_restatement_step_by_step(gpu, grid, k):
    """5 steps with tol = 0.  The allowance is 32 times the largest difference between two restatements that differ in
    the order of the Gram sums alone (rows in natural and in reversed order), plus 1e-13 anorm."""
    A = lap(*grid)
    X0 = np.random.default_rng(0).standard_normal((A.shape[0], k))
    nat_run = lobpcg_ref(A, X0, 5)
    rev_run = lobpcg_ref(A, X0, 5, reverse=True)
    spread = max(np.abs(nat_run[2] - rev_run[2]).max(), np.abs(nat_run[3] - rev_run[3]).max())
    with device_of(A) as dev:
        w, X, th, rh, info, ms = dev.lobpcg(k, 5, X0=X0)
    assert info["status"] == RAN_ALL and info["steps"] == 5 and info["restarts"] == nat_run[4]["restarts"]
    allowed = 32 * spread + 1e-13 * info["anorm"]
    for name, got, ref in (("theta", th, nat_run[2]), ("residual", rh, nat_run[3])):
        d = np.abs(got - ref).max(axis=1)
        print(f"{grid}, k = {k}: {name} history, |device - restatement| per row {d}, the restatements' spread "
              f"{spread:.3e}, ratio {d.max() / max(spread, 1e-300):.2f}")
        assert np.all(d <= allowed), (name, d, allowed)


def test_lobpcg_with_every_k_wide_preconditioner(gpu):
    A = scaled_lap()
    ev = spectrum("scaled", A)
    tol, k = 1e-9, 4
    steps = {}
    with device_of(A) as dev:
        for name, make in (("none", lambda: None), ("jacobi", lambda: dev.preconditioner("jacobi")),
                           ("block3", lambda: dev.preconditioner("block_jacobi", 3)),
                           ("fsai", lambda: dev.preconditioner("fsai"))):
            P = make()
            try:
                w, X, th, rh, info, ms = dev.lobpcg(k, 2000, tol=tol, precond=P)
            finally:
                if P is not None:
                    P.close()
            assert info["status"] == CONVERGED, (name, info)
            assert_eigenpairs(A, ev, w, X, info, tol)
            steps[name] = info["steps"]
        print(f"steps to tol = {tol}: {steps}")
        assert 2 * steps["jacobi"] <= steps["none"], steps
        for kind in ("ssor", "ilu0"):
            P = dev.preconditioner(kind)
            try:
                with pytest.raises(ValueError):
                    dev.lobpcg(k, 10, precond=P)
                words = np.zeros(4, dtype=np.int32)
                X0 = np.ones((A.shape[0], k))
                assert nat.lib().spmv_hip_csr_lobpcg(dev.h, P.h, k, 10, 0.0, 0, X0.ctypes.data_as(nat.c_double_p), None,
                                                     None, None, None, None, None, words.ctypes.data_as(nat.c_int_p),
                                                     None, None) == -1
                assert b"SSOR" in nat.lib().spmv_hip_last_error()
            finally:
                P.close()


def test_lobpcg_edges(gpu):
    A = lap(24, 31)
    n, k = A.shape[0], 4
    X0 = np.random.default_rng(0).standard_normal((n, k))
    with device_of(A) as dev:
        a = dev.lobpcg(k, 40, tol=1e-3, X0=X0)
        b = dev.lobpcg(k, 40, tol=1e-3, X0=X0)
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(u, v), "two calls differ"
        s = a[4]["steps"]
        assert a[4]["status"] == CONVERGED and s < 40
        assert np.all(a[2][s:] == a[2][s]) and np.all(a[3][s:] == a[3][s])
        # two equal columns: no k independent directions at step 0
        twin = X0.copy()
        twin[:, 2] = twin[:, 0]
        w, X, th, rh, info, ms = dev.lobpcg(k, 10, X0=twin)
        assert info["status"] == BREAKDOWN and info["steps"] == 0 and info["min_basis"] == k - 1, info
        assert np.all(w == 0) and np.all(X == 0)
        # a NaN in X0: a breakdown, and no NaN comes back
        bad = X0.copy()
        bad[17, 1] = np.nan
        w, X, th, rh, info, ms = dev.lobpcg(k, 10, X0=bad)
        assert info["status"] == BREAKDOWN and info["steps"] == 0, info
        assert np.all(w == 0) and np.all(X == 0) and np.isfinite(th).all() and np.isfinite(rh).all()
        # iters = 0: the Ritz pairs of X0
        w, X, th, rh, info, ms = dev.lobpcg(k, 0, X0=X0)
        assert info["status"] == RAN_ALL and info["steps"] == 0 and th.shape == (1, k)
        Q, _ = np.linalg.qr(X0)
        ritz = np.linalg.eigvalsh(Q.T @ (A @ Q))
        assert np.abs(w - ritz).max() <= 1e-12 * info["anorm"]
        assert np.abs(X.T @ X - np.eye(k)).max() <= 1e-12
        assert np.abs(np.linalg.norm(A @ X - X * w, axis=0) - rh[0]).max() <= 1e-12 * info["anorm"]
        # the C entry point refuses what the method refuses
        for kk, iters, tol in ((0, 3, 0.0), (17, 3, 0.0), (4, -1, 0.0), (4, 3, -1.0), (4, 3, float("nan"))):
            assert nat.lib().spmv_hip_csr_lobpcg(dev.h, None, kk, iters, tol, 0, X0.ctypes.data_as(nat.c_double_p),
                                                 None, None, None, None, None, None, None, None, None) == -1
    # the zero matrix: converged at step 0 with w = 0
    import scipy.sparse as sps
    Z = sps.csr_matrix((64, 64))
    with device_of(Z) as dev:
        w, X, th, rh, info, ms = dev.lobpcg(2, 10, tol=1e-9)
    assert info["status"] == CONVERGED and info["steps"] == 0 and info["anorm"] == 0, info
    assert np.all(w == 0) and np.isfinite(X).all()
    # n < 4 k and an fp32 handle at the C entry point
    small = lap(7, 9)
    with device_of(small) as dev:
        X0 = np.ones((63, 16))
        assert nat.lib().spmv_hip_csr_lobpcg(dev.h, None, 16, 3, 0.0, 0, X0.ctypes.data_as(nat.c_double_p), None, None,
                                             None, None, None, None, None, None, None) == -1
        with pytest.raises(ValueError):
            dev.lobpcg(16, 3)
    with sp.CsrDevice(63, 63, small.indptr.astype(np.int32), small.indices.astype(np.int32),
                      small.data.astype(np.float32)) as dev32:
        X0 = np.ones((63, 2))
        assert nat.lib().spmv_hip_csr_lobpcg(dev32.h, None, 2, 3, 0.0, 0, X0.ctypes.data_as(nat.c_double_p), None, None,
                                             None, None, None, None, None, None, None) == -1


def test_lobpcg_refuses_an_active_communicator(gpu):
    """With a (single-rank) communicator open the method raises ValueError and the C entry point returns -1 naming the
    communicator; after close() a plain call gives the bits it gave before."""
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    A = lap(24, 31)
    k = 4
    X0 = np.random.default_rng(0).standard_normal((A.shape[0], k))
    with device_of(A) as dev:
        before = dev.lobpcg(k, 10, X0=X0)
        comm = NativeComm(0, 1, lambda ident: ident)
        try:
            with pytest.raises(ValueError, match="communicator"):
                dev.lobpcg(k, 10, X0=X0)
            words = np.zeros(4, dtype=np.int32)
            assert nat.lib().spmv_hip_csr_lobpcg(dev.h, None, k, 10, 0.0, 0, X0.ctypes.data_as(nat.c_double_p), None,
                                                 None, None, None, None, None, words.ctypes.data_as(nat.c_int_p),
                                                 None, None) == -1
            assert b"communicator" in nat.lib().spmv_hip_last_error()
        finally:
            comm.close()
        after = dev.lobpcg(k, 10, X0=X0)
    assert after[4]["status"] == RAN_ALL and after[4]["steps"] == 10
    for u, v in zip(before[:4], after[:4]):
        assert np.array_equal(u, v)
