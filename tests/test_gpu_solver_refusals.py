"""What every solver entry point refuses, word for word, and what a solve that stops early hands back.

The refusals are asked of the library directly (the Python wrappers refuse iters and tol before the library sees them)
and the whole text of spmv_hip_last_error() is compared.  Two bad arguments at once pin the order of the checks.  No
solve runs in those cases.  The texts that differ between the entries are pinned as they are: csr_cg and csr_cg_multi
fold iters and tol into "bad arguments" and take a partial handle without a communicator, csr_cgls and csr_lobpcg word
the partial handle their own way.

The early stops: a strongly diagonally dominant SPD band of 300 rows (more than one workgroup of the single-row
kernels), 40 steps allowed and a tolerance met within a few, so the host's poll at step 16 ends the loop and the
histories' rows past that come from copy_history's repeat.  The existing stop tests (test_bicgstab_tol_stops_early,
test_pcg_stops, test_cgls_tol_stops_at_the_reference_step, test_minres_stops_and_breakdowns,
test_cg_multi_tol_freezes_columns_and_stops_early, test_columns_stop_on_their_own_and_the_loop_ends_early) use
larger matrices and budgets and none asserts a stop before step 16, so every entry with a tolerance has a case here.
"""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- handles
def tridiagonal(n, dtype=np.float64):
    import scipy.sparse as sps
    a = sps.diags([-np.ones(n - 1), 4.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)


def rectangular():
    """3 x 4: (i, i) and (i, i + 1)"""
    rp = np.array([0, 2, 4, 6], np.int32)
    col = np.array([0, 1, 1, 2, 2, 3], np.int32)
    return rp, col, np.ones(6)


@pytest.fixture(scope="module")
def handles(gpu):
    rp, col, val = tridiagonal(4)
    rrp, rcol, rval = rectangular()
    rp64, col64, val64 = tridiagonal(64)
    h = {"square": sp.CsrDevice(4, 4, rp, col, val),
         "rect": sp.CsrDevice(3, 4, rrp, rcol, rval),
         "part": sp.CsrDevice(4, 4, rp, col, val, row0=1, row1=3),
         "rect_part": sp.CsrDevice(3, 4, rrp, rcol, rval, row0=1, row1=3),
         "lob": sp.CsrDevice(64, 64, rp64, col64, val64),
         "lob_part": sp.CsrDevice(64, 64, rp64, col64, val64, row0=1, row1=3)}
    h["square_t"] = h["square"].transpose()
    yield h
    for dev in h.values():
        dev.close()


class Scratch:
    """Host arrays wide enough for every refused call (none is read or written: the refusal comes first)"""

    def __init__(self):
        self.a = [np.zeros(4096) for _ in range(6)]
        self.i = [np.zeros(256, np.int32) for _ in range(2)]
        self.ms = [C.c_float(0), C.c_float(0)]
        self.anorm = C.c_double(0)

    def v(self, j):
        return self.a[j].ctypes.data_as(C.c_void_p)

    def d(self, j):
        return self.a[j].ctypes.data_as(nat.c_double_p)

    def n(self, j):
        return self.i[j].ctypes.data_as(nat.c_int_p)


S = Scratch()


def cg(dev, iters=1):
    return nat.lib().spmv_hip_csr_cg(dev.h, 0, iters, None, 0, S.v(0), S.v(1), S.d(2), C.byref(S.ms[0]))


def cg_multi(dev, iters=1, tol=0.0, k=1):
    return nat.lib().spmv_hip_csr_cg_multi(dev.h, k, iters, tol, None, S.v(0), S.v(1), S.d(2), S.n(0), C.byref(S.ms[0]))


def pcg(dev, iters=1, tol=0.0):
    return nat.lib().spmv_hip_csr_pcg(dev.h, None, 0, iters, tol, None, S.v(0), S.v(1), S.d(2), S.d(3), S.n(0),
                                      C.byref(S.ms[0]))


def pcg_multi(dev, iters=1, tol=0.0, k=1):
    return nat.lib().spmv_hip_csr_pcg_multi(dev.h, None, k, iters, tol, None, S.v(0), S.v(1), S.d(2), S.d(3), S.n(0),
                                            S.n(1), C.byref(S.ms[0]))


def bicgstab(dev, iters=1, tol=0.0):
    return nat.lib().spmv_hip_csr_bicgstab(dev.h, 0, iters, tol, None, S.v(0), S.v(1), S.d(2), S.n(0), C.byref(S.ms[0]))


def pbicgstab(dev, iters=1, tol=0.0):
    return nat.lib().spmv_hip_csr_pbicgstab(dev.h, None, 0, iters, tol, None, S.v(0), S.v(1), S.d(2), S.n(0),
                                            C.byref(S.ms[0]))


def minres(dev, iters=1, tol=0.0, shift=0.0):
    return nat.lib().spmv_hip_csr_minres(dev.h, None, 0, iters, tol, shift, None, S.v(0), S.v(1), S.d(2), S.n(0),
                                         C.byref(S.ms[0]))


def cgls(dev, at, iters=1, tol=0.0, damp=0.0):
    return nat.lib().spmv_hip_csr_cgls(dev.h, at.h, iters, tol, damp, S.v(0), S.v(1), S.d(2), S.d(3), S.n(0),
                                       C.byref(S.ms[0]))


def lobpcg(dev, iters=1, tol=0.0, k=16):
    return nat.lib().spmv_hip_csr_lobpcg(dev.h, None, k, iters, tol, 0, S.d(0), S.d(1), S.d(2), S.d(3), S.d(4), S.d(5),
                                         C.byref(S.anorm), S.n(0), C.byref(S.ms[0]), C.byref(S.ms[1]))


def refused(rc, text):
    assert rc == -1, (rc, text)
    got = nat.lib().spmv_hip_last_error().decode()
    assert got == text, (got, text)


# the entries that share the whole frame: name -> call(dev, iters, tol)
FRAMED = {"csr_pcg": pcg, "csr_pcg_multi": pcg_multi, "csr_bicgstab": bicgstab, "csr_pbicgstab": pbicgstab,
          "csr_minres": minres}


# ---------------------------------------------------------------- the shared refusals
@pytest.mark.parametrize("name", sorted(FRAMED))
def test_shared_refusals_of_the_framed_entries(handles, name):
    call = FRAMED[name]
    refused(call(handles["square"], iters=-1), f"{name}: iters = -1, must be >= 0")
    refused(call(handles["square"], tol=NAN), f"{name}: tol = nan, must be finite and >= 0")
    refused(call(handles["square"], tol=-1.0), f"{name}: tol = -1, must be finite and >= 0")
    refused(call(handles["square"], tol=INF), f"{name}: tol = inf, must be finite and >= 0")
    refused(call(handles["rect"]), f"{name}: needs a square matrix (3 x 4)")
    refused(call(handles["part"]), f"{name}: a handle of rows [1, 3) needs a communicator")
    # precedence: iters before tol, tol before the shape, the shape before the rows
    refused(call(handles["square"], iters=-1, tol=NAN), f"{name}: iters = -1, must be >= 0")
    refused(call(handles["rect"], tol=-1.0), f"{name}: tol = -1, must be finite and >= 0")
    refused(call(handles["rect_part"]), f"{name}: needs a square matrix (3 x 4)")


def test_minres_places_the_shift_between_tol_and_the_shape(handles):
    refused(minres(handles["square"], shift=NAN), "csr_minres: shift = nan, must be finite")
    refused(minres(handles["square"], tol=NAN, shift=INF), "csr_minres: tol = nan, must be finite and >= 0")
    refused(minres(handles["rect"], shift=INF), "csr_minres: shift = inf, must be finite")


def test_pcg_multi_places_k_between_tol_and_the_shape(handles):
    refused(pcg_multi(handles["square"], k=0), "csr_pcg_multi: k = 0, must be in [1, 64]")
    refused(pcg_multi(handles["square"], k=65), "csr_pcg_multi: k = 65, must be in [1, 64]")
    refused(pcg_multi(handles["square"], tol=-1.0, k=0), "csr_pcg_multi: tol = -1, must be finite and >= 0")
    refused(pcg_multi(handles["rect"], k=65), "csr_pcg_multi: k = 65, must be in [1, 64]")
    refused(pcg_multi(handles["part"], k=0), "csr_pcg_multi: k = 0, must be in [1, 64]")


def test_cg_folds_iters_into_bad_arguments(handles):
    refused(cg(handles["square"], iters=-1), "csr_cg: bad arguments")
    refused(cg(handles["rect"]), "csr_cg: needs a square matrix (3 x 4)")
    refused(cg(handles["rect"], iters=-1), "csr_cg: bad arguments")


def test_cg_multi_folds_iters_and_tol_into_bad_arguments(handles):
    refused(cg_multi(handles["square"], iters=-1), "csr_cg_multi: bad arguments")
    refused(cg_multi(handles["square"], tol=NAN), "csr_cg_multi: bad arguments")
    refused(cg_multi(handles["square"], tol=-1.0), "csr_cg_multi: bad arguments")
    refused(cg_multi(handles["square"], k=0), "csr_cg_multi: k = 0, must be in [1, 64]")
    refused(cg_multi(handles["square"], k=65), "csr_cg_multi: k = 65, must be in [1, 64]")
    refused(cg_multi(handles["rect"]), "csr_cg_multi: needs a square matrix (3 x 4)")
    refused(cg_multi(handles["square"], tol=-1.0, k=0), "csr_cg_multi: bad arguments")
    refused(cg_multi(handles["rect"], k=65), "csr_cg_multi: k = 65, must be in [1, 64]")


def test_cgls_refusals(handles):
    a, at = handles["square"], handles["square_t"]
    refused(cgls(a, at, iters=-1), "csr_cgls: iters = -1, must be >= 0")
    refused(cgls(a, at, tol=NAN), "csr_cgls: tol = nan, must be finite and >= 0")
    refused(cgls(a, at, tol=-1.0), "csr_cgls: tol = -1, must be finite and >= 0")
    refused(cgls(a, at, damp=-1.0), "csr_cgls: damp = -1, must be finite and >= 0")
    refused(cgls(handles["part"], at), "csr_cgls: A holds rows [1, 3) of 4; CGLS takes whole matrices")
    refused(cgls(a, handles["part"]), "csr_cgls: A^T holds rows [1, 3) of 4; CGLS takes whole matrices")
    refused(cgls(handles["rect"], at), "csr_cgls: A^T is 4 x 4, A is 3 x 4: not its transpose")
    refused(cgls(a, at, iters=-1, tol=NAN), "csr_cgls: iters = -1, must be >= 0")
    refused(cgls(a, at, tol=-1.0, damp=NAN), "csr_cgls: tol = -1, must be finite and >= 0")
    refused(cgls(handles["part"], at, damp=-1.0), "csr_cgls: damp = -1, must be finite and >= 0")


def test_lobpcg_refusals(handles):
    dev = handles["lob"]
    refused(lobpcg(dev, iters=-1), "csr_lobpcg: iters = -1, must be >= 0")
    refused(lobpcg(dev, tol=NAN), "csr_lobpcg: tol = nan, must be finite and >= 0")
    refused(lobpcg(dev, tol=-1.0), "csr_lobpcg: tol = -1, must be finite and >= 0")
    refused(lobpcg(dev, k=0), "csr_lobpcg: k = 0, must be in [1, 16]")
    refused(lobpcg(dev, k=65), "csr_lobpcg: k = 65, must be in [1, 16]")
    refused(lobpcg(handles["rect"]), "csr_lobpcg: needs a square matrix (3 x 4)")
    refused(lobpcg(handles["lob_part"]), "csr_lobpcg: a handle of rows [1, 3) is not the whole matrix")
    refused(lobpcg(handles["square"], k=2), "csr_lobpcg: n = 4, must be >= 4 k = 8")
    # the shape and the rows come before k, k before iters, iters before tol
    refused(lobpcg(handles["rect"], k=0), "csr_lobpcg: needs a square matrix (3 x 4)")
    refused(lobpcg(handles["lob_part"], k=0), "csr_lobpcg: a handle of rows [1, 3) is not the whole matrix")
    refused(lobpcg(dev, iters=-1, k=65), "csr_lobpcg: k = 65, must be in [1, 16]")
    refused(lobpcg(dev, iters=-1, tol=NAN), "csr_lobpcg: iters = -1, must be >= 0")


# ---------------------------------------------------------------- early stops
N, ITERS, POLL = 300, 40, 16
# the spectrum lies within [4 - 0.8, 5 + 0.8]: a condition number below 2, so CG, MINRES and BiCGSTAB gain a digit per
# step and CGLS (the square of that condition number) one in two; 1e-4 is met by step 10 in both dtypes
TOL = 1e-4


@pytest.fixture(scope="module")
def band():
    """SPD band: diagonal uniform in [4, 5], offsets 1, 2 and 5 with entries uniform in [-0.13, 0.13] (a row's
    off-diagonal entries sum to less than 0.8 in absolute value), and four right-hand sides"""
    import scipy.sparse as sps
    rng = np.random.default_rng(300)
    offs = [rng.uniform(-0.13, 0.13, N - d) for d in (1, 2, 5)]
    a = sps.diags(offs + [rng.uniform(4.0, 5.0, N)] + offs, [1, 2, 5, 0, -1, -2, -5]).tocsr()
    a.sort_indices()
    assert abs(a - a.T).max() == 0 and (np.asarray(abs(a).sum(axis=1)).ravel() - 2 * a.diagonal()).max() < -3.0
    b = rng.uniform(-1, 1, (N, 4))
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data), b


def single(kind):
    """call(dev, P, at, b, iters, tol) -> (x, [histories], steps) of the entries with one right-hand side"""
    def call(dev, P, at, b, iters, tol):
        if kind == "pcg":
            x, rr, rz, info, _ = dev.pcg(b[:, 0].copy(), iters, tol=tol)
            return x, [rr, rz], info["steps"]
        if kind in ("bicgstab", "pbicgstab"):
            x, h, info, _ = dev.bicgstab(b[:, 0].copy(), iters, tol=tol, precond=P if kind == "pbicgstab" else None)
            return x, [h], info["steps"]
        if kind == "minres":
            x, h, info, _ = dev.minres(b[:, 0].copy(), iters, tol=tol)
            return x, [h], info["steps"]
        if kind == "cgls":
            x, ss, rr, info, _ = dev.cgls(b[:, 0].copy(), iters, tol=tol, at=at)
            return x, [ss, rr], info["steps"]
        if kind == "cg_multi":
            X, h, done, _ = dev.cg_multi(np.ascontiguousarray(b[:, :3]), iters, tol=tol)
            return X, [h], int(done.max())
        X, rr, rz, info, _ = dev.pcg_multi(np.ascontiguousarray(b[:, :3]), iters, tol=tol, precond=P)
        return X, [rr, rz], int(info["steps"].max())
    return call


EARLY = ["cg_multi", "pcg", "pcg_multi", "bicgstab", "pbicgstab", "minres", "cgls"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", EARLY)
def test_a_solve_that_stops_before_the_first_poll(gpu, band, kind, dtype):
    """The stop comes before step 16, the histories' rows from the stop on are the stop's row bit for bit, and x is
    that of a solve given exactly that many steps."""
    rp, col, val, b = band
    b = b.astype(dtype)
    call = single(kind)
    with sp.CsrDevice(N, N, rp, col, val.astype(dtype)) as dev, dev.transpose() as at, dev.preconditioner("jacobi") as P:
        x, hists, steps = call(dev, P, at, b, ITERS, TOL)
        print(f"{kind} {np.dtype(dtype).name}: {steps} steps")
        assert 1 <= steps < POLL, (kind, steps)
        for h in hists:
            assert h.shape[0] == ITERS + 1
            for t in range(steps, ITERS + 1):
                assert h[t].tobytes() == h[steps].tobytes(), (kind, t, steps)
        x2, hists2, steps2 = call(dev, P, at, b, steps, TOL)
        assert steps2 == steps and x2.tobytes() == x.tobytes(), (kind, steps, steps2)
        for h, h2 in zip(hists, hists2):
            assert h2.tobytes() == h[:steps + 1].tobytes(), kind


def test_lobpcg_stops_before_step_16(gpu, band):
    """LOBPCG keeps its histories on the host; the same three properties.  The loop of tests/_lobpcg_ref.py meets
    0.01 ||A||_inf (about 0.055) for two pairs from this start at step 7."""
    rp, col, val, _ = band
    tol = 0.01
    with sp.CsrDevice(N, N, rp, col, val) as dev:
        w, X, th, rh, info, _ = dev.lobpcg(2, ITERS, tol=tol, seed=3)
        steps = info["steps"]
        print(f"lobpcg: {steps} steps, residuals {rh[steps]}, anorm {info['anorm']}")
        assert info["status"] == sp.LOBPCG_CONVERGED and steps < POLL, info
        for h in (th, rh):
            for t in range(steps, ITERS + 1):
                assert h[t].tobytes() == h[steps].tobytes(), (t, steps)
        w2, X2, th2, rh2, info2, _ = dev.lobpcg(2, steps, tol=tol, seed=3)
        assert info2["steps"] == steps and X2.tobytes() == X.tobytes() and w2.tobytes() == w.tobytes()
        assert th2.tobytes() == th[:steps + 1].tobytes() and rh2.tobytes() == rh[:steps + 1].tobytes()
