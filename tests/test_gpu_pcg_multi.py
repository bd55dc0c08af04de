"""spmv_hip_csr_pcg_multi and the k-wide preconditioner apply on the GPU: k independent PCG recurrences that share one
SpMM per step, against spmv_hip_csr_pcg column by column, plus the bit-level identities the fixed reduction order
promises (k = 1 is pcg, no preconditioner is cg_multi, column permutations), the apply alone, the per-column stop
rules, the grid edges, a single-rank communicator and refused calls."""
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from _util import FP64_RTOL, U32, U64, gamma

pytestmark = pytest.mark.gpu


def spd_banded(rng, n, per_row, band):
    """symmetric, strictly diagonally dominant (hence positive definite) banded matrix as CSR"""
    import scipy.sparse as sps
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-band, band + 1, len(r)), 0, n - 1)
    b = sps.csr_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n))
    a = b + b.T
    a = a + sps.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0)
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.ascontiguousarray(a.data)


def products(oracle, row_ptr, col, val, X):
    return np.stack([oracle.csr_serial(row_ptr, col, val, X[:, j]) for j in range(X.shape[1])], axis=1)


def assert_columns_close(X, X_ref, rtol, what):
    for j in range(X.shape[1]):
        scale = np.max(np.abs(X_ref[:, j]))
        err = np.max(np.abs(X[:, j] - X_ref[:, j]))
        assert err <= rtol * scale, f"{what}: column {j}: {err:.3e} > {rtol} * {scale:.3e}"


def assert_true_residual(oracle, row_ptr, col, val, B, X, hist):
    """the recurrence's residual is the true one: |b_j - A x_j|^2 <= 4 rr_j"""
    R = B - products(oracle, row_ptr, col, val, np.asarray(X, dtype=np.float64))
    for j in range(B.shape[1]):
        rr = float(R[:, j] @ R[:, j])
        assert rr <= 4.0 * hist[-1, j] + 1e-20 * hist[0, j], f"column {j}: true {rr:.3e} vs recorded {hist[-1, j]:.3e}"


N = 6000
PRECONDS = [None, ("jacobi", 1), ("block_jacobi", 3), ("block_jacobi", 32), ("fsai", 32), ("fsai", 4)]
PRECOND_IDS = ["none", "jacobi", "block3", "block32", "fsai32", "fsai4"]


def make_precond(dev, spec):
    if spec is None:
        return None
    kind, size = spec
    return dev.preconditioner("fsai", cap=size) if kind == "fsai" else dev.preconditioner(kind, size)


def close(P):
    if P is not None:
        P.close()


def pcg_columns(dev, B, iters, P, tol=0.0):
    """the reference: dev.pcg on every column of B -> (X, rr_hist, rz_hist, steps, status)"""
    out = [dev.pcg(np.ascontiguousarray(B[:, j]), iters, tol=tol, precond=P) for j in range(B.shape[1])]
    return (np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1),
            np.stack([o[2] for o in out], axis=1), np.array([o[3]["steps"] for o in out]),
            np.array([o[3]["status"] for o in out]))


def assert_matches_pcg_columns(dev, B, iters, P, what):
    """the comparison of the cg_multi test against its per-column loop, here against dev.pcg: at 5 steps 1e-10 relative
    on X and on both histories, at 25 steps 1e-7 on X and 1e-8 h[0] + 1e-4 h on the histories.  Returns the run."""
    assert iters in (5, 25)
    X, rr, rz, info, ms = dev.pcg_multi(B, iters, precond=P)
    X_ref, rr_ref, rz_ref, steps_ref, status_ref = pcg_columns(dev, B, iters, P)
    k = B.shape[1]
    assert X.shape == B.shape and rr.shape == (iters + 1, k) and rz.shape == (iters + 1, k) and ms > 0
    assert np.array_equal(info["steps"], steps_ref) and np.array_equal(info["status"], status_ref), (what, info)
    for name, h, h_ref in (("rr", rr, rr_ref), ("rz", rz, rz_ref)):
        d = np.abs(h - h_ref)
        print(f"{what}: {iters} steps: {name} history, worst |d| / |h[0]| = {np.max(d / np.abs(h_ref[0])):.3e}")
        if iters == 5:
            assert np.all(d <= 1e-10 * np.abs(h_ref[0])), (what, name)
        else:
            assert np.all(d <= 1e-8 * np.abs(h_ref[0]) + 1e-4 * np.abs(h_ref)), (what, name)
    assert_columns_close(X, X_ref, 1e-10 if iters == 5 else 1e-7, f"{what}: {iters} steps")
    return X, rr, rz, info


@pytest.fixture(scope="module")
def banded(oracle):
    rng = np.random.default_rng(808)
    row_ptr, col, val = spd_banded(rng, N, 7, 60)
    X_true = rng.uniform(-1, 1, (N, 40))
    B = products(oracle, row_ptr, col, val, X_true)
    return row_ptr, col, val, X_true, B


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_k1_is_pcg_bit_for_bit(gpu, banded, dtype):
    """For every P: pcg_multi on an n x 1 B gives pcg's x, both histories, steps and status exactly, with tol = 0 and
    with tol = 1e-6."""
    row_ptr, col, val, _, B_all = banded
    b = np.ascontiguousarray(B_all[:, 0].astype(dtype))
    iters = 25
    with sp.CsrDevice(N, N, row_ptr, col, val.astype(dtype)) as dev:
        for spec, name in zip(PRECONDS, PRECOND_IDS):
            P = make_precond(dev, spec)
            try:
                for tol in (0.0, 1e-6):
                    x, rr, rz, info, _ = dev.pcg(b, iters, tol=tol, precond=P)
                    X, RR, RZ, INFO, _ = dev.pcg_multi(b[:, None], iters, tol=tol, precond=P)
                    what = f"{name} {np.dtype(dtype)} tol={tol}"
                    assert X.shape == (N, 1) and RR.shape == (iters + 1, 1) and RZ.shape == (iters + 1, 1)
                    assert X[:, 0].tobytes() == x.tobytes(), what
                    assert RR[:, 0].tobytes() == rr.tobytes() and RZ[:, 0].tobytes() == rz.tobytes(), what
                    assert INFO["steps"].tolist() == [info["steps"]], what
                    assert INFO["status"].tolist() == [info["status"]], what
            finally:
                close(P)


@pytest.mark.parametrize("k", [2, 3, 8, 40])
def test_no_preconditioner_is_cg_multi_bit_for_bit(gpu, banded, k):
    row_ptr, col, val, _, B_all = banded
    B = np.ascontiguousarray(B_all[:, :k])
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        for iters, tol in ((25, 0.0), (60, 1e-6)):
            X_ref, h_ref, done, _ = dev.cg_multi(B, iters, tol=tol)
            X, rr, rz, info, _ = dev.pcg_multi(B, iters, tol=tol)
            assert X.tobytes() == X_ref.tobytes() and rr.tobytes() == h_ref.tobytes(), (k, tol)
            assert rz.tobytes() == rr.tobytes()                       # z is r
            assert np.array_equal(info["steps"], done), (k, tol, info, done)
            converged = (rr[-1] <= tol * tol * rr[0]) if tol else np.zeros(k, dtype=bool)
            assert np.array_equal(info["status"], np.where(converged, sp.PCG_CONVERGED, sp.PCG_RAN_ALL)), (k, tol, info)
            assert converged.any() == bool(tol)                       # the tol run does stop columns


@pytest.mark.parametrize("spec", PRECONDS, ids=PRECOND_IDS)
def test_permuting_columns_permutes_everything_bit_for_bit(gpu, banded, spec):
    row_ptr, col, val, _, B_all = banded
    B = np.ascontiguousarray(B_all[:, :8])
    B[:, 6] *= 1e-3                                                   # columns that stop at different steps
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        P = make_precond(dev, spec)
        try:
            for iters, tol in ((25, 0.0), (40, 1e-4)):
                X, rr, rz, info, _ = dev.pcg_multi(B, iters, tol=tol, precond=P)
                X2, rr2, rz2, info2, _ = dev.pcg_multi(B, iters, tol=tol, precond=P)
                assert X2.tobytes() == X.tobytes() and rr2.tobytes() == rr.tobytes() and rz2.tobytes() == rz.tobytes()
                assert np.array_equal(info2["steps"], info["steps"]) and np.array_equal(info2["status"], info["status"])
                Xp, rrp, rzp, infop, _ = dev.pcg_multi(np.ascontiguousarray(B[:, perm]), iters, tol=tol, precond=P)
                assert Xp.tobytes() == np.ascontiguousarray(X[:, perm]).tobytes()
                assert rrp.tobytes() == np.ascontiguousarray(rr[:, perm]).tobytes()
                assert rzp.tobytes() == np.ascontiguousarray(rz[:, perm]).tobytes()
                assert np.array_equal(infop["steps"], info["steps"][perm])
                assert np.array_equal(infop["status"], info["status"][perm])
        finally:
            close(P)


@pytest.mark.parametrize("k", [2, 3, 8, 40])
def test_each_column_is_that_columns_pcg(gpu, oracle, banded, k):
    """k = 3: element loads with idle column lanes; k = 2, 8: 16-byte loads; k = 40 crosses the SpMM's 32-column tile."""
    row_ptr, col, val, _, B_all = banded
    B = np.ascontiguousarray(B_all[:, :k])
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        for spec, name in zip(PRECONDS, PRECOND_IDS):
            P = make_precond(dev, spec)
            try:
                assert_matches_pcg_columns(dev, B, 5, P, f"k={k} {name}")
                X, rr, _, info = assert_matches_pcg_columns(dev, B, 25, P, f"k={k} {name}")
                assert info["steps"].tolist() == [25] * k and info["status"].tolist() == [sp.PCG_RAN_ALL] * k
                assert_true_residual(oracle, row_ptr, col, val, B, X, rr)
            finally:
                close(P)


def scipy_csr(triple, n):
    import scipy.sparse as sps
    rp, col, val = triple
    return sps.csr_matrix((val.astype(np.float64), col, rp), shape=(n, n))


def fsai_reference(P, R, n):
    """(G^T (G R) in fp64 from the stored factors, its row-wise bound).  fp64: the SpMM tests' 1e-10 sum |a_ij x_j| with
    both products' terms, 1e-10 (|G^T| (|G| |R|))_i.  fp32: their Higham bound (gamma32(n_i) + gamma64(n_i)) sum |a_ij x_j|
    (_util.f32_row_bound) once per product: e = bound of t = G R, then bound of G^T t on |t| + e plus |G^T| e, what the
    error of t becomes in z; 1e-6 more for this evaluation itself in fp64."""
    G, Gt = (scipy_csr(t, n) for t in P.factors())
    R64 = R.astype(np.float64)
    t = G @ R64
    ref = Gt @ t
    if R.dtype == np.float64:
        return ref, FP64_RTOL * (abs(Gt) @ (abs(G) @ np.abs(R64)))
    g = lambda A: (gamma(np.diff(A.indptr), U32) + gamma(np.diff(A.indptr), U64))[:, None]   # noqa: E731
    e = g(G) * (abs(G) @ np.abs(R64))
    return ref, (g(Gt) * (abs(Gt) @ (np.abs(t) + e)) + abs(Gt) @ e) * (1.0 + 1e-6)


@pytest.mark.parametrize("n", [1, 5, 6001])
def test_apply_multi_alone(gpu, n):
    """Column j of apply_multi(R) is apply(R[:, j]) bit for bit for Jacobi and block-Jacobi (the same sum order; blocks
    of 3 and of 32 both end in a short block at these sizes) and for FSAI at k = 1; FSAI at k > 1, fp64 and fp32,
    against G^T (G R) in numpy from the stored factors, row by row within fsai_reference's bound, and in fp64 norm-wise
    within 1e-10 max |ref| as well."""
    rng = np.random.default_rng(77 + n)
    row_ptr, col, val = spd_banded(rng, n, 7, 60)
    for dtype in (np.float64, np.float32):
        with sp.CsrDevice(n, n, row_ptr, col, val.astype(dtype)) as dev:
            for spec, name in zip(PRECONDS[1:], PRECOND_IDS[1:]):
                P = make_precond(dev, spec)
                try:
                    for k in (1, 3, 8):
                        R = rng.uniform(-1, 1, (n, k)).astype(dtype)
                        Z = P.apply_multi(R)
                        assert Z.shape == (n, k) and Z.dtype == dtype
                        what = f"n={n} k={k} {name} {np.dtype(dtype)}"
                        if spec[0] != "fsai" or k == 1:
                            for j in range(k):
                                z = P.apply(np.ascontiguousarray(R[:, j]))
                                assert np.ascontiguousarray(Z[:, j]).tobytes() == z.tobytes(), (what, j)
                        else:
                            ref, bound = fsai_reference(P, R, n)
                            d = np.abs(Z.astype(np.float64) - ref)
                            print(f"{what}: worst |d| / bound = {np.max(d / bound):.3e}")
                            assert np.all(np.isfinite(Z)) and np.all(d <= bound), what
                            if dtype == np.float64:
                                assert d.max() <= FP64_RTOL * np.abs(ref).max(), what
                finally:
                    close(P)


def test_columns_stop_on_their_own_and_the_loop_ends_early(gpu, oracle, banded):
    """tol = 1e-6 with columns of very different difficulty (an eigenvector of A, a sum of two, a tiny multiple and a
    multiple of another column, a zero column): every column stops where its own pcg run stops (+-1 where the reduction
    order could flip the comparison with tol), the histories then repeat, and a budget fifty times larger costs no more."""
    import scipy.sparse as sps
    from scipy.sparse.linalg import eigsh
    row_ptr, col, val, _, B_all = banded
    A = sps.csr_matrix((val, col, row_ptr), shape=(N, N))
    _, vecs = eigsh(A, k=2, which="LA", tol=1e-14, v0=np.ones(N))
    B = np.ascontiguousarray(np.column_stack([B_all[:, 0], vecs[:, 0], 1e-8 * B_all[:, 1], vecs[:, 0] + vecs[:, 1],
                                              np.zeros(N), B_all[:, 2], 3.0 * B_all[:, 0]]))
    k, tol, iters = B.shape[1], 1e-6, 200
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        for spec, name in zip(PRECONDS, PRECOND_IDS):
            P = make_precond(dev, spec)
            try:
                X, rr, rz, info, ms = dev.pcg_multi(B, iters, tol=tol, precond=P)
                steps, status = info["steps"], info["status"]
                _, _, _, steps_ref, status_ref = pcg_columns(dev, B, iters, P, tol=tol)
                print(f"{name}: steps {steps.tolist()} against pcg's {steps_ref.tolist()}")
                assert status.tolist() == [sp.PCG_CONVERGED] * k and np.array_equal(status, status_ref), name
                assert np.all(np.abs(steps - steps_ref) <= 1), (name, steps, steps_ref)
                assert steps.max() < iters and len(set(steps.tolist())) >= (3 if P is None else 2), (name, steps)
                # (b) the zero column: converged at step 0 with x = 0 exactly
                assert steps[4] == 0 and np.all(X[:, 4] == 0.0) and np.all(rr[:, 4] == 0.0) and np.all(rz[:, 4] == 0.0)
                assert np.all(np.isfinite(X)) and np.all(np.isfinite(rr)) and np.all(np.isfinite(rz))
                for j in range(k):
                    t = int(steps[j])
                    assert np.all(rr[t:, j] == rr[t, j]) and np.all(rz[t:, j] == rz[t, j]), (name, j)
                    assert rr[t, j] <= tol * tol * rr[0, j] and np.all(rr[1:t, j] > tol * tol * rr[0, j]), (name, j)
                assert_true_residual(oracle, row_ptr, col, val, B, X, rr)
                Xb, rrb, rzb, infob, ms_big = dev.pcg_multi(B, 50 * iters, tol=tol, precond=P)
                assert Xb.tobytes() == X.tobytes() and np.array_equal(infob["steps"], steps)
                assert rrb[: iters + 1].tobytes() == rr.tobytes() and np.all(rrb[iters:] == rr[-1])
                assert rzb[: iters + 1].tobytes() == rz.tobytes() and np.all(rzb[iters:] == rz[-1])
                assert ms_big < 5.0 * ms + 2.0, (name, ms_big, ms)
            finally:
                close(P)


@pytest.mark.parametrize("k", [5, 8])
def test_a_column_that_breaks_down_harms_no_other(gpu, oracle, k):
    """A = diag(S, -S) with S SPD.  A column of B supported on the first half converges; one supported on the second
    half breaks down at step 0 (p.A p < 0 without a preconditioner, r.z < 0 with Jacobi) and keeps x = 0; the columns
    beside it agree with their own pcg runs."""
    import scipy.sparse as sps
    rng = np.random.default_rng(31)
    h = 3000
    rp, c, v = spd_banded(rng, h, 7, 60)
    S = sps.csr_matrix((v, c, rp), shape=(h, h))
    A = sps.block_diag([S, -S]).tocsr()
    A.sort_indices()
    row_ptr, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    n = 2 * h
    X_true = np.zeros((n, k))
    second = np.arange(k) % 2 == 1                                   # odd columns live on the negative half
    for j in range(k):
        (X_true[h:, j] if second[j] else X_true[:h, j])[:] = rng.uniform(-1, 1, h)
    B = products(oracle, row_ptr, col, val, X_true)
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev:
        for spec, name in zip(PRECONDS[:2], PRECOND_IDS[:2]):
            P = make_precond(dev, spec)
            try:
                X, rr, rz, info, _ = dev.pcg_multi(B, 100, tol=1e-6, precond=P)
                assert np.all(info["status"][~second] == sp.PCG_CONVERGED), (name, info)
                assert np.all(info["status"][second] == sp.PCG_BREAKDOWN) and np.all(info["steps"][second] == 0), (name, info)
                assert np.all(np.isfinite(X)) and np.all(X[:, second] == 0.0), name
                assert np.all(rr[:, second] == rr[0, second]) and np.all(rz[:, second] == rz[0, second])
                assert_columns_close(X[:, ~second], X_true[:, ~second], 1e-3, f"{name}: towards x_true")
                X5, _, _, info5 = assert_matches_pcg_columns(dev, B, 5, P, f"diag(S, -S) k={k} {name}")
                assert np.all(info5["status"][second] == sp.PCG_BREAKDOWN) and np.all(X5[:, second] == 0.0)
                assert np.all(info5["status"][~second] == sp.PCG_RAN_ALL) and np.all(info5["steps"][~second] == 5)
            finally:
                close(P)


@pytest.mark.parametrize("spec", PRECONDS, ids=PRECOND_IDS)
def test_a_nan_in_one_column_of_B_stays_in_that_column(gpu, banded, spec):
    """The column breaks down at step 0 with a finite x; the others are finite and agree with the same solve over B with
    that column zeroed, within the 5-step tolerance."""
    row_ptr, col, val, _, B_all = banded
    k, j = 8, 3
    B = np.ascontiguousarray(B_all[:, :k])
    B_nan, B_zero = B.copy(), B.copy()
    B_nan[1234, j] = np.nan
    B_zero[:, j] = 0.0
    others = [c for c in range(k) if c != j]
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        P = make_precond(dev, spec)
        try:
            X, rr, rz, info, _ = dev.pcg_multi(B_nan, 5, precond=P)
            X0, rr0, rz0, info0, _ = dev.pcg_multi(B_zero, 5, precond=P)
            assert info["status"][j] == sp.PCG_BREAKDOWN and info["steps"][j] == 0
            assert np.all(np.isfinite(X)) and np.all(X[:, j] == 0.0)
            assert info["steps"][others].tolist() == [5] * (k - 1)
            assert info["status"][others].tolist() == [sp.PCG_RAN_ALL] * (k - 1)
            assert np.all(np.isfinite(rr[:, others])) and np.all(np.isfinite(rz[:, others]))
            assert_columns_close(X[:, others], X0[:, others], 1e-10, "beside a NaN column")
            assert np.all(np.abs(rr[:, others] - rr0[:, others]) <= 1e-10 * rr0[0, others])
            assert np.all(np.abs(rz[:, others] - rz0[:, others]) <= 1e-10 * np.abs(rz0[0, others]))
        finally:
            close(P)


K_MCG_BLOCKS, K_NORM_BLOCKS, K_BLOCK = 2048, 512, 256    # cg_multi_kernels.hpp, solver_ops.hpp


@pytest.mark.parametrize("k,n", [(64, K_MCG_BLOCKS * 8 + 11), (1, K_NORM_BLOCKS * K_BLOCK + 300)])
def test_grid_edges(gpu, k, n):
    """k = 64 in fp64 is 32 column lanes and 8 rows per workgroup: the cap of 2048 workgroups is reached at 16384 rows,
    and at 16395 some lanes take a second row and some do not.  k = 1 keeps csr_pcg's cap of 512 workgroups of 256
    rows: just past it, and still csr_pcg's bits."""
    assert n in (16395, 131372)
    rng = np.random.default_rng(n)
    row_ptr, col, val = spd_banded(rng, n, 7, 60)
    B = rng.uniform(-1, 1, (n, k))
    with sp.CsrDevice(n, n, row_ptr, col, val) as dev:
        for spec, name in ((PRECONDS[1], "jacobi"), (PRECONDS[2], "block3")):
            P = make_precond(dev, spec)
            try:
                X, rr, rz, info = assert_matches_pcg_columns(dev, B, 5, P, f"n={n} k={k} {name}")
                if k == 1:
                    x, hrr, hrz, _, _ = dev.pcg(np.ascontiguousarray(B[:, 0]), 5, precond=P)
                    assert X[:, 0].tobytes() == x.tobytes() and rr[:, 0].tobytes() == hrr.tobytes()
                    assert rz[:, 0].tobytes() == hrz.tobytes()
            finally:
                close(P)


def test_single_rank_communicator_gives_the_same_bits(gpu, banded):
    """bounds = [0, n] with a communicator: the all-gatherv of P with bounds scaled by k, every set of k dot products
    all-gathered and added in rank order -- the bits of the run without one."""
    from sparsematrixvectormultiplication_amd.distributed import NativeComm
    row_ptr, col, val, _, B_all = banded
    specs = (("jacobi", 1), ("fsai", 32))
    cases = ((3, 25, 0.0), (8, 25, 0.0), (8, 40, 1e-6))
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        Ps = [make_precond(dev, s) for s in specs]
        try:
            plain = {(i, c): dev.pcg_multi(np.ascontiguousarray(B_all[:, :c[0]]), c[1], tol=c[2], precond=P)
                     for i, P in enumerate(Ps) for c in cases}
            comm = NativeComm(0, 1, lambda ident: ident)
            try:
                bounds = np.array([0, N], np.int32)
                for (i, c), (X, rr, rz, info, _) in plain.items():
                    Xg, rrg, rzg, infog, _ = dev.pcg_multi(np.ascontiguousarray(B_all[:, :c[0]]), c[1], tol=c[2],
                                                           precond=Ps[i], bounds=bounds)
                    assert Xg.tobytes() == X.tobytes() and rrg.tobytes() == rr.tobytes() and rzg.tobytes() == rz.tobytes()
                    assert np.array_equal(infog["steps"], info["steps"]) and np.array_equal(infog["status"], info["status"])
                with pytest.raises(sp.SpmvHipError, match="bounds"):
                    dev.pcg_multi(np.ascontiguousarray(B_all[:, :2]), 2, precond=Ps[0])   # a communicator needs them
            finally:
                comm.close()
        finally:
            for P in Ps:
                close(P)


class DeviceBuffer:
    """spmv_hip_malloc'd bytes, freed on exit."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        assert sp.lib().spmv_hip_malloc(C.byref(self.p), int(nbytes)) == 0

    def __enter__(self):
        return self.p.value

    def __exit__(self, *exc):
        sp.lib().spmv_hip_free(self.p)


def raw_pcg_multi(dev, P, k, B, iters=2):
    """past the Python checks, into the library"""
    n = B.shape[0]
    X = np.zeros((n, max(k, 1)))
    rr, rz = np.zeros((iters + 1, max(k, 1))), np.zeros((iters + 1, max(k, 1)))
    steps, status = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
    ms = C.c_float(0)
    rc = sp.lib().spmv_hip_csr_pcg_multi(dev.h, None if P is None else P.h, k, iters, 0.0, None,
                                         B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                         rr.ctypes.data_as(nat.c_double_p), rz.ctypes.data_as(nat.c_double_p),
                                         steps.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p),
                                         C.byref(ms))
    sp.device._check(rc, "spmv_hip_csr_pcg_multi")


def test_refused_calls_leave_the_handle_usable(gpu, oracle, banded):
    row_ptr, col, val, _, B_all = banded
    rng = np.random.default_rng(5)
    B = np.ascontiguousarray(B_all[:, :3])
    x = rng.uniform(-1, 1, N)
    y_ref = oracle.csr_serial(row_ptr, col, val, x)
    with sp.CsrDevice(N, N, row_ptr, col, val) as dev:
        jac = dev.preconditioner("jacobi")
        X_good, rr_good, _, _, _ = dev.pcg_multi(B, 5, precond=jac)

        def still_works(after):
            assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref)), after
            X, rr, _, _, _ = dev.pcg_multi(B, 5, precond=jac)
            assert X.tobytes() == X_good.tobytes() and rr.tobytes() == rr_good.tobytes(), after

        assert_matches_pcg_columns(dev, B, 5, jac, "before the refusals")
        for kind in ("ssor", "ilu0"):
            with dev.preconditioner(kind) as tri:
                with pytest.raises(sp.SpmvHipError, match="one right-hand side"):
                    dev.pcg_multi(B, 3, precond=tri)
                with pytest.raises(sp.SpmvHipError, match="one right-hand side"):
                    tri.apply_multi(B)
                with DeviceBuffer(B.nbytes + 128) as d_r, DeviceBuffer(B.nbytes + 128) as d_z:
                    with pytest.raises(sp.SpmvHipError, match="one right-hand side"):
                        tri.apply_multi_on(d_r, d_z, 3, d_work=d_r)
            still_works(kind)
        with pytest.raises(sp.SpmvHipError, match="k = 0"):
            raw_pcg_multi(dev, jac, 0, B)
        still_works("k = 0")
        with pytest.raises(sp.SpmvHipError, match="k = 65"):
            raw_pcg_multi(dev, jac, 65, np.zeros((N, 65)))
        still_works("k = 65")
        rp2 = np.arange(0, 51 * 4, 4, dtype=np.int32)
        c2 = rng.integers(0, 60, 50 * 4).astype(np.int32)
        with sp.CsrDevice(50, 60, rp2, c2, rng.uniform(-1, 1, 200)) as rect:
            with pytest.raises(sp.SpmvHipError, match="square"):
                rect.pcg_multi(np.ones((50, 2)), 2)
        still_works("a non-square handle")
        small_rp, small_col, small_val = spd_banded(rng, 500, 5, 20)
        with sp.CsrDevice(500, 500, small_rp, small_col, small_val) as small, \
                sp.CsrDevice(N, N, row_ptr, col, val.astype(np.float32)) as dev32:
            for other, what in ((small, "another size"), (dev32, "another dtype")):
                with other.preconditioner("jacobi") as P_other:
                    with pytest.raises(sp.SpmvHipError, match="the preconditioner covers rows"):
                        raw_pcg_multi(dev, P_other, 3, B)
                still_works(what)
        with dev.preconditioner("fsai") as fsai:
            with DeviceBuffer(B.nbytes + 128) as d_r, DeviceBuffer(B.nbytes + 128) as d_z:
                with pytest.raises(sp.SpmvHipError, match="d_work"):
                    fsai.apply_multi_on(d_r, d_z, 3)
            still_works("FSAI without d_work")
            # and with d_work the device form gives the host form's bits
            R = rng.uniform(-1, 1, (N, 3))
            Z = np.zeros_like(R)
            L = sp.lib()
            with DeviceBuffer(R.nbytes + 128) as d_r, DeviceBuffer(R.nbytes) as d_z, DeviceBuffer(R.nbytes + 128) as d_w:
                assert L.spmv_hip_memset(C.c_void_p(d_r), 0, R.nbytes + 128) == 0
                assert L.spmv_hip_memcpy_h2d(C.c_void_p(d_r), R.ctypes.data_as(C.c_void_p), R.nbytes) == 0
                fsai.apply_multi_on(d_r, d_z, 3, d_work=d_w)
                sp.hip_sync()
                assert L.spmv_hip_memcpy_d2h(Z.ctypes.data_as(C.c_void_p), C.c_void_p(d_z), Z.nbytes) == 0
            assert Z.tobytes() == fsai.apply_multi(R).tobytes()
        jac.close()
