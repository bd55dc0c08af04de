"""numpy restatements of spmv_lobpcg_rr and of the loop of spmv_hip_csr_lobpcg (include/spmv_hip.h), shared by
test_lobpcg_host.py and test_gpu_lobpcg.py, and the test matrices of both."""
import numpy as np

DROP = 1e-10
RAN_ALL, CONVERGED, BREAKDOWN = 0, 1, 2


def rr_ref(GB, GA, nb, k, largest=False, drop=DROP):
    """(theta, C, Cp, kept, restarted), or None for a breakdown."""
    m = nb * k
    if not (np.isfinite(GB).all() and np.isfinite(GA).all()):
        return None
    B, A = (GB + GB.T) / 2, (GA + GA.T) / 2

    def basis(mm):
        d = np.diag(B)[:mm]
        ok = d > 1e-290
        dinv = np.where(ok, 1.0 / np.sqrt(np.where(ok, d, 1.0)), 0.0)
        L, V = np.linalg.eigh(dinv[:, None] * B[:mm, :mm] * dinv[None, :])
        keep = (L > drop * L.max()) & (L.max() > 0)
        return dinv[:, None] * V[:, keep] / np.sqrt(L[keep])

    mm, restarted = m, 0
    T = basis(mm)
    if T.shape[1] < mm and nb == 3:
        mm, restarted = 2 * k, 1
        T = basis(mm)
    kept = T.shape[1]
    if kept < k:
        return None
    H = T.T @ A[:mm, :mm] @ T
    ritz, Z = np.linalg.eigh((H + H.T) / 2)
    idx = kept - 1 - np.arange(k) if largest else np.arange(k)
    C = np.zeros((m, k))
    C[:mm] = T @ Z[:, idx]
    Cp = C.copy()
    Cp[:k] = 0
    nrm2 = np.einsum("ij,ij->j", Cp, B @ Cp)
    pos = nrm2 > 0
    Cp = Cp * np.where(pos, 1.0 / np.sqrt(np.where(pos, nrm2, 1.0)), 0.0)
    return ritz[idx], C, Cp, kept, restarted


def lobpcg_ref(A, X0, iters, tol=0.0, largest=False, minv=None, reverse=False):
    """The documented loop with numpy products (A: scipy sparse).  minv: R -> M^-1 R, or None.  reverse: the Gram sums
    take the rows in reversed order (another rounding of the same sums).  Returns (w, X, theta_hist, res_hist, info)."""
    n, k = X0.shape
    anorm = float(abs(A).sum(axis=1).max()) if A.nnz else 0.0

    def gram(S, AS):
        if reverse:
            S, AS = S[::-1], AS[::-1]
        S, AS = np.ascontiguousarray(S), np.ascontiguousarray(AS)
        return S.T @ S, S.T @ AS

    th, rh = np.zeros((iters + 1, k)), np.zeros((iters + 1, k))
    info = {"steps": 0, "status": RAN_ALL, "restarts": 0, "min_basis": k, "anorm": anorm}
    X = X0.copy()
    AX = A @ X
    out = rr_ref(*gram(X, AX), 1, k, largest)
    if out is None:
        info["status"] = BREAKDOWN
        return np.zeros(k), np.zeros((n, k)), th, rh, info
    theta, C = out[0], out[1]
    X, AX = X @ C, AX @ C
    P = AP = None
    t = 0
    while True:
        R = AX - X * theta
        th[t], rh[t] = theta, np.linalg.norm(R, axis=0)
        if not np.isfinite(rh[t]).all():
            info["status"] = BREAKDOWN
            break
        if tol > 0 and (rh[t] <= tol * anorm).all():
            info["status"] = CONVERGED
            break
        if t == iters:
            break
        W = minv(R) if minv is not None else R
        AW = A @ W
        nb = 2 if P is None else 3
        S = np.hstack([X, W] if P is None else [X, W, P])
        AS = np.hstack([AX, AW] if P is None else [AX, AW, AP])
        out = rr_ref(*gram(S, AS), nb, k, largest)
        if out is None:
            info["status"] = BREAKDOWN
            break
        theta, C, Cp, kept, restarted = out
        info["restarts"] += restarted
        info["min_basis"] = min(info["min_basis"], kept)
        X, P, AX, AP = S @ C, S @ Cp, AS @ C, AS @ Cp
        t += 1
    info["steps"] = t
    th[t + 1:], rh[t + 1:] = th[t], rh[t]
    return theta, X, th, rh, info


def lap(g1, g2, seed=1):
    """I (x) T_g2 + 1.3 T_g1 (x) I + diag(u), T = tridiag(-1, 2, -1), u uniform in [0, 0.05]: n = g1 g2, CSR."""
    import scipy.sparse as sps
    T = lambda g: sps.diags([-np.ones(g - 1), 2 * np.ones(g), -np.ones(g - 1)], [-1, 0, 1])  # noqa: E731
    u = np.random.default_rng(seed).uniform(0, 0.05, g1 * g2)
    A = sps.kron(sps.identity(g1), T(g2)) + 1.3 * sps.kron(T(g1), sps.identity(g2)) + sps.diags(u)
    A = sps.csr_matrix(A)
    A.sort_indices()
    return A


def scaled_lap(g1=24, g2=31, spread=100.0, seed=5):
    """D lap D with D^2 log-uniform over a factor `spread`."""
    import scipy.sparse as sps
    A = lap(g1, g2)
    d = np.sqrt(np.exp(np.random.default_rng(seed).uniform(0, np.log(spread), A.shape[0])))
    A = sps.csr_matrix(sps.diags(d) @ A @ sps.diags(d))
    A.sort_indices()
    return A
