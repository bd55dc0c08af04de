"""The loop spmv_hip_csr_gmres runs (include/spmv_hip.h), restated in numpy fp64 with a given product and a given
apply: restarted GMRES(m), right-preconditioned, classical Gram-Schmidt done twice, x0 = 0."""
import numpy as np

RAN_ALL, CONVERGED, BREAKDOWN = 0, 1, 2   # SPMV_GMRES_* (sp.GMRES_*)


def forward_dot(a, b):
    """a.b added row by row from row 0 on."""
    s = 0.0
    for v in (a * b).tolist():
        s += v
    return s


def reversed_dot(a, b):
    """a.b added row by row from the last row down."""
    return forward_dot(a[::-1], b[::-1])


def gmres_ref(spmv, b, iters, tol=0.0, restart=30, minv=None, dot=np.dot):
    """Returns (x, history [iters + 1] of the squared residual estimate, info {"steps", "status", "cycles"}).
    spmv(v) = A v; minv(v) = M^-1 v or None; dot(a, b): the dot product every sum of the loop goes through."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.zeros(n)
    rr0 = float(dot(b, b))
    hist = [rr0]
    tol2 = tol * tol
    t, cycles = 0, 0

    def done(status):
        return x, np.array(hist + [hist[-1]] * (iters + 1 - len(hist))), {"steps": t, "status": status, "cycles": cycles}

    if rr0 == 0.0:
        return done(CONVERGED)
    if not np.isfinite(rr0):
        return done(BREAKDOWN)
    while True:
        cycles += 1
        r = b - spmv(x) if cycles > 1 else b.copy()
        beta = float(np.sqrt(dot(r, r)))
        if not np.isfinite(beta):
            return done(BREAKDOWN)
        if beta == 0.0:
            return done(CONVERGED)
        V = [r / beta]
        g = np.zeros(restart + 1)
        g[0] = beta
        R = np.zeros((restart, restart))
        cs, sn = np.zeros(restart), np.zeros(restart)
        J, status = 0, RAN_ALL
        for j in range(restart):
            if t >= iters:
                break
            z = V[j] if minv is None else np.asarray(minv(V[j]), dtype=np.float64)
            w = np.asarray(spmv(z), dtype=np.float64)
            h = np.array([float(dot(V[i], w)) for i in range(j + 1)])
            s = np.zeros(n)
            for i in range(j + 1):
                s = s + h[i] * V[i]
            w = w - s
            h2 = np.array([float(dot(V[i], w)) for i in range(j + 1)])
            s = np.zeros(n)
            for i in range(j + 1):
                s = s + h2[i] * V[i]
            w = w - s
            ww = float(dot(w, w))
            col = h + h2
            with np.errstate(all="ignore"):
                eta = float(np.sqrt(ww))
                ok = bool(np.isfinite(eta) and np.all(np.isfinite(col)))
                for i in range(j):
                    a, c = col[i], col[i + 1]
                    col[i] = cs[i] * a + sn[i] * c
                    col[i + 1] = -sn[i] * a + cs[i] * c
                hj = col[j]
                d = float(np.hypot(hj, eta))
                c_j, s_j = (hj / d, eta / d) if d != 0.0 else (np.nan, np.nan)
                gn = -s_j * g[j]
                rr = gn * gn
                ok = ok and bool(np.all(np.isfinite(col))) and d != 0.0 and \
                    all(np.isfinite(v) for v in (d, c_j, s_j, gn, rr))
            if not ok:
                status = BREAKDOWN
                break
            col[j] = d
            R[: j + 1, j] = col
            cs[j], sn[j] = c_j, s_j
            g[j] = c_j * g[j]
            g[j + 1] = gn
            t += 1
            J = j + 1
            hist.append(rr)
            if rr <= tol2 * rr0:
                status = CONVERGED
                break
            if eta != 0.0:
                V.append(w / eta)
        if J:
            y = np.zeros(J)
            for i in range(J - 1, -1, -1):
                s = g[i]
                for k in range(i + 1, J):
                    s -= R[i, k] * y[k]
                y[i] = s / R[i, i]
            u = np.zeros(n)
            for i in range(J):
                u = u + y[i] * V[i]
            x = x + (u if minv is None else np.asarray(minv(u), dtype=np.float64))
        if status != RAN_ALL:
            return done(status)
        if t >= iters:
            return done(RAN_ALL)
