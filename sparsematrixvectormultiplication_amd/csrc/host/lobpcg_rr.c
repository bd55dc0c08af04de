/* lobpcg_rr.c -- spmv_lobpcg_rr: the Rayleigh-Ritz step of LOBPCG on the two Gram matrices (include/spmv_hip.h).
 *
 * Host only, no device call, no LAPACK: the two symmetric eigenproblems (at most 48 x 48) are solved by Householder
 * tridiagonalisation and implicit QL with the eigenvectors accumulated (the classical tred2 / tql2 pair), eigenvalues
 * sorted ascending.  Everything is a fixed sequence of operations on its input: equal input, equal bits. */
#include <math.h>
#include <string.h>

#include "spmv_hip.h"

#define RR_MAX 48 /* 3 blocks of at most 16 columns */
#define RR_TINY 1e-290

/* a (n x n, row stride RR_MAX, symmetric; overwritten by the eigenvectors as columns) -> d ascending.  0, or 1 when
 * the QL sweeps do not settle (cannot happen for finite input; the caller reports a breakdown). */
static int sym_eig(int n, double a[RR_MAX][RR_MAX], double *d) {
    double e[RR_MAX];
    if (n == 1) {
        d[0] = a[0][0];
        a[0][0] = 1.0;
        return 0;
    }
    /* Householder reduction to tridiagonal form */
    for (int j = 0; j < n; ++j) d[j] = a[n - 1][j];
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) {
                d[j] = a[i - 1][j];
                a[i][j] = 0.0;
                a[j][i] = 0.0;
            }
        } else {
            for (int k = 0; k < i; ++k) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1], g = sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                a[j][i] = f;
                g = e[j] + a[j][j] * f;
                for (int k = j + 1; k <= i - 1; ++k) {
                    g += a[k][j] * d[k];
                    e[k] += a[k][j] * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; ++k) a[k][j] -= f * e[k] + g * d[k];
                d[j] = a[i - 1][j];
                a[i][j] = 0.0;
            }
        }
        d[i] = h;
    }
    /* accumulate the transformations */
    for (int i = 0; i < n - 1; ++i) {
        a[n - 1][i] = a[i][i];
        a[i][i] = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = a[k][i + 1] / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                for (int k = 0; k <= i; ++k) g += a[k][i + 1] * a[k][j];
                for (int k = 0; k <= i; ++k) a[k][j] -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) a[k][i + 1] = 0.0;
    }
    for (int j = 0; j < n; ++j) {
        d[j] = a[n - 1][j];
        a[n - 1][j] = 0.0;
    }
    a[n - 1][n - 1] = 1.0;
    e[0] = 0.0;
    /* implicit QL on the tridiagonal matrix */
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; ++l) {
        const double t = fabs(d[l]) + fabs(e[l]);
        if (t > tst1) tst1 = t;
        int m = l;
        while (m < n - 1 && fabs(e[m]) > eps * tst1) ++m;
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 120) return 1;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    for (int k = 0; k < n; ++k) {
                        h = a[k][i + 1];
                        a[k][i + 1] = s * a[k][i] + c * h;
                        a[k][i] = c * a[k][i] - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    /* ascending order (selection sort: the columns move with their values) */
    for (int i = 0; i < n - 1; ++i) {
        int kmin = i;
        for (int j = i + 1; j < n; ++j)
            if (d[j] < d[kmin]) kmin = j;
        if (kmin != i) {
            const double t = d[i];
            d[i] = d[kmin];
            d[kmin] = t;
            for (int r = 0; r < n; ++r) {
                const double v = a[r][i];
                a[r][i] = a[r][kmin];
                a[r][kmin] = v;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        if (!isfinite(d[i])) return 1;
    return 0;
}

/* the orthonormalising map of the leading mm x mm block of B: T = D V_keep L_keep^-1/2 (mm x *nk).  Returns 0, or 1 when
 * the eigensolver fails. */
static int basis_map(int mm, const double B[RR_MAX][RR_MAX], double drop, double T[RR_MAX][RR_MAX], int *nk) {
    static _Thread_local double V[RR_MAX][RR_MAX];
    double dinv[RR_MAX], L[RR_MAX];
    for (int i = 0; i < mm; ++i) dinv[i] = B[i][i] > RR_TINY ? 1.0 / sqrt(B[i][i]) : 0.0;
    for (int i = 0; i < mm; ++i)
        for (int j = 0; j < mm; ++j) V[i][j] = dinv[i] * B[i][j] * dinv[j];
    if (sym_eig(mm, V, L)) return 1;
    const double lmax = L[mm - 1];
    int kept = 0;
    for (int i = 0; i < mm; ++i) {
        if (!(lmax > 0.0) || !(L[i] > drop * lmax)) continue;
        const double s = 1.0 / sqrt(L[i]);
        for (int r = 0; r < mm; ++r) T[r][kept] = dinv[r] * V[r][i] * s;
        ++kept;
    }
    *nk = kept;
    return 0;
}

int spmv_lobpcg_rr(int nb, int k, const double *GB, const double *GA, int largest, double drop, double *theta,
                   double *C, double *Cp, int *kept, int *restarted) {
    if (nb < 1 || nb > 3 || k < 1 || k > RR_MAX / 3 || !GB || !GA || !theta || !C || !Cp || !(drop >= 0.0) || !(drop < 1.0))
        return -1;
    static _Thread_local double B[RR_MAX][RR_MAX], A[RR_MAX][RR_MAX], T[RR_MAX][RR_MAX], H[RR_MAX][RR_MAX],
        W[RR_MAX][RR_MAX];
    const int m = nb * k;
    if (kept) *kept = 0;
    if (restarted) *restarted = 0;
    memset(theta, 0, (size_t)k * sizeof(double));
    memset(C, 0, (size_t)m * k * sizeof(double));
    memset(Cp, 0, (size_t)m * k * sizeof(double));
    for (int i = 0; i < m * m; ++i)
        if (!isfinite(GB[i]) || !isfinite(GA[i])) return SPMV_LOBPCG_RR_BREAKDOWN;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            B[i][j] = 0.5 * (GB[i * m + j] + GB[j * m + i]);
            A[i][j] = 0.5 * (GA[i * m + j] + GA[j * m + i]);
        }
    int mm = m, nk = 0;
    if (basis_map(mm, B, drop, T, &nk)) return SPMV_LOBPCG_RR_BREAKDOWN;
    if (nk < mm && nb == 3) { /* a restart without P: the leading [X | W] blocks alone */
        mm = 2 * k;
        if (restarted) *restarted = 1;
        if (basis_map(mm, B, drop, T, &nk)) return SPMV_LOBPCG_RR_BREAKDOWN;
    }
    if (kept) *kept = nk;
    if (nk < k) return SPMV_LOBPCG_RR_BREAKDOWN;
    /* H = T^T A T (nk x nk), symmetrised */
    for (int i = 0; i < mm; ++i)
        for (int j = 0; j < nk; ++j) {
            double s = 0.0;
            for (int r = 0; r < mm; ++r) s += A[i][r] * T[r][j];
            W[i][j] = s;
        }
    for (int i = 0; i < nk; ++i)
        for (int j = 0; j < nk; ++j) {
            double s = 0.0;
            for (int r = 0; r < mm; ++r) s += T[r][i] * W[r][j];
            H[i][j] = s;
        }
    for (int i = 0; i < nk; ++i)
        for (int j = i + 1; j < nk; ++j) H[i][j] = H[j][i] = 0.5 * (H[i][j] + H[j][i]);
    double ritz[RR_MAX];
    if (sym_eig(nk, H, ritz)) return SPMV_LOBPCG_RR_BREAKDOWN;
    /* the k smallest ascending, or the k largest descending; C = T Z_k, rows from mm on stay 0 */
    for (int j = 0; j < k; ++j) {
        const int src = largest ? nk - 1 - j : j;
        theta[j] = ritz[src];
        for (int r = 0; r < mm; ++r) {
            double s = 0.0;
            for (int q = 0; q < nk; ++q) s += T[r][q] * H[q][src];
            C[r * k + j] = s;
        }
    }
    /* Cp: C without its X rows, every column scaled to unit B norm (a zero column stays 0) */
    for (int j = 0; j < k; ++j) {
        double nrm2 = 0.0;
        for (int r = k; r < mm; ++r) {
            double s = 0.0;
            for (int q = k; q < mm; ++q) s += B[r][q] * C[q * k + j];
            nrm2 += C[r * k + j] * s;
        }
        const double scale = nrm2 > 0.0 && isfinite(nrm2) ? 1.0 / sqrt(nrm2) : 0.0;
        for (int r = k; r < mm; ++r) Cp[r * k + j] = scale > 0.0 && isfinite(scale) ? C[r * k + j] * scale : 0.0;
    }
    for (int i = 0; i < m * k; ++i)
        if (!isfinite(C[i]) || !isfinite(Cp[i])) return SPMV_LOBPCG_RR_BREAKDOWN;
    return 0;
}
