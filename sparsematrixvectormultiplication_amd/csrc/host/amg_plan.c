/*
 * amg_plan.c -- the host setup of the smoothed-aggregation AMG preconditioner (include/spmv_hip.h: spmv_amg_plan_*):
 * the hierarchy A_0 .. A_L with its prolongations P_l, restrictions R_l = P_l^T, damping factors w_l and the dense
 * inverse of a DIRECT coarsest level.  Plain C, fp64, one thread, no device: two builds give the same bytes.  It runs
 * once per build (spmv_amg.hip) on the canonical diagonal block of a handle (canon_rows.hpp: sorted columns, repeats
 * added), and tests call it directly.
 *
 * Level l (A = A_l, n rows, d_i = a_ii):
 *   1. d_i present, finite and > 0, else refused (level 0 names the row, deeper levels the level)
 *   2. rho = max_i (sum_j |a_ij|) / d_i in stored order (Gershgorin for D^-1 A), w = 4 / (3 rho)
 *   3. n <= coarse_rows: DIRECT, the inverse by Gauss-Jordan with partial pivoting (the first largest |pivot| wins)
 *   4. l + 1 == max_levels: SMOOTH
 *   5. strong (i, j), i != j: a_ij != 0 and |a_ij| >= theta sqrt(d_i d_j); the graph has an edge when either direction
 *      is strong; neighbours ascending
 *   6. three passes in row order: (a) a row with neighbours, itself and all of them free, starts an aggregate of
 *      itself and them; (b) a free row joins the aggregate its first neighbour had after (a); (c) a free row with
 *      neighbours starts an aggregate and takes its free neighbours along.  Rows without neighbours stay outside.
 *   7. na == 0 or 10 na > 9 n: SMOOTH
 *   8. T[i, agg(i)] = 1;  P = T - diag(w / d_i) A T on the pattern of A T (cancelled entries stay);  R = P^T;
 *      A_{l+1} = R (A P).  Every sum in ascending column order, the first term the plain product.
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "amg_plan_parts.h"
#include "spmv_hip.h"

typedef struct {
    amg_csr A, P, R, T;
    double *inv; /* DIRECT: rows x rows, row-major */
    double w, rho;
    int kind, na; /* SPMV_AMG_NOT_COARSEST / _DIRECT / _SMOOTH; aggregates */
} amg_level;

struct spmv_amg_plan {
    int levels;
    amg_level lv[16];
};

static _Thread_local char g_msg[200];

static int refuse(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return -1;
}

const char *spmv_amg_plan_error(void) { return g_msg; }

static void csr_release(amg_csr *m) {
    free(m->rp);
    free(m->col);
    free(m->val);
    memset(m, 0, sizeof *m);
}

static int csr_alloc(amg_csr *m, int rows, int cols, size_t nz) {
    m->rows = rows;
    m->cols = cols;
    m->rp = calloc((size_t)rows + 1, sizeof(int));
    m->col = malloc((nz ? nz : 1) * sizeof(int));
    m->val = malloc((nz ? nz : 1) * sizeof(double));
    return m->rp && m->col && m->val ? 0 : -1;
}

void spmv_amg_plan_free(spmv_amg_plan *p) {
    if (!p) return;
    for (int l = 0; l < 16; ++l) {
        csr_release(&p->lv[l].A);
        csr_release(&p->lv[l].P);
        csr_release(&p->lv[l].R);
        csr_release(&p->lv[l].T);
        free(p->lv[l].inv);
    }
    free(p);
}

static int by_int(const void *a, const void *b) {
    const int x = *(const int *)a, y = *(const int *)b;
    return x < y ? -1 : x > y;
}

/* C = A B, row by row over a dense accumulator: entry (i, c) adds a_ij b_jc with j ascending, the first term the plain
 * product; the pattern is structural (a sum that cancels stays), columns ascending */
static int csr_multiply(const amg_csr *A, const amg_csr *B, amg_csr *C) {
    const int n = A->rows, m = B->cols;
    double *acc = malloc(((size_t)m + 1) * sizeof(double));
    int *mark = malloc(((size_t)m + 1) * sizeof(int)), *list = malloc(((size_t)m + 1) * sizeof(int));
    int rc = -1;
    size_t nz = 0;
    if (!acc || !mark || !list) goto done;
    for (int c = 0; c < m; ++c) mark[c] = -1;
    for (int i = 0; i < n; ++i) { /* count */
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e)
            for (int f = B->rp[A->col[e]]; f < B->rp[A->col[e] + 1]; ++f)
                if (mark[B->col[f]] != i) mark[B->col[f]] = i, ++nz;
    }
    if (nz > 0x7fffffff) goto done;
    if (csr_alloc(C, n, m, nz)) goto done;
    for (int c = 0; c < m; ++c) mark[c] = -1;
    nz = 0;
    for (int i = 0; i < n; ++i) {
        int cnt = 0;
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e) {
            const int j = A->col[e];
            const double a = A->val[e];
            for (int f = B->rp[j]; f < B->rp[j + 1]; ++f) {
                const int c = B->col[f];
                if (mark[c] != i) {
                    mark[c] = i;
                    list[cnt++] = c;
                    acc[c] = a * B->val[f];
                } else {
                    acc[c] += a * B->val[f];
                }
            }
        }
        qsort(list, (size_t)cnt, sizeof(int), by_int);
        for (int q = 0; q < cnt; ++q) {
            C->col[nz] = list[q];
            C->val[nz++] = acc[list[q]];
        }
        C->rp[i + 1] = (int)nz;
    }
    rc = 0;
done:
    free(acc);
    free(mark);
    free(list);
    return rc;
}

/* B = A^T: the entries of a row of B in ascending column order (a counting pass over A's rows in order) */
static int csr_transpose(const amg_csr *A, amg_csr *B) {
    const size_t nz = (size_t)A->rp[A->rows];
    if (csr_alloc(B, A->cols, A->rows, nz)) return -1;
    for (size_t e = 0; e < nz; ++e) B->rp[A->col[e] + 1]++;
    for (int c = 0; c < A->cols; ++c) B->rp[c + 1] += B->rp[c];
    int *fill = malloc(((size_t)A->cols + 1) * sizeof(int));
    if (!fill) return -1;
    memcpy(fill, B->rp, ((size_t)A->cols + 1) * sizeof(int));
    for (int i = 0; i < A->rows; ++i)
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e) {
            const int q = fill[A->col[e]]++;
            B->col[q] = i;
            B->val[q] = A->val[e];
        }
    free(fill);
    return 0;
}

/* d[i] = a_ii (d NULL: not wanted) and *rho = max_i (sum_j |a_ij|) / a_ii, the sums in stored order, a NaN quotient
 * kept.  Returns -1, or the first row whose diagonal is not stored (*missing = 1) or not finite and > 0
 * (*missing = 0); rows behind it are not read (amg_plan_parts.h: the Chebyshev build calls it too) */
int amg_gershgorin(const amg_csr *A, double *d, double *rho, int *missing) {
    double top = 0.0;
    *missing = 0;
    for (int i = 0; i < A->rows; ++i) {
        double di = NAN, sum = 0.0;
        int have = 0;
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e) {
            if (A->col[e] == i) di = A->val[e], have = 1;
            sum += fabs(A->val[e]);
        }
        if (!have || !isfinite(di) || !(di > 0.0)) {
            *missing = !have;
            *rho = top;
            return i;
        }
        if (d) d[i] = di;
        const double q = sum / di;
        if (q > top || isnan(q)) top = q;
    }
    *rho = top;
    return -1;
}

/* inv = A^-1 dense by Gauss-Jordan on [A | I] with partial pivoting; 1: a zero or non-finite pivot; -1: no memory
 * (amg_plan_parts.h: the device setup calls it too) */
int amg_dense_inverse(const amg_csr *A, double **out) {
    const int n = A->rows, w = 2 * n;
    double *aug = calloc((size_t)n * w + 1, sizeof(double));
    double *inv = malloc(((size_t)n * n + 1) * sizeof(double));
    if (!aug || !inv) {
        free(aug);
        free(inv);
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e) aug[(size_t)i * w + A->col[e]] = A->val[e];
        aug[(size_t)i * w + n + i] = 1.0;
    }
    int bad = 0;
    for (int c = 0; c < n && !bad; ++c) {
        int p = c;
        double best = fabs(aug[(size_t)c * w + c]);
        for (int r = c + 1; r < n; ++r) {
            const double v = fabs(aug[(size_t)r * w + c]);
            if (v > best) best = v, p = r;
        }
        const double piv = aug[(size_t)p * w + c];
        if (!(best > 0.0) || !isfinite(piv)) {
            bad = 1;
            break;
        }
        if (p != c)
            for (int j = 0; j < w; ++j) {
                const double t = aug[(size_t)c * w + j];
                aug[(size_t)c * w + j] = aug[(size_t)p * w + j];
                aug[(size_t)p * w + j] = t;
            }
        for (int j = 0; j < w; ++j) aug[(size_t)c * w + j] = aug[(size_t)c * w + j] / piv;
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = aug[(size_t)r * w + c];
            for (int j = 0; j < w; ++j) aug[(size_t)r * w + j] = aug[(size_t)r * w + j] - f * aug[(size_t)c * w + j];
        }
    }
    for (int i = 0; i < n && !bad; ++i)
        for (int j = 0; j < n; ++j) {
            inv[(size_t)i * n + j] = aug[(size_t)i * w + n + j];
            if (!isfinite(inv[(size_t)i * n + j])) bad = 1;
        }
    free(aug);
    if (bad) {
        free(inv);
        return 1;
    }
    *out = inv;
    return 0;
}

/* the symmetrised strength graph of A: s_rp[n + 1], *s_col_out (allocated here), neighbours ascending */
static int strong(const amg_csr *A, const double *d, double theta, int i, int e) {
    const int j = A->col[e];
    const double a = A->val[e];
    return j != i && a != 0.0 && fabs(a) >= theta * sqrt(d[i] * d[j]);
}

static int strength_graph(const amg_csr *A, const double *d, double theta, int *s_rp, int **s_col_out) {
    const int n = A->rows;
    memset(s_rp, 0, ((size_t)n + 1) * sizeof(int));
    /* both directions of every strong entry, then every row sorted and its repeats dropped */
    for (int i = 0; i < n; ++i)
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e)
            if (strong(A, d, theta, i, e)) s_rp[i + 1]++, s_rp[A->col[e] + 1]++;
    for (int i = 0; i < n; ++i) s_rp[i + 1] += s_rp[i];
    int *s_col = malloc(((size_t)s_rp[n] + 1) * sizeof(int)), *fill = malloc(((size_t)n + 1) * sizeof(int));
    if (!s_col || !fill) {
        free(s_col);
        free(fill);
        return -1;
    }
    memcpy(fill, s_rp, ((size_t)n + 1) * sizeof(int));
    for (int i = 0; i < n; ++i)
        for (int e = A->rp[i]; e < A->rp[i + 1]; ++e)
            if (strong(A, d, theta, i, e)) s_col[fill[i]++] = A->col[e], s_col[fill[A->col[e]]++] = i;
    free(fill);
    int out = 0, begin = 0;
    for (int i = 0; i < n; ++i) {
        const int end = s_rp[i + 1], first = out;
        qsort(s_col + begin, (size_t)(end - begin), sizeof(int), by_int);
        for (int q = begin; q < end; ++q)
            if (out == first || s_col[out - 1] != s_col[q]) s_col[out++] = s_col[q];
        begin = end;
        s_rp[i + 1] = out;
    }
    *s_col_out = s_col;
    return 0;
}

/* agg[n] (-1: in no aggregate); returns the number of aggregates, -1 without memory (amg_plan_parts.h: the device
 * setup calls it too) */
int amg_aggregate(int n, const int *s_rp, const int *s_col, int *agg) {
    int na = 0;
    int *after_a = malloc(((size_t)n + 1) * sizeof(int));
    if (!after_a) return -1;
    for (int i = 0; i < n; ++i) agg[i] = -1;
    for (int i = 0; i < n; ++i) { /* (a) */
        if (agg[i] >= 0 || s_rp[i + 1] == s_rp[i]) continue;
        int is_free = 1;
        for (int q = s_rp[i]; q < s_rp[i + 1] && is_free; ++q) is_free = agg[s_col[q]] < 0;
        if (!is_free) continue;
        agg[i] = na;
        for (int q = s_rp[i]; q < s_rp[i + 1]; ++q) agg[s_col[q]] = na;
        ++na;
    }
    memcpy(after_a, agg, (size_t)n * sizeof(int));
    for (int i = 0; i < n; ++i) { /* (b) */
        if (agg[i] >= 0) continue;
        for (int q = s_rp[i]; q < s_rp[i + 1]; ++q)
            if (after_a[s_col[q]] >= 0) {
                agg[i] = after_a[s_col[q]];
                break;
            }
    }
    for (int i = 0; i < n; ++i) { /* (c) */
        if (agg[i] >= 0 || s_rp[i + 1] == s_rp[i]) continue;
        agg[i] = na;
        for (int q = s_rp[i]; q < s_rp[i + 1]; ++q)
            if (agg[s_col[q]] < 0) agg[s_col[q]] = na;
        ++na;
    }
    free(after_a);
    return na;
}

/* T and P = T - diag(w / d) A T of one level */
static int prolongation(const amg_csr *A, const double *d, double w, const int *agg, int na, amg_csr *T, amg_csr *P) {
    const int n = A->rows;
    int rows_in = 0;
    for (int i = 0; i < n; ++i) rows_in += agg[i] >= 0;
    if (csr_alloc(T, n, na, (size_t)rows_in)) return -1;
    for (int i = 0, q = 0; i < n; ++i) {
        if (agg[i] >= 0) T->col[q] = agg[i], T->val[q++] = 1.0;
        T->rp[i + 1] = q;
    }
    amg_csr AT;
    memset(&AT, 0, sizeof AT);
    if (csr_multiply(A, T, &AT)) {
        csr_release(&AT);
        return -1;
    }
    *P = AT; /* P takes A T's arrays */
    for (int i = 0; i < n; ++i) {
        const double g = w / d[i];
        for (int e = P->rp[i]; e < P->rp[i + 1]; ++e)
            P->val[e] = (P->col[e] == agg[i] ? 1.0 : 0.0) - g * P->val[e];
    }
    return 0;
}

int spmv_amg_plan_build(int n, const int *row_ptr, const int *col, const double *val, double theta, int coarse_rows,
                        int max_levels, spmv_amg_plan **out) {
    g_msg[0] = 0;
    if (!out) return refuse("amg_plan_build: out is NULL");
    *out = NULL;
    if (n < 0 || !row_ptr || (n && row_ptr[n] > 0 && (!col || !val))) return refuse("amg_plan_build: bad arguments");
    if (!(theta >= 0.0 && theta < 1.0)) return refuse("amg_plan_build: theta = %g, must be in [0, 1)", theta);
    if (coarse_rows < 1 || coarse_rows > 256)
        return refuse("amg_plan_build: coarse_rows = %d, must be in [1, 256]", coarse_rows);
    if (max_levels < 1 || max_levels > 16)
        return refuse("amg_plan_build: max_levels = %d, must be in [1, 16]", max_levels);
    if (row_ptr[0] != 0) return refuse("amg_plan_build: row_ptr[0] must be 0");
    for (int i = 0; i < n; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return refuse("amg_plan_build: row_ptr decreases at row %d", i);
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            if (col[e] < 0 || col[e] >= n || (e > row_ptr[i] && col[e] <= col[e - 1]))
                return refuse("amg_plan_build: row %d is not canonical (columns in [0, n), ascending, no repeats)", i);
    }
    spmv_amg_plan *p = calloc(1, sizeof *p);
    if (!p) return refuse("amg_plan_build: out of memory");
    int rc = 0, *s_rp = NULL, *s_col = NULL, *agg = NULL;
    double *d = NULL;
    if (n) {
        const size_t nz = (size_t)row_ptr[n];
        if (csr_alloc(&p->lv[0].A, n, n, nz)) goto nomem;
        memcpy(p->lv[0].A.rp, row_ptr, ((size_t)n + 1) * sizeof(int));
        if (nz) memcpy(p->lv[0].A.col, col, nz * sizeof(int)), memcpy(p->lv[0].A.val, val, nz * sizeof(double));
    }
    for (int l = 0; n && l < 16; ++l) {
        amg_level *L = &p->lv[l];
        const amg_csr *A = &L->A;
        const int nl = A->rows;
        p->levels = l + 1;
        free(d), free(s_rp), free(s_col), free(agg);
        s_col = NULL;
        d = malloc(((size_t)nl + 1) * sizeof(double));
        s_rp = malloc(((size_t)nl + 2) * sizeof(int));
        agg = malloc(((size_t)nl + 1) * sizeof(int));
        if (!d || !s_rp || !agg) goto nomem;
        double rho = 0.0;
        int missing = 0;
        const int bad_row = amg_gershgorin(A, d, &rho, &missing);
        if (bad_row >= 0) {
            const char *why = missing ? AMG_WHY_NO_DIAGONAL : AMG_WHY_BAD_DIAGONAL;
            if (l == 0) rc = refuse(AMG_REFUSE_ROW, bad_row, why);
            else rc = refuse(AMG_REFUSE_COARSE_ROW, l, bad_row, why);
            break;
        }
        if (!isfinite(rho) || !(rho > 0.0)) {
            rc = refuse(AMG_REFUSE_NOT_FINITE, l);
            break;
        }
        L->rho = rho;
        L->w = 4.0 / (3.0 * rho);
        if (nl <= coarse_rows) {
            L->kind = SPMV_AMG_DIRECT;
            const int bad = amg_dense_inverse(A, &L->inv);
            if (bad < 0) goto nomem;
            if (bad) rc = refuse(AMG_REFUSE_PIVOT, l, nl);
            break;
        }
        L->kind = SPMV_AMG_SMOOTH;
        if (l + 1 == max_levels) break;
        if (strength_graph(A, d, theta, s_rp, &s_col)) goto nomem;
        const int na = amg_aggregate(nl, s_rp, s_col, agg);
        if (na < 0) goto nomem;
        if (na == 0 || 10LL * na > 9LL * nl) break;
        L->kind = SPMV_AMG_NOT_COARSEST;
        L->na = na;
        amg_csr AP;
        memset(&AP, 0, sizeof AP);
        if (prolongation(A, d, L->w, agg, na, &L->T, &L->P) || csr_transpose(&L->P, &L->R) ||
            csr_multiply(A, &L->P, &AP) || csr_multiply(&L->R, &AP, &p->lv[l + 1].A)) {
            csr_release(&AP);
            goto nomem;
        }
        csr_release(&AP);
    }
    free(d), free(s_rp), free(s_col), free(agg);
    if (rc) {
        spmv_amg_plan_free(p);
        return rc;
    }
    *out = p;
    return 0;
nomem:
    free(d), free(s_rp), free(s_col), free(agg);
    spmv_amg_plan_free(p);
    return refuse(AMG_REFUSE_MEMORY);
}

int spmv_amg_plan_levels(const spmv_amg_plan *p) { return p ? p->levels : -1; }

/* first call: row_ptr = NULL fills scalars alone; second: col = val = NULL fills row_ptr; third: all three */
int spmv_amg_plan_level(const spmv_amg_plan *p, int level, int which, int *row_ptr, int *col, double *val,
                        double *scalars) {
    if (!p || level < 0 || level >= p->levels) return refuse("amg_plan_level: no level %d", level);
    const amg_level *L = &p->lv[level];
    if (scalars) {
        scalars[0] = L->w;
        scalars[1] = L->rho;
        scalars[2] = L->kind;
        scalars[3] = L->A.rows;
        scalars[4] = L->na;
    }
    if (!row_ptr) return 0;
    if (which == SPMV_AMG_INV) {
        const int n = L->A.rows;
        if (!L->inv) return refuse("amg_plan_level: level %d is not a DIRECT coarsest level", level);
        for (int i = 0; i <= n; ++i) row_ptr[i] = i * n;
        if (col && val)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) col[i * n + j] = j, val[i * n + j] = L->inv[(size_t)i * n + j];
        return 0;
    }
    const amg_csr *m = which == SPMV_AMG_A ? &L->A : which == SPMV_AMG_P ? &L->P : which == SPMV_AMG_R ? &L->R
                     : which == SPMV_AMG_T ? &L->T : NULL;
    if (!m) return refuse("amg_plan_level: which = %d", which);
    if (!m->rp) return refuse("amg_plan_level: level %d is the coarsest, it has no P, R or T", level);
    memcpy(row_ptr, m->rp, ((size_t)m->rows + 1) * sizeof(int));
    if (col && val && m->rp[m->rows]) {
        memcpy(col, m->col, (size_t)m->rp[m->rows] * sizeof(int));
        memcpy(val, m->val, (size_t)m->rp[m->rows] * sizeof(double));
    }
    return 0;
}
