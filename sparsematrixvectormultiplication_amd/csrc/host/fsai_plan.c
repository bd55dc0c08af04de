/*
 * fsai_plan.c -- the host pass of the FSAI preconditioner (include/spmv_hip.h: spmv_fsai_plan): which entries row i
 * of the factor G gets, and which lane width the device build gives the row.  One pass per row over its entries; it
 * runs once per build (spmv_fsai.hip) and needs no device.  The matrix is an n x n CSR matrix with local columns;
 * entries whose column lies outside [0, n) are ignored, rows need not be sorted and may repeat a column (repeats are
 * added in entry order in fp64, as the canonical rows of the build do: on canonical rows that changes nothing).
 */
#include <math.h>
#include <stdlib.h>

#include "spmv_hip.h"

typedef struct {
    int col, ord;
    double val;
} fsai_entry;

static int by_col_then_order(const void *pa, const void *pb) {
    const fsai_entry *a = pa, *b = pb;
    if (a->col != b->col) return a->col < b->col ? -1 : 1;
    return a->ord < b->ord ? -1 : a->ord > b->ord;
}

/* a NaN counts as the largest magnitude: it is kept, and the build then refuses the row */
static double magnitude(double v) { return isnan(v) ? INFINITY : fabs(v); }

/* larger |value| first, ties to the larger column */
static int by_magnitude(const void *pa, const void *pb) {
    const fsai_entry *a = pa, *b = pb;
    const double ma = magnitude(a->val), mb = magnitude(b->val);
    if (ma != mb) return ma > mb ? -1 : 1;
    return a->col > b->col ? -1 : a->col < b->col;
}

/* Row i of G has the pattern S_i = {i} and the stored columns j < i of row i; when there are more than cap - 1 such
 * columns the cap - 1 of largest |a_ij| stay (ties to the larger column).  g_ptr[n + 1] / g_col list S_i ascending, i
 * last; g_col needs room for min(n cap, row_ptr[n] + n) entries.  A row of m = |S_i| entries is built by w lanes, w the
 * smallest power of two >= m and at least 4: width_rows[width_ptr[k] .. width_ptr[k + 1]) are the rows of w = 4 << k
 * (k = 0 .. 3) in ascending order (width_ptr[5], width_rows[n]).
 * counts[4] = entries of G, rows that lost entries to the cap, the largest m, the first row that stores no diagonal
 * entry (-1: every row has one; S_i holds i either way). */
int spmv_fsai_plan(int n, const int *row_ptr, const int *col, const double *val, int cap, int *g_ptr, int *g_col,
                   int *width_ptr, int *width_rows, long long *counts) {
    if (n < 0 || cap < 1 || cap > 32 || !row_ptr || !g_ptr || !width_ptr || !counts) return -1;
    if (n && (!g_col || !width_rows || (row_ptr[n] > 0 && (!col || !val)))) return -1;
    counts[0] = counts[1] = counts[2] = 0;
    counts[3] = -1;
    g_ptr[0] = 0;
    for (int k = 0; k <= 4; ++k) width_ptr[k] = 0;
    if (!n) return 0;
    int longest = 0;
    for (int i = 0; i < n; ++i)
        if (row_ptr[i + 1] - row_ptr[i] > longest) longest = row_ptr[i + 1] - row_ptr[i];
    fsai_entry *row = malloc(((size_t)longest + 1) * sizeof *row);
    if (!row) return -1;
    int out = 0;
    for (int i = 0; i < n; ++i) {
        int k = 0, have_diag = 0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] == i) have_diag = 1;
            if (col[e] < 0 || col[e] >= i) continue;
            row[k].col = col[e];
            row[k].ord = k;
            row[k].val = val[e];
            ++k;
        }
        if (!have_diag && counts[3] < 0) counts[3] = i;
        qsort(row, (size_t)k, sizeof *row, by_col_then_order);
        int m = 0; /* repeats folded: row[0 .. m) */
        for (int q = 0; q < k; ++q) {
            if (m && row[m - 1].col == row[q].col) row[m - 1].val += row[q].val;
            else row[m++] = row[q];
        }
        if (m > cap - 1) {
            qsort(row, (size_t)m, sizeof *row, by_magnitude);
            m = cap - 1;
            qsort(row, (size_t)m, sizeof *row, by_col_then_order);
            counts[1]++;
        }
        for (int q = 0; q < m; ++q) g_col[out++] = row[q].col;
        g_col[out++] = i;
        g_ptr[i + 1] = out;
        if (m + 1 > counts[2]) counts[2] = m + 1;
        width_ptr[(m + 1 > 16) + (m + 1 > 8) + (m + 1 > 4) + 1]++;
    }
    free(row);
    counts[0] = out;
    for (int k = 0; k < 4; ++k) width_ptr[k + 1] += width_ptr[k];
    int fill[4] = {width_ptr[0], width_ptr[1], width_ptr[2], width_ptr[3]};
    for (int i = 0; i < n; ++i) {
        const int m = g_ptr[i + 1] - g_ptr[i];
        width_rows[fill[(m > 16) + (m > 8) + (m > 4)]++] = i;
    }
    return 0;
}
