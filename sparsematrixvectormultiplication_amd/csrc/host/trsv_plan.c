/*
 * trsv_plan.c -- the host analysis of the sparse triangular solves (include/spmv_hip.h: spmv_trsv_colour,
 * spmv_trsv_levels).  One sequential pass per row over the pattern; it runs once per build (spmv_trsv.hip) and never
 * inside a solve.  Both functions work on an n x n CSR pattern with local columns; entries whose column lies outside
 * [0, n) are ignored, rows need not be sorted and may repeat a column.
 */
#include <stdlib.h>
#include <string.h>

#include "spmv_hip.h"

/* Greedy first-fit colouring in natural row order over the pattern of A + A^T (the diagonal does not count): row i
 * gets the smallest colour none of its neighbours j < i has.  order[] lists the rows by (colour, row). */
int spmv_trsv_colour(int n, const int *row_ptr, const int *col, int *colour, int *order) {
    if (n < 0 || !row_ptr || !colour || !order || (n && row_ptr[n] > 0 && !col)) return -1;
    if (!n) return 0;
    /* the transposed pattern restricted to j < i: t_ptr / t_col list, for row i, the rows j < i with a_ji != 0 */
    int *t_ptr = calloc((size_t)n + 2, sizeof(int));
    int *seen = malloc((size_t)n * sizeof(int));
    int *count = NULL, *t_col = NULL;
    int colours = -1;
    if (!t_ptr || !seen) goto done;
    for (int j = 0; j < n; ++j)
        for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e)
            if (col[e] > j && col[e] < n) t_ptr[col[e] + 2]++;
    for (int i = 0; i < n; ++i) t_ptr[i + 2] += t_ptr[i + 1];
    t_col = malloc(((size_t)t_ptr[n + 1] + 1) * sizeof(int));
    if (!t_col) goto done;
    for (int j = 0; j < n; ++j) /* t_ptr[i + 1] is row i's fill mark and ends as its end */
        for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e)
            if (col[e] > j && col[e] < n) t_col[t_ptr[col[e] + 1]++] = j;
    colours = 0;
    for (int i = 0; i < n; ++i) seen[i] = -1; /* seen[c] == i: colour c is taken by a neighbour of row i */
    for (int i = 0; i < n; ++i) {
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            if (col[e] >= 0 && col[e] < i) seen[colour[col[e]]] = i;
        for (int e = t_ptr[i]; e < t_ptr[i + 1]; ++e) seen[colour[t_col[e]]] = i;
        int c = 0;
        while (c < colours && seen[c] == i) ++c;
        colour[i] = c;
        if (c == colours) ++colours;
    }
    count = calloc((size_t)colours + 1, sizeof(int));
    if (!count) {
        colours = -1;
        goto done;
    }
    for (int i = 0; i < n; ++i) count[colour[i] + 1]++;
    for (int c = 0; c < colours; ++c) count[c + 1] += count[c];
    for (int i = 0; i < n; ++i) order[count[colour[i]]++] = i;
done:
    free(t_ptr);
    free(seen);
    free(t_col);
    free(count);
    return colours;
}

/* Level schedule of the strict lower (uplo = SPMV_TRSV_LOWER) or strict upper triangle.  The rows a row reads are the
 * columns of its entries on that side; its level is 1 + the largest level among them (1 when it reads none).  perm[]
 * lists the rows level by level; inside a level first the rows with fewer than long_len entries on that side, then the
 * others, each group in ascending row order.  level_ptr[l] .. level_ptr[l + 1] are level l's places in perm
 * (l = 0 .. levels - 1), level_split[l] the place of its first long row.  A level is narrow when it has at most
 * chain_rows rows and chain_entries entries.  plan[3 k] = {kind, first level, one past the last level} of launch k:
 * kind 1 = a run of consecutive narrow levels (one workgroup, a barrier between levels), kind 0 = one wide level.
 * All arrays are the caller's: level[n], perm[n], level_ptr[n + 1], level_split[n], plan[3 n].
 * counts[4] = levels, launches, rows of the widest level, entries on that side (repeats counted). */
int spmv_trsv_levels(int n, const int *row_ptr, const int *col, int uplo, int long_len, int chain_rows,
                     int chain_entries, int *level, int *perm, int *level_ptr, int *level_split, int *plan,
                     long long *counts) {
    if (n < 0 || !row_ptr || !level || !perm || !level_ptr || !level_split || !plan || !counts) return -1;
    if (uplo != SPMV_TRSV_LOWER && uplo != SPMV_TRSV_UPPER) return -1;
    if (n && row_ptr[n] > 0 && !col) return -1;
    const int lower = uplo == SPMV_TRSV_LOWER;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    level_ptr[0] = 0;
    if (!n) return 0;
    int *len = malloc((size_t)n * sizeof(int));
    int *fill = NULL;
    long long *level_entries = NULL;
    int rc = -1, levels = 0;
    if (!len) goto done;
    for (int s = 0; s < n; ++s) {
        const int i = lower ? s : n - 1 - s;
        int lv = 0, k = 0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int j = col[e];
            if (lower ? (j >= 0 && j < i) : (j > i && j < n)) {
                if (level[j] > lv) lv = level[j];
                ++k;
            }
        }
        level[i] = lv + 1;
        len[i] = k;
        if (lv + 1 > levels) levels = lv + 1;
        counts[3] += k;
    }
    /* counting sort by (level, long, row): two bins per level */
    fill = calloc(2 * (size_t)levels + 1, sizeof(int));
    level_entries = calloc((size_t)levels, sizeof(long long));
    if (!fill || !level_entries) goto done;
    for (int i = 0; i < n; ++i) {
        fill[2 * (level[i] - 1) + (len[i] >= long_len) + 1]++;
        level_entries[level[i] - 1] += len[i];
    }
    for (int b = 0; b < 2 * levels; ++b) fill[b + 1] += fill[b];
    for (int l = 0; l < levels; ++l) {
        level_ptr[l] = fill[2 * l];
        level_split[l] = fill[2 * l + 1];
    }
    level_ptr[levels] = n;
    for (int i = 0; i < n; ++i) perm[fill[2 * (level[i] - 1) + (len[i] >= long_len)]++] = i;
    int launches = 0, widest = 0, in_chain = 0;
    for (int l = 0; l < levels; ++l) {
        const int rows = level_ptr[l + 1] - level_ptr[l];
        if (rows > widest) widest = rows;
        const int narrow = rows <= chain_rows && level_entries[l] <= chain_entries;
        if (narrow && in_chain) {
            plan[3 * (launches - 1) + 2] = l + 1;
            continue;
        }
        plan[3 * launches] = narrow;
        plan[3 * launches + 1] = l;
        plan[3 * launches + 2] = l + 1;
        ++launches;
        in_chain = narrow;
    }
    counts[0] = levels;
    counts[1] = launches;
    counts[2] = widest;
    rc = 0;
done:
    free(len);
    free(fill);
    free(level_entries);
    return rc;
}
