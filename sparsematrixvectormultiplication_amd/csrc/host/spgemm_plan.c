/* spgemm_plan.c -- spmv_spgemm_plan: how the rows of C = A B are dealt out to the two tiers of the device product
 * (include/spmv_hip.h; csrc/hip/spmv_spgemm.hip).  Host only: the plan is a function of the rows' product counts.
 *
 * The rows are cut, in order, into contiguous blocks [block_row[b], block_row[b + 1]) that partition [0, M).  A row
 * with more products than the cap is a long row: it joins the block that is open, closes it, and is listed in
 * long_row; the on-chip tier skips it.  Every other row joins the open block unless that would take the block's
 * products (long rows not counted) beyond the cap or its rows (all of them) beyond max_rows; then a new block opens. */
#include <stddef.h>

#include "spmv_hip.h"

int spmv_spgemm_plan(int M, const long long *products, int block_products, int max_rows, int *block_row, int *n_blocks,
                     int *long_row, int *n_long) {
    if (M < 0 || (M > 0 && !products) || !block_row || !n_blocks || !long_row || !n_long) return -1;
    if (max_rows < 1 || max_rows > 4096) return -1;
    long long cap = block_products == 0 ? 4096 : block_products;
    if (block_products == -1) cap = 0; /* no on-chip tier: a row with one product is long already */
    else if (cap < 64 || cap > 4096 || (cap & (cap - 1)) != 0) return -1;
    for (int i = 0; i < M; ++i)
        if (products[i] < 0) return -1;
    int nb = 0, nl = 0, rows = 0; /* rows: those of the open block */
    long long sum = 0;
    block_row[0] = 0;
    for (int i = 0; i < M; ++i) {
        const long long p = products[i];
        const int is_long = p > cap;
        if (rows > 0 && (rows == max_rows || (!is_long && sum + p > cap))) {
            block_row[++nb] = i; /* the open block ends in front of row i */
            rows = 0;
            sum = 0;
        }
        ++rows;
        if (is_long) {
            long_row[nl++] = i;
            block_row[++nb] = i + 1; /* a long row closes its block */
            rows = 0;
            sum = 0;
        } else {
            sum += p;
        }
    }
    if (rows > 0) block_row[++nb] = M;
    *n_blocks = nb;
    *n_long = nl;
    return 0;
}
