/*
 * amg_plan_parts.h -- the parts of the AMG host setup (amg_plan.c) that the device setup (hip/spmv_amg_setup.hip) calls
 * as they are: the aggregation, which is serial by definition, and the dense inverse of the coarsest level; the
 * Gershgorin bound, which the Chebyshev build (hip/spmv_cheb.hip) shares; and the texts of the setup's refusals, so that
 * both setups refuse in the same words.  Private to the library: not installed, not exported (libspmv_amd.map keeps
 * the functions local).
 */
#ifndef SPMV_AMG_PLAN_PARTS_H
#define SPMV_AMG_PLAN_PARTS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int rows, cols;
    int *rp, *col;
    double *val;
} amg_csr;

/* d[i] = a_ii (d NULL: not wanted) and *rho = max_i (sum_j |a_ij|) / a_ii in stored order, the Gershgorin bound of
 * D^-1 A; returns -1, or the first row whose diagonal is missing (*missing = 1) or not finite and > 0 (*missing = 0).
 * The Chebyshev build (hip/spmv_cheb.hip) takes its automatic lmax from it */
int amg_gershgorin(const amg_csr *A, double *d, double *rho, int *missing);
/* agg[n] (-1: in no aggregate) from the strength graph (neighbours ascending); returns the number of aggregates, -1
 * without memory */
int amg_aggregate(int n, const int *s_rp, const int *s_col, int *agg);
/* *out = A^-1 dense, rows x rows row-major (malloc; the caller frees); 1: a zero or non-finite pivot; -1: no memory */
int amg_dense_inverse(const amg_csr *A, double **out);

#define AMG_WHY_NO_DIAGONAL "has no diagonal entry"
#define AMG_WHY_BAD_DIAGONAL "has a diagonal that is not finite and > 0"
#define AMG_REFUSE_ROW "amg_plan_build: row %d %s"
#define AMG_REFUSE_COARSE_ROW "amg_plan_build: level %d: row %d of the coarse matrix %s"
#define AMG_REFUSE_NOT_FINITE "amg_plan_build: level %d: an entry of the matrix is not finite"
#define AMG_REFUSE_PIVOT "amg_plan_build: level %d: a zero or non-finite pivot, the coarsest matrix (%d rows) is singular"
#define AMG_REFUSE_MEMORY "amg_plan_build: out of host memory, or a product beyond int range"

#ifdef __cplusplus
}
#endif
#endif
