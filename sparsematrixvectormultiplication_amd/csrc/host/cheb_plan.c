/*
 * cheb_plan.c -- the coefficients of the Chebyshev polynomial preconditioner (include/spmv_hip.h:
 * spmv_chebyshev_coefficients).  Plain C, fp64, no device: it runs once per build (spmv_cheb.hip) and tests call it
 * directly.  Every line is one rounded operation in the order written; the file is compiled with -ffp-contract=off so
 * that no product is fused with the sum behind it, and a restatement in any language gives the same bits.
 *
 *   theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta
 *   rho_0 = 1 / sigma;  a_0 = 0;  b_0 = 1 / theta
 *   j = 1 .. degree - 1:  rho_j = 1 / (2 sigma - rho_{j-1});  a_j = rho_j rho_{j-1};  b_j = 2 rho_j / delta
 */
#include <math.h>

#include "spmv_hip.h"

int spmv_chebyshev_coefficients(int degree, double lmin, double lmax, double *a, double *b) {
    if (!a || !b) return -1;
    if (degree < 1 || degree > SPMV_CHEBYSHEV_MAX_DEGREE) return -1;
    if (!isfinite(lmin) || !isfinite(lmax) || !(lmin > 0.0) || !(lmin < lmax)) return -1;
    const double sum = lmax + lmin;
    const double theta = sum / 2.0;
    const double diff = lmax - lmin;
    const double delta = diff / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    a[0] = 0.0;
    b[0] = 1.0 / theta;
    for (int j = 1; j < degree; ++j) {
        const double twice = 2.0 * sigma;
        const double below = twice - rho;
        const double next = 1.0 / below;
        a[j] = next * rho;
        const double two_rho = 2.0 * next;
        b[j] = two_rho / delta;
        rho = next;
    }
    return 0;
}
