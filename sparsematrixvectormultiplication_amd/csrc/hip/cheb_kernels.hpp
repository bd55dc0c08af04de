// cheb_kernels.hpp -- the vector passes of the Chebyshev polynomial preconditioner (spmv_cheb.hip launches them between
// the products of P's own handle) (gfx950).
//
// With g = T(1 / a_ii) and the coefficients a_j, b_j of host/cheb_plan.c:
//
//   cheb_first   step 0:       d = b_0 (g r);                        z = d
//   cheb_step    step j >= 1:  d = a_j d + b_j (g (r - q)), q = A z;  z = z + d
//
// Every value is computed in double from the stored values and rounded once to T where it is stored; z takes the
// rounded d, the value the next step reads.  A LAST pass writes z to `zout` (the caller's vector) and stores no d.
//
// One wide (solver_ops.hpp): a lane walks 16-byte pieces (V = 16 / sizeof(T) values; V = 1 when r or zout is not
// 16-byte aligned: the same bits), PieceLane's stride, the grid solver_grid(kChebBlocks, pieces, kBlock).  A trip's
// five loads -- q, r, d, z, g -- are issued before the first value is used.  The loop walks the whole pieces; when n is
// no multiple of V, the lane whose walk ends on the cut piece takes its rows one by one afterwards, so nothing behind
// row n - 1 of r or zout is touched.
// k wide (cg_multi_kernels.hpp): row-major n x k arrays, McgLane's rows and column lanes (V columns of one row per
// lane when a row is whole pieces, else 1; the lanes past k idle), g by row, the grid capped by kMcgBlocks.  Column
// j's values do not depend on j or k.
//
// No LDS, no atomics, no reduction: 5 values read and 2 written per row and column (step 0: 2 and 2; a LAST pass
// writes 1).
#pragma once
#include "cg_multi_kernels.hpp"

namespace spmv {

constexpr int kChebBlocks = 2048;    // grid cap of the one-wide passes
constexpr int kChebMaxDegree = 32;   // SPMV_CHEBYSHEV_MAX_DEGREE

// one value of step 0 and of step j; the parentheses are the definition's.  No product is fused with the sum behind
// it: every instance of a pass (pieces or single values, one or k wide) then rounds alike, whichever way the compiler
// would have contracted a * d + b * t, and an r or z off a 16-byte boundary gives the bits of an aligned one
template <typename T>
__device__ __forceinline__ T cheb_first_value(double b0, T g, T r) {
#pragma clang fp contract(off)
    return (T)(b0 * ((double)g * (double)r));
}
template <typename T>
__device__ __forceinline__ T cheb_step_value(double a, double b, T g, T r, T q, T d) {
#pragma clang fp contract(off)
    const double t = b * ((double)g * ((double)r - (double)q));
    const double ad = a * (double)d;
    return (T)(ad + t);
}

template <typename T, int V, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_first(long long n, double b0, const T *__restrict__ g,
                                                     const T *__restrict__ r, T *__restrict__ d, T *__restrict__ zout) {
    PieceLane l(0, n, V);
    const long long whole = n / V;  // pieces that are not cut
    for (; l.q < whole; l.q += l.stride) {
        const long long i0 = l.q * V;
        T gv[V], rv[V], dv[V];
        piece_load<T, V>(g + i0, gv);
        piece_load<T, V>(r + i0, rv);
#pragma unroll
        for (int v = 0; v < V; ++v) dv[v] = cheb_first_value<T>(b0, gv[v], rv[v]);
        if constexpr (!LAST) piece_store<T, V>(d + i0, dv);
        piece_store<T, V>(zout + i0, dv);
    }
    if (l.q == whole)  // the lane whose walk ends on the cut piece takes its rows one by one
        for (long long i = whole * V; i < n; ++i) {
            const T dn = cheb_first_value<T>(b0, g[i], r[i]);
            if constexpr (!LAST) d[i] = dn;
            zout[i] = dn;
        }
}

// zin and zout are P's z, or (LAST) P's z and the caller's vector: zout is not read
template <typename T, int V, bool LAST>
__global__ __launch_bounds__(kBlock) void cheb_step(long long n, double a, double b, const T *__restrict__ g,
                                                    const T *__restrict__ r, const T *__restrict__ q, const T *zin,
                                                    T *__restrict__ d, T *zout) {
    PieceLane l(0, n, V);
    const long long whole = n / V;
    for (; l.q < whole; l.q += l.stride) {
        const long long i0 = l.q * V;
        T qv[V], rv[V], dv[V], zv[V], gv[V];
        piece_load<T, V>(q + i0, qv);
        piece_load<T, V>(r + i0, rv);
        piece_load<T, V>(d + i0, dv);
        piece_load<T, V>(zin + i0, zv);
        piece_load<T, V>(g + i0, gv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            dv[v] = cheb_step_value<T>(a, b, gv[v], rv[v], qv[v], dv[v]);
            zv[v] = (T)((double)zv[v] + (double)dv[v]);
        }
        if constexpr (!LAST) piece_store<T, V>(d + i0, dv);
        piece_store<T, V>(zout + i0, zv);
    }
    if (l.q == whole)
        for (long long i = whole * V; i < n; ++i) {
            const T dn = cheb_step_value<T>(a, b, g[i], r[i], q[i], d[i]);
            const T zn = (T)((double)zin[i] + (double)dn);
            if constexpr (!LAST) d[i] = dn;
            zout[i] = zn;
        }
}

template <typename T, int V, bool LAST>
__global__ __launch_bounds__(kBlock) void mcheb_first(long long n, int k, int cl, double b0, const T *__restrict__ g,
                                                      const T *__restrict__ R, T *__restrict__ D, T *__restrict__ Zout) {
    const McgLane l(cl, V);
    if (l.j0 >= k) return;
    for (long long i = l.row; i < n; i += l.stride) {
        const long long o = i * k + l.j0;
        T rv[V], dv[V];
        piece_load<T, V>(R + o, rv);
        const T gi = g[i];
#pragma unroll
        for (int v = 0; v < V; ++v) dv[v] = cheb_first_value<T>(b0, gi, rv[v]);
        if constexpr (!LAST) piece_store<T, V>(D + o, dv);
        piece_store<T, V>(Zout + o, dv);
    }
}

template <typename T, int V, bool LAST>
__global__ __launch_bounds__(kBlock) void mcheb_step(long long n, int k, int cl, double a, double b,
                                                     const T *__restrict__ g, const T *__restrict__ R,
                                                     const T *__restrict__ Q, const T *Zin, T *__restrict__ D, T *Zout) {
    const McgLane l(cl, V);
    if (l.j0 >= k) return;
    for (long long i = l.row; i < n; i += l.stride) {
        const long long o = i * k + l.j0;
        T qv[V], rv[V], dv[V], zv[V];
        piece_load<T, V>(Q + o, qv);
        piece_load<T, V>(R + o, rv);
        piece_load<T, V>(D + o, dv);
        piece_load<T, V>(Zin + o, zv);
        const T gi = g[i];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            dv[v] = cheb_step_value<T>(a, b, gi, rv[v], qv[v], dv[v]);
            zv[v] = (T)((double)zv[v] + (double)dv[v]);
        }
        if constexpr (!LAST) piece_store<T, V>(D + o, dv);
        piece_store<T, V>(Zout + o, zv);
    }
}

}  // namespace spmv
