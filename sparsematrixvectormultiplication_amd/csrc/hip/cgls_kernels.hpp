// cgls_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_cgls: CGLS (conjugate gradients on the normal
// equations, the stable form of Bjorck, Elfving and Strakos 1998) for min ||A x - b||^2 + damp^2 ||x||^2, x0 = 0.
//
// One step, around q = A p (m's SpMV) and s = A^T r (mt's SpMV):
//
//   cgls_norm2       partials of q.q (and r.r, s.s at the start; s.s in a step when damp = 0)     1 value per row
//   cgls_update_x_r  x += alpha p on [0, N), r -= alpha q on [0, M), partials of r.r              5 over both
//   cgls_update_s    s -= damp^2 x on [0, N), partials of s.s (damp > 0 only)                      3
//   cgls_update_p    p = s + beta p on [0, N), with partials of p.p when damp > 0                  3
//   cgls_fold        one workgroup folds the workgroups' partials in workgroup order
//   cgls_start / cgls_set_alpha / cgls_set_beta   one thread: the scalars, the stop and breakdown rules, the histories
//
// Vectors start at row 0.  A lane owns pieces of V = 16 / sizeof(T) rows, so every whole piece is one 16-byte load or
// store (the buffers are library-owned and hipMalloc-aligned); the last piece of a vector may be cut and its rows are
// then read and written one by one, none beyond the vector's length.  Pieces stride over the grid.
//
// Reduction order.  Products are accumulated in double for fp32 and fp64 data alike.  A lane adds its pieces in
// stride order and a piece's rows in row order; group_sum<64> adds the lanes of a wave, the waves of a workgroup are
// added in wave order, cgls_fold adds the workgroups in workgroup order.  The grid depends on the lengths only.  No
// atomics: every run gives the same bits.
//
// The state word.  RUN: the step proceeds.  STOP: the vector kernels return before they write anything and the scalar
// kernels only repeat the last history values, so a stopped solve can go on being launched (tol = 0) with x and r
// untouched.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"
#include "wave_ops.hpp"

namespace spmv {

constexpr int kCglsBlocks = 2048;  // grid cap of the vector kernels

// the scalar slots (doubles)
constexpr int kCglsGamma = 0, kCglsGamma0 = 1, kCglsQq = 2, kCglsPp = 3, kCglsAlpha = 4, kCglsRr = 5, kCglsSs = 6,
              kCglsBeta = 7, kCglsLastSs = 8, kCglsLastRr = 9, kCglsSlots = 16;
// the int words
constexpr int kCglsState = 0, kCglsSteps = 1, kCglsStatus = 2, kCglsFlagWords = 4;
constexpr int kCglsRun = 0, kCglsStop = 1;

typedef float v4f_cgls __attribute__((ext_vector_type(4)));

// piece [i0, i0 + V) of a; rows at or beyond n read as 0
template <typename T, int V>
__device__ __forceinline__ void cgls_load(const T *__restrict__ a, long long i0, long long n, T (&v)[V]) {
    static_assert(V * sizeof(T) == 16, "one 16-byte piece per lane");
    if (i0 + V <= n) {
        if constexpr (sizeof(T) == 8) {
            const v2d w = *reinterpret_cast<const v2d *>(a + i0);
            v[0] = w.x, v[1] = w.y;
        } else {
            const v4f_cgls w = *reinterpret_cast<const v4f_cgls *>(a + i0);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = i0 + j < n ? a[i0 + j] : T(0);
    }
}

// piece [i0, i0 + V) of a; rows at or beyond n are not written
template <typename T, int V>
__device__ __forceinline__ void cgls_store(T *__restrict__ a, long long i0, long long n, const T (&v)[V]) {
    if (i0 + V <= n) {
        if constexpr (sizeof(T) == 8) {
            *reinterpret_cast<v2d *>(a + i0) = v2d{v[0], v[1]};
        } else {
            *reinterpret_cast<v4f_cgls *>(a + i0) = v4f_cgls{v[0], v[1], v[2], v[3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j < n) a[i0 + j] = v[j];
    }
}

// the lane's first piece and the stride; pieces q cover rows [q V, q V + V)
__device__ __forceinline__ long long cgls_first() { return (long long)blockIdx.x * kBlock + threadIdx.x; }
__device__ __forceinline__ long long cgls_stride() { return (long long)gridDim.x * kBlock; }

// the lane's sum -> the workgroup's partial part[blockIdx.x], waves added in order
__device__ __forceinline__ void cgls_block_partial(double acc, double *__restrict__ part) {
    __shared__ double wave_sum[kBlock / 64];
    acc = group_sum<64>(acc);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w];
        part[blockIdx.x] = s;
    }
}

// partials of a.a on [0, n)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_norm2(long long n, const int *__restrict__ flags,
                                                     const T *__restrict__ a, double *__restrict__ part) {
    if (flags[kCglsState] != kCglsRun) return;
    double acc = 0.0;
    const long long end = (n + V - 1) / V;
    for (long long q = cgls_first(); q < end; q += cgls_stride()) {
        T av[V];
        cgls_load<T, V>(a, q * V, n, av);
#pragma unroll
        for (int j = 0; j < V; ++j) acc += (double)av[j] * (double)av[j];
    }
    cgls_block_partial(acc, part);
}

// x += alpha p on [0, N), r -= alpha q on [0, M) in one pass over max(M, N) rows; partials of the new r.r
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_x_r(long long N, long long M, const int *__restrict__ flags,
                                                          const double *__restrict__ sc, const T *__restrict__ p,
                                                          const T *__restrict__ q, T *__restrict__ x,
                                                          T *__restrict__ r, double *__restrict__ part) {
    if (flags[kCglsState] != kCglsRun) return;
    const double alpha = sc[kCglsAlpha];
    double acc = 0.0;
    const long long end = ((M > N ? M : N) + V - 1) / V;
    for (long long k = cgls_first(); k < end; k += cgls_stride()) {
        const long long i0 = k * V;
        if (i0 < N) {
            T xv[V], pv[V];
            cgls_load<T, V>(x, i0, N, xv);
            cgls_load<T, V>(p, i0, N, pv);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            cgls_store<T, V>(x, i0, N, xv);
        }
        if (i0 < M) {
            T rv[V], qv[V];
            cgls_load<T, V>(r, i0, M, rv);
            cgls_load<T, V>(q, i0, M, qv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                rv[j] = (T)((double)rv[j] - alpha * (double)qv[j]);
                acc += (double)rv[j] * (double)rv[j];
            }
            cgls_store<T, V>(r, i0, M, rv);
        }
    }
    cgls_block_partial(acc, part);
}

// s -= damp2 x on [0, N), partials of the new s.s
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_s(long long N, const int *__restrict__ flags, double damp2,
                                                        const T *__restrict__ x, T *__restrict__ s,
                                                        double *__restrict__ part) {
    if (flags[kCglsState] != kCglsRun) return;
    double acc = 0.0;
    const long long end = (N + V - 1) / V;
    for (long long k = cgls_first(); k < end; k += cgls_stride()) {
        const long long i0 = k * V;
        T sv[V], xv[V];
        cgls_load<T, V>(s, i0, N, sv);
        cgls_load<T, V>(x, i0, N, xv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sv[j] = (T)((double)sv[j] - damp2 * (double)xv[j]);
            acc += (double)sv[j] * (double)sv[j];
        }
        cgls_store<T, V>(s, i0, N, sv);
    }
    cgls_block_partial(acc, part);
}

// p = s + beta p on [0, N); part != nullptr: partials of the new p.p (the next step's delta when damp > 0)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_p(long long N, const int *__restrict__ flags,
                                                        const double *__restrict__ sc, const T *__restrict__ s,
                                                        T *__restrict__ p, double *__restrict__ part) {
    if (flags[kCglsState] != kCglsRun) return;
    const double beta = sc[kCglsBeta];
    double acc = 0.0;
    const long long end = (N + V - 1) / V;
    for (long long k = cgls_first(); k < end; k += cgls_stride()) {
        const long long i0 = k * V;
        T sv[V], pv[V];
        cgls_load<T, V>(s, i0, N, sv);
        cgls_load<T, V>(p, i0, N, pv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            pv[j] = (T)((double)sv[j] + beta * (double)pv[j]);
            acc += (double)pv[j] * (double)pv[j];
        }
        cgls_store<T, V>(p, i0, N, pv);
    }
    if (part) cgls_block_partial(acc, part);
}

// one workgroup: part[0 .. nparts) added in workgroup order -> *out
__global__ __launch_bounds__(kBlock) void cgls_fold(const int *__restrict__ flags, const double *__restrict__ part,
                                                    int nparts, double *__restrict__ out) {
    if (flags[kCglsState] != kCglsRun) return;
    __shared__ double wave_sum[kBlock / 64];
    double acc = 0.0;
    for (int g = threadIdx.x; g < nparts; g += kBlock) acc += part[g];
    acc = group_sum<64>(acc);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w];
        *out = s;
    }
}

// ---- the scalar kernels: one thread each.  A stop writes the status and the steps taken and never touches x.
__device__ __forceinline__ void cgls_stop(int *__restrict__ flags, int status, int steps) {
    flags[kCglsState] = kCglsStop;
    flags[kCglsStatus] = status;
    flags[kCglsSteps] = steps;
}

// gamma0 = s.s, rr0 = r.r (slots kCglsSs, kCglsRr) with s = A^T b, r = b; history row 0; p = s, so p.p = gamma0.
// A non-finite gamma0 or rr0 breaks down at step 0; gamma0 = 0 (A^T b = 0) has converged at step 0.
__global__ void cgls_start(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ ss_hist,
                           double *__restrict__ rr_hist, int iters) {
    const double gamma0 = sc[kCglsSs], rr0 = sc[kCglsRr];
    sc[kCglsGamma] = gamma0;
    sc[kCglsGamma0] = gamma0;
    sc[kCglsPp] = gamma0;
    sc[kCglsLastSs] = gamma0;
    sc[kCglsLastRr] = rr0;
    ss_hist[0] = gamma0;
    rr_hist[0] = rr0;
    flags[kCglsState] = kCglsRun;
    flags[kCglsSteps] = iters;
    flags[kCglsStatus] = SPMV_CGLS_RAN_ALL;
    if (!isfinite(gamma0) || !isfinite(rr0)) cgls_stop(flags, SPMV_CGLS_BREAKDOWN, 0);
    else if (gamma0 == 0.0) cgls_stop(flags, SPMV_CGLS_CONVERGED, 0);
}

// step t: delta = q.q + damp^2 p.p, alpha = gamma / delta; delta = 0 or anything not finite breaks down (step t not
// taken: x and r stay the iterate of step t - 1)
__global__ void cgls_set_alpha(double *__restrict__ sc, int *__restrict__ flags, int t, double damp2) {
    if (flags[kCglsState] != kCglsRun) return;
    const double delta = sc[kCglsQq] + damp2 * sc[kCglsPp];
    const double alpha = sc[kCglsGamma] / delta;
    if (delta == 0.0 || !isfinite(delta) || !isfinite(alpha)) {
        cgls_stop(flags, SPMV_CGLS_BREAKDOWN, t - 1);
        return;
    }
    sc[kCglsAlpha] = alpha;
}

// end of step t: history row t; gamma' = s.s or r.r not finite breaks down after the step; gamma' <= tol2 gamma0
// converges; else beta = gamma' / gamma, gamma = gamma'
__global__ void cgls_set_beta(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ ss_hist,
                              double *__restrict__ rr_hist, int t, double tol2) {
    if (flags[kCglsState] != kCglsRun) {
        ss_hist[t] = sc[kCglsLastSs];
        rr_hist[t] = sc[kCglsLastRr];
        return;
    }
    const double ss = sc[kCglsSs], rr = sc[kCglsRr];
    sc[kCglsLastSs] = ss;
    sc[kCglsLastRr] = rr;
    ss_hist[t] = ss;
    rr_hist[t] = rr;
    if (!isfinite(ss) || !isfinite(rr)) {
        cgls_stop(flags, SPMV_CGLS_BREAKDOWN, t);
        return;
    }
    if (ss <= tol2 * sc[kCglsGamma0]) {
        cgls_stop(flags, SPMV_CGLS_CONVERGED, t);
        return;
    }
    sc[kCglsBeta] = ss / sc[kCglsGamma];
    sc[kCglsGamma] = ss;
}

}  // namespace spmv
