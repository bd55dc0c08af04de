// cgls_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_cgls: CGLS (conjugate gradients on the normal
// equations, the stable form of Bjorck, Elfving and Strakos 1998) for min ||A x - b||^2 + damp^2 ||x||^2, x0 = 0.
//
// One step, around q = A p (m's SpMV) and s = A^T r (mt's SpMV):
//
//   cgls_norm2       partials of q.q (and r.r, s.s at the start; s.s in a step when damp = 0)     1 value per row
//   cgls_update_x_r  x += alpha p on [0, N), r -= alpha q on [0, M), partials of r.r              5 over both
//   cgls_update_s    s -= damp^2 x on [0, N), partials of s.s (damp > 0 only)                      3
//   cgls_update_p    p = s + beta p on [0, N), with partials of p.p when damp > 0                  3
//   cgls_start / cgls_set_alpha / cgls_set_beta   one thread: the scalars, the stop and breakdown rules, the histories
//
// Vectors start at row 0 and are walked in pieces of V = 16 / sizeof(T) rows (piece_load / piece_store, PieceLane:
// solver_ops.hpp), none beyond the vector's length.  One workgroup folds the partials (solver_fold), in the order of
// solver_ops.hpp.  The grid depends on the lengths only.
//
// The state word.  RUN: the step proceeds.  STOP: the vector kernels return before they write anything and the scalar
// kernels only repeat the last history values, so a stopped solve can go on being launched (tol = 0) with x and r
// untouched.  (The folds run on: the slots they fill are read in the RUN state only.)
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kCglsBlocks = 2048;  // grid cap of the vector kernels

// the scalar slots (doubles)
constexpr int kCglsGamma = 0, kCglsGamma0 = 1, kCglsQq = 2, kCglsPp = 3, kCglsAlpha = 4, kCglsRr = 5, kCglsSs = 6,
              kCglsBeta = 7, kCglsLastSs = 8, kCglsLastRr = 9, kCglsSlots = 16;
// the int words: the stop flags of solver_ops.hpp

// partials of a.a on [0, n)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_norm2(long long n, const int *__restrict__ flags,
                                                     const T *__restrict__ a, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    double acc[1] = {0.0};
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        T av[V];
        piece_load<T, V>(a, l.q * V, 0, n, av);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[0] += (double)av[j] * (double)av[j];
    }
    block_partials<1>(acc, part);
}

// x += alpha p on [0, N), r -= alpha q on [0, M) in one pass over max(M, N) rows; partials of the new r.r
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_x_r(long long N, long long M, const int *__restrict__ flags,
                                                          const double *__restrict__ sc, const T *__restrict__ p,
                                                          const T *__restrict__ q, T *__restrict__ x,
                                                          T *__restrict__ r, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double alpha = sc[kCglsAlpha];
    double acc[1] = {0.0};
    for (PieceLane l(0, M > N ? M : N, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        if (i0 < N) {
            T xv[V], pv[V];
            piece_load<T, V>(x, i0, 0, N, xv);
            piece_load<T, V>(p, i0, 0, N, pv);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            piece_store<T, V>(x, i0, 0, N, xv);
        }
        if (i0 < M) {
            T rv[V], qv[V];
            piece_load<T, V>(r, i0, 0, M, rv);
            piece_load<T, V>(q, i0, 0, M, qv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                rv[j] = (T)((double)rv[j] - alpha * (double)qv[j]);
                acc[0] += (double)rv[j] * (double)rv[j];
            }
            piece_store<T, V>(r, i0, 0, M, rv);
        }
    }
    block_partials<1>(acc, part);
}

// s -= damp2 x on [0, N), partials of the new s.s
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_s(long long N, const int *__restrict__ flags, double damp2,
                                                        const T *__restrict__ x, T *__restrict__ s,
                                                        double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    double acc[1] = {0.0};
    for (PieceLane l(0, N, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T sv[V], xv[V];
        piece_load<T, V>(s, i0, 0, N, sv);
        piece_load<T, V>(x, i0, 0, N, xv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sv[j] = (T)((double)sv[j] - damp2 * (double)xv[j]);
            acc[0] += (double)sv[j] * (double)sv[j];
        }
        piece_store<T, V>(s, i0, 0, N, sv);
    }
    block_partials<1>(acc, part);
}

// p = s + beta p on [0, N); part != nullptr: partials of the new p.p (the next step's delta when damp > 0)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void cgls_update_p(long long N, const int *__restrict__ flags,
                                                        const double *__restrict__ sc, const T *__restrict__ s,
                                                        T *__restrict__ p, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double beta = sc[kCglsBeta];
    double acc[1] = {0.0};
    for (PieceLane l(0, N, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T sv[V], pv[V];
        piece_load<T, V>(s, i0, 0, N, sv);
        piece_load<T, V>(p, i0, 0, N, pv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            pv[j] = (T)((double)sv[j] + beta * (double)pv[j]);
            acc[0] += (double)pv[j] * (double)pv[j];
        }
        piece_store<T, V>(p, i0, 0, N, pv);
    }
    if (part) block_partials<1>(acc, part);
}

// ---- the scalar kernels: one thread each.  A stop (solver_stop) writes the status and the steps taken and never
// touches x.

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
    flags[kSolverState] = kSolverRun;
    flags[kSolverSteps] = iters;
    flags[kSolverStatus] = SPMV_CGLS_RAN_ALL;
    if (!isfinite(gamma0) || !isfinite(rr0)) solver_stop(flags, SPMV_CGLS_BREAKDOWN, 0);
    else if (gamma0 == 0.0) solver_stop(flags, SPMV_CGLS_CONVERGED, 0);
}

// step t: delta = q.q + damp^2 p.p, alpha = gamma / delta; delta = 0 or anything not finite breaks down (step t not
// taken: x and r stay the iterate of step t - 1)
__global__ void cgls_set_alpha(double *__restrict__ sc, int *__restrict__ flags, int t, double damp2) {
    if (flags[kSolverState] != kSolverRun) return;
    const double delta = sc[kCglsQq] + damp2 * sc[kCglsPp];
    const double alpha = sc[kCglsGamma] / delta;
    if (delta == 0.0 || !isfinite(delta) || !isfinite(alpha)) {
        solver_stop(flags, SPMV_CGLS_BREAKDOWN, t - 1);
        return;
    }
    sc[kCglsAlpha] = alpha;
}

// end of step t: history row t; gamma' = s.s or r.r not finite breaks down after the step; gamma' <= tol2 gamma0
// converges; else beta = gamma' / gamma, gamma = gamma'
__global__ void cgls_set_beta(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ ss_hist,
                              double *__restrict__ rr_hist, int t, double tol2) {
    if (flags[kSolverState] != kSolverRun) {
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
        solver_stop(flags, SPMV_CGLS_BREAKDOWN, t);
        return;
    }
    if (ss <= tol2 * sc[kCglsGamma0]) {
        solver_stop(flags, SPMV_CGLS_CONVERGED, t);
        return;
    }
    sc[kCglsBeta] = ss / sc[kCglsGamma];
    sc[kCglsGamma] = ss;
}

}  // namespace spmv
