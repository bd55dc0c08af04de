// bicgstab_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_bicgstab: BiCGSTAB (van der Vorst 1992) for a
// nonsymmetric A, x0 = 0, r^ = r0 = b (gfx950).
//
// One step, after v = A p (the handle's SpMV), and again after t = A s:
//
//   bcg_dot          partials of r^.v                                         2 values per row
//   bcg_update_s     s = r - alpha v (into the second SpMV's input), s.s      3
//   bcg_dot2         partials of t.s and t.t in one pass                      2
//   bcg_update_x_r   x += alpha p + omega s, r = s - omega t, r^.r and r.r    7
//   bcg_update_p     p = r + beta (p - omega v)                               4
//   bcg_start / bcg_set_alpha / bcg_check_s / bcg_set_omega / bcg_set_beta   one thread: the scalars, the stop and
//                    breakdown rules and the history
//
// Right preconditioning (spmv_hip_csr_pbicgstab) swaps three of them: bcg_jac_update_s (also s^ = D^-1 s; 5 values
// per row), bcg_pre_update_x_r (x moves along p^ and s^; 8) and bcg_jac_update_p (also p^ = D^-1 p; 6).
//
// Every vector is indexed by global row; a kernel covers the rows [lo, hi) of this rank in pieces of V = 16 / sizeof(T)
// rows (piece_load / piece_store, PieceLane: solver_ops.hpp); the rows outside [lo, hi) are neither read nor written.
// The partials are folded and added over the ranks by solver_reduce, in the order of solver_ops.hpp.  The grid
// depends on hi - lo only.
//
// The state word.  RUN: the step proceeds.  HALF: s converged in this step; bcg_update_x_r applies x += alpha p,
// r = s and bcg_set_beta turns the state to STOP.  STOP: the vector kernels return before they write anything and
// the scalar kernels only repeat the last history value, so a stopped solve can go on being launched (tol = 0) with
// x and r untouched.
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kBcgBlocks = 2048;  // grid cap of the vector kernels

// the scalar slots (doubles).  Two-value reductions land in adjacent slots: (Rho, Rr0), (Ts, Tt), (RhoNew, Rr).
constexpr int kBcgRho = 0, kBcgRr0 = 1, kBcgRv = 2, kBcgAlpha = 3, kBcgSs = 4, kBcgTs = 5, kBcgTt = 6, kBcgOmega = 7,
              kBcgRhoNew = 8, kBcgRr = 9, kBcgBeta = 10, kBcgLast = 11, kBcgLocal = 12, kBcgSlots = 16;
// the int words: the stop flags of solver_ops.hpp, word 3 = the stop came at a half step; the state passes through
// kBcgHalfStep (the x update of that step still runs) on its way to kBcgStop
constexpr int kBcgHalf = 3;
constexpr int kBcgHalfStep = 1, kBcgStop = 2;

// partials of a.b on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_dot(long long lo, long long hi, const int *__restrict__ flags,
                                                  const T *__restrict__ a, const T *__restrict__ b,
                                                  double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    double acc[1] = {0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T av[V], bv[V];
        piece_load<T, V>(a, i0, lo, hi, av);
        piece_load<T, V>(b, i0, lo, hi, bv);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[0] += (double)av[j] * (double)bv[j];
    }
    block_partials<1>(acc, part);
}

// partials of a.b and a.a on [lo, hi) (r.r^ with r.r at the start; t.s with t.t in a step)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_dot2(long long lo, long long hi, const int *__restrict__ flags,
                                                   const T *__restrict__ a, const T *__restrict__ b,
                                                   double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    double acc[2] = {0.0, 0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T av[V], bv[V];
        piece_load<T, V>(a, i0, lo, hi, av);
        piece_load<T, V>(b, i0, lo, hi, bv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double ad = (double)av[j];
            acc[0] += ad * (double)bv[j];
            acc[1] += ad * ad;
        }
    }
    block_partials<2>(acc, part);
}

// s = r - alpha v on [lo, hi), partials of s.s
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_s(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, const T *__restrict__ r,
                                                       const T *__restrict__ v, T *__restrict__ s,
                                                       double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double alpha = sc[kBcgAlpha];
    double acc[1] = {0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T rv[V], vv[V], sv[V];
        piece_load<T, V>(r, i0, lo, hi, rv);
        piece_load<T, V>(v, i0, lo, hi, vv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sv[j] = (T)((double)rv[j] - alpha * (double)vv[j]);
            acc[0] += (double)sv[j] * (double)sv[j];
        }
        piece_store<T, V>(s, i0, lo, hi, sv);
    }
    block_partials<1>(acc, part);
}

// RUN: x += alpha p + omega s, r = s - omega t on [lo, hi), partials of r^.r and r.r.  HALF: x += alpha p, r = s.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_x_r(long long lo, long long hi, const int *__restrict__ flags,
                                                         const double *__restrict__ sc, const T *__restrict__ rhat,
                                                         const T *__restrict__ p, const T *__restrict__ s,
                                                         const T *__restrict__ t, T *__restrict__ x,
                                                         T *__restrict__ r, double *__restrict__ part) {
    const int state = flags[kSolverState];
    if (state == kBcgStop) return;
    const double alpha = sc[kBcgAlpha];
    double acc[2] = {0.0, 0.0};
    if (state == kBcgHalfStep) {
        for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            T xv[V], pv[V], sv[V];
            piece_load<T, V>(x, i0, lo, hi, xv);
            piece_load<T, V>(p, i0, lo, hi, pv);
            piece_load<T, V>(s, i0, lo, hi, sv);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            piece_store<T, V>(x, i0, lo, hi, xv);
            piece_store<T, V>(r, i0, lo, hi, sv);
        }
    } else {
        const double omega = sc[kBcgOmega];
        for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            T xv[V], pv[V], sv[V], tv[V], hv[V];
            piece_load<T, V>(x, i0, lo, hi, xv);
            piece_load<T, V>(p, i0, lo, hi, pv);
            piece_load<T, V>(s, i0, lo, hi, sv);
            piece_load<T, V>(t, i0, lo, hi, tv);
            piece_load<T, V>(rhat, i0, lo, hi, hv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                xv[j] = (T)((double)xv[j] + (alpha * (double)pv[j] + omega * (double)sv[j]));
                const T rn = (T)((double)sv[j] - omega * (double)tv[j]);
                sv[j] = rn;  // the new r
                acc[0] += (double)hv[j] * (double)rn;
                acc[1] += (double)rn * (double)rn;
            }
            piece_store<T, V>(x, i0, lo, hi, xv);
            piece_store<T, V>(r, i0, lo, hi, sv);
        }
    }
    block_partials<2>(acc, part);
}

// p = r + beta (p - omega v) on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_p(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, const T *__restrict__ r,
                                                       const T *__restrict__ v, T *__restrict__ p) {
    if (flags[kSolverState] != kSolverRun) return;
    const double beta = sc[kBcgBeta], omega = sc[kBcgOmega];
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T rv[V], vv[V], pv[V];
        piece_load<T, V>(r, i0, lo, hi, rv);
        piece_load<T, V>(v, i0, lo, hi, vv);
        piece_load<T, V>(p, i0, lo, hi, pv);
#pragma unroll
        for (int j = 0; j < V; ++j) pv[j] = (T)((double)rv[j] + beta * ((double)pv[j] - omega * (double)vv[j]));
        piece_store<T, V>(p, i0, lo, hi, pv);
    }
}

// ---- right preconditioning (spmv_hip_csr_pbicgstab): the products' inputs are p^ = M^-1 p and s^ = M^-1 s, and x
// moves along them.  Jacobi (dinv = D^-1 by global row) is fused into the s and p updates: one more array read and
// the hat vector written beside.  A block-Jacobi apply is a pc_apply pass after bcg_update_s / bcg_update_p.

// s = r - alpha v, s^ = D^-1 s on [lo, hi), partials of s.s
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_jac_update_s(long long lo, long long hi, const int *__restrict__ flags,
                                                           const double *__restrict__ sc, const T *__restrict__ r,
                                                           const T *__restrict__ v, const T *__restrict__ dinv,
                                                           T *__restrict__ s, T *__restrict__ sh,
                                                           double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double alpha = sc[kBcgAlpha];
    double acc[1] = {0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T rv[V], vv[V], dv[V], sv[V], hv[V];
        piece_load<T, V>(r, i0, lo, hi, rv);
        piece_load<T, V>(v, i0, lo, hi, vv);
        piece_load<T, V>(dinv, i0, lo, hi, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sv[j] = (T)((double)rv[j] - alpha * (double)vv[j]);
            hv[j] = (T)((double)dv[j] * (double)sv[j]);
            acc[0] += (double)sv[j] * (double)sv[j];
        }
        piece_store<T, V>(s, i0, lo, hi, sv);
        piece_store<T, V>(sh, i0, lo, hi, hv);
    }
    block_partials<1>(acc, part);
}

// RUN: x += alpha p^ + omega s^, r = s - omega t on [lo, hi), partials of r^.r and r.r.  HALF: x += alpha p^, r = s.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_pre_update_x_r(long long lo, long long hi, const int *__restrict__ flags,
                                                             const double *__restrict__ sc, const T *__restrict__ rhat,
                                                             const T *__restrict__ ph, const T *__restrict__ sh,
                                                             const T *__restrict__ s, const T *__restrict__ t,
                                                             T *__restrict__ x, T *__restrict__ r,
                                                             double *__restrict__ part) {
    const int state = flags[kSolverState];
    if (state == kBcgStop) return;
    const double alpha = sc[kBcgAlpha];
    double acc[2] = {0.0, 0.0};
    if (state == kBcgHalfStep) {
        for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            T xv[V], pv[V], sv[V];
            piece_load<T, V>(x, i0, lo, hi, xv);
            piece_load<T, V>(ph, i0, lo, hi, pv);
            piece_load<T, V>(s, i0, lo, hi, sv);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            piece_store<T, V>(x, i0, lo, hi, xv);
            piece_store<T, V>(r, i0, lo, hi, sv);
        }
    } else {
        const double omega = sc[kBcgOmega];
        for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            T xv[V], pv[V], shv[V], sv[V], tv[V], hv[V];
            piece_load<T, V>(x, i0, lo, hi, xv);
            piece_load<T, V>(ph, i0, lo, hi, pv);
            piece_load<T, V>(sh, i0, lo, hi, shv);
            piece_load<T, V>(s, i0, lo, hi, sv);
            piece_load<T, V>(t, i0, lo, hi, tv);
            piece_load<T, V>(rhat, i0, lo, hi, hv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                xv[j] = (T)((double)xv[j] + (alpha * (double)pv[j] + omega * (double)shv[j]));
                const T rn = (T)((double)sv[j] - omega * (double)tv[j]);
                sv[j] = rn;  // the new r
                acc[0] += (double)hv[j] * (double)rn;
                acc[1] += (double)rn * (double)rn;
            }
            piece_store<T, V>(x, i0, lo, hi, xv);
            piece_store<T, V>(r, i0, lo, hi, sv);
        }
    }
    block_partials<2>(acc, part);
}

// p = r + beta (p - omega v), p^ = D^-1 p on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_jac_update_p(long long lo, long long hi, const int *__restrict__ flags,
                                                           const double *__restrict__ sc, const T *__restrict__ r,
                                                           const T *__restrict__ v, const T *__restrict__ dinv,
                                                           T *__restrict__ p, T *__restrict__ ph) {
    if (flags[kSolverState] != kSolverRun) return;
    const double beta = sc[kBcgBeta], omega = sc[kBcgOmega];
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T rv[V], vv[V], pv[V], dv[V], hv[V];
        piece_load<T, V>(r, i0, lo, hi, rv);
        piece_load<T, V>(v, i0, lo, hi, vv);
        piece_load<T, V>(p, i0, lo, hi, pv);
        piece_load<T, V>(dinv, i0, lo, hi, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            pv[j] = (T)((double)rv[j] + beta * ((double)pv[j] - omega * (double)vv[j]));
            hv[j] = (T)((double)dv[j] * (double)pv[j]);
        }
        piece_store<T, V>(p, i0, lo, hi, pv);
        piece_store<T, V>(ph, i0, lo, hi, hv);
    }
}

// ---- the scalar kernels: one thread each.  A stop (solver_stop with state kBcgStop) writes the status and the steps
// taken and never touches x.

// rho = r^.r, rr0 = r.r (slots kBcgRho, kBcgRr0), history row 0; rr0 = 0 (b = 0) stops at step 0, converged
__global__ void bcg_start(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int iters) {
    const double rr0 = sc[kBcgRr0];
    sc[kBcgLast] = rr0;
    hist[0] = rr0;
    flags[kSolverState] = kSolverRun;
    flags[kSolverSteps] = iters;
    flags[kSolverStatus] = SPMV_BICG_RAN_ALL;
    flags[kBcgHalf] = 0;
    if (rr0 == 0.0) solver_stop(flags, SPMV_BICG_CONVERGED, 0, kBcgStop);
}

// step t: alpha = rho / r^.v; r^.v = 0 or not finite breaks down (step t not taken)
__global__ void bcg_set_alpha(double *__restrict__ sc, int *__restrict__ flags, int t) {
    if (flags[kSolverState] != kSolverRun) return;
    const double rv = sc[kBcgRv];
    if (rv == 0.0 || !isfinite(rv)) {
        solver_stop(flags, SPMV_BICG_BREAKDOWN_RHO, t - 1, kBcgStop);
        return;
    }
    sc[kBcgAlpha] = sc[kBcgRho] / rv;
}

// step t: s.s <= tol2 rr0 converges at the half step (x += alpha p, r = s are still to be applied: state HALF)
__global__ void bcg_check_s(double *__restrict__ sc, int *__restrict__ flags, int t, double tol2) {
    if (flags[kSolverState] != kSolverRun) return;
    const double ss = sc[kBcgSs];
    if (ss <= tol2 * sc[kBcgRr0]) {
        flags[kSolverState] = kBcgHalfStep;
        flags[kSolverStatus] = SPMV_BICG_CONVERGED;
        flags[kSolverSteps] = t;
        flags[kBcgHalf] = 1;
        sc[kBcgLast] = ss;
    }
}

// step t: omega = t.s / t.t; t.t = 0, t.s = 0 or anything not finite breaks down (step t not taken)
__global__ void bcg_set_omega(double *__restrict__ sc, int *__restrict__ flags, int t) {
    if (flags[kSolverState] != kSolverRun) return;
    const double ts = sc[kBcgTs], tt = sc[kBcgTt], omega = ts / tt;
    if (tt == 0.0 || ts == 0.0 || !isfinite(ts) || !isfinite(tt) || !isfinite(omega)) {
        solver_stop(flags, SPMV_BICG_BREAKDOWN_OMEGA, t - 1, kBcgStop);
        return;
    }
    sc[kBcgOmega] = omega;
}

// end of step t: history row t; r.r <= tol2 rr0 converges; r^.r = 0 or not finite breaks down after the step (x is
// the iterate of step t); else beta = (rho' / rho) (alpha / omega), rho = rho'
__global__ void bcg_set_beta(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int t,
                             double tol2) {
    const int state = flags[kSolverState];
    if (state != kSolverRun) {
        if (state == kBcgHalfStep) flags[kSolverState] = kBcgStop;
        hist[t] = sc[kBcgLast];
        return;
    }
    const double rr = sc[kBcgRr], rho_new = sc[kBcgRhoNew];
    sc[kBcgLast] = rr;
    hist[t] = rr;
    if (rr <= tol2 * sc[kBcgRr0]) {
        solver_stop(flags, SPMV_BICG_CONVERGED, t, kBcgStop);
        return;
    }
    if (rho_new == 0.0 || !isfinite(rho_new)) {
        solver_stop(flags, SPMV_BICG_BREAKDOWN_RHO, t, kBcgStop);
        return;
    }
    sc[kBcgBeta] = (rho_new / sc[kBcgRho]) * (sc[kBcgAlpha] / sc[kBcgOmega]);
    sc[kBcgRho] = rho_new;
}

}  // namespace spmv
