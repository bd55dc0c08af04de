// minres_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_minres: MINRES (Paige and Saunders 1975) for a
// symmetric, possibly indefinite A - shift I with an optional SPD preconditioner M, x0 = 0 (gfx950).
//
// One step, after a = A v (the handle's SpMV):
//
//   mr_lanczos_a     t = a - shift v - (beta / oldb) r1 over r1's buffer (r1 is dead after), v.t     4 values per row
//   mr_lanczos_b     t -= (alfa / beta) r2, t.t (without M this is the next beta^2)                  3
//   mr_dot           with M only, after y = M^-1 t (the preconditioner's own launches): t.y          2
//   mr_update        w = (v - oldeps w1 - delta w2) / gamma over w1's buffer, x += phi w,
//                    the next v = y / beta into the SpMV's input                                     8
//   mr_start / mr_set_alfa / mr_rotate   one thread: the Lanczos scalars, the Givens rotation, the stop and
//                    breakdown rules and the history
//
// The host swaps the roles of the two r buffers and of the two w buffers after every step; it knows the step index.
// Every vector is indexed by global row; a kernel covers the rows [lo, hi) of this rank in pieces of V = 16 / sizeof(T)
// rows (piece_load / piece_store, PieceLane: solver_ops.hpp); the rows outside [lo, hi) are neither read nor written.
// Arithmetic is in double, every stored value is rounded once to T, and the dots are taken of the stored values.  The
// partials are folded and added over the ranks by solver_reduce, in the order of solver_ops.hpp.  The grid depends on
// hi - lo only.
//
// The state word.  RUN: the step proceeds.  STOP: the vector kernels return before they write anything and the scalar
// kernels only repeat the last history value, so a stopped solve can go on being launched (tol = 0) with x untouched.
// The step that converges still owes its x += phi w: mr_rotate turns the state to STOP and leaves the step's index in
// the word kMrFinal, and mr_update of exactly that step applies w and x (not v: beta may be 0 there).
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kMrBlocks = 2048;  // grid cap of the vector kernels

// the scalar slots (doubles)
constexpr int kMrBb0 = 0, kMrBeta = 1, kMrOldb = 2, kMrAlfa = 3, kMrBb = 4, kMrDbar = 5, kMrEpsln = 6, kMrCs = 7,
              kMrSn = 8, kMrPhibar = 9, kMrC1 = 10, kMrC2 = 11, kMrOldeps = 12, kMrDelta = 13, kMrGamma = 14,
              kMrPhi = 15, kMrLast = 16, kMrLocal = 17, kMrSlots = 20;
// the int words: the stop flags of solver_ops.hpp, word 3 = the step that converged (its mr_update still runs)
constexpr int kMrFinal = 3;

// partials of a.b on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mr_dot(long long lo, long long hi, const int *__restrict__ flags,
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

// step k: t = a - shift v (k >= 2: - c1 r1, c1 = beta / oldb) on [lo, hi), written over r1; partials of v.t
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mr_lanczos_a(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, int k, double shift,
                                                       const T *__restrict__ a, const T *__restrict__ v,
                                                       T *__restrict__ r1, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const bool three = k >= 2;
    const double c1 = three ? sc[kMrC1] : 0.0;
    double acc[1] = {0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T av[V], vv[V], rv[V];
        piece_load<T, V>(a, i0, lo, hi, av);
        piece_load<T, V>(v, i0, lo, hi, vv);
        if (three) {
            piece_load<T, V>(r1, i0, lo, hi, rv);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) rv[j] = T(0);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double t = (double)av[j] - shift * (double)vv[j];
            if (three) t -= c1 * (double)rv[j];
            rv[j] = (T)t;
            acc[0] += (double)vv[j] * (double)rv[j];
        }
        piece_store<T, V>(r1, i0, lo, hi, rv);
    }
    block_partials<1>(acc, part);
}

// t -= c2 r2 (c2 = alfa / beta) on [lo, hi); partials of t.t
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mr_lanczos_b(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, const T *__restrict__ r2,
                                                       T *__restrict__ t, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double c2 = sc[kMrC2];
    double acc[1] = {0.0};
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T tv[V], rv[V];
        piece_load<T, V>(t, i0, lo, hi, tv);
        piece_load<T, V>(r2, i0, lo, hi, rv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            tv[j] = (T)((double)tv[j] - c2 * (double)rv[j]);
            acc[0] += (double)tv[j] * (double)tv[j];
        }
        piece_store<T, V>(t, i0, lo, hi, tv);
    }
    block_partials<1>(acc, part);
}

// end of step k: w = (v - oldeps w1 - delta w2) / gamma over w1, x += phi w, then the next v = y / beta (the new
// beta) on [lo, hi).  k = 0 (before step 1): v = y / beta alone.  The step that stopped converged (kMrFinal = k):
// w and x alone.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mr_update(long long lo, long long hi, const int *__restrict__ flags,
                                                    const double *__restrict__ sc, int k, const T *__restrict__ y,
                                                    const T *__restrict__ w2, T *__restrict__ w1, T *__restrict__ x,
                                                    T *__restrict__ v) {
    const bool run = flags[kSolverState] == kSolverRun;
    if (!run && !(k > 0 && flags[kMrFinal] == k)) return;
    const double beta = sc[kMrBeta];
    if (k == 0) {
        for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            T yv[V];
            piece_load<T, V>(y, i0, lo, hi, yv);
#pragma unroll
            for (int j = 0; j < V; ++j) yv[j] = (T)((double)yv[j] / beta);
            piece_store<T, V>(v, i0, lo, hi, yv);
        }
        return;
    }
    const double oldeps = sc[kMrOldeps], delta = sc[kMrDelta], gamma = sc[kMrGamma], phi = sc[kMrPhi];
    for (PieceLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T vv[V], av[V], bv[V], xv[V];
        piece_load<T, V>(v, i0, lo, hi, vv);
        piece_load<T, V>(w1, i0, lo, hi, av);
        piece_load<T, V>(w2, i0, lo, hi, bv);
        piece_load<T, V>(x, i0, lo, hi, xv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            av[j] = (T)((((double)vv[j] - oldeps * (double)av[j]) - delta * (double)bv[j]) / gamma);
            xv[j] = (T)((double)xv[j] + phi * (double)av[j]);
        }
        piece_store<T, V>(w1, i0, lo, hi, av);
        piece_store<T, V>(x, i0, lo, hi, xv);
        if (run) {
            piece_load<T, V>(y, i0, lo, hi, vv);
#pragma unroll
            for (int j = 0; j < V; ++j) vv[j] = (T)((double)vv[j] / beta);
            piece_store<T, V>(v, i0, lo, hi, vv);
        }
    }
}

// ---- the scalar kernels: one thread each.  A stop writes the status and the steps taken; only a converged step's
// mr_update still touches x.

// bb0 = r2.y (slot kMrBb) with r2 = b, y = M^-1 b or b: history row 0, beta = phibar = sqrt(bb0), cs = -1, the rest 0.
// bb0 not finite or < 0 (M not positive definite) breaks down at step 0; bb0 = 0 (b = 0) has converged at step 0.
__global__ void mr_start(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int iters) {
    const double bb0 = sc[kMrBb];
    sc[kMrBb0] = bb0;
    sc[kMrLast] = bb0;
    hist[0] = bb0;
    flags[kSolverState] = kSolverRun;
    flags[kSolverSteps] = iters;
    flags[kSolverStatus] = SPMV_MINRES_RAN_ALL;
    flags[kMrFinal] = -1;
    if (!isfinite(bb0) || bb0 < 0.0) {
        solver_stop(flags, SPMV_MINRES_BREAKDOWN, 0);
        return;
    }
    if (bb0 == 0.0) {
        solver_stop(flags, SPMV_MINRES_CONVERGED, 0);
        return;
    }
    const double beta = sqrt(bb0);
    sc[kMrBeta] = beta;
    sc[kMrPhibar] = beta;
    sc[kMrOldb] = 0.0;
    sc[kMrDbar] = 0.0;
    sc[kMrEpsln] = 0.0;
    sc[kMrCs] = -1.0;
    sc[kMrSn] = 0.0;
    sc[kMrC1] = 0.0;
}

// step k: alfa = v.t (slot kMrAlfa), c2 = alfa / beta; alfa not finite breaks down (step k not taken)
__global__ void mr_set_alfa(double *__restrict__ sc, int *__restrict__ flags, int k) {
    if (flags[kSolverState] != kSolverRun) return;
    const double alfa = sc[kMrAlfa], c2 = alfa / sc[kMrBeta];
    if (!isfinite(alfa) || !isfinite(c2)) {
        solver_stop(flags, SPMV_MINRES_BREAKDOWN, k - 1);
        return;
    }
    sc[kMrC2] = c2;
}

// step k, with bb = r2.y (slot kMrBb): the next beta, the rotation, history row k.  bb < 0 (M not positive
// definite), gamma = 0 or anything not finite breaks down (step k not taken: x stays the iterate of step k - 1);
// phibar^2 <= tol2 bb0 converges at step k, whose mr_update still runs (kMrFinal = k).
__global__ void mr_rotate(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int k,
                          double tol2) {
#pragma clang fp contract(off)
    if (flags[kSolverState] != kSolverRun) {
        hist[k] = sc[kMrLast];
        return;
    }
    const double bb = sc[kMrBb], alfa = sc[kMrAlfa], oldb = sc[kMrBeta];
    const double cs0 = sc[kMrCs], sn0 = sc[kMrSn], dbar0 = sc[kMrDbar], phibar0 = sc[kMrPhibar];
    const double beta = sqrt(bb);  // NaN for bb < 0
    const double oldeps = sc[kMrEpsln];
    const double delta = cs0 * dbar0 + sn0 * alfa;
    const double gbar = sn0 * dbar0 - cs0 * alfa;
    const double epsln = sn0 * beta;
    const double dbar = -cs0 * beta;
    const double gamma = sqrt(gbar * gbar + beta * beta);
    const double cs = gbar / gamma, sn = beta / gamma;
    const double phi = cs * phibar0, phibar = sn * phibar0;
    const double c1 = beta / oldb, rr = phibar * phibar;
    const bool finite = isfinite(bb) && isfinite(delta) && isfinite(epsln) && isfinite(dbar) && isfinite(gamma) &&
                        isfinite(phi) && isfinite(phibar) && isfinite(c1) && isfinite(rr);
    if (!(bb >= 0.0) || gamma == 0.0 || !finite) {
        hist[k] = sc[kMrLast];
        solver_stop(flags, SPMV_MINRES_BREAKDOWN, k - 1);
        return;
    }
    sc[kMrOldb] = oldb;
    sc[kMrBeta] = beta;
    sc[kMrOldeps] = oldeps;
    sc[kMrDelta] = delta;
    sc[kMrEpsln] = epsln;
    sc[kMrDbar] = dbar;
    sc[kMrGamma] = gamma;
    sc[kMrCs] = cs;
    sc[kMrSn] = sn;
    sc[kMrPhi] = phi;
    sc[kMrPhibar] = phibar;
    sc[kMrC1] = c1;
    sc[kMrLast] = rr;
    hist[k] = rr;
    if (rr <= tol2 * sc[kMrBb0]) {
        solver_stop(flags, SPMV_MINRES_CONVERGED, k);
        flags[kMrFinal] = k;
    }
}

}  // namespace spmv
