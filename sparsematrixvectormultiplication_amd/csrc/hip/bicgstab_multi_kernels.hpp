// bicgstab_multi_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_bicgstab_multi: k independent
// right-preconditioned BiCGSTAB recurrences that share the two SpMMs of a step and the k-wide apply (gfx950).
//
// Everything is laid out as in cg_multi_kernels.hpp: row-major n x k arrays, a lane owns V consecutive columns of one
// row (McgLane: V = 16 / sizeof(T) when a row is whole 16-byte pieces, else 1; the column lanes in the low lane bits),
// a workgroup takes kBlock >> cl rows per pass and strides over the grid.  r^.v is cg_multi's own mcg_dot_partial.  One
// step, after V = A P^ (one SpMM), and again after T = A S^:
//
//   mcg_dot_partial   partials of r^.v                                                        2 arrays per value
//   mbcg_update_s     s = r - alpha v on running columns, partials of s.s; JACOBI: also s^ = dinv[i] s; APPLY: the
//                     k-wide apply follows (NONE: s is the second SpMM's input)               3 to 5
//   mbcg_dot2         partials of t.s and t.t in one pass, two planes                         2
//   mbcg_update_x_r   RUN: x += alpha p^ + omega s^, r = s - omega t, partials of r^.r and r.r; HALF: x += alpha p^,
//                     r = s; two sweeps over the rows, x, p^, s^ and then s, t, r^, r         8 (a stopped column: 9)
//   mbcg_update_p     p = r + beta (p - omega v) on running columns; JACOBI: also p^ = dinv[i] p; APPLY: the apply
//                     follows                                                                 4 to 6
//   mbcg_start / mbcg_set_alpha / mbcg_check_s / mbcg_set_omega / mbcg_set_beta   one wavefront, lane j = column j: the
//                     scalars, the state, the stop and breakdown rules of bicgstab_kernels.hpp per column, the history
//                     rows, steps, status, half flag and the count of active columns
//
// Every stored value is computed in double and rounded once to T, in the expression shapes of the one-wide bcg_*
// kernels.  Reduction order: cg_multi's (a lane's rows in grid-stride order, mcg_rows_sum, the waves in wave order,
// solver_fold); a two-value reduction is two planes part0[g k + j], part1[g k + j], each folded by its own
// solver_reduce of k values.  Nothing depends on j and there are no atomics: permuting the columns permutes the
// results bit for bit and two runs give the same bits.
//
// k = 1 is NOT csr_bicgstab bit for bit: that solver's kernels sum over 16-byte pieces of rows (PieceLane, several rows
// per lane and pass), these sum row by row, so the dot products round differently.  The two agree to rounding.
//
// The state of column j (flags[kMbcgState + j]).  RUN: the step proceeds.  HALF: s_j converged in this step;
// mbcg_update_x_r applies x_j += alpha_j p^_j, r_j = s_j and mbcg_set_beta turns the state to STOP.  STOP: the vector
// kernels write back what they read (or skip the lane), so x, r, s and p keep their bits, and the scalar kernels only
// repeat the last history value.  A stopped column still rides in the SpMMs and the applies; nothing it holds is read
// into another column's value.
#pragma once
#include "cg_multi_kernels.hpp"

namespace spmv {

// the scalar slots, kMcgMaxK doubles each
constexpr int kMbcgRho = 0, kMbcgRr0 = 1, kMbcgRv = 2, kMbcgAlpha = 3, kMbcgSs = 4, kMbcgTs = 5, kMbcgTt = 6,
              kMbcgOmega = 7, kMbcgRhoNew = 8, kMbcgRr = 9, kMbcgBeta = 10, kMbcgLocal = 11, kMbcgSlots = 12;
// the int words: cg_multi's first (state[] in place of act[], 0 still meaning "stopped"; done[] = the steps taken; the
// count of active columns), then status[kMcgMaxK] and half[kMcgMaxK]
constexpr int kMbcgState = kMcgAct, kMbcgStatus = kMcgFlagWords, kMbcgHalf = kMcgFlagWords + kMcgMaxK,
              kMbcgFlagWords = kMcgFlagWords + 2 * kMcgMaxK;
constexpr int kMbcgStop = 0, kMbcgRun = 1, kMbcgHalfStep = 2;
constexpr int kMbcgNone = 0, kMbcgJacobi = 1, kMbcgApply = 2;

// the lane's V sums of two dot products -> the workgroup's partials in the two planes.  mcg_block_partials stages in
// one __shared__ array: the barrier keeps the second use from overwriting what the first is still reading.
template <int V>
__device__ __forceinline__ void mbcg_block_partials2(double (&a)[V], double (&b)[V], int k, int cl, int j0,
                                                     double *__restrict__ part0, double *__restrict__ part1) {
    mcg_block_partials<V>(a, k, cl, j0, part0);
    __syncthreads();
    mcg_block_partials<V>(b, k, cl, j0, part1);
}

// s = r - alpha v on running columns, partials of s.s; JACOBI: s^ = dinv[i] s (a stopped column's s has not changed:
// its s^ is rewritten with the bits it holds).  A lane without a running column leaves s and s^ alone.
template <typename T, int V, int MODE>
__global__ __launch_bounds__(kBlock) void mbcg_update_s(long long n, int k, int cl, const double *__restrict__ sc,
                                                        const int *__restrict__ flags, const T *__restrict__ r,
                                                        const T *__restrict__ v, const T *__restrict__ dinv,
                                                        T *__restrict__ s, T *__restrict__ sh,
                                                        double *__restrict__ part) {
    const McgLane l(cl, V);
    double acc[V], alpha[V];
    bool run[V];
    bool any = false, all = true;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const bool in = l.j0 + c < k;
        acc[c] = 0;
        run[c] = in && flags[kMbcgState + l.j0 + c] == kMbcgRun;
        alpha[c] = in ? sc[kMbcgAlpha * kMcgMaxK + l.j0 + c] : 0.0;
        any = any || run[c];
        all = all && (run[c] || !in);
    }
    if (l.j0 < k && any) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T rv[V], vv[V], sv[V];
            piece_load<T, V>(r + o, rv);
            piece_load<T, V>(v + o, vv);
            if (all) {
#pragma unroll
                for (int c = 0; c < V; ++c) sv[c] = (T)((double)rv[c] - alpha[c] * (double)vv[c]);
            } else {
                piece_load<T, V>(s + o, sv);
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const T sn = (T)((double)rv[c] - alpha[c] * (double)vv[c]);
                    sv[c] = run[c] ? sn : sv[c];
                }
            }
            piece_store<T, V>(s + o, sv);
#pragma unroll
            for (int c = 0; c < V; ++c) acc[c] += (double)sv[c] * (double)sv[c];
            if constexpr (MODE == kMbcgJacobi) {
                const double d = (double)dinv[i];
                T hv[V];
#pragma unroll
                for (int c = 0; c < V; ++c) hv[c] = (T)(d * (double)sv[c]);
                piece_store<T, V>(sh + o, hv);
            }
        }
    }
    mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

// partials of a.b and a.a (t.s with t.t)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mbcg_dot2(long long n, int k, int cl, const T *__restrict__ a,
                                                    const T *__restrict__ b, double *__restrict__ part_ab,
                                                    double *__restrict__ part_aa) {
    const McgLane l(cl, V);
    double ab[V], aa[V];
#pragma unroll
    for (int c = 0; c < V; ++c) ab[c] = aa[c] = 0;
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T av[V], bv[V];
            piece_load<T, V>(a + o, av);
            piece_load<T, V>(b + o, bv);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const double ad = (double)av[c];
                ab[c] += ad * (double)bv[c];
                aa[c] += ad * ad;
            }
        }
    }
    mbcg_block_partials2<V>(ab, aa, k, cl, l.j0, part_ab, part_aa);
}

// RUN: x += alpha p^ + omega s^, r = s - omega t, partials of r^.r and r.r.  HALF: x += alpha p^, r = s.  STOP: x and r
// keep their bits.  PRE = false: s^ is s (sh is not read).  A lane whose columns have all stopped writes nothing.
template <typename T, int V, bool PRE>
__global__ __launch_bounds__(kBlock) void mbcg_update_x_r(long long n, int k, int cl, const double *__restrict__ sc,
                                                          const int *__restrict__ flags, const T *__restrict__ rhat,
                                                          const T *__restrict__ ph, const T *__restrict__ sh,
                                                          const T *__restrict__ s, const T *__restrict__ t,
                                                          T *__restrict__ x, T *__restrict__ r,
                                                          double *__restrict__ part_rho, double *__restrict__ part_rr) {
    const McgLane l(cl, V);
    double rho[V], rr[V], alpha[V], omega[V];
    bool run[V], half[V];
    bool any = false, all = true;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const bool in = l.j0 + c < k;
        const int st = in ? flags[kMbcgState + l.j0 + c] : kMbcgStop;
        rho[c] = rr[c] = 0;
        run[c] = st == kMbcgRun;
        half[c] = st == kMbcgHalfStep;
        alpha[c] = in ? sc[kMbcgAlpha * kMcgMaxK + l.j0 + c] : 0.0;
        omega[c] = in ? sc[kMbcgOmega * kMcgMaxK + l.j0 + c] : 0.0;
        any = any || run[c] || half[c];
        all = all && (run[c] || !in);
    }
    if (l.j0 < k && any) {
        // two sweeps over the lane's rows, x and then r: the arrays of one sweep (x, p^, s^ | s, t, r^, r) and its
        // coefficients fit 64 VGPRs with four fp32 columns per lane, those of both together do not
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T xv[V], pv[V], shv[V];
            piece_load<T, V>(x + o, xv);
            piece_load<T, V>(ph + o, pv);
            piece_load<T, V>((PRE ? sh : s) + o, shv);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const double ap = alpha[c] * (double)pv[c];
                const T xfull = (T)((double)xv[c] + (ap + omega[c] * (double)shv[c]));
                const T xhalf = (T)((double)xv[c] + ap);
                const T xkeep = half[c] ? xhalf : xv[c];
                xv[c] = run[c] ? xfull : xkeep;
            }
            piece_store<T, V>(x + o, xv);
        }
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T sv[V], tv[V], hv[V], rv[V];
            piece_load<T, V>(s + o, sv);
            piece_load<T, V>(t + o, tv);
            piece_load<T, V>(rhat + o, hv);
            if (all) {
#pragma unroll
                for (int c = 0; c < V; ++c) rv[c] = sv[c];
            } else {
                piece_load<T, V>(r + o, rv);  // a stopped column's r is written back
            }
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const T rn = (T)((double)sv[c] - omega[c] * (double)tv[c]);
                const T rkeep = half[c] ? sv[c] : rv[c];
                rv[c] = run[c] ? rn : rkeep;
                rho[c] += (double)hv[c] * (double)rv[c];
                rr[c] += (double)rv[c] * (double)rv[c];
            }
            piece_store<T, V>(r + o, rv);
        }
    }
    mbcg_block_partials2<V>(rho, rr, k, cl, l.j0, part_rho, part_rr);
}

// p = r + beta (p - omega v) on running columns; JACOBI: p^ = dinv[i] p.  A lane without a running column returns: p
// has not changed, so p^ holds the bits it would be given.
template <typename T, int V, int MODE>
__global__ __launch_bounds__(kBlock) void mbcg_update_p(long long n, int k, int cl, const double *__restrict__ sc,
                                                        const int *__restrict__ flags, const T *__restrict__ r,
                                                        const T *__restrict__ v, const T *__restrict__ dinv,
                                                        T *__restrict__ p, T *__restrict__ ph) {
    const McgLane l(cl, V);
    if (l.j0 >= k) return;
    double beta[V], omega[V];
    bool run[V];
    bool any = false;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const bool in = l.j0 + c < k;
        run[c] = in && flags[kMbcgState + l.j0 + c] == kMbcgRun;
        beta[c] = in ? sc[kMbcgBeta * kMcgMaxK + l.j0 + c] : 0.0;
        omega[c] = in ? sc[kMbcgOmega * kMcgMaxK + l.j0 + c] : 0.0;
        any = any || run[c];
    }
    if (!any) return;
    for (long long i = l.row; i < n; i += l.stride) {
        const long long o = i * k + l.j0;
        T rv[V], vv[V], pv[V];
        piece_load<T, V>(r + o, rv);
        piece_load<T, V>(v + o, vv);
        piece_load<T, V>(p + o, pv);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const T pn = (T)((double)rv[c] + beta[c] * ((double)pv[c] - omega[c] * (double)vv[c]));
            pv[c] = run[c] ? pn : pv[c];
        }
        piece_store<T, V>(p + o, pv);
        if constexpr (MODE == kMbcgJacobi) {
            const double d = (double)dinv[i];
            T hv[V];
#pragma unroll
            for (int c = 0; c < V; ++c) hv[c] = (T)(d * (double)pv[c]);
            piece_store<T, V>(ph + o, hv);
        }
    }
}

// ---- the scalar kernels: one wavefront, lane j = column j.  A stop writes the status and the steps taken and never
// touches x.
__device__ __forceinline__ void mbcg_stop(int *__restrict__ flags, int j, int status, int steps) {
    flags[kMbcgState + j] = kMbcgStop;
    flags[kMbcgStatus + j] = status;
    flags[kMcgDone + j] = steps;
}

// rr0 = r.r (slot kMbcgRr0) with r = r^ = b, so rho = r^.r = rr0; history row 0; rr0 = 0 (b_j = 0) stops at step 0,
// converged
__global__ __launch_bounds__(64) void mbcg_start(double *__restrict__ sc, int *__restrict__ flags,
                                                 double *__restrict__ hist, int k, int iters) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const double rr0 = sc[kMbcgRr0 * kMcgMaxK + j];
        sc[kMbcgRho * kMcgMaxK + j] = rr0;
        hist[j] = rr0;
        flags[kMbcgState + j] = kMbcgRun;
        flags[kMcgDone + j] = iters;
        flags[kMbcgStatus + j] = SPMV_BICG_RAN_ALL;
        flags[kMbcgHalf + j] = 0;
        live = true;
        if (rr0 == 0.0) mbcg_stop(flags, j, SPMV_BICG_CONVERGED, 0), live = false;
    }
    mcg_count_active(flags, live);
}

// step t: alpha = rho / r^.v; r^.v = 0 or not finite breaks down (step t not taken)
__global__ __launch_bounds__(64) void mbcg_set_alpha(double *__restrict__ sc, int *__restrict__ flags, int k, int t) {
    const int j = threadIdx.x;
    if (j >= k || flags[kMbcgState + j] != kMbcgRun) return;
    const double rv = sc[kMbcgRv * kMcgMaxK + j];
    if (rv == 0.0 || !isfinite(rv)) {
        mbcg_stop(flags, j, SPMV_BICG_BREAKDOWN_RHO, t - 1);
        return;
    }
    sc[kMbcgAlpha * kMcgMaxK + j] = sc[kMbcgRho * kMcgMaxK + j] / rv;
}

// step t: s.s <= tol2 rr0 converges at the half step (x += alpha p^, r = s are still to be applied: state HALF)
__global__ __launch_bounds__(64) void mbcg_check_s(const double *__restrict__ sc, int *__restrict__ flags, int k, int t,
                                                   double tol2) {
    const int j = threadIdx.x;
    if (j >= k || flags[kMbcgState + j] != kMbcgRun) return;
    if (sc[kMbcgSs * kMcgMaxK + j] <= tol2 * sc[kMbcgRr0 * kMcgMaxK + j]) {
        flags[kMbcgState + j] = kMbcgHalfStep;
        flags[kMbcgStatus + j] = SPMV_BICG_CONVERGED;
        flags[kMcgDone + j] = t;
        flags[kMbcgHalf + j] = 1;
    }
}

// step t: omega = t.s / t.t; t.t = 0, t.s = 0 or anything not finite breaks down (step t not taken)
__global__ __launch_bounds__(64) void mbcg_set_omega(double *__restrict__ sc, int *__restrict__ flags, int k, int t) {
    const int j = threadIdx.x;
    if (j >= k || flags[kMbcgState + j] != kMbcgRun) return;
    const double ts = sc[kMbcgTs * kMcgMaxK + j], tt = sc[kMbcgTt * kMcgMaxK + j], omega = ts / tt;
    if (tt == 0.0 || ts == 0.0 || !isfinite(ts) || !isfinite(tt) || !isfinite(omega)) {
        mbcg_stop(flags, j, SPMV_BICG_BREAKDOWN_OMEGA, t - 1);
        return;
    }
    sc[kMbcgOmega * kMcgMaxK + j] = omega;
}

// end of step t: history row t (hist points at it).  STOP: row t - 1 again.  HALF: s.s of this step, then STOP.  RUN:
// r.r; r.r <= tol2 rr0 converges; r^.r = 0 or not finite breaks down after the step (x is the iterate of step t); else
// beta = (rho' / rho) (alpha / omega), rho = rho'
__global__ __launch_bounds__(64) void mbcg_set_beta(double *__restrict__ sc, int *__restrict__ flags,
                                                    double *__restrict__ hist, int k, int t, double tol2) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const int state = flags[kMbcgState + j];
        if (state == kMbcgStop) {
            hist[j] = hist[j - k];
        } else if (state == kMbcgHalfStep) {
            hist[j] = sc[kMbcgSs * kMcgMaxK + j];
            flags[kMbcgState + j] = kMbcgStop;
        } else {
            const double rr = sc[kMbcgRr * kMcgMaxK + j], rho_new = sc[kMbcgRhoNew * kMcgMaxK + j];
            hist[j] = rr;
            if (rr <= tol2 * sc[kMbcgRr0 * kMcgMaxK + j]) {
                mbcg_stop(flags, j, SPMV_BICG_CONVERGED, t);
            } else if (rho_new == 0.0 || !isfinite(rho_new)) {
                mbcg_stop(flags, j, SPMV_BICG_BREAKDOWN_RHO, t);
            } else {
                sc[kMbcgBeta * kMcgMaxK + j] =
                    (rho_new / sc[kMbcgRho * kMcgMaxK + j]) * (sc[kMbcgAlpha * kMcgMaxK + j] / sc[kMbcgOmega * kMcgMaxK + j]);
                sc[kMbcgRho * kMcgMaxK + j] = rho_new;
                live = true;
            }
        }
    }
    mcg_count_active(flags, live);
}

}  // namespace spmv
