// minres_multi_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_minres_multi: k independent MINRES
// recurrences, each with its own shift, that share the one SpMM of a step and the k-wide apply (gfx950).
//
// Everything is laid out as in cg_multi_kernels.hpp: row-major n x k arrays, a lane owns V consecutive columns of one
// row (McgLane: V = 16 / sizeof(T) when a row is whole 16-byte pieces, else 1; the column lanes in the low lane bits),
// a workgroup takes kBlock >> cl rows per pass and strides over the grid.  The dot of t and M^-1 t after a k-wide apply
// is cg_multi's own mcg_dot_partial.  One step, after A_V = A V (one SpMM):
//
//   mmr_lanczos_a   t = a - shift v - (beta / oldb) r1 over r1's buffer (r1 is dead after), partials of v.t    4 arrays
//   mmr_lanczos_b   t -= (alfa / beta) r2; NONE: partials of t.t (the next beta^2); JACOBI: y = dinv[i] t and the
//                   partials of t.y in the same pass; APPLY: no partials, the k-wide apply and mcg_dot_partial
//                   follow                                                                                3 to 4
//   mmr_update      w = (v - oldeps w1 - delta w2) / gamma over w1's buffer, x += phi w, then the next v = y / beta
//                   into the SpMM's input; two sweeps over the lane's rows, v, w1, w2, x and then y, v    8
//   mmr_start / mmr_set_alfa / mmr_rotate   one wavefront, lane j = column j: the Lanczos scalars, the Givens rotation,
//                   the stop and breakdown rules of minres_kernels.hpp per column, the history rows, steps, status and
//                   the count of active columns
//
// Every stored value is computed in double and rounded once to T, in the expression shapes of the one-wide mr_*
// kernels; the dots are taken of the stored values.  Reduction order: cg_multi's (a lane's rows in grid-stride order,
// mcg_rows_sum, the waves in wave order, solver_fold, the ranks in rank order).  Nothing depends on j and there are no
// atomics: permuting the columns with their shifts permutes the results bit for bit and two runs give the same bits.
//
// k = 1 is NOT csr_minres bit for bit: that solver's kernels sum over 16-byte pieces of rows (PieceLane), these sum row
// by row, so the dot products round differently.  The two agree to rounding.
//
// The state of column j (flags[kMmrState + j]).  RUN: the step proceeds.  FINAL: the column converged in this step and
// still owes its x += phi w: mmr_update applies w and x (not v: beta may be 0) and the next mmr_rotate turns the state
// to STOP.  STOP: the vector kernels write back what they read (or skip the lane), so x, r1, r2, w and v keep their
// bits, and mmr_rotate only repeats the last history value.  A stopped column still rides in the SpMM and the applies;
// nothing it holds, a NaN included, is read into another column's value.  The host swaps the roles of the two r
// buffers and of the two w buffers after every step, for every column alike.
#pragma once
#include "cg_multi_kernels.hpp"

namespace spmv {

// the scalar slots, kMcgMaxK doubles each
constexpr int kMmrBb0 = 0, kMmrBeta = 1, kMmrOldb = 2, kMmrAlfa = 3, kMmrBb = 4, kMmrDbar = 5, kMmrEpsln = 6, kMmrCs = 7,
              kMmrSn = 8, kMmrPhibar = 9, kMmrC1 = 10, kMmrC2 = 11, kMmrOldeps = 12, kMmrDelta = 13, kMmrGamma = 14,
              kMmrPhi = 15, kMmrLast = 16, kMmrShift = 17, kMmrLocal = 18, kMmrSlots = 19;
// the int words: cg_multi's first (state[] in place of act[], 0 still meaning "stopped"; done[] = the steps taken; the
// count of running columns), then status[kMcgMaxK]
constexpr int kMmrState = kMcgAct, kMmrStatus = kMcgFlagWords, kMmrFlagWords = kMcgFlagWords + kMcgMaxK;
constexpr int kMmrStop = 0, kMmrRun = 1, kMmrFinal = 2;
constexpr int kMmrNone = 0, kMmrJacobi = 1, kMmrApply = 2;

// step `step`: t = a - shift v (step >= 2: - c1 r1, c1 = beta / oldb) on running columns, written over r1; partials of
// v.t.  A column that is not running keeps r1; a lane without a running column writes nothing.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mmr_lanczos_a(long long n, int k, int cl, const double *__restrict__ sc,
                                                        const int *__restrict__ flags, int step,
                                                        const T *__restrict__ a, const T *__restrict__ v,
                                                        T *__restrict__ r1, double *__restrict__ part) {
    const McgLane l(cl, V);
    const bool three = step >= 2;
    double acc[V], shift[V], c1[V];
    bool run[V];
    bool any = false, all = true;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const bool in = l.j0 + c < k;
        acc[c] = 0;
        run[c] = in && flags[kMmrState + l.j0 + c] == kMmrRun;
        shift[c] = in ? sc[kMmrShift * kMcgMaxK + l.j0 + c] : 0.0;
        c1[c] = in && three ? sc[kMmrC1 * kMcgMaxK + l.j0 + c] : 0.0;
        any = any || run[c];
        all = all && (run[c] || !in);
    }
    if (l.j0 < k && any) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T av[V], vv[V], rv[V];
            piece_load<T, V>(a + o, av);
            piece_load<T, V>(v + o, vv);
            if (three || !all) {
                piece_load<T, V>(r1 + o, rv);
            } else {
#pragma unroll
                for (int c = 0; c < V; ++c) rv[c] = T(0);
            }
#pragma unroll
            for (int c = 0; c < V; ++c) {
                double t = (double)av[c] - shift[c] * (double)vv[c];
                if (three) t -= c1[c] * (double)rv[c];
                rv[c] = run[c] ? (T)t : rv[c];
                acc[c] += (double)vv[c] * (double)rv[c];
            }
            piece_store<T, V>(r1 + o, rv);
        }
    }
    mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

// t -= c2 r2 (c2 = alfa / beta) on running columns.  NONE: partials of t.t.  JACOBI: y = dinv[i] t, partials of t.y (a
// stopped column's t has not changed: its y is rewritten with the bits it holds).  APPLY: t alone.  A lane without a
// running column writes nothing.
template <typename T, int V, int MODE>
__global__ __launch_bounds__(kBlock) void mmr_lanczos_b(long long n, int k, int cl, const double *__restrict__ sc,
                                                        const int *__restrict__ flags, const T *__restrict__ r2,
                                                        const T *__restrict__ dinv, T *__restrict__ t,
                                                        T *__restrict__ y, double *__restrict__ part) {
    const McgLane l(cl, V);
    double acc[V], c2[V];
    bool run[V];
    bool any = false;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const bool in = l.j0 + c < k;
        acc[c] = 0;
        run[c] = in && flags[kMmrState + l.j0 + c] == kMmrRun;
        c2[c] = in ? sc[kMmrC2 * kMcgMaxK + l.j0 + c] : 0.0;
        any = any || run[c];
    }
    if (l.j0 < k && any) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T tv[V], rv[V];
            piece_load<T, V>(t + o, tv);
            piece_load<T, V>(r2 + o, rv);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const T tn = (T)((double)tv[c] - c2[c] * (double)rv[c]);
                tv[c] = run[c] ? tn : tv[c];
            }
            piece_store<T, V>(t + o, tv);
            if constexpr (MODE == kMmrNone) {
#pragma unroll
                for (int c = 0; c < V; ++c) acc[c] += (double)tv[c] * (double)tv[c];
            } else if constexpr (MODE == kMmrJacobi) {
                const double d = (double)dinv[i];
                T yv[V];
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    yv[c] = (T)(d * (double)tv[c]);
                    acc[c] += (double)tv[c] * (double)yv[c];
                }
                piece_store<T, V>(y + o, yv);
            }
        }
    }
    if constexpr (MODE != kMmrApply) mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

// end of step `step`.  RUN: w = (v - oldeps w1 - delta w2) / gamma over w1, x += phi w, then the next v = y / beta (the
// new beta).  FINAL: w and x alone.  STOP: nothing changes.  step = 0 (before step 1): v = y / beta alone.  A lane
// whose columns have all stopped writes nothing.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mmr_update(long long n, int k, int cl, const double *__restrict__ sc,
                                                     const int *__restrict__ flags, int step, const T *__restrict__ y,
                                                     const T *__restrict__ w2, T *__restrict__ w1, T *__restrict__ x,
                                                     T *__restrict__ v) {
    const McgLane l(cl, V);
    if (l.j0 >= k) return;
    // bit c: column c runs; bit V + c: column c runs or is in its final step
    unsigned mask = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int st = l.j0 + c < k ? flags[kMmrState + l.j0 + c] : kMmrStop;
        if (st == kMmrRun) mask |= 1u << c;
        if (st != kMmrStop) mask |= 1u << (V + c);
    }
    if (!mask) return;
    // two sweeps over the lane's rows, w and x and then v: the arrays of one sweep (v, w1, w2, x | y, v) and its
    // coefficients stay in registers, those of both together would be eight arrays and five coefficients a column.
    // With four fp32 columns a lane the first sweep still holds 88 VGPRs (16 fp64 coefficients, four fp64 divisions) and
    // spills when forced under 64; it streams at the rate of the fp32 passes that fit 64 (profiles/minres_multi_step.md)
    if (step > 0) {
        double oldeps[V], delta[V], gamma[V], phi[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int j = l.j0 + c < k ? l.j0 + c : l.j0;
            oldeps[c] = sc[kMmrOldeps * kMcgMaxK + j];
            delta[c] = sc[kMmrDelta * kMcgMaxK + j];
            gamma[c] = sc[kMmrGamma * kMcgMaxK + j];
            phi[c] = sc[kMmrPhi * kMcgMaxK + j];
        }
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T vv[V], av[V], bv[V], xv[V];
            piece_load<T, V>(v + o, vv);
            piece_load<T, V>(w1 + o, av);
            piece_load<T, V>(w2 + o, bv);
            piece_load<T, V>(x + o, xv);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const T wn = (T)((((double)vv[c] - oldeps[c] * (double)av[c]) - delta[c] * (double)bv[c]) / gamma[c]);
                const T xn = (T)((double)xv[c] + phi[c] * (double)wn);
                const bool live = (mask >> (V + c)) & 1u;
                av[c] = live ? wn : av[c];
                xv[c] = live ? xn : xv[c];
            }
            piece_store<T, V>(w1 + o, av);
            piece_store<T, V>(x + o, xv);
        }
    }
    constexpr unsigned kRunBits = (1u << V) - 1u;
    if (!(mask & kRunBits)) return;
    const bool all = (mask & kRunBits) == kRunBits;
    double beta[V];
#pragma unroll
    for (int c = 0; c < V; ++c) beta[c] = sc[kMmrBeta * kMcgMaxK + (l.j0 + c < k ? l.j0 + c : l.j0)];
    for (long long i = l.row; i < n; i += l.stride) {
        const long long o = i * k + l.j0;
        T yv[V], vv[V];
        piece_load<T, V>(y + o, yv);
        if (!all) piece_load<T, V>(v + o, vv);  // a column that does not run keeps its v
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const T vn = (T)((double)yv[c] / beta[c]);
            vv[c] = (mask >> c) & 1u ? vn : vv[c];
        }
        piece_store<T, V>(v + o, vv);
    }
}

// ---- the scalar kernels: one wavefront, lane j = column j.  A stop writes the status and the steps taken; only a
// converged step's mmr_update still touches x.
__device__ __forceinline__ void mmr_stop(int *__restrict__ flags, int j, int status, int steps, int state = kMmrStop) {
    flags[kMmrState + j] = state;
    flags[kMmrStatus + j] = status;
    flags[kMcgDone + j] = steps;
}

// bb0 = r2.y (slot kMmrBb) with r2 = b, y = M^-1 b or b: history row 0, beta = phibar = sqrt(bb0), cs = -1, the rest 0.
// bb0 not finite or < 0 (M not positive definite) breaks down at step 0; bb0 = 0 (b_j = 0) has converged at step 0.
__global__ __launch_bounds__(64) void mmr_start(double *__restrict__ sc, int *__restrict__ flags,
                                                double *__restrict__ hist, int k, int iters) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const double bb0 = sc[kMmrBb * kMcgMaxK + j];
        sc[kMmrBb0 * kMcgMaxK + j] = bb0;
        sc[kMmrLast * kMcgMaxK + j] = bb0;
        hist[j] = bb0;
        flags[kMmrState + j] = kMmrRun;
        flags[kMcgDone + j] = iters;
        flags[kMmrStatus + j] = SPMV_MINRES_RAN_ALL;
        if (!isfinite(bb0) || bb0 < 0.0) {
            mmr_stop(flags, j, SPMV_MINRES_BREAKDOWN, 0);
        } else if (bb0 == 0.0) {
            mmr_stop(flags, j, SPMV_MINRES_CONVERGED, 0);
        } else {
            const double beta = sqrt(bb0);
            sc[kMmrBeta * kMcgMaxK + j] = beta;
            sc[kMmrPhibar * kMcgMaxK + j] = beta;
            sc[kMmrOldb * kMcgMaxK + j] = 0.0;
            sc[kMmrDbar * kMcgMaxK + j] = 0.0;
            sc[kMmrEpsln * kMcgMaxK + j] = 0.0;
            sc[kMmrCs * kMcgMaxK + j] = -1.0;
            sc[kMmrSn * kMcgMaxK + j] = 0.0;
            sc[kMmrC1 * kMcgMaxK + j] = 0.0;
            live = true;
        }
    }
    mcg_count_active(flags, live);
}

// step t: alfa = v.t (slot kMmrAlfa), c2 = alfa / beta; alfa not finite breaks down (step t not taken)
__global__ __launch_bounds__(64) void mmr_set_alfa(double *__restrict__ sc, int *__restrict__ flags, int k, int t) {
    const int j = threadIdx.x;
    if (j >= k || flags[kMmrState + j] != kMmrRun) return;
    const double alfa = sc[kMmrAlfa * kMcgMaxK + j], c2 = alfa / sc[kMmrBeta * kMcgMaxK + j];
    if (!isfinite(alfa) || !isfinite(c2)) {
        mmr_stop(flags, j, SPMV_MINRES_BREAKDOWN, t - 1);
        return;
    }
    sc[kMmrC2 * kMcgMaxK + j] = c2;
}

// step t, with bb = r2.y (slot kMmrBb): the next beta, the rotation, history row t (hist points at it).  STOP, and
// FINAL of the step before (then turned to STOP): the last value again.  bb < 0 (M not positive definite), gamma = 0
// or anything not finite breaks down (step t not taken: x stays the iterate of step t - 1); phibar^2 <= tol2 bb0
// converges at step t, whose mmr_update still runs (state FINAL).
__global__ __launch_bounds__(64) void mmr_rotate(double *__restrict__ sc, int *__restrict__ flags,
                                                 double *__restrict__ hist, int k, int t, double tol2) {
#pragma clang fp contract(off)
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const int state = flags[kMmrState + j];
        if (state != kMmrRun) {
            hist[j] = sc[kMmrLast * kMcgMaxK + j];
            flags[kMmrState + j] = kMmrStop;
        } else {
            const double bb = sc[kMmrBb * kMcgMaxK + j], alfa = sc[kMmrAlfa * kMcgMaxK + j];
            const double oldb = sc[kMmrBeta * kMcgMaxK + j];
            const double cs0 = sc[kMmrCs * kMcgMaxK + j], sn0 = sc[kMmrSn * kMcgMaxK + j];
            const double dbar0 = sc[kMmrDbar * kMcgMaxK + j], phibar0 = sc[kMmrPhibar * kMcgMaxK + j];
            const double beta = sqrt(bb);  // NaN for bb < 0
            const double oldeps = sc[kMmrEpsln * kMcgMaxK + j];
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
                hist[j] = sc[kMmrLast * kMcgMaxK + j];
                mmr_stop(flags, j, SPMV_MINRES_BREAKDOWN, t - 1);
            } else {
                sc[kMmrOldb * kMcgMaxK + j] = oldb;
                sc[kMmrBeta * kMcgMaxK + j] = beta;
                sc[kMmrOldeps * kMcgMaxK + j] = oldeps;
                sc[kMmrDelta * kMcgMaxK + j] = delta;
                sc[kMmrEpsln * kMcgMaxK + j] = epsln;
                sc[kMmrDbar * kMcgMaxK + j] = dbar;
                sc[kMmrGamma * kMcgMaxK + j] = gamma;
                sc[kMmrCs * kMcgMaxK + j] = cs;
                sc[kMmrSn * kMcgMaxK + j] = sn;
                sc[kMmrPhi * kMcgMaxK + j] = phi;
                sc[kMmrPhibar * kMcgMaxK + j] = phibar;
                sc[kMmrC1 * kMcgMaxK + j] = c1;
                sc[kMmrLast * kMcgMaxK + j] = rr;
                hist[j] = rr;
                if (rr <= tol2 * sc[kMmrBb0 * kMcgMaxK + j]) mmr_stop(flags, j, SPMV_MINRES_CONVERGED, t, kMmrFinal);
                else live = true;
            }
        }
    }
    mcg_count_active(flags, live);
}

}  // namespace spmv
