// pcg_multi_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_pcg_multi and of the k-wide preconditioner
// apply: k independent PCG recurrences that share one SpMM per step (gfx950).
//
// Everything is laid out as in cg_multi_kernels.hpp: row-major n x k arrays, a lane owns V consecutive columns of one
// row (McgLane: V = 16 / sizeof(T) when a row is whole 16-byte pieces, else 1; the column lanes in the low lane bits),
// a workgroup takes kBlock >> cl rows per pass and strides over the grid.  p.q and p = z + beta p are cg_multi's own
// mcg_dot_partial and mcg_update_p (the slots kMcgPq, kMcgAlpha, kMcgBeta and the act words are shared); new here:
//
//   mpcg_start_dots   at the start: r.r and r.z per column; JAC: z = dinv[i] r first; else z is r and only r.r is made
//   mpcg_update_x_r   x_j += alpha_j p_j, r_j -= alpha_j q_j on live columns; NONE: partials of r.r; JACOBI: z = dinv[i] r
//                     and partials of r.r and r.z; APPLY: no partials, an apply follows
//   mpc_apply         the k-wide block-Jacobi apply, z[i, j] = sum_c inv_kb[c][ii] r[kb b + c, j] in pc_apply's order
//                     (c ascending, the first term the plain product, in double, rounded once); DOTS: r.r and r.z too
//   mpcg_dots         r.r and r.z after an apply that made none (FSAI's two SpMMs)
//   mpcg_start / mpcg_set_alpha / mpcg_set_beta   one wavefront, lane j = column j: the scalars, the stop rules of
//                     csr_pcg per column, both histories, steps, status and the count of active columns
//
// Reduction order: cg_multi's (a lane's rows in grid-stride order, mcg_rows_sum, the waves in order, solver_fold), for
// r.r and for r.z alike; the two sets of partials are two planes part_rr[g k + j], part_rz[g k + j], each folded by its
// own solver_reduce of k values.  Nothing depends on j and there are no atomics.  With k = 1 the lanes walk single rows
// as PieceLane does and the sums are block_partials': on csr_pcg's grid that is csr_pcg bit for bit.
//
// Stopped columns (act[j] == 0) keep x, r, z and p: the kernels write back what they read.
#pragma once
#include "cg_multi_kernels.hpp"
#include "precond_kernels.hpp"

namespace spmv {

// the scalar slots, kMcgMaxK doubles each: cg_multi's first five (kMcgRs holds the current r.z, kMcgRsNew the r.r just
// reduced, kMcgPq, kMcgAlpha, kMcgBeta as there), then the r.z just reduced, rr0 and the rank's own sums
constexpr int kMpcgRz = kMcgRs, kMpcgRrNew = kMcgRsNew, kMpcgRzNew = 5, kMpcgRr0 = 6, kMpcgLocal = 7, kMpcgSlots = 8;
// the int words beyond cg_multi's act[], done[] (the steps taken) and active count: status[kMcgMaxK]
constexpr int kMpcgStatus = kMcgFlagWords, kMpcgFlagWords = kMcgFlagWords + kMcgMaxK;
constexpr int kMpcgNone = 0, kMpcgJacobi = 1, kMpcgApply = 2;

// the lane's V sums of r.r and of r.z -> the workgroup's partials in the two planes.  mcg_block_partials stages in one
// __shared__ array: the barrier keeps the second use from overwriting what the first is still reading.
template <int V>
__device__ __forceinline__ void mpcg_block_partials2(double (&rr)[V], double (&rz)[V], int k, int cl, int j0,
                                                     double *__restrict__ part_rr, double *__restrict__ part_rz) {
    mcg_block_partials<V>(rr, k, cl, j0, part_rr);
    __syncthreads();
    mcg_block_partials<V>(rz, k, cl, j0, part_rz);
}

template <typename T, int V, bool JAC>
__global__ __launch_bounds__(kBlock) void mpcg_start_dots(long long n, int k, int cl, const T *__restrict__ dinv,
                                                          const T *__restrict__ r, T *__restrict__ z,
                                                          double *__restrict__ part_rr, double *__restrict__ part_rz) {
    const McgLane l(cl, V);
    double rr[V], rz[V];
#pragma unroll
    for (int v = 0; v < V; ++v) rr[v] = rz[v] = 0;
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T rv[V];
            piece_load<T, V>(r + o, rv);
            if constexpr (JAC) {
                const double d = (double)dinv[i];
                T zv[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    zv[v] = (T)(d * (double)rv[v]);
                    rr[v] += (double)rv[v] * (double)rv[v];
                    rz[v] += (double)rv[v] * (double)zv[v];
                }
                piece_store<T, V>(z + o, zv);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) rr[v] += (double)rv[v] * (double)rv[v];
            }
        }
    }
    if constexpr (JAC) mpcg_block_partials2<V>(rr, rz, k, cl, l.j0, part_rr, part_rz);
    else mcg_block_partials<V>(rr, k, cl, l.j0, part_rr);
}

template <typename T, int V, int MODE>
__global__ __launch_bounds__(kBlock) void mpcg_update_x_r(long long n, int k, int cl, const double *__restrict__ s,
                                                          const int *__restrict__ flags, const T *__restrict__ p,
                                                          const T *__restrict__ q, const T *__restrict__ dinv,
                                                          T *__restrict__ x, T *__restrict__ r, T *__restrict__ z,
                                                          double *__restrict__ part_rr, double *__restrict__ part_rz) {
    const McgLane l(cl, V);
    double rr[V], rz[V], alpha[V];
    bool live[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        rr[v] = rz[v] = 0;
        live[v] = l.j0 + v < k && flags[kMcgAct + l.j0 + v] != 0;
        alpha[v] = l.j0 + v < k ? s[kMcgAlpha * kMcgMaxK + l.j0 + v] : 0.0;
    }
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T pv[V], qv[V], xv[V], rv[V];
            piece_load<T, V>(p + o, pv);
            piece_load<T, V>(q + o, qv);
            piece_load<T, V>(x + o, xv);
            piece_load<T, V>(r + o, rv);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const T xn = (T)((double)xv[v] + alpha[v] * (double)pv[v]);
                const T rn = (T)((double)rv[v] - alpha[v] * (double)qv[v]);
                xv[v] = live[v] ? xn : xv[v];
                rv[v] = live[v] ? rn : rv[v];
            }
            piece_store<T, V>(x + o, xv);
            piece_store<T, V>(r + o, rv);
            if constexpr (MODE == kMpcgNone) {
#pragma unroll
                for (int v = 0; v < V; ++v) rr[v] += (double)rv[v] * (double)rv[v];
            } else if constexpr (MODE == kMpcgJacobi) {
                // a stopped column's r has not changed: its z is rewritten with the bits it holds
                const double d = (double)dinv[i];
                T zv[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    zv[v] = (T)(d * (double)rv[v]);
                    rr[v] += (double)rv[v] * (double)rv[v];
                    rz[v] += (double)rv[v] * (double)zv[v];
                }
                piece_store<T, V>(z + o, zv);
            }
        }
    }
    if constexpr (MODE == kMpcgNone) mcg_block_partials<V>(rr, k, cl, l.j0, part_rr);
    else if constexpr (MODE == kMpcgJacobi) mpcg_block_partials2<V>(rr, rz, k, cl, l.j0, part_rr, part_rz);
}

// z = M^-1 r for P's n local rows of k columns; inv in its stored layout (block kb at inv[kb b^2], column-major inside
// the block; b = 1: inv[i] = 1 / d_i).  flags (NULL: none): a lane whose columns have all stopped leaves z alone, a
// stopped column beside a live one keeps the z it holds.
template <typename T, int V, bool DOTS>
__global__ __launch_bounds__(kBlock) void mpc_apply(long long n, int k, int cl, int b, const T *__restrict__ inv,
                                                    const T *__restrict__ r, T *__restrict__ z,
                                                    const int *__restrict__ flags, double *__restrict__ part_rr,
                                                    double *__restrict__ part_rz) {
    const McgLane l(cl, V);
    double rr[V], rz[V];
    bool live[V];
    bool any = false, all = true;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        rr[v] = rz[v] = 0;
        const bool in = l.j0 + v < k;
        live[v] = in && (!flags || flags[kMcgAct + l.j0 + v] != 0);
        any = any || live[v];
        all = all && (live[v] || !in);
    }
    if (l.j0 < k && any) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long kb = i / b;
            const int ii = (int)(i - kb * b);
            const int bk = (int)std::min<long long>(b, n - kb * b);
            const T *ik = inv + kb * b * b + ii;
            const T *rk = r + kb * b * k + l.j0;
            T rv[V], zv[V];
            double acc[V];
            piece_load<T, V>(rk, rv);
            {
                const double a = (double)ik[0];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] = a * (double)rv[v];
            }
            for (int c = 1; c < bk; ++c) {
                const double a = (double)ik[(long long)c * b];
                piece_load<T, V>(rk + (long long)c * k, rv);
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += a * (double)rv[v];
            }
            const long long o = i * k + l.j0;
            if (all) {
#pragma unroll
                for (int v = 0; v < V; ++v) zv[v] = (T)acc[v];
            } else {
                piece_load<T, V>(z + o, zv);
#pragma unroll
                for (int v = 0; v < V; ++v) zv[v] = live[v] ? (T)acc[v] : zv[v];
            }
            piece_store<T, V>(z + o, zv);
            if constexpr (DOTS) {
                piece_load<T, V>(r + o, rv);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double ri = (double)rv[v];
                    rr[v] += ri * ri;
                    rz[v] += ri * (double)zv[v];
                }
            }
        }
    }
    if constexpr (DOTS) mpcg_block_partials2<V>(rr, rz, k, cl, l.j0, part_rr, part_rz);
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mpcg_dots(long long n, int k, int cl, const T *__restrict__ r,
                                                    const T *__restrict__ z, double *__restrict__ part_rr,
                                                    double *__restrict__ part_rz) {
    const McgLane l(cl, V);
    double rr[V], rz[V];
#pragma unroll
    for (int v = 0; v < V; ++v) rr[v] = rz[v] = 0;
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            const long long o = i * k + l.j0;
            T rv[V], zv[V];
            piece_load<T, V>(r + o, rv);
            piece_load<T, V>(z + o, zv);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double ri = (double)rv[v];
                rr[v] += ri * ri;
                rz[v] += ri * (double)zv[v];
            }
        }
    }
    mpcg_block_partials2<V>(rr, rz, k, cl, l.j0, part_rr, part_rz);
}

// ---- the scalar kernels: one wavefront, lane j = column j.  A stop writes the status and the steps taken and never
// touches x.  z_is_r (no preconditioner): r.z is r.r, only r.r was reduced.
__device__ __forceinline__ void mpcg_stop(int *__restrict__ flags, int j, int status, int steps) {
    flags[kMcgAct + j] = 0;
    flags[kMpcgStatus + j] = status;
    flags[kMcgDone + j] = steps;
}

// rr0 = r.r, rz = r.z, history row 0; rr0 = 0 converges at step 0; rz <= 0 or anything not finite breaks down there
__global__ __launch_bounds__(64) void mpcg_start(double *__restrict__ s, int *__restrict__ flags, double *__restrict__ hrr,
                                                 double *__restrict__ hrz, int k, int iters, int z_is_r) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const double rr0 = s[kMpcgRrNew * kMcgMaxK + j], rz = z_is_r ? rr0 : s[kMpcgRzNew * kMcgMaxK + j];
        s[kMpcgRr0 * kMcgMaxK + j] = rr0;
        s[kMpcgRz * kMcgMaxK + j] = rz;
        hrr[j] = rr0;
        hrz[j] = rz;
        live = true;
        flags[kMcgAct + j] = 1;
        flags[kMcgDone + j] = iters;
        flags[kMpcgStatus + j] = SPMV_PCG_RAN_ALL;
        if (rr0 == 0.0) mpcg_stop(flags, j, SPMV_PCG_CONVERGED, 0), live = false;
        else if (!(rz > 0.0) || !isfinite(rz) || !isfinite(rr0)) mpcg_stop(flags, j, SPMV_PCG_BREAKDOWN, 0), live = false;
    }
    mcg_count_active(flags, live);
}

// step t: alpha = rz / p.q; p.q <= 0 or anything not finite breaks down (step t not taken)
__global__ __launch_bounds__(64) void mpcg_set_alpha(double *__restrict__ s, int *__restrict__ flags, int k, int t) {
    const int j = threadIdx.x;
    if (j >= k || flags[kMcgAct + j] == 0) return;
    const double pq = s[kMcgPq * kMcgMaxK + j], alpha = s[kMpcgRz * kMcgMaxK + j] / pq;
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {
        mpcg_stop(flags, j, SPMV_PCG_BREAKDOWN, t - 1);
        return;
    }
    s[kMcgAlpha * kMcgMaxK + j] = alpha;
}

// end of step t: history row t (hrr, hrz point at it; a stopped column repeats row t - 1); a non-finite rr or rz'
// breaks down, rr <= tol2 rr0 converges, rz' <= 0 breaks down (x is the iterate of step t); else beta = rz' / rz,
// rz = rz'
__global__ __launch_bounds__(64) void mpcg_set_beta(double *__restrict__ s, int *__restrict__ flags,
                                                    double *__restrict__ hrr, double *__restrict__ hrz, int k, int t,
                                                    double tol2, int z_is_r) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        live = flags[kMcgAct + j] != 0;
        if (!live) {
            hrr[j] = hrr[j - k];
            hrz[j] = hrz[j - k];
        } else {
            const double rr = s[kMpcgRrNew * kMcgMaxK + j], rz = z_is_r ? rr : s[kMpcgRzNew * kMcgMaxK + j];
            hrr[j] = rr;
            hrz[j] = rz;
            if (!isfinite(rr) || !isfinite(rz)) {
                mpcg_stop(flags, j, SPMV_PCG_BREAKDOWN, t), live = false;
            } else if (rr <= tol2 * s[kMpcgRr0 * kMcgMaxK + j]) {
                mpcg_stop(flags, j, SPMV_PCG_CONVERGED, t), live = false;
            } else if (!(rz > 0.0)) {
                mpcg_stop(flags, j, SPMV_PCG_BREAKDOWN, t), live = false;
            } else {
                s[kMcgBeta * kMcgMaxK + j] = rz / s[kMpcgRz * kMcgMaxK + j];
                s[kMpcgRz * kMcgMaxK + j] = rz;
            }
        }
    }
    mcg_count_active(flags, live);
}

}  // namespace spmv
