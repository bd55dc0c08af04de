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
//   bcg_fold         one workgroup folds the workgroups' partials (one or two values) in workgroup order
//   bcg_start / bcg_set_alpha / bcg_check_s / bcg_set_omega / bcg_set_beta   one thread: the scalars, the stop and
//                    breakdown rules and the history
//
// Every vector is indexed by global row; a kernel covers the rows [lo, hi) of this rank.  A lane owns pieces of
// V = 16 / sizeof(T) rows that start at a global row divisible by V, so every whole piece is one 16-byte load or
// store (the buffers are library-owned and hipMalloc-aligned).  The piece that holds lo or hi - 1 may be cut: its
// rows are read and written one by one, the rows outside [lo, hi) are neither read nor written.  Pieces stride over
// the grid: lane g of the launch takes pieces q0 + g, q0 + g + G, ... (G = grid x kBlock).
//
// Reduction order.  Products are accumulated in double for fp32 and fp64 data alike.  A lane adds its pieces in
// stride order and a piece's V rows in row order; group_sum<64> adds the lanes of a wave, the waves of a workgroup
// are added in wave order, bcg_fold adds the workgroups in workgroup order.  The grid depends on hi - lo only.  No
// atomics: every run gives the same bits.
//
// The state word.  RUN: the step proceeds.  HALF: s converged in this step; bcg_update_x_r applies x += alpha p,
// r = s and bcg_set_beta turns the state to STOP.  STOP: the vector kernels return before they write anything and
// the scalar kernels only repeat the last history value, so a stopped solve can go on being launched (tol = 0) with
// x and r untouched.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"
#include "wave_ops.hpp"

namespace spmv {

constexpr int kBcgBlocks = 2048;  // grid cap of the vector kernels

// the scalar slots (doubles).  Two-value reductions land in adjacent slots: (Rho, Rr0), (Ts, Tt), (RhoNew, Rr).
constexpr int kBcgRho = 0, kBcgRr0 = 1, kBcgRv = 2, kBcgAlpha = 3, kBcgSs = 4, kBcgTs = 5, kBcgTt = 6, kBcgOmega = 7,
              kBcgRhoNew = 8, kBcgRr = 9, kBcgBeta = 10, kBcgLast = 11, kBcgLocal = 12, kBcgSlots = 16;
// the int words
constexpr int kBcgState = 0, kBcgSteps = 1, kBcgStatus = 2, kBcgHalf = 3, kBcgFlagWords = 4;
constexpr int kBcgRun = 0, kBcgHalfStep = 1, kBcgStop = 2;

typedef float v4f_bcg __attribute__((ext_vector_type(4)));

// piece [i0, i0 + V) of a; rows outside [lo, hi) read as 0
template <typename T, int V>
__device__ __forceinline__ void bcg_load(const T *__restrict__ a, long long i0, bool whole, long long lo, long long hi,
                                         T (&v)[V]) {
    static_assert(V * sizeof(T) == 16, "one 16-byte piece per lane");
    if (whole) {
        if constexpr (sizeof(T) == 8) {
            const v2d w = *reinterpret_cast<const v2d *>(a + i0);
            v[0] = w.x, v[1] = w.y;
        } else {
            const v4f_bcg w = *reinterpret_cast<const v4f_bcg *>(a + i0);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = i0 + j >= lo && i0 + j < hi ? a[i0 + j] : T(0);
    }
}

// piece [i0, i0 + V) of a; rows outside [lo, hi) are not written
template <typename T, int V>
__device__ __forceinline__ void bcg_store(T *__restrict__ a, long long i0, bool whole, long long lo, long long hi,
                                          const T (&v)[V]) {
    if (whole) {
        if constexpr (sizeof(T) == 8) {
            *reinterpret_cast<v2d *>(a + i0) = v2d{v[0], v[1]};
        } else {
            *reinterpret_cast<v4f_bcg *>(a + i0) = v4f_bcg{v[0], v[1], v[2], v[3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j >= lo && i0 + j < hi) a[i0 + j] = v[j];
    }
}

// the lane's pieces: q = first, first + stride, ... < end; piece q covers rows [q V, q V + V)
struct BcgLane {
    long long q, stride, end;
    __device__ __forceinline__ BcgLane(long long lo, long long hi, int V) {
        const long long q0 = lo / V;
        q = q0 + (long long)blockIdx.x * kBlock + threadIdx.x;
        stride = (long long)gridDim.x * kBlock;
        end = (hi + V - 1) / V;
    }
};

// the lane's NV sums -> the workgroup's partials part[blockIdx.x * NV + j], waves added in order
template <int NV>
__device__ __forceinline__ void bcg_block_partials(double (&acc)[NV], double *__restrict__ part) {
    __shared__ double wave_sum[kBlock / 64][NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = group_sum<64>(acc[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) wave_sum[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int j = threadIdx.x;
        double s = wave_sum[0][j];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w][j];
        part[(long long)blockIdx.x * NV + j] = s;
    }
}

// partials of a.b on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_dot(long long lo, long long hi, const int *__restrict__ flags,
                                                  const T *__restrict__ a, const T *__restrict__ b,
                                                  double *__restrict__ part) {
    if (flags[kBcgState] != kBcgRun) return;
    double acc[1] = {0.0};
    for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        const bool whole = i0 >= lo && i0 + V <= hi;
        T av[V], bv[V];
        bcg_load<T, V>(a, i0, whole, lo, hi, av);
        bcg_load<T, V>(b, i0, whole, lo, hi, bv);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[0] += (double)av[j] * (double)bv[j];
    }
    bcg_block_partials<1>(acc, part);
}

// partials of a.b and a.a on [lo, hi) (r.r^ with r.r at the start; t.s with t.t in a step)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_dot2(long long lo, long long hi, const int *__restrict__ flags,
                                                   const T *__restrict__ a, const T *__restrict__ b,
                                                   double *__restrict__ part) {
    if (flags[kBcgState] != kBcgRun) return;
    double acc[2] = {0.0, 0.0};
    for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        const bool whole = i0 >= lo && i0 + V <= hi;
        T av[V], bv[V];
        bcg_load<T, V>(a, i0, whole, lo, hi, av);
        bcg_load<T, V>(b, i0, whole, lo, hi, bv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double ad = (double)av[j];
            acc[0] += ad * (double)bv[j];
            acc[1] += ad * ad;
        }
    }
    bcg_block_partials<2>(acc, part);
}

// s = r - alpha v on [lo, hi), partials of s.s
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_s(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, const T *__restrict__ r,
                                                       const T *__restrict__ v, T *__restrict__ s,
                                                       double *__restrict__ part) {
    if (flags[kBcgState] != kBcgRun) return;
    const double alpha = sc[kBcgAlpha];
    double acc[1] = {0.0};
    for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        const bool whole = i0 >= lo && i0 + V <= hi;
        T rv[V], vv[V], sv[V];
        bcg_load<T, V>(r, i0, whole, lo, hi, rv);
        bcg_load<T, V>(v, i0, whole, lo, hi, vv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sv[j] = (T)((double)rv[j] - alpha * (double)vv[j]);
            acc[0] += (double)sv[j] * (double)sv[j];
        }
        bcg_store<T, V>(s, i0, whole, lo, hi, sv);
    }
    bcg_block_partials<1>(acc, part);
}

// RUN: x += alpha p + omega s, r = s - omega t on [lo, hi), partials of r^.r and r.r.  HALF: x += alpha p, r = s.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_x_r(long long lo, long long hi, const int *__restrict__ flags,
                                                         const double *__restrict__ sc, const T *__restrict__ rhat,
                                                         const T *__restrict__ p, const T *__restrict__ s,
                                                         const T *__restrict__ t, T *__restrict__ x,
                                                         T *__restrict__ r, double *__restrict__ part) {
    const int state = flags[kBcgState];
    if (state == kBcgStop) return;
    const double alpha = sc[kBcgAlpha];
    double acc[2] = {0.0, 0.0};
    if (state == kBcgHalfStep) {
        for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            const bool whole = i0 >= lo && i0 + V <= hi;
            T xv[V], pv[V], sv[V];
            bcg_load<T, V>(x, i0, whole, lo, hi, xv);
            bcg_load<T, V>(p, i0, whole, lo, hi, pv);
            bcg_load<T, V>(s, i0, whole, lo, hi, sv);
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            bcg_store<T, V>(x, i0, whole, lo, hi, xv);
            bcg_store<T, V>(r, i0, whole, lo, hi, sv);
        }
    } else {
        const double omega = sc[kBcgOmega];
        for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
            const long long i0 = l.q * V;
            const bool whole = i0 >= lo && i0 + V <= hi;
            T xv[V], pv[V], sv[V], tv[V], hv[V];
            bcg_load<T, V>(x, i0, whole, lo, hi, xv);
            bcg_load<T, V>(p, i0, whole, lo, hi, pv);
            bcg_load<T, V>(s, i0, whole, lo, hi, sv);
            bcg_load<T, V>(t, i0, whole, lo, hi, tv);
            bcg_load<T, V>(rhat, i0, whole, lo, hi, hv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                xv[j] = (T)((double)xv[j] + (alpha * (double)pv[j] + omega * (double)sv[j]));
                const T rn = (T)((double)sv[j] - omega * (double)tv[j]);
                sv[j] = rn;  // the new r
                acc[0] += (double)hv[j] * (double)rn;
                acc[1] += (double)rn * (double)rn;
            }
            bcg_store<T, V>(x, i0, whole, lo, hi, xv);
            bcg_store<T, V>(r, i0, whole, lo, hi, sv);
        }
    }
    bcg_block_partials<2>(acc, part);
}

// p = r + beta (p - omega v) on [lo, hi)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcg_update_p(long long lo, long long hi, const int *__restrict__ flags,
                                                       const double *__restrict__ sc, const T *__restrict__ r,
                                                       const T *__restrict__ v, T *__restrict__ p) {
    if (flags[kBcgState] != kBcgRun) return;
    const double beta = sc[kBcgBeta], omega = sc[kBcgOmega];
    for (BcgLane l(lo, hi, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        const bool whole = i0 >= lo && i0 + V <= hi;
        T rv[V], vv[V], pv[V];
        bcg_load<T, V>(r, i0, whole, lo, hi, rv);
        bcg_load<T, V>(v, i0, whole, lo, hi, vv);
        bcg_load<T, V>(p, i0, whole, lo, hi, pv);
#pragma unroll
        for (int j = 0; j < V; ++j) pv[j] = (T)((double)rv[j] + beta * ((double)pv[j] - omega * (double)vv[j]));
        bcg_store<T, V>(p, i0, whole, lo, hi, pv);
    }
}

// one workgroup: part[g * nv + j], g = 0 .. nparts, added in workgroup order -> out[j], j < nv (nv = 1 or 2)
__global__ __launch_bounds__(kBlock) void bcg_fold(const double *__restrict__ part, int nparts, int nv,
                                                   double *__restrict__ out) {
    __shared__ double wave_sum[kBlock / 64][2];
    double acc[2] = {0.0, 0.0};
    for (int g = threadIdx.x; g < nparts; g += kBlock) {
        acc[0] += part[(long long)g * nv];
        if (nv == 2) acc[1] += part[(long long)g * nv + 1];
    }
    acc[0] = group_sum<64>(acc[0]);
    acc[1] = group_sum<64>(acc[1]);
    if ((threadIdx.x & 63) == 0) {
        wave_sum[threadIdx.x >> 6][0] = acc[0];
        wave_sum[threadIdx.x >> 6][1] = acc[1];
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        const int j = threadIdx.x;
        double s = wave_sum[0][j];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w][j];
        out[j] = s;
    }
}

// the ranks' nv sums (gathered[rank * nv + j]) in rank order -> out[j]; one thread
__global__ void bcg_rank_sum(const double *__restrict__ gathered, int ranks, int nv, double *__restrict__ out) {
    for (int j = 0; j < nv; ++j) {
        double t = gathered[j];
        for (int r = 1; r < ranks; ++r) t += gathered[r * nv + j];
        out[j] = t;
    }
}

// ---- the scalar kernels: one thread each.  A stop writes the status and the steps taken and never touches x.
__device__ __forceinline__ void bcg_stop(int *__restrict__ flags, int status, int steps) {
    flags[kBcgState] = kBcgStop;
    flags[kBcgStatus] = status;
    flags[kBcgSteps] = steps;
}

// rho = r^.r, rr0 = r.r (slots kBcgRho, kBcgRr0), history row 0; rr0 = 0 (b = 0) stops at step 0, converged
__global__ void bcg_start(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int iters) {
    const double rr0 = sc[kBcgRr0];
    sc[kBcgLast] = rr0;
    hist[0] = rr0;
    flags[kBcgState] = kBcgRun;
    flags[kBcgSteps] = iters;
    flags[kBcgStatus] = SPMV_BICG_RAN_ALL;
    flags[kBcgHalf] = 0;
    if (rr0 == 0.0) bcg_stop(flags, SPMV_BICG_CONVERGED, 0);
}

// step t: alpha = rho / r^.v; r^.v = 0 or not finite breaks down (step t not taken)
__global__ void bcg_set_alpha(double *__restrict__ sc, int *__restrict__ flags, int t) {
    if (flags[kBcgState] != kBcgRun) return;
    const double rv = sc[kBcgRv];
    if (rv == 0.0 || !isfinite(rv)) {
        bcg_stop(flags, SPMV_BICG_BREAKDOWN_RHO, t - 1);
        return;
    }
    sc[kBcgAlpha] = sc[kBcgRho] / rv;
}

// step t: s.s <= tol2 rr0 converges at the half step (x += alpha p, r = s are still to be applied: state HALF)
__global__ void bcg_check_s(double *__restrict__ sc, int *__restrict__ flags, int t, double tol2) {
    if (flags[kBcgState] != kBcgRun) return;
    const double ss = sc[kBcgSs];
    if (ss <= tol2 * sc[kBcgRr0]) {
        flags[kBcgState] = kBcgHalfStep;
        flags[kBcgStatus] = SPMV_BICG_CONVERGED;
        flags[kBcgSteps] = t;
        flags[kBcgHalf] = 1;
        sc[kBcgLast] = ss;
    }
}

// step t: omega = t.s / t.t; t.t = 0, t.s = 0 or anything not finite breaks down (step t not taken)
__global__ void bcg_set_omega(double *__restrict__ sc, int *__restrict__ flags, int t) {
    if (flags[kBcgState] != kBcgRun) return;
    const double ts = sc[kBcgTs], tt = sc[kBcgTt], omega = ts / tt;
    if (tt == 0.0 || ts == 0.0 || !isfinite(ts) || !isfinite(tt) || !isfinite(omega)) {
        bcg_stop(flags, SPMV_BICG_BREAKDOWN_OMEGA, t - 1);
        return;
    }
    sc[kBcgOmega] = omega;
}

// end of step t: history row t; r.r <= tol2 rr0 converges; r^.r = 0 or not finite breaks down after the step (x is
// the iterate of step t); else beta = (rho' / rho) (alpha / omega), rho = rho'
__global__ void bcg_set_beta(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int t,
                             double tol2) {
    const int state = flags[kBcgState];
    if (state != kBcgRun) {
        if (state == kBcgHalfStep) flags[kBcgState] = kBcgStop;
        hist[t] = sc[kBcgLast];
        return;
    }
    const double rr = sc[kBcgRr], rho_new = sc[kBcgRhoNew];
    sc[kBcgLast] = rr;
    hist[t] = rr;
    if (rr <= tol2 * sc[kBcgRr0]) {
        bcg_stop(flags, SPMV_BICG_CONVERGED, t);
        return;
    }
    if (rho_new == 0.0 || !isfinite(rho_new)) {
        bcg_stop(flags, SPMV_BICG_BREAKDOWN_RHO, t);
        return;
    }
    sc[kBcgBeta] = (rho_new / sc[kBcgRho]) * (sc[kBcgAlpha] / sc[kBcgOmega]);
    sc[kBcgRho] = rho_new;
}

}  // namespace spmv
