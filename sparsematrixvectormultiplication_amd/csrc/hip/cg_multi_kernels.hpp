// cg_multi_kernels.hpp -- the vector kernels of spmv_hip_csr_cg_multi: k independent CG recurrences that share one
// SpMM per step (gfx950).
//
// Every vector is a row-major n x k array (element (i, j) at i * k + j, the layout of the SpMM).  A lane owns V
// consecutive columns of one row: V = 16 / sizeof(T) when a row is a whole number of 16-byte pieces (one wide load
// per array), else V = 1.  The CL = 2^cl column lanes that cover a row sit in the LOW lane bits, so the lanes of a
// wave read one contiguous run of rows; the 64 / CL rows of a wave sit in the high bits.  Lanes whose columns lie
// past k (k / V not a power of two) idle.  A workgroup takes kBlock / CL rows per pass and strides over the grid:
//
//   mcg_dot_partial   the k column dot products a[:, j] . b[:, j]          -> part[g * k + j] of workgroup g
//   mcg_update_x_r    x_j += alpha_j p_j, r_j -= alpha_j q_j, and r_j . r_j -> part[g * k + j]
//   mcg_update_p      p_j = r_j + beta_j p_j
//   mcg_start / mcg_set_alpha / mcg_set_beta   one workgroup: the k columns' scalars, the freeze rule, the history
//                     (in spmv_cg.hip: spmv_pcg_multi.hip builds on this header with scalar kernels of its own)
//
// Reduction order.  Products are accumulated in double, for fp32 and fp64 data alike.  A lane adds its rows in
// grid-stride order, the rows of one column in a wave are added by an xor butterfly over the high lane bits, the
// waves of a workgroup in wave order, the workgroups by solver_fold (one workgroup per column) in workgroup order.  None
// of it depends on j, so permuting the columns of B permutes the results bit for bit; no atomics, so every run gives
// the same bits.  With k = 1 (CL = 1, V = 1) the lanes, the butterfly (group_sum<64>) and the wave sums are those of
// dot_partial / cg_update_x_r in spmv_cg.hip, and the host keeps their grid cap: k = 1 is csr_cg bit for bit.
//
// Frozen columns (act[j] == 0) keep x, r and p: the update kernels write back what they read.
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kMcgMaxK = 64;      // widest k: one scalar lane per column in one wavefront
constexpr int kMcgBlocks = 2048;  // grid cap of the vector kernels for k > 1 (k = 1 keeps csr_cg's cap)

// the scalar slots, kMcgMaxK doubles each
constexpr int kMcgRs = 0, kMcgPq = 1, kMcgRsNew = 2, kMcgAlpha = 3, kMcgBeta = 4, kMcgRs0 = 5, kMcgLocal = 6,
              kMcgSlots = 7;
// the int words: act[kMcgMaxK] (1 = still iterating), done[kMcgMaxK] (steps taken), then the count of active columns
constexpr int kMcgAct = 0, kMcgDone = kMcgMaxK, kMcgActive = 2 * kMcgMaxK, kMcgFlagWords = 2 * kMcgMaxK + 1;

// host: cl with 2^cl column lanes, the next power of two >= k / V
inline int mcg_column_lanes(int k, int V) {
    int cl = 0;
    while ((1 << cl) * V < k) ++cl;
    return cl;
}

// the value of lane ^ STEP (a true xor: the column lanes below STEP must not be mixed)
template <int STEP>
__device__ __forceinline__ double mcg_xor_partner(double v) {
    if constexpr (STEP <= 2) {
        return partner<STEP>(v);  // quad_perm xor
    } else if constexpr (STEP < 32) {
        constexpr int kSwz = 0x1F | (STEP << 10);  // ds_swizzle bit mode: and 0x1f, or 0, xor STEP
        const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), kSwz);
        const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), kSwz);
        return __hiloint2double(hi, lo);
    } else {
        return partner<32>(v);
    }
}

// sum over the lanes of a wave with the same lane % 2^cl (the rows of one column); every lane gets its sum.  cl = 0
// is group_sum<64>, the tree of dot_partial.
__device__ __forceinline__ double mcg_rows_sum(double v, int cl) {
    if (cl == 0) return group_sum<64>(v);
    if (cl <= 1) v += mcg_xor_partner<2>(v);
    if (cl <= 2) v += mcg_xor_partner<4>(v);
    if (cl <= 3) v += mcg_xor_partner<8>(v);
    if (cl <= 4) v += mcg_xor_partner<16>(v);
    if (cl <= 5) v += mcg_xor_partner<32>(v);
    return v;
}

// the lane's first row, its row stride and its first column (j0 >= k: an idle lane)
struct McgLane {
    long long row, stride;
    int j0;
    __device__ __forceinline__ McgLane(int cl, int V) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const long long rows_per_block = kBlock >> cl;
        row = (long long)blockIdx.x * rows_per_block + ((long long)wave << (6 - cl)) + (lane >> cl);
        stride = (long long)gridDim.x * rows_per_block;
        j0 = (lane & ((1 << cl) - 1)) * V;
    }
};

// the lane's V column sums -> the workgroup's partials part[blockIdx.x * k + j], waves added in order
template <int V>
__device__ __forceinline__ void mcg_block_partials(double (&acc)[V], int k, int cl, int j0, double *__restrict__ part) {
    __shared__ double wave_sum[kBlock / 64][kMcgMaxK];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = mcg_rows_sum(acc[v], cl);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((lane >> cl) == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (j0 + v < k) wave_sum[wave][j0 + v] = acc[v];
    }
    __syncthreads();
    if ((int)threadIdx.x < k) {
        const int j = threadIdx.x;
        double s = wave_sum[0][j];
        for (int w = 1; w < kBlock / 64; ++w) s += wave_sum[w][j];
        part[(long long)blockIdx.x * k + j] = s;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mcg_dot_partial(const T *__restrict__ a, const T *__restrict__ b, long long n,
                                                          int k, int cl, double *__restrict__ part) {
    const McgLane l(cl, V);
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0;
    if (l.j0 < k) {
        for (long long i = l.row; i < n; i += l.stride) {
            T av[V], bv[V];
            piece_load<T, V>(a + i * k + l.j0, av);
            piece_load<T, V>(b + i * k + l.j0, bv);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += (double)av[v] * (double)bv[v];
        }
    }
    mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

// x += alpha p, r -= alpha q on this rank's rows (active columns), and the workgroup's partials of the new r.r
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mcg_update_x_r(long long n, int k, int cl, const double *__restrict__ s,
                                                         const int *__restrict__ flags, const T *__restrict__ p,
                                                         const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                         double *__restrict__ part) {
    const McgLane l(cl, V);
    double acc[V], alpha[V];
    bool live[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        acc[v] = 0;
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
                acc[v] += (double)rv[v] * (double)rv[v];
            }
            piece_store<T, V>(x + o, xv);
            piece_store<T, V>(r + o, rv);
        }
    }
    mcg_block_partials<V>(acc, k, cl, l.j0, part);
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void mcg_update_p(long long n, int k, int cl, const double *__restrict__ s,
                                                       const int *__restrict__ flags, const T *__restrict__ r,
                                                       T *__restrict__ p) {
    const McgLane l(cl, V);
    if (l.j0 >= k) return;
    double beta[V];
    bool live[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        live[v] = l.j0 + v < k && flags[kMcgAct + l.j0 + v] != 0;
        beta[v] = l.j0 + v < k ? s[kMcgBeta * kMcgMaxK + l.j0 + v] : 0.0;
    }
    for (long long i = l.row; i < n; i += l.stride) {
        const long long o = i * k + l.j0;
        T rv[V], pv[V];
        piece_load<T, V>(r + o, rv);
        piece_load<T, V>(p + o, pv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const T pn = (T)((double)rv[v] + beta[v] * (double)pv[v]);
            pv[v] = live[v] ? pn : pv[v];
        }
        piece_store<T, V>(p + o, pv);
    }
}

// the scalar kernels (one wavefront, lane j = column j) count the columns still iterating
__device__ __forceinline__ void mcg_count_active(int *__restrict__ flags, bool live) {
    const unsigned long long m = __ballot(live);
    if (threadIdx.x == 0) flags[kMcgActive] = __popcll(m);
}

}  // namespace spmv
