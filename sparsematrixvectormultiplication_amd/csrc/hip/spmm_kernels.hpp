// spmm_kernels.hpp -- Y = A X for k vectors per pass over a CSR matrix (gfx950).
//
// X is N x k and Y is M x k, both row-major.  The kernels run on the blocks and long-row pieces every CSR handle
// already holds (desc / pieces / long_rows, csr_build_blocks in spmv_csr.hip), so the matrix leaves HBM once per
// launch whatever k is:
//
//   csr_spmm_block    one workgroup per desc block: the block's (col, val) are staged into LDS with full-width
//                     loads, then lane groups take rows.  A group is CL column lanes x S entry lanes: column lane c
//                     owns columns [4c, 4c + 4) of the current column tile (4 CL wide), entry lane s adds the row's
//                     entries s, s + S, ... in entry order, and the S partial sums are added by a fixed xor tree.
//                     S is the widest power of two that still fits every row of the block into one pass, so blocks
//                     of a few long rows keep all lanes busy.  Column tiles past the first re-read the staged
//                     entries from LDS, not from HBM.
//   csr_spmm_pieces   rows longer than a block's stage: one workgroup per piece writes the piece's k-wide partial
//   csr_spmm_finish   sums to a scratch; a second kernel adds each row's pieces in piece order (the scheme of
//                     csr_long_pieces / csr_long_finish, k wide).
//
// Every result is a fixed sequence of adds that depends on the matrix and k only: no atomics, bit-reproducible.
// VEC: X / Y rows are loaded and stored as 16-byte pieces (k * sizeof(T) a multiple of 16 and 16-byte aligned
// X / Y); otherwise element by element.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"

namespace spmv {

constexpr int kSpmmBlock = 256;  // threads per workgroup
constexpr int kSpmmCols = 4;     // columns of X one lane owns in a column tile

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

// the 4 columns [j0, j0 + 4) of X row c (columns >= k read as 0)
template <typename T, bool VEC>
__device__ __forceinline__ void spmm_load_x(const T *__restrict__ X, long long c, int k, int j0, T (&xv)[kSpmmCols]) {
    const T *p = X + c * k + j0;
    if constexpr (VEC && sizeof(T) == 8) {
        v2d a = {0, 0}, b = {0, 0};
        if (j0 < k) a = *reinterpret_cast<const v2d *>(p);  // k is even: a pair is all inside or all outside
        if (j0 + 2 < k) b = *reinterpret_cast<const v2d *>(p + 2);
        xv[0] = a.x, xv[1] = a.y, xv[2] = b.x, xv[3] = b.y;
    } else if constexpr (VEC) {
        v4f a = {0, 0, 0, 0};
        if (j0 < k) a = *reinterpret_cast<const v4f *>(p);  // k is a multiple of 4
        xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w;
    } else {
#pragma unroll
        for (int q = 0; q < kSpmmCols; ++q) xv[q] = j0 + q < k ? p[q] : T(0);
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void spmm_store_y(T *__restrict__ Y, long long row, int k, int j0, const T (&acc)[kSpmmCols]) {
    T *p = Y + row * k + j0;
    if constexpr (VEC && sizeof(T) == 8) {
        if (j0 < k) *reinterpret_cast<v2d *>(p) = v2d{acc[0], acc[1]};
        if (j0 + 2 < k) *reinterpret_cast<v2d *>(p + 2) = v2d{acc[2], acc[3]};
    } else if constexpr (VEC) {
        if (j0 < k) *reinterpret_cast<v4f *>(p) = v4f{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
        for (int q = 0; q < kSpmmCols; ++q)
            if (j0 + q < k) p[q] = acc[q];
    }
}

// acc += v * X[c, j0 .. j0 + 4) for the entries lo, lo + step, ... below hi, in that order; four entries' X rows are
// loaded before the first of them is added
template <typename T, bool VEC>
__device__ __forceinline__ void spmm_walk(const int *s_col, const T *s_val, int lo, int hi, int step,
                                          const T *__restrict__ X, int k, int j0, T (&acc)[kSpmmCols]) {
    int e = lo;
    for (; e + 3 * step < hi; e += 4 * step) {
        T xv[4][kSpmmCols];
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = s_val[e + u * step];
            spmm_load_x<T, VEC>(X, s_col[e + u * step], k, j0, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) acc[q] += v[u] * xv[u][q];
    }
    for (; e < hi; e += step) {
        T xv[kSpmmCols];
        const T v = s_val[e];
        spmm_load_x<T, VEC>(X, s_col[e], k, j0, xv);
#pragma unroll
        for (int q = 0; q < kSpmmCols; ++q) acc[q] += v * xv[q];
    }
}

// the same over global col / val (long-row pieces, not staged)
template <typename T, bool VEC>
__device__ __forceinline__ void spmm_walk_global(const int *__restrict__ col, const T *__restrict__ val, int lo, int hi,
                                                 int step, const T *__restrict__ X, int k, int j0, T (&acc)[kSpmmCols]) {
    int e = lo;
    for (; e + 3 * step < hi; e += 4 * step) {
        T xv[4][kSpmmCols];
        T v[4];
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = col[e + u * step];
            v[u] = val[e + u * step];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) spmm_load_x<T, VEC>(X, c[u], k, j0, xv[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) acc[q] += v[u] * xv[u][q];
    }
    for (; e < hi; e += step) {
        T xv[kSpmmCols];
        spmm_load_x<T, VEC>(X, col[e], k, j0, xv);
        const T v = val[e];
#pragma unroll
        for (int q = 0; q < kSpmmCols; ++q) acc[q] += v * xv[q];
    }
}

// add the partial sums of the lanes lane ^ CL, lane ^ 2 CL, ... below `lanes` (a fixed tree: every lane of the
// group ends with the same bits)
template <typename T, int CL>
__device__ __forceinline__ void spmm_reduce(T (&acc)[kSpmmCols], int lanes) {
    for (int off = CL; off < lanes; off <<= 1)  // lanes is wave-uniform
#pragma unroll
        for (int q = 0; q < kSpmmCols; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
}

// One workgroup per desc block {first row, first entry, rows, end entry}.  Dynamic LDS: cap values, then cap columns
// (cap = the handle's stream_cap rounded up to a multiple of 4).
template <typename T, int CL, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void csr_spmm_block(int num_blocks, int cap, const int4 *__restrict__ desc,
                                                             const int *__restrict__ row_ptr,
                                                             const int *__restrict__ col, const T *__restrict__ val,
                                                             const T *__restrict__ X, T *__restrict__ Y, int k) {
    extern __shared__ __attribute__((aligned(16))) char spmm_lds[];
    T *s_val = reinterpret_cast<T *>(spmm_lds);
    int *s_col = reinterpret_cast<int *>(spmm_lds + (size_t)cap * sizeof(T));
    const int b = blockIdx.x;
    if (b >= num_blocks) return;
    const int t = threadIdx.x;
    const int4 d = desc[b];
    const int r0 = d.x, nrows = d.z;
    const int base = d.y & kBaseMask;

    // stage [base, end) in 16-byte pieces: col / val carry kPad zeroed entries behind the last one, and a block's
    // entries counted from base fit cap, so the rounded-up tail stays inside both the arrays and the stage
    const int quads = (d.w - base + 3) >> 2;
    for (int i = t; i < quads; i += kSpmmBlock) {
        const v4i c = stream_load<true>(reinterpret_cast<const v4i *>(col + base) + i);
        *reinterpret_cast<v4i *>(s_col + 4 * i) = c;
        if constexpr (sizeof(T) == 8) {
            const v2d a = stream_load<true>(reinterpret_cast<const v2d *>(val + base) + 2 * i);
            const v2d bb = stream_load<true>(reinterpret_cast<const v2d *>(val + base) + 2 * i + 1);
            *reinterpret_cast<v2d *>(s_val + 4 * i) = a;
            *reinterpret_cast<v2d *>(s_val + 4 * i + 2) = bb;
        } else {
            *reinterpret_cast<v4f *>(s_val + 4 * i) = stream_load<true>(reinterpret_cast<const v4f *>(val + base) + i);
        }
    }

    // lanes per row: CL column lanes x S entry lanes, S the widest power of two (<= 64 / CL) with one pass
    int S = kSpmmBlock / (max(nrows, 1) * CL);
    S = S <= 1 ? 1 : 1 << (31 - __clz(S));
    if (S > 64 / CL) S = 64 / CL;
    const int lanes = CL * S, rows_per_pass = kSpmmBlock / lanes;
    const int my_row = t / lanes, cl = t % CL, s = (t % lanes) / CL;
    __syncthreads();

    for (int jt = 0; jt < k; jt += kSpmmCols * CL) {
        const int j0 = jt + kSpmmCols * cl;
        for (int first = 0; first < nrows; first += rows_per_pass) {  // all lanes stay in the loop (the xor tree)
            const int row = first + my_row;
            int lo = 0, hi = 0;
            if (row < nrows) {
                lo = row_ptr[r0 + row] - base;
                hi = row_ptr[r0 + row + 1] - base;
            }
            T acc[kSpmmCols] = {};
            if (j0 < k) spmm_walk<T, VEC>(s_col, s_val, lo + s, hi, S, X, k, j0, acc);
            spmm_reduce<T, CL>(acc, lanes);
            if (s == 0 && row < nrows) spmm_store_y<T, VEC>(Y, (long long)r0 + row, k, j0, acc);
        }
    }
}

// piece = {row, first entry, end entry, slot}: one workgroup; partial[slot * k + j] = the piece's sum for column j
template <typename T, int CL, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void csr_spmm_pieces(int count, const int4 *__restrict__ pieces,
                                                              const int *__restrict__ col, const T *__restrict__ val,
                                                              const T *__restrict__ X, T *__restrict__ partial, int k) {
    constexpr int kWaves = kSpmmBlock / 64;
    __shared__ T wave_part[kWaves][CL][kSpmmCols];
    if ((int)blockIdx.x >= count) return;
    const int t = threadIdx.x;
    const int4 d = pieces[blockIdx.x];
    const int cl = t % CL, g = t / CL;
    constexpr int kGroups = kSpmmBlock / CL;
    for (int jt = 0; jt < k; jt += kSpmmCols * CL) {
        const int j0 = jt + kSpmmCols * cl;
        T acc[kSpmmCols] = {};
        if (j0 < k) spmm_walk_global<T, VEC>(col, val, d.y + g, d.z, kGroups, X, k, j0, acc);
        spmm_reduce<T, CL>(acc, 64);
        if ((t & 63) < CL)
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) wave_part[t >> 6][cl][q] = acc[q];
        __syncthreads();
        if (t < CL) {
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) {
                T sum = wave_part[0][t][q];
                for (int w = 1; w < kWaves; ++w) sum += wave_part[w][t][q];
                if (j0 + q < k) partial[(long long)d.w * k + j0 + q] = sum;
            }
        }
        __syncthreads();  // wave_part is reused by the next column tile
    }
}

// long row = {row, first slot, pieces, 0}: Y[row, j] = its pieces' partial sums for column j, in piece order
template <typename T>
__global__ __launch_bounds__(64) void csr_spmm_finish(int count, const int4 *__restrict__ rows,
                                                      const T *__restrict__ partial, T *__restrict__ Y, int k) {
    const int i = blockIdx.x;
    if (i >= count) return;
    const int4 d = rows[i];
    for (int j = threadIdx.x; j < k; j += 64) {
        T acc = 0;
        for (int p = 0; p < d.z; ++p) acc += partial[(long long)(d.y + p) * k + j];
        Y[(long long)d.x * k + j] = acc;
    }
}

}  // namespace spmv
