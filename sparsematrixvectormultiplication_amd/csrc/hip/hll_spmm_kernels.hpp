// hll_spmm_kernels.hpp -- Y = A X for k vectors per pass over an HLL slab (fp64, gfx950).
//
// X is N x k and Y is M x k, both row-major.  The kernels run on the workgroup windows every HLL handle already holds
// (hdesc, hll_build_blocks in spmv_hll.hip), so each slot of the slab leaves HBM once per launch whatever k is:
//
//   hll_spmm_block   one workgroup per window: the window's slots [base, base + span) are staged into LDS with
//                    non-temporal pair loads (8-byte JA pairs, 16-byte AS pairs, from the even base), then lane groups
//                    take rows.  Every row of a hack is maxnz[h] slots long, padding included (value 0, column = the
//                    row's last real column), so the groups are balanced by construction.  The groups follow
//                    csr_spmm_block (spmm_kernels.hpp): CL column lanes x S entry lanes, column lane c owns columns
//                    [4c, 4c + 4) of the current column tile, entry lane s adds the row's slots s, s + S, ... in slot
//                    order, a fixed xor tree adds the S partial sums.  Column tiles past the first re-read the staged
//                    slots from LDS.  LDS = stage_slots x 12 bytes, at most 48 KiB at kHllCap = 4096 slots: 3
//                    workgroups (12 waves) per CU out of its 160 KiB, 6 at a stage of 2048 slots.
//   hll_spmm_row     a window of one row longer than the stage (the windows listed in the handle's long_windows):
//                    the whole workgroup walks the row straight from global memory, once per column tile; the waves'
//                    partial sums are added in wave order through LDS, so nothing needs scratch.
//
// Every result is a fixed sequence of adds that depends on the slab and k only: no atomics, bit-reproducible, and the
// 16-byte X / Y path (VEC) adds in the same order as the element path.
#pragma once
#include <hip/hip_runtime.h>

#include "hll_kernels.hpp"
#include "spmm_kernels.hpp"

namespace spmv {

// One workgroup per hdesc window {first row, rows | span << 16, first slot lo, first slot hi} (span: slots from the even
// base to the window's end, 0 above 65535).  Dynamic LDS: stage_slots values, then stage_slots columns.
template <int CL, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void hll_spmm_block(int num_blocks, int stage_slots,
                                                             const int4 *__restrict__ desc,
                                                             const long long *__restrict__ hack_off,
                                                             const int *__restrict__ maxnz, const int *__restrict__ JA,
                                                             const double *__restrict__ AS,
                                                             const double *__restrict__ X, double *__restrict__ Y,
                                                             int k) {
    extern __shared__ __attribute__((aligned(16))) char hll_spmm_lds[];
    double *s_val = reinterpret_cast<double *>(hll_spmm_lds);
    int *s_col = reinterpret_cast<int *>(hll_spmm_lds + (size_t)stage_slots * sizeof(double));
    const int b = blockIdx.x;
    if (b >= num_blocks) return;
    const int t = threadIdx.x;
    const int4 d = desc[b];
    const int r0 = d.x, nrows = d.y & 0xffff;
    int span = (int)((unsigned)d.y >> 16);
    const long long first_slot = ((long long)d.w << 32) | (unsigned)d.z;
    const long long base = first_slot & ~1LL;
    if (nrows == 1) {
        // a one-row window: its extent from the hack tables (the descriptor holds 0 above 65535 slots); a row longer
        // than the stage is hll_spmm_row's
        const int h = r0 / kHack;
        const long long end = hack_off[h] + (long long)(r0 % kHack + 1) * maxnz[h] - base;
        if (end > stage_slots) return;
        span = (int)end;
    }

    // stage [base, base + span) as pairs, four pairs per lane in flight: the loads are unconditional (JA / AS carry
    // kPad zero slots behind the slab, more than the 3 x 512 pairs a trip can overshoot), only the LDS stores are
    // bounded; the stage holds the rounded-up pair because stage_slots is a multiple of kStreamUnit
    const int pairs = (span + 1) >> 1;
    for (int i0 = t; i0 < pairs; i0 += 4 * kSpmmBlock) {
        v2i c[4];
        v2d v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = stream_load<true>(reinterpret_cast<const v2i *>(JA + base) + i0 + u * kSpmmBlock);
            v[u] = stream_load<true>(reinterpret_cast<const v2d *>(AS + base) + i0 + u * kSpmmBlock);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kSpmmBlock;
            if (i < pairs) {
                *reinterpret_cast<v2i *>(s_col + 2 * i) = c[u];
                *reinterpret_cast<v2d *>(s_val + 2 * i) = v[u];
            }
        }
    }

    // lanes per row: CL column lanes x S entry lanes, S the widest power of two (<= 64 / CL) with one pass
    int S = kSpmmBlock / (nrows * CL);
    S = S <= 1 ? 1 : 1 << (31 - __clz(S));
    if (S > 64 / CL) S = 64 / CL;
    const int lanes = CL * S, rows_per_pass = kSpmmBlock / lanes;
    const int my_row = t / lanes, cl = t % CL, s = (t % lanes) / CL;
    __syncthreads();

    for (int jt = 0; jt < k; jt += kSpmmCols * CL) {
        const int j0 = jt + kSpmmCols * cl;
        for (int first = 0; first < nrows; first += rows_per_pass) {  // all lanes stay in the loop (the xor tree)
            const int q = first + my_row;
            int lo = 0, hi = 0;
            if (q < nrows) {
                const int r = r0 + q, h = r / kHack;
                const int m = maxnz[h];
                lo = (int)(hack_off[h] + (long long)(r % kHack) * m - base);
                hi = lo + m;
            }
            double acc[kSpmmCols] = {};
            if (j0 < k) spmm_walk<double, VEC>(s_col, s_val, lo + s, hi, S, X, k, j0, acc);
            spmm_reduce<double, CL>(acc, lanes);
            if (s == 0 && q < nrows) spmm_store_y<double, VEC>(Y, (long long)r0 + q, k, j0, acc);
        }
    }
}

// One workgroup per listed window (long_windows[i] indexes desc): its single row, straight from global memory
template <int CL, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void hll_spmm_row(int count, const int *__restrict__ long_windows,
                                                           const int4 *__restrict__ desc,
                                                           const long long *__restrict__ hack_off,
                                                           const int *__restrict__ maxnz, const int *__restrict__ JA,
                                                           const double *__restrict__ AS,
                                                           const double *__restrict__ X, double *__restrict__ Y,
                                                           int k) {
    constexpr int kWaves = kSpmmBlock / 64;
    constexpr int kGroups = kSpmmBlock / CL;
    __shared__ double wave_part[kWaves][CL][kSpmmCols];
    if ((int)blockIdx.x >= count) return;
    const int t = threadIdx.x;
    const int r = desc[long_windows[blockIdx.x]].x, h = r / kHack;
    const int m = maxnz[h];
    const long long at = hack_off[h] + (long long)(r % kHack) * m;
    const int cl = t % CL, g = t / CL;
    for (int jt = 0; jt < k; jt += kSpmmCols * CL) {
        const int j0 = jt + kSpmmCols * cl;
        double acc[kSpmmCols] = {};
        if (j0 < k) spmm_walk_global<double, VEC>(JA + at, AS + at, g, m, kGroups, X, k, j0, acc);
        spmm_reduce<double, CL>(acc, 64);
        if ((t & 63) < CL)
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) wave_part[t >> 6][cl][q] = acc[q];
        __syncthreads();
        if (t < CL) {
#pragma unroll
            for (int q = 0; q < kSpmmCols; ++q) {
                double sum = wave_part[0][t][q];
                for (int w = 1; w < kWaves; ++w) sum += wave_part[w][t][q];
                if (j0 + q < k) Y[(long long)r * k + j0 + q] = sum;
            }
        }
        __syncthreads();  // wave_part is reused by the next column tile
    }
}

}  // namespace spmv
