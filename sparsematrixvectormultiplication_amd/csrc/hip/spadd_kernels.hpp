// spadd_kernels.hpp -- the kernels of C = alpha A + beta B on CSR handles (spmv_spadd.hip; the definition:
// include/spmv_hip.h).
//
//   sa_check              is every row of an operand strictly ascending?  8 lanes per row over row_ptr and col; the first
//                         offending row by atomicMin (an index, never a value)
//   sa_long_rows          the rows whose combined length len A_i + len B_i reaches long_from, as a list (its order is
//                         whatever the atomic counter gave: a work list, no value depends on it)
//   sa_merge_rows<T, NUM> the merge tier: `lanes` lanes per row, kBlock / lanes rows per workgroup, the grid sized to the
//                         rows.  NUM = false (symbolic): every A entry looks its column up in B's row by binary search,
//                         count_i = len A_i + len B_i - matches_i.  NUM = true: every entry computes its own final place,
//                             A's entry ia:  rpC[i] + ia + lower_bound(B_i, col) - (matched entries of A_i before ia)
//                             B's entry ib:  rpC[i] + ib + lower_bound(A_i, col) - (matched entries of B_i before ib), unless
//                                            A has the column (A's entry wrote the sum)
//                         and stores column and value there.  The matched entries before an entry are a prefix count of
//                         the match flags in entry order: within a trip the popcount of the group's bits of one ballot,
//                         across trips a running count.  No sort, no LDS, no atomics.
//   sa_merge_long<T, NUM> the same for the listed long rows, a workgroup each: the prefix count is a workgroup rank
//                         (ballot per wave, four wave counts in LDS: 16 bytes, all the LDS of this file)
//   sa_identity           row_ptr / col (one array: 0 .. N) and the ones of I_N, for canon(A) = A I through the product
//
// Every product and sum is one rounded double operation (sa_mul, sa_add: never contracted into a fused multiply-add);
// the value is rounded once to T.  A row's lanes load consecutive entries of col and val.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"

namespace spmv {

// A row of kSaLongRow combined entries or more gets a workgroup (auto).  A lane group walks its row in trips of `lanes`
// entries, one binary search each; the other rows of its wave wait for the longest.  At 64 lanes a row of 2048 entries is
// 32 trips, which the searches of the wave's other rows (a few trips each) no longer hide, and it is 8 tiles of a
// workgroup's 256 lanes: enough for the two barriers per tile of the workgroup rank to be the smaller cost.  With fewer
// lanes the launcher lowers the limit to kSaTrips trips of the group, but not below one workgroup tile (kBlock).
constexpr int kSaLongRow = 2048;
constexpr int kSaTrips = 32;
constexpr int kSaCheckLanes = 8;
constexpr int kSaLongGrid = 4096;  // workgroups of sa_merge_long at most (they stride over the list)

// one rounded IEEE operation each (hipcc contracts a * b + c by default: switched off where the operations are written)
__device__ __forceinline__ double sa_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double sa_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// the first k in [0, n) with col[k] >= c (n if none): col ascending
__device__ __forceinline__ int sa_lower_bound(const int *__restrict__ col, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void sa_check(int M, const int *__restrict__ rp, const int *__restrict__ col,
                                                   int *__restrict__ first_bad) {
    constexpr int kRows = kBlock / kSaCheckLanes;
    const int sub = threadIdx.x % kSaCheckLanes;
    const long long r = (long long)blockIdx.x * kRows + threadIdx.x / kSaCheckLanes;
    if (r >= M) return;
    const int e1 = rp[r + 1];
    bool bad = false;
    for (long long e = (long long)rp[r] + 1 + sub; e < e1; e += kSaCheckLanes) bad |= col[e - 1] >= col[e];
    // One atomic at most per wave, by its first offending lane (the lowest row), and none where a lower row is known
    // already: the read goes to L2 (a cached copy could stay at its first value for the whole launch) and may still be
    // stale, never too small, so it only spares the atomic.
    const unsigned long long any = __ballot(bad);
    if (bad && (int)(threadIdx.x & 63) == __ffsll((long long)any) - 1 &&
        r < __hip_atomic_load(first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(first_bad, (int)r);
}

__global__ __launch_bounds__(kBlock) void sa_long_rows(int M, const int *__restrict__ rpA, const int *__restrict__ rpB,
                                                       int long_from, int *__restrict__ n_long, int *__restrict__ rows) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= M) return;
    if ((rpA[r + 1] - rpA[r]) + (rpB[r + 1] - rpB[r]) >= long_from) rows[atomicAdd(n_long, 1)] = (int)r;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void sa_identity(int N, int *__restrict__ iota, T *__restrict__ ones) {
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (k <= N) iota[k] = (int)k;
    if (k < N) ones[k] = (T)1;
}

// One side of a row's merge: the entries [x0, x0 + lx) of X against the row [y0, y0 + ly) of Y.  rank(matched) returns
// the matched entries of this side before the caller's, and adds the trip's to the running count it keeps; step = the
// lanes that walk the row together, sub = this lane among them.  OWN: X's entries write the sum where they match (A's
// side); otherwise matched entries write nothing (B's side).  Returns nothing: the running count is the rank's.
template <typename T, bool NUM, bool OWN, typename Rank>
__device__ __forceinline__ void sa_side(int step, int sub, int x0, int lx, const int *__restrict__ colX,
                                        const T *__restrict__ valX, double sx, int y0, int ly, const int *__restrict__ colY,
                                        const T *__restrict__ valY, double sy, long long out, int *__restrict__ colC,
                                        T *__restrict__ valC, Rank rank) {
    for (int base = 0; base < lx; base += step) {  // (every lane of the row takes every trip)
        const int i = base + sub;
        const bool live = i < lx;
        int c = 0, p = 0;
        bool matched = false;
        if (live) {
            c = colX[x0 + i];
            p = sa_lower_bound(colY + y0, ly, c);
            matched = p < ly && colY[y0 + p] == c;
        }
        const int before = rank(matched);
        if constexpr (NUM) {
            if (live && (OWN || !matched)) {
                double v = sa_mul(sx, (double)valX[x0 + i]);
                if (OWN && matched) v = sa_add(v, sa_mul(sy, (double)valY[y0 + p]));
                const long long at = out + i + p - before;
                colC[at] = c;
                valC[at] = (T)v;
            }
        }
    }
}

// ---- the merge tier: lanes = 1 << lanes_log2 lanes per row (a group lies inside one wave)
template <typename T, bool NUM>
__global__ __launch_bounds__(kBlock) void sa_merge_rows(int M, int lanes_log2, int long_from, const int *__restrict__ rpA,
                                                        const int *__restrict__ colA, const T *__restrict__ valA,
                                                        const int *__restrict__ rpB, const int *__restrict__ colB,
                                                        const T *__restrict__ valB, double alpha, double beta,
                                                        int *__restrict__ row_cnt, const int *__restrict__ rpC,
                                                        int *__restrict__ colC, T *__restrict__ valC) {
    const int lanes = 1 << lanes_log2;
    const int sub = threadIdx.x & (lanes - 1);
    const long long r = ((long long)blockIdx.x * kBlock + threadIdx.x) >> lanes_log2;
    if (r >= M) return;
    const int a0 = rpA[r], la = rpA[r + 1] - a0, b0 = rpB[r], lb = rpB[r + 1] - b0;
    if (la + lb >= long_from) return;  // sa_merge_long's
    // the group's bits of a ballot: those of its lanes that are in the same trip, which is all of them
    const int shift = (threadIdx.x & 63) & ~(lanes - 1);
    const unsigned long long below = (1ull << sub) - 1;
    int matches = 0;
    auto rank = [&](bool matched) {
        const unsigned long long bits = __ballot(matched) >> shift;
        const int before = matches + __popcll(bits & below);
        matches += __popcll(lanes == 64 ? bits : bits & ((1ull << lanes) - 1));
        return before;
    };
    const long long out = NUM ? (long long)rpC[r] : 0;
    sa_side<T, NUM, true>(lanes, sub, a0, la, colA, valA, alpha, b0, lb, colB, valB, beta, out, colC, valC, rank);
    if constexpr (NUM) {
        matches = 0;
        sa_side<T, true, false>(lanes, sub, b0, lb, colB, valB, beta, a0, la, colA, valA, alpha, out, colC, valC, rank);
    } else {
        if (sub == 0) row_cnt[r] = la + lb - matches;
    }
}

// ---- the long rows, a workgroup each
template <typename T, bool NUM>
__global__ __launch_bounds__(kBlock) void sa_merge_long(const int *__restrict__ n_long, const int *__restrict__ rows,
                                                        const int *__restrict__ rpA, const int *__restrict__ colA,
                                                        const T *__restrict__ valA, const int *__restrict__ rpB,
                                                        const int *__restrict__ colB, const T *__restrict__ valB,
                                                        double alpha, double beta, int *__restrict__ row_cnt,
                                                        const int *__restrict__ rpC, int *__restrict__ colC,
                                                        T *__restrict__ valC) {
    __shared__ int wave_cnt[kBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = *n_long;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int r = rows[k];
        const int a0 = rpA[r], la = rpA[r + 1] - a0, b0 = rpB[r], lb = rpB[r + 1] - b0;
        int matches = 0;
        auto rank = [&](bool matched) {  // (all threads of the workgroup call it: two barriers)
            const unsigned long long mask = __ballot(matched);
            if (lane == 0) wave_cnt[w] = __popcll(mask);
            __syncthreads();
            int before = matches + __popcll(mask & ((1ull << lane) - 1));
            for (int q = 0; q < kBlock / 64; ++q) {
                const int c = wave_cnt[q];
                if (q < w) before += c;
                matches += c;
            }
            __syncthreads();  // wave_cnt is rewritten by the next trip
            return before;
        };
        const long long out = NUM ? (long long)rpC[r] : 0;
        sa_side<T, NUM, true>(kBlock, threadIdx.x, a0, la, colA, valA, alpha, b0, lb, colB, valB, beta, out, colC, valC, rank);
        if constexpr (NUM) {
            matches = 0;
            sa_side<T, true, false>(kBlock, threadIdx.x, b0, lb, colB, valB, beta, a0, la, colA, valA, alpha, out, colC, valC,
                                    rank);
        } else {
            if (threadIdx.x == 0) row_cnt[r] = la + lb - matches;
        }
    }
}

}  // namespace spmv
