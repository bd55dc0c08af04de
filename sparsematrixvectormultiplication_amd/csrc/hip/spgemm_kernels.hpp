// spgemm_kernels.hpp -- the kernels of C = A B on CSR handles (spmv_spgemm.hip; the definition: include/spmv_hip.h).
//
//   sg_count          products[i] = sum over row i's entries of len(B row colA[e]), 64-bit, 8 lanes per row
//   sg_block<T, NUM>  the on-chip tier: one workgroup per row block of at most `cap` products.  expand the products into
//                     LDS in (row, e, f) order -> bitonic sort of the 64-bit keys local_row | column | pos -> heads.
//                     NUM = false (symbolic): keys only, writes each row's count of heads.  NUM = true: the products'
//                     values stay where the expansion wrote them (pos finds them); a head adds its run in pos order
//                     and stores column and value at their final place
//   sg_expand<T, NUM> the global tier: one workgroup per long row of the chunk writes key = row in chunk << col_bits |
//                     column (and the product) into HBM at the row's offset; a stable radix sort follows (host)
//   sg_row_heads      ... then each row's count of heads from the sorted keys
//   sg_row_compress   ... or its columns and values: a head adds its run in sorted order, which the stable sort left in
//                     (e, f) order
//
// Every product is one rounded double multiplication and every sum one rounded double addition (sg_mul, sg_add: never
// contracted into a fused multiply-add), added in the order of the definition; no atomics.  The expansion is
// shared by both tiers: the workgroup takes 256 entries of A at a time, scans their B row lengths, and every thread
// finds the entry of each product it writes by a search in that scan, so a long row of B, or a row of A with 10^6
// products, is spread over all lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"

namespace spmv {

constexpr int kSgMaxRows = 4096;     // rows of a block at most (12 bits of the on-chip key)
constexpr int kSgMaxProducts = 4096; // products of a block at most (12 bits for pos)
constexpr int kSgCountLanes = 8;

__global__ __launch_bounds__(kBlock) void sg_count(int M, const int *__restrict__ rpA, const int *__restrict__ colA,
                                                   const int *__restrict__ rpB, long long *__restrict__ products) {
    constexpr int kRows = kBlock / kSgCountLanes;
    const int sub = threadIdx.x % kSgCountLanes;
    const int g = threadIdx.x / kSgCountLanes;
    const long long stride = (long long)gridDim.x * kRows;
    for (long long r0 = (long long)blockIdx.x * kRows; r0 < M; r0 += stride) {  // (all lanes of a group take every trip)
        const long long r = r0 + g;
        long long sum = 0;
        if (r < M) {
            const int e1 = rpA[r + 1];
            for (int e = rpA[r] + sub; e < e1; e += kSgCountLanes) {
                const int j = colA[e];
                sum += rpB[j + 1] - rpB[j];
            }
        }
        for (int d = kSgCountLanes / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, kSgCountLanes);
        if (r < M && sub == 0) products[r] = sum;
    }
}

// One rounded IEEE operation each.  hipcc contracts a * b + c into a fused multiply-add by default (and its __dmul_rn /
// __dadd_rn are the plain operators), so the contraction is switched off where the operations are written.
__device__ __forceinline__ double sg_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double sg_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// ---- the expansion both tiers share.  Scratch of one workgroup (static LDS):
template <typename I>
struct SgTile {
    I start[kBlock + 1];  // exclusive scan of the tile's B row lengths; start[kBlock] = the tile's products
    int row[kBlock];      // the entry's row (what the caller's row_of returns)
    int f0[kBlock];       // first entry of its B row
    double a[kBlock];     // its value
    I wave_sum[kBlock / 64];
};

// exclusive scan of v over the workgroup into s.start[] (+ the total behind it); ends with a barrier
template <typename I>
__device__ __forceinline__ void sg_scan(SgTile<I> &s, I v) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    I inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const I o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s.wave_sum[w] = inc;
    __syncthreads();
    I base = 0;
    for (int k = 0; k < w; ++k) base += s.wave_sum[k];
    s.start[t] = base + inc - v;
    if (t == kBlock - 1) s.start[kBlock] = base + inc;
    __syncthreads();
}

// The workgroup expands A's entries [e0, e1): emit(p, k, f) is called once for each product, p = its position among
// the products of [e0, e1) in (e, f) order counted from `base`, k = the slot of its A entry in the tile scratch (s.row[k],
// s.a[k]), f = the entry of B.  row_of(e) gives s.row.  Returns base + the products written.  All threads call it.
template <typename T, bool NUM, typename I, typename RowOf, typename Emit>
__device__ __forceinline__ I sg_expand_entries(SgTile<I> &s, int e0, int e1, I base, const int *__restrict__ colA,
                                               const T *__restrict__ valA, const int *__restrict__ rpB, RowOf row_of,
                                               Emit emit) {
    const int t = threadIdx.x;
    for (long long tile = e0; tile < e1; tile += kBlock) {  // (64-bit: e0 + kBlock may pass 2^31)
        const long long e = tile + t;
        I len = 0;
        if (e < e1) {
            const int j = colA[e];
            const int b0 = rpB[j];
            len = (I)(rpB[j + 1] - b0);
            s.f0[t] = b0;
            s.row[t] = row_of((int)e);
            if constexpr (NUM) s.a[t] = (double)valA[e];
        }
        sg_scan(s, len);
        const I total = s.start[kBlock];
        for (I p = t; p < total; p += kBlock) {
            int lo = 0, hi = kBlock - 1;  // the last k with start[k] <= p: entries without products share their successor's start
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s.start[mid] <= p) lo = mid;
                else hi = mid - 1;
            }
            emit(base + p, lo, s.f0[lo] + (int)(p - s.start[lo]));
        }
        base += total;
        __syncthreads();  // the scratch is rewritten by the next tile
    }
    return base;
}

// ranks of the flagged threads of the workgroup: returns this thread's exclusive rank, adds the workgroup's count to total
__device__ __forceinline__ int sg_rank(bool flag, int *wave_cnt, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_cnt[w] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1)), all = 0;
    for (int k = 0; k < kBlock / 64; ++k) {
        const int c = wave_cnt[k];
        if (k < w) before += c;
        all += c;
    }
    __syncthreads();  // wave_cnt is rewritten by the next call
    const int rank = total + before;
    total += all;
    return rank;
}

// ---- the on-chip tier.  desc[b] = {first row, rows, products, 0}: the block's rows in front of its long row, if it
// has one.  Dynamic LDS: keys[cap] (8 bytes each), then NUM ? double vals[cap] : int heads[cap] (heads[p] = heads among
// the sorted positions 0..p).  Key = local row << 44 | column << 12 | pos: total, so the sorted order is unique.
template <typename T, bool NUM>
__global__ __launch_bounds__(kBlock) void sg_block(int num_blocks, int cap, const int4 *__restrict__ desc,
                                                   const int *__restrict__ rpA, const int *__restrict__ colA,
                                                   const T *__restrict__ valA, const int *__restrict__ rpB,
                                                   const int *__restrict__ colB, const T *__restrict__ valB,
                                                   const long long *__restrict__ products, int *__restrict__ row_cnt,
                                                   const int *__restrict__ rpC, int *__restrict__ colC,
                                                   T *__restrict__ valC) {
    extern __shared__ __align__(16) unsigned char sg_lds[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(sg_lds);
    double *vals = reinterpret_cast<double *>(sg_lds + (size_t)cap * 8);
    int *heads = reinterpret_cast<int *>(sg_lds + (size_t)cap * 8);
    __shared__ SgTile<int> s;
    __shared__ int wave_cnt[kBlock / 64];
    const int t = threadIdx.x;
    for (int b = blockIdx.x; b < num_blocks; b += gridDim.x) {
        const int row0 = desc[b].x, nrows = desc[b].y, P = desc[b].z;
        int n2 = 1;
        while (n2 < P) n2 <<= 1;  // <= cap: the plan keeps P <= cap and cap is a power of two
        const int *rp = rpA + row0;
        auto row_of = [&](int e) {  // the last local row with rp[row] <= e (empty rows share their successor's start)
            int lo = 0, hi = nrows - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rp[mid] <= e) lo = mid;
                else hi = mid - 1;
            }
            return lo;
        };
        auto emit = [&](int p, int k, int f) {
            keys[p] = (unsigned long long)s.row[k] << 44 | (unsigned long long)(unsigned)colB[f] << 12 | (unsigned)p;
            if constexpr (NUM) vals[p] = sg_mul(s.a[k], (double)valB[f]);
        };
        sg_expand_entries<T, NUM, int>(s, rp[0], rp[nrows], 0, colA, valA, rpB, row_of, emit);
        for (int p = P + t; p < n2; p += kBlock) keys[p] = ~0ull;
        __syncthreads();
        // bitonic network over n2 keys: each thread takes pairs (i, i | j)
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < (n2 >> 1); q += kBlock) {
                    const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                    const unsigned long long x = keys[i], y = keys[i | j];
                    if ((x > y) == ((i & k) == 0)) {
                        keys[i] = y;
                        keys[i | j] = x;
                    }
                }
                __syncthreads();
            }
        }
        // heads: a sorted position whose (row, column) differs from its predecessor's
        int total = 0;
        for (int p0 = 0; p0 < P; p0 += kBlock) {
            const int p = p0 + t;
            const unsigned long long key = p < P ? keys[p] : 0;
            const bool head = p < P && (p == 0 || (keys[p - 1] >> 12) != (key >> 12));
            const int rank = sg_rank(head, wave_cnt, total);
            if constexpr (NUM) {
                if (head) {
                    double v = vals[key & 4095];
                    for (int q = p + 1; q < P; ++q) {
                        const unsigned long long next = keys[q];
                        if ((next >> 12) != (key >> 12)) break;
                        v = sg_add(v, vals[next & 4095]);
                    }
                    const long long at = (long long)rpC[row0] + rank;
                    colC[at] = (int)(unsigned)(key >> 12);
                    valC[at] = (T)v;
                }
            } else {
                if (p < P) heads[p] = rank + (head ? 1 : 0);
            }
        }
        if constexpr (!NUM) {
            __syncthreads();
            // the first sorted position of a row knows where the row ends: its products are contiguous
            for (int p = t; p < P; p += kBlock) {
                const int r = (int)(keys[p] >> 44);
                if (p == 0 || (int)(keys[p - 1] >> 44) != r) {
                    const int last = p + (int)products[row0 + r] - 1;
                    row_cnt[row0 + r] = heads[last] - (p ? heads[p - 1] : 0);
                }
            }
        }
        __syncthreads();  // the next block rewrites keys
    }
}

// ---- the global tier.  rows[k] = the k-th long row of the chunk, off[k] = its first product in the chunk's arrays
// (off[nrows] = the chunk's products).
template <typename T, bool NUM>
__global__ __launch_bounds__(kBlock) void sg_expand(int nrows, const int *__restrict__ rows, const long long *__restrict__ off,
                                                    int col_bits, const int *__restrict__ rpA, const int *__restrict__ colA,
                                                    const T *__restrict__ valA, const int *__restrict__ rpB,
                                                    const int *__restrict__ colB, const T *__restrict__ valB,
                                                    unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    __shared__ SgTile<long long> s;
    for (int k = blockIdx.x; k < nrows; k += gridDim.x) {
        const int r = rows[k];
        const unsigned long long hi = (unsigned long long)k << col_bits;
        auto row_of = [&](int) { return k; };
        auto emit = [&](long long p, int slot, int f) {
            keys[p] = hi | (unsigned)colB[f];
            if constexpr (NUM) vals[p] = sg_mul(s.a[slot], (double)valB[f]);
        };
        sg_expand_entries<T, NUM, long long>(s, rpA[r], rpA[r + 1], off[k], colA, valA, rpB, row_of, emit);
    }
}

// sorted keys -> the count of heads of every row of the chunk (a row's keys are its own segment: the row leads the key)
__global__ __launch_bounds__(kBlock) void sg_row_heads(int nrows, const int *__restrict__ rows, const long long *__restrict__ off,
                                                       const unsigned long long *__restrict__ keys, int *__restrict__ row_cnt) {
    __shared__ int wave_cnt[kBlock / 64];
    for (int k = blockIdx.x; k < nrows; k += gridDim.x) {
        const long long p0 = off[k], p1 = off[k + 1];
        int total = 0;
        for (long long base = p0; base < p1; base += kBlock) {
            const long long p = base + threadIdx.x;
            const bool head = p < p1 && (p == p0 || keys[p - 1] != keys[p]);
            (void)sg_rank(head, wave_cnt, total);
        }
        if (threadIdx.x == 0) row_cnt[rows[k]] = total;  // (fewer than 2^31: a row of C has at most N entries)
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void sg_row_compress(int nrows, const int *__restrict__ rows, const long long *__restrict__ off,
                                                          unsigned long long col_mask, const unsigned long long *__restrict__ keys,
                                                          const double *__restrict__ vals, const int *__restrict__ rpC,
                                                          int *__restrict__ colC, T *__restrict__ valC) {
    __shared__ int wave_cnt[kBlock / 64];
    for (int k = blockIdx.x; k < nrows; k += gridDim.x) {
        const long long p0 = off[k], p1 = off[k + 1];
        const long long out = rpC[rows[k]];
        int total = 0;
        for (long long base = p0; base < p1; base += kBlock) {
            const long long p = base + threadIdx.x;
            const unsigned long long key = p < p1 ? keys[p] : 0;
            const bool head = p < p1 && (p == p0 || keys[p - 1] != key);
            const int rank = sg_rank(head, wave_cnt, total);
            if (head) {
                double v = vals[p];
                for (long long q = p + 1; q < p1 && keys[q] == key; ++q) v = sg_add(v, vals[q]);
                colC[out + rank] = (int)(key & col_mask);
                valC[out + rank] = (T)v;
            }
        }
    }
}

}  // namespace spmv
