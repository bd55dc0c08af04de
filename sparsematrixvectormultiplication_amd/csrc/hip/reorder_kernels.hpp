// reorder_kernels.hpp -- the kernels of the permuted handle and of the reverse Cuthill-McKee ordering (spmv_reorder.hip;
// the definitions: include/spmv_hip.h).
//
// permute
//   ro_first_position     (first[] and first_bad start at all ones) first[v] = the first position that holds v, by
//                         atomicMin of the position (an index, never a value); the first position with a value outside [0, n) goes to first_bad the same way.  Of a
//                         permutation this is the inverse
//   ro_repeats            a position whose value was first seen earlier repeats it: atomicMin into first_bad as well
//   ro_row_lengths        cnt[i] = the length of A's row row_perm[i]
//   ro_copy_rows<T>       `lanes` lanes per row of C (a group lies inside one wave), rows striding over the grid: col and
//                         val of A's row read coalesced and written coalesced at the row's new place, the column mapped
//                         through the inverse of col_perm
//
// rcm (G: the canonical pattern of A + A^T, rows ascending, a stored diagonal still in it)
//   rcm_degrees           deg[v] = row length minus a stored diagonal (binary search), key[v] = deg << 32 | v
//   rcm_ranks             from the sorted keys: by_key[r] = v, rank[v] = r, and the number of isolated nodes (deg 0: they
//                         lead the sort, in index order)
//   rcm_isolated          the isolated nodes take the first places of seq in that order
//   rcm_next_start        the first unvisited node of by_key from the cursor on (one workgroup, a ballot per 256)
//   rcm_expand<ORDER>     lane groups over the frontier's rows (rcm_expand_rows; a row beyond kRcmLongRow entries is walked
//                         by its whole wave).  Every unvisited neighbour is claimed for the next level by atomicMax of the
//                         level's stamp into mark[] (the first claim appends it to the list: a work list, no result
//                         depends on its order).  ORDER: atomicMin of the parent's position in seq into parent[].
//                         Integer min and max: the outcome does not depend on arrival order
//   rcm_keys / rcm_place  key = (parent - first position of the frontier) << rank bits | rank; after the sort the k-th key
//                         names the node of place f1 + k.  rank is the place in the (deg, index) order, so one 64-bit key
//                         holds the whole triple (parent, deg, index) for any n
//   rcm_min_rank          the smallest (deg, index) node of a list (a search's last level)
//   rcm_chain<ORDER>      ONE workgroup of 1024 threads walks a run of levels whose frontiers hold at most `cap` nodes, a
//                         barrier between levels (trsv_chain's shape): the same expansion into an LDS candidate list, the
//                         bitonic network of spgemm_kernels.hpp over the keys, the places, the next level.  It stops when
//                         the frontier is empty or the next one exceeds cap and leaves its state in `state` for the wide
//                         tier.  ORDER = false (a peripheral search): no sort, the lists stay in global memory
//   rcm_bandwidth         max |place[i] - place[j]| over the stored entries (place NULL: the indices themselves)
//
// No kernel waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"

namespace spmv {

constexpr int kRcmUnvisited = 0x7fffffff;
// The chain's cap.  The workgroup keeps `cap` 64-bit keys in LDS: 8 bytes per node, 32 KiB at the largest cap, which is
// inside the 64 KiB a workgroup may declare statically.  Auto is 1024, set by reasoning from that budget: a wide level
// costs five launches and a four-byte read whatever its size (some tens of microseconds), while one workgroup of 1024
// threads has a level of up to 1024 nodes' rows in flight in one or a few trips of its lane groups and sorts 1024 keys in
// 55 steps of one compare-exchange per thread; beyond 1024 nodes the sort takes several exchanges per thread per step and
// the single CU becomes the slower way.  (profiles/rcm.md has the per-level times measured afterwards.)
constexpr int kRcmChainMin = 64, kRcmChainMax = 4096, kRcmChainAuto = 1024;
constexpr int kRcmChainBlock = 1024;  // threads of the chain's one workgroup: a level's rows are loads in flight, not work
constexpr int kRcmLongRow = 256;      // a longer row is walked by its whole wave
constexpr int kRoMaxGrid = 1 << 14;  // grid cap of the row kernels (rows stride over the groups beyond it)
// rcm_chain's state words
enum { kRcmF0, kRcmF1, kRcmLevels, kRcmStatus, kRcmCount, kRcmWhich, kRcmSmallest, kRcmStateWords };
enum { kRcmDone = 0, kRcmOverflow = 1 };

// ------------------------------------------------------------------ permute
__global__ __launch_bounds__(kBlock) void ro_first_position(int n, const int *__restrict__ perm, unsigned *__restrict__ first,
                                                            unsigned *__restrict__ first_bad) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int v = perm[i];
    if (v < 0 || v >= n) atomicMin(first_bad, (unsigned)i);
    else atomicMin(&first[v], (unsigned)i);
}

__global__ __launch_bounds__(kBlock) void ro_repeats(int n, const int *__restrict__ perm, const unsigned *__restrict__ first,
                                                     unsigned *__restrict__ first_bad) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int v = perm[i];
    if (v >= 0 && v < n && first[v] != (unsigned)i) atomicMin(first_bad, (unsigned)i);
}

__global__ __launch_bounds__(kBlock) void ro_row_lengths(int M, const int *__restrict__ row_perm, const int *__restrict__ rp,
                                                         int *__restrict__ cnt) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const int r = row_perm ? row_perm[i] : (int)i;
    cnt[i] = rp[r + 1] - rp[r];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void ro_copy_rows(int M, int lanes_log2, const int *__restrict__ row_perm,
                                                       const int *__restrict__ inv_col, const int *__restrict__ rpA,
                                                       const int *__restrict__ colA, const T *__restrict__ valA,
                                                       const int *__restrict__ rpC, int *__restrict__ colC,
                                                       T *__restrict__ valC) {
    const int lanes = 1 << lanes_log2;
    const int sub = threadIdx.x & (lanes - 1);
    const long long groups = ((long long)gridDim.x * kBlock) >> lanes_log2;
    for (long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) >> lanes_log2; i < M; i += groups) {
        const int r = row_perm ? row_perm[i] : (int)i;
        const int a0 = rpA[r], len = rpA[r + 1] - a0, c0 = rpC[i];
        for (int k = sub; k < len; k += lanes) {
            const int c = colA[a0 + k];
            colC[c0 + k] = inv_col ? inv_col[c] : c;
            valC[c0 + k] = valA[a0 + k];
        }
    }
}

// ------------------------------------------------------------------ rcm
__global__ __launch_bounds__(kBlock) void rcm_degrees(int n, const int *__restrict__ rp, const int *__restrict__ col,
                                                      int *__restrict__ deg, unsigned long long *__restrict__ key) {
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    const int b = rp[v], len = rp[v + 1] - b;
    int lo = 0, hi = len;  // the first entry with a column >= v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[b + mid] < (int)v) lo = mid + 1;
        else hi = mid;
    }
    const int d = len - (lo < len && col[b + lo] == (int)v ? 1 : 0);
    deg[v] = d;
    key[v] = (unsigned long long)d << 32 | (unsigned)v;
}

__global__ __launch_bounds__(kBlock) void rcm_ranks(int n, const unsigned long long *__restrict__ sorted,
                                                    int *__restrict__ by_key, int *__restrict__ rank,
                                                    int *__restrict__ n_isolated) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const unsigned long long k = sorted[r];
    const int v = (int)(unsigned)k;
    by_key[r] = v;
    rank[v] = (int)r;
    // (n_isolated starts at 0) the last node of degree 0 tells how many there are
    if ((k >> 32) == 0 && (r + 1 == n || (sorted[r + 1] >> 32) != 0)) *n_isolated = (int)r + 1;
}

__global__ __launch_bounds__(kBlock) void rcm_isolated(int n_iso, const int *__restrict__ by_key, int *__restrict__ seq,
                                                       int *__restrict__ pos) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_iso) return;
    const int v = by_key[r];
    seq[r] = v;
    pos[v] = (int)r;
}

// out[0] = the cursor of the first unvisited node of by_key at or behind `cursor` (n: none), out[1] = the node
__global__ __launch_bounds__(kBlock) void rcm_next_start(int n, int cursor, const int *__restrict__ by_key,
                                                         const int *__restrict__ pos, int *__restrict__ out) {
    __shared__ int found;
    if (threadIdx.x == 0) found = n;
    __syncthreads();
    for (long long base = cursor; base < n; base += kBlock) {
        const long long c = base + threadIdx.x;
        if (c < n && pos[by_key[c]] == kRcmUnvisited) atomicMin(&found, (int)c);
        __syncthreads();
        if (found < n) break;  // (uniform: read behind the barrier, not written again before the next one)
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = found;
        out[1] = found < n ? by_key[found] : -1;
    }
}

// the start node of a component takes place f0; ORDER = false: the start of a search is claimed with its stamp
template <bool ORDER>
__global__ void rcm_seed(int s, int f0, int stamp, int *__restrict__ seq, int *__restrict__ pos, int *__restrict__ mark,
                         int *__restrict__ list) {
    if (threadIdx.x || blockIdx.x) return;
    if (ORDER) {
        seq[f0] = s;
        pos[s] = f0;
    } else {
        list[0] = s;
        mark[s] = stamp;
    }
}

// One neighbour of frontier node u (at place p): claim it for the next level.  Returns true for the first claim.
template <bool ORDER>
__device__ __forceinline__ bool rcm_claim(int w, int u, int p, int stamp, const int *pos, int *parent, int *mark) {
    if (w == u || pos[w] != kRcmUnvisited) return false;
    if (ORDER) atomicMin(&parent[w], p);
    return atomicMax(&mark[w], stamp) < stamp;
}

// The expansion both tiers share.  Groups of 2^lanes_log2 lanes take the frontier's nodes: group g takes nodes first + g,
// first + g + stride, ...  (`first` is the node of the calling WAVE's first group, so that the wave leaves the loop
// together).  A row longer than kRcmLongRow is not its group's: the wave finds such rows with a ballot and walks each with
// all 64 lanes, so a hub row costs a wave's trips, not a lane pair's.  emit(w) takes every first claim.
// frontier: `count` nodes; ORDER: they are seq[f0 .. f0 + count), and node k's place is f0 + k
template <bool ORDER, typename Emit>
__device__ __forceinline__ void rcm_expand_rows(long long first, long long stride, int count, int lanes_log2,
                                                const int *frontier, int f0, int stamp, const int *__restrict__ rp,
                                                const int *__restrict__ col, const int *pos, int *parent, int *mark, Emit emit) {
    const int lanes = 1 << lanes_log2;
    const int lane = threadIdx.x & 63, sub = lane & (lanes - 1);
    for (long long kw = first; kw < count; kw += stride) {
        const long long k = kw + (lane >> lanes_log2);
        const bool live = k < count;
        const int u = live ? frontier[k] : 0;
        const int b = live ? rp[u] : 0, e1 = live ? rp[u + 1] : 0;
        const bool is_long = lanes < 64 && e1 - b > kRcmLongRow;
        if (!is_long)
            for (int e = b + sub; e < e1; e += lanes) {
                const int w = col[e];
                if (rcm_claim<ORDER>(w, u, f0 + (int)k, stamp, pos, parent, mark)) emit(w);
            }
        unsigned long long todo = __ballot(is_long && sub == 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int u2 = __shfl(u, src), b2 = __shfl(b, src), end2 = __shfl(e1, src);
            const int p2 = f0 + (int)kw + (src >> lanes_log2);
            for (int e = b2 + lane; e < end2; e += 64) {
                const int w = col[e];
                if (rcm_claim<ORDER>(w, u2, p2, stamp, pos, parent, mark)) emit(w);
            }
        }
    }
}

template <bool ORDER>
__global__ __launch_bounds__(kBlock) void rcm_expand(int count, int lanes_log2, const int *__restrict__ frontier, int f0,
                                                     int stamp, const int *__restrict__ rp, const int *__restrict__ col,
                                                     const int *__restrict__ pos, int *__restrict__ parent,
                                                     int *__restrict__ mark, int *__restrict__ next, int *__restrict__ n_next) {
    const long long wave_thread = ((long long)blockIdx.x * kBlock + threadIdx.x) & ~63ll;
    rcm_expand_rows<ORDER>(wave_thread >> lanes_log2, ((long long)gridDim.x * kBlock) >> lanes_log2, count, lanes_log2, frontier,
                           f0, stamp, rp, col, pos, parent, mark, [&](int w) { next[atomicAdd(n_next, 1)] = w; });
}

__global__ __launch_bounds__(kBlock) void rcm_keys(int count, int f0, unsigned rank_bits, const int *__restrict__ cand,
                                                   const int *__restrict__ parent, const int *__restrict__ rank,
                                                   unsigned long long *__restrict__ key) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int w = cand[i];
    key[i] = (unsigned long long)(unsigned)(parent[w] - f0) << rank_bits | (unsigned)rank[w];
}

__global__ __launch_bounds__(kBlock) void rcm_place(int count, int f1, unsigned rank_bits,
                                                    const unsigned long long *__restrict__ sorted,
                                                    const int *__restrict__ by_key, int *__restrict__ seq,
                                                    int *__restrict__ pos) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int w = by_key[sorted[i] & ((1ull << rank_bits) - 1)];
    seq[f1 + i] = w;
    pos[w] = f1 + (int)i;
}

// (*smallest starts at kRcmUnvisited) the node is by_key[*smallest]
__global__ __launch_bounds__(kBlock) void rcm_min_rank(int count, const int *__restrict__ list, const int *__restrict__ rank,
                                                       int *__restrict__ smallest) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    int r = i < count ? rank[list[i]] : kRcmUnvisited;
    for (int o = 32; o > 0; o >>= 1) r = min(r, __shfl_xor(r, o));
    if ((threadIdx.x & 63) == 0 && r != kRcmUnvisited) atomicMin(smallest, r);
}

// The chained levels.  ORDER: the frontier is seq[f0 .. f1), `levels` is 0 and counts the expansions; stamps stamp0,
// stamp0 + 1, ... one per level.  ORDER = false: the frontier is the f1 - f0 nodes of list `which`, one stamp for the whole
// search, and `levels` is the search's depth so far.  The state on return says where the wide tier goes on.
template <bool ORDER>
__global__ __launch_bounds__(kRcmChainBlock) void rcm_chain(int cap, int lanes_log2, int stamp0, unsigned rank_bits, int f0, int f1,
                                                            int levels, int which, const int *__restrict__ rp,
                                                            const int *__restrict__ col, const int *__restrict__ rank,
                                                            const int *__restrict__ by_key, int *seq, int *pos, int *parent,
                                                            int *mark, int *list0, int *list1, int *state) {
    __shared__ unsigned long long keys[ORDER ? kRcmChainMax : 1];
    __shared__ int n_next, smallest;
    const int t = threadIdx.x;
    const long long wave_first = (t & ~63) >> lanes_log2, stride = kRcmChainBlock >> lanes_log2;
    int count = f1 - f0;
    int status = kRcmDone;
    for (;;) {
        if (t == 0) n_next = 0, smallest = kRcmUnvisited;
        __syncthreads();
        const int *frontier = ORDER ? seq + f0 : (which ? list1 : list0);
        int *next = which ? list0 : list1;
        const int stamp = ORDER ? stamp0 + levels : stamp0;
        rcm_expand_rows<ORDER>(wave_first, stride, count, lanes_log2, frontier, f0, stamp, rp, col, pos, parent, mark, [&](int w) {
            const int at = atomicAdd(&n_next, 1);
            if (ORDER) {
                // the candidate waits in the key's place: its rank names it (parent[] is final behind the barrier)
                if (at < cap) keys[at] = (unsigned)rank[w];
            } else {
                next[at] = w;
            }
        });
        __syncthreads();
        const int found = n_next;
        if (ORDER && found > cap) {  // the level is the wide tier's: it claims with a stamp of its own
            status = kRcmOverflow;
            break;
        }
        if (found == 0) {  // the last level: its smallest node (a search wants it)
            if (!ORDER) {
                for (int k = t; k < count; k += kRcmChainBlock) atomicMin(&smallest, rank[frontier[k]]);
                __syncthreads();
            }
            if (ORDER) ++levels;  // (this expansion counts; a search's depth is the levels that hold nodes)
            f0 = f1;
            count = 0;
            break;
        }
        if (ORDER) {
            int n2 = 2;
            while (n2 < found) n2 <<= 1;
            for (int p = t; p < n2; p += kRcmChainBlock) {
                if (p < found) {
                    const int w = by_key[(unsigned)keys[p]];
                    // (an atomic read: parent[] was written by atomics, which a cached line would not show)
                    const int par = __hip_atomic_load(&parent[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    keys[p] |= (unsigned long long)(unsigned)(par - f0) << rank_bits;
                } else {
                    keys[p] = ~0ull;
                }
            }
            __syncthreads();
            for (int k = 2; k <= n2; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int q = t; q < (n2 >> 1); q += kRcmChainBlock) {
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
            for (int p = t; p < found; p += kRcmChainBlock) {
                const int w = by_key[keys[p] & ((1ull << rank_bits) - 1)];
                seq[f1 + p] = w;
                pos[w] = f1 + p;
            }
            f0 = f1;
            f1 += found;
        } else {
            which ^= 1;
        }
        ++levels;
        count = found;
        __syncthreads();
        if (!ORDER && found > cap) {  // a complete level, too wide to go on here
            status = kRcmOverflow;
            break;
        }
    }
    if (t == 0) {
        state[kRcmF0] = f0;
        state[kRcmF1] = f1;
        state[kRcmLevels] = levels;
        state[kRcmStatus] = status;
        state[kRcmCount] = count;
        state[kRcmWhich] = which;
        state[kRcmSmallest] = smallest != kRcmUnvisited ? by_key[smallest] : -1;  // (the node, not its rank)
    }
}

// (*out starts at 0) place NULL: the bandwidth of the matrix as it is numbered
__global__ __launch_bounds__(kBlock) void rcm_bandwidth(int M, const int *__restrict__ rp, const int *__restrict__ col,
                                                        const int *__restrict__ place, int *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kBlock / 64);
    int widest = 0;
    for (long long r = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < M; r += waves) {
        const int pr = place ? place[r] : (int)r;
        const int e1 = rp[r + 1];
        for (int e = rp[r] + lane; e < e1; e += 64) widest = max(widest, abs(pr - (place ? place[col[e]] : col[e])));
    }
    for (int o = 32; o > 0; o >>= 1) widest = max(widest, __shfl_xor(widest, o));
    if (lane == 0 && widest) atomicMax(out, widest);
}

}  // namespace spmv
