// amg_setup_kernels.hpp -- the kernels of the AMG device setup (spmv_amg_setup.hip runs the level loop; host/amg_plan.c
// is the definition: every kernel here restates one of its loops and gives its bytes) (gfx950).  fp64 throughout.
//
//   as_row_stats      d_i = a_ii and q_i = (sum_j |a_ij|) / d_i, the sum in stored order, one rounded add per entry: a
//                     lane owns a row, one stream over A.  Reduced to three words: the lowest row whose diagonal is
//                     missing or not finite and > 0 (row * 2 + (1: present but bad)), max q over the finite q (their bit
//                     patterns: q >= 0, so the patterns order as the values do), and whether some q is NaN or infinite
//   as_strong_count   strong entries of every row: j != i, a != 0, |a| >= theta sqrt(d_i d_j)
//   as_strong_emit    both directions of every strong entry as keys row << col_bits | col at the row's scanned offset
//   as_graph          sorted keys without repeats -> s_rp (rows without neighbours included, as tr_row_ptr does) and s_col
//   as_smooth         P = T - diag(w / d) (A T) in place on A T's values, the pattern kept (cancelled entries stay)
//   as_round<T>       an operator's values rounded once to T, and whether one of them is not finite in T
//   as_g<T>           g_i = w / (double)(T)d_i, and the lowest row where that is not finite
//
// The arithmetic that decides bytes is written as single IEEE operations with contraction off (sqrt and the division are
// correctly rounded in double on this target); the reductions are integer min / max / or, so their order does not matter.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"

namespace spmv {

constexpr int kAsMaxGrid = 1 << 16;  // grid cap: rows and entries stride over the workgroups beyond it
constexpr int kAsSmoothLanes = 8;    // lanes per row of as_smooth (rows of A T are short)
enum { kAsBadRow = 0, kAsMaxQ = 1, kAsNotFinite = 2, kAsStatWords = 3 };

__device__ __forceinline__ unsigned long long as_wave_min(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long as_wave_max(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// res[kAsStatWords] starts as {~0, 0, 0}
__global__ __launch_bounds__(kBlock) void as_row_stats(int n, const int *__restrict__ rp, const int *__restrict__ col,
                                                       const double *__restrict__ val, double *__restrict__ d,
                                                       unsigned long long *__restrict__ res) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * kBlock;
    unsigned long long bad = ~0ull, qmax = 0, not_finite = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double di = 0.0, sum = 0.0;
        bool have = false;
        const int e1 = rp[i + 1];
        for (int e = rp[i]; e < e1; ++e) {
            const double a = val[e];
            if (col[e] == i) di = a, have = true;
            sum = sum + fabs(a);
        }
        if (!have || !isfinite(di) || !(di > 0.0)) {
            const unsigned long long key = (unsigned long long)i * 2 + (have ? 1 : 0);
            bad = key < bad ? key : bad;
            continue;
        }
        d[i] = di;
        const double q = sum / di;
        if (isfinite(q)) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(q);
            qmax = bits > qmax ? bits : qmax;
        } else {
            not_finite = 1;
        }
    }
    bad = as_wave_min(bad), qmax = as_wave_max(qmax), not_finite = as_wave_max(not_finite);
    if ((threadIdx.x & 63) == 0) {
        if (bad != ~0ull) atomicMin(&res[kAsBadRow], bad);
        if (qmax) atomicMax(&res[kAsMaxQ], qmax);
        if (not_finite) atomicMax(&res[kAsNotFinite], 1ull);
    }
}

__device__ __forceinline__ bool as_strong(int i, int j, double a, double theta, const double *__restrict__ d) {
#pragma clang fp contract(off)
    if (j == i || !(a != 0.0)) return false;
    const double dd = d[i] * d[j];
    const double bound = theta * sqrt(dd);
    return fabs(a) >= bound;
}

__global__ __launch_bounds__(kBlock) void as_strong_count(int n, const int *__restrict__ rp, const int *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ d,
                                                          double theta, int *__restrict__ cnt) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int c = 0;
        const int e1 = rp[i + 1];
        for (int e = rp[i]; e < e1; ++e) c += as_strong((int)i, col[e], val[e], theta, d) ? 1 : 0;
        cnt[i] = c;
    }
}

// off[i] = strong entries in front of row i; keys: two per strong entry
__global__ __launch_bounds__(kBlock) void as_strong_emit(int n, const int *__restrict__ rp, const int *__restrict__ col,
                                                         const double *__restrict__ val, const double *__restrict__ d,
                                                         double theta, int col_bits, const long long *__restrict__ off,
                                                         unsigned long long *__restrict__ keys) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        long long p = 2 * off[i];
        const int e1 = rp[i + 1];
        for (int e = rp[i]; e < e1; ++e) {
            const int j = col[e];
            if (!as_strong((int)i, j, val[e], theta, d)) continue;
            keys[p++] = (unsigned long long)i << col_bits | (unsigned)j;
            keys[p++] = (unsigned long long)(unsigned)j << col_bits | (unsigned long long)i;
        }
    }
}

// E sorted keys without repeats -> s_rp[n + 1] and s_col[E]
__global__ __launch_bounds__(kBlock) void as_graph(long long E, int n, int col_bits, const unsigned long long *__restrict__ keys,
                                                   int *__restrict__ s_rp, int *__restrict__ s_col) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e > E) return;
    if (e == E) {  // rows behind the last edge's row (all of them when E == 0)
        const int last = E ? (int)(keys[E - 1] >> col_bits) : -1;
        for (int r = last + 1; r <= n; ++r) s_rp[r] = (int)E;
        return;
    }
    const unsigned long long key = keys[e];
    const int r = (int)(key >> col_bits);
    const int prev = e ? (int)(keys[e - 1] >> col_bits) : -1;
    for (int q = prev + 1; q <= r; ++q) s_rp[q] = (int)e;
    s_col[e] = (int)(key & ((1ull << col_bits) - 1));
}

__global__ __launch_bounds__(kBlock) void as_smooth(int n, const int *__restrict__ rp, const int *__restrict__ col,
                                                    double *__restrict__ val, const int *__restrict__ agg,
                                                    const double *__restrict__ d, double w) {
#pragma clang fp contract(off)
    const int sub = threadIdx.x % kAsSmoothLanes;
    const long long stride = (long long)gridDim.x * (kBlock / kAsSmoothLanes);
    for (long long i = (long long)blockIdx.x * (kBlock / kAsSmoothLanes) + threadIdx.x / kAsSmoothLanes; i < n; i += stride) {
        const double g = w / d[i];
        const int a = agg[i], e1 = rp[i + 1];
        for (int e = rp[i] + sub; e < e1; e += kAsSmoothLanes) {
            const double t = g * val[e];
            val[e] = (col[e] == a ? 1.0 : 0.0) - t;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void as_round(long long nz, const double *__restrict__ in, T *__restrict__ out,
                                                   int *__restrict__ not_finite) {
    const long long stride = (long long)gridDim.x * kBlock;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < nz; e += stride) {
        const T v = (T)in[e];
        out[e] = v;
        bad = bad || !isfinite((double)v);
    }
    if (bad) atomicOr(not_finite, 1);
}

// bad_row starts as INT_MAX
template <typename T>
__global__ __launch_bounds__(kBlock) void as_g(int n, const double *__restrict__ d, double w, double *__restrict__ g,
                                               int *__restrict__ bad_row) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double v = w / (double)(T)d[i];
        g[i] = v;
        if (!isfinite(v)) atomicMin(bad_row, (int)i);
    }
}

}  // namespace spmv
