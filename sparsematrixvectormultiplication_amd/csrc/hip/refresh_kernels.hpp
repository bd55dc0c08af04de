// refresh_kernels.hpp -- the device side of spmv_hip_precond_refresh and spmv_hip_trsv_refresh: new values of a handle
// into a preconditioner or a triangular solver that keeps its symbolic work (spmv_precond.hip, spmv_trsv.hip).
//
//   rf_digest   a 64-bit digest of a handle's pattern: the sum over row_ptr and col of a mix of (place, value).  A sum,
//               so the order of the atomics does not matter; the refresh compares it with the first refresh's on every call
//   rf_gather   the canonical (and permuted) diagonal block in fp64 from the handle's values: entry e of the block is fed
//               by the handle's entries feed[fp[e] .. fp[e + 1]), added in that order -- entry order, as canon_download
//               adds a repeated pair (canon_rows.hpp): the first the plain value, every further one a rounded fp64 sum
//   rf_diag     per row k of the block: its diagonal d = W[diag[k]] out for the host, the inverse the solves use rounded
//               once to T, and the smallest row whose diagonal or inverse is refused in bad[slot] (the build's checks)
//   rf_scatter  dst[s] = (T) W[src[s]]: a triangle's values in level order, one rounding to the dtype
//   rf_pick     dst[q] = v[row[q]]: the inverses in a triangle's level order
#pragma once
#include "spmv_internal.hpp"

namespace spmv {

constexpr int kRfBlocks = 2048;  // grid cap (the kernels stride beyond it)

__device__ __forceinline__ unsigned long long rf_mix(unsigned long long x) {  // splitmix64's finaliser
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// out[0] += sum_i mix(i << 32 | a[i]) (+ salt in the place): the lanes' sums added across the wavefront (a sum modulo
// 2^64: any order gives the same digest), one atomic per wavefront
template <typename I>
__global__ __launch_bounds__(kBlock) void rf_digest(long long n, const I *__restrict__ a, unsigned long long salt,
                                                    unsigned long long *__restrict__ out) {
    unsigned long long acc = 0;
    const long long step = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += step)
        acc += rf_mix((((unsigned long long)i + salt) << 32) ^ (unsigned long long)(unsigned)a[i]);
    for (int d = 32; d > 0; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, d);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rf_gather(long long n, const int *__restrict__ fp, const int *__restrict__ feed,
                                                    const T *__restrict__ val, double *__restrict__ W) {
    const long long step = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < n; e += step) {
        const int f0 = fp[e], f1 = fp[e + 1];
        double acc = (double)val[feed[f0]];
        for (int f = f0 + 1; f < f1; ++f) acc += (double)val[feed[f]];
        W[e] = acc;
    }
}

// mode 0 (a triangular solve, Jacobi's words): inv = 1 / d, refused when d is zero or not finite or inv is not finite;
// mode 1 (SSOR): inv = omega / d, the same refusal;  mode 2 (ILU(0)): inv = 1 / (T) d, refused when inv is not finite
template <typename T>
__global__ __launch_bounds__(kBlock) void rf_diag(int n, int mode, double omega, const int *__restrict__ diag,
                                                  const double *__restrict__ W, double *__restrict__ d_out,
                                                  T *__restrict__ inv, int *__restrict__ bad) {
    const long long step = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += step) {
        const double d = W[diag[k]];
        d_out[k] = d;
        const T t = mode == 2 ? (T)(1.0 / (double)(T)d) : (T)((mode == 1 ? omega : 1.0) / d);
        inv[k] = t;
        const bool refused = mode == 2 ? !isfinite((double)t) : (d == 0.0 || !isfinite(d) || !isfinite((double)t));
        if (refused) atomicMin(bad, (int)k);
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rf_scatter(long long n, const int *__restrict__ src, const double *__restrict__ W,
                                                     T *__restrict__ dst) {
    const long long step = (long long)gridDim.x * kBlock;
    for (long long s = (long long)blockIdx.x * kBlock + threadIdx.x; s < n; s += step) dst[s] = (T)W[src[s]];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rf_pick(long long n, const int *__restrict__ row, const T *__restrict__ v,
                                                  T *__restrict__ dst) {
    const long long step = (long long)gridDim.x * kBlock;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < n; q += step) dst[q] = v[row[q]];
}

inline int rf_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>(kRfBlocks, (n + kBlock - 1) / kBlock)); }

}  // namespace spmv

// The pattern a preconditioner or a triangular solver was refreshed from first: what every later refresh is held to.
struct PatternStamp {
    bool have = false;
    unsigned long long digest = 0;
    long long nz = 0;
    int rows = 0, cols = 0;
};

// spmv_precond.hip: the stamp of handle m (waits for the device; -1: HIP error), and m's pattern against a stamp --
// taken now when there is none yet; -1 with a message naming `what`
int pattern_stamp(const spmv_csr_dev *m, PatternStamp &out);
int pattern_check(const spmv_csr_dev *m, PatternStamp &stamp, const char *what);
