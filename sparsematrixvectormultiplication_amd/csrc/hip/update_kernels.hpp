// update_kernels.hpp -- the device side of spmv_hip_csr_update_values (spmv_update.hip): new values into the arrays of a
// handle's tile plans that hold matrix values in the plans' own order.
//
//   upd_gather   dst[i] = src[i] >= 0 ? val[src[i]] : 0 over the slots of one such array; src is the handle's source map
//                (UpdateState, spmv_internal.hpp): the entry of `val` a slot holds, -1 for a padding slot.
//
// A pure stream with a mostly local gather: a lane takes FOUR neighbouring slots -- one 16-byte load of the map, four
// value loads (a pass holds a block's entries by (row, column): neighbouring slots read neighbouring or nearby entries
// of val, the same lines), 16-byte stores (one for fp32, two for fp64) -- so a wavefront reads 1 KiB of the map and
// writes 1 or 2 KiB of values per trip, each as whole lines.  Passes start on multiples of 4 and the arrays come from
// hipMalloc, so every quad is aligned; the last n % 4 slots of an array that is no multiple of 4 long (the remainder's
// values) are written one by one.  No LDS, no atomics, nothing that could spill; the value is moved bit for bit, a
// non-finite one like any other, and a padding slot gets +0.0 as the builders give it.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_kernels.hpp"  // kBlock

namespace spmv {

constexpr int kUpdBlocks = 2048;  // grid cap (the quads stride over the workgroups beyond it)

template <typename T>
struct upd_quad;  // four values as 16-byte pieces
template <>
struct upd_quad<float> {
    static __device__ __forceinline__ void store(float *dst, float a, float b, float c, float d) {
        *reinterpret_cast<float4 *>(dst) = make_float4(a, b, c, d);
    }
};
template <>
struct upd_quad<double> {
    static __device__ __forceinline__ void store(double *dst, double a, double b, double c, double d) {
        reinterpret_cast<double2 *>(dst)[0] = make_double2(a, b);
        reinterpret_cast<double2 *>(dst)[1] = make_double2(c, d);
    }
};

// n slots; src and dst 16-byte aligned
template <typename T>
__global__ __launch_bounds__(kBlock) void upd_gather(long long n, const int *__restrict__ src, const T *__restrict__ val,
                                                     T *__restrict__ dst) {
    const long long quads = n >> 2;
    const long long step = (long long)gridDim.x * kBlock;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < quads; q += step) {
        const int4 s = reinterpret_cast<const int4 *>(src)[q];
        const T a = s.x >= 0 ? val[s.x] : T(0);
        const T b = s.y >= 0 ? val[s.y] : T(0);
        const T c = s.z >= 0 ? val[s.z] : T(0);
        const T d = s.w >= 0 ? val[s.w] : T(0);
        upd_quad<T>::store(dst + 4 * q, a, b, c, d);
    }
    // the last n % 4 slots (block 0's first lanes)
    const long long i = 4 * quads + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
        const int s = src[i];
        dst[i] = s >= 0 ? val[s] : T(0);
    }
}

}  // namespace spmv
