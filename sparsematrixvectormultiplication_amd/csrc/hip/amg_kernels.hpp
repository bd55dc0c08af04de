// amg_kernels.hpp -- the kernels of the smoothed-aggregation AMG preconditioner's V(1,1) cycle (spmv_amg.hip builds the
// hierarchy and launches them; host/amg_plan.c is the setup) (gfx950).
//
// A cycle is a fixed list of PASSES (AmgStep), made once at build time.  A pass writes one vector `out` of n rows from
// vectors written by earlier passes:
//
//   kAmgScale    out = g . b                        (the first sweep from x = 0)
//   kAmgSub      out = b - in                       (level 0: r = b - t, t = A_0 x by the handle's own launch)
//   kAmgAxpy     out = in + g . (b - aux)           (level 0: x' = x + g . (b - t))
//   kAmgMul      out = M in                         (b' = R r;  x = Ainv b)
//   kAmgResid    out = b - M in                     (r = b - A x)
//   kAmgAdd      out = out + M in                   (x += P e: in place, a row touches only its own x)
//   kAmgSmooth   out = in + g . (b - M in)          (x' = x + g . (b - A x): out is a SECOND vector, never `in`; in place
//                                                    it would be a racy Gauss-Seidel and lose bit reproducibility)
//
// The first three are element-wise.  The others are amg_rows, in the shape of trsv_rows (trsv_kernels.hpp): G
// neighbouring lanes per row, G a power of two <= 32 chosen per operator at build time from its mean row; lane `sub`
// adds the entries e0 + sub, e0 + sub + G, ... in double, group_sum_rt adds the lanes (a fixed butterfly), lane 0 forms
// the row's value in double and rounds once to T.  The loop bounds are wave-uniform: group_sum needs every lane.
// Vectors are row-major n x k; a group keeps KT columns in registers and walks its row once per tile of KT columns, so
// column j's sum has the order of the k = 1 sum whatever j and k are.  No atomics.
//
//   amg_pass   one launch = one pass over a grid
//   amg_tail   one launch = passes [s0, s1) by ONE workgroup with __syncthreads() between them: the levels that are too
//              small to be worth a launch each.  The visibility argument is trsv_chain's: vectors are written with plain
//              global stores and read with plain global loads, __syncthreads() is a workgroup-scope release before the
//              barrier and an acquire after it, and in the default execution mode a workgroup's waves share one CU's
//              vector L1 (a build for threadgroup-split mode needs a second look).  The vectors are never __restrict__
//              and never read on a scalar or non-temporal path.  0 bytes of LDS.
//
// Both call amg_step, so a chained cycle has the bits of an unchained one.  No kernel waits for another workgroup.
#pragma once
#include "solver_ops.hpp"

namespace spmv {

// The two tail limits are trsv's (kTrsvChainRows, kTrsvChainEntries), set by the same reasoning and not by a sweep: a
// level one workgroup passes over in a round or a few.
constexpr int kAmgChainRows = 256;      // the tail starts at the first level below 0 with at most this many rows ...
constexpr int kAmgChainEntries = 4096;  // ... and this many entries of A_l
constexpr int kAmgBlocks = 2048;        // grid cap of amg_pass (it strides beyond)
constexpr int kAmgMaxLevels = 16;
constexpr int kAmgTile = 4;             // columns a group keeps in registers for k > 1

enum { kAmgScale = 0, kAmgSub, kAmgAxpy, kAmgMul, kAmgResid, kAmgAdd, kAmgSmooth };
// a vector of a pass: an offset >= 0 counts values at k = 1 from the workspace (times k for k columns); the apply's r
// and z are named
enum { kAmgVecNone = -1, kAmgVecR = -2, kAmgVecZ = -3 };

struct AmgStep {
    int op, n, G, pad;
    const int *rp, *col;   // the operator M (NULL for the element-wise passes)
    const void *val;       // ... its values in T
    const double *g;       // w / d of the pass's level (NULL where unused)
    long long in, aux, b, out;  // vectors (kAmgVec*)
};

template <typename T>
__device__ __forceinline__ T *amg_vec(long long v, int k, T *work, const T *R, T *Z) {
    return v >= 0 ? work + v * k : v == kAmgVecR ? const_cast<T *>(R) : v == kAmgVecZ ? Z : nullptr;
}

// rows [0, n) of pass OP by `nthreads` threads of which this is `tid` (nthreads a multiple of 64)
template <typename T, int OP, int KT>
__device__ __forceinline__ void amg_rows(const AmgStep &s, int k, long long tid, long long nthreads, const T *in,
                                         const T *b, T *out) {
    const int *__restrict__ rp = s.rp;
    const int *__restrict__ col = s.col;
    const T *__restrict__ val = (const T *)s.val;
    const double *__restrict__ g = s.g;
    const int G = s.G, sub = (int)(tid & (G - 1)), n = s.n;
    const long long groups = nthreads / G;
    for (long long i0 = 0; i0 < n; i0 += groups) {
        const long long i = i0 + tid / G;
        const bool on = i < n;
        const int e0 = on ? rp[i] : 0, e1 = on ? rp[i + 1] : 0;
        for (int j0 = 0; j0 < k; j0 += KT) {  // k is uniform: every lane of the wave walks every tile
            double acc[KT];
#pragma unroll
            for (int c = 0; c < KT; ++c) acc[c] = 0.0;
            for (int e = e0 + sub; e < e1; e += G) {
                const double a = (double)val[e];
                const T *x = in + (long long)col[e] * k + j0;
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (KT == 1 || j0 + c < k) acc[c] += a * (double)x[c];
            }
#pragma unroll
            for (int c = 0; c < KT; ++c) acc[c] = group_sum_rt(acc[c], G);
            if (on && sub == 0) {
#pragma unroll
                for (int c = 0; c < KT; ++c) {
                    if (KT > 1 && j0 + c >= k) continue;
                    const long long q = i * k + j0 + c;
                    double v;
                    if constexpr (OP == kAmgMul) v = acc[c];
                    else if constexpr (OP == kAmgResid) v = (double)b[q] - acc[c];
                    else if constexpr (OP == kAmgAdd) v = (double)out[q] + acc[c];
                    else v = (double)in[q] + g[i] * ((double)b[q] - acc[c]);
                    out[q] = (T)v;
                }
            }
        }
    }
}

// one pass; every branch on s.op and k is uniform over the launch
template <typename T>
__device__ __forceinline__ void amg_step(const AmgStep &s, int k, long long tid, long long nthreads, T *work, const T *R,
                                         T *Z) {
    const T *in = amg_vec<T>(s.in, k, work, R, Z), *aux = amg_vec<T>(s.aux, k, work, R, Z);
    const T *b = amg_vec<T>(s.b, k, work, R, Z);
    T *out = amg_vec<T>(s.out, k, work, R, Z);
    if (s.op <= kAmgAxpy) {
        const long long total = (long long)s.n * k;
        const double *g = s.g;
        for (long long q = tid; q < total; q += nthreads) {
            const long long i = k == 1 ? q : q / k;
            double v;
            if (s.op == kAmgScale) v = g[i] * (double)b[q];
            else if (s.op == kAmgSub) v = (double)b[q] - (double)in[q];
            else v = (double)in[q] + g[i] * ((double)b[q] - (double)aux[q]);
            out[q] = (T)v;
        }
        return;
    }
    if (k == 1) {
        if (s.op == kAmgMul) amg_rows<T, kAmgMul, 1>(s, 1, tid, nthreads, in, b, out);
        else if (s.op == kAmgResid) amg_rows<T, kAmgResid, 1>(s, 1, tid, nthreads, in, b, out);
        else if (s.op == kAmgAdd) amg_rows<T, kAmgAdd, 1>(s, 1, tid, nthreads, in, b, out);
        else amg_rows<T, kAmgSmooth, 1>(s, 1, tid, nthreads, in, b, out);
    } else {
        if (s.op == kAmgMul) amg_rows<T, kAmgMul, kAmgTile>(s, k, tid, nthreads, in, b, out);
        else if (s.op == kAmgResid) amg_rows<T, kAmgResid, kAmgTile>(s, k, tid, nthreads, in, b, out);
        else if (s.op == kAmgAdd) amg_rows<T, kAmgAdd, kAmgTile>(s, k, tid, nthreads, in, b, out);
        else amg_rows<T, kAmgSmooth, kAmgTile>(s, k, tid, nthreads, in, b, out);
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void amg_pass(AmgStep s, int k, T *work, const T *R, T *Z) {
    amg_step<T>(s, k, (long long)blockIdx.x * kBlock + threadIdx.x, (long long)gridDim.x * kBlock, work, R, Z);
}

// one workgroup: passes [s0, s1) one after the other
template <typename T>
__global__ __launch_bounds__(kBlock) void amg_tail(const AmgStep *__restrict__ steps, int s0, int s1, int k, T *work,
                                                   const T *R, T *Z) {
    for (int q = s0; q < s1; ++q) {
        const AmgStep s = steps[q];
        amg_step<T>(s, k, threadIdx.x, kBlock, work, R, Z);
        __syncthreads();  // pass q's vector: released by, and acquired by, every wave of this workgroup
    }
}

}  // namespace spmv
