// trsv_kernels.hpp -- the kernels of the sparse triangular solves and of the ILU(0) factorisation on CSR handles
// (spmv_trsv.hip builds and launches them; the SSOR and ILU(0) preconditioners are made of them) (gfx950).
//
// A triangle is stored in LEVEL ORDER (spmv_trsv_levels, host/trsv_plan.c): place q = 0 .. n - 1 holds one row, the
// rows of a level are neighbours, inside a level the short rows come first.  Per place: rp[q] .. rp[q + 1] its
// off-diagonal entries (col in the numbering of x, val in T), brow[q] the element of b it reads, xrow[q] the element of
// x it writes, dinv[q] the INVERSE of its diagonal, formed in fp64 and rounded once to T (NULL: a unit diagonal).  The
// rows of a level read only x of earlier levels, so a level is one pass over its places:
//
//   trsv_level   one launch = one wide level.  Short rows take G neighbouring lanes each (G a power of two <= 32 chosen
//                at build time from the mean short row: G = 1 is a lane per row), long rows a wavefront each; a lane
//                adds its entries e0 + sub, e0 + sub + G, ... in double, group_sum adds the lanes (wave_ops.hpp), and
//                lane 0 of the group rounds once: x = (T)((b - sum) dinv), or with SCALED (the backward solve of SSOR)
//                x = (T)(scale b - dinv sum).  No atomics; the order is fixed by G and the stored order alone.
//   trsv_chain   one launch = a run of consecutive narrow levels, ONE workgroup, __syncthreads() between levels.  x is
//                written with plain global stores and read with plain global loads.  What orders them is
//                __syncthreads(): a workgroup-scope release before the barrier and acquire after it, so a value of x
//                written by any wave of the workgroup before the barrier is the value every wave reads after it.  In
//                the default execution mode all waves of a workgroup run on one CU and share its vector L1, which is
//                what makes workgroup scope enough; a build for threadgroup-split mode (tgsplit) puts them on several
//                CUs and needs a second look at this kernel and at ilu0_chain.  x is never __restrict__ and never
//                read through a non-temporal or scalar path.  0 bytes of LDS.
//   ilu0_level / ilu0_chain   the numerical ILU(0) with the schedule of the forward solve: one wavefront per row i of
//                the sorted, duplicate-free matrix W (fp64, in place): for each entry (i, k), k < i, ascending:
//                l_ik = w_ik / u_kk; lanes take the entries (k, j), j > k of row k, find j in row i by bisection and
//                subtract l_ik u_kj.  A lane's update must be seen by the whole wave at the next pivot: a
//                workgroup-scope fence between pivots.  Row i ends by checking its pivot (bad[0] = first bad row).
//
// No kernel waits for another workgroup: order between workgroups is launch order on one stream.
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kTrsvLong = 128;          // rows of this many entries or more take a wavefront each
// The two chain limits are set by reasoning (a level one workgroup passes over in a round or a few), not by a sweep.
constexpr int kTrsvChainRows = 256;     // a narrow level: at most this many rows ...
constexpr int kTrsvChainEntries = 4096; // ... and this many entries
constexpr int kTrsvBlocks = 2048;       // grid cap of trsv_level (it strides beyond)

struct TrsvView {  // one triangle in level order (device pointers)
    const int *rp, *col, *brow, *xrow, *level_ptr, *level_split;
    const void *val, *dinv;
};

// places [first, first + count), G lanes per row, by `nthreads` threads of which this is `tid` (nthreads a multiple of
// 64, the loop bounds wave-uniform: group_sum needs every lane)
template <typename T, bool SCALED>
__device__ __forceinline__ void trsv_rows(const TrsvView &t, int first, int count, int G, long long tid,
                                          long long nthreads, double scale, const T *__restrict__ b, T *x) {
    const int *__restrict__ rp = t.rp;
    const int *__restrict__ col = t.col;
    const T *__restrict__ val = (const T *)t.val;
    const T *__restrict__ dinv = (const T *)t.dinv;
    const int sub = (int)(tid & (G - 1));
    const long long groups = nthreads / G;
    for (long long k0 = 0; k0 < count; k0 += groups) {
        const long long k = k0 + tid / G;
        const bool on = k < count;
        const int q = first + (int)(on ? k : 0);
        double acc = 0.0;
        if (on) {
            const int e1 = rp[q + 1];
            for (int e = rp[q] + sub; e < e1; e += G) acc += (double)val[e] * (double)x[col[e]];
        }
        acc = group_sum_rt(acc, G);
        if (on && sub == 0) {
            const double bi = (double)b[t.brow[q]];
            double v;
            if constexpr (SCALED) v = scale * bi - (double)dinv[q] * acc;
            else v = dinv ? (bi - acc) * (double)dinv[q] : bi - acc;
            x[t.xrow[q]] = (T)v;
        }
    }
}

template <typename T, bool SCALED>
__global__ __launch_bounds__(kBlock) void trsv_level(TrsvView t, int level, int G, double scale,
                                                     const int *__restrict__ flags, const T *__restrict__ b, T *x) {
    if (flags && flags[kSolverState] != kSolverRun) return;
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, nthreads = (long long)gridDim.x * kBlock;
    const int p0 = t.level_ptr[level], ps = t.level_split[level], p1 = t.level_ptr[level + 1];
    trsv_rows<T, SCALED>(t, p0, ps - p0, G, tid, nthreads, scale, b, x);
    trsv_rows<T, SCALED>(t, ps, p1 - ps, 64, tid, nthreads, scale, b, x);
}

// one workgroup: levels [l0, l1) one after the other
template <typename T, bool SCALED>
__global__ __launch_bounds__(kBlock) void trsv_chain(TrsvView t, int l0, int l1, int G, double scale,
                                                     const int *__restrict__ flags, const T *__restrict__ b, T *x) {
    if (flags && flags[kSolverState] != kSolverRun) return;
    for (int l = l0; l < l1; ++l) {
        const int p0 = t.level_ptr[l], ps = t.level_split[l], p1 = t.level_ptr[l + 1];
        trsv_rows<T, SCALED>(t, p0, ps - p0, G, threadIdx.x, kBlock, scale, b, x);
        trsv_rows<T, SCALED>(t, ps, p1 - ps, 64, threadIdx.x, kBlock, scale, b, x);
        __syncthreads();  // level l's x: released by, and acquired by, every wave of this workgroup
    }
}

// ---- ILU(0).  W: the matrix's values in fp64 (rp, col sorted and duplicate-free, diag[i] = the place of (i, i)).
// One wavefront factors row i in place: its strict lower part becomes L's row, the rest U's.
__device__ __forceinline__ void ilu0_row(int i, int lane, const int *__restrict__ rp, const int *__restrict__ col,
                                         const int *__restrict__ diag, double *W, int *__restrict__ bad) {
    const int ed = diag[i], e1 = rp[i + 1];
    for (int e = rp[i]; e < ed; ++e) {  // pivots in ascending column order
        const int k = col[e];
        const double lik = W[e] / W[diag[k]];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // every lane has read w_ik before lane 0 replaces it
        if (lane == 0) W[e] = lik;
        const int f1 = rp[k + 1];
        for (int f = diag[k] + 1 + lane; f < f1; f += 64) {
            const int j = col[f];
            int lo = e + 1, hi = e1;  // the first entry of row i with column >= j
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (col[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < e1 && col[lo] == j) W[lo] -= lik * W[f];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the lanes' updates, before the next pivot reads them
    }
    const double d = W[ed];
    if (lane == 0 && (d == 0.0 || !isfinite(d))) atomicMin(bad, i);
}

// rows perm[p0 .. p1) of one level, a wavefront each
__global__ __launch_bounds__(kBlock) void ilu0_level(int p0, int p1, const int *__restrict__ perm,
                                                     const int *__restrict__ rp, const int *__restrict__ col,
                                                     const int *__restrict__ diag, double *W, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kBlock / 64);
    for (long long q = p0 + (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); q < p1; q += waves)
        ilu0_row(perm[q], lane, rp, col, diag, W, bad);
}

// one workgroup: levels [l0, l1) one after the other (the barrier as in trsv_chain)
__global__ __launch_bounds__(kBlock) void ilu0_chain(int l0, int l1, const int *__restrict__ level_ptr,
                                                     const int *__restrict__ perm, const int *__restrict__ rp,
                                                     const int *__restrict__ col, const int *__restrict__ diag,
                                                     double *W, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    for (int l = l0; l < l1; ++l) {
        const int p1 = level_ptr[l + 1];
        for (int q = level_ptr[l] + (threadIdx.x >> 6); q < p1; q += kBlock / 64)
            ilu0_row(perm[q], lane, rp, col, diag, W, bad);
        __syncthreads();
    }
}

}  // namespace spmv
