// gmres_kernels.hpp -- the vector and scalar kernels of spmv_hip_csr_gmres: restarted GMRES(m) (Saad and Schultz 1986)
// with classical Gram-Schmidt done twice (CGS2), right-preconditioned, x0 = 0 (gfx950).
//
// The basis is nvec vectors of n values of T, vector i at Vb + i ld (ld in elements, ld sizeof(T) a multiple of 16, so
// every vector starts on a 16-byte piece); the ld - n elements behind a vector are never read.  One Arnoldi step,
// after w = A M^-1 v_j (the handle's SpMV into the slot of v_{j+1}):
//
//   gmres_dots     h_i = v_i.w for i < nvec, eight vectors a trip                  nvec + ceil(nvec / 8) values per row
//   gmres_update   w = T(double(w) - sum_i h_i double(v_i)), optionally w.w        nvec + 2
//   gm_rotate      one wavefront: h = h + h', the rotations, g, the history, the stop rules
//   gm_scale       v_{j+1} = w / eta in place                                      2
//
// and per cycle gm_residual (r = b - q with r.r; 3), gm_cycle (beta = sqrt(r.r), g = beta e_0), gm_solve (R y = g,
// coefficients -y), gmres_update again for u = V y from a zeroed u, and gm_add (x += u; 3).
//
// gmres_dots runs on a grid of (workgroups over the pieces) x (tiles of NV vectors).  A workgroup reads its pieces of
// w once and of each of its tile's vectors once, the NV loads of a trip issued together, NV fp64 sums per lane.  Its
// partials go to part[g nvp + i] (nvp = nvec rounded up to NV; a vector past nvec gives 0) and are folded by
// solver_fold in workgroup order: the sum for one vector depends on n and the grid's x extent alone, not on nvec or on
// the tile it falls in.  The reduction order is that of solver_ops.hpp.
//
// flags: a solver's stop flags (solver_ops.hpp); any state but kSolverRun returns before writing.  NULL: none -- the
// passes exposed alone (spmv_hip_gmres_dots / _update) and the close of a cycle, which runs after a stop.
#pragma once
#include "solver_ops.hpp"

namespace spmv {

constexpr int kGmBlocks = 1024;    // grid cap of the vector kernels (the x extent of gmres_dots' grid)
constexpr int kGmMaxRestart = 64;  // widest basis the dots, the update and the scalar kernels take
constexpr int kGmTile = 8;         // NV: basis vectors per trip

// the scalar slots (doubles).  R is column-major with kGmMaxRestart rows a column.
constexpr int kGmRr = 0, kGmRr0 = 1, kGmWw = 2, kGmEta = 3, kGmBeta = 4, kGmLast = 5;
constexpr int kGmHa = 8, kGmHb = kGmHa + kGmMaxRestart, kGmG = kGmHb + kGmMaxRestart;
constexpr int kGmCs = kGmG + kGmMaxRestart + 8, kGmSn = kGmCs + kGmMaxRestart, kGmCoef = kGmSn + kGmMaxRestart;
constexpr int kGmLocal = kGmCoef + kGmMaxRestart, kGmR = kGmLocal + kGmMaxRestart;
constexpr int kGmSlots = kGmR + kGmMaxRestart * kGmMaxRestart;
// the int words: the stop flags of solver_ops.hpp, word 3 = the stop came from b itself, before the first cycle
constexpr int kGmAtStart = 3;

__device__ __forceinline__ bool gm_stopped(const int *__restrict__ flags) {
    return flags && flags[kSolverState] != kSolverRun;
}

// one trip of gmres_dots: the lane's piece of w against the pieces of cnt <= NV vectors from vb on
template <typename T, int V, int NV, bool FULL>
__device__ __forceinline__ void gm_dots_trip(const T *__restrict__ vb, long long ld, int cnt, long long i0, long long n,
                                             const T (&wv)[V], double (&acc)[NV]) {
    T bv[NV][V];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (FULL || j < cnt) {
            piece_load<T, V>(vb + j * ld, i0, 0, n, bv[j]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) bv[j][e] = T(0);
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[j] += (double)bv[j][e] * (double)wv[e];
}

// partials of v_i.w, i in [NV blockIdx.y, NV blockIdx.y + NV), on rows [0, n): part[blockIdx.x nvp + i]
template <typename T, int V, int NV = kGmTile>
__global__ __launch_bounds__(kBlock) void gmres_dots(long long n, const int *__restrict__ flags,
                                                     const T *__restrict__ Vb, long long ld, int nvec,
                                                     const T *__restrict__ w, double *__restrict__ part) {
    if (gm_stopped(flags)) return;
    const int first = (int)blockIdx.y * NV, cnt = min(NV, nvec - first), nvp = (nvec + NV - 1) / NV * NV;
    const T *vb = Vb + (long long)first * ld;
    double acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T wv[V];
        piece_load<T, V>(w, i0, 0, n, wv);
        if (cnt == NV) gm_dots_trip<T, V, NV, true>(vb, ld, cnt, i0, n, wv, acc);
        else gm_dots_trip<T, V, NV, false>(vb, ld, cnt, i0, n, wv, acc);
    }
    // block_partials writes part[blockIdx.x NV + j]: shifted to row blockIdx.x of nvp sums, column first + j
    block_partials<NV>(acc, part + first + (long long)blockIdx.x * (nvp - NV));
}

// one trip of gmres_update: s += h_j v_j for the cnt <= NV vectors from vb on, in index order
template <typename T, int V, int NV, bool FULL>
__device__ __forceinline__ void gm_update_trip(const T *__restrict__ vb, long long ld, int cnt,
                                               const double *__restrict__ h, long long i0, long long n,
                                               double (&s)[V]) {
    T bv[NV][V];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (FULL || j < cnt) {
            piece_load<T, V>(vb + j * ld, i0, 0, n, bv[j]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) bv[j][e] = T(0);
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (FULL || j < cnt) {
            const double hj = h[j];  // wave-uniform
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] += hj * (double)bv[j][e];
        }
    }
}

// w = T(double(w) - sum_i h_i double(v_i)) on rows [0, n), the terms added for i = 0 .. nvec - 1 in double and the
// result rounded once; part != NULL: the workgroup's partial of w.w of what was stored
template <typename T, int V, int NV = kGmTile>
__global__ __launch_bounds__(kBlock) void gmres_update(long long n, const int *__restrict__ flags,
                                                       const T *__restrict__ Vb, long long ld, int nvec,
                                                       const double *__restrict__ h, T *__restrict__ w,
                                                       double *__restrict__ part) {
    if (gm_stopped(flags)) return;
    double acc[1] = {0.0};
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T wv[V];
        piece_load<T, V>(w, i0, 0, n, wv);
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        for (int first = 0; first < nvec; first += NV) {
            const int cnt = min(NV, nvec - first);
            const T *vb = Vb + (long long)first * ld;
            if (cnt == NV) gm_update_trip<T, V, NV, true>(vb, ld, cnt, h + first, i0, n, s);
            else gm_update_trip<T, V, NV, false>(vb, ld, cnt, h + first, i0, n, s);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            wv[e] = (T)((double)wv[e] - s[e]);
            // a piece cut by n holds zeros behind row n - 1 (piece_load), and 0 - 0 adds nothing
            acc[0] += (double)wv[e] * (double)wv[e];
        }
        piece_store<T, V>(w, i0, 0, n, wv);
    }
    if (part) block_partials<1>(acc, part);
}

// r = b - q on rows [0, n), partials of r.r
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void gm_residual(long long n, const int *__restrict__ flags,
                                                      const T *__restrict__ b, const T *__restrict__ q,
                                                      T *__restrict__ r, double *__restrict__ part) {
    if (gm_stopped(flags)) return;
    double acc[1] = {0.0};
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T bv[V], qv[V];
        piece_load<T, V>(b, i0, 0, n, bv);
        piece_load<T, V>(q, i0, 0, n, qv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            bv[e] = (T)((double)bv[e] - (double)qv[e]);
            acc[0] += (double)bv[e] * (double)bv[e];
        }
        piece_store<T, V>(r, i0, 0, n, bv);
    }
    block_partials<1>(acc, part);
}

// v = v / *div on rows [0, n), in place: a division, not a product with the reciprocal
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void gm_scale(long long n, const int *__restrict__ flags,
                                                   const double *__restrict__ div, T *__restrict__ v) {
    if (gm_stopped(flags)) return;
    const double d = *div;
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T vv[V];
        piece_load<T, V>(v, i0, 0, n, vv);
#pragma unroll
        for (int e = 0; e < V; ++e) vv[e] = (T)((double)vv[e] / d);
        piece_store<T, V>(v, i0, 0, n, vv);
    }
}

// x += u on rows [0, n) (the close of a cycle: no flags)
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void gm_add(long long n, const T *__restrict__ u, T *__restrict__ x) {
    for (PieceLane l(0, n, V); l.q < l.end; l.q += l.stride) {
        const long long i0 = l.q * V;
        T uv[V], xv[V];
        piece_load<T, V>(u, i0, 0, n, uv);
        piece_load<T, V>(x, i0, 0, n, xv);
#pragma unroll
        for (int e = 0; e < V; ++e) xv[e] = (T)((double)xv[e] + (double)uv[e]);
        piece_store<T, V>(x, i0, 0, n, xv);
    }
}

// ---- the scalar kernels.  A stop (solver_stop) writes the status and the steps counted and never touches x.

// rr0 = b.b (slot kGmRr, the first cycle's r.r), history row 0; rr0 = 0 converges at step 0, a non-finite rr0 breaks down
__global__ void gm_start(double *__restrict__ sc, int *__restrict__ flags, double *__restrict__ hist, int iters) {
    const double rr0 = sc[kGmRr];
    sc[kGmRr0] = rr0;
    sc[kGmLast] = rr0;
    hist[0] = rr0;
    flags[kSolverState] = kSolverRun;
    flags[kSolverSteps] = iters;
    flags[kSolverStatus] = SPMV_GMRES_RAN_ALL;
    flags[kGmAtStart] = rr0 == 0.0 || !isfinite(rr0);
    if (rr0 == 0.0) solver_stop(flags, SPMV_GMRES_CONVERGED, 0);
    else if (!isfinite(rr0)) solver_stop(flags, SPMV_GMRES_BREAKDOWN, 0);
}

// the start of a cycle after t steps: beta = sqrt(r.r) (slot kGmBeta, v_0 = r / beta follows), g = (beta, 0, ..., 0)
__global__ void gm_cycle(double *__restrict__ sc, int *__restrict__ flags, int t) {
    if (flags[kSolverState] != kSolverRun) return;
    const double beta = sqrt(sc[kGmRr]);
    if (!isfinite(beta)) {
        solver_stop(flags, SPMV_GMRES_BREAKDOWN, t);
        return;
    }
    if (beta == 0.0) {
        solver_stop(flags, SPMV_GMRES_CONVERGED, t);
        return;
    }
    sc[kGmBeta] = beta;
    sc[kGmG] = beta;
    for (int i = 1; i <= kGmMaxRestart; ++i) sc[kGmG + i] = 0.0;
}

// Column j of a cycle, step t (1-based) of the solve.  The lanes add the two passes' coefficients, h = h + h'; lane 0
// applies the rotations 0 .. j - 1 to (h_0 .. h_j, eta = sqrt(w.w)), makes rotation j from d = hypot(h_j, eta), keeps
// the column of R, turns g and writes history row t.  d = 0 or anything not finite breaks down with t - 1 steps
// counted; g_{j+1}^2 <= tol2 rr0 converges with t.  eta stays in slot kGmEta for gm_scale.
__global__ __launch_bounds__(64) void gm_rotate(double *__restrict__ sc, int *__restrict__ flags,
                                                double *__restrict__ hist, int j, int t, double tol2) {
    if (flags[kSolverState] != kSolverRun) {
        if (threadIdx.x == 0) hist[t] = sc[kGmLast];
        return;
    }
    double *col = sc + kGmR + j * kGmMaxRestart;
    if ((int)threadIdx.x <= j) col[threadIdx.x] = sc[kGmHa + threadIdx.x] + sc[kGmHb + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double eta = sqrt(sc[kGmWw]);
    bool ok = isfinite(eta);
    for (int i = 0; i <= j; ++i) ok = ok && isfinite(col[i]);
    for (int i = 0; i < j; ++i) {
        const double c = sc[kGmCs + i], s = sc[kGmSn + i], a = col[i], b = col[i + 1];
        col[i] = c * a + s * b;
        col[i + 1] = -s * a + c * b;
    }
    const double hj = col[j], d = hypot(hj, eta);
    const double c = hj / d, s = eta / d, gj = sc[kGmG + j], gn = -s * gj, rr = gn * gn;
    for (int i = 0; i <= j; ++i) ok = ok && isfinite(col[i]);
    if (!ok || d == 0.0 || !isfinite(d) || !isfinite(c) || !isfinite(s) || !isfinite(gn) || !isfinite(rr)) {
        solver_stop(flags, SPMV_GMRES_BREAKDOWN, t - 1);
        hist[t] = sc[kGmLast];
        return;
    }
    col[j] = d;
    sc[kGmCs + j] = c;
    sc[kGmSn + j] = s;
    sc[kGmG + j] = c * gj;
    sc[kGmG + j + 1] = gn;
    sc[kGmEta] = eta;
    sc[kGmLast] = rr;
    hist[t] = rr;
    if (rr <= tol2 * sc[kGmRr0]) solver_stop(flags, SPMV_GMRES_CONVERGED, t);
}

// the close of a cycle with J counted columns: R y = g by back substitution, coefficients -y for gmres_update
__global__ void gm_solve(double *__restrict__ sc, int J) {
    double *y = sc + kGmCoef;
    for (int i = J - 1; i >= 0; --i) {
        double s = sc[kGmG + i];
        for (int k = i + 1; k < J; ++k) s -= sc[kGmR + k * kGmMaxRestart + i] * -y[k];
        y[i] = -(s / sc[kGmR + i * kGmMaxRestart + i]);
    }
}

}  // namespace spmv
