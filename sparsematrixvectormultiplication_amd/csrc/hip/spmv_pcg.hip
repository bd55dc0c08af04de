// spmv_pcg.hip -- spmv_hip_csr_pcg: preconditioned conjugate gradients on a CSR handle, entirely on the device
// (include/spmv_hip.h).
//
//     r = b; z = M^-1 r; p = z; rz = r.z; rr0 = r.r
//     per step:  q = A p; alpha = rz / p.q; x += alpha p; r -= alpha q; z = M^-1 r; rz' = r.z; rr = r.r
//                (rr <= tol^2 rr0: stop); beta = rz' / rz; p = z + beta p
//
// The layout and the walk are csr_cg's: p is the handle's x (all-gathered with the bounds when a communicator exists),
// q its y, x / r / z hold this rank's rows at local index, the lanes walk single rows (PieceLane with V = 1) on
// csr_cg's grid, and the dots fold as csr_cg's do.  That is what makes P = NULL (z is r) and Jacobi with a unit
// diagonal give csr_cg's bits.  The paths of the x / r update (precond_path):
//
//   NONE    x += alpha p, r -= alpha q, partials of r.r twice (z is r)                    6 values moved per row
//   JACOBI  the same and z = D^-1 r (one more read, one more write), partials of r.r, r.z  8
//   BLOCK   x += alpha p, r -= alpha q (6), then pc_apply: z = M^-1 r with r.r and r.z    b + 2 more (L2 serves r's
//           repeats inside a block)
//   OWN     x += alpha p, r -= alpha q (6), then the kind's own launches -- SSOR's / ILU(0)'s two solves (spmv_trsv.hip),
//           FSAI's two SpMVs (spmv_fsai.hip), AMG's V-cycle (spmv_amg.hip), CHEBYSHEV's passes (spmv_cheb.hip) --, then
//           pcg_dots: r.r and r.z by the walk and the fold of the other paths (2 more reads); the solves' last kernel is
//           a level of a few rows and the other kinds' launches are handles' own, so the dots are a pass of their own
//
// pcg_dot (p.q, 2 values) and pcg_update_p (p = z + beta p, 3) complete the step: fp64 Jacobi PCG moves 13 values =
// 104 B per row against csr_cg's 11 (88 B).  The scalars and the stop state never leave the device; after a stop the
// vector kernels return before they write, so a stopped solve can go on being launched with x untouched (tol = 0).
#include "spmv_internal.hpp"

#include "precond_kernels.hpp"

namespace {

// the scalar slots (doubles); two-value reductions land in adjacent slots: (Rr, Rz), (RrNew, RzNew)
constexpr int kPcgRr = 0, kPcgRz = 1, kPcgPq = 2, kPcgRrNew = 3, kPcgRzNew = 4, kPcgAlpha = 5, kPcgBeta = 6,
              kPcgRr0 = 7, kPcgLastRr = 8, kPcgLastRz = 9, kPcgLocal = 10, kPcgSlots = 16;
// the int words: the stop flags of solver_ops.hpp

// partials of a.b on [0, n): dot_partial of spmv_cg.hip with the stop check
template <typename T>
__global__ __launch_bounds__(kBlock) void pcg_dot(long long n, const int *__restrict__ flags, const T *__restrict__ a,
                                                  const T *__restrict__ b, double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    double acc[1] = {0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) acc[0] += (double)a[l.q] * (double)b[l.q];
    block_partials<1>(acc, part);
}

// partials of r.r and r.z after an apply that made none (flags NULL: at the start)
template <typename T>
__global__ __launch_bounds__(kBlock) void pcg_dots(long long n, const int *__restrict__ flags, const T *__restrict__ r,
                                                   const T *__restrict__ z, double *__restrict__ part) {
    if (flags && flags[kSolverState] != kSolverRun) return;
    double acc[2] = {0.0, 0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) {
        const double rk = (double)r[l.q];
        acc[0] += rk * rk;
        acc[1] += rk * (double)z[l.q];
    }
    block_partials<2>(acc, part);
}

// at the start: partials of r.r and r.z; JAC: z = D^-1 r first (else z is r)
template <typename T, bool JAC>
__global__ __launch_bounds__(kBlock) void pcg_start_dots(long long n, const T *__restrict__ dinv,
                                                         const T *__restrict__ r, T *__restrict__ z,
                                                         double *__restrict__ part) {
    double acc[2] = {0.0, 0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) {
        const long long k = l.q;
        const T rk = r[k];
        T zk = rk;
        if constexpr (JAC) {
            zk = (T)((double)dinv[k] * (double)rk);
            z[k] = zk;
        }
        acc[0] += (double)rk * (double)rk;
        acc[1] += (double)rk * (double)zk;
    }
    block_partials<2>(acc, part);
}

// x += alpha p, r -= alpha q on this rank's rows; NONE: partials of r.r (twice), JACOBI: z = D^-1 r and partials of
// r.r, r.z, BLOCK: no partials (pc_apply makes them)
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void pcg_update_x_r(long long n, const int *__restrict__ flags,
                                                         const double *__restrict__ s, const T *__restrict__ p,
                                                         const T *__restrict__ q, const T *__restrict__ dinv,
                                                         T *__restrict__ x, T *__restrict__ r, T *__restrict__ z,
                                                         double *__restrict__ part) {
    if (flags[kSolverState] != kSolverRun) return;
    const double alpha = s[kPcgAlpha];
    double acc[2] = {0.0, 0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) {
        const long long k = l.q;
        x[k] = (T)((double)x[k] + alpha * (double)p[k]);
        const T rk = (T)((double)r[k] - alpha * (double)q[k]);
        r[k] = rk;
        if constexpr (MODE == kPathNone) {
            acc[0] += (double)rk * (double)rk;
            acc[1] = acc[0];
        } else if constexpr (MODE == kPathJacobi) {
            const T zk = (T)((double)dinv[k] * (double)rk);
            z[k] = zk;
            acc[0] += (double)rk * (double)rk;
            acc[1] += (double)rk * (double)zk;
        }
    }
    if constexpr (MODE != kPathBlock) block_partials<2>(acc, part);
}

// p = z + beta p on this rank's rows
template <typename T>
__global__ __launch_bounds__(kBlock) void pcg_update_p(long long n, const int *__restrict__ flags,
                                                       const double *__restrict__ s, const T *__restrict__ z,
                                                       T *__restrict__ p) {
    if (flags[kSolverState] != kSolverRun) return;
    const double beta = s[kPcgBeta];
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) p[l.q] = (T)((double)z[l.q] + beta * (double)p[l.q]);
}

// ---- the scalar kernels: one thread each.  A stop (solver_stop) writes the status and the steps taken and never
// touches x.
// rr0 = r.r, rz = r.z, history row 0; rr0 = 0 converges at step 0; rz <= 0 or anything not finite breaks down there
__global__ void pcg_start(double *__restrict__ s, int *__restrict__ flags, double *__restrict__ hrr,
                          double *__restrict__ hrz, int iters) {
    const double rr0 = s[kPcgRr], rz = s[kPcgRz];
    s[kPcgRr0] = rr0;
    s[kPcgLastRr] = rr0;
    s[kPcgLastRz] = rz;
    hrr[0] = rr0;
    hrz[0] = rz;
    flags[kSolverState] = kSolverRun;
    flags[kSolverSteps] = iters;
    flags[kSolverStatus] = SPMV_PCG_RAN_ALL;
    if (rr0 == 0.0) solver_stop(flags, SPMV_PCG_CONVERGED, 0);
    else if (!(rz > 0.0) || !isfinite(rz) || !isfinite(rr0)) solver_stop(flags, SPMV_PCG_BREAKDOWN, 0);
}

// step t: alpha = rz / p.q; p.q <= 0 or anything not finite breaks down (step t not taken)
__global__ void pcg_set_alpha(double *__restrict__ s, int *__restrict__ flags, int t) {
    if (flags[kSolverState] != kSolverRun) return;
    const double pq = s[kPcgPq], alpha = s[kPcgRz] / pq;
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {
        solver_stop(flags, SPMV_PCG_BREAKDOWN, t - 1);
        return;
    }
    s[kPcgAlpha] = alpha;
}

// end of step t: history row t; a non-finite rr or rz' breaks down, rr <= tol2 rr0 converges, rz' <= 0 breaks down
// (x is the iterate of step t); else beta = rz' / rz, rz = rz'
__global__ void pcg_set_beta(double *__restrict__ s, int *__restrict__ flags, double *__restrict__ hrr,
                             double *__restrict__ hrz, int t, double tol2) {
    if (flags[kSolverState] != kSolverRun) {
        hrr[t] = s[kPcgLastRr];
        hrz[t] = s[kPcgLastRz];
        return;
    }
    const double rr = s[kPcgRrNew], rz = s[kPcgRzNew];
    s[kPcgLastRr] = rr;
    s[kPcgLastRz] = rz;
    hrr[t] = rr;
    hrz[t] = rz;
    if (!isfinite(rr) || !isfinite(rz)) {
        solver_stop(flags, SPMV_PCG_BREAKDOWN, t);
        return;
    }
    if (rr <= tol2 * s[kPcgRr0]) {
        solver_stop(flags, SPMV_PCG_CONVERGED, t);
        return;
    }
    if (!(rz > 0.0)) {
        solver_stop(flags, SPMV_PCG_BREAKDOWN, t);
        return;
    }
    s[kPcgBeta] = rz / s[kPcgRz];
    s[kPcgRz] = rz;
}

struct PcgBuffers {
    void *x, *r, *z;  // x: M_total values (the all-gatherv's), r, z: this rank's rows (z is r without P)
    double *sc, *part, *gath, *hrr, *hrz;
    int *flags;
};

int pcg_exchange_p(spmv_csr_dev *m, const int *bounds) {
    if (!g_comm) return 0;
    return spmv_hip_comm_allgatherv(m->x, bounds, m->value_bytes, g_stream);
}

// the loop; *steps_run = the steps launched (< iters when tol > 0 and the solve stopped)
template <typename T>
int pcg_run(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, const int *bounds,
            const PcgBuffers &b, int *steps_run) {
    const long long n = m->M_local;
    const int grid = solver_grid(kNormBlocks, n, kBlock);
    const PrecondPath mode = precond_path(P);
    const double tol2 = tol * tol;
    T *p_own = (T *)m->x + m->row0, *q_own = (T *)m->y + m->row0, *x_own = (T *)b.x + m->row0;
    T *r = (T *)b.r, *z = (T *)b.z;
    const T *dinv = P ? (const T *)P->inv : nullptr;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock);
    auto reduce = [&](int nv, int slot) {
        return solver_reduce(b.part, grid, nv, b.sc + slot, b.sc + kPcgLocal, b.gath, "csr_pcg");
    };
    // z = M^-1 r, rr0 = r.r, rz = r.z with r = b; p = z (the own range of the handle's x; the rest by the exchange)
    if (mode == kPathNone)
        hipLaunchKernelGGL((pcg_start_dots<T, false>), g, blk, 0, g_stream, n, dinv, (const T *)r, z, b.part);
    else if (mode == kPathJacobi)
        hipLaunchKernelGGL((pcg_start_dots<T, true>), g, blk, 0, g_stream, n, dinv, (const T *)r, z, b.part);
    else if (mode == kPathBlock)
        precond_launch<T, true>(P, r, z, nullptr, b.part, grid, g_stream);
    else {
        if (P->family->apply(P, r, z, nullptr, g_stream)) return -1;
        hipLaunchKernelGGL((pcg_dots<T>), g, blk, 0, g_stream, n, (const int *)nullptr, (const T *)r, (const T *)z, b.part);
    }
    if (reduce(2, kPcgRr)) return -1;
    hipLaunchKernelGGL(pcg_start, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hrr, b.hrz, iters);
    if (n) HIP_TRY(hipMemcpyAsync(p_own, z, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, g_stream));
    if (pcg_exchange_p(m, bounds)) return -1;
    *steps_run = iters;
    for (int t = 1; t <= iters; ++t) {
        if (csr_launch_any(m, variant, m->x, m->y, g_stream)) return -1;  // q = A p on this rank's rows
        hipLaunchKernelGGL((pcg_dot<T>), g, blk, 0, g_stream, n, fl, (const T *)p_own, (const T *)q_own, b.part);
        if (reduce(1, kPcgPq)) return -1;
        hipLaunchKernelGGL(pcg_set_alpha, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, t);
        if (mode == kPathNone) {
            hipLaunchKernelGGL((pcg_update_x_r<T, kPathNone>), g, blk, 0, g_stream, n, fl, (const double *)b.sc,
                               (const T *)p_own, (const T *)q_own, dinv, x_own, r, z, b.part);
        } else if (mode == kPathJacobi) {
            hipLaunchKernelGGL((pcg_update_x_r<T, kPathJacobi>), g, blk, 0, g_stream, n, fl, (const double *)b.sc,
                               (const T *)p_own, (const T *)q_own, dinv, x_own, r, z, b.part);
        } else {
            hipLaunchKernelGGL((pcg_update_x_r<T, kPathBlock>), g, blk, 0, g_stream, n, fl, (const double *)b.sc,
                               (const T *)p_own, (const T *)q_own, dinv, x_own, r, z, b.part);
            if (mode == kPathBlock) {
                precond_launch<T, true>(P, r, z, fl, b.part, grid, g_stream);
            } else {
                if (P->family->apply(P, r, z, fl, g_stream)) return -1;
                hipLaunchKernelGGL((pcg_dots<T>), g, blk, 0, g_stream, n, fl, (const T *)r, (const T *)z, b.part);
            }
        }
        if (reduce(2, kPcgRrNew)) return -1;
        hipLaunchKernelGGL(pcg_set_beta, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hrr, b.hrz, t, tol2);
        hipLaunchKernelGGL((pcg_update_p<T>), g, blk, 0, g_stream, n, fl, (const double *)b.sc, (const T *)z, p_own);
        if (pcg_exchange_p(m, bounds)) return -1;
        bool stop = false;
        if (solver_poll(t, iters, tol, b.flags + kSolverState, kSolverStop, &stop)) return -1;
        if (stop) {
            *steps_run = t;
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int pcg_body(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, const int *bounds,
             const void *b_host, void *x_host, double *rr_hist, double *rz_hist, int *info, float *ms_total) {
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local, vb = sizeof(T);
    SolverScope scope;
    PcgBuffers b;
    b.x = scope.alloc(std::max<size_t>(n_all, 1) * vb);
    b.r = scope.alloc(std::max<size_t>(n_own, 1) * vb);
    b.z = P ? scope.alloc(std::max<size_t>(n_own, 1) * vb) : b.r;
    b.sc = scope.alloc<double>(kPcgSlots * sizeof(double));
    b.part = scope.alloc<double>((size_t)kNormBlocks * 2 * sizeof(double));
    b.gath = scope.alloc<double>((size_t)kMaxRanks * 2 * sizeof(double));
    b.hrr = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    b.hrz = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    b.flags = scope.alloc<int>(kSolverFlagWords * sizeof(int));
    // r = b on this rank's rows; the handle's x (p) starts at 0 (its own range is set to z by the loop)
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(b.r, (const T *)b_host + m->row0, n_own * vb, hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->x, 0, (size_t)m->N * vb, g_stream);
    if (solver_begin(scope, e, "csr_pcg")) return -1;
    int steps_run = 0;
    if (pcg_run<T>(m, P, variant, iters, tol, bounds, b, &steps_run)) return -1;
    int flags[kSolverFlagWords] = {0, 0, 0, 0};
    if (solver_finish(scope, "csr_pcg", m->value_bytes, bounds, b.x, x_host, n_all * vb,
                      {{rr_hist, b.hrr}, {rz_hist, b.hrz}}, steps_run, iters, 1, b.flags, flags, kSolverFlagWords, ms_total))
        return -1;
    if (info) {
        info[0] = flags[kSolverSteps];
        info[1] = flags[kSolverStatus];
    }
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_pcg(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol,
                                const int *bounds, const void *b_host, void *x_host, double *rr_hist, double *rz_hist,
                                int *info, float *ms_total) {
    if (need_device()) return -1;
    const char *what = "csr_pcg";
    if (!m || !b_host) return fail("%s: bad arguments", what);
    if (solver_check_steps(what, iters, tol) || solver_check_square(what, m) || solver_check_rows(what, m, bounds))
        return -1;
    if (P && precond_matches(m, P, what)) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return pcg_body<decltype(t)>(m, P, variant, iters, tol, bounds, b_host, x_host, rr_hist, rz_hist, info, ms_total);
    });
}
