// spmv_bicgstab.hip -- spmv_hip_csr_bicgstab: BiCGSTAB on a CSR handle, entirely on the device (include/spmv_hip.h).
//
//     x = 0; r = r^ = p = b; rho = r^.r; rr0 = r.r
//     per step:  v = A p; alpha = rho / r^.v; s = r - alpha v; (s.s small: x += alpha p, r = s, stop)
//                t = A s; omega = t.s / t.t; x += alpha p + omega s; r = s - omega t; rho' = r^.r; rr = r.r
//                beta = (rho' / rho) (alpha / omega); rho = rho'; p = r + beta (p - omega v)
//
// The two products are the handle's SpMV (csr_launch_any) on library-owned p and s: full length with the 128-byte line
// tail the x-window kernels read, as the handle's own x.  v, t, x, r, r^ are indexed by global row; this rank works on
// its rows [row0, row0 + M_local).  The vector and scalar kernels are in bicgstab_kernels.hpp; the scalars and the stop
// state never leave the device.  With a communicator s and p are all-gathered with the row bounds after they are made
// (two exchanges per step) and every reduction is all-gathered and added in rank order, as csr_cg does: every rank
// holds the same bits and stops at the same step.
//
// spmv_hip_csr_pbicgstab runs the same loop right-preconditioned: p^ = M^-1 p and s^ = M^-1 s are the products' inputs
// (library-owned, all-gathered in place of p and s), x moves along them, and r stays the true residual.  Jacobi is
// fused into the s and p updates (bcg_jac_update_s / _p, with D^-1 copied to global row indexing so the 16-byte pieces
// line up); every other kind is a precond_apply after bcg_update_s / bcg_update_p: a pc_apply pass for block-Jacobi,
// the kind's own launches for the rest.  P = NULL takes the unpreconditioned path: exactly csr_bicgstab's launches.
#include "spmv_internal.hpp"

#include "bicgstab_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

struct BcgBuffers {
    void *p, *s, *v, *t, *x, *r, *rhat;
    void *ph, *sh, *dinv;  // with a preconditioner: M^-1 p, M^-1 s (the products' inputs), Jacobi's D^-1 by global row
    double *sc, *part, *gath, *hist;
    int *flags;
};

// the loop; *steps_run = the steps launched (< iters when tol > 0 and the solve stopped)
template <typename T>
int bcg_run(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, const int *bounds,
            const BcgBuffers &b, int *steps_run) {
    constexpr int V = 16 / sizeof(T);
    const long long lo = m->row0, hi = (long long)m->row0 + m->M_local;
    const int grid = solver_grid(kBcgBlocks, (hi + V - 1) / V - lo / V, kBlock);  // over the 16-byte pieces
    const double tol2 = tol * tol;
    T *p = (T *)b.p, *s = (T *)b.s, *v = (T *)b.v, *t = (T *)b.t, *x = (T *)b.x, *r = (T *)b.r, *rhat = (T *)b.rhat;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock);
    // part[0 .. grid) x nv of this rank -> the nv global sums in sc[slot ..] on every rank
    auto reduce = [&](int nv, int slot) {
        return solver_reduce(b.part, grid, nv, b.sc + slot, b.sc + kBcgLocal, b.gath, "csr_bicgstab");
    };
    // rho = r.r^, rr0 = r.r with r = r^ = b
    hipLaunchKernelGGL((bcg_dot2<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const T *)r, (const T *)rhat, b.part);
    if (reduce(2, kBcgRho)) return -1;
    hipLaunchKernelGGL(bcg_start, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hist, iters);
    // with P: the products read p^ and s^; Jacobi fuses into the updates, every other kind's apply follows them
    const bool jac = precond_path(P) == kPathJacobi;
    auto apply_after = [&](const T *in, T *out) { return P ? precond_apply<T>(P, in, out, fl, g_stream) : 0; };
    T *ph = P ? (T *)b.ph : p, *sh = P ? (T *)b.sh : s;
    const T *dinv = (const T *)b.dinv;
    const long long own = lo;  // P's local row 0 in the global vectors
    if (apply_after(p + own, ph + own)) return -1;  // p^ = M^-1 b (Jacobi too: the updates fuse it from step 1 on)
    if (g_comm && spmv_hip_comm_allgatherv(ph, bounds, m->value_bytes, g_stream)) return -1;
    *steps_run = iters;
    for (int k = 1; k <= iters; ++k) {
        if (csr_launch_any(m, variant, ph, v, g_stream)) return -1;  // v = A p (A p^) on this rank's rows
        hipLaunchKernelGGL((bcg_dot<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const T *)rhat, (const T *)v, b.part);
        if (reduce(1, kBcgRv)) return -1;
        hipLaunchKernelGGL(bcg_set_alpha, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, k);
        if (jac) {
            hipLaunchKernelGGL((bcg_jac_update_s<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)r, (const T *)v, dinv, s, sh, b.part);
        } else {
            hipLaunchKernelGGL((bcg_update_s<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)r, (const T *)v, s, b.part);
            if (apply_after(s + own, sh + own)) return -1;
        }
        if (reduce(1, kBcgSs)) return -1;
        hipLaunchKernelGGL(bcg_check_s, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, k, tol2);
        if (g_comm && spmv_hip_comm_allgatherv(sh, bounds, m->value_bytes, g_stream)) return -1;
        if (csr_launch_any(m, variant, sh, t, g_stream)) return -1;  // t = A s (A s^)
        hipLaunchKernelGGL((bcg_dot2<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const T *)t, (const T *)s, b.part);
        if (reduce(2, kBcgTs)) return -1;
        hipLaunchKernelGGL(bcg_set_omega, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, k);
        if (P)
            hipLaunchKernelGGL((bcg_pre_update_x_r<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)rhat, (const T *)ph, (const T *)sh, (const T *)s, (const T *)t, x, r, b.part);
        else
            hipLaunchKernelGGL((bcg_update_x_r<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)rhat, (const T *)p, (const T *)s, (const T *)t, x, r, b.part);
        if (reduce(2, kBcgRhoNew)) return -1;
        hipLaunchKernelGGL(bcg_set_beta, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hist, k, tol2);
        if (jac) {
            hipLaunchKernelGGL((bcg_jac_update_p<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)r, (const T *)v, dinv, p, ph);
        } else {
            hipLaunchKernelGGL((bcg_update_p<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const double *)b.sc,
                               (const T *)r, (const T *)v, p);
            if (apply_after(p + own, ph + own)) return -1;
        }
        if (g_comm && spmv_hip_comm_allgatherv(ph, bounds, m->value_bytes, g_stream)) return -1;
        bool stop = false;
        if (solver_poll(k, iters, tol, b.flags + kSolverState, kBcgStop, &stop)) return -1;
        if (stop) {
            *steps_run = k;
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int bcg_body(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, const int *bounds,
             const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total) {
    const size_t vb = sizeof(T), n_all = (size_t)m->M_total, n_own = (size_t)m->M_local;
    SolverScope scope;
    // p, s: SpMV inputs, read in whole 128-byte lines by the x-window kernels; the rest: whole 16-byte pieces
    const size_t in_bytes = ((size_t)m->N * vb + 15) / 16 * 16 + kLineBytes;
    const size_t vec_bytes = std::max<size_t>((n_all * vb + 15) / 16 * 16, 16);
    BcgBuffers b;
    b.p = scope.alloc(in_bytes);
    b.s = scope.alloc(in_bytes);
    b.v = scope.alloc(vec_bytes);
    b.t = scope.alloc(vec_bytes);
    b.x = scope.alloc(vec_bytes);
    b.r = scope.alloc(vec_bytes);
    b.rhat = scope.alloc(vec_bytes);
    b.sc = scope.alloc<double>(kBcgSlots * sizeof(double));
    b.part = scope.alloc<double>((size_t)kBcgBlocks * 2 * sizeof(double));
    b.gath = scope.alloc<double>((size_t)kMaxRanks * 2 * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    b.flags = scope.alloc<int>(kSolverFlagWords * sizeof(int));
    b.ph = b.sh = b.dinv = nullptr;
    if (P) {
        b.ph = scope.alloc(in_bytes);
        b.sh = scope.alloc(in_bytes);
        if (precond_path(P) == kPathJacobi) b.dinv = scope.alloc(vec_bytes);
    }
    // r = r^ = p = b on this rank's rows (the rest of p arrives by the all-gatherv)
    const size_t own_off = (size_t)m->row0 * vb, own_bytes = n_own * vb;
    hipError_t e = scope.err;
    if (e == hipSuccess && b.dinv && n_own)  // D^-1 by global row
        e = hipMemcpyAsync((char *)b.dinv + own_off, P->inv, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((char *)b.r + own_off, (const char *)b_host + own_off, own_bytes, hipMemcpyHostToDevice,
                           g_stream);
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((char *)b.rhat + own_off, (char *)b.r + own_off, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((char *)b.p + own_off, (char *)b.r + own_off, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (solver_begin(scope, e, "csr_bicgstab")) return -1;
    int steps_run = 0;
    if (bcg_run<T>(m, P, variant, iters, tol, bounds, b, &steps_run)) return -1;
    int flags[kSolverFlagWords] = {0, 0, 0, 0};
    if (solver_finish(scope, "csr_bicgstab", m->value_bytes, bounds, b.x, x_host, n_all * vb, {{rr_hist, b.hist}},
                      steps_run, iters, 1, b.flags, flags, kSolverFlagWords, ms_total))
        return -1;
    if (info) {
        info[0] = flags[kSolverSteps];
        info[1] = flags[kSolverStatus];
        info[2] = flags[kBcgHalf];
    }
    return 0;
}

int bcg_entry(const char *what, spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol,
              const int *bounds, const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total) {
    if (need_device()) return -1;
    if (!m || !b_host) return fail("%s: bad arguments", what);
    if (solver_check_steps(what, iters, tol) || solver_check_square(what, m) || solver_check_rows(what, m, bounds))
        return -1;
    if (P && precond_matches(m, P, what)) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return bcg_body<decltype(t)>(m, P, variant, iters, tol, bounds, b_host, x_host, rr_hist, info, ms_total);
    });
}

}  // namespace

extern "C" int spmv_hip_csr_bicgstab(spmv_csr_dev *m, int variant, int iters, double tol, const int *bounds,
                                     const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total) {
    return bcg_entry("csr_bicgstab", m, nullptr, variant, iters, tol, bounds, b_host, x_host, rr_hist, info, ms_total);
}

extern "C" int spmv_hip_csr_pbicgstab(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol,
                                      const int *bounds, const void *b_host, void *x_host, double *rr_hist, int *info,
                                      float *ms_total) {
    return bcg_entry("csr_pbicgstab", m, P, variant, iters, tol, bounds, b_host, x_host, rr_hist, info, ms_total);
}
