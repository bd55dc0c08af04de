// spmv_bicgstab_multi.hip -- spmv_hip_csr_bicgstab_multi: k independent right-preconditioned BiCGSTAB recurrences on a
// CSR handle that share the two SpMMs of a step and the k-wide preconditioner apply (include/spmv_hip.h; the kernels
// are in bicgstab_multi_kernels.hpp).
//
//     X = 0; R = R^ = P = B; P^ = M^-1 P; rho_j = rr0_j = r_j.r_j
//     per step:  V = A P^ (one SpMM); alpha_j = rho_j / r^_j.v_j; s_j = r_j - alpha_j v_j; S^ = M^-1 S;
//                (s_j.s_j small: x_j += alpha_j p^_j, r_j = s_j, column j stops)
//                T = A S^ (one SpMM); omega_j = t_j.s_j / t_j.t_j; x_j += alpha_j p^_j + omega_j s^_j;
//                r_j = s_j - omega_j t_j; rho'_j = r^_j.r_j; rr_j = r_j.r_j;
//                beta_j = (rho'_j / rho_j) (alpha_j / omega_j); rho_j = rho'_j; p_j = r_j + beta_j (p_j - omega_j v_j);
//                P^ = M^-1 P
//
// The loop of csr_pbicgstab with the layout of csr_cg_multi.  P^ and S^ (N x k, the SpMMs' inputs, all-gathered with
// the bounds scaled by k when a communicator exists), V, T and X (M_total x k), R, R^, S and P (this rank's rows) are
// row-major.  Without a preconditioner P^ is P and S^ is S: the products read the buffers the updates write.  The
// paths of the s and p updates (precond_path):
//
//   NONE    the updates write the SpMMs' inputs
//   JACOBI  s^ = D^-1 s and p^ = D^-1 p fused into the updates
//   BLOCK, OWN   the update, then the k-wide apply through spmv_hip_precond_apply_multi_on: mpc_apply without dots for
//           block-Jacobi, the family's launches for FSAI, AMG and CHEBYSHEV
//
// A kind without a k-wide apply is refused (precond_refuse_one_wide).  Every column carries its own scalars, state,
// steps, status and half-step flag on the device; a stopped column still rides in the SpMMs and the applies and keeps
// x, r, s and p.
#include "spmv_internal.hpp"

#include "bicgstab_multi_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

struct MbcgBuffers {
    // ph, sh: the SpMMs' inputs; without a preconditioner p and s are their own ranges
    void *ph, *sh, *p, *s, *v, *t, *x, *r, *rhat, *work;
    double *sc, *part0, *part1, *gath, *hist;
    int *flags;
};

// the loop; V = values of T per lane.  *steps = the steps run (< iters when tol > 0 and every column stopped)
template <typename T, int V>
int mbcg_run(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const int *kbounds,
             const MbcgBuffers &b, int *steps) {
    const char *what = "csr_bicgstab_multi";
    const long long n = m->M_local, kk = k, own = m->row0 * kk;
    const int cl = mcg_column_lanes(k, V);
    const int grid = solver_grid(kMcgBlocks, n, kBlock >> cl);
    const PrecondPath path = precond_path(pc);
    const double tol2 = tol * tol;
    T *PH = (T *)b.ph, *SH = (T *)b.sh, *ph_own = PH + own, *sh_own = SH + own;
    T *p = (T *)b.p, *s = (T *)b.s, *x_own = (T *)b.x + own, *r = (T *)b.r;
    const T *v_own = (const T *)b.v + own, *t_own = (const T *)b.t + own, *rhat = (const T *)b.rhat;
    const T *dinv = path == kPathJacobi ? (const T *)pc->inv : nullptr;
    const double *sc = b.sc;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock), one(1), wave(64);
    // one plane of part[0 .. grid) x k of this rank -> the k global sums in slot `slot` of b.sc on every rank
    auto reduce = [&](const double *part, int slot) {
        return solver_reduce(part, grid, k, b.sc + (size_t)slot * kMcgMaxK, b.sc + (size_t)kMbcgLocal * kMcgMaxK, b.gath, what);
    };
    // out = M^-1 in on this rank's rows, for the kinds that do not fuse into the updates
    auto apply = [&](const T *in, T *out) { return spmv_hip_precond_apply_multi_on(pc, k, in, out, b.work, g_stream); };
    // rr0 = r.r with R = R^ = P = B; P^ = M^-1 B (Jacobi too: the updates fuse it from step 1 on)
    hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, (const T *)r, (const T *)r, n, k, cl, b.part0);
    if (reduce(b.part0, kMbcgRr0)) return -1;
    hipLaunchKernelGGL(mbcg_start, one, wave, 0, g_stream, b.sc, b.flags, b.hist, k, iters);
    if (pc && apply(p, ph_own)) return -1;
    if (g_comm && spmv_hip_comm_allgatherv(PH, kbounds, m->value_bytes, g_stream)) return -1;
    *steps = iters;
    for (int t = 1; t <= iters; ++t) {
        if (spmv_hip_csr_spmm_on(m, k, PH, b.v, g_stream)) return -1;  // V = A P^ on this rank's rows
        hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, rhat, v_own, n, k, cl, b.part0);
        if (reduce(b.part0, kMbcgRv)) return -1;
        hipLaunchKernelGGL(mbcg_set_alpha, one, wave, 0, g_stream, b.sc, b.flags, k, t);
        if (path == kPathNone) {
            hipLaunchKernelGGL((mbcg_update_s<T, V, kMbcgNone>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, s, sh_own, b.part0);
        } else if (path == kPathJacobi) {
            hipLaunchKernelGGL((mbcg_update_s<T, V, kMbcgJacobi>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, s, sh_own, b.part0);
        } else {
            hipLaunchKernelGGL((mbcg_update_s<T, V, kMbcgApply>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, s, sh_own, b.part0);
            if (apply(s, sh_own)) return -1;
        }
        if (reduce(b.part0, kMbcgSs)) return -1;
        hipLaunchKernelGGL(mbcg_check_s, one, wave, 0, g_stream, sc, b.flags, k, t, tol2);
        if (g_comm && spmv_hip_comm_allgatherv(SH, kbounds, m->value_bytes, g_stream)) return -1;
        if (spmv_hip_csr_spmm_on(m, k, SH, b.t, g_stream)) return -1;  // T = A S^
        hipLaunchKernelGGL((mbcg_dot2<T, V>), g, blk, 0, g_stream, n, k, cl, t_own, (const T *)s, b.part0, b.part1);
        if (reduce(b.part0, kMbcgTs) || reduce(b.part1, kMbcgTt)) return -1;
        hipLaunchKernelGGL(mbcg_set_omega, one, wave, 0, g_stream, b.sc, b.flags, k, t);
        if (pc)
            hipLaunchKernelGGL((mbcg_update_x_r<T, V, true>), g, blk, 0, g_stream, n, k, cl, sc, fl, rhat, (const T *)ph_own,
                               (const T *)sh_own, (const T *)s, t_own, x_own, r, b.part0, b.part1);
        else
            hipLaunchKernelGGL((mbcg_update_x_r<T, V, false>), g, blk, 0, g_stream, n, k, cl, sc, fl, rhat, (const T *)ph_own,
                               (const T *)sh_own, (const T *)s, t_own, x_own, r, b.part0, b.part1);
        if (reduce(b.part0, kMbcgRhoNew) || reduce(b.part1, kMbcgRr)) return -1;
        hipLaunchKernelGGL(mbcg_set_beta, one, wave, 0, g_stream, b.sc, b.flags, b.hist + (size_t)t * kk, k, t, tol2);
        if (path == kPathNone) {
            hipLaunchKernelGGL((mbcg_update_p<T, V, kMbcgNone>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, p, ph_own);
        } else if (path == kPathJacobi) {
            hipLaunchKernelGGL((mbcg_update_p<T, V, kMbcgJacobi>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, p, ph_own);
        } else {
            hipLaunchKernelGGL((mbcg_update_p<T, V, kMbcgApply>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r, v_own,
                               dinv, p, ph_own);
            if (apply(p, ph_own)) return -1;
        }
        if (g_comm && spmv_hip_comm_allgatherv(PH, kbounds, m->value_bytes, g_stream)) return -1;
        bool stop = false;  // every column stopped
        if (solver_poll(t, iters, tol, b.flags + kMcgActive, 0, &stop)) return -1;
        if (stop) {
            *steps = t;
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int mbcg_body(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const int *bounds,
              const void *B_host, void *X_host, double *rr_hist, int *steps_out, int *status_out, int *half_out,
              float *ms_total) {
    const char *what = "csr_bicgstab_multi";
    const size_t kk = (size_t)k, vb = sizeof(T);
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local, ncols = (size_t)m->N;
    const std::vector<int> kbounds = solver_scaled_bounds(bounds, k);
    SolverScope scope;
    // what feeds a product at k = 1 is read in whole 128-byte lines by the x-window SpMV kernels: P^ and S^ by A, and
    // with a family's apply S and P by its first product (FSAI's G)
    const size_t in_bytes = std::max<size_t>(ncols * kk * vb, 16) + kLineBytes;
    const size_t out_bytes = std::max<size_t>(n_all * kk * vb, 16);
    const size_t own_off = (size_t)m->row0 * kk * vb, own_bytes = n_own * kk * vb;
    const size_t r_bytes = std::max<size_t>(own_bytes, 16) + kLineBytes;
    MbcgBuffers b;
    b.ph = scope.alloc(in_bytes);
    b.sh = scope.alloc(in_bytes);
    b.p = pc ? scope.alloc(r_bytes) : (b.ph ? (char *)b.ph + own_off : nullptr);
    b.s = pc ? scope.alloc(r_bytes) : (b.sh ? (char *)b.sh + own_off : nullptr);
    b.v = scope.alloc(out_bytes);
    b.t = scope.alloc(out_bytes);
    b.x = scope.alloc(out_bytes);
    b.r = scope.alloc(r_bytes);
    b.rhat = scope.alloc(r_bytes);
    b.work = precond_work_alloc(scope, pc, k);
    b.sc = scope.alloc<double>(kMbcgSlots * kMcgMaxK * sizeof(double));
    b.part0 = scope.alloc<double>((size_t)2 * kMcgBlocks * kMcgMaxK * sizeof(double));
    b.part1 = b.part0 ? b.part0 + (size_t)kMcgBlocks * kMcgMaxK : nullptr;
    b.gath = scope.alloc<double>((size_t)kMaxRanks * kMcgMaxK * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * kk * sizeof(double));
    b.flags = scope.alloc<int>(kMbcgFlagWords * sizeof(int));
    // R = R^ = P = B on this rank's rows (the rest of P^ arrives by the all-gatherv)
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(b.r, (const char *)B_host + own_off, own_bytes, hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && n_own) e = hipMemcpyAsync(b.rhat, b.r, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (e == hipSuccess && n_own) e = hipMemcpyAsync(b.p, b.r, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (solver_begin(scope, e, what)) return -1;
    int steps = 0;
    const bool wide = kk * vb % 16 == 0;
    if (wide ? mbcg_run<T, 16 / sizeof(T)>(m, pc, k, iters, tol, kbounds.data(), b, &steps)
             : mbcg_run<T, 1>(m, pc, k, iters, tol, kbounds.data(), b, &steps))
        return -1;
    // stopped early: every column has stopped, its history repeats its last value
    int flags[kMbcgFlagWords];
    if (solver_finish(scope, what, m->value_bytes, kbounds.data(), b.x, X_host, n_all * kk * vb, {{rr_hist, b.hist}}, steps,
                      iters, kk, b.flags, flags, kMbcgFlagWords, ms_total))
        return -1;
    if (steps_out) std::memcpy(steps_out, flags + kMcgDone, kk * sizeof(int));
    if (status_out) std::memcpy(status_out, flags + kMbcgStatus, kk * sizeof(int));
    if (half_out) std::memcpy(half_out, flags + kMbcgHalf, kk * sizeof(int));
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_bicgstab_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol,
                                           const int *bounds, const void *B_host, void *X_host, double *rr_hist,
                                           int *steps, int *status, int *half_step, float *ms_total) {
    if (need_device()) return -1;
    const char *what = "csr_bicgstab_multi";
    if (!m || !B_host) return fail("%s: bad arguments", what);
    if (solver_check_steps(what, iters, tol)) return -1;
    if (k < 1 || k > kMcgMaxK) return fail("%s: k = %d, must be in [1, %d]", what, k, kMcgMaxK);
    if (solver_check_square(what, m)) return -1;
    if (m->tiles_only) return fail("%s: a tiles-only handle has no SpMM kernels", what);
    if ((long long)m->M_total * k > 0x7fffffffLL)
        return fail("%s: n * k = %lld values is beyond int range", what, (long long)m->M_total * k);
    if (solver_check_rows(what, m, bounds)) return -1;
    if (P && (precond_refuse_one_wide(P, what) || precond_matches(m, P, what))) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return mbcg_body<decltype(t)>(m, P, k, iters, tol, bounds, B_host, X_host, rr_hist, steps, status, half_step, ms_total);
    });
}
