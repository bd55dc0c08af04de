// spmv_minres_multi.hip -- spmv_hip_csr_minres_multi: k independent MINRES recurrences on a CSR handle, each with its
// own shift, that share the one SpMM of a step and the k-wide preconditioner apply (include/spmv_hip.h; the kernels are
// in minres_multi_kernels.hpp).
//
//     R1 = R2 = B; Y = M^-1 R2 (or R2); bb0_j = r2_j.y_j; beta_j = sqrt(bb0_j); phibar_j = beta_j; cs_j = -1; the rest 0
//     per step:  v_j = y_j / beta_j; A_V = A V (one SpMM); t_j = a_j - shift_j v_j - (beta_j / oldb_j) r1_j;
//                alfa_j = v_j.t_j; t_j -= (alfa_j / beta_j) r2_j; r1_j = r2_j; r2_j = t_j; Y = M^-1 R2 (or R2);
//                bb_j = r2_j.y_j; the rotation; w_j = (v_j - oldeps_j w1_j - delta_j w2_j) / gamma_j; x_j += phi_j w_j
//
// The loop of csr_minres with the layout of csr_cg_multi.  V (N x k, the SpMM's input, with the 128-byte line tail the
// x-window kernels read at k = 1; all-gathered with the bounds scaled by k when a communicator exists), A_V and X
// (M_total x k), the two R buffers, the two W buffers and Y (this rank's rows) are row-major.  t is written over r1's
// buffer and w over w1's, so the host swaps the two r pointers and the two w pointers after every step.  Without a
// preconditioner y is r2 itself and mmr_lanczos_b's t.t is bb.  The paths of y (precond_path):
//
//   NONE    y is r2: no apply, no extra dot
//   JACOBI  y = D^-1 t and t.y fused into mmr_lanczos_b
//   BLOCK, OWN   mmr_lanczos_b, then the k-wide apply through spmv_hip_precond_apply_multi_on (mpc_apply for
//           block-Jacobi, the family's launches for FSAI, AMG and CHEBYSHEV), then mcg_dot_partial for t.y
//
// A kind without a k-wide apply is refused (precond_refuse_one_wide).  Every column carries its own shift, scalars,
// state, steps and status on the device; a stopped column still rides in the SpMM and the applies and keeps x, r1, r2,
// w and v.
#include "spmv_internal.hpp"

#include "minres_multi_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

struct MmrBuffers {
    void *v, *a, *r[2], *w[2], *x;
    void *y, *work;  // with a preconditioner: M^-1 r2 and the workspace of its k-wide apply
    double *sc, *part, *gath, *hist;
    int *flags;
};

// the loop; V = values of T per lane.  *steps = the steps run (< iters when tol > 0 and every column stopped)
template <typename T, int V>
int mmr_run(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const int *kbounds,
            const MmrBuffers &b, int *steps) {
    const char *what = "csr_minres_multi";
    const long long n = m->M_local, kk = k, own = m->row0 * kk;
    const int cl = mcg_column_lanes(k, V);
    const int grid = solver_grid(kMcgBlocks, n, kBlock >> cl);
    const PrecondPath path = precond_path(pc);
    const double tol2 = tol * tol;
    T *VV = (T *)b.v, *v_own = VV + own, *x_own = (T *)b.x + own, *y = (T *)b.y;
    const T *a_own = (const T *)b.a + own;
    T *r1 = (T *)b.r[0], *r2 = (T *)b.r[1], *w1 = (T *)b.w[0], *w2 = (T *)b.w[1];
    const T *dinv = path == kPathJacobi ? (const T *)pc->inv : nullptr;
    const double *sc = b.sc;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock), one(1), wave(64);
    // part[0 .. grid) x k of this rank -> the k global sums in slot `slot` of b.sc on every rank
    auto reduce = [&](int slot) {
        return solver_reduce(b.part, grid, k, b.sc + (size_t)slot * kMcgMaxK, b.sc + (size_t)kMmrLocal * kMcgMaxK, b.gath, what);
    };
    // Y = M^-1 R on this rank's rows by the k-wide apply, and bb = r.y in slot kMmrBb
    auto apply_and_dot = [&](const T *r) {
        if (spmv_hip_precond_apply_multi_on(pc, k, r, y, b.work, g_stream)) return -1;
        hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, r, (const T *)y, n, k, cl, b.part);
        return reduce(kMmrBb);
    };
    if (pc) {
        if (apply_and_dot(r2)) return -1;  // Jacobi too: mmr_lanczos_b fuses it from step 1 on
    } else {
        hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, (const T *)r2, (const T *)r2, n, k, cl, b.part);
        if (reduce(kMmrBb)) return -1;
    }
    hipLaunchKernelGGL(mmr_start, one, wave, 0, g_stream, b.sc, b.flags, b.hist, k, iters);
    hipLaunchKernelGGL((mmr_update<T, V>), g, blk, 0, g_stream, n, k, cl, sc, fl, 0, (const T *)(pc ? y : r2),
                       (const T *)w2, w1, x_own, v_own);  // v = y / beta
    if (g_comm && spmv_hip_comm_allgatherv(VV, kbounds, m->value_bytes, g_stream)) return -1;
    *steps = iters;
    for (int t = 1; t <= iters; ++t) {
        if (spmv_hip_csr_spmm_on(m, k, VV, b.a, g_stream)) return -1;  // A_V = A V on this rank's rows
        hipLaunchKernelGGL((mmr_lanczos_a<T, V>), g, blk, 0, g_stream, n, k, cl, sc, fl, t, a_own, (const T *)v_own, r1,
                           b.part);
        if (reduce(kMmrAlfa)) return -1;
        hipLaunchKernelGGL(mmr_set_alfa, one, wave, 0, g_stream, b.sc, b.flags, k, t);
        if (path == kPathNone) {
            hipLaunchKernelGGL((mmr_lanczos_b<T, V, kMmrNone>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r2, dinv,
                               r1, y, b.part);
            if (reduce(kMmrBb)) return -1;
        } else if (path == kPathJacobi) {
            hipLaunchKernelGGL((mmr_lanczos_b<T, V, kMmrJacobi>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r2,
                               dinv, r1, y, b.part);
            if (reduce(kMmrBb)) return -1;
        } else {
            hipLaunchKernelGGL((mmr_lanczos_b<T, V, kMmrApply>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)r2, dinv,
                               r1, y, b.part);
        }
        std::swap(r1, r2);  // r1 = r2; r2 = t
        if (path >= kPathBlock && apply_and_dot(r2)) return -1;
        hipLaunchKernelGGL(mmr_rotate, one, wave, 0, g_stream, b.sc, b.flags, b.hist + (size_t)t * kk, k, t, tol2);
        hipLaunchKernelGGL((mmr_update<T, V>), g, blk, 0, g_stream, n, k, cl, sc, fl, t, (const T *)(pc ? y : r2),
                           (const T *)w2, w1, x_own, v_own);
        std::swap(w1, w2);  // w1 = w2; w2 = w
        if (g_comm && spmv_hip_comm_allgatherv(VV, kbounds, m->value_bytes, g_stream)) return -1;
        bool stop = false;  // no column is running
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
int mmr_body(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const double *shift,
             const int *bounds, const void *B_host, void *X_host, double *rr_hist, int *steps_out, int *status_out,
             float *ms_total) {
    const char *what = "csr_minres_multi";
    const size_t kk = (size_t)k, vb = sizeof(T);
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local, ncols = (size_t)m->N;
    const std::vector<int> kbounds = solver_scaled_bounds(bounds, k);
    SolverScope scope;
    // what feeds a product at k = 1 is read in whole 128-byte lines by the x-window SpMV kernels: V by A, and with a
    // family's apply either R buffer by its first product (FSAI's G)
    const size_t in_bytes = std::max<size_t>(ncols * kk * vb, 16) + kLineBytes;
    const size_t out_bytes = std::max<size_t>(n_all * kk * vb, 16);
    const size_t own_off = (size_t)m->row0 * kk * vb, own_bytes = n_own * kk * vb;
    const size_t r_bytes = std::max<size_t>(own_bytes, 16) + kLineBytes;
    MmrBuffers b;
    b.v = scope.alloc(in_bytes);
    b.a = scope.alloc(out_bytes);
    b.r[0] = scope.alloc(r_bytes);
    b.r[1] = scope.alloc(r_bytes);
    b.w[0] = scope.alloc(r_bytes);
    b.w[1] = scope.alloc(r_bytes);
    b.x = scope.alloc(out_bytes);
    b.y = pc ? scope.alloc(r_bytes) : nullptr;
    b.work = precond_work_alloc(scope, pc, k);
    b.sc = scope.alloc<double>(kMmrSlots * kMcgMaxK * sizeof(double));
    b.part = scope.alloc<double>((size_t)kMcgBlocks * kMcgMaxK * sizeof(double));
    b.gath = scope.alloc<double>((size_t)kMaxRanks * kMcgMaxK * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * kk * sizeof(double));
    b.flags = scope.alloc<int>(kMmrFlagWords * sizeof(int));
    // R2 = B on this rank's rows (R1 is first read at step 2, after step 1 made it R2); the k shifts (NULL: all 0)
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(b.r[1], (const char *)B_host + own_off, own_bytes, hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && shift)
        e = hipMemcpyAsync(b.sc + (size_t)kMmrShift * kMcgMaxK, shift, kk * sizeof(double), hipMemcpyHostToDevice, g_stream);
    if (solver_begin(scope, e, what)) return -1;
    int steps = 0;
    const bool wide = kk * vb % 16 == 0;
    if (wide ? mmr_run<T, 16 / sizeof(T)>(m, pc, k, iters, tol, kbounds.data(), b, &steps)
             : mmr_run<T, 1>(m, pc, k, iters, tol, kbounds.data(), b, &steps))
        return -1;
    // stopped early: every column has stopped, its history repeats its last value
    int flags[kMmrFlagWords];
    if (solver_finish(scope, what, m->value_bytes, kbounds.data(), b.x, X_host, n_all * kk * vb, {{rr_hist, b.hist}}, steps,
                      iters, kk, b.flags, flags, kMmrFlagWords, ms_total))
        return -1;
    if (steps_out) std::memcpy(steps_out, flags + kMcgDone, kk * sizeof(int));
    if (status_out) std::memcpy(status_out, flags + kMmrStatus, kk * sizeof(int));
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_minres_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol,
                                         const double *shift, const int *bounds, const void *B_host, void *X_host,
                                         double *rr_hist, int *steps, int *status, float *ms_total) {
    if (need_device()) return -1;
    const char *what = "csr_minres_multi";
    if (!m || !B_host) return fail("%s: bad arguments", what);
    if (solver_check_steps(what, iters, tol)) return -1;
    if (k < 1 || k > kMcgMaxK) return fail("%s: k = %d, must be in [1, %d]", what, k, kMcgMaxK);
    for (int j = 0; shift && j < k; ++j)
        if (!std::isfinite(shift[j])) return fail("%s: shift[%d] = %g, must be finite", what, j, shift[j]);
    if (solver_check_square(what, m)) return -1;
    if (m->tiles_only) return fail("%s: a tiles-only handle has no SpMM kernels", what);
    if ((long long)m->M_total * k > 0x7fffffffLL)
        return fail("%s: n * k = %lld values is beyond int range", what, (long long)m->M_total * k);
    if (solver_check_rows(what, m, bounds)) return -1;
    if (P && (precond_refuse_one_wide(P, what) || precond_matches(m, P, what))) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return mmr_body<decltype(t)>(m, P, k, iters, tol, shift, bounds, B_host, X_host, rr_hist, steps, status, ms_total);
    });
}
