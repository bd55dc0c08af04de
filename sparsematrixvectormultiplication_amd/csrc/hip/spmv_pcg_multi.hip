// spmv_pcg_multi.hip -- spmv_hip_csr_pcg_multi: k independent preconditioned CG recurrences on a CSR handle that share
// one SpMM per step, and the k-wide preconditioner apply (include/spmv_hip.h; the kernels are in pcg_multi_kernels.hpp).
//
//     R = B; Z = M^-1 R; P = Z; rz_j = r_j.z_j; rr0_j = r_j.r_j
//     per step:  Q = A P (one SpMM); alpha_j = rz_j / p_j.q_j; x_j += alpha_j p_j; r_j -= alpha_j q_j; Z = M^-1 R;
//                rz'_j = r_j.z_j; rr_j = r_j.r_j (rr_j <= tol^2 rr0_j: column j stops); beta_j = rz'_j / rz_j;
//                p_j = z_j + beta_j p_j
//
// The loop of csr_pcg with the layout of csr_cg_multi: P (N x k, the SpMM's input, all-gathered with the bounds scaled
// by k when a communicator exists), Q, X (M_total x k), R and Z (this rank's rows) are row-major.  The paths of the
// x / r update (precond_path):
//
//   NONE    x += alpha p, r -= alpha q and the partials of r.r (z is r): cg_multi's step, cg_multi's bits
//   JACOBI  the same with z = D^-1 r fused in, partials of r.r and r.z
//   BLOCK   x += alpha p, r -= alpha q, then mpc_apply: Z = M^-1 R with the partials of r.r and r.z
//   OWN     x += alpha p, r -= alpha q, then the kind's k-wide apply through products alone (FSAI: Z = G^T (G R), two
//           SpMMs through P's handles; AMG: one V(1,1) cycle on R; CHEBYSHEV: its passes), then mpcg_dots
//
// A kind without a k-wide apply is refused (precond_refuse_one_wide).  Every column carries its own scalars,
// stop state, steps and status on the device; a stopped column still rides in the SpMMs and keeps x, r, z and p.
#include "spmv_internal.hpp"

#include "pcg_multi_kernels.hpp"

namespace {

// Z = M^-1 R for Jacobi / block-Jacobi on stream s, V values per lane; DOTS, flags and the partials as mpc_apply
template <typename T, int V, bool DOTS>
void mpc_launch(const spmv_precond *P, int k, const void *R, void *Z, const int *flags, double *part_rr, double *part_rz,
                int grid, hipStream_t s) {
    const int cl = mcg_column_lanes(k, V);
    hipLaunchKernelGGL((mpc_apply<T, V, DOTS>), dim3(grid), dim3(kBlock), 0, s, (long long)P->rows, k, cl, P->block,
                       (const T *)P->inv, (const T *)R, (T *)Z, flags, part_rr, part_rz);
}

// the k-wide apply outside a solve (csr_lobpcg's too, through spmv_hip_precond_apply_multi_on): any kind with one; a
// family's own launches, or mpc_apply in 16-byte pieces when the rows and both arrays allow them
template <typename T>
int mpc_apply_on(const spmv_precond *P, int k, const void *R, void *Z, void *work, hipStream_t s) {
    if (!P->rows) return 0;
    if (P->family) return P->family->apply_multi(P, k, R, Z, work, s);
    constexpr int W = 16 / sizeof(T);
    const bool wide = (size_t)k * sizeof(T) % 16 == 0 && (((uintptr_t)R | (uintptr_t)Z) & 15) == 0;
    const int grid = solver_grid(kMcgBlocks, P->rows, kBlock >> mcg_column_lanes(k, wide ? W : 1));
    if (wide) mpc_launch<T, W, false>(P, k, R, Z, nullptr, nullptr, nullptr, grid, s);
    else mpc_launch<T, 1, false>(P, k, R, Z, nullptr, nullptr, nullptr, grid, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpc_apply_check(const spmv_precond *P, int k, const void *R, const void *Z, const char *what) {
    if (!P || k < 1 || (P->rows && (!R || !Z))) return fail("%s: bad arguments", what);
    if (k > kMcgMaxK) return fail("%s: k = %d, must be in [1, %d]", what, k, kMcgMaxK);
    if ((long long)P->rows * k > 0x7fffffffLL)
        return fail("%s: rows * k = %lld values is beyond int range", what, (long long)P->rows * k);
    return precond_refuse_one_wide(P, what);
}

struct MpcgBuffers {
    // Z is R without a preconditioner; work: FSAI's G R, AMG's level vectors, CHEBYSHEV's three arrays
    void *P, *Q, *X, *R, *Z, *work;
    double *s, *part_rr, *part_rz, *gath, *hrr, *hrz;
    int *flags;
};

// the loop; V = values of T per lane.  *steps = the steps run (< iters when tol > 0 and every column stopped)
template <typename T, int V>
int mpcg_run(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const int *kbounds,
             const MpcgBuffers &b, int *steps) {
    const long long n = m->M_local, kk = k;
    const int cl = mcg_column_lanes(k, V);
    const int cap = k == 1 ? kNormBlocks : kMcgBlocks;  // k = 1: csr_pcg's workgroups, csr_pcg's bits
    const int grid = solver_grid(cap, n, kBlock >> cl);
    const PrecondPath path = precond_path(pc);
    const int z_is_r = path == kPathNone;
    const double tol2 = tol * tol;
    T *P = (T *)b.P, *p_own = P + m->row0 * kk, *q_own = (T *)b.Q + m->row0 * kk, *x_own = (T *)b.X + m->row0 * kk;
    T *R = (T *)b.R, *Z = (T *)b.Z;
    const T *dinv = pc ? (const T *)pc->inv : nullptr;
    const double *sc = b.s;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock);
    // one plane of part[0 .. grid) x k of this rank -> the k global sums in slot `slot` of b.s on every rank
    auto reduce = [&](const double *part, int slot) {
        return solver_reduce(part, grid, k, b.s + (size_t)slot * kMcgMaxK, b.s + (size_t)kMpcgLocal * kMcgMaxK, b.gath,
                             "csr_pcg_multi");
    };
    // r.r -> kMpcgRrNew, and with a preconditioner r.z -> kMpcgRzNew
    auto reduce_dots = [&] { return reduce(b.part_rr, kMpcgRrNew) || (!z_is_r && reduce(b.part_rz, kMpcgRzNew)); };
    // after the x / r update of the paths that do not fuse their apply: Z = M^-1 R and the two sets of partials
    auto apply_dots = [&](const int *flags) {
        if (path == kPathBlock) {
            mpc_launch<T, V, true>(pc, k, R, Z, flags, b.part_rr, b.part_rz, grid, g_stream);
            return 0;
        }
        if (pc->family->apply_multi(pc, k, R, Z, b.work, g_stream)) return -1;
        hipLaunchKernelGGL((mpcg_dots<T, V>), g, blk, 0, g_stream, n, k, cl, (const T *)R, (const T *)Z, b.part_rr, b.part_rz);
        return 0;
    };
    // Z = M^-1 R, rr0 = r.r, rz = r.z with R = B; P = Z (its own range; the rest by the all-gatherv)
    if (path == kPathNone)
        hipLaunchKernelGGL((mpcg_start_dots<T, V, false>), g, blk, 0, g_stream, n, k, cl, dinv, (const T *)R, Z, b.part_rr, b.part_rz);
    else if (path == kPathJacobi)
        hipLaunchKernelGGL((mpcg_start_dots<T, V, true>), g, blk, 0, g_stream, n, k, cl, dinv, (const T *)R, Z, b.part_rr, b.part_rz);
    else if (apply_dots(nullptr))
        return -1;
    if (reduce_dots()) return -1;
    hipLaunchKernelGGL(mpcg_start, dim3(1), dim3(64), 0, g_stream, b.s, b.flags, b.hrr, b.hrz, k, iters, z_is_r);
    if (n) HIP_TRY(hipMemcpyAsync(p_own, Z, (size_t)(n * kk) * sizeof(T), hipMemcpyDeviceToDevice, g_stream));
    if (g_comm && spmv_hip_comm_allgatherv(P, kbounds, m->value_bytes, g_stream)) return -1;
    *steps = iters;
    for (int t = 1; t <= iters; ++t) {
        if (spmv_hip_csr_spmm_on(m, k, P, b.Q, g_stream)) return -1;  // Q = A P on this rank's rows
        hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, (const T *)p_own, (const T *)q_own, n, k, cl,
                           b.part_rr);
        if (reduce(b.part_rr, kMcgPq)) return -1;
        hipLaunchKernelGGL(mpcg_set_alpha, dim3(1), dim3(64), 0, g_stream, b.s, b.flags, k, t);
        if (path == kPathNone) {
            hipLaunchKernelGGL((mpcg_update_x_r<T, V, kMpcgNone>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)p_own,
                               (const T *)q_own, dinv, x_own, R, Z, b.part_rr, b.part_rz);
        } else if (path == kPathJacobi) {
            hipLaunchKernelGGL((mpcg_update_x_r<T, V, kMpcgJacobi>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)p_own,
                               (const T *)q_own, dinv, x_own, R, Z, b.part_rr, b.part_rz);
        } else {
            hipLaunchKernelGGL((mpcg_update_x_r<T, V, kMpcgApply>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)p_own,
                               (const T *)q_own, dinv, x_own, R, Z, b.part_rr, b.part_rz);
            if (apply_dots(fl)) return -1;
        }
        if (reduce_dots()) return -1;
        hipLaunchKernelGGL(mpcg_set_beta, dim3(1), dim3(64), 0, g_stream, b.s, b.flags, b.hrr + (size_t)t * kk,
                           b.hrz + (size_t)t * kk, k, t, tol2, z_is_r);
        hipLaunchKernelGGL((mcg_update_p<T, V>), g, blk, 0, g_stream, n, k, cl, sc, fl, (const T *)Z, p_own);
        if (g_comm && spmv_hip_comm_allgatherv(P, kbounds, m->value_bytes, g_stream)) return -1;
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
int mpcg_body(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, const int *bounds,
              const void *B_host, void *X_host, double *rr_hist, double *rz_hist, int *steps_out, int *status_out,
              float *ms_total) {
    const size_t kk = (size_t)k, vb = sizeof(T);
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local, ncols = (size_t)m->N;
    const std::vector<int> kbounds = solver_scaled_bounds(bounds, k);
    SolverScope scope;
    // what feeds a product at k = 1 is read in whole 128-byte lines by the x-window SpMV kernels: P by A, and with
    // FSAI R by G and work by G^T
    const size_t p_bytes = std::max<size_t>(ncols * kk * vb, 16) + kLineBytes;
    const size_t q_bytes = std::max<size_t>(n_all * kk * vb, 16);
    const size_t own_bytes = n_own * kk * vb, r_bytes = std::max<size_t>(own_bytes, 16) + kLineBytes;
    MpcgBuffers b;
    b.P = scope.alloc(p_bytes);
    b.Q = scope.alloc(q_bytes);
    b.X = scope.alloc(q_bytes);
    b.R = scope.alloc(r_bytes);
    b.Z = pc ? scope.alloc(r_bytes) : b.R;
    b.work = precond_work_alloc(scope, pc, k);
    b.s = scope.alloc<double>(kMpcgSlots * kMcgMaxK * sizeof(double));
    b.part_rr = scope.alloc<double>((size_t)2 * kMcgBlocks * kMcgMaxK * sizeof(double));
    b.part_rz = b.part_rr ? b.part_rr + (size_t)kMcgBlocks * kMcgMaxK : nullptr;
    b.gath = scope.alloc<double>((size_t)kMaxRanks * kMcgMaxK * sizeof(double));
    b.hrr = scope.alloc<double>(((size_t)iters + 1) * kk * sizeof(double));
    b.hrz = scope.alloc<double>(((size_t)iters + 1) * kk * sizeof(double));
    b.flags = scope.alloc<int>(kMpcgFlagWords * sizeof(int));
    // R = B on this rank's rows; P starts at 0 (its own range is set to Z by the loop)
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(b.R, (const char *)B_host + (size_t)m->row0 * kk * vb, own_bytes, hipMemcpyHostToDevice, g_stream);
    if (solver_begin(scope, e, "csr_pcg_multi")) return -1;
    int steps = 0;
    const bool wide = kk * vb % 16 == 0;
    if (wide ? mpcg_run<T, 16 / sizeof(T)>(m, pc, k, iters, tol, kbounds.data(), b, &steps)
             : mpcg_run<T, 1>(m, pc, k, iters, tol, kbounds.data(), b, &steps))
        return -1;
    // stopped early: every column has stopped, its histories repeat their last value
    int flags[kMpcgFlagWords];
    if (solver_finish(scope, "csr_pcg_multi", m->value_bytes, kbounds.data(), b.X, X_host, n_all * kk * vb,
                      {{rr_hist, b.hrr}, {rz_hist, b.hrz}}, steps, iters, kk, b.flags, flags, kMpcgFlagWords, ms_total))
        return -1;
    if (steps_out) std::memcpy(steps_out, flags + kMcgDone, kk * sizeof(int));
    if (status_out) std::memcpy(status_out, flags + kMpcgStatus, kk * sizeof(int));
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_pcg_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol,
                                      const int *bounds, const void *B_host, void *X_host, double *rr_hist,
                                      double *rz_hist, int *steps, int *status, float *ms_total) {
    if (need_device()) return -1;
    const char *what = "csr_pcg_multi";
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
        return mpcg_body<decltype(t)>(m, P, k, iters, tol, bounds, B_host, X_host, rr_hist, rz_hist, steps, status, ms_total);
    });
}

extern "C" int spmv_hip_precond_apply_multi_on(const spmv_precond *P, int k, const void *d_R, void *d_Z, void *d_work,
                                               void *stream) {
    if (need_device()) return -1;
    if (mpc_apply_check(P, k, d_R, d_Z, "precond_apply_multi_on")) return -1;
    if (P->family && P->rows && !d_work) return fail("precond_apply_multi_on: %s", P->family->work_text);
    if (((uintptr_t)d_R | (uintptr_t)d_Z | (uintptr_t)d_work) % (uintptr_t)P->value_bytes)
        return fail("precond_apply_multi_on: R, Z and work must be aligned to %d bytes", P->value_bytes);
    hipStream_t s = stream ? (hipStream_t)stream : g_stream;
    return P->value_bytes == 8 ? mpc_apply_on<double>(P, k, d_R, d_Z, d_work, s) : mpc_apply_on<float>(P, k, d_R, d_Z, d_work, s);
}

extern "C" int spmv_hip_precond_apply_multi(const spmv_precond *P, int k, const void *R_host, void *Z_host) {
    if (need_device()) return -1;
    if (mpc_apply_check(P, k, R_host, Z_host, "precond_apply_multi")) return -1;
    return guarded("precond_apply_multi", [&] {
        const size_t bytes = (size_t)P->rows * (size_t)k * P->value_bytes, padded = std::max<size_t>(bytes, 16) + kLineBytes;
        SolverScope scope;
        void *R = scope.alloc(padded);
        void *Z = scope.alloc(padded);
        void *work = precond_work_alloc(scope, P, k);
        hipError_t e = scope.err;
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(R, R_host, bytes, hipMemcpyHostToDevice, g_stream);
        if (e != hipSuccess) return solver_setup_failed("precond_apply_multi", e);
        if (P->value_bytes == 8 ? mpc_apply_on<double>(P, k, R, Z, work, g_stream)
                                : mpc_apply_on<float>(P, k, R, Z, work, g_stream))
            return -1;
        e = hipStreamSynchronize(g_stream);
        if (e == hipSuccess && bytes) e = hipMemcpy(Z_host, Z, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return solver_run_failed("precond_apply_multi", e);
        return 0;
    });
}

extern "C" int spmv_hip_precond_work_bytes(const spmv_precond *P, int k, long long *bytes) {
    if (!P || !bytes) return fail("precond_work_bytes: bad arguments");
    *bytes = -1;
    if (k < 1 || k > kMcgMaxK) return fail("precond_work_bytes: k = %d, must be in [1, %d]", k, kMcgMaxK);
    if (precond_refuse_one_wide(P, "precond_work_bytes")) return -1;
    *bytes = precond_work_bytes(P, k);
    return 0;
}
