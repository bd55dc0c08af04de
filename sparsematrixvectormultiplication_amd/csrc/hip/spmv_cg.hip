// spmv_cg.hip -- conjugate gradients on a CSR handle, entirely on the device (include/spmv_hip.h): spmv_hip_csr_cg for
// one right-hand side and spmv_hip_csr_cg_multi for k that share one SpMM per step.
#include "spmv_internal.hpp"

#include "cg_multi_kernels.hpp"

// ------------------------------------------------------------- conjugate gradients
// SURVEY.md 8(f) N4, the second iterated skeleton (the reference multiplies by a fixed x; a Krylov method is what
// an SpMV engine is for).  Plain CG for a symmetric positive definite A, x0 = 0:
//     r = b, p = b, rs = r.r;   repeat:  q = A p;  alpha = rs / p.q;  x += alpha p;  r -= alpha q;
//                                        rs' = r.r;  beta = rs' / rs;  p = r + beta p;  rs = rs'
// p is the handle's x (the SpMV input, full length on every rank), q its y (this rank's rows).  Every rank keeps
// its own rows of x, r; the SpMV's exchange is the same as in the power iteration -- all-gatherv of p, or the
// halo exchange when spmv_hip_comm_halo_setup has run and use_halo is set.  Dot products are fixed-order device
// reductions (grid-stride partial sums per workgroup, folded by one workgroup); across ranks the partial sums are
// ALL-GATHERED and added in rank order by every rank (solver_reduce), so all ranks hold the same bits whatever
// reduction tree the collective library would pick for an all-reduce.  Scalars stay on the device: no host
// synchronisation in the loop.
namespace {

constexpr int kCgRs = 0, kCgPq = 1, kCgRsNew = 2, kCgAlpha = 3, kCgBeta = 4, kCgLocal = 5, kCgScalars = 8;

// the lanes walk single elements (PieceLane with V = 1): the order of norm2_partial
template <typename T>
__global__ __launch_bounds__(kBlock) void dot_partial(const T *__restrict__ a, const T *__restrict__ b, long long n,
                                                      double *__restrict__ part) {
    double acc[1] = {0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) acc[0] += (double)a[l.q] * (double)b[l.q];
    block_partials<1>(acc, part);
}

// x += alpha p, r -= alpha q on this rank's rows, and the workgroup's partial of the new r.r
template <typename T>
__global__ __launch_bounds__(kBlock) void cg_update_x_r(long long n, const double *__restrict__ s, const T *__restrict__ p,
                                                        const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                        double *__restrict__ part) {
    const double alpha = s[kCgAlpha];
    double acc[1] = {0.0};
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) {
        const long long k = l.q;
        x[k] = (T)((double)x[k] + alpha * (double)p[k]);
        const T rk = (T)((double)r[k] - alpha * (double)q[k]);
        r[k] = rk;
        acc[0] += (double)rk * (double)rk;
    }
    block_partials<1>(acc, part);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void cg_update_p(long long n, const double *__restrict__ s, const T *__restrict__ r,
                                                      T *__restrict__ p) {
    const double beta = s[kCgBeta];
    for (PieceLane l(0, n, 1); l.q < l.end; l.q += l.stride) p[l.q] = (T)((double)r[l.q] + beta * (double)p[l.q]);
}

__global__ void cg_set_alpha(double *__restrict__ s) { s[kCgAlpha] = s[kCgPq] != 0.0 ? s[kCgRs] / s[kCgPq] : 0.0; }
__global__ void cg_set_beta(double *__restrict__ s, double *__restrict__ hist, int k) {
    s[kCgBeta] = s[kCgRs] != 0.0 ? s[kCgRsNew] / s[kCgRs] : 0.0;
    s[kCgRs] = s[kCgRsNew];
    if (hist) hist[k] = s[kCgRsNew];
}
__global__ void cg_record(const double *__restrict__ s, double *__restrict__ hist) { hist[0] = s[kCgRs]; }

int cg_exchange_p(spmv_csr_dev *m, const int *bounds, int use_halo) {
    if (!g_comm) return 0;
    if (use_halo) return spmv_hip_comm_halo_exchange(m->x, m->value_bytes, g_stream);
    return spmv_hip_comm_allgatherv(m->x, bounds, m->value_bytes, g_stream);
}

template <typename T>
int cg_run(spmv_csr_dev *m, int variant, int iters, const int *bounds, int use_halo, T *d_xs, T *d_r, double *d_s,
           double *d_part, double *d_gath, double *d_hist) {
    const long long n = m->M_local;
    const int grid = solver_grid(kNormBlocks, n, kBlock);
    T *p_own = (T *)m->x + m->row0, *q_own = (T *)m->y + m->row0, *x_own = d_xs + m->row0;
    // part[0 .. grid) of this rank -> the global sum in d_s[slot] on every rank
    auto reduce = [&](int slot) { return solver_reduce(d_part, grid, 1, d_s + slot, d_s + kCgLocal, d_gath, "csr_cg"); };
    // rs = r.r with r = b (already in d_r and in p's own range); every rank gets the whole p
    hipLaunchKernelGGL((dot_partial<T>), dim3(grid), dim3(kBlock), 0, g_stream, (const T *)d_r, (const T *)d_r, n, d_part);
    if (reduce(kCgRs)) return -1;
    hipLaunchKernelGGL(cg_record, dim3(1), dim3(1), 0, g_stream, d_s, d_hist);
    if (cg_exchange_p(m, bounds, use_halo)) return -1;
    for (int k = 0; k < iters; ++k) {
        if (csr_launch_any(m, variant, m->x, m->y, g_stream)) return -1;  // q = A p on this rank's rows
        hipLaunchKernelGGL((dot_partial<T>), dim3(grid), dim3(kBlock), 0, g_stream, (const T *)p_own, (const T *)q_own, n, d_part);
        if (reduce(kCgPq)) return -1;
        hipLaunchKernelGGL(cg_set_alpha, dim3(1), dim3(1), 0, g_stream, d_s);
        hipLaunchKernelGGL((cg_update_x_r<T>), dim3(grid), dim3(kBlock), 0, g_stream, n, d_s, (const T *)p_own,
                           (const T *)q_own, x_own, d_r, d_part);
        if (reduce(kCgRsNew)) return -1;
        hipLaunchKernelGGL(cg_set_beta, dim3(1), dim3(1), 0, g_stream, d_s, d_hist, k + 1);
        hipLaunchKernelGGL((cg_update_p<T>), dim3(grid), dim3(kBlock), 0, g_stream, n, d_s, (const T *)d_r, p_own);
        if (cg_exchange_p(m, bounds, use_halo)) return -1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int cg_body(spmv_csr_dev *m, int variant, int iters, const int *bounds, int use_halo, const void *b_host, void *x_host,
            double *rr_hist, float *ms_total) {
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local;
    SolverScope scope;
    T *d_xs = scope.alloc<T>(std::max<size_t>(n_all, 1) * sizeof(T));
    T *d_r = scope.alloc<T>(std::max<size_t>(n_own, 1) * sizeof(T));
    double *d_s = scope.alloc<double>(kCgScalars * sizeof(double));
    double *d_part = scope.alloc<double>(kNormBlocks * sizeof(double));
    double *d_gath = scope.alloc<double>(kMaxRanks * sizeof(double));
    double *d_hist = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    // r = b on this rank's rows; p = b: the own range of the handle's x (the rest arrives by the exchange)
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(d_r, (const T *)b_host + m->row0, n_own * sizeof(T), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->x, 0, (size_t)m->N * sizeof(T), g_stream);
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((T *)m->x + m->row0, d_r, n_own * sizeof(T), hipMemcpyDeviceToDevice, g_stream);
    if (solver_begin(scope, e, "csr_cg")) return -1;
    if (cg_run<T>(m, variant, iters, bounds, use_halo, d_xs, d_r, d_s, d_part, d_gath, d_hist)) return -1;
    return solver_finish(scope, "csr_cg", m->value_bytes, bounds, d_xs, x_host, n_all * sizeof(T), {{rr_hist, d_hist}},
                         iters, iters, 1, nullptr, nullptr, 0, ms_total);
}

}  // namespace

extern "C" int spmv_hip_csr_cg(spmv_csr_dev *m, int variant, int iters, const int *bounds, int use_halo,
                               const void *b_host, void *x_host, double *rr_hist, float *ms_total) {
    if (need_device()) return -1;
    if (!m || iters < 0 || !b_host) return fail("csr_cg: bad arguments");
    if (solver_check_square("csr_cg", m)) return -1;
    // (its own lines from here: a partial handle is not refused, and the halo check sits between the shared two)
    if (g_comm && !bounds) return fail("csr_cg: a communicator exists, the row bounds are required");
    if (g_comm && use_halo && !g_halo_ready) return fail("csr_cg: call spmv_hip_comm_halo_setup first");
    if (g_comm_size > kMaxRanks) return fail("csr_cg: more than %d ranks", kMaxRanks);
    return solver_dispatch("csr_cg", m->value_bytes, [&](auto t) {
        return cg_body<decltype(t)>(m, variant, iters, bounds, use_halo, b_host, x_host, rr_hist, ms_total);
    });
}

// ------------------------------------------------------------- k right-hand sides
// spmv_hip_csr_cg_multi: k independent CG recurrences (one alpha, beta per column; not block CG) that share one SpMM
// per step, so the matrix streams from HBM once per step for all k.  The loop of csr_cg, k wide: P (N x k, the SpMM
// input), Q = A P (M_total x k), X and R (this rank's rows) are row-major; the vector kernels and the scalar kernels
// are in cg_multi_kernels.hpp.  With a communicator P is all-gathered with the row bounds scaled by k (a row of P is
// k contiguous values) and the k dot products travel as in csr_cg: all-gathered, added in rank order (solver_reduce).
namespace {

// ---- the scalar kernels: one wavefront, lane j = column j (mcg_count_active and the slots: cg_multi_kernels.hpp)
// after r.r of r = b: rs0 = rs, history row 0; a column with rs0 <= tol2 * rs0 (rs0 = 0 when tol < 1) is frozen at 0
__global__ __launch_bounds__(64) void mcg_start(double *__restrict__ s, int *__restrict__ flags, double *__restrict__ hist,
                                                int k, int iters, double tol2) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        const double rs = s[kMcgRs * kMcgMaxK + j];
        s[kMcgRs0 * kMcgMaxK + j] = rs;
        live = !(rs <= tol2 * rs);
        flags[kMcgAct + j] = live;
        flags[kMcgDone + j] = live ? iters : 0;
        hist[j] = rs;
    }
    mcg_count_active(flags, live);
}

// alpha = rs / p.q (0 when p.q = 0), as cg_set_alpha
__global__ __launch_bounds__(64) void mcg_set_alpha(double *__restrict__ s, int k) {
    const int j = threadIdx.x;
    if (j >= k) return;
    const double pq = s[kMcgPq * kMcgMaxK + j];
    s[kMcgAlpha * kMcgMaxK + j] = pq != 0.0 ? s[kMcgRs * kMcgMaxK + j] / pq : 0.0;
}

// after step t: beta = rs' / rs (0 when rs = 0), rs = rs', as cg_set_beta; then the freeze rule rs' <= tol2 * rs0, and
// history row t (a frozen column repeats its last value)
__global__ __launch_bounds__(64) void mcg_set_beta(double *__restrict__ s, int *__restrict__ flags,
                                                   double *__restrict__ hist_row, int k, int t, double tol2) {
    const int j = threadIdx.x;
    bool live = false;
    if (j < k) {
        live = flags[kMcgAct + j] != 0;
        if (live) {
            const double rs = s[kMcgRs * kMcgMaxK + j], rs_new = s[kMcgRsNew * kMcgMaxK + j];
            s[kMcgBeta * kMcgMaxK + j] = rs != 0.0 ? rs_new / rs : 0.0;
            s[kMcgRs * kMcgMaxK + j] = rs_new;
            if (rs_new <= tol2 * s[kMcgRs0 * kMcgMaxK + j]) {
                live = false;
                flags[kMcgAct + j] = 0;
                flags[kMcgDone + j] = t;
            }
        }
        hist_row[j] = s[kMcgRs * kMcgMaxK + j];
    }
    mcg_count_active(flags, live);
}

struct McgBuffers {
    void *P, *Q, *X, *R;
    double *s, *part, *gath, *hist;
    int *flags;
};

// the loop; V = values of T per lane (16-byte pieces or single elements).  *steps = the steps run (< iters when tol > 0
// and every column froze).
template <typename T, int V>
int mcg_run(spmv_csr_dev *m, int k, int iters, double tol, const int *kbounds, const McgBuffers &b, int *steps) {
    const long long n = m->M_local, kk = k;
    const int cl = mcg_column_lanes(k, V);
    const int cap = k == 1 ? kNormBlocks : kMcgBlocks;  // k = 1: csr_cg's workgroups, csr_cg's bits
    const int grid = solver_grid(cap, n, kBlock >> cl);
    const double tol2 = tol * tol;
    T *P = (T *)b.P, *p_own = P + m->row0 * kk, *q_own = (T *)b.Q + m->row0 * kk, *x_own = (T *)b.X + m->row0 * kk;
    T *R = (T *)b.R;
    const dim3 g(grid), blk(kBlock);
    // part[0 .. grid) x k of this rank -> the k global sums in slot `slot` of b.s on every rank
    auto reduce = [&](int slot) {
        return solver_reduce(b.part, grid, k, b.s + (size_t)slot * kMcgMaxK, b.s + (size_t)kMcgLocal * kMcgMaxK, b.gath,
                             "csr_cg_multi");
    };
    hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, (const T *)R, (const T *)R, n, k, cl, b.part);
    if (reduce(kMcgRs)) return -1;
    hipLaunchKernelGGL(mcg_start, dim3(1), dim3(64), 0, g_stream, b.s, b.flags, b.hist, k, iters, tol2);
    if (g_comm && spmv_hip_comm_allgatherv(P, kbounds, m->value_bytes, g_stream)) return -1;
    *steps = iters;
    for (int t = 1; t <= iters; ++t) {
        if (spmv_hip_csr_spmm_on(m, k, P, b.Q, g_stream)) return -1;  // Q = A P on this rank's rows
        hipLaunchKernelGGL((mcg_dot_partial<T, V>), g, blk, 0, g_stream, (const T *)p_own, (const T *)q_own, n, k, cl,
                           b.part);
        if (reduce(kMcgPq)) return -1;
        hipLaunchKernelGGL(mcg_set_alpha, dim3(1), dim3(64), 0, g_stream, b.s, k);
        hipLaunchKernelGGL((mcg_update_x_r<T, V>), g, blk, 0, g_stream, n, k, cl, (const double *)b.s,
                           (const int *)b.flags, (const T *)p_own, (const T *)q_own, x_own, R, b.part);
        if (reduce(kMcgRsNew)) return -1;
        hipLaunchKernelGGL(mcg_set_beta, dim3(1), dim3(64), 0, g_stream, b.s, b.flags, b.hist + (size_t)t * kk, k, t,
                           tol2);
        hipLaunchKernelGGL((mcg_update_p<T, V>), g, blk, 0, g_stream, n, k, cl, (const double *)b.s,
                           (const int *)b.flags, (const T *)R, p_own);
        if (g_comm && spmv_hip_comm_allgatherv(P, kbounds, m->value_bytes, g_stream)) return -1;
        bool stop = false;  // every column frozen
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
int mcg_body(spmv_csr_dev *m, int k, int iters, double tol, const int *bounds, const void *B_host, void *X_host,
             double *rr_hist, int *iters_done, float *ms_total) {
    const size_t kk = (size_t)k, vb = sizeof(T);
    const size_t n_all = (size_t)m->M_total, n_own = (size_t)m->M_local, ncols = (size_t)m->N;
    const std::vector<int> kbounds = solver_scaled_bounds(bounds, k);
    SolverScope scope;
    // P: read in whole 128-byte lines by the x-window SpMV kernels (k = 1), as the handle's x
    const size_t p_bytes = std::max<size_t>(ncols * kk * vb, 16) + kLineBytes;
    const size_t q_bytes = std::max<size_t>(n_all * kk * vb, 16);
    McgBuffers b;
    b.P = scope.alloc(p_bytes);
    b.Q = scope.alloc(q_bytes);
    b.X = scope.alloc(q_bytes);
    b.R = scope.alloc(std::max<size_t>(n_own * kk * vb, 16));
    b.s = scope.alloc<double>(kMcgSlots * kMcgMaxK * sizeof(double));
    b.part = scope.alloc<double>((size_t)kMcgBlocks * kMcgMaxK * sizeof(double));
    b.gath = scope.alloc<double>((size_t)kMaxRanks * kMcgMaxK * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * kk * sizeof(double));
    b.flags = scope.alloc<int>(kMcgFlagWords * sizeof(int));
    // r = b on this rank's rows; p = b: its own range of P (the rest arrives by the all-gatherv)
    const size_t own_off = (size_t)m->row0 * kk * vb, own_bytes = n_own * kk * vb;
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync(b.R, (const char *)B_host + own_off, own_bytes, hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((char *)b.P + own_off, b.R, own_bytes, hipMemcpyDeviceToDevice, g_stream);
    if (solver_begin(scope, e, "csr_cg_multi")) return -1;
    int steps = 0;
    const bool wide = kk * vb % 16 == 0;
    if (wide ? mcg_run<T, 16 / sizeof(T)>(m, k, iters, tol, kbounds.data(), b, &steps)
             : mcg_run<T, 1>(m, k, iters, tol, kbounds.data(), b, &steps))
        return -1;
    // stopped early: every column is frozen, its history repeats its last value; the flags are read only when asked for
    int flags[kMcgFlagWords];
    if (solver_finish(scope, "csr_cg_multi", m->value_bytes, kbounds.data(), b.X, X_host, n_all * kk * vb,
                      {{rr_hist, b.hist}}, steps, iters, kk, b.flags, iters_done ? flags : nullptr, kMcgFlagWords, ms_total))
        return -1;
    if (iters_done) std::memcpy(iters_done, flags + kMcgDone, kk * sizeof(int));
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_cg_multi(spmv_csr_dev *m, int k, int iters, double tol, const int *bounds,
                                     const void *B_host, void *X_host, double *rr_hist, int *iters_done,
                                     float *ms_total) {
    if (need_device()) return -1;
    int rc = 0;
    if (!m || iters < 0 || !B_host || !(tol >= 0)) rc = fail("csr_cg_multi: bad arguments");
    else if (k < 1 || k > kMcgMaxK) rc = fail("csr_cg_multi: k = %d, must be in [1, %d]", k, kMcgMaxK);
    else if (solver_check_square("csr_cg_multi", m)) rc = -1;
    else if (m->tiles_only) rc = fail("csr_cg_multi: a tiles-only handle has no SpMM kernels");
    else if ((long long)m->M_total * k > 0x7fffffffLL)
        rc = fail("csr_cg_multi: n * k = %lld values is beyond int range", (long long)m->M_total * k);
    else if (g_comm && !bounds) rc = fail("csr_cg_multi: a communicator exists, the row bounds are required");
    else if (g_comm_size > kMaxRanks) rc = fail("csr_cg_multi: more than %d ranks", kMaxRanks);
    if (rc) return rc;
    return solver_dispatch("csr_cg_multi", m->value_bytes, [&](auto t) {
        return mcg_body<decltype(t)>(m, k, iters, tol, bounds, B_host, X_host, rr_hist, iters_done, ms_total);
    });
}
