// spmv_gmres.hip -- spmv_hip_csr_gmres: restarted GMRES(m) on a CSR handle, right-preconditioned (include/spmv_hip.h).
//
//     x = 0; rr0 = b.b
//     per cycle:  r = b - A x (the first cycle: r = b); beta = sqrt(r.r); v_0 = r / beta; g = beta e_0
//       per step: z = M^-1 v_j (or v_j); w = A z; h = V^T w; w -= V h; h' = V^T w; w -= V h'; h += h'; eta = sqrt(w.w)
//                 the rotations on (h, eta); g_{j+1} = -s g_j; g_j = c g_j; hist[t] = g_{j+1}^2; v_{j+1} = w / eta
//       close:    R y = g; u = V y; x += M^-1 u (or u)
//
// The product is the handle's SpMV (csr_launch_any).  Its inputs -- a basis vector without a preconditioner, z with
// one, x at a restart -- and the applies' inputs are library-owned vectors of one stride: N values rounded up to 16
// bytes plus the 128-byte line tail the x-window kernels read, rounded up to whole lines so that every basis vector
// starts on one; the tails stay zero.  w is written into the slot of v_{j+1} and scaled in place.  The vector and
// scalar kernels are in gmres_kernels.hpp; the Hessenberg column, the rotations, g and the stop state stay on the device.
//
// The host reads the flag words once per cycle, after its last step: from the steps counted it knows the columns J of
// the cycle and launches the close with J as an argument.  Inside a cycle nothing synchronises; after a stop the
// vector kernels and the applies return at once, so a stop costs at most restart - 1 empty steps.  The apply of the
// close gets no flags: it runs after a stop.
//
// spmv_hip_gmres_dots and spmv_hip_gmres_update run the two Gram-Schmidt passes alone on device buffers.
#include "spmv_internal.hpp"

#include "gmres_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

// the vector kernels' grid over n rows in pieces of V
int gm_grid(long long n, int V) { return solver_grid(kGmBlocks, (n + V - 1) / V, kBlock); }

// h[0 .. nvec) = V^T w into out (nvec rounded up to kGmTile doubles are written; local: as many, solver_reduce's)
template <typename T>
int gm_dots_launch(long long n, const int *flags, const T *Vb, long long ld, int nvec, const T *w, double *part,
                   double *out, double *local, const char *what) {
    constexpr int V = 16 / sizeof(T);
    const int grid = gm_grid(n, V), tiles = (nvec + kGmTile - 1) / kGmTile;
    hipLaunchKernelGGL((gmres_dots<T, V>), dim3(grid, tiles), dim3(kBlock), 0, g_stream, n, flags, Vb, ld, nvec, w, part);
    return solver_reduce(part, grid, tiles * kGmTile, out, local, nullptr, what);
}

// w -= V h with h on the device; ww != NULL: w.w of what was stored
template <typename T>
int gm_update_launch(long long n, const int *flags, const T *Vb, long long ld, int nvec, const double *h, T *w,
                     double *part, double *ww, double *local, const char *what) {
    constexpr int V = 16 / sizeof(T);
    const int grid = gm_grid(n, V);
    hipLaunchKernelGGL((gmres_update<T, V>), dim3(grid), dim3(kBlock), 0, g_stream, n, flags, Vb, ld, nvec, h, w,
                       ww ? part : nullptr);
    return ww ? solver_reduce(part, grid, 1, ww, local, nullptr, what) : 0;
}

struct GmBuffers {
    void *basis, *b, *q, *x, *u;
    void *z;  // with a preconditioner: M^-1 v_j, and M^-1 u at the close
    double *sc, *part, *hist;
    int *flags;
    long long ld;  // elements between basis vectors
};

struct GmResult {
    int steps = 0, status = SPMV_GMRES_RAN_ALL, cycles = 0;
};

// the cycles
template <typename T>
int gm_run(spmv_csr_dev *m, const spmv_precond *P, int variant, int restart, int iters, double tol,
           const GmBuffers &b, GmResult &res) {
    constexpr int V = 16 / sizeof(T);
    const char *what = "csr_gmres";
    const long long n = m->M_total;
    const int grid = gm_grid(n, V);
    const double tol2 = tol * tol;
    T *basis = (T *)b.basis, *q = (T *)b.q, *x = (T *)b.x, *u = (T *)b.u, *z = (T *)b.z;
    const T *rhs = (const T *)b.b;
    double *sc = b.sc, *local = b.sc + kGmLocal;
    const int *fl = b.flags;
    const dim3 g(grid), blk(kBlock);
    auto vec = [&](int i) { return basis + (long long)i * b.ld; };
    // r = b - q into v_0 with r.r in slot kGmRr
    auto residual = [&] {
        hipLaunchKernelGGL((gm_residual<T, V>), g, blk, 0, g_stream, n, fl, rhs, (const T *)q, vec(0), b.part);
        return solver_reduce(b.part, grid, 1, sc + kGmRr, local, nullptr, what);
    };
    if (residual()) return -1;  // q = 0: r = b, rr0 = b.b
    hipLaunchKernelGGL(gm_start, dim3(1), dim3(1), 0, g_stream, sc, b.flags, b.hist, iters);
    int t = 0;
    for (;;) {
        ++res.cycles;
        hipLaunchKernelGGL(gm_cycle, dim3(1), dim3(1), 0, g_stream, sc, b.flags, t);
        hipLaunchKernelGGL((gm_scale<T, V>), g, blk, 0, g_stream, n, fl, (const double *)(sc + kGmBeta), vec(0));
        const int t0 = t;
        for (int j = 0; j < restart && t < iters; ++j) {
            const T *in = vec(j);
            T *w = vec(j + 1);
            if (P) {
                if (precond_apply<T>(P, vec(j), z, fl, g_stream)) return -1;
                in = z;
            }
            if (csr_launch_any(m, variant, in, w, g_stream)) return -1;  // w = A z
            if (gm_dots_launch<T>(n, fl, basis, b.ld, j + 1, w, b.part, sc + kGmHa, local, what)) return -1;
            if (gm_update_launch<T>(n, fl, basis, b.ld, j + 1, sc + kGmHa, w, b.part, nullptr, local, what)) return -1;
            if (gm_dots_launch<T>(n, fl, basis, b.ld, j + 1, w, b.part, sc + kGmHb, local, what)) return -1;
            if (gm_update_launch<T>(n, fl, basis, b.ld, j + 1, sc + kGmHb, w, b.part, sc + kGmWw, local, what)) return -1;
            ++t;
            hipLaunchKernelGGL(gm_rotate, dim3(1), dim3(64), 0, g_stream, sc, b.flags, b.hist, j, t, tol2);
            if (j + 1 < restart && t < iters)  // the cycle's last w starts no further step
                hipLaunchKernelGGL((gm_scale<T, V>), g, blk, 0, g_stream, n, fl, (const double *)(sc + kGmEta), w);
        }
        // the one read of the cycle: the stop state, the steps counted, the status
        int flags[kSolverFlagWords] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(flags, b.flags, sizeof(flags), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        const bool stopped = flags[kSolverState] != kSolverRun;
        res.steps = stopped ? flags[kSolverSteps] : t;
        res.status = flags[kSolverStatus];
        if (flags[kGmAtStart]) res.cycles = 0;  // b = 0 or a non-finite b.b: no cycle began
        const int J = res.steps - t0;  // the columns this cycle counted
        if (J < 0 || J > restart) return fail("%s: the device counted %d columns in a cycle of %d", what, J, restart);
        if (J > 0) {
            hipLaunchKernelGGL(gm_solve, dim3(1), dim3(1), 0, g_stream, sc, J);
            HIP_TRY(hipMemsetAsync(u, 0, (size_t)n * sizeof(T), g_stream));
            if (gm_update_launch<T>(n, nullptr, basis, b.ld, J, sc + kGmCoef, u, b.part, nullptr, local, what)) return -1;
            const T *du = u;
            if (P) {
                if (precond_apply<T>(P, u, z, nullptr, g_stream)) return -1;
                du = z;
            }
            hipLaunchKernelGGL((gm_add<T, V>), g, blk, 0, g_stream, n, du, x);
        }
        if (stopped || t >= iters) break;
        if (csr_launch_any(m, variant, x, q, g_stream)) return -1;  // q = A x
        if (residual()) return -1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int gm_body(spmv_csr_dev *m, const spmv_precond *P, int variant, int restart, int iters, double tol,
            const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total) {
    const size_t vb = sizeof(T), n = (size_t)m->M_total;
    SolverScope scope;
    // every vector a product or an apply reads: N values in whole 16-byte pieces and the 128-byte line tail the
    // x-window kernels read, in whole lines (a basis vector starts on a line); b, q: whole 16-byte pieces
    const size_t in_bytes = (((size_t)m->N * vb + 15) / 16 * 16 + kLineBytes + kLineBytes - 1) / kLineBytes * kLineBytes;
    const size_t vec_bytes = std::max<size_t>((n * vb + 15) / 16 * 16, 16);
    const int nbasis = std::min(restart, std::max(iters, 1)) + 1;  // v_0 .. v_J of the longest cycle
    GmBuffers b;
    b.ld = (long long)(in_bytes / vb);
    b.basis = scope.alloc((size_t)nbasis * in_bytes);
    b.x = scope.alloc(in_bytes);
    b.u = scope.alloc(in_bytes);
    b.z = P ? scope.alloc(in_bytes) : nullptr;
    b.b = scope.alloc(vec_bytes);
    b.q = scope.alloc(vec_bytes);
    b.sc = scope.alloc<double>(kGmSlots * sizeof(double));
    b.part = scope.alloc<double>((size_t)kGmBlocks * kGmMaxRestart * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    b.flags = scope.alloc<int>(kSolverFlagWords * sizeof(int));
    hipError_t e = scope.err;
    if (e == hipSuccess && n) e = hipMemcpyAsync(b.b, b_host, n * vb, hipMemcpyHostToDevice, g_stream);
    if (solver_begin(scope, e, "csr_gmres")) return -1;
    GmResult res;
    if (gm_run<T>(m, P, variant, restart, iters, tol, b, res)) return -1;
    if (solver_finish(scope, "csr_gmres", m->value_bytes, nullptr, b.x, x_host, n * vb, {{rr_hist, b.hist}}, res.steps,
                      iters, 1, nullptr, nullptr, 0, ms_total))
        return -1;
    if (info) info[0] = res.steps, info[1] = res.status, info[2] = res.cycles;
    return 0;
}

// what the two passes alone ask of their arguments
int gm_hook_check(const char *what, const void *d_V, long long ld, int nvec, const void *d_w, long long n,
                  int value_bytes) {
    if (!d_V || !d_w) return fail("%s: bad arguments", what);
    if (g_comm) return fail("%s: runs on one device, a communicator is active", what);
    if (value_bytes != 4 && value_bytes != 8) return fail("%s: value_bytes = %d, must be 4 or 8", what, value_bytes);
    if (n < 0) return fail("%s: n = %lld, must be >= 0", what, n);
    if (nvec < 1 || nvec > kGmMaxRestart) return fail("%s: nvec = %d, must be in [1, %d]", what, nvec, kGmMaxRestart);
    if (ld < n) return fail("%s: ld = %lld is below n = %lld", what, ld, n);
    if (ld * value_bytes % 16) return fail("%s: ld = %lld values of %d bytes is not a multiple of 16 bytes", what, ld, value_bytes);
    if (((uintptr_t)d_V | (uintptr_t)d_w) % 16) return fail("%s: the arrays are not aligned to 16 bytes", what);
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_gmres(spmv_csr_dev *m, const spmv_precond *P, int variant, int restart, int iters,
                                  double tol, const void *b_host, void *x_host, double *rr_hist, int *info,
                                  float *ms_total) {
    const char *what = "csr_gmres";
    if (need_device()) return -1;
    if (!m || !b_host) return fail("%s: bad arguments", what);
    if (restart < 1 || restart > kGmMaxRestart)
        return fail("%s: restart = %d, must be in [1, %d]", what, restart, kGmMaxRestart);
    if (solver_check_steps(what, iters, tol) || solver_check_square(what, m)) return -1;
    if (m->tiles_only) return fail("%s: a tiles-only handle runs the tile kernel only", what);
    if (m->row0 != 0 || m->M_local != m->M_total)
        return fail("%s: a handle of rows [%d, %d) is not the whole matrix", what, m->row0, m->row0 + m->M_local);
    if (g_comm) return fail("%s: runs on one device, a communicator is active", what);
    if (P && precond_matches(m, P, what)) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return gm_body<decltype(t)>(m, P, variant, restart, iters, tol, b_host, x_host, rr_hist, info, ms_total);
    });
}

extern "C" int spmv_hip_gmres_dots(const void *d_V, long long ld, int nvec, const void *d_w, long long n,
                                   int value_bytes, double *h_out_host) {
    const char *what = "gmres_dots";
    if (need_device()) return -1;
    if (gm_hook_check(what, d_V, ld, nvec, d_w, n, value_bytes)) return -1;
    if (!h_out_host) return fail("%s: bad arguments", what);
    return solver_dispatch(what, value_bytes, [&](auto t) {
        using T = decltype(t);
        SolverScope scope;
        double *part = scope.alloc<double>((size_t)kGmBlocks * kGmMaxRestart * sizeof(double));
        double *out = scope.alloc<double>((size_t)2 * kGmMaxRestart * sizeof(double));
        if (scope.err != hipSuccess) return solver_setup_failed(what, scope.err);
        if (gm_dots_launch<T>(n, nullptr, (const T *)d_V, ld, nvec, (const T *)d_w, part, out, out + kGmMaxRestart, what))
            return -1;
        HIP_TRY(hipMemcpyAsync(h_out_host, out, (size_t)nvec * sizeof(double), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    });
}

extern "C" int spmv_hip_gmres_update(const void *d_V, long long ld, int nvec, const double *h_host, void *d_w,
                                     long long n, int value_bytes, double *ww_out_host) {
    const char *what = "gmres_update";
    if (need_device()) return -1;
    if (gm_hook_check(what, d_V, ld, nvec, d_w, n, value_bytes)) return -1;
    if (!h_host) return fail("%s: bad arguments", what);
    return solver_dispatch(what, value_bytes, [&](auto t) {
        using T = decltype(t);
        SolverScope scope;
        double *part = scope.alloc<double>((size_t)kGmBlocks * sizeof(double));
        double *h = scope.alloc<double>((size_t)kGmMaxRestart * sizeof(double));
        double *out = scope.alloc<double>(2 * sizeof(double));
        if (scope.err != hipSuccess) return solver_setup_failed(what, scope.err);
        HIP_TRY(hipMemcpyAsync(h, h_host, (size_t)nvec * sizeof(double), hipMemcpyHostToDevice, g_stream));
        if (gm_update_launch<T>(n, nullptr, (const T *)d_V, ld, nvec, h, (T *)d_w, part, ww_out_host ? out : nullptr,
                                out + 1, what))
            return -1;
        if (ww_out_host) HIP_TRY(hipMemcpyAsync(ww_out_host, out, sizeof(double), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    });
}
