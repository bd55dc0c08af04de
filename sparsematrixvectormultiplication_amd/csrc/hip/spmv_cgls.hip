// spmv_cgls.hip -- spmv_hip_csr_cgls: CGLS for min ||A x - b||^2 + damp^2 ||x||^2 on a CSR handle and its transpose,
// entirely on the device (include/spmv_hip.h).
//
//     x = 0; r = b; s = A^T r; p = s; gamma = gamma0 = s.s; rr0 = r.r
//     per step:  q = A p; delta = q.q + damp^2 p.p; alpha = gamma / delta; x += alpha p; r -= alpha q
//                s = A^T r - damp^2 x; gamma' = s.s (stop if gamma' <= tol^2 gamma0); beta = gamma' / gamma; p = s + beta p
//
// The two products are the handles' own SpMVs (csr_launch_any with AUTO): A p through m, A^T r through mt, on
// library-owned p and r, each sized and padded as its handle's x (the 128-byte line tail the x-window kernels read).
// p, s, x have N rows and q, r have M.  The vector and scalar kernels are in cgls_kernels.hpp; the scalars and the
// stop state never leave the device.  Single device: the handles hold whole matrices.
#include "spmv_internal.hpp"

#include "cgls_kernels.hpp"

namespace {

struct CglsBuffers {
    void *p, *q, *r, *s, *x;
    double *sc, *part, *ss_hist, *rr_hist;
    int *flags;
};

// the vector kernels' grid over n rows in pieces of V
int cgls_grid(long long n, int V) { return solver_grid(kCglsBlocks, (n + V - 1) / V, kBlock); }

// the loop; *steps_run = the steps launched (< iters when tol > 0 and the solve stopped)
template <typename T>
int cgls_run(spmv_csr_dev *m, spmv_csr_dev *mt, int iters, double tol, double damp, const CglsBuffers &b,
             int *steps_run) {
    constexpr int V = 16 / sizeof(T);
    const long long M = m->M_total, N = m->N;
    const int gM = cgls_grid(M, V), gN = cgls_grid(N, V), gMN = cgls_grid(std::max(M, N), V);
    const double tol2 = tol * tol, damp2 = damp * damp;
    T *p = (T *)b.p, *q = (T *)b.q, *r = (T *)b.r, *s = (T *)b.s, *x = (T *)b.x;
    const int *fl = b.flags;
    const dim3 blk(kBlock);
    // the grid's partials -> sc[slot].  This rank's sums only: the handles hold whole matrices, so there is nothing to
    // add over ranks even when a communicator exists.
    auto fold = [&](int grid, int slot) {
        hipLaunchKernelGGL(solver_fold, dim3(1), blk, 0, g_stream, (const double *)b.part, grid, 1, b.sc + slot);
    };
    // rr0 = r.r with r = b; s = A^T r, gamma0 = s.s; p = s
    hipLaunchKernelGGL((cgls_norm2<T, V>), dim3(gM), blk, 0, g_stream, M, fl, (const T *)r, b.part);
    fold(gM, kCglsRr);
    if (csr_launch_any(mt, SPMV_CSR_AUTO, r, s, g_stream)) return -1;
    hipLaunchKernelGGL((cgls_norm2<T, V>), dim3(gN), blk, 0, g_stream, N, fl, (const T *)s, b.part);
    fold(gN, kCglsSs);
    if (N) HIP_TRY(hipMemcpyAsync(p, s, (size_t)N * sizeof(T), hipMemcpyDeviceToDevice, g_stream));
    hipLaunchKernelGGL(cgls_start, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.ss_hist, b.rr_hist, iters);
    *steps_run = iters;
    for (int k = 1; k <= iters; ++k) {
        if (csr_launch_any(m, SPMV_CSR_AUTO, p, q, g_stream)) return -1;  // q = A p
        hipLaunchKernelGGL((cgls_norm2<T, V>), dim3(gM), blk, 0, g_stream, M, fl, (const T *)q, b.part);
        fold(gM, kCglsQq);
        hipLaunchKernelGGL(cgls_set_alpha, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, k, damp2);
        hipLaunchKernelGGL((cgls_update_x_r<T, V>), dim3(gMN), blk, 0, g_stream, N, M, fl, (const double *)b.sc,
                           (const T *)p, (const T *)q, x, r, b.part);
        fold(gMN, kCglsRr);
        if (csr_launch_any(mt, SPMV_CSR_AUTO, r, s, g_stream)) return -1;  // s = A^T r
        if (damp > 0)
            hipLaunchKernelGGL((cgls_update_s<T, V>), dim3(gN), blk, 0, g_stream, N, fl, damp2, (const T *)x, s, b.part);
        else
            hipLaunchKernelGGL((cgls_norm2<T, V>), dim3(gN), blk, 0, g_stream, N, fl, (const T *)s, b.part);
        fold(gN, kCglsSs);
        hipLaunchKernelGGL(cgls_set_beta, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.ss_hist, b.rr_hist, k, tol2);
        // p.p feeds the next step's delta only when damp > 0
        hipLaunchKernelGGL((cgls_update_p<T, V>), dim3(gN), blk, 0, g_stream, N, fl, (const double *)b.sc,
                           (const T *)s, p, damp > 0 ? b.part : nullptr);
        if (damp > 0) fold(gN, kCglsPp);
        bool stop = false;
        if (solver_poll(k, iters, tol, b.flags + kSolverState, kSolverStop, &stop)) return -1;
        if (stop) {
            *steps_run = k;
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int cgls_body(spmv_csr_dev *m, spmv_csr_dev *mt, int iters, double tol, double damp, const void *b_host,
              void *x_host, double *ss_hist, double *rr_hist, int *info, float *ms_total) {
    const size_t vb = sizeof(T), M = (size_t)m->M_total, N = (size_t)m->N;
    const size_t hist_bytes = ((size_t)iters + 1) * sizeof(double);
    SolverScope scope;
    // p (m's x), r (mt's x): read in whole 128-byte lines by the x-window kernels; q, s, x: whole 16-byte pieces
    const size_t p_bytes = (N * vb + 15) / 16 * 16 + kLineBytes, r_bytes = (M * vb + 15) / 16 * 16 + kLineBytes;
    const size_t vecM = std::max<size_t>((M * vb + 15) / 16 * 16, 16), vecN = std::max<size_t>((N * vb + 15) / 16 * 16, 16);
    CglsBuffers b;
    b.p = scope.alloc(p_bytes);
    b.r = scope.alloc(r_bytes);
    b.q = scope.alloc(vecM);
    b.s = scope.alloc(vecN);
    b.x = scope.alloc(vecN);
    b.sc = scope.alloc<double>(kCglsSlots * sizeof(double));
    b.part = scope.alloc<double>((size_t)kCglsBlocks * sizeof(double));
    b.ss_hist = scope.alloc<double>(hist_bytes);
    b.rr_hist = scope.alloc<double>(hist_bytes);
    b.flags = scope.alloc<int>(kSolverFlagWords * sizeof(int));
    hipError_t e = scope.err;
    if (e == hipSuccess && M) e = hipMemcpyAsync(b.r, b_host, M * vb, hipMemcpyHostToDevice, g_stream);
    if (solver_begin(scope, e, "csr_cgls")) return -1;
    int steps_run = 0;
    if (cgls_run<T>(m, mt, iters, tol, damp, b, &steps_run)) return -1;
    // no bounds: the handles hold whole matrices, x is whole on every rank
    int flags[kSolverFlagWords] = {0, 0, 0, 0};
    if (solver_finish(scope, "csr_cgls", m->value_bytes, nullptr, b.x, x_host, N * vb,
                      {{ss_hist, b.ss_hist}, {rr_hist, b.rr_hist}}, steps_run, iters, 1, b.flags, flags, kSolverFlagWords,
                      ms_total))
        return -1;
    if (info) {
        info[0] = flags[kSolverSteps];
        info[1] = flags[kSolverStatus];
    }
    return 0;
}

// a handle CGLS can launch by itself: the whole matrix, with its CSR arrays
int cgls_whole(const spmv_csr_dev *h, const char *which) {
    if (h->row0 != 0 || h->M_local != h->M_total)
        return fail("csr_cgls: %s holds rows [%d, %d) of %d; CGLS takes whole matrices", which, h->row0,
                    h->row0 + h->M_local, h->M_total);
    if (h->tiles_only) return fail("csr_cgls: %s is a tiles-only handle", which);
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_cgls(spmv_csr_dev *m, spmv_csr_dev *mt, int iters, double tol, double damp,
                                 const void *b_host, void *x_host, double *ss_hist, double *rr_hist, int *info,
                                 float *ms_total) {
    if (need_device()) return -1;
    int rc = 0;
    if (!m || !mt || !b_host) rc = fail("csr_cgls: bad arguments");
    else if (solver_check_steps("csr_cgls", iters, tol)) rc = -1;
    else if (!(damp >= 0) || !std::isfinite(damp)) rc = fail("csr_cgls: damp = %g, must be finite and >= 0", damp);
    else if (cgls_whole(m, "A") || cgls_whole(mt, "A^T")) rc = -1;
    else if (mt->M_total != m->N || mt->N != m->M_total)
        rc = fail("csr_cgls: A^T is %d x %d, A is %d x %d: not its transpose", mt->M_total, mt->N, m->M_total, m->N);
    else if (mt->nz != m->nz) rc = fail("csr_cgls: A^T has %lld entries, A %lld: not its transpose", mt->nz, m->nz);
    else if (mt->value_bytes != m->value_bytes)
        rc = fail("csr_cgls: A^T holds %d-byte values, A %d-byte: not its transpose", mt->value_bytes, m->value_bytes);
    if (rc) return rc;
    return solver_dispatch("csr_cgls", m->value_bytes, [&](auto t) {
        return cgls_body<decltype(t)>(m, mt, iters, tol, damp, b_host, x_host, ss_hist, rr_hist, info, ms_total);
    });
}
