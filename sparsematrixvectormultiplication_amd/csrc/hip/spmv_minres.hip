// spmv_minres.hip -- spmv_hip_csr_minres: MINRES on a CSR handle, entirely on the device (include/spmv_hip.h).
//
//     r1 = r2 = b; y = M^-1 r2 (or r2); bb0 = r2.y; beta = sqrt(bb0); phibar = beta; cs = -1; the rest 0
//     per step:  v = y / beta; t = A v - shift v - (beta / oldb) r1; alfa = v.t; t -= (alfa / beta) r2
//                r1 = r2; r2 = t; y = M^-1 r2 (or r2); bb = r2.y; the rotation; w = (v - oldeps w1 - delta w2) / gamma
//                x += phi w
//
// The product is the handle's SpMV (csr_launch_any) on library-owned v: full length with the 128-byte line tail the
// x-window kernels read, as the handle's own x.  a = A v, the two r buffers, the two w buffers, y and x are indexed by
// global row; this rank works on its rows [row0, row0 + M_local).  t is written over r1's buffer and w over w1's, so
// the host swaps the two r pointers and the two w pointers after every step.  The vector and scalar kernels are in
// minres_kernels.hpp; the scalars and the stop state never leave the device.  With a communicator the next v is
// all-gathered with the row bounds after mr_update (one exchange per step) and every reduction is all-gathered and
// added in rank order, as csr_bicgstab does: every rank holds the same bits and stops at the same step.
//
// With a preconditioner y = M^-1 r2 is an apply of its own after mr_lanczos_b (precond_apply: a pc_apply pass for Jacobi
// and block-Jacobi, the kind's own launches for the rest) followed by mr_dot for r2.y.
// Without one y is r2 itself and mr_lanczos_b's t.t is bb: no apply, no extra dot.
#include "spmv_internal.hpp"

#include "minres_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

struct MrBuffers {
    void *v, *a, *r[2], *w[2], *x;
    void *y;  // with a preconditioner: M^-1 r2
    double *sc, *part, *gath, *hist;
    int *flags;
};

// the loop; *steps_run = the steps launched (< iters when tol > 0 and the solve stopped)
template <typename T>
int mr_run(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, double shift,
           const int *bounds, const MrBuffers &b, int *steps_run) {
    constexpr int V = 16 / sizeof(T);
    const long long lo = m->row0, hi = (long long)m->row0 + m->M_local;
    const int grid = solver_grid(kMrBlocks, (hi + V - 1) / V - lo / V, kBlock);  // over the 16-byte pieces
    const double tol2 = tol * tol;
    T *v = (T *)b.v, *a = (T *)b.a, *x = (T *)b.x, *yb = (T *)b.y;
    T *r1 = (T *)b.r[0], *r2 = (T *)b.r[1], *w1 = (T *)b.w[0], *w2 = (T *)b.w[1];
    const int *fl = b.flags;
    const double *sc = b.sc;
    const dim3 g(grid), blk(kBlock);
    const long long own = lo;  // P's local row 0 in the global vectors
    // part[0 .. grid) of this rank -> the global sum in sc[slot] on every rank
    auto reduce = [&](int slot) {
        return solver_reduce(b.part, grid, 1, b.sc + slot, b.sc + kMrLocal, b.gath, "csr_minres");
    };
    // y = M^-1 r on this rank's rows and bb = r.y in slot kMrBb
    auto apply_and_dot = [&](const T *r) {
        if (precond_apply<T>(P, r + own, yb + own, fl, g_stream)) return -1;
        hipLaunchKernelGGL((mr_dot<T, V>), g, blk, 0, g_stream, lo, hi, fl, r, (const T *)yb, b.part);
        return reduce(kMrBb);
    };
    if (P) {
        if (apply_and_dot(r2)) return -1;
    } else {
        hipLaunchKernelGGL((mr_dot<T, V>), g, blk, 0, g_stream, lo, hi, fl, (const T *)r2, (const T *)r2, b.part);
        if (reduce(kMrBb)) return -1;
    }
    hipLaunchKernelGGL(mr_start, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hist, iters);
    hipLaunchKernelGGL((mr_update<T, V>), g, blk, 0, g_stream, lo, hi, fl, sc, 0, (const T *)(P ? yb : r2),
                       (const T *)w2, w1, x, v);  // v = y / beta
    if (g_comm && spmv_hip_comm_allgatherv(v, bounds, m->value_bytes, g_stream)) return -1;
    *steps_run = iters;
    for (int k = 1; k <= iters; ++k) {
        if (csr_launch_any(m, variant, v, a, g_stream)) return -1;  // a = A v on this rank's rows
        hipLaunchKernelGGL((mr_lanczos_a<T, V>), g, blk, 0, g_stream, lo, hi, fl, sc, k, shift, (const T *)a,
                           (const T *)v, r1, b.part);
        if (reduce(kMrAlfa)) return -1;
        hipLaunchKernelGGL(mr_set_alfa, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, k);
        hipLaunchKernelGGL((mr_lanczos_b<T, V>), g, blk, 0, g_stream, lo, hi, fl, sc, (const T *)r2, r1, b.part);
        if (reduce(kMrBb)) return -1;
        std::swap(r1, r2);  // r1 = r2; r2 = t
        if (P && apply_and_dot(r2)) return -1;
        hipLaunchKernelGGL(mr_rotate, dim3(1), dim3(1), 0, g_stream, b.sc, b.flags, b.hist, k, tol2);
        hipLaunchKernelGGL((mr_update<T, V>), g, blk, 0, g_stream, lo, hi, fl, sc, k, (const T *)(P ? yb : r2),
                           (const T *)w2, w1, x, v);
        std::swap(w1, w2);  // w1 = w2; w2 = w
        if (g_comm && spmv_hip_comm_allgatherv(v, bounds, m->value_bytes, g_stream)) return -1;
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
int mr_body(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, double shift,
            const int *bounds, const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total) {
    const size_t vb = sizeof(T), n_all = (size_t)m->M_total, n_own = (size_t)m->M_local;
    SolverScope scope;
    // v: the SpMV input, read in whole 128-byte lines by the x-window kernels; the rest: whole 16-byte pieces
    const size_t in_bytes = ((size_t)m->N * vb + 15) / 16 * 16 + kLineBytes;
    const size_t vec_bytes = std::max<size_t>((n_all * vb + 15) / 16 * 16, 16);
    MrBuffers b;
    b.v = scope.alloc(in_bytes);
    b.a = scope.alloc(vec_bytes);
    b.r[0] = scope.alloc(vec_bytes);
    b.r[1] = scope.alloc(vec_bytes);
    b.w[0] = scope.alloc(vec_bytes);
    b.w[1] = scope.alloc(vec_bytes);
    b.x = scope.alloc(vec_bytes);
    b.y = P ? scope.alloc(vec_bytes) : nullptr;
    b.sc = scope.alloc<double>(kMrSlots * sizeof(double));
    b.part = scope.alloc<double>((size_t)kMrBlocks * sizeof(double));
    b.gath = scope.alloc<double>((size_t)kMaxRanks * sizeof(double));
    b.hist = scope.alloc<double>(((size_t)iters + 1) * sizeof(double));
    b.flags = scope.alloc<int>(kSolverFlagWords * sizeof(int));
    // r2 = b on this rank's rows (r1 is first read at step 2, after step 1 made it r2)
    const size_t own_off = (size_t)m->row0 * vb, own_bytes = n_own * vb;
    hipError_t e = scope.err;
    if (e == hipSuccess && n_own)
        e = hipMemcpyAsync((char *)b.r[1] + own_off, (const char *)b_host + own_off, own_bytes, hipMemcpyHostToDevice,
                           g_stream);
    if (solver_begin(scope, e, "csr_minres")) return -1;
    int steps_run = 0;
    if (mr_run<T>(m, P, variant, iters, tol, shift, bounds, b, &steps_run)) return -1;
    int flags[kSolverFlagWords] = {0, 0, 0, 0};
    if (solver_finish(scope, "csr_minres", m->value_bytes, bounds, b.x, x_host, n_all * vb, {{rr_hist, b.hist}}, steps_run,
                      iters, 1, b.flags, flags, kSolverFlagWords, ms_total))
        return -1;
    if (info) {
        info[0] = flags[kSolverSteps];
        info[1] = flags[kSolverStatus];
    }
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_minres(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol,
                                   double shift, const int *bounds, const void *b_host, void *x_host, double *rr_hist,
                                   int *info, float *ms_total) {
    const char *what = "csr_minres";
    if (need_device()) return -1;
    if (!m || !b_host) return fail("%s: bad arguments", what);
    if (solver_check_steps(what, iters, tol)) return -1;
    if (!std::isfinite(shift)) return fail("%s: shift = %g, must be finite", what, shift);
    if (solver_check_square(what, m)) return -1;
    if (m->tiles_only) return fail("%s: a tiles-only handle runs the tile kernel only", what);
    if (solver_check_rows(what, m, bounds)) return -1;
    if (P && precond_matches(m, P, what)) return -1;
    return solver_dispatch(what, m->value_bytes, [&](auto t) {
        return mr_body<decltype(t)>(m, P, variant, iters, tol, shift, bounds, b_host, x_host, rr_hist, info, ms_total);
    });
}
