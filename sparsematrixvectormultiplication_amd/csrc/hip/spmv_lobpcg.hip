// spmv_lobpcg.hip -- spmv_hip_csr_lobpcg: LOBPCG for a few extreme eigenpairs of a symmetric fp64 CSR handle, and the two
// dense passes on their own (include/spmv_hip.h; the kernels are in lobpcg_kernels.hpp, the Rayleigh-Ritz step in
// csrc/host/lobpcg_rr.c).
//
//     X = X0; AX = A X; (theta, C) = rr(X^T X, X^T AX); X = X C; AX = AX C
//     per step:  W = AX - X diag(theta) with ||w_j||; stop rules; W = M^-1 W; AW = A W (one SpMM);
//                G_B = S^T S, G_A = S^T AS over S = [X | W | P], AS = [AX | AW | AP] (one pass, fp64 MFMA);
//                (theta, C, Cp) = rr(G_B, G_A) on the host; X = S C, P = S Cp, AX = AS C, AP = AS Cp (one pass, in place)
//
// The host reads the residual norms and the Gram matrices in every step, so the loop is host-driven: the stop state,
// the histories and theta live on the host, theta and the coefficients are uploaded per step.  With a preconditioner
// the residual goes to a buffer of its own and the k-wide apply writes W.
#include "spmv_internal.hpp"

#include <chrono>
#include <cmath>

#include "lobpcg_kernels.hpp"
#include "precond_kernels.hpp"

namespace {

constexpr double kLobDrop = 1e-10;  // basis directions below drop * the largest are dropped (spmv_lobpcg_rr)

int lob_gram_tiles(int m) { return (m + 15) / 16; }

// workgroups of the Gram pass over n rows
int lob_gram_grid(long long n) {
    return solver_grid(kLobGramBlocks, (n + 3) / 4, kBlock / 64);  // a wave takes a group of 4 rows
}

// G_B and G_A of the first nb blocks -> out[0 .. 2 MP^2) on the device (MP = 16 tiles(m); the lower tiles of G_B stay 0);
// part: grid x 2 MP^2 doubles; what a call of another shape left in it is overwritten or, in G_B's lower tiles, never read
int lob_gram_launch(long long n, int k, int nb, const double *const *S, const double *const *AS, double *part, double *out) {
    const int m = nb * k, mt = lob_gram_tiles(m), mp = 16 * mt, grid = lob_gram_grid(n);
    const double *s1 = nb > 1 ? S[1] : nullptr, *s2 = nb > 2 ? S[2] : nullptr;
    const double *a1 = nb > 1 ? AS[1] : nullptr, *a2 = nb > 2 ? AS[2] : nullptr;
    const dim3 g(grid), blk(kBlock);
    if (mt == 1) hipLaunchKernelGGL(lob_gram<1>, g, blk, 0, g_stream, n, k, m, S[0], s1, s2, AS[0], a1, a2, part);
    else if (mt == 2) hipLaunchKernelGGL(lob_gram<2>, g, blk, 0, g_stream, n, k, m, S[0], s1, s2, AS[0], a1, a2, part);
    else hipLaunchKernelGGL(lob_gram<3>, g, blk, 0, g_stream, n, k, m, S[0], s1, s2, AS[0], a1, a2, part);
    hipLaunchKernelGGL(solver_fold, dim3(2 * mp * mp), blk, 0, g_stream, part, grid, 2 * mp * mp, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the folded tiles (host copy) -> GB, GA (m x m row-major); G_B's lower triangle is its upper one
void lob_gram_unpack(const double *folded, int m, double *GB, double *GA) {
    const int mp = 16 * lob_gram_tiles(m);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            GB[i * m + j] = folded[std::min(i, j) * mp + std::max(i, j)];
            GA[i * m + j] = folded[mp * mp + i * mp + j];
        }
}

template <int NB, bool VEC>
void lob_update_vec(long long n, int k, const double *const *S, const double *const *AS, const double *coef, double *X,
                    double *P, double *AX, double *AP) {
    const int grid = solver_grid(kLobUpdateBlocks, n, kBlock);
    const double *s1 = NB > 1 ? S[1] : nullptr, *s2 = NB > 2 ? S[2] : nullptr;
    const double *a1 = NB > 1 ? AS[1] : nullptr, *a2 = NB > 2 ? AS[2] : nullptr;
    const dim3 g(grid), blk(kBlock);
    if (k <= 4) hipLaunchKernelGGL((lob_update<NB, 4, VEC>), g, blk, 0, g_stream, n, k, S[0], s1, s2, AS[0], a1, a2, coef, X, P, AX, AP);
    else if (k <= 8) hipLaunchKernelGGL((lob_update<NB, 8, VEC>), g, blk, 0, g_stream, n, k, S[0], s1, s2, AS[0], a1, a2, coef, X, P, AX, AP);
    else hipLaunchKernelGGL((lob_update<NB, 16, VEC>), g, blk, 0, g_stream, n, k, S[0], s1, s2, AS[0], a1, a2, coef, X, P, AX, AP);
}

// 16-byte pieces when a row of k values is whole pieces and every array is 16-byte aligned
template <int NB>
void lob_update_nb(long long n, int k, const double *const *S, const double *const *AS, const double *coef, double *X,
                   double *P, double *AX, double *AP) {
    uintptr_t bits = (uintptr_t)X | (uintptr_t)P | (uintptr_t)AX | (uintptr_t)AP;
    for (int b = 0; b < NB; ++b) bits |= (uintptr_t)S[b] | (uintptr_t)AS[b];
    if (k % 2 == 0 && (bits & 15) == 0) lob_update_vec<NB, true>(n, k, S, AS, coef, X, P, AX, AP);
    else lob_update_vec<NB, false>(n, k, S, AS, coef, X, P, AX, AP);
}

// coef: nb k x k pairs {C, Cp} on the device
int lob_update_launch(long long n, int k, int nb, const double *const *S, const double *const *AS, const double *coef,
                      double *X, double *P, double *AX, double *AP) {
    if (nb == 1) lob_update_nb<1>(n, k, S, AS, coef, X, P, AX, AP);
    else if (nb == 2) lob_update_nb<2>(n, k, S, AS, coef, X, P, AX, AP);
    else lob_update_nb<3>(n, k, S, AS, coef, X, P, AX, AP);
    HIP_TRY(hipGetLastError());
    return 0;
}

// {C[c][j], Cp[c][j]} pairs, element (c, j) at 2 (c k + j)
void lob_pack_coef(int m, int k, const double *C, const double *Cp, std::vector<double> &coef) {
    coef.resize((size_t)2 * m * k);
    for (int i = 0; i < m * k; ++i) coef[2 * i] = C[i], coef[2 * i + 1] = Cp[i];
}

int lob_hook_check(long long n, int k, int nb, const void *const *S, const void *const *AS, const char *what) {
    if (n < 0 || !S || !AS) return fail("%s: bad arguments", what);
    if (k < 1 || k > kLobMaxK) return fail("%s: k = %d, must be in [1, %d]", what, k, kLobMaxK);
    if (nb < 1 || nb > kLobMaxBlocks) return fail("%s: nb = %d, must be in [1, %d]", what, nb, kLobMaxBlocks);
    if (n * k > 0x7fffffffLL) return fail("%s: n * k = %lld values is beyond int range", what, n * k);
    for (int b = 0; b < nb; ++b) {
        if (!S[b] || !AS[b]) return fail("%s: block %d is NULL", what, b);
        if (((uintptr_t)S[b] | (uintptr_t)AS[b]) % sizeof(double)) return fail("%s: block %d is not aligned to 8 bytes", what, b);
    }
    return 0;
}

struct LobBuffers {
    double *X, *W, *P, *AX, *AW, *AP;
    double *R;     // with a preconditioner: the residual, W is M^-1 R
    void *work;    // the workspace of the k-wide apply (precond_work_bytes)
    double *theta, *coef, *res_part, *res_sum, *gram_part, *gram_out, *an_part, *an_out;
};

struct LobResult {
    int steps = 0, status = SPMV_LOBPCG_RAN_ALL, restarts = 0, min_basis = 0;
    double host_ms = 0;
};

int lob_run(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, int largest, const LobBuffers &b,
            double anorm, std::vector<double> &theta, double *theta_hist, double *res_hist, double *resid, LobResult &out) {
    const long long n = m->M_total;
    const size_t kk = (size_t)k;
    const bool wide = k % 2 == 0;
    const int V = wide ? 2 : 1, cl = mcg_column_lanes(k, V);  // the residual pass walks as cg_multi's kernels do
    const int rgrid = solver_grid(kMcgBlocks, n, kBlock >> cl);
    std::vector<double> folded((size_t)2 * 48 * 48), GB((size_t)48 * 48), GA((size_t)48 * 48), C((size_t)48 * 16),
        Cp((size_t)48 * 16), coef, rsum(kk);
    // ||AX - X diag(theta)||_2 per column -> rsum (the host waits); R: where the residual goes (nullptr: nowhere)
    auto residual = [&](const double *AX, double *R) {
        HIP_TRY(hipMemcpyAsync(b.theta, theta.data(), kk * sizeof(double), hipMemcpyHostToDevice, g_stream));
        if (wide) hipLaunchKernelGGL(lob_residual<2>, dim3(rgrid), dim3(kBlock), 0, g_stream, n, k, cl, b.theta, b.X, AX, R, b.res_part);
        else hipLaunchKernelGGL(lob_residual<1>, dim3(rgrid), dim3(kBlock), 0, g_stream, n, k, cl, b.theta, b.X, AX, R, b.res_part);
        hipLaunchKernelGGL(solver_fold, dim3(k), dim3(kBlock), 0, g_stream, b.res_part, rgrid, k, b.res_sum);
        HIP_TRY(hipMemcpyAsync(rsum.data(), b.res_sum, kk * sizeof(double), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        for (size_t j = 0; j < kk; ++j) rsum[j] = std::sqrt(rsum[j]);
        return 0;
    };
    // the Gram pass over nb blocks and the Rayleigh-Ritz step; *broke = 1: a breakdown, X is not to be touched
    auto gram_rr = [&](int nb, int *broke) {
        const double *S[3] = {b.X, b.W, b.P}, *AS[3] = {b.AX, b.AW, b.AP};
        const int mm = nb * k, mp = 16 * lob_gram_tiles(mm);
        if (lob_gram_launch(n, k, nb, S, AS, b.gram_part, b.gram_out)) return -1;
        HIP_TRY(hipMemcpyAsync(folded.data(), b.gram_out, (size_t)2 * mp * mp * sizeof(double), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        lob_gram_unpack(folded.data(), mm, GB.data(), GA.data());
        const auto t0 = std::chrono::steady_clock::now();
        int kept = 0, restarted = 0;
        std::vector<double> th(kk);
        const int rc = spmv_lobpcg_rr(nb, k, GB.data(), GA.data(), largest, kLobDrop, th.data(), C.data(), Cp.data(), &kept,
                                      &restarted);
        out.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc < 0) return fail("csr_lobpcg: the Rayleigh-Ritz step refused its arguments");
        out.min_basis = std::min(out.min_basis, kept);
        *broke = rc != 0;
        if (rc) return 0;
        theta = th;
        out.restarts += restarted;
        lob_pack_coef(mm, k, C.data(), Cp.data(), coef);
        HIP_TRY(hipMemcpyAsync(b.coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, g_stream));
        return lob_update_launch(n, k, nb, S, AS, b.coef, b.X, b.P, b.AX, b.AP);
    };
    auto record = [&](int t) {
        if (theta_hist) std::memcpy(theta_hist + (size_t)t * kk, theta.data(), kk * sizeof(double));
        if (res_hist) std::memcpy(res_hist + (size_t)t * kk, rsum.data(), kk * sizeof(double));
    };
    out.min_basis = k;
    int broke = 0;
    if (spmv_hip_csr_spmm_on(m, k, b.X, b.AX, g_stream)) return -1;
    if (gram_rr(1, &broke)) return -1;
    if (broke) {  // X0 has no k independent finite columns: w and X are zeros
        out.status = SPMV_LOBPCG_BREAKDOWN;
        std::fill(theta.begin(), theta.end(), 0.0);
        std::fill(rsum.begin(), rsum.end(), 0.0);
        HIP_TRY(hipMemsetAsync(b.X, 0, (size_t)n * kk * sizeof(double), g_stream));
        for (int t = 0; t <= iters; ++t) record(t);
        if (resid) std::memset(resid, 0, kk * sizeof(double));
        return 0;
    }
    double *R = pc ? b.R : b.W;
    int t = 0;
    for (;; ++t) {
        if (residual(b.AX, R)) return -1;
        bool finite = true, small = true;
        for (size_t j = 0; j < kk; ++j) {
            finite = finite && std::isfinite(rsum[j]);
            small = small && rsum[j] <= tol * anorm;
        }
        record(t);
        if (!finite) {
            out.status = SPMV_LOBPCG_BREAKDOWN;
            break;
        }
        if (tol > 0 && small) {
            out.status = SPMV_LOBPCG_CONVERGED;
            break;
        }
        if (t == iters) {
            out.status = SPMV_LOBPCG_RAN_ALL;
            break;
        }
        if (pc && spmv_hip_precond_apply_multi_on(pc, k, b.R, b.W, b.work, g_stream)) return -1;
        if (spmv_hip_csr_spmm_on(m, k, b.W, b.AW, g_stream)) return -1;
        if (gram_rr(t == 0 ? 2 : 3, &broke)) return -1;
        if (broke) {
            out.status = SPMV_LOBPCG_BREAKDOWN;
            break;
        }
    }
    out.steps = t;
    for (int r = t + 1; r <= iters; ++r) {  // after a stop both histories repeat their last row
        if (theta_hist) std::memcpy(theta_hist + (size_t)r * kk, theta_hist + (size_t)t * kk, kk * sizeof(double));
        if (res_hist) std::memcpy(res_hist + (size_t)r * kk, res_hist + (size_t)t * kk, kk * sizeof(double));
    }
    // the true residual of what is returned
    if (spmv_hip_csr_spmm_on(m, k, b.X, b.AW, g_stream)) return -1;
    if (residual(b.AW, nullptr)) return -1;
    if (resid) std::memcpy(resid, rsum.data(), kk * sizeof(double));
    return 0;
}

int lob_body(spmv_csr_dev *m, const spmv_precond *pc, int k, int iters, double tol, int largest, const double *X0_host,
             double *w, double *X_host, double *theta_hist, double *res_hist, double *resid, double *anorm_out,
             int *info, float *ms_out, float *host_ms) {
    const size_t n = (size_t)m->M_total, kk = (size_t)k;
    // every block may feed a product: at k = 1 the x-window SpMV kernels read whole 128-byte lines
    const size_t vec_bytes = std::max<size_t>(n * kk * sizeof(double), 16) + kLineBytes;
    const int mp_max = 16 * lob_gram_tiles(3 * k);
    SolverScope scope;
    LobBuffers b;
    b.X = scope.alloc<double>(vec_bytes);
    b.W = scope.alloc<double>(vec_bytes);
    b.P = scope.alloc<double>(vec_bytes);
    b.AX = scope.alloc<double>(vec_bytes);
    b.AW = scope.alloc<double>(vec_bytes);
    b.AP = scope.alloc<double>(vec_bytes);
    b.R = pc ? scope.alloc<double>(vec_bytes) : nullptr;
    b.work = precond_work_alloc(scope, pc, k);
    b.theta = scope.alloc<double>(kLobMaxK * sizeof(double));
    b.coef = scope.alloc<double>((size_t)2 * 48 * kLobMaxK * sizeof(double));
    b.res_part = scope.alloc<double>((size_t)kMcgBlocks * kLobMaxK * sizeof(double));
    b.res_sum = scope.alloc<double>(kLobMaxK * sizeof(double));
    const size_t part_doubles = (size_t)lob_gram_grid((long long)n) * 2 * mp_max * mp_max;  // the widest shape's
    b.gram_part = scope.alloc<double>(part_doubles * sizeof(double));
    b.gram_out = scope.alloc<double>((size_t)2 * mp_max * mp_max * sizeof(double));
    b.an_part = scope.alloc<double>((size_t)kNormBlocks * sizeof(double));
    b.an_out = scope.alloc<double>(sizeof(double));
    // (not solver_begin: the timed part has always included the copy of X0)
    hipError_t e = scope.err;
    if (e == hipSuccess) e = hipEventRecord(scope.e0, g_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.X, X0_host, n * kk * sizeof(double), hipMemcpyHostToDevice, g_stream);
    if (e != hipSuccess) return solver_setup_failed("csr_lobpcg", e);
    // anorm = ||A||_inf
    const int agrid = solver_grid(kNormBlocks, (long long)n, kBlock);
    hipLaunchKernelGGL(lob_row_abs_max, dim3(agrid), dim3(kBlock), 0, g_stream, (long long)n, m->row_ptr,
                       (const double *)m->val, b.an_part);
    hipLaunchKernelGGL(lob_max, dim3(1), dim3(kBlock), 0, g_stream, b.an_part, agrid, b.an_out);
    double anorm = 0;
    HIP_TRY(hipMemcpyAsync(&anorm, b.an_out, sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    LobResult res;
    std::vector<double> theta(kk, 0.0);
    if (lob_run(m, pc, k, iters, tol, largest, b, anorm, theta, theta_hist, res_hist, resid, res)) return -1;
    // X alone comes from the device here: the histories and the stop state are the host's
    if (solver_finish(scope, "csr_lobpcg", 8, nullptr, b.X, X_host, n * kk * sizeof(double), {}, 0, 0, 0, nullptr, nullptr, 0,
                      ms_out))
        return -1;
    if (w) std::memcpy(w, theta.data(), kk * sizeof(double));
    if (anorm_out) *anorm_out = anorm;
    if (info) info[0] = res.steps, info[1] = res.status, info[2] = res.restarts, info[3] = res.min_basis;
    if (host_ms) *host_ms = (float)res.host_ms;
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_lobpcg(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol, int largest,
                                   const double *X0_host, double *w, double *X_host, double *theta_hist,
                                   double *res_hist, double *resid, double *anorm, int *info, float *ms, float *host_ms) {
    const char *what = "csr_lobpcg";
    if (need_device()) return -1;
    int rc = 0;
    if (!m || !X0_host) rc = fail("%s: bad arguments", what);
    else if (m->value_bytes != 8) rc = fail("%s: needs an fp64 handle", what);
    else if (solver_check_square(what, m)) rc = -1;
    else if (m->tiles_only) rc = fail("%s: a tiles-only handle has no SpMM kernels", what);
    else if (m->row0 != 0 || m->M_local != m->M_total)
        rc = fail("%s: a handle of rows [%d, %d) is not the whole matrix", what, m->row0, m->row0 + m->M_local);
    else if (g_comm) rc = fail("%s: runs on one device, a communicator is active", what);
    else if (k < 1 || k > kLobMaxK) rc = fail("%s: k = %d, must be in [1, %d]", what, k, kLobMaxK);
    else if (m->M_total < 4 * k) rc = fail("%s: n = %d, must be >= 4 k = %d", what, m->M_total, 4 * k);
    else if (solver_check_steps(what, iters, tol)) rc = -1;
    else if ((long long)m->M_total * k > 0x7fffffffLL)
        rc = fail("%s: n * k = %lld values is beyond int range", what, (long long)m->M_total * k);
    else if (P && precond_refuse_one_wide(P, what)) rc = -1;
    else if (P && largest) rc = fail("%s: a preconditioner serves the smallest eigenvalues only", what);
    else if (P) rc = precond_matches(m, P, what);
    if (rc) return rc;
    return guarded(what, [&] {
        return lob_body(m, P, k, iters, tol, largest, X0_host, w, X_host, theta_hist, res_hist, resid, anorm, info, ms, host_ms);
    });
}

extern "C" int spmv_hip_lobpcg_gram(long long n, int k, int nb, const void *const *d_S, const void *const *d_AS,
                                    double *GB_host, double *GA_host) {
    const char *what = "lobpcg_gram";
    if (need_device()) return -1;
    if (lob_hook_check(n, k, nb, d_S, d_AS, what)) return -1;
    if (!GB_host || !GA_host) return fail("%s: bad arguments", what);
    return guarded(what, [&] {
        const int m = nb * k, mp = 16 * lob_gram_tiles(m);
        SolverScope scope;
        double *part = scope.alloc<double>((size_t)lob_gram_grid(n) * 2 * mp * mp * sizeof(double));
        double *out = scope.alloc<double>((size_t)2 * mp * mp * sizeof(double));
        if (scope.err != hipSuccess) return solver_setup_failed(what, scope.err);
        if (lob_gram_launch(n, k, nb, (const double *const *)d_S, (const double *const *)d_AS, part, out)) return -1;
        std::vector<double> folded((size_t)2 * mp * mp);
        HIP_TRY(hipMemcpyAsync(folded.data(), out, folded.size() * sizeof(double), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        lob_gram_unpack(folded.data(), m, GB_host, GA_host);
        return 0;
    });
}

extern "C" int spmv_hip_lobpcg_update(long long n, int k, int nb, const void *const *d_S, const void *const *d_AS,
                                      const double *C_host, const double *Cp_host, void *d_X, void *d_P, void *d_AX,
                                      void *d_AP) {
    const char *what = "lobpcg_update";
    if (need_device()) return -1;
    if (lob_hook_check(n, k, nb, d_S, d_AS, what)) return -1;
    if (!C_host || !Cp_host || !d_X || !d_P || !d_AX || !d_AP) return fail("%s: bad arguments", what);
    if (((uintptr_t)d_X | (uintptr_t)d_P | (uintptr_t)d_AX | (uintptr_t)d_AP) % sizeof(double))
        return fail("%s: the outputs are not aligned to 8 bytes", what);
    return guarded(what, [&] {
        const int m = nb * k;
        std::vector<double> coef;
        lob_pack_coef(m, k, C_host, Cp_host, coef);
        SolverScope scope;
        double *d_coef = scope.alloc<double>(coef.size() * sizeof(double));
        if (scope.err != hipSuccess) return solver_setup_failed(what, scope.err);
        HIP_TRY(hipMemcpyAsync(d_coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, g_stream));
        if (lob_update_launch(n, k, nb, (const double *const *)d_S, (const double *const *)d_AS, d_coef, (double *)d_X,
                              (double *)d_P, (double *)d_AX, (double *)d_AP))
            return -1;
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    });
}
