// spmv_amg.hip -- the smoothed-aggregation AMG preconditioner of a CSR handle: one V(1,1) cycle per apply
// (include/spmv_hip.h; the kernels are in amg_kernels.hpp, the setup in host/amg_plan.c).  spmv_amg_setup.hip makes the
// same object with the setup on the device; what the two share (the object, amg_finish, amg_wrap) is in amg_levels.hpp.
//
// The build, once per object:
//   1. the handle's diagonal block is downloaded and made canonical (canon_rows.hpp), as the triangular and FSAI builds do;
//   2. spmv_amg_plan_build makes the hierarchy on the host in fp64: A_l, P_l, R_l = P_l^T, w_l, the dense inverse of a
//      DIRECT coarsest level;
//   3. level 0 goes to the device through the normal upload (an ordinary whole rows x rows handle with whatever plan
//      upload picks), everything else as plain CSR arrays rounded once to the handle's dtype, g_l = w_l / d in fp64 with
//      d the rounded diagonal;
//   4. the cycle is written out as a list of passes (AmgStep) over vectors at fixed workspace offsets.
//
// The loop, with b the right-hand side of level l (level 0: r) and the result of level 0 written to z:
//
//   cycle(l, b):
//     DIRECT:        x = Ainv b                                                  (one amg_rows pass)
//     SMOOTH:        x = g.b;  x' = x + g.(b - A x)
//     not coarsest:  x = g.b;  r = b - A x;  b' = R r;  e = cycle(l + 1, b');  x = x + P e;  x' = x + g.(b - A x)
//
//   level 0:   A x is t = A_0 x by the handle's AUTO launch (k vectors: spmv_hip_csr_spmm_on), r = b - t and
//              z = x + g.(b - t) are element-wise passes (t is ready, so the second sweep needs no second vector)
//   level > 0: r = b - A x and x' = x + g.(b - A x) are fused amg_rows passes, x' a second vector
//   the tail:  with chain, the passes of every level from the first l > 0 with n_l <= 256 and nnz(A_l) <= 4096 on are
//              ONE launch of amg_tail (one workgroup); a single-level DIRECT hierarchy is that launch alone
//
// Vector v of a level has n_l rows and sits at offset off_v (values at k = 1) of the workspace, off_v a multiple of 32
// and 32 rows behind the vector's last: for k columns the vector is at k off_v, 128-byte aligned, with a line tail the
// x-window kernels may read (zero in P's own workspace; a caller's d_work should be zeroed once).  An apply allocates
// nothing and reads nothing back.
#include "amg_levels.hpp"

#include <memory>

#include "canon_rows.hpp"

namespace {

constexpr int kAmgSpmv = 100;  // a host-side pass: out = A_0 in through the level-0 handle

struct PlanGuard {
    spmv_amg_plan *p = nullptr;
    ~PlanGuard() { spmv_amg_plan_free(p); }
};

int plan_read(const spmv_amg_plan *plan, int level, int which, int rows, HostOp &h) {
    h.rp.assign((size_t)rows + 1, 0);
    if (spmv_amg_plan_level(plan, level, which, h.rp.data(), nullptr, nullptr, nullptr)) return fail("%s", spmv_amg_plan_error());
    const size_t nz = (size_t)h.rp[(size_t)rows];
    h.col.assign(std::max<size_t>(nz, 1), 0);
    h.val.assign(std::max<size_t>(nz, 1), 0.0);
    if (spmv_amg_plan_level(plan, level, which, h.rp.data(), h.col.data(), h.val.data(), nullptr))
        return fail("%s", spmv_amg_plan_error());
    h.col.resize(nz), h.val.resize(nz);
    return 0;
}

// rows of a vector in the workspace: a multiple of 32 and a spare 32 (a 128-byte line of fp32) behind the last value
long long vec_rows(int n) { return ((long long)n + 31) / 32 * 32 + 32; }

// the passes of level l on right-hand side vector b; returns the vector that holds the level's result
struct CycleWriter {
    spmv_amg_precond *ap;
    std::vector<int> level_of;  // per pass
    long long next = 0;
    long long take(int n) {
        const long long off = next;
        next += vec_rows(n);
        return off;
    }
    void push(int level, int op, int n, const AmgOp *M, const double *g, long long in, long long aux, long long b, long long out) {
        AmgStep s;
        s.op = op, s.n = n, s.G = M ? M->G : 1, s.pad = 0;
        s.rp = M ? M->rp : nullptr, s.col = M ? M->col : nullptr, s.val = M ? M->val : nullptr;
        s.g = g;
        s.in = in, s.aux = aux, s.b = b, s.out = out;
        ap->steps.push_back(s);
        level_of.push_back(level);
    }
    long long emit(int l, long long b) {
        const int n = ap->n[l], none = kAmgVecNone;
        const double *g = ap->g[l];
        if (ap->kind[l] == SPMV_AMG_DIRECT) {
            const long long x = l ? take(n) : (long long)kAmgVecZ;
            push(l, kAmgMul, n, &ap->inv, nullptr, b, none, none, x);
            return x;
        }
        const long long x = take(n), y = take(n);  // y: level 0's t = A x; below, r and then x'
        const bool last = ap->kind[l] == SPMV_AMG_SMOOTH;
        push(l, kAmgScale, n, nullptr, g, none, none, b, x);
        if (!last) {
            if (l == 0) {
                push(l, kAmgSpmv, n, nullptr, nullptr, x, none, none, y);
                push(l, kAmgSub, n, nullptr, nullptr, y, none, b, y);
            } else {
                push(l, kAmgResid, n, &ap->A[l], nullptr, x, none, b, y);
            }
            const long long bc = take(ap->n[l + 1]);
            push(l, kAmgMul, ap->n[l + 1], &ap->R[l], nullptr, y, none, none, bc);
            const long long e = emit(l + 1, bc);
            push(l, kAmgAdd, n, &ap->P[l], nullptr, e, none, none, x);
        }
        if (l == 0) {
            push(l, kAmgSpmv, n, nullptr, nullptr, x, none, none, y);
            push(l, kAmgAxpy, n, nullptr, g, x, y, b, kAmgVecZ);
            return kAmgVecZ;
        }
        push(l, kAmgSmooth, n, &ap->A[l], g, x, none, b, y);
        return y;
    }
};

template <typename T>
int amg_build(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels, int chain, spmv_precond **out) {
    const double t0 = now_ms();
    Canon A;
    if (canon_download<T>(m, A)) return -1;
    const int n = A.n;
    const double t1 = now_ms();
    PlanGuard plan;
    if (spmv_amg_plan_build(n, A.rp.data(), A.col.data(), A.val.data(), theta, coarse_rows, max_levels, &plan.p))
        return fail(kAmgMsgPlan, m->row0, spmv_amg_plan_error());
    const double t2 = now_ms();
    std::unique_ptr<spmv_amg_precond> ap(new spmv_amg_precond);
    ap->levels = spmv_amg_plan_levels(plan.p);
    ap->chain = chain != 0;
    HostOp h;
    for (int l = 0; l < ap->levels; ++l) {
        double sc[5];
        if (spmv_amg_plan_level(plan.p, l, SPMV_AMG_A, nullptr, nullptr, nullptr, sc)) return fail("%s", spmv_amg_plan_error());
        ap->w[l] = sc[0], ap->rho[l] = sc[1], ap->kind[l] = (int)sc[2], ap->n[l] = (int)sc[3], ap->na[l] = (int)sc[4];
        const int nl = ap->n[l];
        if (plan_read(plan.p, l, SPMV_AMG_A, nl, h)) return -1;
        ap->a_nz[l] = (long long)h.col.size();
        // g = w / d with d as the device holds it
        std::vector<double> g((size_t)nl, 0.0);
        for (int i = 0; i < nl; ++i)
            for (int e = h.rp[i]; e < h.rp[i + 1]; ++e)
                if (h.col[e] == i) g[i] = ap->w[l] / (double)(T)h.val[e];
        for (int i = 0; i < nl; ++i)
            if (!std::isfinite(g[i]))
                return fail(kAmgMsgDiagonal, l, i);
        if (to_device(&ap->g[l], g)) return -1;
        if (l == 0 && ap->kind[0] != SPMV_AMG_DIRECT) {
            int rc;
            if constexpr (sizeof(T) == 8) {
                rc = spmv_hip_csr_upload(n, n, h.rp.data(), h.col.data(), h.val.data(), 0, n, &ap->A0);
            } else {
                std::vector<float> v(h.val.begin(), h.val.end());
                rc = spmv_hip_csr_upload_f32(n, n, h.rp.data(), h.col.data(), v.data(), 0, n, &ap->A0);
            }
            if (rc) return -1;
        } else if (amg_op_upload<T>(h, nl, ap->A[l], "A", l)) {
            return -1;
        }
        if (ap->kind[l] == SPMV_AMG_DIRECT) {
            if (plan_read(plan.p, l, SPMV_AMG_INV, nl, h) || amg_op_upload<T>(h, nl, ap->inv, "the inverse", l)) return -1;
        } else if (ap->kind[l] == SPMV_AMG_NOT_COARSEST) {
            if (plan_read(plan.p, l, SPMV_AMG_P, nl, h) || amg_op_upload<T>(h, nl, ap->P[l], "P", l)) return -1;
            if (plan_read(plan.p, l, SPMV_AMG_R, ap->na[l], h) || amg_op_upload<T>(h, ap->na[l], ap->R[l], "R", l)) return -1;
        }
    }
    if (amg_finish(ap.get(), (int)sizeof(T))) return -1;
    ap->us[0] = (int)((t1 - t0) * 1e3);
    ap->us[1] = (int)((t2 - t1) * 1e3);
    ap->us[2] = (int)((now_ms() - t2) * 1e3);
    *out = amg_wrap(m, ap.release(), sizeof(T));
    return 0;
}

template <typename T>
int amg_run(const spmv_amg_precond *ap, int k, const void *R, void *Z, void *work, hipStream_t s) {
    T *w = (T *)work;
    const int ns = (int)ap->steps.size();
    for (int q = 0; q < ns; ++q) {
        const AmgStep &st = ap->steps[q];
        if (q == ap->tail0) {
            hipLaunchKernelGGL((amg_tail<T>), dim3(1), dim3(kBlock), 0, s, (const AmgStep *)ap->d_steps, ap->tail0, ap->tail1,
                               k, w, (const T *)R, (T *)Z);
            q = ap->tail1 - 1;
            continue;
        }
        if (st.op == kAmgSpmv) {
            if (spmv_hip_csr_spmm_on(ap->A0, k, w + st.in * k, w + st.out * k, s)) return -1;  // k = 1: the AUTO launch
            continue;
        }
        const long long threads = st.op <= kAmgAxpy ? (long long)st.n * k : (long long)st.n * st.G;
        const int grid = (int)std::max<long long>(1, std::min<long long>(kAmgBlocks, (threads + kBlock - 1) / kBlock));
        hipLaunchKernelGGL((amg_pass<T>), dim3(grid), dim3(kBlock), 0, s, st, k, w, (const T *)R, (T *)Z);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// z = one V(1,1) cycle on r by P's own launches on stream s, the level vectors P's own (as FSAI's, they do not look at a
// solver's flags)
int amg_apply(const spmv_precond *P, const void *r, void *z, const int *, hipStream_t s) {
    const spmv_amg_precond *ap = (const spmv_amg_precond *)P->impl;
    if (!P->rows) return 0;
    return P->value_bytes == 8 ? amg_run<double>(ap, 1, r, z, ap->work, s) : amg_run<float>(ap, 1, r, z, ap->work, s);
}

// Z = M^-1 R for rows x k row-major R and Z; work: work_values * k values (the level vectors; the part behind each
// vector's values zero), P's own vectors are not used
int amg_apply_multi(const spmv_precond *P, int k, const void *R, void *Z, void *work, hipStream_t s) {
    const spmv_amg_precond *ap = (const spmv_amg_precond *)P->impl;
    if (!P->rows) return 0;
    return P->value_bytes == 8 ? amg_run<double>(ap, k, R, Z, work, s) : amg_run<float>(ap, k, R, Z, work, s);
}

long long amg_work_bytes(const spmv_precond *P, int k) {
    return std::max<long long>(((const spmv_amg_precond *)P->impl)->work_values * k * P->value_bytes, 16);
}

const precond_family kAmgFamily = {"AMG", "an AMG apply needs d_work (spmv_hip_precond_work_bytes: its level vectors)",
                                   amg_apply, amg_apply_multi, amg_work_bytes, nullptr,
                                   [](void *impl) { delete (spmv_amg_precond *)impl; }};

}  // namespace

int amg_finish(spmv_amg_precond *ap, int value_bytes) {
    if (!ap->levels) return 0;
    ap->coarsest = ap->kind[ap->levels - 1];
    CycleWriter cw{ap, {}, 0};
    cw.emit(0, kAmgVecR);
    ap->work_values = std::max<long long>(cw.next, 32);
    // the chained tail: the passes of the levels from the first narrow one below 0 on
    int lc = -1;
    for (int l = 1; l < ap->levels && lc < 0; ++l)
        if (ap->n[l] <= kAmgChainRows && ap->a_nz[l] <= kAmgChainEntries) lc = l;
    if (ap->levels == 1 && ap->coarsest == SPMV_AMG_DIRECT) lc = 0;
    const int ns = (int)ap->steps.size();
    if (lc >= 0 && ap->chain) {
        ap->first_chained = lc;
        for (int q = 0; q < ns; ++q)
            if (cw.level_of[q] >= lc) {
                if (ap->tail0 < 0) ap->tail0 = q;
                ap->tail1 = q + 1;
            }
    }
    ap->launches = ns - (ap->tail0 >= 0 ? ap->tail1 - ap->tail0 - 1 : 0);
    if (upload_array(&ap->d_steps, ap->steps.data(), (size_t)ns, 0)) return -1;
    const size_t bytes = (size_t)ap->work_values * (size_t)value_bytes;
    hipError_t e = hipMalloc(&ap->work, bytes);
    if (e == hipSuccess) e = hipMemset(ap->work, 0, bytes);
    if (e != hipSuccess) return fail("csr_precond_build_amg: allocation failed: %s", hipGetErrorString(e));
    return 0;
}

spmv_precond *amg_wrap(const spmv_csr_dev *m, spmv_amg_precond *ap, size_t value_bytes) {
    return precond_new(m, SPMV_PRECOND_AMG, 1, value_bytes, &kAmgFamily, ap);
}

const spmv_amg_precond *amg_of(const spmv_precond *P, const char *what) {
    return (const spmv_amg_precond *)precond_impl(P, &kAmgFamily, what);
}

extern "C" int spmv_hip_csr_precond_build_amg(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels,
                                              int chain, spmv_precond **out) {
    auto check = [&] { return amg_check_args(theta, coarse_rows, max_levels); };
    return precond_build_frame("csr_precond_build_amg", m, out, check, [&](auto t, spmv_precond **P) {
        return amg_build<decltype(t)>(m, theta, coarse_rows, max_levels, chain, P);
    });
}

extern "C" int spmv_hip_precond_amg_info(const spmv_precond *P, int *info) {
    if (!P || !info) return fail("precond_amg_info: bad arguments");
    const spmv_amg_precond *ap = amg_of(P, "precond_amg_info");
    if (!ap) return -1;
    long long total = 0;
    for (int l = 0; l < ap->levels; ++l) total += ap->a_nz[l];
    std::fill(info, info + SPMV_PRECOND_AMG_INFO_WORDS, 0);
    info[0] = ap->levels;
    info[1] = ap->first_chained;
    info[2] = ap->launches;
    info[3] = ap->coarsest;
    info[4] = ap->levels && ap->a_nz[0] ? (int)(total * 1000 / ap->a_nz[0]) : 0;
    info[5] = ap->us[0], info[6] = ap->us[1], info[7] = ap->us[2];
    info[8] = ap->chain;
    for (int l = 0; l < ap->levels; ++l) {
        info[9 + l] = ap->n[l];
        info[9 + kAmgMaxLevels + l] = (int)std::min<long long>(ap->a_nz[l], 0x7fffffff);
    }
    return 0;
}

extern "C" int spmv_hip_precond_amg_level(const spmv_precond *P, int level, int which, int *row_ptr, int *col, void *val,
                                          double *scalars) {
    if (need_device()) return -1;
    if (!P) return fail("precond_amg_level: bad arguments");
    const spmv_amg_precond *ap = amg_of(P, "precond_amg_level");
    if (!ap) return -1;
    if (level < 0 || level >= ap->levels) return fail("precond_amg_level: no level %d (the hierarchy has %d)", level, ap->levels);
    if (scalars) {
        scalars[0] = ap->w[level], scalars[1] = ap->rho[level], scalars[2] = ap->kind[level];
        scalars[3] = ap->n[level], scalars[4] = ap->na[level];
    }
    if (!row_ptr) return 0;
    const int *d_rp = nullptr, *d_col = nullptr;
    const void *d_val = nullptr;
    int rows = ap->n[level];
    if (which == SPMV_AMG_A && level == 0 && ap->A0) {
        d_rp = ap->A0->row_ptr, d_col = ap->A0->col, d_val = ap->A0->val;
    } else {
        const AmgOp *op = which == SPMV_AMG_A ? &ap->A[level] : which == SPMV_AMG_P ? &ap->P[level]
                        : which == SPMV_AMG_R ? &ap->R[level]
                        : which == SPMV_AMG_INV && ap->kind[level] == SPMV_AMG_DIRECT ? &ap->inv : nullptr;
        if (!op) return fail("precond_amg_level: which = %d at level %d", which, level);
        if (!op->rp) return fail("precond_amg_level: level %d is the coarsest, it has no P or R", level);
        d_rp = op->rp, d_col = op->col, d_val = op->val, rows = op->rows;
    }
    HIP_TRY(hipMemcpy(row_ptr, d_rp, ((size_t)rows + 1) * sizeof(int), hipMemcpyDeviceToHost));
    const size_t nz = (size_t)row_ptr[rows];
    if (col && val && nz) {
        HIP_TRY(hipMemcpy(col, d_col, nz * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(val, d_val, nz * (size_t)P->value_bytes, hipMemcpyDeviceToHost));
    }
    return 0;
}
