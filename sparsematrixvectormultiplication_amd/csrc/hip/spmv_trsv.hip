// spmv_trsv.hip -- sparse triangular solves on CSR handles and the two preconditioners made of them, SSOR and ILU(0)
// (include/spmv_hip.h; the kernels are in trsv_kernels.hpp, the level analysis and the colouring in host/trsv_plan.c).
//
// The build, once per object, on the host except for the factorisation:
//   1. the handle's CSR arrays are downloaded and the diagonal block A[row0:row1, row0:row1] is made canonical
//      (canon_rows.hpp, shared with spmv_fsai.hip): local columns, every row sorted by column (a stable sort), entries
//      that repeat a column added in entry order in fp64;
//   2. ordering MULTICOLOR: spmv_trsv_colour, the rows ordered by (colour, row), the canonical matrix permuted;
//   3. spmv_trsv_levels on each triangle: levels, the level order, the launch plan;
//   4. ILU(0) only: the canonical matrix goes to the device in fp64 and ilu0_level / ilu0_chain factor it in place with
//      the forward solve's plan; the factors come back and are rounded once to the handle's dtype;
//   5. the triangles are stored in level order (TrsvView) and uploaded.
// A solve is the plan's launches on one stream and nothing else: no host read, no allocation.
//
// The apply of a preconditioner is two solves through P's own vector y (so one P serves one stream at a time):
//   ILU(0)   L y = r (unit diagonal), U z = y
//   SSOR     (D/w + L) y = r, then z_i = s y_i - (w / d_i) sum_j u_ij z_j with s = (2 - w) / w, which is
//            (D/w + U) z = s (D/w) y without forming the right-hand side (w = 1 on a diagonal matrix: Jacobi's bytes)
// With the multicolour order the forward solve reads r through the order and the backward solve writes z through it
// (its columns are stored in the caller's numbering), so no kernel exists only to permute.
#include "spmv_internal.hpp"

#include <climits>
#include <cmath>
#include <memory>

#include "canon_rows.hpp"
#include "precond_kernels.hpp"
#include "trsv_kernels.hpp"

namespace {

struct TriPlan {
    std::vector<int> perm, level_ptr, level_split, plan;  // plan: {kind, first level, end level} per launch
    int levels = 0, launches = 0, widest = 0, median = 0;
    long long entries = 0;
};

struct TriDev {  // one triangle on the device
    int n = 0, levels = 0, launches = 0, widest = 0, median = 0, G = 1;
    long long entries = 0;
    int *rp = nullptr, *col = nullptr, *brow = nullptr, *xrow = nullptr, *level_ptr = nullptr, *level_split = nullptr;
    void *val = nullptr, *dinv = nullptr;
    std::vector<int> plan;  // {kind, first level, end level, grid} per launch
    TriDev() = default;
    TriDev(const TriDev &) = delete;
    TriDev &operator=(const TriDev &) = delete;
    ~TriDev() {
        for (void *p : {(void *)rp, (void *)col, (void *)brow, (void *)xrow, (void *)level_ptr, (void *)level_split, val,
                        dinv})
            (void)hipFree(p);
    }
    spmv::TrsvView view() const { return {rp, col, brow, xrow, level_ptr, level_split, val, dinv}; }
};

// What an object's first refresh builds (tri_refresh_analyse) and every later one runs on: the canonical (and, for the
// multicolour order, permuted) diagonal block B as a pattern, which entries of the handle feed each of its entries, and
// where each entry goes in the triangles' level order.  All on the device; an object that is never refreshed has none.
struct TriRefresh {
    long long nzb = 0;                      // entries of B
    int *fp = nullptr, *feed = nullptr;     // entry e of B = the handle's entries feed[fp[e] .. fp[e + 1]) added in that order
    int *rp = nullptr, *col = nullptr, *diag = nullptr;  // B (rp, col: ILU(0) only; diag: NULL for a unit triangular solve)
    int *src[2] = {nullptr, nullptr};       // per slot of the lower / upper triangle's val: the entry of B
    int *urow = nullptr;                    // the upper triangle's rows of B in its level order (the lower one's: its xrow)
    std::vector<int> fwd_level_ptr;         // ILU(0): the forward plan's level_ptr, for the factorisation's grids
    TriRefresh() = default;
    TriRefresh(const TriRefresh &) = delete;
    TriRefresh &operator=(const TriRefresh &) = delete;
    ~TriRefresh() {
        for (int *p : {fp, feed, rp, col, diag, src[0], src[1], urow}) (void)hipFree(p);
    }
};

// B = Q A Q^T with row k of B = row order[k] of A
void canon_permute(const Canon &A, const std::vector<int> &order, Canon &B) {
    const int n = A.n;
    std::vector<int> inv((size_t)n);
    for (int k = 0; k < n; ++k) inv[order[k]] = k;
    B.n = n;
    B.rp.assign((size_t)n + 1, 0);
    B.diag.assign((size_t)n, -1);
    B.col.resize(A.col.size());
    B.val.resize(A.val.size());
    std::vector<std::pair<int, double>> row;
    int out = 0;
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        row.clear();
        for (int e = A.rp[i]; e < A.rp[i + 1]; ++e) row.emplace_back(inv[A.col[e]], A.val[e]);
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (const auto &cv : row) {
            if (cv.first == k) B.diag[k] = out;
            B.col[out] = cv.first;
            B.val[out++] = cv.second;
        }
        B.rp[k + 1] = out;
    }
}

int tri_analyse(const Canon &B, int uplo, TriPlan &p) {
    const size_t n = (size_t)B.n;
    std::vector<int> level(n + 1);
    p.perm.assign(n + 1, 0);
    p.level_ptr.assign(n + 1, 0);
    p.level_split.assign(n + 1, 0);
    p.plan.assign(3 * n + 3, 0);
    long long counts[4] = {0, 0, 0, 0};
    if (spmv_trsv_levels(B.n, B.rp.data(), B.col.data(), uplo, spmv::kTrsvLong, spmv::kTrsvChainRows,
                         spmv::kTrsvChainEntries, level.data(), p.perm.data(), p.level_ptr.data(), p.level_split.data(),
                         p.plan.data(), counts))
        return fail("trsv: the level analysis failed (out of host memory)");
    p.levels = (int)counts[0];
    p.launches = (int)counts[1];
    p.widest = (int)counts[2];
    p.entries = counts[3];
    p.level_ptr.resize((size_t)p.levels + 1);
    p.level_split.resize(std::max<size_t>((size_t)p.levels, 1));
    p.plan.resize(3 * (size_t)p.launches);
    std::vector<int> width((size_t)p.levels);
    for (int l = 0; l < p.levels; ++l) width[l] = p.level_ptr[l + 1] - p.level_ptr[l];
    std::sort(width.begin(), width.end());
    p.median = p.levels ? width[(size_t)p.levels / 2] : 0;
    return 0;
}

// the triangle of B on side uplo in level order.  dinv: by row of B (NULL: unit diagonal).  bmap / xmap (NULL: the
// identity): the element of b row i reads, the element of x it writes; the columns are mapped like x.
template <typename T>
int tri_upload(const Canon &B, int uplo, const TriPlan &p, const T *dinv, const int *bmap, const int *xmap, TriDev &t) {
    const int n = B.n;
    const bool lower = uplo == SPMV_TRSV_LOWER;
    std::vector<int> rp((size_t)n + 1, 0), col((size_t)p.entries), brow((size_t)n), xrow((size_t)n);
    std::vector<T> val((size_t)p.entries), dv(dinv ? (size_t)n : 0);
    long long short_rows = 0, short_entries = 0;
    int out = 0;
    for (int q = 0; q < n; ++q) {
        const int i = p.perm[q];
        for (int e = B.rp[i]; e < B.rp[i + 1]; ++e) {
            const int c = B.col[e];
            if (lower ? c >= i : c <= i) continue;
            col[out] = xmap ? xmap[c] : c;
            val[out++] = (T)B.val[e];
        }
        rp[q + 1] = out;
        brow[q] = bmap ? bmap[i] : i;
        xrow[q] = xmap ? xmap[i] : i;
        if (dinv) dv[q] = dinv[i];
        if (out - rp[q] < spmv::kTrsvLong) ++short_rows, short_entries += out - rp[q];
    }
    const double mean = short_rows ? (double)short_entries / (double)short_rows : 0.0;
    int G = 1;
    while (G < 32 && 2 * G < mean) G *= 2;  // about half a short row's entries per lane
    t.n = n;
    t.G = G;
    t.levels = p.levels, t.launches = p.launches, t.widest = p.widest, t.median = p.median, t.entries = p.entries;
    for (int k = 0; k < p.launches; ++k) {
        const int kind = p.plan[3 * k], l0 = p.plan[3 * k + 1], l1 = p.plan[3 * k + 2];
        long long threads = 0;
        if (!kind) {
            const long long ns = p.level_split[l0] - p.level_ptr[l0], nl = p.level_ptr[l0 + 1] - p.level_split[l0];
            threads = std::max(ns * G, nl * 64);
        }
        const int grid = solver_grid(spmv::kTrsvBlocks, threads, kBlock);
        t.plan.insert(t.plan.end(), {kind, l0, l1, grid});
    }
    if (to_device(&t.rp, rp) || to_device(&t.col, col) || to_device(&t.brow, brow) || to_device(&t.xrow, xrow) ||
        to_device(&t.level_ptr, p.level_ptr) || to_device(&t.level_split, p.level_split))
        return -1;
    if (upload_array((T **)&t.val, val.data(), val.size(), val.empty() ? 4 : 0)) return -1;
    if (dinv && upload_array((T **)&t.dinv, dv.data(), dv.size(), dv.empty() ? 4 : 0)) return -1;
    return 0;
}

template <typename T, bool SCALED>
void tri_launch(const TriDev &t, double scale, const int *flags, const T *b, T *x, hipStream_t s) {
    const spmv::TrsvView v = t.view();
    for (size_t k = 0; k < t.plan.size(); k += 4) {
        if (t.plan[k])
            hipLaunchKernelGGL((spmv::trsv_chain<T, SCALED>), dim3(1), dim3(kBlock), 0, s, v, t.plan[k + 1],
                               t.plan[k + 2], t.G, scale, flags, b, x);
        else
            hipLaunchKernelGGL((spmv::trsv_level<T, SCALED>), dim3(t.plan[k + 3]), dim3(kBlock), 0, s, v, t.plan[k + 1],
                               t.G, scale, flags, b, x);
    }
}

}  // namespace

// ---------------------------------------------------------------- the objects
struct spmv_trsv {
    TriDev t;
    int rows = 0, row0 = 0, value_bytes = 8;
    int analysis_us = 0, upload_us = 0;
    int uplo = SPMV_TRSV_LOWER, diag = SPMV_TRSV_NONUNIT;
    std::unique_ptr<TriRefresh> rf;  // spmv_hip_trsv_refresh's maps, from the first refresh on
    PatternStamp stamp;              // ... and the pattern they were made from
};

struct spmv_tri_precond {
    TriDev fwd, bwd;
    void *y = nullptr;  // the vector between the two solves
    bool scaled = false;
    double scale = 1.0, omega = 1.0;
    std::unique_ptr<TriRefresh> rf;  // the refresh's maps, from the first refresh on
    int colours = 0;
    int analysis_us = 0, factor_us = 0, upload_us = 0;
    bool unit_lower = false;  // ILU(0): L's diagonal is 1
    std::vector<double> diag;  // the diagonal (ILU(0): U's) by row of the permuted matrix; the device keeps only its
                               // inverse, everything else spmv_hip_precond_factors reads back from the triangles
    std::vector<int> order;    // row k of the permuted matrix = row order[k] of the handle (empty: the identity)
    ~spmv_tri_precond() { (void)hipFree(y); }
};

namespace {

extern const precond_family kTriFamily;  // at the end of the file, behind the functions it names

template <typename T>
int trsv_build(const spmv_csr_dev *m, int uplo, int diag, spmv_trsv **out) {
    const double t0 = now_ms();
    Canon A;
    if (canon_download<T>(m, A)) return -1;
    std::vector<T> dinv;
    if (diag == SPMV_TRSV_NONUNIT) {
        dinv.resize((size_t)A.n);
        for (int i = 0; i < A.n; ++i) {
            if (A.diag[i] < 0)
                return fail("csr_trsv_build: row %d (global row %d) has no diagonal entry", i, m->row0 + i);
            const double d = A.val[A.diag[i]];
            dinv[i] = (T)(1.0 / d);
            if (d == 0.0 || !std::isfinite(d) || !std::isfinite((double)dinv[i]))
                return fail("csr_trsv_build: row %d (global row %d): the diagonal is zero or not finite, or so small "
                            "that its inverse is not finite", i, m->row0 + i);
        }
    }
    TriPlan p;
    if (tri_analyse(A, uplo, p)) return -1;
    const double t1 = now_ms();
    std::unique_ptr<spmv_trsv> S(new spmv_trsv);
    if (tri_upload<T>(A, uplo, p, dinv.empty() ? nullptr : dinv.data(), nullptr, nullptr, S->t)) return -1;
    S->rows = A.n, S->row0 = m->row0, S->value_bytes = (int)sizeof(T);
    S->uplo = uplo, S->diag = diag;
    S->analysis_us = (int)((t1 - t0) * 1e3);
    S->upload_us = (int)((now_ms() - t1) * 1e3);
    *out = S.release();
    return 0;
}

// the numerical ILU(0) of B in place (B.val) with the forward plan p
int ilu0_factor(Canon &B, const TriPlan &p, const std::vector<int> &order, int row0) {
    const int n = B.n;
    if (!n) return 0;
    int *rp = nullptr, *col = nullptr, *diag = nullptr, *perm = nullptr, *lptr = nullptr, *bad = nullptr;
    double *W = nullptr;
    int rc = -1;
    do {
        std::vector<int> perm_h(p.perm.begin(), p.perm.begin() + n);
        if (to_device(&rp, B.rp) || to_device(&col, B.col) || to_device(&diag, B.diag) || to_device(&perm, perm_h) ||
            to_device(&lptr, p.level_ptr) || to_device(&W, B.val))
            break;
        const int none = INT_MAX;
        if (upload_array(&bad, &none, 1, 0)) break;
        for (int k = 0; k < p.launches; ++k) {
            const int l0 = p.plan[3 * k + 1], l1 = p.plan[3 * k + 2];
            if (p.plan[3 * k]) {
                hipLaunchKernelGGL(spmv::ilu0_chain, dim3(1), dim3(kBlock), 0, g_stream, l0, l1, (const int *)lptr,
                                   (const int *)perm, (const int *)rp, (const int *)col, (const int *)diag, W, bad);
            } else {
                const int p0 = p.level_ptr[l0], p1 = p.level_ptr[l1];
                const int grid = std::min(spmv::kTrsvBlocks, (p1 - p0 + kBlock / 64 - 1) / (kBlock / 64));
                hipLaunchKernelGGL(spmv::ilu0_level, dim3(grid), dim3(kBlock), 0, g_stream, p0, p1, (const int *)perm,
                                   (const int *)rp, (const int *)col, (const int *)diag, W, bad);
            }
        }
        int h = INT_MAX;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e == hipSuccess) e = hipMemcpy(&h, bad, sizeof h, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(B.val.data(), W, B.val.size() * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            fail("csr_precond_build_tri: the factorisation failed: %s", hipGetErrorString(e));
            break;
        }
        if (h != INT_MAX) {
            const int i = order.empty() ? h : order[h];
            fail("csr_precond_build_tri: row %d (global row %d): ILU(0) meets a zero or non-finite pivot", i, row0 + i);
            break;
        }
        rc = 0;
    } while (0);
    for (void *q : {(void *)rp, (void *)col, (void *)diag, (void *)perm, (void *)lptr, (void *)bad, (void *)W})
        (void)hipFree(q);
    (void)hipGetLastError();
    return rc;
}

template <typename T>
int tri_precond_build(const spmv_csr_dev *m, int kind, int ordering, double omega, spmv_precond **out) {
    const double t0 = now_ms();
    std::unique_ptr<spmv_tri_precond> tp(new spmv_tri_precond);
    Canon B;
    {
        Canon A;
        if (canon_download<T>(m, A)) return -1;
        const int miss = first_missing_diag(A);
        if (miss >= 0)
            return fail("csr_precond_build_tri: row %d (global row %d) has no diagonal entry", miss, m->row0 + miss);
        if (ordering == SPMV_ORDER_MULTICOLOR) {
            std::vector<int> colour((size_t)A.n + 1);
            tp->order.assign((size_t)A.n + 1, 0);
            tp->colours = spmv_trsv_colour(A.n, A.rp.data(), A.col.data(), colour.data(), tp->order.data());
            if (tp->colours < 0) return fail("csr_precond_build_tri: the colouring failed (out of host memory)");
            tp->order.resize((size_t)A.n);
            canon_permute(A, tp->order, B);
        } else {
            B = std::move(A);
        }
    }
    const int n = B.n;
    const int *order = tp->order.empty() ? nullptr : tp->order.data();
    auto original = [&](int k) { return order ? order[k] : k; };
    TriPlan pl, pu;
    if (tri_analyse(B, SPMV_TRSV_LOWER, pl) || tri_analyse(B, SPMV_TRSV_UPPER, pu)) return -1;
    const double t1 = now_ms();
    std::vector<T> dinv((size_t)n);
    if (kind == SPMV_PRECOND_SSOR) {
        for (int k = 0; k < n; ++k) {
            const double d = B.val[B.diag[k]];
            dinv[k] = (T)(omega / d);
            if (d == 0.0 || !std::isfinite(d) || !std::isfinite((double)dinv[k]))
                return fail("csr_precond_build_tri: row %d (global row %d): the diagonal is zero or not finite, or so "
                            "small that its inverse is not finite", original(k), m->row0 + original(k));
        }
        tp->scaled = true;
        tp->scale = (2.0 - omega) / omega;
        tp->omega = omega;
    } else {
        if (ilu0_factor(B, pl, tp->order, m->row0)) return -1;
        for (int k = 0; k < n; ++k) {
            dinv[k] = (T)(1.0 / (double)(T)B.val[B.diag[k]]);  // the inverse of the diagonal as it is returned
            if (!std::isfinite((double)dinv[k]))
                return fail("csr_precond_build_tri: row %d (global row %d): the pivot's inverse is not finite",
                            original(k), m->row0 + original(k));
        }
        tp->unit_lower = true;
    }
    const double t2 = now_ms();
    // forward: reads r in the caller's numbering, writes y in B's; backward: reads y, writes z in the caller's
    if (tri_upload<T>(B, SPMV_TRSV_LOWER, pl, tp->unit_lower ? nullptr : dinv.data(), order, nullptr, tp->fwd)) return -1;
    if (tri_upload<T>(B, SPMV_TRSV_UPPER, pu, dinv.data(), nullptr, order, tp->bwd)) return -1;
    HIP_TRY(hipMalloc(&tp->y, std::max<size_t>((size_t)n * sizeof(T), 16)));  // the forward solve writes all of it
    tp->diag.resize((size_t)n);
    for (int k = 0; k < n; ++k) tp->diag[k] = B.val[B.diag[k]];
    tp->analysis_us = (int)((t1 - t0) * 1e3);
    tp->factor_us = (int)((t2 - t1) * 1e3);
    tp->upload_us = (int)((now_ms() - t2) * 1e3);
    *out = precond_new(m, kind, 1, sizeof(T), &kTriFamily, tp.release());
    return 0;
}

// ---------------------------------------------------------------- refresh: new values, the symbolic work kept
int not_the_pattern(const char *what) {
    return fail("%s: the handle's pattern is not the one this object was built from: a changed pattern needs a new build", what);
}

// The first refresh's analysis, a host pass over m's pattern (no value comes back): the canonical block as
// canon_download makes it with the feeds of every entry, permuted by `order` as canon_permute does (order empty: the
// identity), then per triangle the place of every entry in the level order the build stored -- each held to the columns
// the triangle holds, so a handle of another pattern is refused here.  lower / upper: the triangles the object has; an
// object with one triangle maps, gathers and keeps that triangle's entries alone (and the diagonal where it is read).
// want_pattern: the block's rp and col go to the device as well (ILU(0) factors on them).
int tri_refresh_analyse(const spmv_csr_dev *m, const std::vector<int> &order, const TriDev *lower, const TriDev *upper,
                        bool want_diag, bool want_pattern, const char *what, std::unique_ptr<TriRefresh> &out) {
    const int n = m->M_local;
    const size_t nz = (size_t)m->nz;
    std::vector<int> rp((size_t)n + 1, 0), col(nz);
    HIP_TRY(hipMemcpy(rp.data(), m->row_ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (nz) HIP_TRY(hipMemcpy(col.data(), m->col, nz * sizeof(int), hipMemcpyDeviceToHost));
    // the canonical block; A.val[e] = e, so that the permutation carries every entry's place along
    Canon A;
    std::vector<int> fpA(1, 0), feedA, idx;
    A.n = n;
    A.rp.assign((size_t)n + 1, 0);
    A.diag.assign((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        idx.clear();
        for (int e = rp[i]; e < rp[i + 1]; ++e)
            if (col[e] >= m->row0 && col[e] < m->row0 + n) idx.push_back(e);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return col[a] < col[b]; });
        for (size_t k = 0; k < idx.size(); ++k) {
            const int c = col[idx[k]] - m->row0;
            if (k && c == A.col.back()) {
                feedA.push_back(idx[k]);
                fpA.back() = (int)feedA.size();
                continue;
            }
            if (c == i) A.diag[i] = (int)A.col.size();
            A.val.push_back((double)A.col.size());
            A.col.push_back(c);
            feedA.push_back(idx[k]);
            fpA.push_back((int)feedA.size());
        }
        A.rp[i + 1] = (int)A.col.size();
    }
    Canon B;
    if (!order.empty()) {
        if ((int)order.size() != n) return not_the_pattern(what);
        canon_permute(A, order, B);
    } else {
        B = std::move(A);
    }
    if (!lower || !upper) {  // one triangle: B shrinks to its side of the diagonal
        Canon C;
        C.n = n;
        C.rp.assign((size_t)n + 1, 0);
        C.diag.assign((size_t)n, -1);
        for (int i = 0; i < n; ++i) {
            for (int e = B.rp[i]; e < B.rp[i + 1]; ++e) {
                const int c = B.col[e];
                if (c == i ? !want_diag : (lower ? c > i : c < i)) continue;
                if (c == i) C.diag[i] = (int)C.col.size();
                C.col.push_back(c);
                C.val.push_back(B.val[e]);
            }
            C.rp[i + 1] = (int)C.col.size();
        }
        B = std::move(C);
    }
    const size_t nzb = B.col.size();
    std::vector<int> fp(1, 0), feed;
    feed.reserve(feedA.size());
    for (size_t e = 0; e < nzb; ++e) {
        const size_t a = (size_t)B.val[e];
        feed.insert(feed.end(), feedA.begin() + fpA[a], feedA.begin() + fpA[a + 1]);
        fp.push_back((int)feed.size());
    }
    if (want_diag && first_missing_diag(B) >= 0) return not_the_pattern(what);
    std::unique_ptr<TriRefresh> rf(new TriRefresh);
    rf->nzb = (long long)nzb;
    std::vector<int> where((size_t)n);  // of handle row i: its row of B
    for (int k = 0; k < n; ++k) where[order.empty() ? k : order[k]] = k;
    for (int side = 0; side < 2; ++side) {
        const TriDev *t = side ? upper : lower;
        if (!t) continue;
        if (t->n != n) return not_the_pattern(what);
        // the lower triangle is numbered like B and its columns too; the upper one's rows and columns like the handle
        const bool mapped = side && !order.empty();
        std::vector<int> xrow((size_t)n), trp((size_t)n + 1, 0), tcol((size_t)t->entries), src((size_t)t->entries), rows((size_t)n);
        if (n) HIP_TRY(hipMemcpy(xrow.data(), t->xrow, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (n) HIP_TRY(hipMemcpy(trp.data(), t->rp, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
        if (t->entries) HIP_TRY(hipMemcpy(tcol.data(), t->col, tcol.size() * sizeof(int), hipMemcpyDeviceToHost));
        int slot = 0;
        for (int q = 0; q < n; ++q) {
            if (xrow[q] < 0 || xrow[q] >= n || trp[q] != slot) return not_the_pattern(what);
            const int i = mapped ? where[xrow[q]] : xrow[q];
            rows[q] = i;
            for (int e = B.rp[i]; e < B.rp[i + 1]; ++e) {
                const int c = B.col[e];
                if (side ? c <= i : c >= i) continue;
                if (slot >= trp[q + 1] || tcol[slot] != (mapped ? order[c] : c)) return not_the_pattern(what);
                src[slot++] = (int)e;
            }
            if (slot != trp[q + 1]) return not_the_pattern(what);
        }
        if ((long long)slot != t->entries) return not_the_pattern(what);
        if (to_device(&rf->src[side], src)) return -1;
        if (side && to_device(&rf->urow, rows)) return -1;
    }
    if (to_device(&rf->fp, fp) || to_device(&rf->feed, feed)) return -1;
    if (want_pattern && (to_device(&rf->rp, B.rp) || to_device(&rf->col, B.col))) return -1;
    if (want_diag && to_device(&rf->diag, B.diag)) return -1;
    out = std::move(rf);
    return 0;
}

// One refresh on the device.  W: B's values gathered from m in fp64 (ILU(0): factored in place); then the diagonal's
// checks into scratch, and only behind them the scatters into the triangles.  mode as rf_diag (-1: a unit triangular
// solve, no diagonal); diag_host (optional): the diagonal as P->factors returns it.  On -1 the object is as it was.
template <typename T>
int tri_refresh_run(const spmv_csr_dev *m, const TriRefresh &rf, TriDev *lower, TriDev *upper, int mode, double omega,
                    const std::vector<int> &order, const char *what, std::vector<double> *diag_host) {
    const int n = m->M_local;
    if (!n) return 0;
    DevBuf W, dtmp, dout, bad;
    hipError_t e = W.alloc((size_t)rf.nzb * sizeof(double));
    if (e == hipSuccess) e = dtmp.alloc((size_t)n * sizeof(T));
    if (e == hipSuccess) e = dout.alloc((size_t)n * sizeof(double));
    if (e == hipSuccess) e = bad.alloc(2 * sizeof(int));
    const int none[2] = {INT_MAX, INT_MAX};
    if (e == hipSuccess) e = hipMemcpyAsync(bad.p, none, sizeof none, hipMemcpyHostToDevice, g_stream);
    if (e != hipSuccess) return fail("refresh: allocation failed: %s", hipGetErrorString(e));
    if (rf.nzb)
        hipLaunchKernelGGL((spmv::rf_gather<T>), dim3(spmv::rf_grid(rf.nzb)), dim3(kBlock), 0, g_stream, rf.nzb, (const int *)rf.fp,
                           (const int *)rf.feed, (const T *)m->val, W.as<double>());
    if (mode == 2) {  // ILU(0): the build's launches, on the forward plan
        const TriDev &f = *lower;
        for (size_t k = 0; k < f.plan.size(); k += 4) {
            const int l0 = f.plan[k + 1], l1 = f.plan[k + 2];
            if (f.plan[k]) {
                hipLaunchKernelGGL(spmv::ilu0_chain, dim3(1), dim3(kBlock), 0, g_stream, l0, l1, (const int *)f.level_ptr,
                                   (const int *)f.xrow, (const int *)rf.rp, (const int *)rf.col, (const int *)rf.diag,
                                   W.as<double>(), bad.as<int>());
            } else {
                const int p0 = rf.fwd_level_ptr[(size_t)l0], p1 = rf.fwd_level_ptr[(size_t)l1];
                const int grid = std::min(spmv::kTrsvBlocks, (p1 - p0 + kBlock / 64 - 1) / (kBlock / 64));
                hipLaunchKernelGGL(spmv::ilu0_level, dim3(grid), dim3(kBlock), 0, g_stream, p0, p1, (const int *)f.xrow,
                                   (const int *)rf.rp, (const int *)rf.col, (const int *)rf.diag, W.as<double>(), bad.as<int>());
            }
        }
    }
    std::vector<double> d_host((size_t)n);
    int h[2] = {INT_MAX, INT_MAX};
    if (mode >= 0)
        hipLaunchKernelGGL((spmv::rf_diag<T>), dim3(spmv::rf_grid(n)), dim3(kBlock), 0, g_stream, n, mode, omega, (const int *)rf.diag,
                           (const double *)W.as<double>(), dout.as<double>(), dtmp.as<T>(), bad.as<int>() + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, bad.p, sizeof h, hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess && mode >= 0) e = hipMemcpyAsync(d_host.data(), dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("refresh: the factorisation failed: %s", hipGetErrorString(e));
    auto original = [&](int k) { return order.empty() ? k : order[(size_t)k]; };
    // the build's refusals, in the build's order and words behind the refresh's name
    if (h[0] != INT_MAX)
        return fail("%s: row %d (global row %d): ILU(0) meets a zero or non-finite pivot", what, original(h[0]),
                    m->row0 + original(h[0]));
    if (h[1] != INT_MAX) {
        const int i = original(h[1]);
        if (mode == 2) return fail("%s: row %d (global row %d): the pivot's inverse is not finite", what, i, m->row0 + i);
        return fail("%s: row %d (global row %d): the diagonal is zero or not finite, or so small that its inverse is not finite",
                    what, i, m->row0 + i);
    }
    // publish: one rounding to the dtype per value
    TriDev *tri[2] = {lower, upper};
    for (int side = 0; side < 2; ++side) {
        TriDev *t = tri[side];
        if (!t) continue;
        if (t->entries)
            hipLaunchKernelGGL((spmv::rf_scatter<T>), dim3(spmv::rf_grid(t->entries)), dim3(kBlock), 0, g_stream, t->entries,
                               (const int *)rf.src[side], (const double *)W.as<double>(), (T *)t->val);
        if (t->dinv)
            hipLaunchKernelGGL((spmv::rf_pick<T>), dim3(spmv::rf_grid(n)), dim3(kBlock), 0, g_stream, (long long)n,
                               (const int *)(side ? rf.urow : t->xrow), (const T *)dtmp.as<T>(), (T *)t->dinv);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("refresh: the scatter failed: %s", hipGetErrorString(e));
    if (diag_host) *diag_host = d_host;
    return 0;
}

// the family's refresh: SSOR and ILU(0), either ordering
int tri_precond_refresh(spmv_precond *P, const spmv_csr_dev *m) {
    spmv_tri_precond *tp = (spmv_tri_precond *)P->impl;
    if (!tp->rf) {
        // Stamp and maps live and die together: the frame has just stamped m's pattern, and whatever ends this block
        // without maps -- a handle of another pattern, a HIP error, an exception -- takes the stamp along, so that the next
        // refresh is held to the triangles again.  Once there are maps the stamp stays, whatever a refresh refuses.
        struct DropStamp {
            PatternStamp &stamp;
            bool armed = true;
            ~DropStamp() {
                if (armed) stamp = PatternStamp();
            }
        } drop{P->stamp};
        std::unique_ptr<TriRefresh> rf;
        if (tri_refresh_analyse(m, tp->order, &tp->fwd, &tp->bwd, true, tp->unit_lower, "precond_refresh", rf)) return -1;
        if (tp->unit_lower) {
            rf->fwd_level_ptr.resize((size_t)tp->fwd.levels + 1);
            HIP_TRY(hipMemcpy(rf->fwd_level_ptr.data(), tp->fwd.level_ptr, rf->fwd_level_ptr.size() * sizeof(int), hipMemcpyDeviceToHost));
        }
        tp->rf = std::move(rf);
        drop.armed = false;
    }
    const int mode = tp->unit_lower ? 2 : 1;
    const char *name = "precond_refresh";
    return P->value_bytes == 8 ? tri_refresh_run<double>(m, *tp->rf, &tp->fwd, &tp->bwd, mode, tp->omega, tp->order, name, &tp->diag)
                               : tri_refresh_run<float>(m, *tp->rf, &tp->fwd, &tp->bwd, mode, tp->omega, tp->order, name, &tp->diag);
}

int trsv_refresh(spmv_trsv *S, const spmv_csr_dev *m) {
    const bool lower = S->uplo == SPMV_TRSV_LOWER, unit = S->diag == SPMV_TRSV_UNIT;
    if (!S->rf && tri_refresh_analyse(m, {}, lower ? &S->t : nullptr, lower ? nullptr : &S->t, !unit, false, "trsv_refresh", S->rf)) {
        S->stamp = PatternStamp();  // no maps: no stamp either (the next refresh is held to the triangle again)
        return -1;
    }
    TriDev *lo = lower ? &S->t : nullptr, *up = lower ? nullptr : &S->t;
    return S->value_bytes == 8 ? tri_refresh_run<double>(m, *S->rf, lo, up, unit ? -1 : 0, 1.0, {}, "trsv_refresh", nullptr)
                               : tri_refresh_run<float>(m, *S->rf, lo, up, unit ? -1 : 0, 1.0, {}, "trsv_refresh", nullptr);
}

template <typename T>
int trsv_solve_host(const spmv_trsv *S, const void *b_host, void *x_host) {
    const size_t bytes = (size_t)S->rows * sizeof(T);
    SolverScope scope;
    T *b = (T *)scope.alloc(std::max<size_t>(bytes, 16));
    T *x = (T *)scope.alloc(std::max<size_t>(bytes, 16));
    hipError_t e = scope.err;
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(b, b_host, bytes, hipMemcpyHostToDevice, g_stream);
    if (e != hipSuccess) return fail("trsv_solve: setup failed: %s", hipGetErrorString(e));
    tri_launch<T, false>(S->t, 1.0, nullptr, b, x, g_stream);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e == hipSuccess && bytes) e = hipMemcpy(x_host, x, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("trsv_solve: run failed: %s", hipGetErrorString(e));
    return 0;
}

// z = M^-1 r by P's two solves on stream s (flags as pc_apply: a stopped solver's launches return)
int tri_precond_apply(const spmv_precond *P, const void *r, void *z, const int *flags, hipStream_t s) {
    const spmv_tri_precond *tp = (const spmv_tri_precond *)P->impl;
    if (!P->rows) return 0;
    if (P->value_bytes == 8) {
        tri_launch<double, false>(tp->fwd, 1.0, flags, (const double *)r, (double *)tp->y, s);
        if (tp->scaled) tri_launch<double, true>(tp->bwd, tp->scale, flags, (const double *)tp->y, (double *)z, s);
        else tri_launch<double, false>(tp->bwd, 1.0, flags, (const double *)tp->y, (double *)z, s);
    } else {
        tri_launch<float, false>(tp->fwd, 1.0, flags, (const float *)r, (float *)tp->y, s);
        if (tp->scaled) tri_launch<float, true>(tp->bwd, tp->scale, flags, (const float *)tp->y, (float *)z, s);
        else tri_launch<float, false>(tp->bwd, 1.0, flags, (const float *)tp->y, (float *)z, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_trsv_build(const spmv_csr_dev *m, int uplo, int diag, int ordering, spmv_trsv **out) {
    if (need_device()) return -1;
    if (!out) return fail("csr_trsv_build: out is NULL");
    *out = nullptr;
    if (!m) return fail("csr_trsv_build: NULL handle");
    if (uplo != SPMV_TRSV_LOWER && uplo != SPMV_TRSV_UPPER)
        return fail("csr_trsv_build: uplo = %d, must be SPMV_TRSV_LOWER or SPMV_TRSV_UPPER", uplo);
    if (diag != SPMV_TRSV_NONUNIT && diag != SPMV_TRSV_UNIT)
        return fail("csr_trsv_build: diag = %d, must be SPMV_TRSV_NONUNIT or SPMV_TRSV_UNIT", diag);
    if (ordering != SPMV_ORDER_NATURAL)
        return fail("csr_trsv_build: ordering = %d: a bare triangular solve takes SPMV_ORDER_NATURAL only (the "
                    "multicolour order changes which matrix a preconditioner factors)", ordering);
    if (handle_ok(m, "csr_trsv_build")) return -1;
    const int rc = guarded("csr_trsv_build", [&] {
        return m->value_bytes == 8 ? trsv_build<double>(m, uplo, diag, out) : trsv_build<float>(m, uplo, diag, out);
    });
    (void)hipGetLastError();
    return rc;
}

extern "C" void spmv_hip_trsv_free(spmv_trsv *S) { delete S; }

// S from the values m holds now (include/spmv_hip.h): the level order and the launch plan stay, the values and the
// diagonal's inverses are gathered and scattered on the device; all or nothing
extern "C" int spmv_hip_trsv_refresh(spmv_trsv *S, const spmv_csr_dev *m) {
    if (need_device()) return -1;
    if (!S || !m) return fail("trsv_refresh: NULL argument");
    if (S->rows != m->M_local || S->row0 != m->row0 || S->value_bytes != m->value_bytes)
        return fail("trsv_refresh: the solver covers rows [%d, %d) with %d-byte values, the handle rows [%d, %d) with %d",
                    S->row0, S->row0 + S->rows, S->value_bytes, m->row0, m->row0 + m->M_local, m->value_bytes);
    if (handle_ok(m, "trsv_refresh")) return -1;
    const int rc = guarded("trsv_refresh", [&] {
        if (pattern_check(m, S->stamp, "trsv_refresh")) return -1;
        return trsv_refresh(S, m);
    });
    if (rc && !S->rf) S->stamp = PatternStamp();  // stamp and maps live and die together (an exception in the analysis)
    (void)hipGetLastError();
    return rc;
}

extern "C" int spmv_hip_trsv_info(const spmv_trsv *S, int *info) {
    if (!S || !info) return fail("trsv_info: bad arguments");
    const int v[SPMV_TRSV_INFO_WORDS] = {S->rows, S->row0, S->value_bytes, (int)S->t.entries, S->t.levels, S->t.launches,
                                         S->t.widest, 0, S->t.median, S->t.G, S->analysis_us, S->upload_us};
    std::copy(v, v + SPMV_TRSV_INFO_WORDS, info);
    return 0;
}

extern "C" int spmv_hip_trsv_solve_on(const spmv_trsv *S, const void *d_b, void *d_x, void *stream) {
    if (need_device()) return -1;
    if (!S || (S->rows && (!d_b || !d_x))) return fail("trsv_solve_on: bad arguments");
    const uintptr_t ub = (uintptr_t)d_b, ux = (uintptr_t)d_x, span = (uintptr_t)S->rows * (uintptr_t)S->value_bytes;
    if (ub < ux + span && ux < ub + span) return fail("trsv_solve_on: b and x must not overlap");
    if (((uintptr_t)d_b | (uintptr_t)d_x) % (uintptr_t)S->value_bytes)
        return fail("trsv_solve_on: b and x must be aligned to %d bytes", S->value_bytes);
    hipStream_t s = stream ? (hipStream_t)stream : g_stream;
    if (S->value_bytes == 8) tri_launch<double, false>(S->t, 1.0, nullptr, (const double *)d_b, (double *)d_x, s);
    else tri_launch<float, false>(S->t, 1.0, nullptr, (const float *)d_b, (float *)d_x, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int spmv_hip_trsv_solve(const spmv_trsv *S, const void *b_host, void *x_host) {
    if (need_device()) return -1;
    if (!S || (S->rows && (!b_host || !x_host))) return fail("trsv_solve: bad arguments");
    return guarded("trsv_solve", [&] {
        return S->value_bytes == 8 ? trsv_solve_host<double>(S, b_host, x_host) : trsv_solve_host<float>(S, b_host, x_host);
    });
}

extern "C" int spmv_hip_csr_precond_build_tri(const spmv_csr_dev *m, int kind, int ordering, double omega,
                                              spmv_precond **out) {
    auto check = [&] {
        if (kind != SPMV_PRECOND_SSOR && kind != SPMV_PRECOND_ILU0)
            return fail("csr_precond_build_tri: kind = %d, must be SPMV_PRECOND_SSOR or SPMV_PRECOND_ILU0", kind);
        if (ordering != SPMV_ORDER_NATURAL && ordering != SPMV_ORDER_MULTICOLOR)
            return fail("csr_precond_build_tri: ordering = %d, must be SPMV_ORDER_NATURAL or SPMV_ORDER_MULTICOLOR", ordering);
        if (kind == SPMV_PRECOND_SSOR && !(omega > 0.0 && omega < 2.0))
            return fail("csr_precond_build_tri: omega = %g, SSOR needs 0 < omega < 2", omega);
        return 0;
    };
    return precond_build_frame("csr_precond_build_tri", m, out, check, [&](auto t, spmv_precond **P) {
        return tri_precond_build<decltype(t)>(m, kind, ordering, omega, P);
    });
}

extern "C" int spmv_hip_precond_tri_info(const spmv_precond *P, int *info) {
    if (!P || !info) return fail("precond_tri_info: bad arguments");
    const spmv_tri_precond *tp = (const spmv_tri_precond *)precond_impl(P, &kTriFamily, "precond_tri_info");
    if (!tp) return -1;
    const int v[SPMV_PRECOND_TRI_INFO_WORDS] = {tp->fwd.levels, tp->fwd.launches, tp->fwd.widest, tp->fwd.median,
                                                tp->bwd.levels, tp->bwd.launches, tp->bwd.widest, tp->bwd.median,
                                                tp->colours, (int)(tp->fwd.entries + P->rows), (int)(tp->bwd.entries + P->rows),
                                                tp->analysis_us, tp->factor_us, tp->upload_us};
    std::copy(v, v + SPMV_PRECOND_TRI_INFO_WORDS, info);
    return 0;
}

namespace {

// L (which = SPMV_FACTOR_L) or U of P in the handle's numbering, both with their diagonal, columns ascending (col =
// val = NULL: row_ptr alone).  The strict triangle is read back from the device's level-ordered copy (P keeps no host
// copy of it); only the diagonal is P's.
template <typename T>
int factors_body(const spmv_precond *P, bool lower, int *row_ptr, int *col, T *val) {
    const spmv_tri_precond *tp = (const spmv_tri_precond *)P->impl;
    const TriDev &t = lower ? tp->fwd : tp->bwd;
    const int n = P->rows;
    const size_t nz = (size_t)t.entries;
    std::vector<int> rp((size_t)n + 1, 0), xrow((size_t)n), tcol(col ? nz : 0);
    std::vector<T> tval(col ? nz : 0);
    if (n) HIP_TRY(hipMemcpy(rp.data(), t.rp, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (n) HIP_TRY(hipMemcpy(xrow.data(), t.xrow, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (col && nz) HIP_TRY(hipMemcpy(tcol.data(), t.col, nz * sizeof(int), hipMemcpyDeviceToHost));
    if (col && nz) HIP_TRY(hipMemcpy(tval.data(), t.val, nz * sizeof(T), hipMemcpyDeviceToHost));
    // the forward triangle is numbered like the permuted matrix, the backward one like the handle
    auto original = [&](int k) { return lower && !tp->order.empty() ? tp->order[k] : k; };
    std::vector<int> place((size_t)n), where((size_t)n);  // of handle row i: its place in t, its row of the permuted matrix
    for (int q = 0; q < n; ++q) place[original(xrow[q])] = q;
    for (int k = 0; k < n; ++k) where[tp->order.empty() ? k : tp->order[k]] = k;
    std::vector<std::pair<int, T>> row;
    int out = 0;
    row_ptr[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int q = place[i];
        if (col) {
            row.clear();
            for (int e = rp[q]; e < rp[q + 1]; ++e) row.emplace_back(original(tcol[e]), tval[e]);
            row.emplace_back(i, lower && tp->unit_lower ? T(1) : (T)tp->diag[where[i]]);
            std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
            for (const auto &cv : row) {
                col[out] = cv.first;
                val[out++] = cv.second;
            }
        } else {
            out += rp[q + 1] - rp[q] + 1;
        }
        row_ptr[i + 1] = out;
    }
    return 0;
}

int tri_precond_factors(const spmv_precond *P, int which, int *row_ptr, int *col, void *val) {
    return P->value_bytes == 8 ? factors_body<double>(P, which == SPMV_FACTOR_L, row_ptr, col, (double *)val)
                               : factors_body<float>(P, which == SPMV_FACTOR_L, row_ptr, col, (float *)val);
}

// two solves take one right-hand side: no k-wide apply, no workspace
const precond_family kTriFamily = {"made of triangular solves", nullptr, tri_precond_apply, nullptr, nullptr, tri_precond_factors,
                                   [](void *impl) { delete (spmv_tri_precond *)impl; }, tri_precond_refresh};

}  // namespace
