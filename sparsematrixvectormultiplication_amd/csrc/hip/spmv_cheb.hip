// spmv_cheb.hip -- the Chebyshev polynomial preconditioner of a CSR handle: m steps of Jacobi-preconditioned Chebyshev
// iteration on A z = r from z = 0 (include/spmv_hip.h; the passes are in cheb_kernels.hpp, the coefficients in
// host/cheb_plan.c).
//
// The build, once per object:
//   1. the handle's diagonal block is downloaded and made canonical (canon_rows.hpp), as the triangular, FSAI and AMG
//      builds do;
//   2. one pass over the rows (amg_gershgorin, the function the AMG setup takes its rho from): every a_ii present,
//      finite and > 0, and the Gershgorin bound max_i sum_j |a_ij| / a_ii of D^-1 A; g_i = T(1 / a_ii);
//   3. [lmin, lmax] from the arguments (0: lmax = the bound, lmin = lmax / ratio), the coefficients a_j, b_j on the host;
//   4. the canonical block rounded to the handle's dtype is adopted as an ordinary whole rows x rows handle (the upload's
//      plans and searches); g and the three vectors z, d, q, each with the 128-byte tail the x-window kernels read.
// No factorisation, no levels, no colouring, no pattern pass.
//
// The apply, all on one stream, nothing allocated and nothing read back:
//   step 0:        d = b_0 g.r;  z = d                                       (one launch)
//   step j >= 1:   q = A z  by the handle's AUTO launch (k vectors: spmv_hip_csr_spmm_on);
//                  d = a_j d + b_j g.(r - q);  z = z + d                      (one fused pass)
// The iterate lives in P's z (k vectors: in the caller's work), so no product reads a caller's buffer as its x; the last
// pass writes the caller's z and stores no d.  With degree 1 the first pass is the last.
#include "spmv_internal.hpp"

#include <cmath>
#include <memory>

#include "../host/amg_plan_parts.h"
#include "canon_rows.hpp"
#include "cheb_kernels.hpp"
#include "precond_kernels.hpp"

struct spmv_cheb_precond {
    spmv_csr_dev *A = nullptr;  // P's own upload of the canonical block
    void *g = nullptr;          // T(1 / a_ii)
    void *z = nullptr, *d = nullptr, *q = nullptr;  // the iterate, its last change and A z: rows values and a line tail
    int degree = 1;
    double lmin = 0, lmax = 0, gershgorin = 0;
    double a[kChebMaxDegree] = {}, b[kChebMaxDegree] = {};
    int download_us = 0, upload_us = 0;
    ~spmv_cheb_precond() {
        spmv_hip_csr_free(A);
        for (void *p : {g, z, d, q}) (void)hipFree(p);
    }
};

namespace {

constexpr const char *kWhat = "csr_precond_build_chebyshev";
extern const precond_family kChebFamily;  // behind the functions it names
static_assert(kChebMaxDegree == SPMV_CHEBYSHEV_MAX_DEGREE, "the header's limit is the coefficient arrays' size");

// col / val of the block on their way into P's handle: freed unless the handle took them
template <typename T>
struct BlockArrays {
    int *col = nullptr;
    T *val = nullptr;
    BlockArrays() = default;
    BlockArrays(const BlockArrays &) = delete;
    BlockArrays &operator=(const BlockArrays &) = delete;
    ~BlockArrays() {
        (void)hipFree(col);
        (void)hipFree(val);
        (void)hipGetLastError();  // a refused build is reported by its return value, not by the next launch
    }
};

template <typename T>
int cheb_build(const spmv_csr_dev *m, int degree, double lmin, double lmax, double ratio, spmv_precond **out) {
    const double t0 = now_ms();
    Canon A;
    if (canon_download<T>(m, A)) return -1;
    const int n = A.n;
    const amg_csr block = {n, n, A.rp.data(), A.col.data(), A.val.data()};
    std::vector<double> diag((size_t)n, 0.0);
    double bound = 0.0;
    int missing = 0;
    const int bad = amg_gershgorin(&block, diag.data(), &bound, &missing);
    if (bad >= 0 && missing) return fail("%s: row %d (global row %d) has no diagonal entry", kWhat, bad, m->row0 + bad);
    if (bad >= 0)
        return fail("%s: row %d (global row %d): the diagonal is not positive or not finite", kWhat, bad, m->row0 + bad);
    if (!n) bound = 1.0;  // no rows: any interval serves, the apply launches nothing
    if (!std::isfinite(bound)) return fail("%s: an entry of the matrix is not finite", kWhat);
    std::vector<T> g((size_t)n);
    for (int i = 0; i < n; ++i) {
        g[i] = (T)(1.0 / diag[i]);
        if (!std::isfinite((double)g[i]))
            return fail("%s: row %d (global row %d): the diagonal is so small that its inverse is not finite", kWhat, i,
                        m->row0 + i);
    }
    std::unique_ptr<spmv_cheb_precond> cp(new spmv_cheb_precond);
    cp->degree = degree;
    cp->gershgorin = bound;
    cp->lmax = lmax == 0.0 ? bound : lmax;
    cp->lmin = lmin == 0.0 ? cp->lmax / ratio : lmin;
    if (!(cp->lmin < cp->lmax))
        return fail("%s: lmin = %g, lmax = %g: lmin must be below lmax", kWhat, cp->lmin, cp->lmax);
    if (spmv_chebyshev_coefficients(degree, cp->lmin, cp->lmax, cp->a, cp->b))
        return fail("%s: no coefficients for degree %d on [%g, %g]", kWhat, degree, cp->lmin, cp->lmax);
    for (int j = 0; j < degree; ++j)
        if (!std::isfinite(cp->a[j]) || !std::isfinite(cp->b[j]))
            return fail("%s: coefficient %d of the polynomial on [%g, %g] is not finite", kWhat, j, cp->lmin, cp->lmax);
    const double t1 = now_ms();

    if (n) {
        const size_t nz = A.col.size();
        const std::vector<T> val(A.val.begin(), A.val.end());
        BlockArrays<T> d;
        if (upload_array(&d.col, A.col.data(), nz, (size_t)kPad) || upload_array(&d.val, val.data(), nz, (size_t)kPad))
            return -1;
        if (csr_adopt<T>(n, n, A.rp.data(), d.col, d.val, &cp->A)) return -1;
        d.col = nullptr, d.val = nullptr;  // the handle owns them now
    }
    if (to_device((T **)&cp->g, g)) return -1;
    const size_t vec_bytes = ((size_t)n * sizeof(T) + 15) / 16 * 16 + kLineBytes;
    for (void **v : {&cp->z, &cp->d, &cp->q}) {
        hipError_t e = hipMalloc(v, vec_bytes);
        if (e == hipSuccess) e = hipMemset(*v, 0, vec_bytes);
        if (e != hipSuccess) return fail("%s: allocation failed: %s", kWhat, hipGetErrorString(e));
    }
    cp->download_us = (int)((t1 - t0) * 1e3);
    cp->upload_us = (int)((now_ms() - t1) * 1e3);
    *out = precond_new(m, SPMV_PRECOND_CHEBYSHEV, 1, sizeof(T), &kChebFamily, cp.release());
    return 0;
}

// The passes of one apply on n x k row-major arrays (k = 1: vectors).  z, d, q: P's own vectors or the three parts of a
// caller's work.  k = 1 takes the one-wide kernels and the handle's AUTO launch whoever calls, hence the same bits.
template <typename T>
int cheb_run(const spmv_cheb_precond *cp, long long n, int k, const T *R, T *Zout, T *z, T *d, T *q, hipStream_t s) {
    constexpr int W = 16 / sizeof(T);
    const int m = cp->degree;
    const T *g = (const T *)cp->g;
    const bool aligned = (((uintptr_t)R | (uintptr_t)Zout | (uintptr_t)z | (uintptr_t)d | (uintptr_t)q) & 15) == 0;
    const bool wide = aligned && (k == 1 || (size_t)k * sizeof(T) % 16 == 0);
    const int V = wide ? W : 1;
    const int cl = mcg_column_lanes(k, V);
    const dim3 blk(kBlock);
    const dim3 grid(k == 1 ? solver_grid(kChebBlocks, (n + V - 1) / V, kBlock) : solver_grid(kMcgBlocks, n, kBlock >> cl));
    auto first = [&](auto v, auto last) {
        constexpr int VV = decltype(v)::value;
        constexpr bool L = decltype(last)::value;
        if (k == 1) hipLaunchKernelGGL((cheb_first<T, VV, L>), grid, blk, 0, s, n, cp->b[0], g, R, d, L ? Zout : z);
        else hipLaunchKernelGGL((mcheb_first<T, VV, L>), grid, blk, 0, s, n, k, cl, cp->b[0], g, R, d, L ? Zout : z);
    };
    auto step = [&](int j, auto v, auto last) {
        constexpr int VV = decltype(v)::value;
        constexpr bool L = decltype(last)::value;
        if (k == 1)
            hipLaunchKernelGGL((cheb_step<T, VV, L>), grid, blk, 0, s, n, cp->a[j], cp->b[j], g, R, (const T *)q, (const T *)z,
                               d, L ? Zout : z);
        else
            hipLaunchKernelGGL((mcheb_step<T, VV, L>), grid, blk, 0, s, n, k, cl, cp->a[j], cp->b[j], g, R, (const T *)q,
                               (const T *)z, d, L ? Zout : z);
    };
    using One = std::integral_constant<int, 1>;
    using Piece = std::integral_constant<int, W>;
    for (int j = 0; j < m; ++j) {
        const bool last = j == m - 1;
        if (j) {
            if (k == 1 ? csr_launch_any(cp->A, SPMV_CSR_AUTO, z, q, s) : spmv_hip_csr_spmm_on(cp->A, k, z, q, s)) return -1;
        }
        auto pass = [&](auto v) {
            if (j == 0) last ? first(v, std::true_type()) : first(v, std::false_type());
            else last ? step(j, v, std::true_type()) : step(j, v, std::false_type());
        };
        if (wide) pass(Piece());
        else pass(One());
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// z = p(D^-1 A) D^-1 r, degree - 1 products of P's own handle between fused passes on stream s, the iterate in P's own
// vectors (as FSAI's and AMG's, the launches do not look at a solver's flags)
int cheb_apply(const spmv_precond *P, const void *r, void *z, const int *, hipStream_t s) {
    const spmv_cheb_precond *cp = (const spmv_cheb_precond *)P->impl;
    if (!P->rows) return 0;
    if (P->value_bytes == 8)
        return cheb_run<double>(cp, P->rows, 1, (const double *)r, (double *)z, (double *)cp->z, (double *)cp->d,
                                (double *)cp->q, s);
    return cheb_run<float>(cp, P->rows, 1, (const float *)r, (float *)z, (float *)cp->z, (float *)cp->d, (float *)cp->q, s);
}

// bytes of one of the three arrays of a k-wide apply: rows x k values rounded up to whole 128-byte lines, and a line tail
long long cheb_vec_bytes(const spmv_precond *P, int k) {
    const long long bytes = std::max<long long>((long long)P->rows * k * P->value_bytes, 16);
    return (bytes + kLineBytes - 1) / kLineBytes * kLineBytes + kLineBytes;
}

// Z = M^-1 R for rows x k row-major R and Z.  work: three arrays of cheb_vec_bytes(P, k) bytes -- Z's iterate, D and
// Q = A Z --, P's own vectors are not used (k = 1: the launches of cheb_apply)
int cheb_apply_multi(const spmv_precond *P, int k, const void *R, void *Z, void *work, hipStream_t s) {
    const spmv_cheb_precond *cp = (const spmv_cheb_precond *)P->impl;
    if (!P->rows) return 0;
    const long long stride = cheb_vec_bytes(P, k);
    char *w = (char *)work;
    if (P->value_bytes == 8)
        return cheb_run<double>(cp, P->rows, k, (const double *)R, (double *)Z, (double *)w, (double *)(w + stride),
                                (double *)(w + 2 * stride), s);
    return cheb_run<float>(cp, P->rows, k, (const float *)R, (float *)Z, (float *)w, (float *)(w + stride),
                           (float *)(w + 2 * stride), s);
}

const precond_family kChebFamily = {
    "CHEBYSHEV", "a CHEBYSHEV apply needs d_work (spmv_hip_precond_work_bytes: its three arrays)", cheb_apply, cheb_apply_multi,
    [](const spmv_precond *P, int k) { return 3 * cheb_vec_bytes(P, k); }, nullptr,
    [](void *impl) { delete (spmv_cheb_precond *)impl; }};

}  // namespace

extern "C" int spmv_hip_csr_precond_build_chebyshev(const spmv_csr_dev *m, int degree, double lmin, double lmax,
                                                    double ratio, spmv_precond **out) {
    auto check = [&] {
        if (degree < 1 || degree > kChebMaxDegree)
            return fail("%s: degree = %d, must be in [1, %d]", kWhat, degree, kChebMaxDegree);
        if (!std::isfinite(ratio) || !(ratio > 1.0)) return fail("%s: ratio = %g, must be finite and > 1", kWhat, ratio);
        if (!std::isfinite(lmax) || lmax < 0.0)
            return fail("%s: lmax = %g, must be finite and >= 0 (0: the Gershgorin bound)", kWhat, lmax);
        if (!std::isfinite(lmin) || lmin < 0.0)
            return fail("%s: lmin = %g, must be finite and >= 0 (0: lmax / ratio)", kWhat, lmin);
        return 0;
    };
    return precond_build_frame(kWhat, m, out, check, [&](auto t, spmv_precond **P) {
        return cheb_build<decltype(t)>(m, degree, lmin, lmax, ratio, P);
    });
}

extern "C" int spmv_hip_precond_cheb_info(const spmv_precond *P, double *info) {
    if (!P || !info) return fail("precond_cheb_info: bad arguments");
    const spmv_cheb_precond *cp = (const spmv_cheb_precond *)precond_impl(P, &kChebFamily, "precond_cheb_info");
    if (!cp) return -1;
    const double v[SPMV_PRECOND_CHEB_INFO_WORDS] = {(double)cp->degree, cp->lmin, cp->lmax, cp->gershgorin,
                                                    (double)(cp->degree - 1), (double)plan_of(cp->A),
                                                    (double)cp->download_us, (double)cp->upload_us};
    std::copy(v, v + SPMV_PRECOND_CHEB_INFO_WORDS, info);
    return 0;
}
