// spmv_fsai.hip -- the FSAI preconditioner of a CSR handle (Kolotilina and Yeremin): a sparse lower-triangular G with
// G^T G ~ A^-1, applied as two SpMVs (include/spmv_hip.h; the kernel is in fsai_kernels.hpp, the pattern pass in
// host/fsai_plan.c).
//
// The build, once per object:
//   1. the handle's diagonal block is downloaded and made canonical (canon_rows.hpp), as the triangular builds do;
//   2. spmv_fsai_plan selects every row's pattern S_i from its lower triangle and groups the rows by lane width;
//   3. the canonical block goes to the device in fp64 and fsai_rows<T, W> builds the rows of each width: gather the
//      local matrix A~[S_i, S_i] into LDS, Cholesky in place, one back substitution, the row rounded once to T straight
//      into G's value array; a status word per row comes back (no atomics);
//   4. G's arrays are adopted as an ordinary whole rows x rows handle (the upload's plans and searches), G^T is
//      spmv_hip_csr_transpose of it.
// The apply is t = G r, z = G^T t through the two handles' AUTO launches on one stream and nothing else; t is P's own
// vector (so one P serves one stream at a time), with the line tail the x-window kernels read.
#include "spmv_internal.hpp"

#include <cmath>
#include <memory>

#include "canon_rows.hpp"
#include "fsai_kernels.hpp"
#include "precond_kernels.hpp"

struct spmv_fsai_precond {
    spmv_csr_dev *G = nullptr, *Gt = nullptr;
    void *t = nullptr;  // G r, between the two products
    int cap = 0, truncated = 0, widest = 0;
    long long entries = 0;
    int analysis_us = 0, build_us = 0, upload_us = 0;
    ~spmv_fsai_precond() {
        spmv_hip_csr_free(G);
        spmv_hip_csr_free(Gt);
        (void)hipFree(t);
    }
};

namespace {

extern const precond_family kFsaiFamily;  // behind the functions it names

template <typename T, int W>
void fsai_launch(int count, const int *rows, const int *a_rp, const int *a_col, const double *a_val, const int *g_rp,
                 const int *g_col, T *g_val, int *status) {
    if (!count) return;
    constexpr int per = kFsaiBlock / W;
    const int grid = (int)std::min<long long>(kFsaiMaxGrid, ((long long)count + per - 1) / per);
    hipLaunchKernelGGL((fsai_rows<T, W>), dim3(grid), dim3(kFsaiBlock), 0, g_stream, count, rows, a_rp, a_col, a_val,
                       g_rp, g_col, g_val, status);
}

// the device arrays of one build: freed on every path, an exception's (host out of memory under guarded()) included;
// d_col / d_val are set to NULL once G's handle owns them
template <typename T>
struct BuildArrays {
    int *a_rp = nullptr, *a_col = nullptr, *d_rp = nullptr, *d_rows = nullptr, *status = nullptr, *d_col = nullptr;
    double *a_val = nullptr;
    T *d_val = nullptr;
    BuildArrays() = default;
    BuildArrays(const BuildArrays &) = delete;
    BuildArrays &operator=(const BuildArrays &) = delete;
    ~BuildArrays() {
        for (void *q : {(void *)a_rp, (void *)a_col, (void *)a_val, (void *)d_rp, (void *)d_rows, (void *)status,
                        (void *)d_col, (void *)d_val})
            (void)hipFree(q);
        (void)hipGetLastError();  // a refused build is reported by its return value, not by the next launch
    }
};

template <typename T>
int fsai_build(const spmv_csr_dev *m, int cap, spmv_precond **out) {
    const double t0 = now_ms();
    Canon A;
    if (canon_download<T>(m, A)) return -1;
    const int n = A.n;
    const int miss = first_missing_diag(A);
    if (miss >= 0)
        return fail("csr_precond_build_fsai: row %d (global row %d) has no diagonal entry", miss, m->row0 + miss);
    std::vector<int> g_rp((size_t)n + 1, 0), g_col(std::min((size_t)n * (size_t)cap, A.col.size() + (size_t)n)),
        rows((size_t)n);
    int width_ptr[5] = {0, 0, 0, 0, 0};
    long long counts[4] = {0, 0, 0, -1};
    if (spmv_fsai_plan(n, A.rp.data(), A.col.data(), A.val.data(), cap, g_rp.data(), g_col.data(), width_ptr,
                       rows.data(), counts))
        return fail("csr_precond_build_fsai: the pattern pass failed (out of host memory)");
    const size_t nzg = (size_t)counts[0];
    g_col.resize(nzg);
    const double t1 = now_ms();

    std::unique_ptr<spmv_fsai_precond> fp(new spmv_fsai_precond);
    BuildArrays<T> d;
    std::vector<int> st((size_t)n, 0);
    int rc = -1;
    do {
        if (to_device(&d.a_rp, A.rp) || to_device(&d.a_col, A.col) || to_device(&d.a_val, A.val) ||
            to_device(&d.d_rp, g_rp) || to_device(&d.d_rows, rows) ||
            upload_array(&d.d_col, g_col.data(), nzg, (size_t)kPad))
            break;
        hipError_t e = hipMalloc((void **)&d.d_val, (nzg + kPad) * sizeof(T));
        if (e == hipSuccess) e = hipMemsetAsync(d.d_val, 0, (nzg + kPad) * sizeof(T), g_stream);
        if (e == hipSuccess) e = hipMalloc((void **)&d.status, std::max<size_t>((size_t)n, 4) * sizeof(int));
        if (e == hipSuccess) e = hipMemsetAsync(d.status, 0, std::max<size_t>((size_t)n, 4) * sizeof(int), g_stream);
        if (e != hipSuccess) {
            fail("csr_precond_build_fsai: allocation failed: %s", hipGetErrorString(e));
            break;
        }
        for (int k = 0; k < 4; ++k) {  // the rows of 4 << k lanes
            const int count = width_ptr[k + 1] - width_ptr[k];
            const int *r = d.d_rows + width_ptr[k];
            if (k == 0) fsai_launch<T, 4>(count, r, d.a_rp, d.a_col, d.a_val, d.d_rp, d.d_col, d.d_val, d.status);
            if (k == 1) fsai_launch<T, 8>(count, r, d.a_rp, d.a_col, d.a_val, d.d_rp, d.d_col, d.d_val, d.status);
            if (k == 2) fsai_launch<T, 16>(count, r, d.a_rp, d.a_col, d.a_val, d.d_rp, d.d_col, d.d_val, d.status);
            if (k == 3) fsai_launch<T, 32>(count, r, d.a_rp, d.a_col, d.a_val, d.d_rp, d.d_col, d.d_val, d.status);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e == hipSuccess && n) e = hipMemcpy(st.data(), d.status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            fail("csr_precond_build_fsai: the build failed: %s", hipGetErrorString(e));
            break;
        }
        int bad = -1;
        for (int i = 0; i < n && bad < 0; ++i)
            if (st[i]) bad = i;
        if (bad >= 0) {
            if (st[bad] == 1)
                fail("csr_precond_build_fsai: row %d (global row %d): a Cholesky pivot of its local matrix is not "
                     "positive or not finite (the matrix is not positive definite on the row's pattern)", bad,
                     m->row0 + bad);
            else
                fail("csr_precond_build_fsai: row %d (global row %d): an entry of G is not finite in the handle's dtype",
                     bad, m->row0 + bad);
            break;
        }
        const double t2 = now_ms();
        if (n) {  // (a handle without rows has no factors: the apply returns before it would launch them)
            if (csr_adopt<T>(n, n, g_rp.data(), d.d_col, d.d_val, &fp->G)) break;
            d.d_col = nullptr, d.d_val = nullptr;  // the handle owns them now
            if (spmv_hip_csr_transpose(fp->G, &fp->Gt)) break;
        }
        const size_t t_bytes = ((size_t)n * sizeof(T) + 15) / 16 * 16 + kLineBytes;
        e = hipMalloc(&fp->t, t_bytes);
        if (e == hipSuccess) e = hipMemset(fp->t, 0, t_bytes);
        if (e != hipSuccess) {
            fail("csr_precond_build_fsai: allocation failed: %s", hipGetErrorString(e));
            break;
        }
        fp->analysis_us = (int)((t1 - t0) * 1e3);
        fp->build_us = (int)((t2 - t1) * 1e3);
        fp->upload_us = (int)((now_ms() - t2) * 1e3);
        rc = 0;
    } while (0);
    if (rc) return rc;
    fp->cap = cap;
    fp->entries = counts[0];
    fp->truncated = (int)counts[1];
    fp->widest = (int)counts[2];
    *out = precond_new(m, SPMV_PRECOND_FSAI, 1, sizeof(T), &kFsaiFamily, fp.release());
    return 0;
}

// z = G^T (G r) by the two handles' own launches on stream s (they do not look at a solver's flags: after a stop r no
// longer changes, so z is rewritten with the bits it holds)
int fsai_apply(const spmv_precond *P, const void *r, void *z, const int *, hipStream_t s) {
    const spmv_fsai_precond *fp = (const spmv_fsai_precond *)P->impl;
    if (!P->rows) return 0;
    if (csr_launch_any(fp->G, SPMV_CSR_AUTO, r, fp->t, s)) return -1;
    return csr_launch_any(fp->Gt, SPMV_CSR_AUTO, fp->t, z, s);
}

// Z = G^T (G R) for rows x k row-major R: two SpMMs through the same two handles (k = 1: their AUTO launches, the bits
// of fsai_apply).  work (rows x k values and a line tail) stands in for P's own t, which is not touched.
int fsai_apply_multi(const spmv_precond *P, int k, const void *R, void *Z, void *work, hipStream_t s) {
    const spmv_fsai_precond *fp = (const spmv_fsai_precond *)P->impl;
    if (!P->rows) return 0;
    if (spmv_hip_csr_spmm_on(fp->G, k, R, work, s)) return -1;
    return spmv_hip_csr_spmm_on(fp->Gt, k, work, Z, s);
}

// G (which = SPMV_FACTOR_L) or G^T as their handles hold them: columns ascending, values of the handle's dtype
int fsai_factors(const spmv_precond *P, int which, int *row_ptr, int *col, void *val) {
    const spmv_fsai_precond *fp = (const spmv_fsai_precond *)P->impl;
    const spmv_csr_dev *h = which == SPMV_FACTOR_L ? fp->G : fp->Gt;
    const size_t n = (size_t)P->rows, nz = h ? (size_t)h->nz : 0;
    row_ptr[0] = 0;
    if (!h) return 0;
    HIP_TRY(hipMemcpy(row_ptr, h->row_ptr, (n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (col && nz) HIP_TRY(hipMemcpy(col, h->col, nz * sizeof(int), hipMemcpyDeviceToHost));
    if (col && nz) HIP_TRY(hipMemcpy(val, h->val, nz * (size_t)h->value_bytes, hipMemcpyDeviceToHost));
    return 0;
}

long long fsai_work_bytes(const spmv_precond *P, int k) {
    return std::max<long long>((long long)P->rows * k * P->value_bytes, 16) + kLineBytes;
}

const precond_family kFsaiFamily = {"FSAI", "an FSAI apply needs d_work (rows x k values and one 128-byte line)",
                                    fsai_apply, fsai_apply_multi, fsai_work_bytes, fsai_factors,
                                    [](void *impl) { delete (spmv_fsai_precond *)impl; }};

}  // namespace

extern "C" int spmv_hip_csr_precond_build_fsai(const spmv_csr_dev *m, int cap, spmv_precond **out) {
    auto check = [&] {
        return cap < 1 || cap > kFsaiMaxCap ? fail("csr_precond_build_fsai: cap = %d, must be in [1, %d]", cap, kFsaiMaxCap) : 0;
    };
    return precond_build_frame("csr_precond_build_fsai", m, out, check, [&](auto t, spmv_precond **P) {
        return fsai_build<decltype(t)>(m, cap, P);
    });
}

extern "C" int spmv_hip_precond_fsai_info(const spmv_precond *P, int *info) {
    if (!P || !info) return fail("precond_fsai_info: bad arguments");
    const spmv_fsai_precond *fp = (const spmv_fsai_precond *)precond_impl(P, &kFsaiFamily, "precond_fsai_info");
    if (!fp) return -1;
    const int v[SPMV_PRECOND_FSAI_INFO_WORDS] = {fp->cap, (int)fp->entries, fp->truncated, fp->widest, plan_of(fp->G),
                                                 plan_of(fp->Gt), fp->analysis_us, fp->build_us, fp->upload_us};
    std::copy(v, v + SPMV_PRECOND_FSAI_INFO_WORDS, info);
    return 0;
}
