// spmv_spmm.hip -- Y = A X for k vectors per pass over a CSR handle: launcher and C-ABI (include/spmv_hip.h,
// "CSR: several vectors per pass").  Kernels: spmm_kernels.hpp.  No plan of its own: the kernels run on the blocks
// and long-row pieces upload built for the gather kernels; k = 1 is the handle's SpMV launch.
#include "spmv_internal.hpp"

#include "spmm_kernels.hpp"

namespace {

// column lanes per row group: the narrowest column tile (4 columns per lane) that holds k, up to 32 columns; wider
// k loops over tiles of 32
int spmm_column_lanes(int k) {
    if (k <= 4) return 1;
    if (k <= 8) return 2;
    if (k <= 16) return 4;
    return 8;
}

template <typename T, int CL, bool VEC>
int spmm_launch_cfg(spmv_csr_dev *m, int k, const T *X, T *Y, hipStream_t s) {
    const int cap = (m->stream_cap + 3) & ~3;
    if (m->num_blocks > 0) {
        const size_t lds = (size_t)cap * (sizeof(T) + sizeof(int));
        hipLaunchKernelGGL((csr_spmm_block<T, CL, VEC>), dim3(m->num_blocks), dim3(kSpmmBlock), lds, s, m->num_blocks,
                           cap, m->desc, m->row_ptr, m->col, (const T *)m->val, X, Y, k);
    }
    if (m->num_long > 0) {
        hipLaunchKernelGGL((csr_spmm_pieces<T, CL, VEC>), dim3(m->num_partial), dim3(kSpmmBlock), 0, s, m->num_partial,
                           m->pieces, m->col, (const T *)m->val, X, (T *)m->spmm_partial, k);
        hipLaunchKernelGGL((csr_spmm_finish<T>), dim3(m->num_long), dim3(64), 0, s, m->num_long, m->long_rows,
                           (const T *)m->spmm_partial, Y, k);
    }
    return 0;
}

template <typename T, bool VEC>
int spmm_launch_vec(spmv_csr_dev *m, int k, const T *X, T *Y, hipStream_t s) {
    switch (spmm_column_lanes(k)) {
        case 1: return spmm_launch_cfg<T, 1, VEC>(m, k, X, Y, s);
        case 2: return spmm_launch_cfg<T, 2, VEC>(m, k, X, Y, s);
        case 4: return spmm_launch_cfg<T, 4, VEC>(m, k, X, Y, s);
        default: return spmm_launch_cfg<T, 8, VEC>(m, k, X, Y, s);
    }
}

// Y (element 0 of the full M_total x k array) = A X on stream s; arguments checked by the caller
template <typename T>
int spmm_launch(spmv_csr_dev *m, int k, const T *X, T *Y, hipStream_t s) {
    if (m->M_local == 0) return 0;
    T *Yh = Y + (size_t)m->row0 * (size_t)k;
    // the pieces' k-wide partial sums: a scratch of the handle that only grows (freed with it)
    const size_t need = (size_t)m->num_partial * (size_t)k * sizeof(T);
    if (m->num_long > 0 && need > m->spmm_partial_bytes) {
        (void)hipFree(m->spmm_partial);
        m->spmm_partial = nullptr;
        m->spmm_partial_bytes = 0;
        HIP_TRY(hipMalloc(&m->spmm_partial, need));
        m->spmm_partial_bytes = need;
    }
    const bool vec = (size_t)k * sizeof(T) % 16 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 15) == 0;
    const int rc = vec ? spmm_launch_vec<T, true>(m, k, X, Yh, s) : spmm_launch_vec<T, false>(m, k, X, Yh, s);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the rules of every entry point; -1 + message (and a clean HIP error state) when one is broken
int spmm_check(const spmv_csr_dev *m, int k, const void *X, const void *Y, const char *what) {
    int rc = 0;
    if (!m || !X || !Y) rc = fail("%s: NULL argument", what);
    else if (k < 1) rc = fail("%s: k = %d, must be >= 1", what, k);
    else if (m->tiles_only) rc = fail("%s: a tiles-only handle has no SpMM kernels", what);
    else if (((uintptr_t)X | (uintptr_t)Y) % (uintptr_t)m->value_bytes != 0)
        rc = fail("%s: X / Y are not aligned to the element size (%d bytes)", what, m->value_bytes);
    if (rc) (void)hipGetLastError();
    return rc;
}

int spmm_any(spmv_csr_dev *m, int k, const void *X, void *Y, hipStream_t s) {
    if (k == 1) return csr_launch_any(m, SPMV_CSR_AUTO, X, Y, s);  // the handle's SpMV: the same bits
    if (m->value_bytes == 8) return spmm_launch<double>(m, k, (const double *)X, (double *)Y, s);
    return spmm_launch<float>(m, k, (const float *)X, (float *)Y, s);
}

}  // namespace

extern "C" int spmv_hip_csr_spmm_on(spmv_csr_dev *m, int k, const void *d_X, void *d_Y, void *stream) {
    if (need_device()) return -1;
    if (spmm_check(m, k, d_X, d_Y, "csr_spmm_on")) return -1;
    return spmm_any(m, k, d_X, d_Y, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_csr_spmm(spmv_csr_dev *m, int k, const void *X_host, void *Y_host) {
    if (need_device()) return -1;
    if (spmm_check(m, k, X_host, Y_host, "csr_spmm")) return -1;
    const size_t vb = (size_t)m->value_bytes, kk = (size_t)k;
    const size_t x_bytes = std::max<size_t>((size_t)m->N * kk * vb, 16);
    const size_t y_bytes = std::max<size_t>((size_t)m->M_total * kk * vb, 16);
    void *dX = nullptr, *dY = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&dX, x_bytes));
        HIP_TRY(hipMalloc(&dY, y_bytes));
        HIP_TRY(hipMemcpyAsync(dX, X_host, (size_t)m->N * kk * vb, hipMemcpyHostToDevice, g_stream));
        if (spmm_any(m, k, dX, dY, g_stream)) return -1;
        // only the handle's rows go back: row-block handles fill one shared Y
        const size_t off = (size_t)m->row0 * kk * vb, len = (size_t)m->M_local * kk * vb;
        HIP_TRY(hipMemcpyAsync((char *)Y_host + off, (const char *)dY + off, len, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(g_stream);
    (void)hipFree(dX);
    (void)hipFree(dY);
    return rc;
}

extern "C" int spmv_hip_csr_spmm_time(spmv_csr_dev *m, int k, int warmup, int iters, float *ms_each) {
    if (need_device()) return -1;
    if (!m) return fail("csr_spmm_time: NULL handle");
    if (k < 1) return fail("csr_spmm_time: k = %d, must be >= 1", k);
    if (m->tiles_only) return fail("csr_spmm_time: a tiles-only handle has no SpMM kernels");
    const size_t vb = (size_t)m->value_bytes, kk = (size_t)k;
    const size_t x_bytes = std::max<size_t>((size_t)m->N * kk * vb, 16);
    const size_t y_bytes = std::max<size_t>((size_t)m->M_total * kk * vb, 16);
    void *dX = nullptr, *dY = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&dX, x_bytes));
        HIP_TRY(hipMalloc(&dY, y_bytes));
        HIP_TRY(hipMemsetAsync(dX, 0, x_bytes, g_stream));
        return time_loop(warmup, iters, ms_each, [&] { return spmm_any(m, k, dX, dY, g_stream); }, [] { return 0; });
    };
    const int rc = body();
    (void)hipStreamSynchronize(g_stream);
    (void)hipFree(dX);
    (void)hipFree(dY);
    return rc;
}
