// spmv_hll_spmm.hip -- Y = A X for k vectors per pass over an HLL handle: launcher and C-ABI (include/spmv_hip.h,
// "HLL: several vectors per pass").  Kernels: hll_spmm_kernels.hpp.  No plan of its own: the kernels run on the
// workgroup windows (hdesc) upload built for hll_lds and ignore the x-window, pattern and tile plans; k = 1 is the
// handle's SpMV launch.
#include "spmv_internal.hpp"

#include "hll_spmm_kernels.hpp"

namespace {

// column lanes per row group: the narrowest column tile (4 columns per lane) that holds k, up to 32 columns; wider
// k loops over tiles of 32 (the rule of the CSR launcher, spmv_spmm.hip)
int hll_spmm_column_lanes(int k) {
    if (k <= 4) return 1;
    if (k <= 8) return 2;
    if (k <= 16) return 4;
    return 8;
}

template <int CL, bool VEC>
void hll_spmm_launch_cfg(const spmv_hll_dev *m, int k, const double *X, double *Y, hipStream_t s) {
    const size_t lds = (size_t)m->stage_slots * (sizeof(double) + sizeof(int));
    hipLaunchKernelGGL((hll_spmm_block<CL, VEC>), dim3(m->num_blocks), dim3(kSpmmBlock), lds, s, m->num_blocks,
                       m->stage_slots, m->hdesc, m->hack_off, m->maxnz, m->JA, m->AS, X, Y, k);
    if (m->num_long_windows > 0)
        hipLaunchKernelGGL((hll_spmm_row<CL, VEC>), dim3(m->num_long_windows), dim3(kSpmmBlock), 0, s,
                           m->num_long_windows, m->long_windows, m->hdesc, m->hack_off, m->maxnz, m->JA, m->AS, X, Y,
                           k);
}

template <bool VEC>
void hll_spmm_launch_vec(const spmv_hll_dev *m, int k, const double *X, double *Y, hipStream_t s) {
    switch (hll_spmm_column_lanes(k)) {
        case 1: hll_spmm_launch_cfg<1, VEC>(m, k, X, Y, s); break;
        case 2: hll_spmm_launch_cfg<2, VEC>(m, k, X, Y, s); break;
        case 4: hll_spmm_launch_cfg<4, VEC>(m, k, X, Y, s); break;
        default: hll_spmm_launch_cfg<8, VEC>(m, k, X, Y, s); break;
    }
}

// Y (element 0 of the full M_total x k array) = A X on stream s; arguments checked by the caller
int hll_spmm_any(const spmv_hll_dev *m, int k, const double *X, double *Y, hipStream_t s) {
    if (k == 1) return hll_launch(m, SPMV_HLL_AUTO, X, Y, s);  // the handle's SpMV: the same bits
    if (m->M == 0) return 0;
    double *Yh = Y + (size_t)m->row0 * (size_t)k;
    const bool vec = (size_t)k * sizeof(double) % 16 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 15) == 0;
    if (vec) hll_spmm_launch_vec<true>(m, k, X, Yh, s);
    else hll_spmm_launch_vec<false>(m, k, X, Yh, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the rules of every entry point; -1 + message (and a clean HIP error state) when one is broken
int hll_spmm_check(const spmv_hll_dev *m, int k, const void *X, const void *Y, const char *what) {
    int rc = 0;
    if (!m || !X || !Y) rc = fail("%s: NULL argument", what);
    else if (k < 1) rc = fail("%s: k = %d, must be >= 1", what, k);
    else if (((uintptr_t)X | (uintptr_t)Y) % sizeof(double) != 0)
        rc = fail("%s: X / Y are not aligned to the element size (8 bytes)", what);
    if (rc) (void)hipGetLastError();
    return rc;
}

}  // namespace

extern "C" int spmv_hip_hll_spmm_on(spmv_hll_dev *m, int k, const void *d_X, void *d_Y, void *stream) {
    if (need_device()) return -1;
    if (hll_spmm_check(m, k, d_X, d_Y, "hll_spmm_on")) return -1;
    return hll_spmm_any(m, k, (const double *)d_X, (double *)d_Y, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_hll_spmm(spmv_hll_dev *m, int k, const double *X_host, double *Y_host) {
    if (need_device()) return -1;
    if (hll_spmm_check(m, k, X_host, Y_host, "hll_spmm")) return -1;
    const size_t kk = (size_t)k;
    // (+ one line: at k = 1 the SpMV kernels may read x in whole 128-byte lines, as the handle's own x allows)
    const size_t x_bytes = (size_t)m->N * kk * sizeof(double) + kLineBytes;
    const size_t y_bytes = std::max<size_t>((size_t)m->M_total * kk * sizeof(double), 16);
    double *dX = nullptr, *dY = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc((void **)&dX, x_bytes));
        HIP_TRY(hipMalloc((void **)&dY, y_bytes));
        HIP_TRY(hipMemsetAsync(dX, 0, x_bytes, g_stream));
        HIP_TRY(hipMemcpyAsync(dX, X_host, (size_t)m->N * kk * sizeof(double), hipMemcpyHostToDevice, g_stream));
        if (hll_spmm_any(m, k, dX, dY, g_stream)) return -1;
        // only the handle's rows go back: hack-range handles fill one shared Y
        const size_t off = (size_t)m->row0 * kk, len = (size_t)m->M * kk * sizeof(double);
        HIP_TRY(hipMemcpyAsync(Y_host + off, dY + off, len, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(g_stream);
    (void)hipFree(dX);
    (void)hipFree(dY);
    return rc;
}

extern "C" int spmv_hip_hll_spmm_time(spmv_hll_dev *m, int k, int warmup, int iters, float *ms_each) {
    if (need_device()) return -1;
    if (!m) return fail("hll_spmm_time: NULL handle");
    if (k < 1) return fail("hll_spmm_time: k = %d, must be >= 1", k);
    const size_t kk = (size_t)k;
    const size_t x_bytes = (size_t)m->N * kk * sizeof(double) + kLineBytes;
    const size_t y_bytes = std::max<size_t>((size_t)m->M_total * kk * sizeof(double), 16);
    double *dX = nullptr, *dY = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc((void **)&dX, x_bytes));
        HIP_TRY(hipMalloc((void **)&dY, y_bytes));
        HIP_TRY(hipMemsetAsync(dX, 0, x_bytes, g_stream));
        return time_loop(warmup, iters, ms_each, [&] { return hll_spmm_any(m, k, dX, dY, g_stream); },
                         [] { return 0; });
    };
    const int rc = body();
    (void)hipStreamSynchronize(g_stream);
    (void)hipFree(dX);
    (void)hipFree(dY);
    return rc;
}
