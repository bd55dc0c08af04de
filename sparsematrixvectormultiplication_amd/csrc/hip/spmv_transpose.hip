// spmv_transpose.hip -- spmv_hip_csr_transpose: A^T of a whole CSR handle, built on the device (include/spmv_hip.h).
//
//   tr_make_pairs   one wavefront per row: payload[e] = row << 32 | e for the row's entries (no per-entry search)
//   radix sort      (column, payload) pairs, stable, on the ceil(log2 N) bits a column can use (rocPRIM, as
//                   spmv_coo.hip): CSR entries are in row order, so each column's entries come out in ascending row
//                   order and entries that repeat a (row, column) pair keep their order in A
//   tr_gather       colT[k] = row, valT[k] = val[e] at every sorted position: values are moved, never combined
//   tr_row_ptr      row_ptr of A^T from the sorted columns (columns without entries included)
//
// Everything in front of the adopt is transpose_core, on a view of bare device arrays (the AMG device setup calls it
// too); algebra_ops.hpp has the frame the handle producers share.
// The columns of A are the sort's key input as they are; only the N + 1 row pointers of A^T cross to the host, and
// the arrays go to csr_upload_impl through the adopt path, so A^T gets every plan and search an upload gives.
#include "algebra_ops.hpp"

#include <rocprim/rocprim.hpp>

namespace {

constexpr int kTrWaves = kBlock / 64;
constexpr int kTrMaxGrid = 1 << 20;  // grid cap of the row kernel (rows stride over the waves beyond it)

__global__ __launch_bounds__(kBlock) void tr_make_pairs(int M, const int *__restrict__ row_ptr,
                                                        unsigned long long *__restrict__ payload) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kTrWaves;
    for (long long r = (long long)blockIdx.x * kTrWaves + (threadIdx.x >> 6); r < M; r += waves) {
        const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
        const unsigned long long hi = (unsigned long long)r << 32;
        for (int e = e0 + lane; e < e1; e += 64) payload[e] = hi | (unsigned)e;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tr_gather(long long nz, const unsigned long long *__restrict__ payload,
                                                    const T *__restrict__ val, int *__restrict__ colT,
                                                    T *__restrict__ valT) {
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= nz) return;
    const unsigned long long p = payload[k];
    colT[k] = (int)(p >> 32);
    valT[k] = val[(unsigned)p];
}

// sorted columns -> row_ptr of A^T, N + 1 entries (columns without entries included)
__global__ __launch_bounds__(kBlock) void tr_row_ptr(long long nz, int N, const unsigned *__restrict__ key,
                                                     int *__restrict__ row_ptr) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e > nz) return;
    if (e == nz) {  // columns behind the last entry's column (all of them when nz == 0)
        const int last = nz ? (int)key[nz - 1] : -1;
        for (int c = last + 1; c <= N; ++c) row_ptr[c] = (int)nz;
        return;
    }
    const int c = (int)key[e];
    const int prev = e ? (int)key[e - 1] : -1;
    for (int q = prev + 1; q <= c; ++q) row_ptr[q] = (int)e;  // usually zero or one iteration
}

// the transpose on bare arrays: everything but the adopt
template <typename T>
int transpose_core_t(const CsrView &A, DevCsr &At_out, std::vector<int> &rp) {
    const CsrView *m = &A;
    const int M = m->rows, N = m->cols;
    const long long nz = m->nz;
    const size_t n = (size_t)nz;
    ClearHipError clear;
    DevBuf d_pin, d_pout, d_kout, d_tmp;
    DevCsr At(N, M);
    rp.assign((size_t)N + 1, 0);
    UploadTrace trace("csr_transpose");  // SPMV_TRACE_UPLOAD=1: the build here, then upload's own phases
    hipError_t e = d_pin.alloc(n * sizeof(unsigned long long));
    if (e == hipSuccess) e = d_pout.alloc(n * sizeof(unsigned long long));
    if (e == hipSuccess) e = d_kout.alloc(n * sizeof(unsigned));
    if (e == hipSuccess) e = At.alloc_entries<T>(nz, kPad, g_stream);
    if (e == hipSuccess) e = At.alloc_rp();
    if (e != hipSuccess) return fail("csr_transpose: allocation failed: %s", hipGetErrorString(e));
    if (n) {
        const int rgrid = (int)std::min<long long>(kTrMaxGrid, ((long long)M + kTrWaves - 1) / kTrWaves);
        hipLaunchKernelGGL(tr_make_pairs, dim3(rgrid), dim3(kBlock), 0, g_stream, M, m->rp, d_pin.as<unsigned long long>());
        // only the bits a column index can use (a matrix of one column: a single bit, every key 0)
        const unsigned col_bits = std::min(32u, algebra::bits_for((unsigned long long)N));
        const unsigned *keys = reinterpret_cast<const unsigned *>(m->col);  // columns are in [0, N)
        size_t tmp_bytes = 0;
        e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, d_kout.as<unsigned>(), d_pin.as<unsigned long long>(),
                                      d_pout.as<unsigned long long>(), n, 0u, col_bits, g_stream);
        if (e == hipSuccess) e = d_tmp.alloc(tmp_bytes);
        if (e == hipSuccess)
            e = rocprim::radix_sort_pairs(d_tmp.p, tmp_bytes, keys, d_kout.as<unsigned>(), d_pin.as<unsigned long long>(),
                                          d_pout.as<unsigned long long>(), n, 0u, col_bits, g_stream);
        if (e != hipSuccess) return fail("csr_transpose: sort failed: %s", hipGetErrorString(e));
        const int egrid = (int)((nz + kBlock - 1) / kBlock);
        hipLaunchKernelGGL((tr_gather<T>), dim3(egrid), dim3(kBlock), 0, g_stream, nz, d_pout.as<unsigned long long>(),
                           (const T *)m->val, At.col, static_cast<T *>(At.val));
    }
    const int pgrid = (int)((nz + kBlock) / kBlock);  // covers e == nz as well
    hipLaunchKernelGGL(tr_row_ptr, dim3(pgrid), dim3(kBlock), 0, g_stream, nz, N, d_kout.as<unsigned>(), At.rp);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(rp.data(), At.rp, rp.size() * sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_transpose: build failed: %s", hipGetErrorString(e));
    trace.mark("device build");
    At_out = std::move(At);
    return 0;
}

// core, then the adopt: A^T is an ordinary handle with upload's plans
template <typename T>
int transpose_body(const spmv_csr_dev *m, spmv_csr_dev **out) {
    DevCsr At;
    std::vector<int> rp;
    if (transpose_core_t<T>(csr_view(m), At, rp)) return -1;
    return algebra::adopt<T>(std::move(At), rp, out);
}

}  // namespace

int transpose_core(int value_bytes, const CsrView &A, DevCsr &At, std::vector<int> &rp_host) {
    return value_bytes == 8 ? transpose_core_t<double>(A, At, rp_host) : transpose_core_t<float>(A, At, rp_host);
}

extern "C" int spmv_hip_csr_transpose(const spmv_csr_dev *m, spmv_csr_dev **out) {
    if (need_device()) return -1;
    if (!out) return fail("csr_transpose: out is NULL");
    *out = nullptr;
    if (!m) return fail("csr_transpose: NULL handle");
    if (algebra::operand_ok("csr_transpose", nullptr, "transpose", m)) return -1;
    if ((unsigned long long)m->M_total * (unsigned long long)m->value_bytes >= (1ull << 32))
        return fail("csr_transpose: M = %d: the transpose's x exceeds the 32-bit gather offset range of the kernels",
                    m->M_total);
    return guarded("csr_transpose", [&] {
        return m->value_bytes == 8 ? transpose_body<double>(m, out) : transpose_body<float>(m, out);
    });
}
