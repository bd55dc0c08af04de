// spmv_coo.hip -- COO -> CSR on the device: the reference's convert_in_csr
// (src/csr_matrix.c:63-126: histogram, scan, scatter in file order, per-row quicksort on the host)
// as upload of the triplets + one stable radix sort by (row, column) + two small kernels.  The sort
// is rocPRIM's (a ROCm library routine; nothing on the SpMV path goes through it).  The build's arrays are DevBuf and an
// owning DevCsr, the adopt and the sort width are the handle producers' (algebra_ops.hpp).
#include "algebra_ops.hpp"

#include <rocprim/rocprim.hpp>

namespace {

// key = row << 32 | column; out-of-range indices are reported through *bad (first offender wins)
__global__ __launch_bounds__(kBlock) void coo_make_keys(long long nz, int M, int N, const int *__restrict__ I,
                                                        const int *__restrict__ J, unsigned long long *__restrict__ key,
                                                        unsigned long long *__restrict__ bad) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= nz) return;
    const int r = I[e], c = J[e];
    if ((unsigned)r >= (unsigned)M || (unsigned)c >= (unsigned)N) atomicMin(bad, (unsigned long long)e);
    key[e] = ((unsigned long long)(unsigned)r << 32) | (unsigned)c;
}

// sorted keys -> col[e] and row_ptr (rows without entries included)
__global__ __launch_bounds__(kBlock) void coo_split_keys(long long nz, int M, const unsigned long long *__restrict__ key,
                                                         int *__restrict__ col, int *__restrict__ row_ptr) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e > nz) return;
    if (e == nz) {  // rows behind the last entry's row (all rows when nz == 0)
        const int last = nz ? (int)(key[nz - 1] >> 32) : -1;
        for (int r = last + 1; r <= M; ++r) row_ptr[r] = (int)nz;
        return;
    }
    const unsigned long long k = key[e];
    col[e] = (int)(unsigned)k;
    const int r = (int)(k >> 32);
    const int prev = e ? (int)(key[e - 1] >> 32) : -1;
    for (int q = prev + 1; q <= r; ++q) row_ptr[q] = (int)e;  // usually zero or one iteration
}

}  // namespace

// COO triplets (0-based, any order, file order = tie order) -> a CSR handle, built on the device.
// Equal to convert_in_csr + spmv_hip_csr_upload except for the order of entries that repeat the same
// (row, column): the stable sort keeps them in file order, the reference's quicksort does not.
static int spmv_hip_csr_from_coo_body(int M, int N, long long nz, const int *I, const int *J, const double *val,
                                     spmv_csr_dev **out) {
    if (need_device()) return -1;
    if (!out) return fail("csr_from_coo: out is NULL");
    *out = nullptr;
    if (M < 0 || N < 0 || nz < 0 || nz > kMaxEntries || (nz > 0 && (!I || !J || !val)))
        return fail("csr_from_coo: bad arguments");
    const size_t n = (size_t)nz;
    ClearHipError clear;
    DevBuf d_I, d_J, d_vin, d_kin, d_kout, d_bad, d_tmp;
    DevCsr C(M, N);
    std::vector<int> rp((size_t)M + 1, 0);
    hipError_t e = d_I.alloc(n * sizeof(int));
    if (e == hipSuccess) e = d_J.alloc(n * sizeof(int));
    if (e == hipSuccess) e = d_vin.alloc(n * sizeof(double));
    if (e == hipSuccess) e = d_kin.alloc(n * sizeof(unsigned long long));
    if (e == hipSuccess) e = d_kout.alloc(n * sizeof(unsigned long long));
    if (e == hipSuccess) e = C.alloc_entries<double>(nz, kPad, g_stream);
    if (e == hipSuccess) e = C.alloc_rp();
    if (e == hipSuccess) e = d_bad.alloc(sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(d_bad.p, 0xFF, sizeof(unsigned long long), g_stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_I.p, I, n * sizeof(int), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_J.p, J, n * sizeof(int), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_vin.p, val, n * sizeof(double), hipMemcpyHostToDevice, g_stream);
    if (e != hipSuccess) return fail("csr_from_coo: allocation / upload failed: %s", hipGetErrorString(e));
    unsigned long long *kin = d_kin.as<unsigned long long>(), *kout = d_kout.as<unsigned long long>();
    const int grid = (int)((nz + kBlock) / kBlock);  // covers e == nz as well
    if (n) {
        hipLaunchKernelGGL(coo_make_keys, dim3(grid), dim3(kBlock), 0, g_stream, nz, M, N, d_I.as<int>(), d_J.as<int>(), kin,
                           d_bad.as<unsigned long long>());
        // only the bits that can differ: 32 of the column + those of the row
        const unsigned row_bits = std::min(32u, algebra::bits_for((unsigned long long)std::max(M, 1)));
        double *vin = d_vin.as<double>(), *vout = static_cast<double *>(C.val);
        size_t tmp_bytes = 0;
        e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin, kout, vin, vout, n, 0u, 32u + row_bits, g_stream);
        if (e == hipSuccess) e = d_tmp.alloc(tmp_bytes);
        if (e == hipSuccess) e = rocprim::radix_sort_pairs(d_tmp.p, tmp_bytes, kin, kout, vin, vout, n, 0u, 32u + row_bits, g_stream);
        if (e != hipSuccess) return fail("csr_from_coo: sort failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(coo_split_keys, dim3(grid), dim3(kBlock), 0, g_stream, nz, M, kout, C.col, C.rp);
    unsigned long long bad = 0;
    e = hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rp.data(), C.rp, rp.size() * sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_from_coo: build failed: %s", hipGetErrorString(e));
    if (bad != ~0ull) return fail("csr_from_coo: entry %llu (%d, %d) is outside the %d x %d matrix", bad, I[bad], J[bad], M, N);
    return algebra::adopt<double>(std::move(C), rp, out);
}

extern "C" int spmv_hip_csr_from_coo(int M, int N, long long nz, const int *I, const int *J, const double *val,
                                     spmv_csr_dev **out) {
    return guarded("csr_from_coo", [&] { return spmv_hip_csr_from_coo_body(M, N, nz, I, J, val, out); });
}

// The CSR arrays of a handle back to the host (tests; hosts that let the device build the matrix):
// row_ptr[M_local + 1] (rebased to 0), col[nz], val[nz] of the handle's dtype; any pointer may be NULL.
extern "C" int spmv_hip_csr_download(const spmv_csr_dev *m, int *row_ptr, int *col, void *val) {
    if (need_device()) return -1;
    if (!m) return fail("csr_download: NULL handle");
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (row_ptr) HIP_TRY(hipMemcpy(row_ptr, m->row_ptr, ((size_t)m->M_local + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (col && m->nz) HIP_TRY(hipMemcpy(col, m->col, (size_t)m->nz * sizeof(int), hipMemcpyDeviceToHost));
    if (val && m->nz) HIP_TRY(hipMemcpy(val, m->val, (size_t)m->nz * m->value_bytes, hipMemcpyDeviceToHost));
    return 0;
}
