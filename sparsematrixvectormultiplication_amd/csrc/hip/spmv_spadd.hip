// spmv_spadd.hip -- spmv_hip_csr_add: C = alpha A + beta B of two whole CSR handles (or alpha canon(A)) as a new handle,
// built on the device (include/spmv_hip.h has the definition; spadd_kernels.hpp the kernels).
//
//   check      sa_check over each operand: are its rows strictly ascending?  two flags to the host
//   canonical  an operand that is not (or every operand, method 2) becomes canon(X) = X I through the product's core
//              (spgemm_core) on a view of the operand and a view of the identity's bare arrays; the result stays bare
//              arrays: no handle, no adopt
//   symbolic   sa_long_rows lists the long rows; sa_merge_rows<T, false> and sa_merge_long<T, false> count the matches:
//              the entries of every row of C, 4 bytes per row to the host, which makes row_ptr of them
//   numeric    col / val of C at their exact size; sa_merge_rows<T, true> and sa_merge_long<T, true>
//   adopt      csr_adopt_*: C is an ordinary handle with upload's plans
//
// Everything in front of the adopt is spadd_core, on views of bare device arrays (algebra_ops.hpp has the frame).
//
// The workspace is the per-row counts, the list of long rows, C's row_ptr and, with B absent, a row_ptr of zeros.
#include "algebra_ops.hpp"

#include <cmath>

#include "spadd_kernels.hpp"

namespace {

int log2_of(int pow2) {
    int k = 0;
    while ((1 << k) < pow2) ++k;
    return k;
}

// canon(X) = X I_N through the product's own tiers; the identity's row_ptr and col are one array 0 .. N
template <typename T>
int canonical_of(const CsrView &x, DevCsr &out) {
    const int N = x.cols;
    DevBuf d_iota, d_ones;
    hipError_t e = d_iota.alloc(((size_t)N + 1) * sizeof(int));
    if (e == hipSuccess) e = d_ones.alloc((size_t)N * sizeof(T));
    if (e != hipSuccess) return fail("csr_add: allocation of the identity of %d columns failed: %s", N, hipGetErrorString(e));
    hipLaunchKernelGGL((sa_identity<T>), dim3((unsigned)(((long long)N + kBlock) / kBlock)), dim3(kBlock), 0, g_stream, N,
                       d_iota.as<int>(), d_ones.as<T>());
    HIP_TRY(hipGetLastError());
    const CsrView eye = {N, N, N, d_iota.as<int>(), d_iota.as<int>(), d_ones.p};
    std::vector<int> rp_host;
    return spgemm_core((int)sizeof(T), x, eye, 0, 0, out, rp_host, nullptr, nullptr);  // (waits for the stream)
}

// the sum on bare arrays: everything but the adopt.  b: NULL (C = alpha canon(a)), or a itself (one check, one canon(a))
template <typename T>
int spadd_core_t(const CsrView *a, double alpha, const CsrView *b, double beta, int method, int lanes_arg, int long_arg,
                 DevCsr &C_out, std::vector<int> &rp, long long *stats, double *ms) {
    const int M = a->rows, N = a->cols;
    UploadTrace trace("csr_add");
    double split[4] = {0, 0, 0, 0};
    algebra::PhaseTimer timer{split};
    ClearHipError clear;
    DevCsr C(M, N);

    // ---- check
    int first_bad[2] = {0x7fffffff, 0x7fffffff};
    DevBuf d_flags;  // {first offending row of A, of B, long rows}
    hipError_t e = d_flags.alloc(4 * sizeof(int));
    if (e != hipSuccess) return fail("csr_add: allocation of the flags failed: %s", hipGetErrorString(e));
    {
        const int init[4] = {first_bad[0], first_bad[1], 0, 0};
        HIP_TRY(hipMemcpyAsync(d_flags.p, init, sizeof(init), hipMemcpyHostToDevice, g_stream));
        constexpr int kRows = kBlock / kSaCheckLanes;
        const unsigned grid = (unsigned)(((long long)M + kRows - 1) / kRows);
        if (M) {
            hipLaunchKernelGGL(sa_check, dim3(grid), dim3(kBlock), 0, g_stream, M, a->rp, a->col, d_flags.as<int>());
            if (b && b != a)
                hipLaunchKernelGGL(sa_check, dim3(grid), dim3(kBlock), 0, g_stream, M, b->rp, b->col, d_flags.as<int>() + 1);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(first_bad, d_flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail("csr_add: check failed: %s", hipGetErrorString(e));
        if (b == a) first_bad[1] = first_bad[0];
    }
    const bool a_canon = first_bad[0] == 0x7fffffff, b_canon = first_bad[1] == 0x7fffffff;
    if (method == 1 && !(a_canon && b_canon))
        return fail("csr_add: %s is not canonical: row %d is the first whose columns do not ascend strictly; method = 1 (merge "
                    "only) takes canonical operands",
                    a_canon ? "B" : "A", a_canon ? first_bad[1] : first_bad[0]);
    timer.lap(0);
    trace.mark("check");

    // ---- canonical
    DevCsr ca, cb;
    CsrView va = *a, vb = b ? *b : CsrView();
    if (method == 2 || !a_canon) {
        if (canonical_of<T>(*a, ca)) return -1;
        va = ca.view();
    }
    if (b && b != a && (method == 2 || !b_canon)) {
        if (canonical_of<T>(*b, cb)) return -1;
        vb = cb.view();
    }
    const CsrView *A = &va;
    const CsrView *B = !b ? nullptr : b == a ? A : &vb;
    timer.lap(1);
    trace.mark("canonical");

    // ---- symbolic
    const long long nzA = A->nz, nzB = B ? B->nz : 0;
    int lanes = lanes_arg;
    if (lanes == 0) lanes = std::min(64, pow2_floor((int)std::max<long long>(1, M ? (nzA + nzB) / M : 1)));
    const int lanes_log2 = log2_of(lanes);
    const int long_from = long_arg ? long_arg : std::min(kSaLongRow, std::max(kBlock, lanes * kSaTrips));
    DevBuf d_cnt, d_long, d_zero;
    e = d_cnt.alloc((size_t)M * sizeof(int));
    if (e == hipSuccess) e = d_long.alloc((size_t)M * sizeof(int));
    if (e == hipSuccess) e = C.alloc_rp();
    if (e == hipSuccess && !B) {
        e = d_zero.alloc(((size_t)M + 1) * sizeof(int));
        if (e == hipSuccess) e = hipMemsetAsync(d_zero.p, 0, std::max<size_t>(((size_t)M + 1) * sizeof(int), 16), g_stream);
    }
    if (e != hipSuccess) return fail("csr_add: allocation of the counts of %d rows failed: %s", M, hipGetErrorString(e));
    trace.mark("workspace");
    const int *rpA = A->rp, *colA = A->col, *rpB = B ? B->rp : d_zero.as<int>(), *colB = B ? B->col : A->col;
    const T *valA = static_cast<const T *>(A->val), *valB = B ? static_cast<const T *>(B->val) : valA;
    int *d_nlong = d_flags.as<int>() + 2;
    int *d_colC = nullptr;  // (C's, once the symbolic pass has counted them)
    T *d_valC = nullptr;
    const unsigned row_grid = (unsigned)((((long long)M << lanes_log2) + kBlock - 1) / kBlock);
    int n_long = 0;  // known after the symbolic pass, whose own launch for the long rows is sized blind
    auto run = [&](bool numeric) {
        if (!M) return;
        if (numeric) {
            hipLaunchKernelGGL((sa_merge_rows<T, true>), dim3(row_grid), dim3(kBlock), 0, g_stream, M, lanes_log2, long_from, rpA,
                               colA, valA, rpB, colB, valB, alpha, beta, d_cnt.as<int>(), C.rp, d_colC, d_valC);
            if (n_long)
                hipLaunchKernelGGL((sa_merge_long<T, true>), dim3((unsigned)std::min(n_long, kSaLongGrid)), dim3(kBlock), 0,
                                   g_stream, d_nlong, d_long.as<int>(), rpA, colA, valA, rpB, colB, valB, alpha, beta,
                                   d_cnt.as<int>(), C.rp, d_colC, d_valC);
        } else {
            hipLaunchKernelGGL(sa_long_rows, dim3((unsigned)(((long long)M + kBlock - 1) / kBlock)), dim3(kBlock), 0, g_stream, M,
                               rpA, rpB, long_from, d_nlong, d_long.as<int>());
            hipLaunchKernelGGL((sa_merge_rows<T, false>), dim3(row_grid), dim3(kBlock), 0, g_stream, M, lanes_log2, long_from, rpA,
                               colA, valA, rpB, colB, valB, alpha, beta, d_cnt.as<int>(), C.rp, d_colC, d_valC);
            hipLaunchKernelGGL((sa_merge_long<T, false>), dim3((unsigned)std::min(M, kSaLongGrid)), dim3(kBlock), 0, g_stream, d_nlong, d_long.as<int>(), rpA,
                               colA, valA, rpB, colB, valB, alpha, beta, d_cnt.as<int>(), C.rp, d_colC, d_valC);
        }
    };
    std::vector<int> cnt((size_t)M, 0);
    run(false);
    trace.mark("symbolic kernels");
    e = hipGetLastError();
    if (e == hipSuccess && M) e = hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_long, d_nlong, sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_add: symbolic pass failed: %s", hipGetErrorString(e));
    RowCounts counts;
    if (algebra::row_ptr_of_counts("csr_add", cnt, rp, counts)) return -1;
    const long long nz = counts.nz;
    timer.lap(2);
    trace.mark("symbolic");

    // ---- numeric
    e = C.alloc_entries<T>(nz, kPad, g_stream);
    if (e != hipSuccess) return fail("csr_add: allocation of C's %lld entries failed: %s", nz, hipGetErrorString(e));
    d_colC = C.col, d_valC = static_cast<T *>(C.val);
    e = hipMemcpyAsync(C.rp, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess) {
        run(true);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_add: numeric pass failed: %s", hipGetErrorString(e));
    timer.lap(3);
    trace.mark("numeric");
    C_out = std::move(C);
    if (stats) {
        const long long s[6] = {nz, nzA + nzB - nz, a_canon ? 1 : 0, b_canon ? 1 : 0, n_long, counts.widest};
        std::copy(s, s + 6, stats);
    }
    if (ms) std::copy(split, split + 4, ms);
    return 0;
}

// core, then the adopt: C is an ordinary handle with upload's plans
template <typename T>
int add_body(const spmv_csr_dev *a, double alpha, const spmv_csr_dev *b, double beta, int method, int lanes, int long_row,
             spmv_csr_dev **out, long long *stats, double *ms) {
    const CsrView va = csr_view(a), vb = b ? csr_view(b) : CsrView();
    DevCsr C;
    std::vector<int> rp;
    double split[5] = {0, 0, 0, 0, 0};
    if (spadd_core_t<T>(&va, alpha, !b ? nullptr : b == a ? &va : &vb, beta, method, lanes, long_row, C, rp, stats, split)) return -1;
    algebra::PhaseTimer timer{split};
    const int rc = algebra::adopt<T>(std::move(C), rp, out);
    timer.lap(4);
    if (rc) return rc;
    if (ms) std::copy(split, split + 5, ms);
    return 0;
}

}  // namespace

int spadd_core(int value_bytes, const CsrView *a, double alpha, const CsrView *b, double beta, int method, int lanes,
               int long_row, DevCsr &C, std::vector<int> &rp_host, long long *stats, double *ms) {
    return value_bytes == 8 ? spadd_core_t<double>(a, alpha, b, beta, method, lanes, long_row, C, rp_host, stats, ms)
                            : spadd_core_t<float>(a, alpha, b, beta, method, lanes, long_row, C, rp_host, stats, ms);
}

extern "C" int spmv_hip_csr_add(const spmv_csr_dev *a, double alpha, const spmv_csr_dev *b, double beta, int method, int lanes,
                                int long_row, spmv_csr_dev **out, long long *stats, double *ms) {
    if (need_device()) return -1;
    if (!out) return fail("csr_add: out is NULL");
    *out = nullptr;
    if (!a) return fail("csr_add: NULL handle (a = %p)", (const void *)a);
    if (algebra::operand_ok("csr_add", "A", "add", a) || (b && algebra::operand_ok("csr_add", "B", "add", b))) return -1;
    if (b && (a->M_total != b->M_total || a->N != b->N))
        return fail("csr_add: A is %d x %d and B is %d x %d: the shapes must agree", a->M_total, a->N, b->M_total, b->N);
    if (b && a->value_bytes != b->value_bytes)
        return fail("csr_add: A holds %d-byte values and B %d-byte values; the dtypes must agree", a->value_bytes, b->value_bytes);
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return fail("csr_add: alpha = %g, beta = %g; both must be finite", alpha, beta);
    if (method < 0 || method > 2) return fail("csr_add: method = %d; 0 (auto), 1 (merge only) or 2 (canonicalise first)", method);
    if (lanes != 0 && (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0))
        return fail("csr_add: lanes = %d; 0 (auto) or a power of two in [1, 64]", lanes);
    if (long_row < 0) return fail("csr_add: long_row = %d; 0 (auto) or the combined row length of a long row, at least 1", long_row);
    return guarded("csr_add", [&] {
        return a->value_bytes == 8 ? add_body<double>(a, alpha, b, beta, method, lanes, long_row, out, stats, ms)
                                   : add_body<float>(a, alpha, b, beta, method, lanes, long_row, out, stats, ms);
    });
}
