// spmv_precond.hip -- Jacobi and block-Jacobi preconditioners of CSR handles, built and applied on the device
// (include/spmv_hip.h).
//
// The build: pc_extract gathers the diagonal (or each block's b x b diagonal block) in fp64 from the handle's CSR
// arrays, pc_invert_diag / pc_invert_block invert it into P's own array (precond_kernels.hpp).  Only two ints cross to
// the host: the first row without its diagonal entry and the first bad row or block.  The fp64 blocks are a temporary
// of ceil(rows / b) b^2 doubles, freed on every path.
//
// The other kinds are the same spmv_precond with a family table and the family's own object in P->impl
// (precond_kernels.hpp), built and applied by the file that owns the family: SSOR and ILU(0) in spmv_trsv.hip, FSAI in
// spmv_fsai.hip, AMG in spmv_amg.hip and spmv_amg_setup.hip, CHEBYSHEV in spmv_cheb.hip.  free / info / apply /
// apply_on / factors here go through the table and name no kind.
#include "spmv_internal.hpp"

#include <climits>

#include "precond_kernels.hpp"

namespace {

constexpr int kPcMaxGrid = 1 << 20;  // grid cap of the build kernels (they stride beyond it)

// the stored inverse of m's diagonal blocks of b rows in a new array (*inv_out, the caller's on 0); the refusals name `what`
template <typename T>
int precond_invert(const spmv_csr_dev *m, int b, const char *what, void **inv_out) {
    const int n = m->M_local;
    const long long nblocks = ((long long)n + b - 1) / b;
    const size_t entries = std::max<size_t>((size_t)nblocks * b * b, 1);
    const size_t inv_bytes = std::max<size_t>(entries * sizeof(T), 16);
    double *D = nullptr;
    int *bad = nullptr;
    void *inv = nullptr;
    int rc = -1;
    do {
        hipError_t e = hipMalloc((void **)&D, entries * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(&inv, inv_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&bad, 2 * sizeof(int));
        if (e == hipSuccess) e = hipMemsetAsync(D, 0, entries * sizeof(double), g_stream);
        if (e == hipSuccess) e = hipMemsetAsync(inv, 0, inv_bytes, g_stream);
        const int none[2] = {INT_MAX, INT_MAX};
        if (e == hipSuccess) e = hipMemcpy(bad, none, sizeof none, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            fail("%s: allocation failed: %s", what, hipGetErrorString(e));
            break;
        }
        if (n) {
            const int rgrid = (int)std::min<long long>(kPcMaxGrid, ((long long)n + kPcWaves - 1) / kPcWaves);
            hipLaunchKernelGGL((pc_extract<T>), dim3(rgrid), dim3(kBlock), 0, g_stream, n, m->row0, b, m->row_ptr,
                               m->col, (const T *)m->val, D, bad);
            if (b == 1) {
                const int grid = (int)std::min<long long>(kPcMaxGrid, ((long long)n + kBlock - 1) / kBlock);
                hipLaunchKernelGGL((pc_invert_diag<T>), dim3(grid), dim3(kBlock), 0, g_stream, n, (const double *)D,
                                   (T *)inv, bad);
            } else {
                const int grid = (int)std::min<long long>(kPcMaxGrid, nblocks);
                hipLaunchKernelGGL((pc_invert_block<T>), dim3(grid), dim3(64), 0, g_stream, n, b, (const double *)D,
                                   (T *)inv, bad);
            }
        }
        int h[2] = {INT_MAX, INT_MAX};
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h, bad, sizeof h, hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) {
            fail("%s: build failed: %s", what, hipGetErrorString(e));
            break;
        }
        if (h[0] != INT_MAX) {
            fail("%s: row %d (global row %d) has no diagonal entry", what, h[0], m->row0 + h[0]);
            break;
        }
        if (h[1] != INT_MAX) {
            if (b == 1)
                fail("%s: row %d (global row %d): the diagonal is zero or not finite, or so small that "
                     "its inverse is not finite", what, h[1], m->row0 + h[1]);
            else
                fail("%s: block %d (global rows [%d, %d)): a zero or non-finite pivot, or an inverse "
                     "that is not finite", what, h[1], m->row0 + h[1] * b, m->row0 + (int)std::min<long long>(
                                                                                          (long long)(h[1] + 1) * b, n));
            break;
        }
        *inv_out = inv;
        inv = nullptr;  // the caller's now
        rc = 0;
    } while (0);
    (void)hipFree(D);
    (void)hipFree(bad);
    (void)hipFree(inv);
    return rc;
}

template <typename T>
int precond_build(const spmv_csr_dev *m, int kind, int b, spmv_precond **out) {
    void *inv = nullptr;
    if (precond_invert<T>(m, b, "csr_precond_build", &inv)) return -1;
    *out = precond_new(m, kind, b, sizeof(T));
    (*out)->inv = inv;  // P owns it
    return 0;
}

// JACOBI / BLOCK_JACOBI from m's values: the device build once more into an array of its own, copied over P's only when
// no row or block was refused
template <typename T>
int precond_refresh_inverse(spmv_precond *P, const spmv_csr_dev *m) {
    void *inv = nullptr;
    if (precond_invert<T>(m, P->block, "precond_refresh", &inv)) return -1;
    const long long nblocks = ((long long)P->rows + P->block - 1) / P->block;
    const size_t bytes = (size_t)nblocks * P->block * P->block * sizeof(T);
    hipError_t e = bytes ? hipMemcpyAsync(P->inv, inv, bytes, hipMemcpyDeviceToDevice, g_stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    (void)hipFree(inv);
    if (e != hipSuccess) return fail("precond_refresh: the copy failed: %s", hipGetErrorString(e));
    return 0;
}

int precond_apply_launch(const spmv_precond *P, const void *d_r, void *d_z, hipStream_t s) {
    if (!P->rows) return 0;
    if (P->value_bytes == 8 ? precond_apply<double>(P, d_r, d_z, nullptr, s) : precond_apply<float>(P, d_r, d_z, nullptr, s))
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// the stamp of handle m (waits for the device); -1: HIP error
int pattern_stamp(const spmv_csr_dev *m, PatternStamp &out) {
    DevBuf d;
    HIP_TRY(d.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(unsigned long long), g_stream));
    hipLaunchKernelGGL((spmv::rf_digest<int>), dim3(spmv::rf_grid(m->M_local + 1LL)), dim3(kBlock), 0, g_stream, m->M_local + 1LL,
                       (const int *)m->row_ptr, 0ull, d.as<unsigned long long>());
    if (m->nz)
        hipLaunchKernelGGL((spmv::rf_digest<int>), dim3(spmv::rf_grid(m->nz)), dim3(kBlock), 0, g_stream, (long long)m->nz,
                           (const int *)m->col, 1ull << 31, d.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&out.digest, d.p, sizeof out.digest, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    out.have = true;
    out.nz = m->nz;
    out.rows = m->M_local;
    out.cols = m->N;
    return 0;
}

// m's pattern against the stamp (taken now when there is none yet); -1 with a message naming `what`
int pattern_check(const spmv_csr_dev *m, PatternStamp &stamp, const char *what) {
    PatternStamp now;
    if (pattern_stamp(m, now)) return -1;
    if (!stamp.have) {
        stamp = now;
        return 0;
    }
    if (now.digest != stamp.digest || now.nz != stamp.nz || now.rows != stamp.rows || now.cols != stamp.cols)
        return fail("%s: the handle's pattern is not the one this object was refreshed from first: a changed pattern "
                    "needs a new build", what);
    return 0;
}

extern "C" int spmv_hip_csr_precond_build(const spmv_csr_dev *m, int kind, int block, spmv_precond **out) {
    auto check = [&] {
        if (kind != SPMV_PRECOND_JACOBI && kind != SPMV_PRECOND_BLOCK_JACOBI)
            return fail("csr_precond_build: kind = %d, must be SPMV_PRECOND_JACOBI or SPMV_PRECOND_BLOCK_JACOBI", kind);
        if (kind == SPMV_PRECOND_JACOBI && block != 1) return fail("csr_precond_build: JACOBI takes block = 1, not %d", block);
        if (block < 1 || block > kPcMaxBlock)
            return fail("csr_precond_build: block = %d, must be in [1, %d]", block, kPcMaxBlock);
        return 0;
    };
    return precond_build_frame("csr_precond_build", m, out, check, [&](auto t, spmv_precond **P) {
        return precond_build<decltype(t)>(m, kind, block, P);
    });
}

// P from the values m holds now (include/spmv_hip.h): the shared checks, then the kind's own refresh
extern "C" int spmv_hip_precond_refresh(spmv_precond *P, const spmv_csr_dev *m) {
    if (need_device()) return -1;
    if (!P || !m) return fail("precond_refresh: NULL argument");
    if (P->family && !P->family->refresh)
        return fail("precond_refresh: a preconditioner of kind %d (%s) depends on the values: its pattern, hierarchy or "
                    "interval is a function of them.  Build it again", P->kind, P->family->name);
    if (precond_matches(m, P, "precond_refresh") || handle_ok(m, "precond_refresh")) return -1;
    const bool stamped = P->stamp.have;
    const int rc = guarded("precond_refresh", [&] {
        if (pattern_check(m, P->stamp, "precond_refresh")) return -1;
        if (P->family) return P->family->refresh(P, m);
        return P->value_bytes == 8 ? precond_refresh_inverse<double>(P, m) : precond_refresh_inverse<float>(P, m);
    });
    // JACOBI / BLOCK_JACOBI keep nothing made from the pattern: a first refresh that is refused leaves no stamp behind.
    // A family with maps keeps stamp and maps together (its refresh drops the stamp when it installs no maps).
    if (rc && !stamped && !P->family) P->stamp = PatternStamp();
    (void)hipGetLastError();
    return rc;
}

extern "C" void spmv_hip_precond_free(spmv_precond *P) {
    if (!P) return;
    (void)hipFree(P->inv);
    if (P->family) P->family->free(P->impl);
    delete P;
}

extern "C" int spmv_hip_precond_info(const spmv_precond *P, int *info) {
    if (!P || !info) return fail("precond_info: bad arguments");
    info[0] = P->kind;
    info[1] = P->block;
    info[2] = P->rows;
    info[3] = P->row0;
    info[4] = P->value_bytes;
    return 0;
}

extern "C" int spmv_hip_precond_apply_on(const spmv_precond *P, const void *d_r, void *d_z, void *stream) {
    if (need_device()) return -1;
    if (!P || (P->rows && (!d_r || !d_z))) return fail("precond_apply_on: bad arguments");
    if (((uintptr_t)d_r | (uintptr_t)d_z) % (uintptr_t)P->value_bytes)
        return fail("precond_apply_on: r and z must be aligned to %d bytes", P->value_bytes);
    return precond_apply_launch(P, d_r, d_z, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_precond_apply(const spmv_precond *P, const void *r_host, void *z_host) {
    if (need_device()) return -1;
    if (!P || (P->rows && (!r_host || !z_host))) return fail("precond_apply: bad arguments");
    return guarded("precond_apply", [&] {
        const size_t bytes = (size_t)P->rows * P->value_bytes;
        SolverScope scope;
        void *r = scope.alloc(std::max<size_t>(bytes, 16));
        void *z = scope.alloc(std::max<size_t>(bytes, 16));
        hipError_t e = scope.err;
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(r, r_host, bytes, hipMemcpyHostToDevice, g_stream);
        if (e != hipSuccess) return fail("precond_apply: setup failed: %s", hipGetErrorString(e));
        if (precond_apply_launch(P, r, z, g_stream)) return -1;
        e = hipStreamSynchronize(g_stream);
        if (e == hipSuccess && bytes) e = hipMemcpy(z_host, z, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail("precond_apply: run failed: %s", hipGetErrorString(e));
        return 0;
    });
}

// L (which = SPMV_FACTOR_L) or U of a kind that has factors, as the family's table returns them.  Call with
// col = val = NULL for row_ptr alone (row_ptr[rows] = the entries to allocate), then with all three.
extern "C" int spmv_hip_precond_factors(const spmv_precond *P, int which, int *row_ptr, int *col, void *val) {
    if (need_device()) return -1;
    if (!P || !row_ptr || (!col) != (!val)) return fail("precond_factors: bad arguments");
    if (!P->family || !P->family->factors) return fail("precond_factors: kind %d has no factors", P->kind);
    if (which != SPMV_FACTOR_L && which != SPMV_FACTOR_U) return fail("precond_factors: which = %d", which);
    return guarded("precond_factors", [&] { return P->family->factors(P, which, row_ptr, col, val); });
}
