// spmv_spgemm.hip -- spmv_hip_csr_spgemm: C = A B of two whole CSR handles as a new handle, built on the device
// (include/spmv_hip.h has the definition; spgemm_kernels.hpp the kernels).
//
//   count      sg_count: the products of every row of A, 8 bytes per row to the host
//   plan       spmv_spgemm_plan (host/spgemm_plan.c): row blocks of at most block_products products for the on-chip tier,
//              long rows for the global tier, dealt into chunks of whole rows of at most chunk_products products
//   symbolic   sg_block<T, false> over the blocks; per chunk sg_expand<T, false>, a radix sort of the keys and
//              sg_row_heads: the entries of every row of C, 4 bytes per row to the host, which makes row_ptr of them
//   numeric    col / val of C at their exact size; sg_block<T, true>; per chunk sg_expand<T, true>, one stable
//              radix_sort_pairs on the bits in use and sg_row_compress
//   adopt      csr_adopt_*: C is an ordinary handle with upload's plans
//
// Everything in front of the adopt is spgemm_core, on views of bare device arrays (algebra_ops.hpp has the frame): the AMG
// device setup (spmv_amg_setup.hip) forms its products with it and keeps the arrays, the sum (spmv_spadd.hip) makes an
// operand canonical with it.
//
// The workspace is the per-row counts, the block list and one chunk's keys and products (twice: the sort's output).
#include "algebra_ops.hpp"

#include <rocprim/rocprim.hpp>

#include "spgemm_kernels.hpp"

namespace {

constexpr int kSgMaxGrid = 1 << 16;            // grid cap (blocks and rows stride over the workgroups beyond it)
constexpr long long kSgAutoChunk = 1LL << 23;  // products of a chunk (auto): 32 bytes of workspace each

// the on-chip kernels ask for up to 64 KiB of dynamic LDS beside their static scratch: HIP wants that allowed per kernel
template <typename T>
int sg_allow_lds() {
    static int done_for_device = -1;
    if (done_for_device == g_device) return 0;
    for (const void *fn : {(const void *)sg_block<T, false>, (const void *)sg_block<T, true>})
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    done_for_device = g_device;
    return 0;
}

using algebra::bits_for;

struct Chunk {
    int first = 0, rows = 0;  // in the list of long rows
    long long products = 0;
};

// the product on bare arrays: everything but the adopt
template <typename T>
int spgemm_core_t(const CsrView &A, const CsrView &B, int block_products, long long chunk_products, DevCsr &C_out,
                  std::vector<int> &rp, long long *stats, double *ms) {
    const CsrView *a = &A, *b = &B;
    const int M = a->rows, N = b->cols;
    const int cap = block_products == 0 ? kSgMaxProducts : block_products;  // -1: no on-chip tier
    const long long chunk_cap = chunk_products ? chunk_products : kSgAutoChunk;
    const T *valA = static_cast<const T *>(a->val), *valB = static_cast<const T *>(b->val);
    UploadTrace trace("csr_spgemm");
    double split[3] = {0, 0, 0};
    algebra::PhaseTimer timer{split};
    ClearHipError clear;
    DevCsr C(M, N);
    if (sg_allow_lds<T>()) return -1;

    // ---- count
    std::vector<long long> products((size_t)M, 0);
    DevBuf d_products, d_cnt;
    hipError_t e = d_products.alloc((size_t)M * sizeof(long long));
    if (e == hipSuccess) e = d_cnt.alloc((size_t)M * sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt.p, 0, std::max<size_t>((size_t)M * sizeof(int), 16), g_stream);
    if (e != hipSuccess) return fail("csr_spgemm: allocation of the counts of %d rows failed: %s", M, hipGetErrorString(e));
    if (M) {
        constexpr int kRows = kBlock / kSgCountLanes;
        const int grid = (int)std::min<long long>(kSgMaxGrid, ((long long)M + kRows - 1) / kRows);
        hipLaunchKernelGGL(sg_count, dim3(grid), dim3(kBlock), 0, g_stream, M, a->rp, a->col, b->rp,
                           d_products.as<long long>());
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(products.data(), d_products.p, (size_t)M * sizeof(long long), hipMemcpyDeviceToHost, g_stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_spgemm: count failed: %s", hipGetErrorString(e));
    timer.lap(0);
    trace.mark("count");

    // ---- plan
    std::vector<int> block_row((size_t)M + 1, 0), long_row((size_t)std::max(M, 1), 0);
    int n_blocks = 0, n_long = 0;
    if (spmv_spgemm_plan(M, products.data(), block_products, kSgMaxRows, block_row.data(), &n_blocks, long_row.data(), &n_long))
        return fail("csr_spgemm: the plan refused block_products = %d", block_products);
    const long long long_from = cap < 0 ? 0 : cap;  // a row is long when it has more products than this
    long long total = 0, widest = 0, block_rows = 0;
    for (int i = 0; i < M; ++i) total += products[i], widest = std::max(widest, products[i]);
    std::vector<int4> desc;
    for (int k = 0; k < n_blocks; ++k) {
        const int r0 = block_row[k], r1 = block_row[k + 1];
        const int nrows = r1 - r0 - (products[r1 - 1] > long_from ? 1 : 0);
        long long P = 0;
        for (int r = r0; r < r0 + nrows; ++r) P += products[r];
        if (P > 0) desc.push_back(make_int4(r0, nrows, (int)P, 0)), block_rows += nrows;
    }
    std::vector<Chunk> chunks;
    std::vector<long long> off;  // chunk c's offsets: off[first + c .. first + c + rows]
    for (int k = 0; k < n_long; ++k) {
        const long long p = products[long_row[k]];
        if (chunks.empty() || chunks.back().products + p > chunk_cap) {
            if (!chunks.empty()) off.push_back(chunks.back().products);
            chunks.push_back({k, 0, 0});
        }
        off.push_back(chunks.back().products);
        chunks.back().rows += 1;
        chunks.back().products += p;
    }
    if (!chunks.empty()) off.push_back(chunks.back().products);
    long long chunk_max = 0;
    for (const Chunk &c : chunks) chunk_max = std::max(chunk_max, c.products);

    // ---- workspace
    DevBuf d_desc, d_lrows, d_off, d_kin, d_kout, d_vin, d_vout, d_tmp;
    const unsigned col_bits = bits_for((unsigned long long)N);
    size_t tmp_bytes = 0;
    e = d_desc.alloc(desc.size() * sizeof(int4));
    if (e == hipSuccess) e = d_lrows.alloc((size_t)n_long * sizeof(int));
    if (e == hipSuccess) e = d_off.alloc(off.size() * sizeof(long long));
    if (e == hipSuccess) e = C.alloc_rp();
    if (e == hipSuccess && chunk_max) {
        e = d_kin.alloc((size_t)chunk_max * 8);
        if (e == hipSuccess) e = d_kout.alloc((size_t)chunk_max * 8);
        if (e == hipSuccess) e = d_vin.alloc((size_t)chunk_max * 8);
        if (e == hipSuccess) e = d_vout.alloc((size_t)chunk_max * 8);
        if (e == hipSuccess)  // (the pairs sort needs no less than the keys sort)
            e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_kin.as<unsigned long long>(), d_kout.as<unsigned long long>(),
                                          d_vin.as<double>(), d_vout.as<double>(), (size_t)chunk_max, 0u, 64u, g_stream);
        if (e == hipSuccess) e = d_tmp.alloc(tmp_bytes);
    }
    if (e != hipSuccess)
        return fail("csr_spgemm: allocation of the workspace failed (%zu blocks, %d long rows, chunks of up to %lld products): %s",
                    desc.size(), n_long, chunk_max, hipGetErrorString(e));
    if (!desc.empty()) e = hipMemcpyAsync(d_desc.p, desc.data(), desc.size() * sizeof(int4), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && n_long) {
        e = hipMemcpyAsync(d_lrows.p, long_row.data(), (size_t)n_long * sizeof(int), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, g_stream);
    }
    if (e != hipSuccess) return fail("csr_spgemm: upload of the plan failed: %s", hipGetErrorString(e));

    int *d_colC = nullptr;  // (C's, once the symbolic pass has counted them)
    T *d_valC = nullptr;
    const int bgrid = (int)std::min<size_t>(kSgMaxGrid, desc.size());
    auto run_blocks = [&](bool numeric) {
        if (desc.empty()) return;
        if (numeric)
            hipLaunchKernelGGL((sg_block<T, true>), dim3(bgrid), dim3(kBlock), (size_t)cap * 16, g_stream, (int)desc.size(), cap,
                               d_desc.as<int4>(), a->rp, a->col, valA, b->rp, b->col, valB, d_products.as<long long>(),
                               d_cnt.as<int>(), C.rp, d_colC, d_valC);
        else
            hipLaunchKernelGGL((sg_block<T, false>), dim3(bgrid), dim3(kBlock), (size_t)cap * 12, g_stream, (int)desc.size(), cap,
                               d_desc.as<int4>(), a->rp, a->col, valA, b->rp, b->col, valB, d_products.as<long long>(),
                               d_cnt.as<int>(), C.rp, d_colC, d_valC);
    };
    auto run_chunks = [&](bool numeric) -> hipError_t {
        for (size_t c = 0; c < chunks.size(); ++c) {
            const Chunk &ch = chunks[c];
            const int *rows = d_lrows.as<int>() + ch.first;
            const long long *o = d_off.as<long long>() + ch.first + c;
            const int grid = std::min(kSgMaxGrid, ch.rows);
            const unsigned bits = col_bits + (ch.rows > 1 ? bits_for((unsigned long long)ch.rows) : 0);
            unsigned long long *kin = d_kin.as<unsigned long long>(), *kout = d_kout.as<unsigned long long>();
            hipError_t err;
            if (numeric) {
                hipLaunchKernelGGL((sg_expand<T, true>), dim3(grid), dim3(kBlock), 0, g_stream, ch.rows, rows, o, (int)col_bits,
                                   a->rp, a->col, valA, b->rp, b->col, valB, kin, d_vin.as<double>());
                size_t bytes = tmp_bytes;
                err = rocprim::radix_sort_pairs(d_tmp.p, bytes, kin, kout, d_vin.as<double>(), d_vout.as<double>(),
                                                (size_t)ch.products, 0u, bits, g_stream);
                if (err != hipSuccess) return err;
                hipLaunchKernelGGL((sg_row_compress<T>), dim3(grid), dim3(kBlock), 0, g_stream, ch.rows, rows, o,
                                   (1ull << col_bits) - 1, kout, d_vout.as<double>(), C.rp, d_colC, d_valC);
            } else {
                hipLaunchKernelGGL((sg_expand<T, false>), dim3(grid), dim3(kBlock), 0, g_stream, ch.rows, rows, o, (int)col_bits,
                                   a->rp, a->col, valA, b->rp, b->col, valB, kin, (double *)nullptr);
                size_t bytes = tmp_bytes;
                err = rocprim::radix_sort_keys(d_tmp.p, bytes, kin, kout, (size_t)ch.products, 0u, bits, g_stream);
                if (err != hipSuccess) return err;
                hipLaunchKernelGGL(sg_row_heads, dim3(grid), dim3(kBlock), 0, g_stream, ch.rows, rows, o, kout, d_cnt.as<int>());
            }
        }
        return hipGetLastError();
    };

    // ---- symbolic
    std::vector<int> cnt((size_t)M, 0);
    run_blocks(false);
    e = run_chunks(false);
    if (e == hipSuccess && M)
        e = hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_spgemm: symbolic pass failed: %s", hipGetErrorString(e));
    RowCounts counts;
    if (algebra::row_ptr_of_counts("csr_spgemm", cnt, rp, counts)) return -1;
    const long long nz = counts.nz;
    timer.lap(1);
    trace.mark("symbolic");

    // ---- numeric
    e = C.alloc_entries<T>(nz, kPad, g_stream);
    if (e != hipSuccess) return fail("csr_spgemm: allocation of C's %lld entries failed: %s", nz, hipGetErrorString(e));
    d_colC = C.col, d_valC = static_cast<T *>(C.val);
    e = hipMemcpyAsync(C.rp, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess) {
        run_blocks(true);
        e = run_chunks(true);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_spgemm: numeric pass failed: %s", hipGetErrorString(e));
    timer.lap(2);
    trace.mark("numeric");
    C_out = std::move(C);
    if (stats) {
        const long long s[8] = {total, nz, (long long)desc.size(), block_rows, n_long, (long long)chunks.size(), widest, counts.widest};
        std::copy(s, s + 8, stats);
    }
    if (ms) std::copy(split, split + 3, ms);
    return 0;
}

// core, then the adopt: C is an ordinary handle with upload's plans
template <typename T>
int spgemm_body(const spmv_csr_dev *a, const spmv_csr_dev *b, int block_products, long long chunk_products,
                spmv_csr_dev **out, long long *stats, double *ms) {
    DevCsr C;
    std::vector<int> rp;
    double split[4] = {0, 0, 0, 0};
    if (spgemm_core_t<T>(csr_view(a), csr_view(b), block_products, chunk_products, C, rp, stats, split)) return -1;
    algebra::PhaseTimer timer{split};
    const int rc = algebra::adopt<T>(std::move(C), rp, out);
    C = DevCsr();  // (the free of what C still holds has always been part of this phase)
    timer.lap(3);
    if (rc) return rc;
    if (ms) std::copy(split, split + 4, ms);
    return 0;
}

}  // namespace

int spgemm_max_block_products() { return kSgMaxProducts; }

int spgemm_core(int value_bytes, const CsrView &A, const CsrView &B, int block_products, long long chunk_products, DevCsr &C,
                std::vector<int> &rp_host, long long *stats, double *ms) {
    return value_bytes == 8 ? spgemm_core_t<double>(A, B, block_products, chunk_products, C, rp_host, stats, ms)
                            : spgemm_core_t<float>(A, B, block_products, chunk_products, C, rp_host, stats, ms);
}

extern "C" int spmv_hip_csr_spgemm(const spmv_csr_dev *a, const spmv_csr_dev *b, int block_products, long long chunk_products,
                                   spmv_csr_dev **out, long long *stats, double *ms) {
    if (need_device()) return -1;
    if (!out) return fail("csr_spgemm: out is NULL");
    *out = nullptr;
    if (!a || !b) return fail("csr_spgemm: NULL handle (a = %p, b = %p)", (const void *)a, (const void *)b);
    if (algebra::operand_ok("csr_spgemm", "A", "multiply", a) || algebra::operand_ok("csr_spgemm", "B", "multiply", b)) return -1;
    if (a->N != b->M_total)
        return fail("csr_spgemm: A is %d x %d and B is %d x %d: A's columns must be B's rows", a->M_total, a->N, b->M_total, b->N);
    if (a->value_bytes != b->value_bytes)
        return fail("csr_spgemm: A holds %d-byte values and B %d-byte values; the dtypes must agree", a->value_bytes,
                    b->value_bytes);
    if (!spgemm_block_products_ok(block_products))
        return fail("csr_spgemm: block_products = %d; 0 (auto), -1 (no on-chip tier) or a power of two in [64, %d]",
                    block_products, kSgMaxProducts);
    if (chunk_products != 0 && chunk_products < 64)
        return fail("csr_spgemm: chunk_products = %lld; 0 (auto) or at least 64", chunk_products);
    if ((unsigned long long)b->N * (unsigned long long)b->value_bytes >= (1ull << 32))
        return fail("csr_spgemm: N = %d: C's x exceeds the 32-bit gather offset range of the kernels", b->N);
    return guarded("csr_spgemm", [&] {
        return a->value_bytes == 8 ? spgemm_body<double>(a, b, block_products, chunk_products, out, stats, ms)
                                   : spgemm_body<float>(a, b, block_products, chunk_products, out, stats, ms);
    });
}
