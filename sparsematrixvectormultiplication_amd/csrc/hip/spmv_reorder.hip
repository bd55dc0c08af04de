// spmv_reorder.hip -- spmv_hip_csr_permute: C = P A Q^T of a whole CSR handle as a new handle, and spmv_hip_csr_rcm: the
// reverse Cuthill-McKee ordering of include/spmv_hip.h, both built on the device (reorder_kernels.hpp has the kernels;
// algebra_ops.hpp the frame).
//
// permute
//   check      ro_first_position + ro_repeats over each permutation: the first position whose value is out of range or
//              repeats an earlier position, one word to the host.  What the first kernel leaves is the inverse
//   lengths    ro_row_lengths; 4 bytes per row to the host, which makes row_ptr of them (as the sum does)
//   rows       ro_copy_rows: a lane group per row, sized by the mean row
//   adopt      csr_adopt_*: C is an ordinary handle with upload's plans
//
// rcm
//   graph      the pattern of A + A^T by transpose_core and spadd_core on views (no handle, no adopt; the values are not
//              looked at); degrees; ONE sort of all nodes by (deg, index): a node's rank in it stands for (deg, index) in
//              every later key, the sorted list gives the start nodes, and its head the isolated nodes
//   search     (peripheral passes) levels by rcm_chain<false> while they hold at most `cap` nodes, by rcm_expand<false>
//              otherwise: no sort, only the depth and the last level's smallest node
//   order      per level: rcm_chain<true> while frontier and next frontier hold at most `cap` nodes, else rcm_expand<true>
//              (atomicMin of the parent's place), rcm_keys, one radix sort of (parent, rank) on the bits in use, rcm_place;
//              four bytes per wide level cross to the host: the next frontier's size
//
// The exactness rests on one fact: inside one search the next level, in the order the serial queue appends it, is the
// set of unvisited neighbours of the frontier sorted by (place of the earliest frontier parent, deg, index).
#include "algebra_ops.hpp"

#include <rocprim/rocprim.hpp>

#include "reorder_kernels.hpp"

namespace {

thread_local double g_permute_ms[2] = {0, 0};  // device build, adopt of the last spmv_hip_csr_permute on this thread

int log2_of(int pow2) {
    int k = 0;
    while ((1 << k) < pow2) ++k;
    return k;
}
unsigned grid_for(long long threads, int cap = 0x7fffffff) {
    return (unsigned)std::max<long long>(1, std::min<long long>(cap, (threads + kBlock - 1) / kBlock));
}
int lanes_log2_for(long long entries, long long rows) {
    return log2_of(std::min(64, pow2_floor((int)std::min<long long>(64, std::max<long long>(1, rows ? entries / rows : 1)))));
}

// One permutation to the device, checked.  d_first: first[v] = the position of v (the inverse).  name: "row_perm" / "col_perm"
int checked_perm(const char *name, int n, const int *perm, DevBuf &d_perm, DevBuf &d_first, DevBuf &d_bad) {
    hipError_t e = d_perm.alloc((size_t)n * sizeof(int));
    if (e == hipSuccess) e = d_first.alloc((size_t)n * sizeof(int));
    if (e != hipSuccess) return fail("csr_permute: allocation of %s (%d entries) failed: %s", name, n, hipGetErrorString(e));
    unsigned bad = 0xffffffffu;
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_perm.p, perm, (size_t)n * sizeof(int), hipMemcpyHostToDevice, g_stream));
        HIP_TRY(hipMemsetAsync(d_first.p, 0xff, (size_t)n * sizeof(int), g_stream));
        HIP_TRY(hipMemsetAsync(d_bad.p, 0xff, sizeof(unsigned), g_stream));
        hipLaunchKernelGGL(ro_first_position, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, d_perm.as<int>(),
                           d_first.as<unsigned>(), d_bad.as<unsigned>());
        hipLaunchKernelGGL(ro_repeats, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, d_perm.as<int>(), d_first.as<unsigned>(),
                           d_bad.as<unsigned>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
    }
    if (bad != 0xffffffffu) {
        const int v = perm[bad];
        if (v < 0 || v >= n)
            return fail("csr_permute: %s[%u] = %d is outside [0, %d): not a permutation", name, bad, v, n);
        return fail("csr_permute: %s[%u] = %d repeats an earlier position: not a permutation", name, bad, v);
    }
    return 0;
}

template <typename T>
int permute_body(const spmv_csr_dev *m, const int *row_perm, const int *col_perm, spmv_csr_dev **out) {
    const CsrView A = csr_view(m);
    const int M = A.rows, N = A.cols;
    ClearHipError clear;
    UploadTrace trace("csr_permute");
    double split[2] = {0, 0};
    algebra::PhaseTimer timer{split};
    DevBuf d_bad, d_rows, d_rows_first, d_cols, d_cols_first, d_cnt;
    DevCsr C(M, N);
    hipError_t e = d_bad.alloc(sizeof(unsigned));
    if (e != hipSuccess) return fail("csr_permute: allocation failed: %s", hipGetErrorString(e));
    if (row_perm && checked_perm("row_perm", M, row_perm, d_rows, d_rows_first, d_bad)) return -1;
    if (col_perm && checked_perm("col_perm", N, col_perm, d_cols, d_cols_first, d_bad)) return -1;
    trace.mark("check");

    std::vector<int> cnt((size_t)M, 0), rp;
    e = d_cnt.alloc((size_t)M * sizeof(int));
    if (e == hipSuccess) e = C.alloc_rp();
    if (e == hipSuccess) e = C.alloc_entries<T>(A.nz, kPad, g_stream);
    if (e != hipSuccess) return fail("csr_permute: allocation of C (%d rows, %lld entries) failed: %s", M, A.nz, hipGetErrorString(e));
    const int *d_row_perm = row_perm ? d_rows.as<int>() : nullptr;
    if (M) {
        hipLaunchKernelGGL(ro_row_lengths, dim3(grid_for(M)), dim3(kBlock), 0, g_stream, M, d_row_perm, A.rp, d_cnt.as<int>());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail("csr_permute: row lengths failed: %s", hipGetErrorString(e));
    }
    RowCounts counts;
    if (algebra::row_ptr_of_counts("csr_permute", cnt, rp, counts)) return -1;
    e = hipMemcpyAsync(C.rp, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess && M && A.nz) {
        const int lanes_log2 = lanes_log2_for(A.nz, M);
        hipLaunchKernelGGL((ro_copy_rows<T>), dim3(grid_for((long long)M << lanes_log2, kRoMaxGrid)), dim3(kBlock), 0, g_stream, M,
                           lanes_log2, d_row_perm, col_perm ? d_cols_first.as<int>() : nullptr, A.rp, A.col,
                           static_cast<const T *>(A.val), C.rp, C.col, static_cast<T *>(C.val));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) return fail("csr_permute: build failed: %s", hipGetErrorString(e));
    timer.lap(0);
    trace.mark("device build");
    const int rc = algebra::adopt<T>(std::move(C), rp, out);
    timer.lap(1);
    if (rc == 0) std::copy(split, split + 2, g_permute_ms);
    return rc;
}

// ------------------------------------------------------------------ rcm
struct RcmRun {
    int n = 0, cap = 0, lanes_log2 = 0;
    unsigned rank_bits = 1;
    const int *rp = nullptr, *col = nullptr;  // G
    int *deg, *rank, *by_key, *pos, *parent, *mark, *seq, *list[2], *words;  // words: state[kRcmStateWords], then scratch
    unsigned long long *key_in, *key_out;
    DevBuf sort_tmp;
    size_t sort_tmp_bytes = 0;
    int stamp = 0;
    long long launches = 0, chained = 0, wide = 0, levels = 0, searches = 0;

    int *scratch() const { return words + kRcmStateWords; }  // two words: a counter, a minimum

    int sort(int count, unsigned bits) {
        size_t bytes = 0;
        hipError_t e = rocprim::radix_sort_keys(nullptr, bytes, key_in, key_out, (size_t)count, 0u, bits, g_stream);
        if (e == hipSuccess && bytes > sort_tmp_bytes) {
            HIP_TRY(hipStreamSynchronize(g_stream));
            (void)hipFree(sort_tmp.p);
            sort_tmp.p = nullptr;
            e = sort_tmp.alloc(bytes);
            sort_tmp_bytes = e == hipSuccess ? bytes : 0;
        }
        if (e == hipSuccess) e = rocprim::radix_sort_keys(sort_tmp.p, bytes, key_in, key_out, (size_t)count, 0u, bits, g_stream);
        if (e != hipSuccess) return fail("csr_rcm: sort of %d keys failed: %s", count, hipGetErrorString(e));
        ++launches;
        return 0;
    }
    // stamps only grow; before they could wrap, mark[] starts over (a chain may use one per node)
    int stamps_left() {
        if (stamp < 0x7fffffff - n - 8) return 0;
        HIP_TRY(hipMemsetAsync(mark, 0, (size_t)n * sizeof(int), g_stream));
        stamp = 0;
        return 0;
    }
    int read_words(int *host, int first, int count) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, words + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    }
    unsigned expand_grid(int count) const { return grid_for((long long)count << lanes_log2, 1 << 16); }

    // a breadth-first search from s over the unvisited nodes: its levels and the smallest node of the last one
    int search(int s, int &depth, int &smallest) {
        if (stamps_left()) return -1;
        ++stamp, ++searches;
        hipLaunchKernelGGL((rcm_seed<false>), dim3(1), dim3(64), 0, g_stream, s, 0, stamp, seq, pos, mark, list[0]);
        ++launches;
        int which = 0, count = 1, st[kRcmStateWords];
        depth = 1;
        for (;;) {
            if (cap && count <= cap) {
                hipLaunchKernelGGL((rcm_chain<false>), dim3(1), dim3(kRcmChainBlock), 0, g_stream, cap, lanes_log2, stamp, rank_bits, 0, count, depth,
                                   which, rp, col, rank, by_key, seq, pos, parent, mark, list[0], list[1], words);
                ++launches;
                if (read_words(st, 0, kRcmStateWords)) return -1;
                depth = st[kRcmLevels], which = st[kRcmWhich], count = st[kRcmCount];
                if (st[kRcmStatus] == kRcmDone) {
                    smallest = st[kRcmSmallest];
                    return 0;
                }
            }
            HIP_TRY(hipMemsetAsync(scratch(), 0, sizeof(int), g_stream));
            hipLaunchKernelGGL((rcm_expand<false>), dim3(expand_grid(count)), dim3(kBlock), 0, g_stream, count, lanes_log2,
                               list[which], 0, stamp, rp, col, pos, parent, mark, list[which ^ 1], scratch());
            ++launches;
            int found = 0;
            if (read_words(&found, kRcmStateWords, 1)) return -1;
            if (!found) break;
            which ^= 1, count = found, ++depth;
        }
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(scratch() + 1), kRcmUnvisited, 1, g_stream));
        hipLaunchKernelGGL(rcm_min_rank, dim3(grid_for(count)), dim3(kBlock), 0, g_stream, count, list[which], rank, scratch() + 1);
        ++launches;
        int r = 0;
        if (read_words(&r, kRcmStateWords + 1, 1)) return -1;
        HIP_TRY(hipMemcpyAsync(&smallest, by_key + r, sizeof(int), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        return 0;
    }

    // the Cuthill-McKee levels of s's component; s takes place `filled`, which ends as the place behind the component
    int order(int s, int &filled) {
        hipLaunchKernelGGL((rcm_seed<true>), dim3(1), dim3(64), 0, g_stream, s, filled, 0, seq, pos, mark, list[0]);
        ++launches;
        int f0 = filled, f1 = filled + 1, st[kRcmStateWords];
        for (;;) {
            if (stamps_left()) return -1;
            if (cap && f1 - f0 <= cap) {
                hipLaunchKernelGGL((rcm_chain<true>), dim3(1), dim3(kRcmChainBlock), 0, g_stream, cap, lanes_log2, stamp + 1, rank_bits, f0, f1, 0, 0, rp,
                                   col, rank, by_key, seq, pos, parent, mark, list[0], list[1], words);
                ++launches;
                if (read_words(st, 0, kRcmStateWords)) return -1;
                stamp += st[kRcmLevels] + 1;  // (one more: the level it gave up on claimed with its own)
                chained += st[kRcmLevels], levels += st[kRcmLevels];
                f0 = st[kRcmF0], f1 = st[kRcmF1];
                if (st[kRcmStatus] == kRcmDone) break;
            }
            const int count = f1 - f0;
            ++stamp;
            HIP_TRY(hipMemsetAsync(scratch(), 0, sizeof(int), g_stream));
            hipLaunchKernelGGL((rcm_expand<true>), dim3(expand_grid(count)), dim3(kBlock), 0, g_stream, count, lanes_log2, seq + f0, f0,
                               stamp, rp, col, pos, parent, mark, list[0], scratch());
            ++launches, ++levels, ++wide;
            int found = 0;
            if (read_words(&found, kRcmStateWords, 1)) return -1;  // the four bytes of a wide level
            if (!found) break;
            hipLaunchKernelGGL(rcm_keys, dim3(grid_for(found)), dim3(kBlock), 0, g_stream, found, f0, rank_bits, list[0], parent, rank,
                               key_in);
            ++launches;
            if (sort(found, rank_bits + algebra::bits_for((unsigned long long)count))) return -1;
            hipLaunchKernelGGL(rcm_place, dim3(grid_for(found)), dim3(kBlock), 0, g_stream, found, f1, rank_bits, key_out, by_key, seq,
                               pos);
            ++launches;
            f0 = f1, f1 += found;
        }
        filled = f1;
        return 0;
    }
};

int rcm_body(const spmv_csr_dev *m, int peripheral, int cap, int *perm, long long *stats, double *ms) {
    const CsrView A = csr_view(m);
    const int n = A.rows;
    long long st[SPMV_RCM_STATS] = {0};
    double split[3] = {0, 0, 0};
    auto finish = [&] {
        if (stats) std::copy(st, st + SPMV_RCM_STATS, stats);
        if (ms) std::copy(split, split + 3, ms);
        return 0;
    };
    if (!n) return finish();
    ClearHipError clear;
    UploadTrace trace("csr_rcm");
    double t_mark = UploadTrace::now();
    auto lap = [&](int k) {
        const double t = UploadTrace::now();
        split[k] += (t - t_mark) * 1e3;
        t_mark = t;
    };

    // ---- graph
    DevCsr G;
    {
        DevCsr At;
        std::vector<int> rp_host;
        if (transpose_core(m->value_bytes, A, At, rp_host)) return -1;
        const CsrView vt = At.view();
        if (spadd_core(m->value_bytes, &A, 1.0, &vt, 1.0, 0, 0, 0, G, rp_host, nullptr, nullptr)) return -1;
    }
    trace.mark("pattern of A + A^T");
    RcmRun R;
    R.n = n, R.cap = cap, R.rp = G.rp, R.col = G.col;
    R.rank_bits = algebra::bits_for((unsigned long long)n);
    R.lanes_log2 = lanes_log2_for(G.nz, n);
    DevBuf d_ints, d_keys;
    hipError_t e = d_ints.alloc(((size_t)n * 9 + kRcmStateWords + 8) * sizeof(int));
    if (e == hipSuccess) e = d_keys.alloc((size_t)n * 2 * sizeof(unsigned long long));
    if (e != hipSuccess) return fail("csr_rcm: allocation of the workspace of %d nodes failed: %s", n, hipGetErrorString(e));
    {
        int *p = d_ints.as<int>();
        for (int **a : {&R.deg, &R.rank, &R.by_key, &R.pos, &R.parent, &R.mark, &R.seq, &R.list[0], &R.list[1]}) *a = p, p += n;
        R.words = p;
        R.key_in = d_keys.as<unsigned long long>(), R.key_out = R.key_in + n;
    }
    int *d_n_iso = R.scratch(), *d_band = R.scratch() + 2;  // (band: two words, before and after)
    HIP_TRY(hipMemsetAsync(R.words, 0, (kRcmStateWords + 8) * sizeof(int), g_stream));
    HIP_TRY(hipMemsetAsync(R.mark, 0, (size_t)n * sizeof(int), g_stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)R.pos, kRcmUnvisited, (size_t)n, g_stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)R.parent, kRcmUnvisited, (size_t)n, g_stream));
    hipLaunchKernelGGL(rcm_degrees, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, R.rp, R.col, R.deg, R.key_in);
    if (R.sort(n, 32 + R.rank_bits)) return -1;  // (a degree is below n)
    hipLaunchKernelGGL(rcm_ranks, dim3(grid_for(n)), dim3(kBlock), 0, g_stream, n, R.key_out, R.by_key, R.rank, d_n_iso);
    hipLaunchKernelGGL(rcm_bandwidth, dim3(grid_for((long long)n * 64, 1 << 16)), dim3(kBlock), 0, g_stream, n, A.rp, A.col,
                       (const int *)nullptr, d_band);
    int n_iso = 0;
    if (R.read_words(&n_iso, kRcmStateWords, 1)) return -1;
    if (n_iso)
        hipLaunchKernelGGL(rcm_isolated, dim3(grid_for(n_iso)), dim3(kBlock), 0, g_stream, n_iso, R.by_key, R.seq, R.pos);
    R.launches = 0;  // (the launches of the searches and the levels are what info reports)
    lap(0);
    trace.mark("degrees and ranks");

    // ---- components: start nodes from the cursor over by_key
    int filled = n_iso, cursor = n_iso;
    long long components = n_iso;
    while (filled < n) {
        hipLaunchKernelGGL(rcm_next_start, dim3(1), dim3(kBlock), 0, g_stream, n, cursor, R.by_key, R.pos, R.scratch());
        ++R.launches;
        int start[2];
        if (R.read_words(start, kRcmStateWords, 2)) return -1;
        if (start[0] >= n) return fail("csr_rcm: internal error: %d of %d nodes placed and no start node left", filled, n);
        cursor = start[0] + 1;
        int s = start[1];
        ++components;
        lap(2);
        if (peripheral > 0) {
            int depth_s = 0, t = 0, depth_t = 0, t2 = 0;
            if (R.search(s, depth_s, t)) return -1;
            for (int pass = 0; pass < peripheral; ++pass) {
                if (R.search(t, depth_t, t2)) return -1;
                if (depth_t <= depth_s) break;
                s = t, depth_s = depth_t, t = t2;
            }
            lap(1);
        }
        if (R.order(s, filled)) return -1;
        lap(2);
    }
    trace.mark("searches and levels");

    // ---- the result: perm[i] = seq[n - 1 - i]; |inv[i] - inv[j]| = |pos[i] - pos[j]|
    hipLaunchKernelGGL(rcm_bandwidth, dim3(grid_for((long long)n * 64, 1 << 16)), dim3(kBlock), 0, g_stream, n, A.rp, A.col,
                       (const int *)R.pos, d_band + 1);
    int band[2] = {0, 0};
    if (R.read_words(band, kRcmStateWords + 2, 2)) return -1;
    std::vector<int> seq((size_t)n);
    HIP_TRY(hipMemcpy(seq.data(), R.seq, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) perm[i] = seq[(size_t)n - 1 - i];
    lap(2);
    const long long s[SPMV_RCM_STATS] = {components, n_iso, R.levels, R.chained, R.wide, R.launches, R.searches, band[0], band[1]};
    std::copy(s, s + SPMV_RCM_STATS, st);
    return finish();
}

}  // namespace

extern "C" int spmv_hip_csr_permute(const spmv_csr_dev *m, const int *row_perm, const int *col_perm, spmv_csr_dev **out) {
    if (need_device()) return -1;
    if (!out) return fail("csr_permute: out is NULL");
    *out = nullptr;
    if (!m) return fail("csr_permute: NULL handle");
    if (algebra::operand_ok("csr_permute", nullptr, "permute", m)) return -1;
    return guarded("csr_permute", [&] {
        return m->value_bytes == 8 ? permute_body<double>(m, row_perm, col_perm, out)
                                   : permute_body<float>(m, row_perm, col_perm, out);
    });
}

extern "C" int spmv_hip_csr_permute_ms(double *ms) {
    if (!ms) return fail("csr_permute_ms: ms is NULL");
    std::copy(g_permute_ms, g_permute_ms + 2, ms);
    return 0;
}

extern "C" int spmv_hip_rcm_chain_nodes(int *smallest, int *largest, int *automatic) {
    if (smallest) *smallest = kRcmChainMin;
    if (largest) *largest = kRcmChainMax;
    if (automatic) *automatic = kRcmChainAuto;
    return 0;
}

extern "C" int spmv_hip_csr_rcm(const spmv_csr_dev *m, int peripheral, int chain_nodes, int *perm, long long *stats, double *ms) {
    if (need_device()) return -1;
    if (!m) return fail("csr_rcm: NULL handle");
    if (algebra::operand_ok("csr_rcm", nullptr, "are reordered", m)) return -1;
    if (m->M_total != m->N) return fail("csr_rcm: the matrix is %d x %d; only square matrices are reordered", m->M_total, m->N);
    if (!perm && m->M_total) return fail("csr_rcm: perm is NULL");
    if (peripheral < 0 || peripheral > SPMV_RCM_MAX_PERIPHERAL)
        return fail("csr_rcm: peripheral = %d; the passes lie in [0, %d]", peripheral, SPMV_RCM_MAX_PERIPHERAL);
    const bool pow2 = chain_nodes > 0 && (chain_nodes & (chain_nodes - 1)) == 0;
    if (chain_nodes != 0 && chain_nodes != -1 && !(pow2 && chain_nodes >= kRcmChainMin && chain_nodes <= kRcmChainMax))
        return fail("csr_rcm: chain_nodes = %d; 0 (auto), -1 (never chain) or a power of two in [%d, %d]", chain_nodes, kRcmChainMin,
                    kRcmChainMax);
    const int cap = chain_nodes == 0 ? kRcmChainAuto : chain_nodes == -1 ? 0 : chain_nodes;
    return guarded("csr_rcm", [&] { return rcm_body(m, peripheral, cap, perm, stats, ms); });
}
