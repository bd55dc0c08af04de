// spmv_csr.hip -- CSR side of the C-ABI: upload-time preprocessing (workgroup blocks, the
// x-window plan, split long rows; the tile plans: tile_upload.hpp), kernel launchers, timing.  Replaces the device code of the
// reference's per-matrix CSR section (its main_cuda.cu, lines 135-145, 149-166, 212-238, 285-317
// and 682-685).
#include "spmv_internal.hpp"

#include "launch_dispatch.hpp"
#include "upload_ops.hpp"

#include "tile_upload.hpp"

// ----------------------------------------------------------- CSR: upload
namespace {

// Cut rows [0, M) (row_ptr rebased to 0) into workgroup-sized blocks for the
// stream kernels: desc = {first row, first entry, rows, end entry}, each block's entries
// (counted from the even entry at or below its first) fit `cap`.  A row that
// cannot be staged is cut into pieces {row, first entry, end entry, slot} whose
// partial sums csr_long_finish adds up per long row {row, first slot, pieces, 0}.
// `split` (optional, one byte per row) marks rows that go to the split-row kernels whatever their
// length: rows the x-window plan cannot take (more x lines than a block may list).
void csr_build_blocks(int M, const int *rp, int cap, int rows_cap, std::vector<int4> &desc,
                      std::vector<int4> &pieces, std::vector<int4> &long_rows,
                      const std::vector<unsigned char> *split = nullptr) {
    desc.clear();
    pieces.clear();
    long_rows.clear();
    auto is_long = [&](int row) { return rp[row + 1] - rp[row] > cap - 3 || (split && (*split)[row]); };
    int r = 0;
    while (r < M) {
        const int n0 = rp[r];
        const int base = n0 & kBaseMask;
        if (is_long(r)) {
            const int first_slot = (int)pieces.size();
            for (int p = n0; p < rp[r + 1]; p += kLongPiece)
                pieces.push_back(int4{r, p, std::min(p + kLongPiece, rp[r + 1]), (int)pieces.size()});
            long_rows.push_back(int4{r, first_slot, (int)pieces.size() - first_slot, 0});
            ++r;
            continue;
        }
        int r1 = r, maxlen = 0;
        while (r1 < M && r1 - r < rows_cap && rp[r1 + 1] - base <= cap && !is_long(r1) &&
               !skew_cut(r1 - r, maxlen, rp[r1 + 1] - rp[r1])) {
            maxlen = std::max(maxlen, rp[r1 + 1] - rp[r1]);
            ++r1;
        }
        desc.push_back(int4{r, n0, r1 - r, rp[r1]});
        r = r1;
    }
}

// The host builder of the x-window plan (LocalPlan, spmv_internal.hpp): csr_build_blocks' cut with the line limit on top
// (1 << line_shift elements per line).  Returns false when some row alone needs more than lines_max lines, or when the
// line limit (rather than cap) decides so many cuts that the blocks would run mostly empty: the caller then keeps the
// gather kernel.
bool csr_build_local(int M, int N, const int *rp, const int *col, long long nz, int cap, int rows_cap,
                     int line_shift, int lines_max, const std::vector<int4> &baseline, LocalPlan<int2> &plan) {
    const int total_lines = (int)(((long long)N + (1 << line_shift) - 1) >> line_shift);
    const int line_mask = (1 << line_shift) - 1;
    std::vector<int> stamp((size_t)total_lines + 1, -1), rank((size_t)total_lines + 1, 0), cur;
    plan.lcol.assign((size_t)nz + kPad, 0);
    plan.split.assign((size_t)M, 0);
    plan.desc.clear();
    plan.ldesc.clear();
    plan.lines.clear();
    int widest = 0;
    long long split_entries = 0;
    int r = 0;
    while (r < M) {
        const int n0 = rp[r];
        const int base = n0 & kBaseMask;
        if (rp[r + 1] - n0 > cap - 3) {  // long row: csr_long_pieces, as in csr_build_blocks
            ++r;
            continue;
        }
        const int blk = (int)plan.desc.size();
        cur.clear();
        int r1 = r, maxlen = 0;
        while (r1 < M && r1 - r < rows_cap && rp[r1 + 1] - base <= cap && rp[r1 + 1] - rp[r1] <= cap - 3 &&
               !skew_cut(r1 - r, maxlen, rp[r1 + 1] - rp[r1])) {
            const size_t before = cur.size();
            for (int e = rp[r1]; e < rp[r1 + 1]; ++e) {
                const int l = col[e] >> line_shift;
                if (stamp[l] != blk) {
                    stamp[l] = blk;
                    cur.push_back(l);
                }
            }
            if ((int)cur.size() > lines_max) {  // this row does not fit any more: take it back
                for (size_t k = before; k < cur.size(); ++k) stamp[cur[k]] = -1;
                cur.resize(before);
                break;
            }
            maxlen = std::max(maxlen, rp[r1 + 1] - rp[r1]);
            ++r1;
        }
        if (r1 == r) {
            // one row alone touches more lines than a block may list: it goes to the split-row
            // (gather) kernels like a long row; a matrix made of such rows keeps the gather kernel
            // ... and a SMALL matrix with such a row keeps it too: the split-row kernels are two more launches
            // (~5 us), more than the whole product of a matrix below ~1 M entries (adder_dcop_32-size stand-in:
            // 11.5 us with the plan + split rows against 6.3 us for one launch, profiles/r2_reference_list_stand_ins.md)
            if (nz < kSplitMinEntries) return false;
            plan.split[r] = 1;
            split_entries += rp[r + 1] - n0;
            if (split_entries * 20 > nz) return false;
            ++r;
            continue;
        }
        if (cur.empty()) cur.push_back(0);  // only empty rows: the kernel still stages one line
        std::sort(cur.begin(), cur.end());
        for (size_t k = 0; k < cur.size(); ++k) rank[cur[k]] = (int)k;
        for (int e = rp[r]; e < rp[r1]; ++e)
            plan.lcol[e] = (unsigned short)((rank[col[e] >> line_shift] << line_shift) | (col[e] & line_mask));
        plan.desc.push_back(int4{r, n0, r1 - r, rp[r1]});
        plan.ldesc.push_back(int2{(int)plan.lines.size(), (int)cur.size()});
        plan.lines.insert(plan.lines.end(), cur.begin(), cur.end());
        widest = std::max(widest, (int)cur.size());
        r = r1;
        // the line limit is cutting blocks well short of what cap alone allows: give up early
        if ((plan.desc.size() & 1023) == 0) {
            const size_t plain = std::lower_bound(baseline.begin(), baseline.end(), r,
                                                  [](const int4 &d, int row) { return d.x < row; }) -
                                 baseline.begin();
            if (plan.desc.size() > plain + plain / 5 + 16) return false;
        }
    }
    if (plan.desc.size() > baseline.size() + baseline.size() / 5 + 1) return false;
    // the kernel stages whole passes of kLocalLineQuantum lines and reads the list unconditionally
    plan.stage_lines = std::max(kLocalLineQuantum,
                                (widest + kLocalLineQuantum - 1) / kLocalLineQuantum * kLocalLineQuantum);
    plan.lines.insert(plan.lines.end(), (size_t)kLocalLinesMax, 0);
    return true;
}

// The x-window plan of the blocks `desc` (cut by entries and rows only) built on the device from the uploaded column
// indices (upload_ops.hpp).  1: the handle carries the plan; 0: some block lists more than kLocalLinesMax lines, the
// host builder (which may cut blocks by lines or split rows) has to decide; 2: so many blocks list so many lines that
// the host builder would refuse too; -1: HIP error.
template <int SHIFT>
int csr_plan_on_device(spmv_csr_dev *m, const std::vector<int4> &desc, long long nz) {
    const int W = (int)desc.size();
    std::vector<long long> begin((size_t)W);
    std::vector<int> len((size_t)W), nl;
    for (int w = 0; w < W; ++w) {
        begin[w] = desc[w].y;
        len[w] = desc[w].w - desc[w].y;
        if (len[w] > kPlanCap) return 0;
    }
    const int rc = plan_on_device<SHIFT>(m->xw, m->col, (size_t)nz, desc, begin, len,
                                         [](int, int first, int n) { return int2{first, n}; }, nl);
    if (rc != 0 || nl.empty()) return rc;
    // Some block lists too many lines.  The host builder may still find a plan (blocks cut by lines, a few rows split) --
    // unless the matrix is plainly scattered: a block with n lines needs at least n / 256 line-limited blocks, a
    // line-limited block can overlap two of ours, and the host refuses a plan with more than 1.2 x our block count.
    // 2 = refused here (the host builder would spend ~0.2 s at 2.6e8 entries to say the same).
    long long need = 0;
    for (int n : nl) need += std::max(1, (n + kLocalLinesMax - 1) / kLocalLinesMax);
    return (need + 1) / 2 > (long long)W + W / 5 + 1 ? 2 : 0;
}

// The pattern plan of a handle's x-window plan (csr_kernels.hpp, PAT; plan_kernels.hpp): built on the device from the
// plan's own arrays, whichever builder made them -- the tables (build_pattern_tables, upload_ops.hpp), then one segment
// per block out of them where it fits the LDS budget (csr_pattern_segments).  auto: kept when the tables hold at most a
// quarter of the slots.
// Where it pays (same handle, same placement, the two instantiations alternately: profiles/r3_ab_patterns.txt): the
// nlpkkt-like matrix 190 -> 178 us (bench.py over 4 uploads each; 204 -> 185 on a slow placement), a 27-point stencil
// 197 -> 190; neutral on the FEM-shaped matrix (75 per row: 155 / 157) and on nlpkkt80-size (59 / 60); a loss where the
// rows are short -- several rows per lane group, their patterns fetched pass after pass: 7-point 271 -> 285, 5-point
// 186 -> 210 --, in fp32 (124 -> 133: the same LDS work for half the bytes) and for matrices that live in the Infinity
// Cache (cant-size 10.8 -> 12.4).  The gain goes with the placement of the arrays: 1-2 % on a fast one, 9 % on a slow one.
// (nlpkkt80-size, 29 M entries: 56.3 -> 58.4.)  And even where it gains the gain goes with the placement of the arrays
// (27-point stencil: 204 -> 195 on one box, 177 -> 183 on another).  Hence auto: streamed matrices (the `nt` threshold)
// of at least 12 entries per row whose tables hold at most a quarter of the slots get a plan BUILT, and upload then
// times its own kernel with and without it and keeps the plan only if it is at least 2 % faster on this handle
// (tune_pattern_plan, beside the placement search).
// The widest segment (uint4s, at most one per lane) whose LDS copy keeps as many workgroups of csr_stream_local<.., PAT>
// resident per CU as its stage and slots alone would, up to the 7 its VGPRs allow.  LDS is counted in 512-byte granules
// (no finer than the hardware's), of the 160 KiB of a gfx950 CU.
constexpr size_t kLdsPerCu = 160 * 1024, kLdsGranule = 512;
constexpr int kLocalWgsPerCu = 7;
static int pattern_segment_cap(int value_bytes, int local_cap, int stage_lines) {
    const size_t stage = std::max((size_t)local_cap * (size_t)value_bytes, (size_t)stage_lines * kLineBytes);
    const size_t fixed = stage + ((size_t)local_cap + 8) * sizeof(unsigned short);
    auto per_cu = [](size_t bytes) { return kLdsPerCu / ((bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule); };
    const size_t want = std::min((size_t)kLocalWgsPerCu, per_cu(fixed));
    int cap = 0;
    while (cap < kBlock && per_cu(fixed + (size_t)(cap + 1) * sizeof(uint4)) >= want) ++cap;
    return cap;
}
int csr_pattern_segment_cap(const spmv_csr_dev *m) {
    const int cap = pattern_segment_cap(m->value_bytes, m->local_cap, m->xw.stage_lines);
    return g_local_segment_cap > 0 ? std::min(cap, g_local_segment_cap / (int)sizeof(uint4)) : cap;  // ("local_segment_cap")
}
extern "C" int spmv_hip_csr_pattern_segment_cap(int value_bytes, int local_cap, int stage_lines) {
    if ((value_bytes != 4 && value_bytes != 8) || local_cap <= 0 || local_cap > kStreamCapMax || stage_lines < 0 ||
        stage_lines > kLocalLinesMax)
        return fail("csr_pattern_segment_cap: bad arguments (%d, %d, %d)", value_bytes, local_cap, stage_lines);
    return 16 * pattern_segment_cap(value_bytes, local_cap, stage_lines);
}

// The segments of a pattern plan whose tables are built (count[b]: elements of block b's table).  The LDS budget of a
// segment: the kernel's stage and slots take stage + (cap + 8) * 2 bytes; the segment's copy may not cost a resident
// workgroup per CU (at most the 7 the kernel's VGPRs allow).  A block whose segment is wider keeps its table.  A
// failure drops the whole plan (and clears the last HIP error).
void csr_pattern_segments(spmv_csr_dev *m, const std::vector<int> &count) {
    PatternPlan &pat = m->xw.pat;
    if (!pat.ptab) return;
    UploadTrace trace("csr_pattern_segments");
    const int B = m->xw.blocks;
    const int cap16 = csr_pattern_segment_cap(m);
    std::vector<int4> h_desc((size_t)B);  // the blocks' row counts: the size of their segments
    hipError_t e = hipMemcpyAsync(h_desc.data(), m->xw.ldesc4, (size_t)B * sizeof(int4), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    std::vector<int2> h_sdesc((size_t)B, make_int2(0, 0));
    long long seg_total = 0, table_rows = 0, segments = 0;
    int seg_max = 0;
    for (int b = 0; b < B && e == hipSuccess; ++b) {
        const int4 d = h_desc[(size_t)b];
        const int len = seg_groups_at(d.z) + count[(size_t)b] / 8;
        if (len <= cap16) {
            h_sdesc[(size_t)b] = make_int2((int)seg_total, len);
            seg_total += len;
            seg_max = std::max(seg_max, len);
            ++segments;
        } else {
            table_rows += d.z;
        }
    }
    if (seg_max > 0 && seg_total <= 0x7fffffffLL) {
        e = hipMalloc((void **)&pat.pseg, (size_t)seg_total * sizeof(uint4));
        if (e == hipSuccess) e = hipMalloc((void **)&pat.sdesc, (size_t)B * sizeof(int2));
        if (e == hipSuccess) e = hipMemsetAsync(pat.pseg, 0, (size_t)seg_total * sizeof(uint4), g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(pat.sdesc, h_sdesc.data(), (size_t)B * sizeof(int2), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL((pat_segment<256>), dim3(B), dim3(256), 0, g_stream, B, m->xw.ldesc4, m->row_ptr, pat.rinfo,
                               pat.ptab, pat.pdesc, pat.sdesc, pat.pseg);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    } else {
        seg_total = 0;
        seg_max = 0;
        segments = 0;
        table_rows = m->M_local;
    }
    if (e != hipSuccess) {
        pat.release();
        (void)hipGetLastError();
        return;
    }
    pat.seg_total = seg_total;
    pat.seg_distinct = segments;
    pat.seg_max = seg_max;
    pat.seg_cap = cap16;
    pat.table_rows = table_rows;
    trace.mark("segments");
}

// Shared plans ("local_share"; share_spans, upload_ops.hpp).  The blocks of a stencil repeat with the period of (row start
// mod 16, position in the grid line): on the nlpkkt-like matrix 48 069 blocks hold 1 173 distinct segments and 361
// distinct line lists relative to their first line, and every block streamed its own copy from HBM in every
// launch.  One pass over whichever plan was built (device or host builder) stores each distinct segment once -- a segment
// is position-independent, sdesc[b] points anywhere in pseg -- and each distinct relative line list once, the block's
// first line in lbase[b]; the kernel then reads them from the caches.  A rule, not a measurement: only a span that is not
// its group's canonical word for word keeps its own copy.  A failure leaves the plan unshared.  What it buys on that
// matrix: 51 MB of 893 MB per launch, and no time (profiles/plan_sharing_bench_ab.txt).
void csr_share_plan(spmv_csr_dev *m) {
    XWindowPlan<int2> &xw = m->xw;
    if (g_local_share == 0 || xw.blocks <= 0 || !xw.lines || !xw.ldesc) return;
    UploadTrace trace("csr_share_plan");
    const bool weak = g_local_share == 2;
    PatternPlan &pat = xw.pat;
    if (pat.pseg && pat.sdesc) {
        long long stored = 0, distinct = 0;
        if (share_spans(pat.pseg, pat.sdesc, xw.blocks, 0, false, weak, nullptr, stored, distinct)) {
            pat.seg_total = stored;
            pat.seg_distinct = distinct;
        }
    }
    long long stored = 0, distinct = 0;
    if (share_spans(xw.lines, xw.ldesc, xw.blocks, (size_t)kLocalLinesMax, true, weak, &xw.lbase, stored, distinct)) {
        xw.lines_stored = stored;
        xw.lists_stored = distinct;
    }
    trace.mark("shared segments and line lists");
}

// The x-window phase of upload (csr_stream_local): own blocks at the stage m->local_cap.  One stage size per handle, so
// that its blocks, the gather kernel's and the split long rows agree on which rows are long: a matrix that gets a plan
// runs everything at 2048.  An explicit stream_cap other than that asks for the gather kernel's configuration and skips
// the plan.  rp: the handle's row_ptr, `rows` the same on its way to the device; col: the handle's columns.
// 1: m->xw is the plan, complete -- uploaded, with its pattern plan and the sharing pass -- and `split` marks the rows it
// hands to the split-row kernels; 0: no plan, nothing of it allocated; -1: error.
template <typename T>
int csr_x_window_phase(spmv_csr_dev *m, const std::vector<int> &rp, UploadSource<int> &rows, UploadSource<int> &col,
                       UploadTrace &trace, std::vector<unsigned char> &split) {
    constexpr int line_shift = sizeof(T) == 8 ? 4 : 5;  // 128-byte lines
    const int Ml = m->M_local, lcap = m->local_cap;
    const long long nz = m->nz;
    LocalPlan<int2> local;
    bool have_local = false, on_device = false;
    if (g_stream_local && nz > 0 && (g_stream_cap == 0 || g_stream_cap == lcap)) {
        std::vector<int4> desc, pieces, long_rows;
        csr_build_blocks(Ml, rp.data(), lcap, kStreamRowsCap, desc, pieces, long_rows);
        // on the device when no block lists more than 256 lines (the common case for matrices that get
        // a plan at all: then the line limit would not have moved a block boundary on the host either);
        // otherwise the host builder decides (line-limited blocks, split rows, or no plan)
        int dev = 0;
        if (g_plan_on_device && lcap == kPlanCap) {
            if (col.device_view()) return -1;
            dev = csr_plan_on_device<line_shift>(m, desc, nz);
            if (dev < 0) return -1;
        }
        on_device = have_local = dev == 1;
        if (dev == 0) {  // (2: plainly scattered columns -- no plan, and no need to ask the host builder)
            const int *col_host = col.host_view("csr_upload: copying the columns back for the host plan failed");
            if (!col_host) return -1;
            have_local = csr_build_local(Ml, m->N, rp.data(), col_host, nz, lcap, kStreamRowsCap, line_shift, kLocalLinesMax, desc, local);
        }
        if (on_device) split.assign((size_t)Ml, 0);
        else if (have_local) split.swap(local.split);
    }
    trace.mark("x-window plan (or its refusal)");
    if (!have_local) return 0;
    if (rows.device_view()) return -1;
    if (!on_device && m->xw.upload(local)) return -1;
    // the pattern plan (optional: one that cannot be built is simply not there); all of the plan ahead of the value
    // array (the allocation order above csr_upload_impl)
    csr_pattern_segments(m, build_pattern_tables<false>(m->xw, Ml, nz, m->value_bytes, m->row_ptr));
    // equal segments and line lists once: before the searches, which time the plan the handle keeps
    csr_share_plan(m);
    return 1;
}

// The checks of upload, all ahead of the handle.  rp: rows [row0, row1) of row_ptr, rebased to 0.  Returns the longest
// row, or -1.
template <typename T>
int csr_upload_checks(int M, int N, const int *row_ptr, int row0, int row1, const MatrixSource<T> &from, UploadTrace &trace,
                      std::vector<int> &rp) {
    if (M < 0 || N < 0 || !row_ptr) return fail("csr_upload: bad arguments");
    if (row0 < 0 || row1 < row0 || row1 > M) return fail("csr_upload: bad row range [%d, %d) of %d", row0, row1, M);
    const int Ml = row1 - row0;
    const int e0 = row_ptr[row0], e1 = row_ptr[row1];
    const long long nz = (long long)e1 - e0;
    if (nz < 0) return fail("csr_upload: row_ptr is not monotone");
    if (nz > 0x7fffffffLL - kPad) return fail("csr_upload: %lld entries exceed the 32-bit entry index of the kernels", nz);
    if (nz > 0 && !from.col.adopted && !from.on_host()) return fail("csr_upload: col_idx / values are NULL");
    if ((unsigned long long)N * sizeof(T) >= (1ull << 32))
        return fail("csr_upload: N = %d exceeds the 32-bit gather offset range of the kernels", N);
    // a column index outside [0, N) would make the kernels gather out of bounds (adopted columns are checked already)
    const int *col_idx = from.col.host;
    if (col_idx && e1 > e0) {  // (a few threads: one pass over 2.6e8 indices is 0.15 s of a 1 s upload on one core)
        const int threads = (long long)e1 - e0 >= (1 << 22) ? (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1;
        std::vector<long long> first_bad((size_t)threads, -1);
        tile_detail::run_threads(threads, [&](int th) {
            const long long lo = e0 + ((long long)e1 - e0) * th / threads, hi = e0 + ((long long)e1 - e0) * (th + 1) / threads;
            for (long long e = lo; e < hi; ++e)
                if ((unsigned)col_idx[e] >= (unsigned)N) {
                    first_bad[(size_t)th] = e;
                    break;
                }
        });
        for (long long e : first_bad)
            if (e >= 0) return fail("csr_upload: column index %d at entry %lld is outside [0, %d)", col_idx[e], e, N);
    }
    trace.mark("column check");
    rp.resize((size_t)Ml + 1);
    int max_row = 0;
    for (int r = 0; r <= Ml; ++r) rp[r] = row_ptr[row0 + r] - e0;
    for (int r = 0; r < Ml; ++r) {
        if (rp[r + 1] < rp[r]) return fail("csr_upload: row_ptr decreases at row %d", row0 + r);
        max_row = std::max(max_row, rp[r + 1] - rp[r]);
    }
    return max_row;
}

// The tile phase of upload, for a handle without an x-window plan (columns too scattered for 256 lines per block): the
// 2-D tiles (csr_tile) -- row-block accumulators in LDS, the block's entries re-ordered into column passes so that all
// workgroups sweep x together (L2-resident band), dense passes staged in LDS.  Needs enough row blocks to fill the chip;
// rows longer than tile_lmax stay with the split-row kernels, their pieces cut at column stripes.  tb: the plans, for
// csr_blocks_and_uploads to put into the handle.  -1: error.
template <typename T>
int csr_tile_phase(spmv_csr_dev *m, const std::vector<int> &rp, UploadSource<int> &rows, MatrixSource<T> &src, UploadTrace &trace,
                   TileBuild<T> &tb) {
    const int Ml = m->M_local;
    const long long nz = m->nz;
    if (nz <= 0 || g_stream_tile == 0 || g_stream_cap != 0) return 0;
    if (g_stream_tile != 1 && (long long)Ml < kTileMinRows && nz < kTileMidEntries) return 0;
    // (the host arrays: the host builder's input, the device builder's fallback, and what the stripe-cut pieces are cut from)
    const char *no_copy = "csr_upload: copying the matrix back for the tile plan failed";
    const int *hcol = src.col.host_view(no_copy);
    const T *hval = hcol ? src.val.host_view(no_copy) : nullptr;
    if (!hcol || !hval) return -1;
    std::vector<int> row_len((size_t)Ml);
    for (int r = 0; r < Ml; ++r) row_len[(size_t)r] = rp[(size_t)r + 1] - rp[(size_t)r];
    // the plan is built on the device from the CSR arrays there (tile_plan_device.hpp; "tile_plan_on_device" 0: on
    // host threads, tile_plan.hpp -- the two give the same bytes): the matrix goes up first
    TileDevInput<T> din;
    DevBuf d_row_len;
    const bool on_dev = g_tile_plan_on_device != 0;
    if (on_dev) {
        if (src.col.device_view() || src.val.device_view() || rows.device_view() ||
            upload_array((int **)&d_row_len.p, row_len.data(), row_len.size(), 1))
            return -1;
        din.row_begin = m->row_ptr;
        din.row_len = d_row_len.as<int>();
        din.col = m->col;
        din.val = (const T *)m->val;
        din.stream = g_stream;
    }
    trace.mark("matrix to the device");
    tile_plan_all<T>(Ml, m->N, rp.data(), row_len.data(), rp.data(), nz, hcol, hval, tb, on_dev ? &din : nullptr);
    trace.mark("tile plans");
    return 0;
}

// The workgroup blocks and split rows of the gather kernels, then whatever of the handle is not on the device yet.
// split: the rows the x-window plan hands to the split-row kernels (nullptr: no plan); tb: the tile phase's plans.
template <typename T>
int csr_blocks_and_uploads(spmv_csr_dev *m, const std::vector<int> &rp, UploadSource<int> &rows, MatrixSource<T> &src,
                           const std::vector<unsigned char> *split, TileBuild<T> &tb) {
    const int Ml = m->M_local;
    const long long nz = m->nz;
    // larger stages amortise per-workgroup latency on big matrices; small ones need enough workgroups to fill 256 CUs
    // (measured: cant-like 2048, nlpkkt-like 4096); a matrix with an x-window plan runs everything at the plan's stage
    m->stream_cap = split ? m->local_cap : (g_stream_cap ? g_stream_cap : (nz >= (16LL << 20) ? 4096 : 2048));
    // Skewed rows (gather kernels): a block's rows are summed by lane groups sized for the NUMBER of rows in it, so in
    // a block of a few hundred short rows one row of a thousand entries is summed by a single lane while everybody else
    // waits (webbase-like stand-in, 1 M rows, 3.3 entries per row on average, 2 262 in the longest: 73 us; with its rows
    // beyond the limit below handed to the split-row kernels, one workgroup each: see profiles/r2_reference_list_stand_ins.md).
    // Rows longer than max(128, 16 x the average row) count as long there -- from 2^20 entries on: the two extra
    // launches of the split-row kernels cost ~5 us, more than a small matrix's whole product.
    std::vector<unsigned char> skew_split;
    if (!split && g_skew_rows && Ml > 0 && nz >= (1LL << 20)) {
        const long long limit = std::max<long long>(128, 16 * (nz / Ml));
        if (limit < m->stream_cap - 3) {
            bool any = false;
            skew_split.assign((size_t)Ml, 0);
            for (int r = 0; r < Ml; ++r)
                if (rp[(size_t)r + 1] - rp[(size_t)r] > limit) skew_split[(size_t)r] = 1, any = true;
            if (any) split = &skew_split;
        }
    }
    std::vector<int4> desc, pieces, long_rows;
    csr_build_blocks(Ml, rp.data(), m->stream_cap, kStreamRowsCap, desc, pieces, long_rows, split);
    m->num_blocks = (int)desc.size();
    m->num_long = (int)long_rows.size();
    m->num_partial = (int)pieces.size();
    // (the tile plans add their own bytes)
    m->rest_bytes = rp.size() * 4 + ((size_t)nz + kPad) * (4 + sizeof(T)) + desc.size() * 16 + long_rows.size() * 16 +
                    pieces.size() * 16 + (size_t)m->num_partial * sizeof(T) + ((size_t)m->N + (size_t)m->M_total) * sizeof(T);
    if (rows.device_view() || src.col.device_view() || src.val.device_view()) return -1;
    if (upload_array(&m->desc, desc.data(), desc.size(), 1)) return -1;
    if (m->num_long && upload_array(&m->long_rows, long_rows.data(), long_rows.size(), 0)) return -1;
    if (m->num_partial && upload_array(&m->pieces, pieces.data(), pieces.size(), 0)) return -1;
    if (tile_upload_all<T>(m, tb) < 0) return -1;  // (1 = the device refused the LDS size: no tiles, not an error)
    const int partial_slots = std::max(m->num_partial, (int)tb.tile_pieces.size());
    if (partial_slots) {
        hipError_t e = hipMalloc(&m->partial, (size_t)partial_slots * sizeof(T));
        if (e != hipSuccess) return fail("hipMalloc(partial) failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// What SPMV_CSR_AUTO runs, and the lanes per row of the lane-group kernel.
// Mid-size matrices that get neither plan (scattered columns, below the tile plans' size): the lane-group kernel
// beats the gather stream kernels by 3-10 % on every such stand-in of the reference's list (cop20k_A-size 19.2 vs
// 21.2 us, PR02R-size 37 vs 41, amazon0302-size 12.1 vs 13.5; profiles/r2_reference_list_stand_ins.md) -- unless rows
// are skewed (its lanes per row are fixed), and not on large ones (road-like 12 M rows: 282 vs 255 us).
void csr_auto_variant(spmv_csr_dev *m, bool have_plan) {
    const double mean = m->M_local ? (double)m->nz / m->M_local : 0.0;
    m->lanes_per_row = lanes_for_mean_row(mean);
    m->auto_variant = SPMV_CSR_STREAM;
    if (!have_plan && m->nz < (20LL << 20) && m->max_row <= std::max(64.0, 8.0 * mean)) m->auto_variant = SPMV_CSR_SUBWAVE;
}

// The searches of a finished handle (upload_ops.hpp); the placement of m->val where it is large and streamed by the
// handle's kernel (a tile plan without an x-window plan streams its own re-ordered copy).
template <typename T>
void csr_upload_searches(spmv_csr_dev *m) {
    const bool place = (size_t)m->nz * sizeof(T) >= kPlaceMinBytes && !m->tiles_only && (m->xw.blocks > 0 || m->tile.blocks == 0);
    upload_searches(m, place ? &m->val : nullptr, ((size_t)m->nz + kPad) * sizeof(T),
                    [m] { return csr_launch_any(m, SPMV_CSR_AUTO, m->x, m->y, g_stream); });
}

// Upload: the matrix `from` -- host arrays, or device arrays of row_ptr[row1] - row_ptr[row0] (+ kPad zeroed) entries
// that the handle adopts, their columns already checked -- becomes a handle over rows [row0, row1).
//
// THE ORDER OF THE DEVICE ALLOCATIONS is part of the handle: where an array lands follows from what was allocated before
// it, and the first placement of the value array decides what the x-window kernel makes of it (tune_placement,
// upload_ops.hpp).  An array is allocated by the first phase that asks for its device view, so the order is:
//   1. x-window phase   (a) only when the plan is tried on the device: col, the builder's scratch (freed again), then
//                           the plan -- lines, slot, ldesc4, ldesc;
//                       (b) only when there is a plan: row_ptr; a host-built plan's ldesc4, ldesc, lines, slot; the
//                           pattern plan; the shared segments and line lists.
//   2. tile phase       only without an x-window plan, and only when the tile plan is built on the device: col, val,
//                       row_ptr (each unless it is there), the row lengths (freed again), the device builder's arrays.
//   3. blocks, uploads  row_ptr, col, val (each unless it is there), desc, long_rows, pieces, the tile plans, partial.
//   4. vectors          x, y.
//   5. searches         candidates for val (tune_placement).
// So with an x-window plan val comes behind the whole plan, and with a device-built tile plan ahead of it.
template <typename T>
int csr_upload_impl(int M, int N, const int *row_ptr, int row0, int row1, const MatrixSource<T> &from, spmv_csr_dev **out) {
    if (need_device()) return -1;
    if (!out) return fail("csr_upload: out is NULL");
    *out = nullptr;
    UploadTrace trace("csr_upload");
    std::vector<int> rp;
    const int max_row = csr_upload_checks<T>(M, N, row_ptr, row0, row1, from, trace, rp);
    if (max_row < 0) return -1;

    HandleGuard<spmv_csr_dev, spmv_hip_csr_free> guard(new (std::nothrow) spmv_csr_dev());
    spmv_csr_dev *m = guard.h;
    if (!m) return fail("csr_upload: out of host memory");
    m->value_bytes = (int)sizeof(T), m->nz = rp.back(), m->max_row = max_row;
    m->M_local = row1 - row0, m->M_total = M, m->N = N, m->row0 = row0;
    // (1024-entry x-window blocks were tried for small matrices: cant-like 13.2 us against 11.7 us at 2048)
    m->local_cap = g_local_cap ? g_local_cap : 2048;
    // (behind the guard: on a failure the source goes first and takes adopted arrays out of the handle again)
    MatrixSource<T> src(from);
    src.bind(&m->col, (T **)&m->val, (size_t)row_ptr[row0], (size_t)m->nz, kPad);
    UploadSource<int> rows;
    rows.host = rp.data();
    rows.bind(&m->row_ptr, 0, rp.size(), (size_t)kRowPtrPad);

    std::vector<unsigned char> split;
    TileBuild<T> tb;
    const int planned = csr_x_window_phase<T>(m, rp, rows, src.col, trace, split);
    if (planned < 0) return -1;
    if (!planned && csr_tile_phase<T>(m, rp, rows, src, trace, tb)) return -1;
    if (csr_blocks_and_uploads<T>(m, rp, rows, src, planned ? &split : nullptr, tb)) return -1;
    if (alloc_vectors(&m->x, &m->y, N, M, (int)sizeof(T))) return -1;
    csr_auto_variant(m, planned || tb.tiles.have);
    trace.mark("blocks, remaining uploads, vectors");
    csr_upload_searches<T>(m);
    trace.mark("placement tuning");
    src.keep();
    *out = guard.release();
    return 0;
}

}  // namespace

// Host-only self-check of the upload-time preprocessing (no device needed): builds the workgroup
// blocks and the x-window plan for the given CSR structure exactly as upload does and verifies
// their invariants -- blocks and split rows partition the rows, every block fits the stage and
// lists at most kLocalLinesMax strictly ascending lines, every entry's 16-bit slot leads back to
// its column.  stats (optional, 6 ints): gather blocks, x-window blocks (0 = no plan), listed
// lines, widest block's lines, long rows, rows handed over because of the line limit.
static int spmv_hip_csr_plan_check_body(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes,
                                       int *stats) {
    if (M < 0 || N < 0 || !row_ptr || (value_bytes != 4 && value_bytes != 8)) return fail("plan_check: bad arguments");
    const long long nz = row_ptr[M];
    if (nz > 0 && !col_idx) return fail("plan_check: col_idx is NULL");
    for (int r = 0; r < M; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail("plan_check: row_ptr decreases at row %d", r);
    for (long long e = 0; e < nz; ++e)
        if ((unsigned)col_idx[e] >= (unsigned)N) return fail("plan_check: column %d outside [0, %d)", col_idx[e], N);
    const int cap = 2048, shift = value_bytes == 8 ? 4 : 5, mask = (1 << shift) - 1;
    std::vector<int4> desc, pieces, long_rows;
    LocalPlan<int2> plan;
    csr_build_blocks(M, row_ptr, cap, kStreamRowsCap, desc, pieces, long_rows);
    const bool have = nz > 0 && csr_build_local(M, N, row_ptr, col_idx, nz, cap, kStreamRowsCap, shift,
                                                kLocalLinesMax, desc, plan);
    csr_build_blocks(M, row_ptr, cap, kStreamRowsCap, desc, pieces, long_rows, have ? &plan.split : nullptr);
    // gather blocks + long rows partition the rows
    std::vector<unsigned char> seen((size_t)M, 0);
    auto claim = [&](int r0, int n, const char *what) {
        for (int r = r0; r < r0 + n; ++r) {
            if (r < 0 || r >= M || seen[r]) return fail("plan_check: row %d claimed twice or out of range (%s)", r, what);
            seen[r] = 1;
        }
        return 0;
    };
    // no lane of the row-sum phase adds up more than kSkewPerLane entries unless its row is alone in the block
    auto lane_load_ok = [&](const int4 &d) {
        int longest = 0;
        for (int r = d.x; r < d.x + d.z; ++r) longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
        return d.z == 1 || longest / host_lanes_for_rows(d.z) <= kSkewPerLane;
    };
    for (const int4 &d : desc) {
        if (claim(d.x, d.z, "gather block")) return -1;
        if (d.z <= 0 || d.z > kStreamRowsCap || d.y != row_ptr[d.x] || d.w != row_ptr[d.x + d.z] ||
            d.w - (d.y & kBaseMask) > cap)
            return fail("plan_check: gather block at row %d is malformed", d.x);
        if (!lane_load_ok(d)) return fail("plan_check: gather block at row %d leaves a long row to too few lanes", d.x);
    }
    int split_rows = 0;
    for (const int4 &l : long_rows) {
        if (claim(l.x, 1, "long row")) return -1;
        long long covered = 0;
        for (int k = 0; k < l.z; ++k) {
            const int4 &pc = pieces[(size_t)l.y + k];
            if (pc.x != l.x || pc.z - pc.y <= 0 || pc.z - pc.y > kLongPiece) return fail("plan_check: bad piece of row %d", l.x);
            covered += pc.z - pc.y;
        }
        if (covered != row_ptr[l.x + 1] - row_ptr[l.x]) return fail("plan_check: pieces of row %d do not cover it", l.x);
        const bool by_length = row_ptr[l.x + 1] - row_ptr[l.x] > cap - 3;
        if (!by_length && !(have && plan.split[l.x])) return fail("plan_check: row %d is split without a reason", l.x);
        split_rows += !by_length;
    }
    for (int r = 0; r < M; ++r)
        if (!seen[r]) return fail("plan_check: row %d belongs to no block", r);
    int widest = 0;
    if (have) {
        std::fill(seen.begin(), seen.end(), 0);
        if (plan.desc.size() != plan.ldesc.size()) return fail("plan_check: descriptor arrays differ in length");
        for (size_t b = 0; b < plan.desc.size(); ++b) {
            const int4 &d = plan.desc[b];
            const int2 &ld = plan.ldesc[b];
            if (claim(d.x, d.z, "x-window block")) return -1;
            if (d.z <= 0 || d.z > kStreamRowsCap || d.y != row_ptr[d.x] || d.w != row_ptr[d.x + d.z] ||
                d.w - (d.y & kBaseMask) > cap)
                return fail("plan_check: x-window block at row %d is malformed", d.x);
            if (!lane_load_ok(d)) return fail("plan_check: x-window block at row %d leaves a long row to too few lanes", d.x);
            if (ld.y < 1 || ld.y > kLocalLinesMax || ld.x < 0 || (size_t)ld.x + ld.y > plan.lines.size())
                return fail("plan_check: line list of block %zu is malformed", b);
            for (int k = 1; k < ld.y; ++k)
                if (plan.lines[ld.x + k] <= plan.lines[ld.x + k - 1]) return fail("plan_check: lines of block %zu not ascending", b);
            for (int e = d.y; e < d.w; ++e) {
                const int slot = plan.lcol[e], rank = slot >> shift;
                if (rank >= ld.y || plan.lines[ld.x + rank] != (col_idx[e] >> shift) || (slot & mask) != (col_idx[e] & mask))
                    return fail("plan_check: entry %d (column %d) has slot %d, which is not its column", e, col_idx[e], slot);
            }
            widest = std::max(widest, ld.y);
        }
        // every row is in an x-window block, long, or split because of its lines
        for (int r = 0; r < M; ++r) {
            const bool by_length = row_ptr[r + 1] - row_ptr[r] > cap - 3;
            if (!seen[r] && !by_length && !plan.split[r]) return fail("plan_check: row %d is in no x-window block", r);
            if (seen[r] && (by_length || plan.split[r])) return fail("plan_check: row %d is both in a block and split", r);
        }
        if (plan.stage_lines < widest || plan.stage_lines % kLocalLineQuantum) return fail("plan_check: bad stage size");
    }
    if (stats) {
        stats[0] = (int)desc.size();
        stats[1] = have ? (int)plan.desc.size() : 0;
        stats[2] = have ? (int)plan.lines.size() - kLocalLinesMax : 0;
        stats[3] = widest;
        stats[4] = (int)long_rows.size();
        stats[5] = split_rows;
    }
    return 0;
}

extern "C" int spmv_hip_csr_plan_check(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes,
                                       int *stats) {
    return guarded("csr_plan_check", [&] { return spmv_hip_csr_plan_check_body(M, N, row_ptr, col_idx, value_bytes, stats); });
}

// Host-only self-check of the csr_tile plan (no device needed): builds the tiles and the stripe-cut pieces
// exactly as upload does and (1) verifies the structural invariants the kernel relies on (aligned passes
// within the chunk, ascending rows with a head flag on every row's first entry, staged columns inside the
// window, passes walking the columns upwards), (2) adds an integer checksum per entry into its row's
// accumulator and compares every row with the checksum of its entries taken straight from the CSR arrays.  stats (optional, 6 values per
// plan kind): blocks, passes, entries in tiles, entries in staged passes, rows left to the split-row kernels, widest window.
template <typename T>
static int tile_plan_check(int M, int N, const int *rp, const int *col, int rows_per_block, int lmax, int density,
                           int chunk, int balance, bool pack, long long *stats) {
    const long long nz = rp[M];
    std::vector<T> val((size_t)nz);
    for (long long e = 0; e < nz; ++e) val[(size_t)e] = (T)(1 + e % 7);
    TilePlan<T> plan;
    std::vector<int> row_len((size_t)M);
    for (int r = 0; r < M; ++r) row_len[(size_t)r] = rp[r + 1] - rp[r];
    if (!tile_build<T>(M, N, rp, row_len.data(), col, val.data(), rows_per_block, lmax, density, chunk, balance != 0, 17, plan, pack, 0, pack ? 256 : 0))
        return fail("tile_plan_check: the plan does not fit 32-bit entry offsets");
    // the remainder (packed plans: entries of windows too sparse for a pass): by (row, column), rows of the tiles only
    std::vector<unsigned long long> rem_sum((size_t)M, 0ull);
    if (plan.rem_row.size() != plan.rem_col.size() || plan.rem_row.size() != plan.rem_val.size() || (!pack && !plan.rem_row.empty()))
        return fail("tile_plan_check: remainder arrays disagree");
    for (size_t k = 0; k < plan.rem_row.size(); ++k) {
        const int r = plan.rem_row[k], c = plan.rem_col[k];
        if ((unsigned)r >= (unsigned)M || (unsigned)c >= (unsigned)N || plan.split[(size_t)r])
            return fail("tile_plan_check: remainder entry %zu is out of range", k);
        if (k > 0 && (plan.rem_row[k - 1] > r || (plan.rem_row[k - 1] == r && plan.rem_col[k - 1] > c)))
            return fail("tile_plan_check: the remainder is not ordered by (row, column)");
        rem_sum[(size_t)r] += (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull + (unsigned long long)(double)plan.rem_val[k];
    }
    const int win_cols = plan.win_cols;
    auto h = [](long long c, double v) { return (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull + (unsigned long long)v; };
    if ((int)plan.block_pass.size() != plan.num_blocks + 1 || plan.block_pass.back() != (int)plan.pass_desc.size() ||
        (int)plan.block_row.size() != plan.num_blocks + 1 || plan.block_row[0] != 0 || plan.block_row.back() != M)
        return fail("tile_plan_check: block / pass tables disagree");
    long long seen_entries = 0;
    std::vector<unsigned long long> acc((size_t)rows_per_block);
    for (int b = 0; b < plan.num_blocks; ++b) {
        std::fill(acc.begin(), acc.end(), 0ull);
        const int r0 = plan.block_row[(size_t)b], nrows = plan.block_row[(size_t)b + 1] - r0;
        if (nrows <= 0 || nrows > rows_per_block) return fail("tile_plan_check: block %d holds %d rows", b, nrows);
        long long last_max_col = -1;
        for (int p = plan.block_pass[b]; p < plan.block_pass[b + 1]; ++p) {
            const int4 d = plan.pass_desc[p];
            const int count = d.y, wbase = d.z, wlen = d.w & kTileWlenMask;
            const bool packed = (d.w & kTilePassPacked) != 0;
            if (packed && !wlen) return fail("tile_plan_check: pass %d is packed without a window", p);
            // a packed plan is for the kernel without gather code: every pass staged and packed, no key array
            if (packed != pack) return fail("tile_plan_check: pass %d of a %s plan is %s", p, pack ? "packed" : "plain", packed ? "packed" : "not");
            constexpr int kPer = 16 / (int)sizeof(T);
            // (a block without entries carries one pass of none)
            const bool none = count == 0 && plan.block_pass[b + 1] - plan.block_pass[b] == 1;
            if ((count <= 0 && !none) || count > chunk || (d.x & 3) || (wbase & 3) || (wlen % kPer) || wlen < 0)
                return fail("tile_plan_check: pass %d is malformed", p);
            if ((size_t)d.x + (size_t)count > plan.tcol.size() - kTileChunkMax) return fail("tile_plan_check: pass %d leaves the arrays", p);
            if (wlen && (wlen > win_cols || wbase + wlen > (N + kPer - 1) / kPer * kPer))
                return fail("tile_plan_check: window of pass %d is too wide or leaves x", p);
            int prev_row = -1;
            long long cmin = 1LL << 40, cmax = -1;
            for (int i = 0; i < count; ++i) {
                // a pass that can be staged holds packed words; decode as the kernel does
                const unsigned word = (unsigned)plan.tcol[(size_t)d.x + i];
                const int c = packed ? wbase + (int)(word & kTilePackColMask) : (int)word;
                const unsigned key = packed ? ((word >> 16) & (unsigned)kTileHead) | ((word >> kTilePackShift) & (unsigned)kTileRowMask)
                                            : plan.tkey[(size_t)d.x + i];
                const int lrow = (int)(key & kTileRowMask);
                if ((unsigned)c >= (unsigned)N || lrow >= nrows) return fail("tile_plan_check: entry %d of pass %d is out of range", i, p);
                if (wlen && (c < wbase || c >= wbase + wlen)) return fail("tile_plan_check: staged pass %d misses column %d", p, c);
                if (!wlen && c < wbase) return fail("tile_plan_check: pass %d has a column below its base", p);
                const bool head = (key & kTileHead) != 0;
                if (head != (lrow != prev_row)) return fail("tile_plan_check: head flag of entry %d in pass %d is wrong", i, p);
                if (lrow < prev_row) return fail("tile_plan_check: rows of pass %d are not ascending", p);
                if (key & ~(unsigned)(kTileHead | kTileRowMask)) return fail("tile_plan_check: stray key bits in pass %d", p);
                prev_row = lrow;
                cmin = std::min<long long>(cmin, c);
                cmax = std::max<long long>(cmax, c);
                // what the kernel does with the entry: every run goes to its row's accumulator exactly once
                acc[(size_t)lrow] += h(c, (double)plan.tval[(size_t)d.x + i]);
            }
            // passes of a block walk the columns upwards (that is what keeps the gathered band in L2)
            if (cmin < last_max_col) return fail("tile_plan_check: passes of block %d do not ascend in columns", b);
            last_max_col = cmax;
            seen_entries += count;
        }
        for (int i = 0; i < nrows; ++i) {
            unsigned long long want = 0;
            if (!plan.split[(size_t)r0 + i])
                for (int e = rp[r0 + i]; e < rp[r0 + i + 1]; ++e) want += h(col[e], (double)val[(size_t)e]);
            if (acc[(size_t)i] + rem_sum[(size_t)r0 + i] != want) return fail("tile_plan_check: row %d does not add up through the tiles", r0 + i);
        }
    }
    if (seen_entries != plan.entries) return fail("tile_plan_check: entry count disagrees");
    // streams (what a workgroup walks): every block exactly once, its passes in order, the flag on its last pass
    for (int places : {8, 64, 512, 1 << 30}) {
        tile_make_streams(plan, places);
        if (plan.spass.size() != plan.pass_desc.size() || (int)plan.sblock_rows.size() != plan.num_blocks ||
            (int)plan.stream_pass.size() != plan.num_streams + 1 || (int)plan.stream_block.size() != plan.num_streams + 1 ||
            (plan.num_streams & 7) || (plan.num_blocks > places && plan.num_streams > std::max(8, places / 8 * 8)))
            return fail("tile_plan_check: stream tables disagree (%d places)", places);
        std::vector<unsigned char> seen_block((size_t)plan.num_blocks, 0);
        for (int st = 0; st < plan.num_streams; ++st) {
            int p = plan.stream_pass[(size_t)st];
            for (int k = plan.stream_block[(size_t)st]; k < plan.stream_block[(size_t)st + 1]; ++k) {
                const int2 br = plan.sblock_rows[(size_t)k];
                const int b = (int)(std::upper_bound(plan.block_row.begin(), plan.block_row.end() - 1, br.x) - plan.block_row.begin()) - 1;
                if (b < 0 || b >= plan.num_blocks || plan.block_row[(size_t)b] != br.x || plan.block_row[(size_t)b + 1] - br.x != br.y ||
                    seen_block[(size_t)b]++)
                    return fail("tile_plan_check: stream %d lists a block twice or with the wrong rows", st);
                for (int q = plan.block_pass[(size_t)b]; q < plan.block_pass[(size_t)b + 1]; ++q, ++p) {
                    const int4 a = plan.pass_desc[(size_t)q], c = plan.spass[(size_t)p];
                    const bool last = q + 1 == plan.block_pass[(size_t)b + 1];
                    if (a.x != c.x || a.y != c.y || a.z != c.z || (a.w | (last ? kTilePassLast : 0)) != c.w)
                        return fail("tile_plan_check: stream %d does not repeat block %d's passes", st, b);
                }
            }
            if (p != plan.stream_pass[(size_t)st + 1]) return fail("tile_plan_check: stream %d's passes and blocks disagree", st);
        }
        for (unsigned char c : seen_block)
            if (c != 1) return fail("tile_plan_check: a block is in no stream");
    }
    // rows beyond the limit: stripe-cut pieces cover each exactly once, slots row by row
    std::vector<int4> pieces, long_rows;
    const int stripe_cols = (1 << 20) / (int)sizeof(T);
    build_striped_pieces(M, rp, col, plan.split, stripe_cols, pieces, long_rows);
    std::vector<const int4 *> by_slot(pieces.size(), nullptr);
    long long split_entries = 0;
    int last_stripe = -1;
    for (const int4 &pc : pieces) {
        if (pc.w < 0 || (size_t)pc.w >= pieces.size() || by_slot[(size_t)pc.w]) return fail("tile_plan_check: piece slots are not a permutation");
        by_slot[(size_t)pc.w] = &pc;
        if (pc.z <= pc.y || pc.z - pc.y > kLongPiece) return fail("tile_plan_check: bad piece of row %d", pc.x);
        const int stripe = col[pc.y] / stripe_cols;
        if (stripe < last_stripe) return fail("tile_plan_check: pieces are not ordered by stripe");
        last_stripe = stripe;
    }
    int n_split = 0;
    for (const int4 &l : long_rows) {
        if (!plan.split[(size_t)l.x]) return fail("tile_plan_check: row %d is split without being long", l.x);
        int at = rp[l.x];
        for (int k = 0; k < l.z; ++k) {
            const int4 *pc = by_slot[(size_t)l.y + k];
            if (!pc || pc->x != l.x || pc->y != at) return fail("tile_plan_check: pieces of row %d are not contiguous in slot order", l.x);
            at = pc->z;
        }
        if (at != rp[l.x + 1]) return fail("tile_plan_check: pieces of row %d do not cover it", l.x);
        split_entries += rp[l.x + 1] - rp[l.x];
        ++n_split;
    }
    for (int r = 0; r < M; ++r) n_split -= plan.split[(size_t)r];
    if (n_split != 0) return fail("tile_plan_check: split rows and piece lists disagree");
    if (split_entries + plan.entries + (long long)plan.rem_row.size() != nz) return fail("tile_plan_check: tiles + remainder + split rows do not hold every entry");
    if (stats) {
        stats[0] = plan.num_blocks;
        stats[1] = (long long)plan.pass_desc.size();
        stats[2] = plan.entries + (long long)plan.rem_row.size();  // (packed: the remainder counts as held, not as staged)
        stats[3] = plan.staged_entries;
        stats[4] = (long long)long_rows.size();
        stats[5] = plan.max_win;
    }
    return 0;
}

extern "C" int spmv_hip_csr_tile_plan_check(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes,
                                            int rows_per_block, int lmax, int density, int chunk, int balance,
                                            long long *stats) {
    if (M < 0 || N < 0 || !row_ptr || (value_bytes != 4 && value_bytes != 8)) return fail("tile_plan_check: bad arguments");
    if (rows_per_block < 256 || rows_per_block > kTileRowsMax || (rows_per_block & 255) || lmax < 1 ||
        lmax > 65536 || density < 1 || chunk != 2048)
        return fail("tile_plan_check: bad plan parameters");
    const long long nz = row_ptr[M];
    if (nz > 0 && !col_idx) return fail("tile_plan_check: col_idx is NULL");
    for (int r = 0; r < M; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail("tile_plan_check: row_ptr decreases at row %d", r);
    for (long long e = 0; e < nz; ++e)
        if ((unsigned)col_idx[e] >= (unsigned)N) return fail("tile_plan_check: column %d outside [0, %d)", col_idx[e], N);
    // both kinds of plan: with gather passes (the stats are this one's) and packed (every pass staged)
    return guarded("tile_plan_check", [&] {
        for (int pack = 0; pack < 2; ++pack) {
            long long *st = pack ? (stats ? stats + 6 : nullptr) : stats;
            const int rc = value_bytes == 8 ? tile_plan_check<double>(M, N, row_ptr, col_idx, rows_per_block, lmax, density, chunk, balance, pack != 0, st)
                                            : tile_plan_check<float>(M, N, row_ptr, col_idx, rows_per_block, lmax, density, chunk, balance, pack != 0, st);
            if (rc) return rc;
        }
        return 0;
    });
}

// What upload would decide for this structure (host only, current tunings): tile_plan_all's choices.
template <typename T>
static int tile_auto_plan(int M, int N, const int *rp, const int *col, long long *stats) {
    const long long nz = rp[M];
    std::vector<T> val((size_t)nz, T(1));
    std::vector<int> row_len((size_t)M);
    for (int r = 0; r < M; ++r) row_len[(size_t)r] = rp[r + 1] - rp[r];
    TileBuild<T> tb;
    tile_plan_all<T>(M, N, rp, row_len.data(), rp, nz, col, val.data(), tb);
    for (int k = 0; k < 10; ++k) stats[k] = 0;
    stats[0] = tb.tiles.have;
    if (!tb.tiles.have) return 0;
    const TilePlan<T> &tiles = tb.tiles.plan;
    int tallest = 0;
    for (int b = 0; b < tiles.num_blocks; ++b) tallest = std::max(tallest, tiles.block_row[(size_t)b + 1] - tiles.block_row[(size_t)b]);
    stats[1] = tb.tiles.packed;
    stats[2] = tb.scattered;
    stats[3] = tiles.rows_per_block;
    stats[4] = tiles.num_blocks;
    stats[5] = tiles.num_streams;
    stats[6] = (long long)tiles.pass_desc.size();
    stats[7] = tallest;
    stats[8] = tb.lt.have ? (long long)tb.lt.work.size() : 0;
    stats[9] = tiles.entries;
    return 0;
}

extern "C" int spmv_hip_csr_tile_auto_plan(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes,
                                           long long *stats) {
    if (M < 0 || N < 0 || !row_ptr || !stats || (value_bytes != 4 && value_bytes != 8)) return fail("tile_auto_plan: bad arguments");
    const long long nz = row_ptr[M];
    if (nz > 0 && !col_idx) return fail("tile_auto_plan: col_idx is NULL");
    for (int r = 0; r < M; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail("tile_auto_plan: row_ptr decreases at row %d", r);
    for (long long e = 0; e < nz; ++e)
        if ((unsigned)col_idx[e] >= (unsigned)N) return fail("tile_auto_plan: column %d outside [0, %d)", col_idx[e], N);
    return guarded("tile_auto_plan", [&] {
        return value_bytes == 8 ? tile_auto_plan<double>(M, N, row_ptr, col_idx, stats) : tile_auto_plan<float>(M, N, row_ptr, col_idx, stats);
    });
}

// a whole fp64 matrix whose col / val already sit on the device (spmv_coo.hip)
int csr_adopt_f64(int M, int N, const int *row_ptr_host, int *d_col, double *d_val, spmv_csr_dev **out) {
    return guarded("csr_adopt", [&] { return csr_upload_impl<double>(M, N, row_ptr_host, 0, M, MatrixSource<double>::adopting(d_col, d_val), out); });
}
// ... and its fp32 twin (spmv_transpose.hip)
int csr_adopt_f32(int M, int N, const int *row_ptr_host, int *d_col, float *d_val, spmv_csr_dev **out) {
    return guarded("csr_adopt", [&] { return csr_upload_impl<float>(M, N, row_ptr_host, 0, M, MatrixSource<float>::adopting(d_col, d_val), out); });
}

// A handle that carries NOTHING but tile plans, for rows given as (first entry, length) pairs over host arrays:
// how an HLL slab whose columns are too scattered for the x-window plan gets csr_tile (spmv_hll.hip).  The rows
// are rows [row0, row0 + M_local) of a matrix with M_total rows; launched with the caller's x and full-length y.
// *out stays NULL (return 0) when the rows get no plan.
// (Defined here, behind the uploads above, and not with the rest of the tile orchestration in tile_upload.hpp: the order in
// which this translation unit first names tile_plan_all<float> and <double> is the order of their kernels in its code object.)
int csr_tiles_from_rows_f64(int M_local, int M_total, int row0, int N, const int *row_begin, const int *row_len,
                            long long entries, MatrixSource<double> &slab, spmv_csr_dev **out) {
    *out = nullptr;
    if (M_local <= 0 || entries <= 0 || g_stream_tile == 0) return 0;
    if (g_stream_tile < 0 && (long long)M_local < kTileMinRows && entries < kTileMidEntries) return 0;
    return guarded("hll tile plan", [&] {
        TileBuild<double> tb;
        // the slab on the device: the plan is built there (the rows' begin / length lists go up), and host arrays the
        // caller happens to have are the fallback; else by the host builder, from the host view
        TileDevInput<double> din;
        int *d_begin = nullptr, *d_len = nullptr;
        bool on_dev = g_tile_plan_on_device != 0 && slab.on_device();
        const int *col = slab.col.host;
        const double *val = slab.val.host;
        if (!on_dev) {
            col = slab.col.host_view("hll_from_csr: JA download failed: %s");
            val = col ? slab.val.host_view("hll_from_csr: AS download failed: %s") : nullptr;
            if (!col || !val) return -1;
        }
        if (on_dev && (upload_array(&d_begin, row_begin, (size_t)M_local, 1) || upload_array(&d_len, row_len, (size_t)M_local, 1)))
            on_dev = false;
        if (on_dev) {
            din.row_begin = d_begin;
            din.row_len = d_len;
            din.col = *slab.col.field;
            din.val = *slab.val.field;
            din.stream = g_stream;
        }
        tile_plan_all<double>(M_local, N, row_begin, row_len, nullptr, entries, col, val, tb, on_dev ? &din : nullptr);
        (void)hipFree(d_begin);
        (void)hipFree(d_len);
        if (!tb.tiles.have) return 0;
        HandleGuard<spmv_csr_dev, spmv_hip_csr_free> guard(new (std::nothrow) spmv_csr_dev());
        spmv_csr_dev *m = guard.h;
        if (!m) return fail("hll tile plan: out of host memory");
        m->value_bytes = 8;
        m->M_local = M_local;
        m->M_total = M_total;
        m->N = N;
        m->row0 = row0;
        m->nz = entries;
        m->tiles_only = true;
        m->auto_variant = SPMV_CSR_STREAM;
        const int trc = tile_upload_all<double>(m, tb);
        if (trc) return trc < 0 ? -1 : 0;  // 1: no tiles on this device (the slab keeps hll_lds), -1: a real failure
        *out = guard.release();
        return 0;
    });
}

static void release_relocated(spmv_csr_dev::relocated &r) {
    if (!r.raw) return;
    if (r.vmm) {
        (void)hipMemUnmap(r.raw, r.mapped);
        (void)hipMemAddressFree(r.raw, r.mapped);
        (void)hipMemRelease(r.phys);
    } else {
        (void)hipFree(r.raw);
    }
    r.raw = nullptr;
}

extern "C" int spmv_hip_csr_upload(int M, int N, const int *row_ptr, const int *col_idx,
                                   const double *values, int row0, int row1, spmv_csr_dev **out) {
    return guarded("csr_upload", [&] { return csr_upload_impl<double>(M, N, row_ptr, row0, row1, MatrixSource<double>::on_host(col_idx, values), out); });
}

extern "C" int spmv_hip_csr_upload_f32(int M, int N, const int *row_ptr, const int *col_idx,
                                       const float *values, int row0, int row1, spmv_csr_dev **out) {
    return guarded("csr_upload_f32", [&] { return csr_upload_impl<float>(M, N, row_ptr, row0, row1, MatrixSource<float>::on_host(col_idx, values), out); });
}

extern "C" int spmv_hip_csr_upload_matrix(const CSRMatrix *csr, spmv_csr_dev **out) {
    if (!csr) return fail("csr_upload_matrix: csr is NULL");
    return spmv_hip_csr_upload(csr->M, csr->N, csr->row_ptr, csr->col_idx, csr->values, 0, csr->M, out);
}

// (here: the expansion is a complete type in this translation unit)
void OwnTiles::release() {
    free_all(arrays());
    delete expansion;
    *this = OwnTiles();
}

extern "C" void spmv_hip_csr_free(spmv_csr_dev *m) {
    if (!m) return;
    spmv_hip_csr_free(m->own_part);
    spmv_hip_csr_free(m->halo_part);
    for (auto &r : m->relocs) {  // relocated arrays: the field points into r.raw
        *r.field = nullptr;
        release_relocated(r);
    }
    (void)hipFree(m->row_ptr);
    (void)hipFree(m->col);
    (void)hipFree(m->val);
    (void)hipFree(m->desc);
    m->xw.release();
    m->tile.release();
    m->lt.release();
    m->mt.release();
    (void)hipFree(m->interior_ids);
    (void)hipFree(m->boundary_ids);
    (void)hipFree(m->long_rows);
    (void)hipFree(m->pieces);
    (void)hipFree(m->partial);
    (void)hipFree(m->spmm_partial);
    (void)hipFree(m->x);
    (void)hipFree(m->y);
    delete m->upd;
    delete m;
}

// Placement study / placement rule: move one array of the handle to an address of the form
// (multiple of `align`) + offset.  which: 0 row_ptr, 1 col, 2 val, 3 x, 4 y, 5 lcol, 6 lines, 7 ldesc4.
// vmm != 0: the new home is built with the virtual-memory API instead of hipMalloc -- physical memory from
// hipMemCreate (one handle, size rounded to the recommended granularity), a virtual range reserved with the asked
// alignment, mapped and made accessible: VA alignment is then ours to choose, the physical side is whatever the
// driver's allocator gives a request of that size.
static int relocate_impl(spmv_csr_dev *m, int which, unsigned long long align, unsigned long long offset, int vmm) {
    if (need_device()) return -1;
    if (!m || which < 0 || which > 7) return fail("csr_relocate: bad arguments");
    if (align < 256 || (align & (align - 1)) || (offset & 255) || offset >= align)
        return fail("csr_relocate: align must be a power of two >= 256, offset a multiple of 256 below it");
    void **fields[8] = {(void **)&m->row_ptr, (void **)&m->col, &m->val, &m->x, &m->y, (void **)&m->xw.slot,
                        (void **)&m->xw.lines, (void **)&m->xw.ldesc4};
    void **field = fields[which];
    if (!*field) return 0;  // the handle has no such array
    HIP_TRY(hipStreamSynchronize(g_stream));
    size_t size = 0;
    size_t at = m->relocs.size();
    for (size_t k = 0; k < m->relocs.size(); ++k)
        if (m->relocs[k].field == field) at = k;
    if (at < m->relocs.size()) size = m->relocs[at].size;
    else HIP_TRY(hipMemPtrGetInfo(*field, &size));
    spmv_csr_dev::relocated fresh;
    fresh.field = field;
    fresh.size = size;
    char *p = nullptr;
    if (!vmm) {
        HIP_TRY(hipMalloc(&fresh.raw, size + align + offset));
        p = (char *)(((uintptr_t)fresh.raw + align - 1) & ~(uintptr_t)(align - 1)) + offset;
    } else {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = g_device;
        size_t gran = 0;
        HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
        if (gran == 0) gran = 2u << 20;
        fresh.vmm = true;
        fresh.mapped = (size + offset + gran - 1) / gran * gran;
        HIP_TRY(hipMemCreate(&fresh.phys, fresh.mapped, &prop, 0));
        hipError_t e = hipMemAddressReserve(&fresh.raw, fresh.mapped, align, nullptr, 0);
        if (e == hipSuccess) {
            e = hipMemMap(fresh.raw, fresh.mapped, 0, fresh.phys, 0);
            if (e == hipSuccess) {
                hipMemAccessDesc acc = {};
                acc.location = prop.location;
                acc.flags = hipMemAccessFlagsProtReadWrite;
                e = hipMemSetAccess(fresh.raw, fresh.mapped, &acc, 1);
                if (e != hipSuccess) (void)hipMemUnmap(fresh.raw, fresh.mapped);
            }
            if (e != hipSuccess) (void)hipMemAddressFree(fresh.raw, fresh.mapped);
        }
        if (e != hipSuccess) {
            (void)hipMemRelease(fresh.phys);
            return fail("csr_relocate: virtual-memory allocation failed: %s", hipGetErrorString(e));
        }
        if ((uintptr_t)fresh.raw & (align - 1)) {
            release_relocated(fresh);
            return fail("csr_relocate: the reserved range is not aligned to %llu", align);
        }
        p = (char *)fresh.raw + offset;
    }
    hipError_t e = hipMemcpy(p, *field, size, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        release_relocated(fresh);
        return fail("csr_relocate: copy failed: %s", hipGetErrorString(e));
    }
    if (at < m->relocs.size()) release_relocated(m->relocs[at]);
    else (void)hipFree(*field);
    *field = p;
    if (at < m->relocs.size()) m->relocs[at] = fresh;
    else m->relocs.push_back(fresh);
    return 0;
}

extern "C" int spmv_hip_csr_relocate(spmv_csr_dev *m, int which, unsigned long long align, unsigned long long offset) {
    return guarded("csr_relocate", [&] { return relocate_impl(m, which, align, offset, 0); });
}
extern "C" int spmv_hip_csr_relocate_vmm(spmv_csr_dev *m, int which, unsigned long long align, unsigned long long offset) {
    return guarded("csr_relocate_vmm", [&] { return relocate_impl(m, which, align, offset, 1); });
}

// Measurement only: one launch of the x-window kernel's STAMP instantiation (same code + three stores per workgroup)
// behind `warm` ordinary launches; stamps[3 * b] = {start, end (ticks of the constant 100 MHz clock), dispatch id << 8 |
// XCD} of block b.  Shows WHERE a slow launch loses its time: every block a little, or one XCD's share as a tail.
extern "C" int spmv_hip_csr_stamp_blocks(spmv_csr_dev *m, int warm, unsigned long long *stamps_host) {
    if (need_device()) return -1;
    if (!m || !stamps_host) return fail("csr_stamp_blocks: NULL argument");
    const XWindowPlan<int2> &p = m->xw;
    if (p.blocks <= 0 || m->value_bytes != 8 || m->local_cap != 2048)
        return fail("csr_stamp_blocks: needs an fp64 handle with an x-window plan at the 2048-entry stage");
    unsigned long long *d = nullptr;
    const size_t bytes = (size_t)p.blocks * 3 * sizeof(unsigned long long);
    HIP_TRY(hipMalloc((void **)&d, bytes));
    int rc = 0;
    // (warm >= 1000, measurement only: the stamped launch does not read the slot stream -- the time the kernel would take
    // if the slots came from a per-block pattern; y is then wrong)
    // (warm >= 2000, i.e. probe & 2: the second word of every stamp is the time the block's records were back -- the end
    // of its head -- instead of its end; y stays right)
    const int probe = warm / 1000 & 3;
    warm %= 1000;
    for (int i = 0; i < warm && !rc; ++i) rc = csr_launch_any(m, SPMV_CSR_STREAM, m->x, m->y, g_stream);
    if (!rc) {
        const XWindowLaunch L = p.launch_shape(p.blocks, m->local_cap, 8, m->nz);
        double *y = (double *)m->y + m->row0;
        with_flag(L.nt, [&](auto nt) {
            hipLaunchKernelGGL((csr_stream_local<double, decltype(nt)::value, 2048, true>), dim3(L.grid), dim3(kBlock), L.lds, g_stream,
                               p.blocks, L.chunk, (const int *)nullptr, p.ldesc4, p.ldesc, p.lines, m->row_ptr, p.slot,
                               (const double *)m->val, (const double *)m->x, y, d, probe, (const int2 *)nullptr,
                               (const unsigned *)nullptr, (const unsigned short *)nullptr, 0, (const int2 *)nullptr,
                               (const uint4 *)nullptr, p.lbase, p.lbase ? kXwShared : 0);
        });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e == hipSuccess) e = hipMemcpy(stamps_host, d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail("csr_stamp_blocks: %s", hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

// Digest of every array of the handle's tile plans (tests: a plan built on the device against one built on the host):
// out[2 k] = elements, out[2 k + 1] = FNV-1a of the bytes of array k, in the order tcol, tkey, tval, pass descriptors
// (stream order), stream_pass, block_row, stream_block, sblock_rows, rem_row, rem_ptr, rem_col, rem_val, then the long
// rows' plan: tcol, tkey, tval, pass, block_row, block_pass, work, item_first, row_map, block_of_row, and the same ten
// for the middle tier: the tiers' own lists (arrays(), spmv_internal.hpp) without what they mark as scratch.  32 arrays.
int csr_tile_digest(const spmv_csr_dev *m, unsigned long long *out) {
    if (need_device()) return -1;
    if (!m || !out) return fail("csr_tile_digest: NULL argument");
    HIP_TRY(hipStreamSynchronize(g_stream));
    const size_t vb = (size_t)m->value_bytes;
    std::vector<TileArr> arrs;
    for (const std::vector<TileArr> &tier : {m->tile.arrays(vb), m->lt.arrays(vb), m->mt.arrays(vb)})
        for (const TileArr &a : tier)
            if (a.elem) arrs.push_back(a);
    if (arrs.size() * 2 != 64) return fail("csr_tile_digest: %zu arrays do not fill the 64-word digest", arrs.size());
    std::vector<unsigned char> buf;
    for (size_t k = 0; k < arrs.size(); ++k) {
        const size_t bytes = arrs[k].p ? arrs[k].count * arrs[k].elem : 0;
        unsigned long long h = 1469598103934665603ull;
        if (bytes) {
            buf.resize(bytes);
            HIP_TRY(hipMemcpy(buf.data(), arrs[k].p, bytes, hipMemcpyDeviceToHost));
            // eight interleaved lanes of FNV-1a (one serial chain would take seconds per GB), folded at the end
            unsigned long long lane[8];
            for (int j = 0; j < 8; ++j) lane[j] = 1469598103934665603ull + (unsigned long long)j;
            size_t i = 0;
            for (; i + 8 <= bytes; i += 8)
                for (int j = 0; j < 8; ++j) lane[j] = (lane[j] ^ buf[i + j]) * 1099511628211ull;
            for (; i < bytes; ++i) lane[0] = (lane[0] ^ buf[i]) * 1099511628211ull;
            for (int j = 0; j < 8; ++j) h = (h ^ lane[j]) * 1099511628211ull;
        }
        out[2 * k] = arrs[k].p ? arrs[k].count : 0;
        out[2 * k + 1] = h;
    }
    return 0;
}

extern "C" int spmv_hip_csr_tile_digest(const spmv_csr_dev *m, unsigned long long *out) {
    return guarded("csr_tile_digest", [&] { return csr_tile_digest(m, out); });
}

extern "C" int spmv_hip_csr_addresses(const spmv_csr_dev *m, unsigned long long *out) {
    if (!m || !out) return fail("csr_addresses: NULL argument");
    const void *p[8] = {m->row_ptr, m->col, m->val, m->x, m->y, m->xw.slot, m->xw.lines, m->xw.ldesc4};
    for (int i = 0; i < 8; ++i) out[i] = (unsigned long long)(uintptr_t)p[i];
    return 0;
}

extern "C" int spmv_hip_csr_info(const spmv_csr_dev *m, spmv_dev_info *out) {
    if (!m || !out) return fail("csr_info: NULL argument");
    memset(out, 0, sizeof *out);
    out->M_local = m->M_local;
    out->M_total = m->M_total;
    out->N = m->N;
    out->row0 = m->row0;
    out->nz = m->nz;
    out->value_bytes = m->value_bytes;
    out->auto_variant = m->auto_variant;
    out->lanes_per_row = m->lanes_per_row;
    out->stream_blocks = m->num_blocks;
    out->long_rows = m->num_long;
    const long long vb = m->value_bytes;
    // nnz (val + 4) + 4 (M + 1) + val M [y] + val N [x]
    out->algo_bytes = m->nz * (vb + 4) + 4LL * (m->M_local + 1) + vb * m->M_local + vb * m->N;
    out->device_bytes = (long long)csr_device_bytes(m);
    const XWindowPlan<int2> &p = m->xw;
    const PatternPlan &pat = p.pat;
    out->local_blocks = p.blocks;
    out->local_stage_lines = p.stage_lines;
    out->local_lines = p.lines_listed;
    const OwnTiles &t = m->tile;
    out->tile_blocks = t.blocks;
    out->tile_passes = t.passes;
    out->tile_entries = t.entries + t.rem_entries;
    out->tile_remainder_entries = t.rem_entries;
    out->tile_staged_entries = t.staged;
    out->tile_split_rows = t.num_long;
    out->tile_long_rows = m->lt.rows;
    out->tile_long_entries = m->lt.entries;
    out->tile_staged_cols = t.staged_cols + m->lt.staged_cols + m->mt.staged_cols;
    out->tile_long_items = m->lt.items;
    out->tile_mid_rows = m->mt.rows;
    out->tile_mid_entries = m->mt.entries;
    out->tile_mid_items = m->mt.items;
    out->place_tries = m->place_tries;
    out->place_first_us = m->place_first_us;
    out->place_best_us = m->place_best_us;
    out->val_address = (unsigned long long)(uintptr_t)m->val;
    out->tile_expanded_entries = t.xe && t.expansion ? (long long)t.expansion->entries : 0;
    out->pattern_slots = pat.ptab ? pat.slots : 0;
    out->pattern_with_us = pat.with_us;
    out->pattern_without_us = pat.without_us;
    out->pattern_segment_max = pat.ptab ? 16 * pat.seg_max : 0;
    out->pattern_segment_cap = 16 * pat.seg_cap;
    out->pattern_table_rows = pat.ptab ? pat.table_rows : 0;
    out->pattern_segments_stored = pat.ptab && pat.pseg ? pat.seg_distinct : 0;
    out->local_lists_stored = p.lists_stored;
    out->local_lines_stored = p.lines_stored;
    out->stream_kernel = p.blocks > 0 ? 1 : t.blocks > 0 ? 3 : csr_short_rows(m) ? 2 : 0;
    if (p.blocks > 0)  // (a pattern plan: the tables and 4 bytes per row instead of 2 bytes per entry)
        // (a pattern plan: the segments instead of the slots; a block whose segment did not fit reads its table, rinfo
        // and row_ptr -- counted as its share of the tables)
        out->stream_bytes = m->nz * vb + (pat.ptab ? 16 * pat.seg_total + 8LL * p.blocks +
                                                         (2 * pat.slots + 8LL * m->M_local) * pat.table_rows / std::max(1, m->M_local)
                                                   : 2 * m->nz + 4LL * (m->M_local + 1)) +
                            4 * p.lines_stored + (p.lbase ? 4LL * p.blocks : 0) + 24LL * p.blocks + vb * m->M_local + vb * m->N;
    else if (t.blocks > 0) {  // tiles: 4-byte column + 2-byte key + value per (padded) entry; rows beyond the limit as CSR
        // a tier's entries and descriptors
        auto tier_bytes = [vb](const TileTier &tier) { return tier.padded * (vb + 6) - (tier.packed ? 2 : 0) * tier.staged + 16LL * tier.passes; };
        out->stream_bytes = tier_bytes(t) + 4LL * t.blocks +
                            std::max<long long>(0, m->nz - t.entries - t.rem_entries - m->lt.entries - m->mt.entries) * (vb + 4) +
                            t.rem_entries * (vb + 4) + 16LL * t.num_pieces + vb * m->M_local + vb * m->N;
        // an expanded plan: tile_expand reads 2 bytes per entry (+ 4 per run and per 64 entries) and writes its x value,
        // csr_tile reads that value as its window and a packed column word where it read column and key; every chunk
        // copies its 32 KiB slice of x (out of L2 mostly)
        if (t.xe && t.expansion)
            out->stream_bytes += (long long)t.expansion->entries * (2 * vb) + 24LL * t.expansion->chunks +
                                 4LL * (long long)(t.expansion->runs + t.expansion->groups);
        for (const CompactTiles *tier : {&m->lt, &m->mt})  // ... slabs written and read
            out->stream_bytes += tier_bytes(*tier) + 2 * vb * (long long)tier->items * tier->rows_per_block;
    }
    return 0;
}

extern "C" int spmv_hip_csr_set_x(spmv_csr_dev *m, const void *x_host) {
    if (need_device()) return -1;
    if (!m || !x_host) return fail("csr_set_x: NULL argument");
    HIP_TRY(hipMemcpyAsync(m->x, x_host, (size_t)m->N * m->value_bytes, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int spmv_hip_csr_get_y(spmv_csr_dev *m, void *y_host) {
    if (need_device()) return -1;
    if (!m || !y_host) return fail("csr_get_y: NULL argument");
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(y_host, m->y, (size_t)m->M_total * m->value_bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void *spmv_hip_csr_x_ptr(spmv_csr_dev *m) { return m ? m->x : nullptr; }
extern "C" void *spmv_hip_csr_y_ptr(spmv_csr_dev *m) { return m ? m->y : nullptr; }

// ----------------------------------------------------------- CSR: launch
namespace {

template <typename T, int L>
void launch_vector(const spmv_csr_dev *m, const T *x, T *y, hipStream_t s) {
    constexpr int rows = kBlock / L;
    const int grid = (m->M_local + rows - 1) / rows;
    hipLaunchKernelGGL((csr_vector<T, L, 1, false>), dim3(grid), dim3(kBlock), 0, s, m->M_local,
                       m->row_ptr, m->col, (const T *)m->val, x, y);
}

// the split-row pair: 8192-entry pieces into `partial`, then every row's slots added in slot order
template <typename T>
void launch_split_rows(const spmv_csr_dev *m, int num_pieces, const int4 *pieces, int num_rows, const int4 *rows,
                       const T *x, T *y, hipStream_t s) {
    hipLaunchKernelGGL((csr_long_pieces<T, true>), dim3(num_pieces), dim3(kBlock), 0, s, num_pieces, pieces, m->col,
                       (const T *)m->val, x, (T *)m->partial);
    hipLaunchKernelGGL((csr_long_finish<T>), dim3(num_rows), dim3(64), 0, s, num_rows, rows, (const T *)m->partial, y);
}

// the x-window kernel over all blocks (part < 0) or the interior / boundary sub-list (part 0 / 1, csr_launch_part)
template <typename T>
void launch_x_window(const spmv_csr_dev *m, const T *x, T *y, hipStream_t s, int part) {
    const XWindowPlan<int2> &p = m->xw;
    const PatternPlan &pat = p.pat;
    const int lcount = part < 0 ? p.blocks : part == 0 ? m->num_interior : m->num_boundary;
    const int *lids = part < 0 ? nullptr : part == 0 ? m->interior_ids : m->boundary_ids;
    if (lcount <= 0) return;
    const XWindowLaunch L = p.launch_shape(lcount, m->local_cap, (int)sizeof(T), m->nz);
    // what the plan has is said here, in `shape` (the kernel tests no pointer and runs the body compiled for that
    // shape): shared line lists, and -- a pattern plan -- segments (sdesc and pseg are allocated together)
    const int shape = (p.lbase ? kXwShared : 0) | (L.patterns && pat.sdesc && pat.pseg ? kXwSegs : 0);
    with_value<1024, 3072, 2048>(m->local_cap, [&](auto cap) {
        with_flag(L.nt, [&](auto nt) {
            constexpr int CAP = decltype(cap)::value;
            constexpr bool NT = decltype(nt)::value;
            if (L.patterns)
                hipLaunchKernelGGL((csr_stream_local<T, NT, CAP, false, true>), dim3(L.grid), dim3(kBlock), L.pat_lds, s, lcount, L.chunk,
                                   lids, p.ldesc4, p.ldesc, p.lines, m->row_ptr, p.slot, (const T *)m->val, x, y,
                                   (unsigned long long *)nullptr, 0, pat.pdesc, pat.rinfo, pat.ptab, (int)L.lds, pat.sdesc,
                                   (const uint4 *)pat.pseg, p.lbase, shape);
            else
                hipLaunchKernelGGL((csr_stream_local<T, NT, CAP>), dim3(L.grid), dim3(kBlock), L.lds, s, lcount, L.chunk, lids,
                                   p.ldesc4, p.ldesc, p.lines, m->row_ptr, p.slot, (const T *)m->val, x, y,
                                   (unsigned long long *)nullptr, 0, (const int2 *)nullptr, (const unsigned *)nullptr,
                                   (const unsigned short *)nullptr, 0, (const int2 *)nullptr, (const uint4 *)nullptr, p.lbase, shape);
        });
    });
}

// what one csr_tile launch is given: filled for the handle's tiles, for their expansion and for each compacted tier
template <typename T>
struct tile_args {
    int items, rows_per_block, stage_ok;  // workgroups' work (streams | work items), accumulators per block
    size_t lds;
    const int4 *work;  // compacted tiers only: the work items and their slabs
    T *slab;
    const int *block_row, *block_pass;
    const int4 *pass;
    const int *tcol;
    const unsigned short *tkey;
    const T *tval;
    const int *stream_block;  // the handle's own tiles only: the streams' blocks
    const int2 *sblock_rows;
    const T *x;
};

// (more than 64 KiB of dynamic LDS: allowed for these kernels once, at upload -- tile_allow_lds)
template <typename T, int TRIPS, bool PACK, bool GA = false>
void launch_csr_tile(const tile_args<T> &a, bool nt, T *y, hipStream_t s) {
    with_flag(nt, [&](auto NT) {
        hipLaunchKernelGGL((csr_tile<T, decltype(NT)::value, 2048, TRIPS, PACK, GA>), dim3((a.items + 7) / 8 * 8), dim3(kTileBlock),
                           a.lds, s, a.items, a.rows_per_block, a.stage_ok, g_tile_probe, a.work, a.slab, a.block_row, a.block_pass,
                           a.pass, a.tcol, a.tkey, a.tval, a.stream_block, a.sblock_rows, a.x, y);
    });
}

// the LDS of one csr_tile workgroup over a tier: slots, accumulators, and the staged window (the packed kernel stores every
// trip's piece; a plan with gather passes stages its widest window when x can be staged at all)
template <typename T>
size_t tile_lds(const TileTier &t, int stage_ok) {
    return (size_t)kTileSlotBytes + (size_t)t.rows_per_block * sizeof(T) +
           (t.packed ? (size_t)kTileTrips * kTileTripBytes : stage_ok ? (size_t)t.max_win * sizeof(T) : 0);
}

// what every tier gives a launch; items / work / slab / streams are the caller's
template <typename T>
tile_args<T> tile_args_of(const TileTier &t, int items, int stage_ok, size_t lds, const T *x) {
    return {items, t.rows_per_block, stage_ok, lds, nullptr, nullptr, t.block_row, t.block_pass, t.pass, t.tcol, t.tkey, (const T *)t.tval,
            nullptr, nullptr, x};
}

// the tile plan: (expansion of x,) the tiles, the packed plan's remainder, the long and middle tiers, the split rows
template <typename T>
void launch_tiles(const spmv_csr_dev *m, const T *x, T *y, hipStream_t s) {
    const OwnTiles &t = m->tile;
    // staging copies 16-byte pieces of x: plans with gather passes fall back on gathering everything when
    // x is not 16-byte aligned, packed plans (no gather code) load the pieces unaligned
    const int stage_ok = ((uintptr_t)x & 15) == 0;
    // (probe bit 3, measurement only: one workgroup per CU)
    const size_t lds = std::max((size_t)std::max(t.lds_min, g_tile_probe & 8 ? 84 * 1024 : 0), tile_lds<T>(t, stage_ok));
    const bool tnt = m->nz * (long long)(sizeof(T) + 6) > (128LL << 20);
    tile_args<T> own = tile_args_of<T>(t, t.streams, stage_ok, lds, x);
    own.stream_block = t.stream_block;
    own.sblock_rows = t.sblock_rows;
    // an expanded plan: x into the passes' segments first, then the packed kernel over x' (16-byte pieces of
    // x: aligned x only)
    const bool expanded = t.xe && t.expansion && t.expansion->chunks > 0 && stage_ok && g_tile_expand != 0;
    if (expanded) {
        hipLaunchKernelGGL((tile_expand<T>), dim3(t.expansion->chunks), dim3(kExpandBlock), 0, s, m->N, g_tile_probe,
                           t.expansion->chunk, t.expansion->chunk_runs, t.expansion->lcol, t.expansion->group_run, t.expansion->delta, x, (T *)t.xe);
        // (a pass's window is its own segment: 2048 values at most, one staging trip in fp32, two in fp64)
        constexpr int kXpTrips = 2048 * (int)sizeof(T) / kTileTripBytes;
        tile_args<T> xp = own;
        xp.stage_ok = 1;
        xp.lds = std::max((size_t)t.lds_min, (size_t)kTileSlotBytes + (size_t)t.rows_per_block * sizeof(T) +
                                                 (size_t)kXpTrips * kTileTripBytes);
        xp.pass = t.expansion->pass;
        xp.tcol = t.expansion->words;
        xp.tkey = nullptr;
        xp.x = (const T *)t.xe;
        launch_csr_tile<T, kXpTrips, true>(xp, tnt, y, s);
    }
    else if (t.packed) launch_csr_tile<T, kTileTrips, true>(own, tnt, y, s);
    else if (g_tile_gather_ahead) launch_csr_tile<T, kTileTrips, false, true>(own, tnt, y, s);  // gathers one pass early
    else launch_csr_tile<T, kTileTrips, false>(own, tnt, y, s);
    if (t.rem_rows > 0)  // what the packed plan left out: added behind the tiles
        hipLaunchKernelGGL((tile_remainder<T>), dim3((t.rem_rows + 255) / 256), dim3(256), 0, s, t.rem_rows,
                           t.rem_row, t.rem_ptr, t.rem_col, (const T *)t.rem_val, x, y);
    // the compacted tiers -- the long rows' own tiles, the middle tier of a scattered matrix: work items ->
    // slabs -> y (after the ordinary tiles wrote 0 there)
    for (const CompactTiles *tier : {&m->lt, &m->mt}) {
        const CompactTiles &L = *tier;
        if (L.items <= 0) continue;
        tile_args<T> la = tile_args_of<T>(L, L.items, stage_ok, tile_lds<T>(L, stage_ok), x);
        la.work = L.work;
        la.slab = (T *)L.slab;
        if (L.packed) launch_csr_tile<T, kTileTrips, true>(la, tnt, y, s);
        else launch_csr_tile<T, kTileTrips, false>(la, tnt, y, s);
        hipLaunchKernelGGL((tile_slab_finish<T>), dim3((L.rows + kFinishRows - 1) / kFinishRows),
                           dim3(kFinishRows * kFinishGroups), 0, s, L.rows,
                           L.rows_per_block, L.block_row, L.block_of_row, L.item_first, L.row_map,
                           (const T *)L.slab, y);
    }
    if (t.num_long)  // rows beyond the tile limit: stripe-ordered pieces, slots added row by row
        launch_split_rows<T>(m, t.num_pieces, t.pieces, t.num_long, t.long_rows, x, y, s);
}

// the gather stream: csr_stream at the handle's stage and the knob's block size, csr_stream_short for short rows
template <typename T>
void launch_gather_stream(const spmv_csr_dev *m, const T *x, T *y, hipStream_t s) {
    // blocks per XCD run; the grid is rounded up to whole runs (a workgroup past the last block returns at once)
    const int chunk = g_stream_xcd < 0 ? (m->num_blocks + 7) / 8 : g_stream_xcd;
    const int grid_blocks = chunk > 0 ? (m->num_blocks + 8 * chunk - 1) / (8 * chunk) * (8 * chunk)
                                      : m->num_blocks;
    const int cap = m->stream_cap, blk = g_stream_block;
    // (the (stage, block) pairs named below are the instantiations there are)
    auto full = [&](auto cap_c, auto block_c) {
        constexpr int CAP = decltype(cap_c)::value, BLOCK = decltype(block_c)::value;
        with_flag(g_stream_nt, [&](auto nt) {
            hipLaunchKernelGGL((csr_stream<T, decltype(nt)::value, CAP, BLOCK>), dim3(grid_blocks), dim3(BLOCK), 0, s,
                               m->num_blocks, chunk, m->desc, m->row_ptr, m->col, (const T *)m->val, x, y);
        });
    };
    // short rows: blocks of up to 1024 rows, row extents of all passes loaded up front
    auto brief = [&](auto cap_c) {
        with_flag(g_stream_nt, [&](auto nt) {
            hipLaunchKernelGGL((csr_stream_short<T, decltype(nt)::value, decltype(cap_c)::value, 256>), dim3(grid_blocks), dim3(256), 0, s,
                               m->num_blocks, chunk, m->desc, m->row_ptr, m->col, (const T *)m->val, x, y);
        });
    };
    const bool short_rows = csr_short_rows(m);
    if (cap == 1024) full(int_c<1024>, int_c<256>);
    else if (cap == 3072) full(int_c<3072>, int_c<256>);
    else if (cap == 2048 && short_rows) brief(int_c<2048>);
    else if (cap == 2048) full(int_c<2048>, int_c<256>);
    else if (cap == 4096 && blk == 512) full(int_c<4096>, int_c<512>);
    else if (cap == 4096 && short_rows) brief(int_c<4096>);
    else if (cap == 4096) full(int_c<4096>, int_c<256>);
    else if (blk == 1024) full(int_c<8192>, int_c<1024>);
    else full(int_c<8192>, int_c<512>);
}

template <typename T>
int csr_launch(const spmv_csr_dev *m, int variant, const T *x, T *y_full, hipStream_t s, int part = -1) {
    if (m->M_local == 0) return 0;
    T *y = y_full + m->row0;
    if (variant == SPMV_CSR_AUTO) variant = m->auto_variant;
    if (m->tiles_only && variant != SPMV_CSR_STREAM) return fail("csr_launch: a tiles-only handle runs the tile kernel only");
    switch (variant) {
        case SPMV_CSR_THREAD_ROW: {
            const int grid = (m->M_local + kBlock - 1) / kBlock;
            hipLaunchKernelGGL((csr_thread_row<T>), dim3(grid), dim3(kBlock), 0, s, m->M_local,
                               m->row_ptr, m->col, (const T *)m->val, x, y);
            break;
        }
        case SPMV_CSR_WAVE_ROW: {
            constexpr int rows = kBlock / 64;
            const int grid = (m->M_local + rows - 1) / rows;
            hipLaunchKernelGGL((csr_vector<T, 64, 2, true>), dim3(grid), dim3(kBlock), 0, s,
                               m->M_local, m->row_ptr, m->col, (const T *)m->val, x, y);
            break;
        }
        case SPMV_CSR_SUBWAVE:
            switch (m->lanes_per_row) {
                case 2: launch_vector<T, 2>(m, x, y, s); break;
                case 4: launch_vector<T, 4>(m, x, y, s); break;
                case 8: launch_vector<T, 8>(m, x, y, s); break;
                case 16: launch_vector<T, 16>(m, x, y, s); break;
                default: launch_vector<T, 32>(m, x, y, s); break;
            }
            break;
        case SPMV_CSR_STREAM:
            if (m->num_blocks > 0 || m->tiles_only) {
                switch (csr_stream_route(m, x, part)) {
                    case stream_route::nothing_else: return fail("csr_launch: a tiles-only handle has nothing else to run");
                    // (other handles take such an x to the gather kernels)
                    case stream_route::unaligned_x: return fail("csr_launch: a packed tile plan needs a 16-byte aligned x");
                    case stream_route::tiles:  // (its own split rows included)
                        launch_tiles<T>(m, x, y, s);
                        HIP_TRY(hipGetLastError());
                        return 0;
                    case stream_route::x_window: launch_x_window<T>(m, x, y, s, part); break;
                    case stream_route::gather: launch_gather_stream<T>(m, x, y, s); break;
                }
            }
            if (m->num_long && part != 0) launch_split_rows<T>(m, m->num_partial, m->pieces, m->num_long, m->long_rows, x, y, s);
            break;
        default:
            return fail("unknown CSR variant %d", variant);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int csr_launch_any(const spmv_csr_dev *m, int variant, const void *x, void *y, hipStream_t s) {
    if (m->value_bytes == 8) return csr_launch<double>(m, variant, (const double *)x, (double *)y, s);
    return csr_launch<float>(m, variant, (const float *)x, (float *)y, s);
}

// N4 overlap: the interior x-window blocks (part 0: rows whose x lines all lie in the handle's own range, so
// they can run while the halo of x is still travelling) / everything else (part 1).  Together = one
// csr_launch_any(STREAM): the same kernels on the same blocks, hence the same bits.  A handle without the
// split (no x-window plan, foreign misaligned x) runs everything as part 1.
int csr_launch_part(const spmv_csr_dev *m, int part, const void *x, void *y, hipStream_t s) {
    const bool split_ok = csr_stream_route(m, x, part) == stream_route::x_window;
    if (!split_ok) return part == 0 ? 0 : csr_launch_any(m, SPMV_CSR_STREAM, x, y, s);
    if (m->value_bytes == 8) return csr_launch<double>(m, SPMV_CSR_STREAM, (const double *)x, (double *)y, s, part);
    return csr_launch<float>(m, SPMV_CSR_STREAM, (const float *)x, (float *)y, s, part);
}

// The handle's line lists on the host, whichever way they are stored: ld[b] = {first id in `lines`, ids}, base[b] = what
// block b adds to its ids (0 where the lists hold absolute ids).
int csr_lines_to_host(const spmv_csr_dev *m, std::vector<int2> &ld, std::vector<int> &lines, std::vector<int> &base) {
    const XWindowPlan<int2> &p = m->xw;
    const size_t B = (size_t)p.blocks;
    ld.resize(B);
    base.assign(B, 0);
    lines.resize((size_t)p.lines_stored);
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (B) HIP_TRY(hipMemcpy(ld.data(), p.ldesc, B * sizeof(int2), hipMemcpyDeviceToHost));
    if (B && p.lbase) HIP_TRY(hipMemcpy(base.data(), p.lbase, B * sizeof(int), hipMemcpyDeviceToHost));
    if (!lines.empty()) HIP_TRY(hipMemcpy(lines.data(), p.lines, lines.size() * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// Which x-window blocks of the handle are interior: every x line they list lies inside the handle's own rows'
// range of x (square matrix, x owned like y: entries [row0, row0 + M_local)).  Computed from the plan's line
// lists (ascending inside a block: first and last line decide).  counts (optional, 4 values): interior blocks,
// boundary blocks, entries in interior blocks, entries in boundary blocks + split rows.
static int csr_split_interior_body(spmv_csr_dev *m, long long *counts) {
    if (need_device()) return -1;
    if (!m) return fail("csr_split_interior: NULL handle");
    if (m->M_total != m->N) return fail("csr_split_interior: needs a square matrix (%d x %d)", m->M_total, m->N);
    (void)hipFree(m->interior_ids);
    (void)hipFree(m->boundary_ids);
    m->interior_ids = m->boundary_ids = nullptr;
    m->num_interior = m->num_boundary = 0;
    m->have_split = false;
    long long e_in = 0, e_out = m->nz;
    if (m->xw.blocks > 0) {
        const int B = m->xw.blocks;
        std::vector<int2> ld;
        std::vector<int4> d4((size_t)B);
        std::vector<int> lines, lbase;
        if (csr_lines_to_host(m, ld, lines, lbase)) return -1;
        HIP_TRY(hipMemcpy(d4.data(), m->xw.ldesc4, d4.size() * sizeof(int4), hipMemcpyDeviceToHost));
        const int per_line = kLineBytes / m->value_bytes;
        const long long own_lo = m->row0, own_hi = (long long)m->row0 + m->M_local;  // [lo, hi) of x
        std::vector<int> in_ids, out_ids;
        for (int b = 0; b < B; ++b) {
            const long long first = ((long long)lines[(size_t)ld[b].x] + lbase[b]) * per_line;
            const long long last = ((long long)lines[(size_t)ld[b].x + ld[b].y - 1] + lbase[b] + 1) * per_line;  // exclusive
            // (a block of empty rows lists line 0 only to have something to stage: it reads nothing)
            const bool empty = d4[b].w == d4[b].y;
            if (empty || (first >= own_lo && std::min<long long>(last, m->N) <= own_hi)) {
                in_ids.push_back(b);
                e_in += d4[b].w - d4[b].y;
            } else {
                out_ids.push_back(b);
            }
        }
        e_out = m->nz - e_in;
        if (upload_array(&m->interior_ids, in_ids.data(), in_ids.size(), 1)) return -1;
        if (upload_array(&m->boundary_ids, out_ids.data(), out_ids.size(), 1)) return -1;
        m->num_interior = (int)in_ids.size();
        m->num_boundary = (int)out_ids.size();
        m->have_split = true;
    }
    if (counts) {
        counts[0] = m->num_interior;
        counts[1] = m->num_boundary;
        counts[2] = e_in;
        counts[3] = e_out;
    }
    return 0;
}

extern "C" int spmv_hip_csr_split_interior(spmv_csr_dev *m, long long *counts) {
    return guarded("csr_split_interior", [&] { return csr_split_interior_body(m, counts); });
}

// ---- N4 overlap below block granularity: the column split
namespace {

template <typename T>
__global__ __launch_bounds__(kBlock) void add_rows(long long n, const T *__restrict__ t, T *__restrict__ y) {
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += (long long)gridDim.x * kBlock) y[k] += t[k];
}

template <typename T>
int csr_split_columns_impl(spmv_csr_dev *m, int col_lo, int col_hi, long long *counts) {
    spmv_hip_csr_free(m->own_part);
    spmv_hip_csr_free(m->halo_part);
    m->own_part = m->halo_part = nullptr;
    m->own_entries = m->halo_entries = 0;
    const int Ml = m->M_local;
    const size_t nz = (size_t)m->nz;
    std::vector<int> rp((size_t)Ml + 1), col(nz);
    std::vector<T> val(nz);
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(rp.data(), m->row_ptr, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (nz) HIP_TRY(hipMemcpy(col.data(), m->col, nz * sizeof(int), hipMemcpyDeviceToHost));
    if (nz) HIP_TRY(hipMemcpy(val.data(), m->val, nz * sizeof(T), hipMemcpyDeviceToHost));
    // two CSR matrices over the same rows: entries keep their order inside a row
    std::vector<int> rp_own((size_t)m->M_total + 1, 0), rp_halo((size_t)m->M_total + 1, 0), c_own, c_halo;
    std::vector<T> v_own, v_halo;
    c_own.reserve(nz);
    v_own.reserve(nz);
    for (int r = 0; r < Ml; ++r) {
        for (int e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) {
            if (col[(size_t)e] >= col_lo && col[(size_t)e] < col_hi) {
                c_own.push_back(col[(size_t)e]);
                v_own.push_back(val[(size_t)e]);
            } else {
                c_halo.push_back(col[(size_t)e]);
                v_halo.push_back(val[(size_t)e]);
            }
        }
        rp_own[(size_t)m->row0 + r + 1] = (int)c_own.size();
        rp_halo[(size_t)m->row0 + r + 1] = (int)c_halo.size();
    }
    for (int r = m->row0 + Ml; r < m->M_total; ++r) {  // rows behind the handle's block: empty
        rp_own[(size_t)r + 1] = (int)c_own.size();
        rp_halo[(size_t)r + 1] = (int)c_halo.size();
    }
    m->own_entries = (long long)c_own.size();
    m->halo_entries = (long long)c_halo.size();
    if (counts) {
        counts[0] = m->own_entries;
        counts[1] = m->halo_entries;
    }
    if (c_halo.empty()) return 0;  // nothing comes from other ranks: the handle itself is the interior (same bits as ever)
    // (the sub-handles are ordinary handles: plans, block cuts, AUTO -- but no placement search of their own)
    const int keep = g_place_tries;
    g_place_tries = 0;
    int rc = csr_upload_impl<T>(m->M_total, m->N, rp_own.data(), m->row0, m->row0 + Ml, MatrixSource<T>::on_host(c_own.data(), v_own.data()), &m->own_part);
    if (!rc) rc = csr_upload_impl<T>(m->M_total, m->N, rp_halo.data(), m->row0, m->row0 + Ml, MatrixSource<T>::on_host(c_halo.data(), v_halo.data()), &m->halo_part);
    g_place_tries = keep;
    if (rc) {
        spmv_hip_csr_free(m->own_part);
        spmv_hip_csr_free(m->halo_part);
        m->own_part = m->halo_part = nullptr;
        return -1;
    }
    return 0;
}

}  // namespace

// Split the handle's entries by column: [col_lo, col_hi) = the rank's own range of x.  counts[2] (optional): entries
// whose column lies inside / outside.  Afterwards spmv_hip_csr_run_split(part 0) computes y = A_own x -- it reads
// nothing of x outside [col_lo, col_hi) -- and part 1 adds A_halo x; 0 then 1 = the handle's product up to the
// order in which a row's two partial sums are added.  A handle without outside entries keeps no sub-handles.
extern "C" int spmv_hip_csr_split_columns(spmv_csr_dev *m, int col_lo, int col_hi, long long *counts) {
    if (need_device()) return -1;
    if (!m || col_lo < 0 || col_hi < col_lo || col_hi > m->N) return fail("csr_split_columns: bad arguments");
    if (m->tiles_only || !m->col || !m->val) return fail("csr_split_columns: the handle does not hold its CSR arrays");
    return guarded("csr_split_columns", [&] {
        return m->value_bytes == 8 ? csr_split_columns_impl<double>(m, col_lo, col_hi, counts)
                                   : csr_split_columns_impl<float>(m, col_lo, col_hi, counts);
    });
}

int csr_launch_split(const spmv_csr_dev *m, int part, const void *x, void *y, hipStream_t s) {
    if (!m->own_part || !m->halo_part) {  // no split (nothing comes from outside): everything is part 0
        return part == 0 ? csr_launch_any(m, SPMV_CSR_AUTO, x, y, s) : 0;
    }
    if (part == 0) return csr_launch_any(m->own_part, SPMV_CSR_AUTO, x, y, s);
    // y_own += A_halo x: the product into the sub-handle's own y, then one pass over this rank's rows
    if (csr_launch_any(m->halo_part, SPMV_CSR_AUTO, x, m->halo_part->y, s)) return -1;
    const long long n = m->M_local;
    const int grid = (int)std::max<long long>(1, std::min<long long>(2048, (n + kBlock - 1) / kBlock));
    if (m->value_bytes == 8)
        hipLaunchKernelGGL((add_rows<double>), dim3(grid), dim3(kBlock), 0, s, n, (const double *)m->halo_part->y + m->row0, (double *)y + m->row0);
    else
        hipLaunchKernelGGL((add_rows<float>), dim3(grid), dim3(kBlock), 0, s, n, (const float *)m->halo_part->y + m->row0, (float *)y + m->row0);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int spmv_hip_csr_run_split(spmv_csr_dev *m, int part, const void *d_x, void *d_y, void *stream) {
    if (need_device()) return -1;
    if (!m || (part != 0 && part != 1)) return fail("csr_run_split: bad arguments");
    return csr_launch_split(m, part, d_x ? d_x : m->x, d_y ? d_y : m->y, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_csr_run_part(spmv_csr_dev *m, int part, const void *d_x, void *d_y, void *stream) {
    if (need_device()) return -1;
    if (!m || (part != 0 && part != 1)) return fail("csr_run_part: bad arguments");
    return csr_launch_part(m, part, d_x ? d_x : m->x, d_y ? d_y : m->y, stream ? (hipStream_t)stream : g_stream);
}



extern "C" int spmv_hip_csr_run(spmv_csr_dev *m, int variant) {
    if (need_device()) return -1;
    if (!m) return fail("csr_run: NULL handle");
    return csr_launch_any(m, variant, m->x, m->y, g_stream);
}

extern "C" int spmv_hip_csr_run_on(spmv_csr_dev *m, int variant, const void *d_x, void *d_y, void *stream) {
    if (need_device()) return -1;
    if (!m || !d_x || !d_y) return fail("csr_run_on: NULL argument");
    return csr_launch_any(m, variant, d_x, d_y, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_csr_time(spmv_csr_dev *m, int variant, int warmup, int iters, int zero_y,
                                 float *ms_each) {
    if (need_device()) return -1;
    if (!m) return fail("csr_time: NULL handle");
    return time_loop(
        warmup, iters, ms_each, [&] { return csr_launch_any(m, variant, m->x, m->y, g_stream); },
        [&]() -> int {
            if (zero_y) HIP_TRY(hipMemsetAsync(m->y, 0, (size_t)m->M_total * m->value_bytes, g_stream));
            return 0;
        });
}

extern "C" int spmv_hip_csr_time_graph(spmv_csr_dev *m, int variant, int iters, int replays, float *ms_per_iter) {
    if (need_device()) return -1;
    if (!m) return fail("csr_time_graph: NULL handle");
    return graph_loop(iters, replays, ms_per_iter, [&] { return csr_launch_any(m, variant, m->x, m->y, g_stream); });
}

