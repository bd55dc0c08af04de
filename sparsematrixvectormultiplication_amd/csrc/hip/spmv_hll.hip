// spmv_hll.hip -- HLL side of the C-ABI: the flat slab, its workgroup windows and x-window plan,
// the device builder from a resident CSR matrix, launchers, timing.  Replaces the per-hack
// allocations and launches of the reference's main_cuda.cu, lines 369-455, 545-568, 613-637 and 731-744.
#include "spmv_internal.hpp"

#include "launch_dispatch.hpp"
#include "upload_ops.hpp"

namespace {

// first pass of the device builder (see hll_fill_from_csr in hll_kernels.hpp): per-hack maximum row length
__global__ __launch_bounds__(kBlock) void hll_hack_maxnz(int M, int hacks, const int *__restrict__ row_ptr,
                                                         int *__restrict__ maxnz) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= hacks) return;
    const int r0 = h * kHack, r1 = min(r0 + kHack, M);
    int m = 0;
    for (int r = r0; r < r1; ++r) m = max(m, row_ptr[r + 1] - row_ptr[r]);
    maxnz[h] = m;
}

}  // namespace

// ----------------------------------------------------------------- HLL
namespace {

// Cut the rows of the flat slab into workgroup windows for hll_lds: consecutive rows whose
// slots, counted from the even slot at or below the first row's start, fit `cap` (at most
// kStreamRowsCap rows).  A row that alone does not fit gets a window of its own.  Returns
// the widest window (in slots, from its even base).
long long hll_build_blocks(int M, int hacks, const long long *off, const int *mz, int cap,
                           std::vector<int4> &desc) {
    desc.clear();
    (void)hacks;
    long long widest = 0;
    auto start_of = [&](int r) { return off[r / kHack] + (long long)(r % kHack) * mz[r / kHack]; };
    int r = 0;
    while (r < M) {
        const long long s0 = start_of(r);
        const long long base = s0 & ~1LL;
        int r1 = r + 1;  // the first row is always taken (even if it alone exceeds cap)
        int maxlen = mz[r / kHack];
        // (skew_cut: a window on the border between a hack of short rows and one of long rows -- see spmv_internal.hpp)
        while (r1 < M && r1 - r < kStreamRowsCap && start_of(r1) + mz[r1 / kHack] - base <= cap &&
               !skew_cut(r1 - r, maxlen, mz[r1 / kHack])) {
            maxlen = std::max(maxlen, mz[r1 / kHack]);
            ++r1;
        }
        const long long span = start_of(r1 - 1) + mz[(r1 - 1) / kHack] - base;
        if (r1 - r > 1 || span <= cap) widest = std::max(widest, span);
        desc.push_back(int4{r, r1 - r, (int)(s0 & 0xffffffffLL), (int)(s0 >> 32)});
        r = r1;
    }
    return widest;
}

}  // namespace

namespace {

// Windows for hll_lds_local: hll_build_blocks' cut at `cap` slots with the line limit on top
// (see csr_build_local).  ja is the flat host slab.  false: keep the gather kernel.
bool hll_build_local(int M, int N, const long long *off, const int *mz, const int *ja, long long slots_padded,
                     int cap, int lines_max, const std::vector<int4> &baseline, LocalPlan<int4> &plan) {
    constexpr int line_shift = 4;  // fp64: 16 per 128-byte line
    const int total_lines = (int)(((long long)N + 15) >> line_shift);
    std::vector<int> stamp((size_t)total_lines + 1, -1), rank((size_t)total_lines + 1, 0), cur;
    plan.lcol.assign((size_t)slots_padded + kPad, 0);
    plan.desc.clear();
    plan.ldesc.clear();
    plan.lines.clear();
    int widest = 0;
    auto start_of = [&](int r) { return off[r / kHack] + (long long)(r % kHack) * mz[r / kHack]; };
    int r = 0;
    while (r < M) {
        const long long s0 = start_of(r);
        const long long base = s0 & ~1LL;
        const int blk = (int)plan.desc.size();
        cur.clear();
        int r1 = r, maxlen = 0;
        while (r1 < M && r1 - r < kStreamRowsCap && start_of(r1) + mz[r1 / kHack] - base <= cap &&
               !skew_cut(r1 - r, maxlen, mz[r1 / kHack])) {
            const size_t before = cur.size();
            const long long a = start_of(r1);
            for (long long k = a; k < a + mz[r1 / kHack]; ++k) {
                const int l = ja[k] >> line_shift;
                if (stamp[l] != blk) {
                    stamp[l] = blk;
                    cur.push_back(l);
                }
            }
            if ((int)cur.size() > lines_max) {
                for (size_t k = before; k < cur.size(); ++k) stamp[cur[k]] = -1;
                cur.resize(before);
                break;
            }
            maxlen = std::max(maxlen, mz[r1 / kHack]);
            ++r1;
        }
        if (r1 == r) return false;  // a row that alone exceeds the stage or the line limit
        if (cur.empty()) cur.push_back(0);  // rows without slots: the kernel still stages one line
        std::sort(cur.begin(), cur.end());
        for (size_t k = 0; k < cur.size(); ++k) rank[cur[k]] = (int)k;
        for (long long k = s0; k < start_of(r1 - 1) + mz[(r1 - 1) / kHack]; ++k)
            plan.lcol[k] = (unsigned short)((rank[ja[k] >> line_shift] << line_shift) | (ja[k] & 15));
        plan.desc.push_back(int4{r, r1 - r, (int)(s0 & 0xffffffffLL), (int)(s0 >> 32)});
        plan.ldesc.push_back(int4{(int)plan.lines.size(), (int)cur.size(),
                                  (int)(start_of(r1 - 1) + mz[(r1 - 1) / kHack] - base), 0});
        plan.lines.insert(plan.lines.end(), cur.begin(), cur.end());
        widest = std::max(widest, (int)cur.size());
        r = r1;
        if ((plan.desc.size() & 1023) == 0) {
            const size_t plain = std::lower_bound(baseline.begin(), baseline.end(), r,
                                                  [](const int4 &d, int row) { return d.x < row; }) -
                                 baseline.begin();
            if (plan.desc.size() > plain + plain / 5 + 16) return false;
        }
    }
    if (plan.desc.size() > baseline.size() + baseline.size() / 5 + 1) return false;
    plan.stage_lines = std::max(kLocalLineQuantum,
                                (widest + kLocalLineQuantum - 1) / kLocalLineQuantum * kLocalLineQuantum);
    plan.lines.insert(plan.lines.end(), (size_t)kLocalLinesMax, 0);
    return true;
}

// offsets of the hacks in the flat slab: every hack starts on an even slot
long long hll_offsets(int total_rows, const std::vector<int> &mz, std::vector<long long> &off,
                      long long &true_slots) {
    const int H = (int)mz.size();
    off.assign((size_t)H + 1, 0);
    true_slots = 0;
    for (int h = 0; h < H; ++h) {
        const int rows = (h == H - 1) ? total_rows - h * kHack : kHack;
        const long long s = (long long)rows * mz[h];
        true_slots += s;
        off[h + 1] = off[h] + ((s + 1) & ~1LL);
    }
    return off[H];
}

// row_seg[r] = (first slot of row r relative to its window's even base) | (slots of the row << 16), for the
// rows of the x-window plan's windows: what hll_lds_local's row-sum phase needs, in one word.
__global__ __launch_bounds__(kBlock) void hll_row_segments(int num_blocks, const int4 *__restrict__ desc,
                                                           const long long *__restrict__ hack_off,
                                                           const int *__restrict__ maxnz,
                                                           unsigned *__restrict__ row_seg) {
    const int b = blockIdx.x;
    if (b >= num_blocks) return;
    const int4 d = desc[b];
    const long long base = (((long long)d.w << 32) | (unsigned)d.z) & ~1LL;
    for (int q = threadIdx.x; q < d.y; q += kBlock) {
        const int r = d.x + q, h = r / kHack;
        const int m = maxnz[h];
        const long long lo = hack_off[h] + (long long)(r % kHack) * m - base;
        row_seg[r] = (unsigned)lo | ((unsigned)m << 16);
    }
}

// row_seg for the rows of the x-window plan's windows (hack tables and window descriptors are on the device)
int hll_fill_row_segments(spmv_hll_dev *m) {
    XWindowPlan<int4> &p = m->xw;
    HIP_TRY(hipMalloc((void **)&p.row_seg, std::max<size_t>((size_t)m->M, 1) * sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(p.row_seg, 0, std::max<size_t>((size_t)m->M, 1) * sizeof(unsigned), g_stream));
    hipLaunchKernelGGL(hll_row_segments, dim3(p.blocks), dim3(kBlock), 0, g_stream, p.blocks, p.ldesc4, m->hack_off, m->maxnz,
                       p.row_seg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return 0;
}

// The pattern plan (tables only) and the searches of a finished handle (upload_ops.hpp).  The placement of AS where it is
// large and streamed by the slab's own kernels (csr_tile over the slab's rows streams its own re-ordered copy).
// (Ahead of hll_plan_on_device: the order in which this translation unit first names build_pattern_tables<true> and
// plan_on_device<4> is the order of their kernels in its code object.)
void hll_upload_searches(spmv_hll_dev *m) {
    (void)build_pattern_tables<true>(m->xw, m->M, m->slots, 8, nullptr);
    size_t bytes = 0;
    bool place = m->AS && (size_t)m->slots * sizeof(double) >= kPlaceMinBytes && (m->xw.blocks > 0 || !m->tiles);
    if (place && (hipMemPtrGetInfo(m->AS, &bytes) != hipSuccess || bytes < (size_t)m->slots * sizeof(double))) {
        (void)hipGetLastError();
        place = false;
    }
    upload_searches(m, place ? &m->AS : nullptr, bytes,
                    [m] { return hll_launch(m, SPMV_HLL_AUTO, m->x, m->y, g_stream); });
}

// x-window plan of a device-resident slab (upload_ops.hpp): the windows of hll_build_blocks at kPlanCap slots.  Returns 1
// when the handle now carries the plan, 0 when some window lists more than kLocalLinesMax lines (caller falls back to
// the host builder), -1 on a HIP error.
int hll_plan_on_device(spmv_hll_dev *m, int total_rows, const std::vector<long long> &off, const std::vector<int> &mz) {
    std::vector<int4> win;
    hll_build_blocks(total_rows, (int)mz.size(), off.data(), mz.data(), kPlanCap, win);
    const int W = (int)win.size();
    auto start_of = [&](int r) { return off[r / kHack] + (long long)(r % kHack) * mz[r / kHack]; };
    std::vector<long long> begin((size_t)W);
    std::vector<int> len((size_t)W), count((size_t)W), nl;
    for (int w = 0; w < W; ++w) {
        const int r0 = win[w].x, r1 = r0 + win[w].y - 1;
        const long long s0 = start_of(r0), end = start_of(r1) + mz[r1 / kHack];
        if (end - (s0 & ~1LL) > kPlanCap) return 0;  // a row that alone exceeds the stage: no plan
        begin[w] = s0;
        len[w] = (int)(end - s0);
        count[w] = (int)(end - (s0 & ~1LL));
    }
    return plan_on_device<4>(m->xw, m->JA, (size_t)off.back(), win, begin, len,
                             [&](int w, int first, int n) { return int4{first, n, count[w], 0}; }, nl);
}

// Everything of a handle but its slab: the x-window plan, workgroup windows, small arrays, vectors, the tile plan, the
// heuristics.  The handle's shape (M, N, M_total, row0, slots) is set; off / mz: hack offsets and row lengths on the
// host; slab: JA / AS, bound to the handle -- on the device already (hll_from_csr), or going there first thing.  The
// host builders (x-window plan, tile plan) ask the slab for its host view, which only then costs hll_from_csr a copy back.
int hll_finish_handle(spmv_hll_dev *m, const std::vector<long long> &off, const std::vector<int> &mz, MatrixSource<double> &slab) {
    const int total_rows = m->M, N = m->N, H = (int)mz.size();
    const long long true_slots = m->slots;
    // like the CSR stream kernel: larger stages for matrices that have plenty of work
    const int cap = true_slots >= (16LL << 20) ? kHllCap : kHllCap / 2;
    std::vector<int4> hdesc;
    const long long widest =
        std::max<long long>(2 * kStreamUnit, hll_build_blocks(total_rows, H, off.data(), mz.data(), cap, hdesc));
    m->hacks = H;
    // what hll_lds gets: .y = rows | slots of the window (from its even base) << 16 -- the kernel then knows how much to
    // stage without first asking the hack tables (0 in the upper half: a single row of more than 65535 slots, which has
    // its own path in the kernel)
    m->stage_slots = (int)std::min<long long>(kHllCap, (widest + kStreamUnit - 1) / kStreamUnit * kStreamUnit);
    std::vector<int> long_windows;  // one-row windows longer than the stage: SpMM's hll_spmm_row (spmv_hll_spmm.hip)
    for (int4 &d : hdesc) {
        const int last = d.x + d.y - 1;
        const long long s0 = (((long long)d.w << 32) | (unsigned)d.z) & ~1LL;
        const long long span = off[(size_t)(last / kHack)] + (long long)(last % kHack) * mz[(size_t)(last / kHack)] + mz[(size_t)(last / kHack)] - s0;
        if (d.y == 1 && span > m->stage_slots) long_windows.push_back((int)(&d - hdesc.data()));
        d.y |= span <= 0xffff ? (int)span << 16 : 0;
    }
    m->num_blocks = (int)hdesc.size();
    m->rest_bytes = off.size() * 8 + mz.size() * 4 + ((size_t)off[H] + kPad) * 12 + hdesc.size() * 16 +
                    long_windows.size() * 4 + ((size_t)N + (size_t)total_rows) * 8;
    if (slab.col.device_view() || slab.val.device_view()) return -1;
    // the x-window kernel (windows of 2048 slots, 16-bit local JA): its plan on the device when every window lists at
    // most 256 lines (then the line limit would not have moved any window boundary on the host either); otherwise the
    // host builder decides below (line-limited windows or no plan)
    const bool want_plan = g_stream_local && true_slots > 0;
    if (want_plan && g_plan_on_device && hll_plan_on_device(m, total_rows, off, mz) < 0) return -1;
    if (!m->hack_off && upload_array(&m->hack_off, off.data(), off.size(), 0)) return -1;
    if (!m->maxnz && upload_array(&m->maxnz, mz.data(), mz.size(), 1)) return -1;
    if (upload_array(&m->hdesc, hdesc.data(), hdesc.size(), 1)) return -1;
    if (!long_windows.empty() && upload_array(&m->long_windows, long_windows.data(), long_windows.size(), 0)) return -1;
    m->num_long_windows = (int)long_windows.size();
    if (alloc_vectors((void **)&m->x, (void **)&m->y, N, m->M_total, 8)) return -1;
    if (want_plan && m->xw.blocks == 0) {
        const int *ja = slab.col.host_view("hll_from_csr: JA download failed: %s");
        if (!ja) return -1;
        std::vector<int4> plain;
        LocalPlan<int4> local;
        hll_build_blocks(total_rows, H, off.data(), mz.data(), 2048, plain);
        if (hll_build_local(total_rows, N, off.data(), mz.data(), ja, off[H], 2048, kLocalLinesMax, plain, local) && m->xw.upload(local))
            return -1;
    }
    if (m->xw.blocks > 0 && hll_fill_row_segments(m)) return -1;
    // no x-window plan (columns too scattered): the 2-D tiles over the slab's rows, padding slots included -- the
    // rows of hack h are maxnz[h] slots each, starting at hack_off[h] + i * maxnz[h]
    // (auto: not for a skewed slab -- a hack whose rows are 16 times the mean is 32 rows of mostly padding, and tiles
    // over such rows lose to hll_lds: webbase-like stand-in, 1 M rows, 455 vs 159 us)
    bool skewed = false;
    if (g_stream_tile < 0 && total_rows > 0) {
        const long long mean = std::max<long long>(1, off[H] / total_rows);
        for (int h = 0; h < H && !skewed; ++h) skewed = mz[(size_t)h] > 16 * mean;
    }
    if (!skewed && m->xw.blocks == 0 && true_slots > 0 && off[H] < 0x7fffffffLL) {
        std::vector<int> row_begin((size_t)total_rows), row_len((size_t)total_rows);
        for (int r = 0; r < total_rows; ++r) {
            const int h = r / kHack;
            row_len[(size_t)r] = mz[(size_t)h];
            row_begin[(size_t)r] = (int)(off[(size_t)h] + (long long)(r % kHack) * mz[(size_t)h]);
        }
        if (csr_tiles_from_rows_f64(total_rows, m->M_total, m->row0, N, row_begin.data(), row_len.data(), true_slots, slab, &m->tiles))
            return -1;
    }
    const double mean = total_rows ? (double)true_slots / total_rows : 0.0;
    m->lanes_per_row = lanes_for_mean_row(mean);
    // Mid-size slabs that get neither plan (scattered columns, below the tile plans' size): the lane-group kernel beats
    // hll_lds by 10-27 % on every such stand-in of the reference's list (thermal1-size 6.7 vs 8.4 us, thermomech_TK-size
    // 7.2 vs 9.2, cop20k_A-size 19.1 vs 21.5, mac_econ-size 10.9 vs 12.2, amazon0302-size 12.0 vs 13.4;
    // profiles/r3_reference_list_stand_ins.md) -- unless hacks are skewed (its lanes per row are fixed); the rule CSR
    // upload has had since round 2
    int widest_hack = 0;
    for (int h = 0; h < H; ++h) widest_hack = std::max(widest_hack, mz[(size_t)h]);
    m->auto_variant = SPMV_HLL_LDS;
    if (m->xw.blocks == 0 && !m->tiles && true_slots < (20LL << 20) && widest_hack <= std::max(64.0, 8.0 * mean))
        m->auto_variant = SPMV_HLL_SUBWAVE;
    return 0;
}

using HllGuard = HandleGuard<spmv_hll_dev, spmv_hip_hll_free>;

}  // namespace

// Host-only self-check of what HLL upload precomputes (flat slab offsets, workgroup windows, the
// x-window plan); needs no device.  stats (optional, 4 ints): gather windows, x-window windows
// (0 = no plan), listed lines, widest window's lines.
static int spmv_hip_hll_plan_check_body(const HLLMatrix *hll, int total_rows, int N, int *stats) {
    if (!hll || total_rows < 0 || N < 0) return fail("hll_plan_check: bad arguments");
    const int H = hll->num_blocks;
    if (H != (total_rows + kHack - 1) / kHack) return fail("hll_plan_check: %d hacks do not match %d rows", H, total_rows);
    std::vector<int> mz((size_t)H, 0);
    for (int h = 0; h < H; ++h) {
        const ELLPACKBlock *b = &hll->blocks[h];
        if (b->MAXNZ < 0 || (b->MAXNZ > 0 && (!b->JA || !b->AS))) return fail("hll_plan_check: hack %d is malformed", h);
        if (b->M != ((h == H - 1) ? total_rows - h * kHack : kHack)) return fail("hll_plan_check: hack %d has %d rows", h, b->M);
        mz[h] = b->MAXNZ;
    }
    std::vector<long long> off;
    long long true_slots = 0;
    const long long S = hll_offsets(total_rows, mz, off, true_slots);
    std::vector<int> ja((size_t)S + kPad, 0);
    for (int h = 0; h < H; ++h) {
        const size_t s = (size_t)hll->blocks[h].M * mz[h];
        for (size_t k = 0; k < s; ++k) {
            if ((unsigned)hll->blocks[h].JA[k] >= (unsigned)N) return fail("hll_plan_check: column outside [0, %d) in hack %d", N, h);
            ja[(size_t)off[h] + k] = hll->blocks[h].JA[k];
        }
    }
    auto start_of = [&](int r) { return off[r / kHack] + (long long)(r % kHack) * mz[r / kHack]; };
    std::vector<int4> plain;
    LocalPlan<int4> plan;
    hll_build_blocks(total_rows, H, off.data(), mz.data(), 2048, plain);
    int next = 0;
    for (const int4 &d : plain) {  // windows tile the rows in order
        if (d.x != next || d.y <= 0) return fail("hll_plan_check: gather window at row %d out of order", d.x);
        next = d.x + d.y;
    }
    if (next != total_rows) return fail("hll_plan_check: gather windows end at row %d of %d", next, total_rows);
    const bool have = true_slots > 0 && hll_build_local(total_rows, N, off.data(), mz.data(), ja.data(), S, 2048,
                                                        kLocalLinesMax, plain, plan);
    int widest = 0;
    if (have) {
        next = 0;
        for (size_t b = 0; b < plan.desc.size(); ++b) {
            const int4 &d = plan.desc[b];
            const int4 &ld = plan.ldesc[b];
            if (d.x != next || d.y <= 0 || d.y > kStreamRowsCap) return fail("hll_plan_check: x-window window %zu out of order", b);
            next = d.x + d.y;
            const long long s0 = ((long long)d.w << 32) | (unsigned)d.z, base = s0 & ~1LL;
            const long long end = start_of(d.x + d.y - 1) + mz[(d.x + d.y - 1) / kHack];
            if (s0 != start_of(d.x) || ld.z != (int)(end - base) || ld.z > 2048) return fail("hll_plan_check: window %zu has a wrong extent", b);
            if (ld.y < 1 || ld.y > kLocalLinesMax) return fail("hll_plan_check: window %zu lists %d lines", b, ld.y);
            for (int k = 1; k < ld.y; ++k)
                if (plan.lines[ld.x + k] <= plan.lines[ld.x + k - 1]) return fail("hll_plan_check: lines of window %zu not ascending", b);
            for (long long k = s0; k < end; ++k) {
                const int slot = plan.lcol[k], rank = slot >> 4;
                if (rank >= ld.y || plan.lines[ld.x + rank] != (ja[k] >> 4) || (slot & 15) != (ja[k] & 15))
                    return fail("hll_plan_check: slot %lld (column %d) maps to %d", k, ja[k], slot);
            }
            widest = std::max(widest, ld.y);
        }
        if (next != total_rows) return fail("hll_plan_check: x-window windows end at row %d of %d", next, total_rows);
    }
    if (stats) {
        stats[0] = (int)plain.size();
        stats[1] = have ? (int)plan.desc.size() : 0;
        stats[2] = have ? (int)plan.lines.size() - kLocalLinesMax : 0;
        stats[3] = widest;
    }
    return 0;
}

extern "C" int spmv_hip_hll_plan_check(const HLLMatrix *hll, int total_rows, int N, int *stats) {
    return guarded("hll_plan_check", [&] { return spmv_hip_hll_plan_check_body(hll, total_rows, N, stats); });
}

// Hacks [hack0, hack1) of the matrix, i.e. rows [32 hack0, min(32 hack1, total_rows)): one
// rank's share under the reference's hack partitioner (prepare_thread_distribution_hll,
// src/hll_matrix.c:410-540); y stays full length, the kernels write this handle's rows.
static int spmv_hip_hll_upload_part_body(const HLLMatrix *hll, int total_rows, int N, int hack0, int hack1,
                                        spmv_hll_dev **out) {
    if (need_device()) return -1;
    if (!hll || !out) return fail("hll_upload: NULL argument");
    *out = nullptr;
    if ((unsigned long long)N * 8 >= (1ull << 32))
        return fail("hll_upload: N = %d exceeds the 32-bit gather offset range of the kernels", N);
    const int Hall = hll->num_blocks;
    if (Hall != (total_rows + kHack - 1) / kHack)
        return fail("hll_upload: %d hacks do not match %d rows", Hall, total_rows);
    if (hack0 < 0 || hack1 < hack0 || hack1 > Hall)
        return fail("hll_upload: bad hack range [%d, %d) of %d", hack0, hack1, Hall);
    const int H = hack1 - hack0;
    const int row0 = hack0 * kHack;
    const int rows = std::min(hack1 * kHack, total_rows) - std::min(row0, total_rows);

    std::vector<int> mz((size_t)H, 0);
    for (int h = 0; h < H; ++h) {
        const ELLPACKBlock *b = &hll->blocks[hack0 + h];
        const int expect = (hack0 + h == Hall - 1) ? total_rows - (hack0 + h) * kHack : kHack;
        if (b->M != expect) return fail("hll_upload: hack %d holds %d rows, expected %d", hack0 + h, b->M, expect);
        if (b->MAXNZ < 0 || (b->MAXNZ > 0 && (!b->JA || !b->AS)))
            return fail("hll_upload: hack %d is malformed", hack0 + h);
        mz[h] = b->MAXNZ;
        const long long s = (long long)b->M * b->MAXNZ;
        for (long long k = 0; k < s; ++k)
            if ((unsigned)b->JA[k] >= (unsigned)N)
                return fail("hll_upload: column index %d in hack %d is outside [0, %d)", b->JA[k], hack0 + h, N);
    }
    std::vector<long long> off;
    long long true_slots = 0;
    const long long S = hll_offsets(rows, mz, off, true_slots);
    if (S > (1LL << 40)) return fail("hll_upload: %lld padded slots is unreasonable", S);

    // pack every hack into one flat pair of host arrays, then two copies
    std::vector<int> ja((size_t)S + kPad, 0);
    std::vector<double> as((size_t)S + kPad, 0.0);
    for (int h = 0; h < H; ++h) {
        const ELLPACKBlock *b = &hll->blocks[hack0 + h];
        const size_t s = (size_t)b->M * b->MAXNZ;
        if (!s) continue;
        memcpy(&ja[(size_t)off[h]], b->JA, s * sizeof(int));
        memcpy(&as[(size_t)off[h]], b->AS, s * sizeof(double));
    }
    HllGuard guard(new (std::nothrow) spmv_hll_dev());
    spmv_hll_dev *m = guard.h;
    if (!m) return fail("hll_upload: out of host memory");
    m->M = rows, m->N = N, m->M_total = total_rows, m->row0 = row0, m->slots = true_slots;
    MatrixSource<double> slab = MatrixSource<double>::on_host(ja.data(), as.data());
    slab.bind(&m->JA, &m->AS, 0, ja.size(), 0);
    if (hll_finish_handle(m, off, mz, slab)) return -1;
    hll_upload_searches(m);
    *out = guard.release();
    return 0;
}

extern "C" int spmv_hip_hll_upload_part(const HLLMatrix *hll, int total_rows, int N, int hack0, int hack1,
                                        spmv_hll_dev **out) {
    return guarded("hll_upload", [&] { return spmv_hip_hll_upload_part_body(hll, total_rows, N, hack0, hack1, out); });
}

extern "C" int spmv_hip_hll_upload(const HLLMatrix *hll, int total_rows, int N, spmv_hll_dev **out) {
    if (!hll) return fail("hll_upload: NULL argument");
    return spmv_hip_hll_upload_part(hll, total_rows, N, 0, hll->num_blocks, out);
}

// HLL built on the device from a resident CSR matrix (whole matrix, fp64).
static int spmv_hip_hll_from_csr_body(const spmv_csr_dev *csr, spmv_hll_dev **out) {
    if (need_device()) return -1;
    if (!csr || !out) return fail("hll_from_csr: NULL argument");
    *out = nullptr;
    // a row block works when it starts on a hack boundary and ends on one (or at the last row)
    if (csr->value_bytes != 8 || csr->row0 % kHack != 0 ||
        ((csr->row0 + csr->M_local) % kHack != 0 && csr->row0 + csr->M_local != csr->M_total))
        return fail("hll_from_csr: needs a whole fp64 CSR matrix (or a row block cut on hack boundaries)");
    const int M = csr->M_local, N = csr->N, H = (M + kHack - 1) / kHack;
    HllGuard guard(new (std::nothrow) spmv_hll_dev());
    spmv_hll_dev *m = guard.h;
    if (!m) return fail("hll_from_csr: out of host memory");
    std::vector<int> mz((size_t)H, 0);
    std::vector<long long> off;
    hipError_t e = hipMalloc((void **)&m->maxnz, ((size_t)H + 1) * sizeof(int));
    if (e != hipSuccess) return fail("hipMalloc(maxnz) failed: %s", hipGetErrorString(e));
    if (H > 0) {
        hipLaunchKernelGGL(hll_hack_maxnz, dim3((H + kBlock - 1) / kBlock), dim3(kBlock), 0, g_stream, M, H,
                           csr->row_ptr, m->maxnz);
        e = hipMemcpyAsync(mz.data(), m->maxnz, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail("hll_from_csr: maxnz pass failed: %s", hipGetErrorString(e));
    }
    m->M = M, m->N = N, m->M_total = csr->M_total, m->row0 = csr->row0;
    const long long S = hll_offsets(M, mz, off, m->slots);  // H-sized scan on the host
    if (S > (1LL << 40)) return fail("hll_from_csr: %lld padded slots is unreasonable", S);
    e = hipMalloc((void **)&m->JA, ((size_t)S + kPad) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&m->AS, ((size_t)S + kPad) * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(m->JA, 0, ((size_t)S + kPad) * sizeof(int), g_stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->AS, 0, ((size_t)S + kPad) * sizeof(double), g_stream);
    if (e != hipSuccess) return fail("hll_from_csr: slab allocation failed: %s", hipGetErrorString(e));
    if (upload_array(&m->hack_off, off.data(), off.size(), 0)) return -1;
    if (M > 0) {
        hipLaunchKernelGGL((hll_fill_from_csr<double>), dim3((M + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock),
                           0, g_stream, M, csr->row_ptr, csr->col, (const double *)csr->val, m->hack_off,
                           m->maxnz, m->JA, m->AS);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail("hll_from_csr: fill failed: %s", hipGetErrorString(e));
    }
    MatrixSource<double> slab;  // on the device only: S slots (+ kPad zeroed) in the handle's JA / AS
    slab.bind(&m->JA, &m->AS, 0, (size_t)S, kPad);
    if (hll_finish_handle(m, off, mz, slab)) return -1;
    hll_upload_searches(m);
    *out = guard.release();
    return 0;
}

extern "C" int spmv_hip_hll_from_csr(const spmv_csr_dev *csr, spmv_hll_dev **out) {
    return guarded("hll_from_csr", [&] { return spmv_hip_hll_from_csr_body(csr, out); });
}

// flat slab back to the host (tests; hosts that want the HLL arrays): hack_off[hacks + 1],
// maxnz[hacks], JA / AS [hack_off[hacks]]; any pointer may be NULL
extern "C" int spmv_hip_hll_download(const spmv_hll_dev *m, long long *hack_off, int *maxnz, int *JA, double *AS) {
    if (need_device()) return -1;
    if (!m) return fail("hll_download: NULL handle");
    HIP_TRY(hipStreamSynchronize(g_stream));
    std::vector<long long> off((size_t)m->hacks + 1);
    HIP_TRY(hipMemcpy(off.data(), m->hack_off, off.size() * sizeof(long long), hipMemcpyDeviceToHost));
    if (hack_off) memcpy(hack_off, off.data(), off.size() * sizeof(long long));
    if (maxnz && m->hacks) HIP_TRY(hipMemcpy(maxnz, m->maxnz, (size_t)m->hacks * sizeof(int), hipMemcpyDeviceToHost));
    const size_t S = (size_t)off[m->hacks];
    if (JA && S) HIP_TRY(hipMemcpy(JA, m->JA, S * sizeof(int), hipMemcpyDeviceToHost));
    if (AS && S) HIP_TRY(hipMemcpy(AS, m->AS, S * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void spmv_hip_hll_free(spmv_hll_dev *m) {
    if (!m) return;
    (void)hipFree(m->hack_off);
    (void)hipFree(m->maxnz);
    (void)hipFree(m->JA);
    (void)hipFree(m->AS);
    (void)hipFree(m->hdesc);
    (void)hipFree(m->long_windows);
    m->xw.release();
    spmv_hip_csr_free(m->tiles);
    (void)hipFree(m->x);
    (void)hipFree(m->y);
    delete m;
}

// the digest of the tile plan over the slab's rows (tests); all zeros without one
extern "C" int spmv_hip_hll_tile_digest(const spmv_hll_dev *m, unsigned long long *out) {
    if (!m || !out) return fail("hll_tile_digest: NULL argument");
    if (!m->tiles) {
        memset(out, 0, 64 * sizeof(unsigned long long));
        return 0;
    }
    return guarded("hll_tile_digest", [&] { return csr_tile_digest(m->tiles, out); });
}

extern "C" int spmv_hip_hll_info(const spmv_hll_dev *m, spmv_dev_info *out) {
    if (!m || !out) return fail("hll_info: NULL argument");
    memset(out, 0, sizeof *out);
    out->M_local = m->M;
    out->M_total = m->M_total;
    out->row0 = m->row0;
    out->N = m->N;
    out->value_bytes = 8;
    out->auto_variant = m->auto_variant;
    out->lanes_per_row = m->lanes_per_row;
    out->stream_blocks = m->num_blocks;
    out->slots = m->slots;
    out->hacks = m->hacks;
    // S (val + 4) + 12 H + val (M + N)
    out->algo_bytes = m->slots * 12 + 12LL * m->hacks + 8LL * ((long long)m->M + m->N);
    out->device_bytes = (long long)hll_device_bytes(m);
    const XWindowPlan<int4> &p = m->xw;
    out->local_blocks = p.blocks;
    out->place_tries = m->place_tries;
    out->place_first_us = m->place_first_us;
    out->place_best_us = m->place_best_us;
    out->val_address = (unsigned long long)(uintptr_t)m->AS;
    out->pattern_slots = p.pat.ptab ? p.pat.slots : 0;
    out->pattern_with_us = p.pat.with_us;
    out->pattern_without_us = p.pat.without_us;
    out->stream_kernel = p.blocks > 0 ? 1 : m->tiles ? 2 : 0;
    if (m->tiles) {
        spmv_dev_info t;
        if (spmv_hip_csr_info(m->tiles, &t) == 0) {
            out->tile_blocks = t.tile_blocks;
            out->tile_passes = t.tile_passes;
            out->tile_entries = t.tile_entries;
            out->tile_staged_entries = t.tile_staged_entries;
            out->tile_long_rows = t.tile_long_rows;
            out->tile_long_items = t.tile_long_items;
            out->tile_long_entries = t.tile_long_entries;
            out->tile_staged_cols = t.tile_staged_cols;
            out->tile_remainder_entries = t.tile_remainder_entries;
            out->stream_bytes = t.stream_bytes + 12LL * m->hacks;
        }
    }
    out->local_stage_lines = p.stage_lines;
    out->local_lines = p.lines_listed;
    if (p.blocks > 0)  // (a pattern plan: the tables and 4 bytes per row instead of 2 bytes per slot)
        out->stream_bytes = m->slots * 8 + (p.pat.ptab ? 2 * p.pat.slots + 4LL * m->M + 8LL * p.blocks : 2 * m->slots) +
                            4 * p.lines_listed + 32LL * p.blocks + 12LL * m->hacks + 8LL * ((long long)m->M + m->N);
    return 0;
}

extern "C" void *spmv_hip_hll_x_ptr(spmv_hll_dev *m) { return m ? m->x : nullptr; }
extern "C" void *spmv_hip_hll_y_ptr(spmv_hll_dev *m) { return m ? m->y : nullptr; }

extern "C" int spmv_hip_hll_set_x(spmv_hll_dev *m, const double *x_host) {
    if (need_device()) return -1;
    if (!m || !x_host) return fail("hll_set_x: NULL argument");
    HIP_TRY(hipMemcpyAsync(m->x, x_host, (size_t)m->N * 8, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int spmv_hip_hll_get_y(spmv_hll_dev *m, double *y_host) {
    if (need_device()) return -1;
    if (!m || !y_host) return fail("hll_get_y: NULL argument");
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(y_host, m->y, (size_t)m->M_total * 8, hipMemcpyDeviceToHost));  // whole y, as for CSR
    return 0;
}

namespace {

template <int L>
void launch_hll_vector(const spmv_hll_dev *m, const double *x, double *y, hipStream_t s) {
    constexpr int rows = kBlock / L;
    hipLaunchKernelGGL((hll_vector<double, L>), dim3((m->M + rows - 1) / rows), dim3(kBlock), 0, s,
                       m->M, m->hack_off, m->maxnz, m->JA, m->AS, x, y);
}

}  // namespace

int hll_launch(const spmv_hll_dev *m, int variant, const double *x, double *y_full, hipStream_t s) {
    if (m->M == 0) return 0;
    double *y = y_full + m->row0;  // the kernels number this handle's rows from 0
    if (variant == SPMV_HLL_AUTO) variant = m->auto_variant;
    switch (variant) {
        case SPMV_HLL_THREAD_ROW:
            hipLaunchKernelGGL((hll_thread_row<double>), dim3((m->M + kBlock - 1) / kBlock),
                               dim3(kBlock), 0, s, m->M, m->hack_off, m->maxnz, m->JA, m->AS, x, y);
            break;
        case SPMV_HLL_SUBWAVE:
            switch (m->lanes_per_row) {
                case 2: launch_hll_vector<2>(m, x, y, s); break;
                case 4: launch_hll_vector<4>(m, x, y, s); break;
                case 8: launch_hll_vector<8>(m, x, y, s); break;
                case 16: launch_hll_vector<16>(m, x, y, s); break;
                default: launch_hll_vector<32>(m, x, y, s); break;
            }
            break;
        case SPMV_HLL_LDS: {
            const XWindowPlan<int4> &p = m->xw;
            if (x_window_runs(p.blocks, x)) {
                // (a pattern plan: tables only, so no segment behind the rebuilt slots)
                const XWindowLaunch L = p.launch_shape(p.blocks, 2048, 8, m->slots);
                with_flag(L.nt, [&](auto nt) {
                    constexpr bool NT = decltype(nt)::value;
                    if (L.patterns)
                        hipLaunchKernelGGL((hll_lds_local<double, NT, 2048, true>), dim3(L.grid), dim3(kBlock), L.pat_lds, s,
                                           p.blocks, L.chunk, p.ldesc4, p.ldesc, p.lines, p.row_seg, p.slot, m->AS, x, y,
                                           p.pat.pdesc, p.pat.rinfo, p.pat.ptab, (int)L.lds);
                    else
                        hipLaunchKernelGGL((hll_lds_local<double, NT, 2048>), dim3(L.grid), dim3(kBlock), L.lds, s, p.blocks,
                                           L.chunk, p.ldesc4, p.ldesc, p.lines, p.row_seg, p.slot, m->AS, x, y);
                });
                break;
            }
            // csr_tile over the slab's rows (a packed plan with a foreign x that is not 16-byte aligned goes to hll_lds
            // below instead of being read past its end)
            if (m->tiles && tiles_run(m->tiles, x, false)) return csr_launch_any(m->tiles, SPMV_CSR_STREAM, x, y_full, s);
            const size_t lds = 32 + ((size_t)m->stage_slots + 2) * sizeof(double);
            // (the instantiations stage an even number of 512-slot units: the handle's, rounded up)
            with_value<2, 4, 6, 8>((m->stage_slots / kStreamUnit + 1) / 2 * 2, [&](auto maxu) {
                hipLaunchKernelGGL((hll_lds<double, true, decltype(maxu)::value>), dim3(m->num_blocks), dim3(kBlock), lds, s,
                                   m->stage_slots, m->hdesc, m->hack_off, m->maxnz, m->JA, m->AS, x, y);
            });
            break;
        }
        default:
            return fail("unknown HLL variant %d", variant);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}



extern "C" int spmv_hip_hll_run(spmv_hll_dev *m, int variant) {
    if (need_device()) return -1;
    if (!m) return fail("hll_run: NULL handle");
    return hll_launch(m, variant, m->x, m->y, g_stream);
}

extern "C" int spmv_hip_hll_run_on(spmv_hll_dev *m, int variant, const void *d_x, void *d_y, void *stream) {
    if (need_device()) return -1;
    if (!m || !d_x || !d_y) return fail("hll_run_on: NULL argument");
    return hll_launch(m, variant, (const double *)d_x, (double *)d_y, stream ? (hipStream_t)stream : g_stream);
}

extern "C" int spmv_hip_hll_time(spmv_hll_dev *m, int variant, int warmup, int iters, int zero_y,
                                 float *ms_each) {
    if (need_device()) return -1;
    if (!m) return fail("hll_time: NULL handle");
    return time_loop(
        warmup, iters, ms_each, [&] { return hll_launch(m, variant, m->x, m->y, g_stream); },
        [&]() -> int {
            if (zero_y) HIP_TRY(hipMemsetAsync(m->y, 0, (size_t)m->M_total * 8, g_stream));
            return 0;
        });
}

extern "C" int spmv_hip_hll_time_graph(spmv_hll_dev *m, int variant, int iters, int replays, float *ms_per_iter) {
    if (need_device()) return -1;
    if (!m) return fail("hll_time_graph: NULL handle");
    return graph_loop(iters, replays, ms_per_iter, [&] { return hll_launch(m, variant, m->x, m->y, g_stream); });
}

