// upload_ops.hpp -- what CSR upload (spmv_csr.hip) and HLL upload (spmv_hll.hip) share: the x-window plan built on the
// device, the pattern plan's tables, and the searches that time the finished handle's own kernel (settle, the pattern
// plan, the placement of the value array).
//
// A step that upload may do without (the pattern plan, a search) never costs the handle: when it fails, it leaves
// nothing half-built and clears the last HIP error, which the next launch would otherwise report as its own.
#pragma once
#include <chrono>

#include "spmv_internal.hpp"

#include "plan_kernels.hpp"

namespace {

constexpr size_t kPlaceMinBytes = (size_t)128 << 20;  // value arrays from which upload searches their placement

// The x-window plan of the windows win[w] (plan_kernels.hpp), window w over idx[begin[w], begin[w] + len[w]) of the
// device column array idx, at 1 << SHIFT columns per 128-byte line: the count pass, then -- when no window lists more
// than kLocalLinesMax lines -- the line lists (m->lines), the 16-bit slots (`slot`, slots + kPad entries), the fill pass
// and the windows' descriptors (m->ldesc4 = win; ldesc[w] = desc_of(w, first line, lines)).  nlines: every window's line
// count.  1: the handle carries the plan; 0: some window lists too many lines; -1: HIP error.  Anything but 1 leaves
// no plan behind.
template <int SHIFT, typename H, typename D, typename Desc>
int plan_on_device(H *m, const int *idx, size_t slots, const std::vector<int4> &win, const std::vector<long long> &begin,
                   const std::vector<int> &len, unsigned short *&slot, D *&ldesc, Desc desc_of, std::vector<int> &nlines) {
    const int W = (int)win.size();
    if (W == 0) return 0;
    long long *d_begin = nullptr;
    int *d_len = nullptr, *d_n = nullptr, *d_off = nullptr;
    int result = -1;
    do {
        if (upload_array(&d_begin, begin.data(), begin.size(), 0) || upload_array(&d_len, len.data(), len.size(), 0)) break;
        hipError_t e = hipMalloc((void **)&d_n, (size_t)W * sizeof(int));
        if (e != hipSuccess) { fail("x-window plan: hipMalloc failed: %s", hipGetErrorString(e)); break; }
        hipLaunchKernelGGL((plan_count<SHIFT>), dim3(W), dim3(kBlock), 0, g_stream, W, d_begin, d_len, idx, d_n);
        nlines.assign((size_t)W, 0);
        e = hipMemcpyAsync(nlines.data(), d_n, (size_t)W * sizeof(int), hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) { fail("x-window plan: count pass failed: %s", hipGetErrorString(e)); break; }
        std::vector<int> line_off((size_t)W);
        std::vector<D> h_ldesc((size_t)W);
        long long total = 0;
        int widest = 0;
        bool fits = true;
        for (int w = 0; w < W && fits; ++w) {
            const int n = std::max(nlines[w], 1);  // a window of empty rows still stages one line
            fits = nlines[w] <= kLocalLinesMax && total + n < (1LL << 31);
            line_off[w] = (int)total;
            h_ldesc[w] = desc_of(w, (int)total, n);
            total += n;
            widest = std::max(widest, n);
        }
        if (!fits) { result = 0; break; }
        if (upload_array(&d_off, line_off.data(), line_off.size(), 0)) break;
        e = hipMalloc((void **)&m->lines, ((size_t)total + kLocalLinesMax) * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void **)&slot, (slots + kPad) * sizeof(unsigned short));
        if (e == hipSuccess) e = hipMemsetAsync(m->lines, 0, ((size_t)total + kLocalLinesMax) * sizeof(int), g_stream);
        if (e == hipSuccess) e = hipMemsetAsync(slot, 0, (slots + kPad) * sizeof(unsigned short), g_stream);
        if (e != hipSuccess) { fail("x-window plan: allocation failed: %s", hipGetErrorString(e)); break; }
        hipLaunchKernelGGL((plan_fill<SHIFT>), dim3(W), dim3(kBlock), 0, g_stream, W, d_begin, d_len, idx, d_off,
                           m->lines, slot);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) { fail("x-window plan: fill pass failed: %s", hipGetErrorString(e)); break; }
        if (upload_array(&m->ldesc4, win.data(), win.size(), 1) || upload_array(&ldesc, h_ldesc.data(), h_ldesc.size(), 1))
            break;
        m->local_blocks = W;
        m->local_lines = total;
        m->local_stage_lines = std::max(kLocalLineQuantum,
                                        (widest + kLocalLineQuantum - 1) / kLocalLineQuantum * kLocalLineQuantum);
        result = 1;
    } while (0);
    for (void *p : {(void *)d_begin, (void *)d_len, (void *)d_n, (void *)d_off}) (void)hipFree(p);
    if (result != 1) {
        for (void *p : {(void *)m->lines, (void *)slot, (void *)m->ldesc4, (void *)ldesc}) (void)hipFree(p);
        m->lines = nullptr;
        slot = nullptr;
        m->ldesc4 = nullptr;
        ldesc = nullptr;
        m->local_blocks = 0;
    }
    return result;
}

// The pattern plan's tables (plan_kernels.hpp: pat_mark, pat_fill) of the blocks ldesc4[0, blocks) over their 16-bit
// slots `slot`, a row's slots found through row_ptr, or through row_seg (ROW_SEG: HLL windows).  auto: built for streamed
// handles (the `nt` threshold) of at least 12 slots per row, and only where the tables hold at most a quarter of the
// slots.  Returns the elements of every block's table; pat.ptab == nullptr: no plan (not wanted, or it could not be
// built -- then nothing is left of it and the last HIP error is cleared).
template <bool ROW_SEG>
std::vector<int> build_pattern_tables(PatternPlan &pat, int blocks, int rows, long long slots, int value_bytes,
                                      const int4 *ldesc4, const int *row_ptr, const unsigned *row_seg,
                                      const unsigned short *slot) {
    std::vector<int> count;
    if (g_local_patterns == 0 || blocks <= 0 || rows <= 0 || !ldesc4 || !slot || (!row_ptr && !row_seg)) return count;
    if (g_local_patterns < 0 && (slots * (value_bytes + 2LL) <= (128LL << 20) || slots < 12LL * rows)) return count;
    int *rowflag = nullptr, *pcount = nullptr;
    long long *pbase = nullptr;
    hipError_t e = hipMalloc((void **)&rowflag, (size_t)rows * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&pcount, (size_t)blocks * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&pbase, (size_t)blocks * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(rowflag, 0, (size_t)rows * sizeof(int), g_stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((pat_mark<256, ROW_SEG>), dim3(blocks), dim3(256), 0, g_stream, blocks, ldesc4, row_ptr, slot,
                           rowflag, pcount, row_seg);
        count.assign((size_t)blocks, 0);
        e = hipMemcpyAsync(count.data(), pcount, (size_t)blocks * sizeof(int), hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    }
    std::vector<long long> base((size_t)blocks);
    long long total = 0;
    int widest = 0;
    for (int b = 0; b < blocks && e == hipSuccess; ++b) {
        base[(size_t)b] = total;
        total += count[(size_t)b];
        widest = std::max(widest, count[(size_t)b]);
    }
    // (auto) a plan whose tables hold more than a quarter of the slots keeps reading the slot stream
    const bool wanted = !(g_local_patterns < 0 && total * 4 > slots) && total <= 0x7ffffff0LL;
    if (e == hipSuccess && wanted) {
        e = hipMalloc((void **)&pat.ptab, ((size_t)total + 1024) * sizeof(unsigned short));
        if (e == hipSuccess) e = hipMalloc((void **)&pat.rinfo, (size_t)rows * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc((void **)&pat.pdesc, (size_t)blocks * sizeof(int2));
        if (e == hipSuccess) e = hipMemsetAsync(pat.ptab, 0, ((size_t)total + 1024) * sizeof(unsigned short), g_stream);
        if (e == hipSuccess) e = hipMemsetAsync(pat.rinfo, 0, (size_t)rows * sizeof(unsigned), g_stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pbase, base.data(), (size_t)blocks * sizeof(long long), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL((pat_fill<256, ROW_SEG>), dim3(blocks), dim3(256), 0, g_stream, blocks, ldesc4, row_ptr,
                               slot, rowflag, pbase, pat.rinfo, pat.ptab, pat.pdesc, row_seg);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    }
    for (void *p : {(void *)rowflag, (void *)pcount, (void *)pbase}) (void)hipFree(p);
    if (e != hipSuccess || !wanted) {
        pat.release();
        (void)hipGetLastError();
        count.clear();
        return count;
    }
    pat.slots = total;
    pat.widest = widest;
    return count;
}

// One pair of events for the searches.  time(): 2 untimed + 6 timed launches -> us per launch; false when a launch or
// the timing failed.
struct UploadTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = false;

    UploadTimer() {
        ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
        if (!ok) (void)hipGetLastError();
    }
    UploadTimer(const UploadTimer &) = delete;
    UploadTimer &operator=(const UploadTimer &) = delete;
    ~UploadTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    template <typename Launch>
    bool time(Launch launch, float &us) {
        hipError_t e = launch() == 0 && launch() == 0 ? hipEventRecord(e0, g_stream) : hipErrorUnknown;
        for (int i = 0; i < 6 && e == hipSuccess; ++i)
            if (launch()) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipEventRecord(e1, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        us = ms * 1e3f / 6.0f;
        return true;
    }
};

// Both searches compare launch times: they begin in the card's steady state -- after an idle stretch (the upload) the
// same launch costs 178, then 208, then, from about the 60th on, 175 us (profiles/r3_launch_time_series.txt), a drift as
// large as what the searches look for.  ~15 ms of the handle's own kernel first.
template <typename Launch>
void upload_settle(Launch launch) {
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() < 15.0) {
        bool bad = false;
        for (int i = 0; i < 16 && !bad; ++i) bad = launch() != 0;
        if (bad || hipStreamSynchronize(g_stream) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
    }
}

// (auto) the handle's kernel with and without its pattern plan, alternately, two rounds of 2 + 6 launches each: the plan
// stays if it is at least 2 % faster here.
template <typename H, typename Launch>
void tune_pattern_plan(H *m, long long rows, Launch launch) {
    UploadTimer timer;
    if (!timer.ok) return;
    auto measure = [&](int patterns, float &us) {
        const int keep = g_local_patterns;
        g_local_patterns = patterns;
        const bool ok = timer.time(launch, us);
        g_local_patterns = keep;
        return ok;
    };
    PatternPlan &pat = m->pat;
    bool ok = true;
    for (int round = 0; round < 2 && ok; ++round) {
        float a = 0, b = 0;
        ok = measure(1, a) && measure(0, b);
        pat.with_us = round ? std::min(pat.with_us, a) : a;
        pat.without_us = round ? std::min(pat.without_us, b) : b;
    }
    if (!ok || pat.with_us > 0.98f * pat.without_us) {  // not faster here: the slot stream stays
        m->device_bytes -= std::min(m->device_bytes, pat.bytes(rows, m->local_blocks));
        pat.release();
    }
}

// Where the value array lies decides -- for as long as the allocation lives, by a mechanism the counters at hand do not
// name (profiles/r3_placement_*.txt: not the XCD mapping, not the TLB, not one slow XCD; every block of one HALF of
// the matrix is a little slower) -- whether the x-window kernel runs the headline matrix in 182-187 or in 199-205 us.
// So a handle that streams enough values for it to matter times its own kernel on a few placements and keeps the best:
// up to g_place_tries fresh allocations of the value array `val` (`bytes` long; earlier candidates stay allocated
// meanwhile, so every one is a different place), 2 + 6 launches each.  ~2 ms per candidate at 100 M entries; upload
// itself takes 50-100.  Three levels exist -- both halves of the array fast (180-182 us on the headline matrix), one
// (186-194), none (199-205); fresh allocations land on them roughly 2 : 5 : 5 (profiles/r3_placement_*.txt) -- so the
// search goes on until a candidate is 8.5 % faster than the slowest seen (= the top level reached) or the tries are used
// up.
template <typename H, typename V, typename Launch>
void tune_placement(H *m, V *&val, size_t bytes, Launch launch) {
    UploadTimer timer;
    if (!timer.ok) return;
    V *first = val, *best = val;
    std::vector<V *> others;
    float best_us = 0;
    bool ok = timer.time(launch, best_us);
    m->place_first_us = best_us;
    m->place_tries = 1;
    float worst_us = best_us;
    for (int t = 0; t < g_place_tries && ok; ++t) {
        V *p = nullptr;
        if (hipMalloc((void **)&p, bytes) != hipSuccess) {  // (out of memory for another copy: keep what we have)
            (void)hipGetLastError();
            break;
        }
        others.push_back(p);
        if (hipMemcpy(p, first, bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        val = p;
        float us = 0;
        ok = timer.time(launch, us);
        if (!ok) break;
        ++m->place_tries;
        if (us < best_us * 0.985f) {  // (1.5 %: above the run-to-run noise of 6 launches)
            best = p;
            best_us = us;
        }
        worst_us = std::max(worst_us, us);
        if (best_us < worst_us * 0.915f) break;  // both halves of the array at their fast level (see above): nothing better to find
    }
    val = best;
    m->place_best_us = best_us;
    if (best != first) (void)hipFree(first);
    for (V *p : others)
        if (p != best) (void)hipFree(p);
}

// The searches of a finished handle, in this order: settle, the pattern plan (auto; `rows` rows), the placement of the
// value array *val (`bytes` long; val == nullptr: the handle's kernel does not stream it, or it is below
// kPlaceMinBytes).  launch() runs the handle's own kernel.  None is ever a reason to lose the handle.
template <typename H, typename V, typename Launch>
void upload_searches(H *m, long long rows, V **val, size_t bytes, Launch launch) {
    const bool patterns = g_local_patterns < 0 && m->pat.ptab;
    const bool place = val && *val && g_place_tries > 0;
    if (patterns || place) upload_settle(launch);
    if (patterns) tune_pattern_plan(m, rows, launch);
    if (place) tune_placement(m, *val, bytes, launch);
}

}  // namespace
