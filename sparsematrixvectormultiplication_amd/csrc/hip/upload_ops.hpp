// upload_ops.hpp -- what CSR upload (spmv_csr.hip) and HLL upload (spmv_hll.hip) share: the source of a matrix's entry
// arrays (where they live, host or device, and the one way to the other side), the guard of a handle under
// construction, the vectors, the x-window plan built on the device, the pattern plan's tables, and the searches that
// time the finished handle's own kernel (settle, the pattern plan, the placement of the value array).
//
// A step that upload may do without (the pattern plan, a search) never costs the handle: when it fails, it leaves
// nothing half-built and clears the last HIP error, which the next launch would otherwise report as its own.
#pragma once
#include <chrono>

#include "spmv_internal.hpp"

#include "plan_kernels.hpp"

// One array of a matrix on its way into a handle, and where it lives right now: with the caller on the host (`host`), on
// the device in the handle's field (*field: adopted from the caller, uploaded by an earlier phase, or filled by a device
// builder), or both.  A phase of upload asks for the side it needs; it never tests the pointers itself.
template <typename E>
struct UploadSource {
    const E *host = nullptr;    // the caller's array; nullptr: the array exists on the device only
    E *adopted = nullptr;       // a device array (count + pad elements, the pad zeroed) that the handle takes over
    E **field = nullptr;        // where the handle keeps the device array; nullptr: not bound to a handle yet
    size_t count = 0, pad = 0;  // elements, and the zeroed elements behind them on the device
    bool kept = false;
    std::vector<E> back;        // the one copy back from the device (host_view)

    // an adopted array is the caller's again unless the handle was handed out (keep): declared behind the handle's guard,
    // the source goes first and takes the array out of the handle before the guard frees it
    ~UploadSource() { if (field && adopted && !kept) *field = nullptr; }
    // elements [first, first + n) of the caller's array go to *f (an adopted array holds exactly those)
    void bind(E **f, size_t first, size_t n, size_t pad_behind) {
        field = f;
        if (host) host += first;
        count = n, pad = pad_behind;
        if (adopted) *f = adopted;
    }
    // The array on the host: the caller's, or ONE copy back from the device, kept until the upload ends.  nullptr: the
    // copy failed and `message` is the error (it may print HIP's own text as its one %s).
    const E *host_view(const char *message) {
        if (host) return host;
        if (!back.empty()) return back.data();
        back.resize(std::max<size_t>(count, 1));
        const hipError_t e = count ? hipMemcpy(back.data(), *field, count * sizeof(E), hipMemcpyDeviceToHost) : hipSuccess;
        if (e == hipSuccess) return back.data();
        back.clear();
        fail(message, hipGetErrorString(e));
        return nullptr;
    }
    // the array on the device, in the handle's field: uploaded once, a no-op when it is there already
    int device_view() { return *field ? 0 : upload_array(field, host, count, pad); }
};

// The two entry arrays of a matrix: col / val of a CSR handle, JA / AS of an HLL slab.
template <typename V>
struct MatrixSource {
    UploadSource<int> col;
    UploadSource<V> val;

    static MatrixSource on_host(const int *col_host, const V *val_host) { MatrixSource s; s.col.host = col_host, s.val.host = val_host; return s; }
    static MatrixSource adopting(int *d_col, V *d_val) { MatrixSource s; s.col.adopted = d_col, s.val.adopted = d_val; return s; }
    void bind(int **col_field, V **val_field, size_t first, size_t n, size_t pad_behind) {
        col.bind(col_field, first, n, pad_behind);
        val.bind(val_field, first, n, pad_behind);
    }
    bool on_host() const { return col.host && val.host; }
    bool on_device() const { return *col.field && *val.field; }
    void keep() { col.kept = val.kept = true; }  // the handle is handed out: it owns what it adopted
};

// spmv_csr.hip: tile plans alone for rows given as (first entry, length) over the arrays `slab` (an HLL slab's rows): built
// on the device where the slab is there, else from its host view; *out = NULL when the rows get no plan
int csr_tiles_from_rows_f64(int M_local, int M_total, int row0, int N, const int *row_begin, const int *row_len,
                            long long entries, MatrixSource<double> &slab, spmv_csr_dev **out);

// Owns a handle from `new` until it is handed out (release); on every other way out the handle is freed.
template <typename H, void (*Free)(H *)>
struct HandleGuard {
    H *h;
    explicit HandleGuard(H *handle) : h(handle) {}
    HandleGuard(const HandleGuard &) = delete;
    ~HandleGuard() { if (h) Free(h); }
    H *release() { return std::exchange(h, nullptr); }
};

// The vectors of a handle, zeroed.  x is read in whole 128-byte lines by the x-window kernels: room for the tail of the
// last one.
inline int alloc_vectors(void **x, void **y, int N, int M_total, int value_bytes) {
    const size_t x_bytes = std::max<size_t>((size_t)N, 1) * (size_t)value_bytes + kLineBytes;
    const size_t y_bytes = std::max<size_t>((size_t)M_total, 1) * (size_t)value_bytes;
    hipError_t e = hipMalloc(x, x_bytes);
    if (e == hipSuccess) e = hipMalloc(y, y_bytes);
    if (e == hipSuccess) e = hipMemset(*x, 0, x_bytes);
    if (e == hipSuccess) e = hipMemset(*y, 0, y_bytes);
    return e == hipSuccess ? 0 : fail("hipMalloc(x/y) failed: %s", hipGetErrorString(e));
}

// lanes per row for the lane-group (SUBWAVE) kernels: about half the mean row length, rounded down to a power of two, so
// that a typical row takes 1-2 passes
inline int lanes_for_mean_row(double mean) { return std::min(32, std::max(2, pow2_floor(std::max(2, (int)(mean / 2.0 + 0.5))))); }

namespace {

constexpr size_t kPlaceMinBytes = (size_t)128 << 20;  // value arrays from which upload searches their placement

// The x-window plan of the windows win[w] (plan_kernels.hpp), window w over idx[begin[w], begin[w] + len[w]) of the
// device column array idx, at 1 << SHIFT columns per 128-byte line: the count pass, then -- when no window lists more
// than kLocalLinesMax lines -- the line lists, the 16-bit slots (slots + kPad entries), the fill pass and the windows'
// descriptors (ldesc4 = win; ldesc[w] = desc_of(w, first line, lines)), all into `plan`.  nlines: every window's line
// count.  1: `plan` is the plan; 0: some window lists too many lines; -1: HIP error.  Anything but 1 leaves no plan
// behind.
template <int SHIFT, typename D, typename DescOf>
int plan_on_device(XWindowPlan<D> &plan, const int *idx, size_t slots, const std::vector<int4> &win,
                   const std::vector<long long> &begin, const std::vector<int> &len, DescOf desc_of, std::vector<int> &nlines) {
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
        e = hipMalloc((void **)&plan.lines, ((size_t)total + kLocalLinesMax) * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void **)&plan.slot, (slots + kPad) * sizeof(unsigned short));
        if (e == hipSuccess) e = hipMemsetAsync(plan.lines, 0, ((size_t)total + kLocalLinesMax) * sizeof(int), g_stream);
        if (e == hipSuccess) e = hipMemsetAsync(plan.slot, 0, (slots + kPad) * sizeof(unsigned short), g_stream);
        if (e != hipSuccess) { fail("x-window plan: allocation failed: %s", hipGetErrorString(e)); break; }
        hipLaunchKernelGGL((plan_fill<SHIFT>), dim3(W), dim3(kBlock), 0, g_stream, W, d_begin, d_len, idx, d_off,
                           plan.lines, plan.slot);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) { fail("x-window plan: fill pass failed: %s", hipGetErrorString(e)); break; }
        if (upload_array(&plan.ldesc4, win.data(), win.size(), 1) || upload_array(&plan.ldesc, h_ldesc.data(), h_ldesc.size(), 1))
            break;
        plan.blocks = W;
        plan.lines_listed = plan.lines_stored = total;
        plan.slots = (long long)slots;
        plan.stage_lines = std::max(kLocalLineQuantum, (widest + kLocalLineQuantum - 1) / kLocalLineQuantum * kLocalLineQuantum);
        result = 1;
    } while (0);
    for (void *p : {(void *)d_begin, (void *)d_len, (void *)d_n, (void *)d_off}) (void)hipFree(p);
    if (result != 1) plan.release();
    return result;
}

// The pattern plan's tables (plan_kernels.hpp: pat_mark, pat_fill) of the x-window plan `xw` over its 16-bit slots, a
// row's slots found through row_ptr, or through the plan's row_seg (ROW_SEG: HLL windows); `slots` of the handle's `rows`
// rows.  auto: built for streamed handles (the `nt` threshold) of at least 12 slots per row, and only where the tables
// hold at most a quarter of the slots.  Returns the elements of every block's table; xw.pat.ptab == nullptr: no plan
// (not wanted, or it could not be built -- then nothing is left of it and the last HIP error is cleared).
template <bool ROW_SEG, typename D>
std::vector<int> build_pattern_tables(XWindowPlan<D> &xw, int rows, long long slots, int value_bytes, const int *row_ptr) {
    PatternPlan &pat = xw.pat;
    const int blocks = xw.blocks;
    const unsigned *row_seg = xw.row_seg;
    std::vector<int> count;
    if (g_local_patterns == 0 || blocks <= 0 || rows <= 0 || !xw.ldesc4 || !xw.slot || (!row_ptr && !row_seg)) return count;
    if (g_local_patterns < 0 && (slots * (value_bytes + 2LL) <= (128LL << 20) || slots < 12LL * rows)) return count;
    int *rowflag = nullptr, *pcount = nullptr;
    long long *pbase = nullptr;
    hipError_t e = hipMalloc((void **)&rowflag, (size_t)rows * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&pcount, (size_t)blocks * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&pbase, (size_t)blocks * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(rowflag, 0, (size_t)rows * sizeof(int), g_stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((pat_mark<256, ROW_SEG>), dim3(blocks), dim3(256), 0, g_stream, blocks, xw.ldesc4, row_ptr, xw.slot,
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
            hipLaunchKernelGGL((pat_fill<256, ROW_SEG>), dim3(blocks), dim3(256), 0, g_stream, blocks, xw.ldesc4, row_ptr,
                               xw.slot, rowflag, pbase, pat.rinfo, pat.ptab, pat.pdesc, row_seg);
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

// Every distinct span of `data` stored once (plan_kernels.hpp, shared spans).  desc[b] = {first element, elements} of
// block b's span ({.., 0}: none, left alone); relative: spans count from their first element, which goes to *base
// ([blocks], allocated here).  The spans are hashed on the device, equal (length, hash) keys grouped on the host, the
// first block of a group its canonical; a block whose span is not the canonical's word for word keeps its own copy.
// `data` is replaced by the compacted array (`pad` zeroed elements behind it) and desc rewritten; stored / distinct:
// its elements and its spans.  False: a HIP failure -- the plan is what it was and the last error is cleared.
template <typename E>
bool share_spans(E *&data, int2 *desc, int blocks, size_t pad, bool relative, bool weak, int **base, long long &stored,
                 long long &distinct) {
    static_assert(sizeof(E) % 4 == 0, "spans are compared in 32-bit words");
    constexpr int words = (int)(sizeof(E) / 4);
    const size_t B = (size_t)blocks;
    std::vector<int2> h_desc(B), keep;
    std::vector<unsigned long long> h_hash(B);
    std::vector<int> canon(B, -1), differs(B, 0), order;
    unsigned long long *d_hash = nullptr;
    int *d_base = nullptr, *d_canon = nullptr, *d_differs = nullptr;
    int2 *d_keep = nullptr;
    E *fresh = nullptr;
    long long total = 0;
    const unsigned *words_in = reinterpret_cast<const unsigned *>(data);
    hipError_t e = hipMalloc((void **)&d_hash, B * sizeof(unsigned long long));
    if (e == hipSuccess && relative) e = hipMalloc((void **)&d_base, B * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_canon, B * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_differs, B * sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(d_differs, 0, B * sizeof(int), g_stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((share_hash<256>), dim3(blocks), dim3(256), 0, g_stream, blocks, desc, words_in, words,
                           relative ? 1 : 0, weak ? 1 : 0, d_hash, d_base);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_hash.data(), d_hash, B * sizeof(unsigned long long), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_desc.data(), desc, B * sizeof(int2), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e == hipSuccess) {
        for (int b = 0; b < blocks; ++b)
            if (h_desc[(size_t)b].y > 0) order.push_back(b);
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            if (h_desc[(size_t)a].y != h_desc[(size_t)b].y) return h_desc[(size_t)a].y < h_desc[(size_t)b].y;
            if (h_hash[(size_t)a] != h_hash[(size_t)b]) return h_hash[(size_t)a] < h_hash[(size_t)b];
            return a < b;
        });
        for (size_t k = 0; k < order.size(); ++k) {
            const int b = order[k], p = k ? order[k - 1] : -1;
            const bool same = p >= 0 && h_desc[(size_t)p].y == h_desc[(size_t)b].y && h_hash[(size_t)p] == h_hash[(size_t)b];
            canon[(size_t)b] = same ? canon[(size_t)p] : b;
        }
        e = hipMemcpyAsync(d_canon, canon.data(), B * sizeof(int), hipMemcpyHostToDevice, g_stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL((share_verify<256>), dim3(blocks), dim3(256), 0, g_stream, blocks, desc, words_in, words,
                           relative ? 1 : 0, d_canon, d_differs);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(differs.data(), d_differs, B * sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e == hipSuccess) {
        // the kept spans in block order (a canonical is the first block of its group: it comes before its sharers)
        for (int b = 0; b < blocks; ++b) {
            int2 &d = h_desc[(size_t)b];
            if (d.y <= 0) continue;
            if (canon[(size_t)b] == b || differs[(size_t)b]) {
                canon[(size_t)b] = b;
                keep.push_back(make_int2(b, (int)total));
                total += d.y;
            }
        }
        e = hipMalloc((void **)&fresh, ((size_t)total + pad) * sizeof(E));
        if (e == hipSuccess && pad) e = hipMemsetAsync(fresh + total, 0, pad * sizeof(E), g_stream);
        if (e == hipSuccess) e = hipMalloc((void **)&d_keep, std::max<size_t>(keep.size(), 1) * sizeof(int2));
        if (e == hipSuccess && !keep.empty())
            e = hipMemcpyAsync(d_keep, keep.data(), keep.size() * sizeof(int2), hipMemcpyHostToDevice, g_stream);
    }
    if (e == hipSuccess && !keep.empty()) {
        hipLaunchKernelGGL((share_gather<256>), dim3((unsigned)keep.size()), dim3(256), 0, g_stream, (int)keep.size(), d_keep,
                           desc, words_in, words, relative ? 1 : 0, reinterpret_cast<unsigned *>(fresh));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e == hipSuccess) {
        // (the descriptors last: until here the plan is untouched)
        for (const int2 &k : keep) h_desc[(size_t)k.x].x = k.y;
        for (int b = 0; b < blocks; ++b)
            if (h_desc[(size_t)b].y > 0) h_desc[(size_t)b].x = h_desc[(size_t)canon[(size_t)b]].x;
        e = hipMemcpy(desc, h_desc.data(), B * sizeof(int2), hipMemcpyHostToDevice);
    }
    for (void *p : {(void *)d_hash, (void *)d_canon, (void *)d_differs, (void *)d_keep}) (void)hipFree(p);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        (void)hipFree(d_base);
        (void)hipGetLastError();
        return false;
    }
    (void)hipFree(data);
    data = fresh;
    if (base) *base = d_base;
    stored = total;
    distinct = (long long)keep.size();
    return true;
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
template <typename Launch>
void tune_pattern_plan(PatternPlan &pat, Launch launch) {
    UploadTimer timer;
    if (!timer.ok) return;
    auto measure = [&](int patterns, float &us) {
        const int keep = g_local_patterns;
        g_local_patterns = patterns;
        const bool ok = timer.time(launch, us);
        g_local_patterns = keep;
        return ok;
    };
    bool ok = true;
    for (int round = 0; round < 2 && ok; ++round) {
        float a = 0, b = 0;
        ok = measure(1, a) && measure(0, b);
        pat.with_us = round ? std::min(pat.with_us, a) : a;
        pat.without_us = round ? std::min(pat.without_us, b) : b;
    }
    if (!ok || pat.with_us > 0.98f * pat.without_us) pat.release();  // not faster here: the slot stream stays
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

// The searches of a finished handle, in this order: settle, the pattern plan (auto), the placement of the
// value array *val (`bytes` long; val == nullptr: the handle's kernel does not stream it, or it is below
// kPlaceMinBytes).  launch() runs the handle's own kernel.  None is ever a reason to lose the handle.
template <typename H, typename V, typename Launch>
void upload_searches(H *m, V **val, size_t bytes, Launch launch) {
    const bool patterns = g_local_patterns < 0 && m->xw.pat.ptab;
    const bool place = val && *val && g_place_tries > 0;
    if (patterns || place) upload_settle(launch);
    if (patterns) tune_pattern_plan(m->xw.pat, launch);
    if (place) tune_placement(m, *val, bytes, launch);
}

}  // namespace
