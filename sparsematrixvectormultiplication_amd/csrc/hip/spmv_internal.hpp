// spmv_internal.hpp -- what the translation units behind include/spmv_hip.h share: error
// reporting, library state, the two device handles, upload helpers and the timing loops.
// Not installed; nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "csr_kernels.hpp"
#include "hll_kernels.hpp"
#include "tile_kernels.hpp"
#include "row_counts.hpp"
#include "tuning.hpp"  // the tuning knobs, g_stream_cap .. g_stream_local
#include "spmv_hip.h"

using namespace spmv;

// ------------------------------------------------------------------ state (spmv_device.hip)
extern int g_device;
extern hipStream_t g_stream;
extern hipStream_t g_stream2;  // second stream: the halo exchange that runs beside the interior blocks
extern ncclComm_t g_comm;
extern int g_comm_rank, g_comm_size;
constexpr int kMaxRanks = 64;  // widest communicator: the all-gatherv's bounds, the solvers' gathered sums

extern bool g_halo_ready;     // spmv_hip_comm_halo_setup has made this rank's send / receive segments
constexpr long long kTileMidEntries = 4LL << 20;  // (auto) entries from which a scattered plan's middle tier, or a band of dense rows (packed plans only), gets a tier
constexpr long long kSplitMinEntries = 1LL << 20;  // entries from which rows may be handed to the split-row kernels (two more launches)
constexpr long long kTileMinRows = 800000;  // (auto) rows from which a handle without an x-window plan gets a tile plan
extern int g_num_cus;

int fail(const char *fmt, ...);  // records the message for spmv_hip_last_error(), returns -1
int need_device();               // 0, or -1 when spmv_hip_init() has not succeeded

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t err__ = (expr);                                                        \
        if (err__ != hipSuccess)                                                          \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), __FILE__, \
                        __LINE__);                                                        \
    } while (0)

#define NCCL_TRY(expr)                                                                     \
    do {                                                                                   \
        ncclResult_t err__ = (expr);                                                       \
        if (err__ != ncclSuccess)                                                          \
            return fail("%s failed: %s (%s:%d)", #expr, ncclGetErrorString(err__), __FILE__, \
                        __LINE__);                                                         \
    } while (0)

// The C-ABI never lets a C++ exception cross into the caller: host-side packing uses std::vector,
// whose allocation failure (a matrix too large for host memory) becomes -1 + message like any other.
template <typename F>
int guarded(const char *what, F body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail("%s: out of host memory", what);
    } catch (const std::exception &e) {
        return fail("%s: %s", what, e.what());
    }
}

constexpr int kRowPtrPad = 384;  // entries behind row_ptr (kernels that stage whole row_ptr segments)
// (kPad, the zero entries behind col/val: row_counts.hpp)

template <typename T>
int upload_array(T **dptr, const T *host, size_t count, size_t pad) {
    HIP_TRY(hipMalloc((void **)dptr, (count + pad) * sizeof(T)));
    if (count) HIP_TRY(hipMemcpy(*dptr, host, count * sizeof(T), hipMemcpyHostToDevice));
    if (pad) HIP_TRY(hipMemset(*dptr + count, 0, pad * sizeof(T)));
    return 0;
}

// SPMV_TRACE_UPLOAD=1: where an upload spends its time, phase by phase, on stderr (tools/time_upload.py).
// mark(name) closes the phase that began at the previous mark (the device is synchronised first, so device work is
// charged to the phase that launched it).
struct UploadTrace {
    bool on;
    double t_last;
    const char *who;
    static double now() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    }
    explicit UploadTrace(const char *name) : on(getenv("SPMV_TRACE_UPLOAD") != nullptr), t_last(0), who(name) {
        if (on) t_last = now();
    }
    void mark(const char *phase) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const double t = now();
        fprintf(stderr, "[upload trace] %-18s %-34s %8.1f ms\n", who, phase, (t - t_last) * 1e3);
        t_last = t;
    }
};

inline int pow2_floor(int v) {
    int p = 1;
    while (p * 2 <= v) p *= 2;
    return p;
}

// The row-sum phase of the stream / LDS kernels gives every row of a block the same number of lanes, sized by the
// NUMBER of rows in the block (lanes_for_rows in csr_kernels.hpp; mirrored here for the host).  One row of hundreds of
// entries in a block of hundreds of short rows is then summed by a single lane while the other 255 wait (circuit
// matrices: adder_dcop_32-size stand-in 11.5 us where one launch costs 6.3).  Upload therefore closes a block before a
// row -- or before more rows join a long one -- whenever some lane would have to add up more than kSkewPerLane entries:
// the long row ends up in a block of few rows and gets 8..64 lanes.  Uniform matrices never get there (rows x length
// <= stage, so length / lanes <= 32).
constexpr int kSkewPerLane = 64;
inline int host_lanes_for_rows(int nrows) {
    if (nrows > kBlock / 2 || nrows <= 0) return 1;
    return std::min(64, pow2_floor(kBlock / nrows));
}
inline bool skew_cut(int nrows, int maxlen, int len) {
    if (nrows <= 0) return false;  // a block always takes its first row
    return std::max(maxlen, len) / host_lanes_for_rows(nrows + 1) > kSkewPerLane;
}

// ---------------------------------------------------------------- handles
namespace spmv {
struct TileExpansion;  // tile_plan_device.hpp
}
// The pattern plan of an x-window plan (csr_kernels.hpp, PAT; hll_lds_local<.., PAT>): where most rows of the blocks are
// their predecessor shifted by a constant, the kernel rebuilds the slots instead of reading the 16-bit slot stream -- from
// one segment per block (its rows' records and its pattern groups, copied into LDS), or, for a block whose segment is
// wider than the LDS budget, from its table.  Built and timed at upload (upload_ops.hpp); HLL has the tables only.
struct PatternPlan {
    unsigned short *ptab = nullptr;   // [slots + pad] the blocks' pattern tables
    unsigned *rinfo = nullptr;        // [rows] start of the row's pattern in its block's table | shift << 16
    int2 *pdesc = nullptr;            // [blocks] {first element in ptab (even), elements}
    uint4 *pseg = nullptr;            // [seg_total] the segments, 16-byte units (nullptr: no block's fits)
    int2 *sdesc = nullptr;            // [blocks] {first uint4 of the block's segment, uint4s}; {0, 0}: the table
    long long slots = 0;              // elements of all tables
    int widest = 0;                   // the largest table (elements)
    long long seg_total = 0;          // uint4s of all segments
    int seg_max = 0;                  // the widest segment kept (uint4s): the LDS the kernel adds behind the slots
    int seg_cap = 0;                  // the widest segment the LDS budget allowed (uint4s)
    long long table_rows = 0;         // rows of the blocks whose segment did not fit (they read rinfo, row_ptr and ptab)
    long long seg_distinct = 0;       // segments stored: equal ones are stored once (share_spans), sdesc points many blocks at one
    float with_us = 0, without_us = 0;  // (auto) the kernel with / without the plan, timed at upload (tune_pattern_plan)

    size_t bytes(long long rows, long long blocks) const {
        if (!ptab) return 0;
        return ((size_t)slots + 1024) * 2 + (size_t)rows * 4 + (size_t)blocks * 8 +
               (pseg ? (size_t)seg_total * sizeof(uint4) + (size_t)blocks * sizeof(int2) : 0);
    }
    // the arrays and what describes them; seg_cap and the timings stay for info()
    void release() {
        for (void *p : {(void *)ptab, (void *)rinfo, (void *)pdesc, (void *)pseg, (void *)sdesc}) (void)hipFree(p);
        ptab = nullptr;
        rinfo = nullptr;
        pdesc = nullptr;
        pseg = nullptr;
        sdesc = nullptr;
        slots = 0;
        seg_total = 0;
        seg_max = 0;
        table_rows = 0;
        seg_distinct = 0;
    }
};
// What a host builder of the x-window plan makes (csr_build_local, spmv_csr.hip; hll_build_local, spmv_hll.hip): blocks cut
// like the gather kernel's with one more limit, the number of distinct x lines (128 bytes of x each) a block touches.
// Per block the ascending list of those lines, per entry its 16-bit slot (rank of its line in the list * elements per
// line + column % elements per line).  Desc: the kernel's line descriptor, as in XWindowPlan.
template <typename Desc>
struct LocalPlan {
    std::vector<unsigned char> split;  // CSR: rows handed to the split-row kernels (too many x lines)
    std::vector<int4> desc;
    std::vector<Desc> ldesc;
    std::vector<int> lines;            // kLocalLinesMax zeros behind the last list
    std::vector<unsigned short> lcol;  // [slots + kPad]
    int stage_lines = 0;
};
// how an x-window kernel is launched over some of a plan's blocks (XWindowPlan::launch_shape)
struct XWindowLaunch {
    int chunk, grid;      // blocks per XCD run; workgroups: whole runs on all 8 XCDs (one past the last block returns at once)
    size_t lds, pat_lds;  // dynamic LDS without / with the pattern plan: the stage; behind it the slots and the widest segment
    bool nt, patterns;    // non-temporal loads of the streamed arrays; the PAT instantiation
};
// The x-window plan of a handle (csr_stream_local, hll_lds_local): own blocks whose x lines are staged in LDS, every entry
// a 16-bit slot in its block's staged lines.  One type for both handles; Desc is the kernel's line descriptor: int2
// {first line in `lines`, lines} for CSR, int4 {first line, lines, slots of the window from its even base, 0} for HLL.
// The arrays are listed ONCE, in arrays(): release() frees that list, bytes() is what they were allocated with.
template <typename Desc>
struct XWindowPlan {
    int4 *ldesc4 = nullptr;           // [blocks] CSR: like desc; HLL: like hdesc
    Desc *ldesc = nullptr;            // [blocks]
    int *lines = nullptr;             // [lines_stored + kLocalLinesMax] x line ids, block after block, ascending inside a block
    int *lbase = nullptr;             // [blocks] shared line lists ("local_share"): a block's list counts from its first
                                      // line, lbase[b]; equal lists are stored once.  nullptr: the lists hold absolute ids
    unsigned short *slot = nullptr;   // [slots + kPad] slot of each entry in its block's staged lines
    unsigned *row_seg = nullptr;      // HLL: [rows] a row's (first slot in its window | slots << 16)
    PatternPlan pat;                  // the pattern plan of the blocks (the kernel then does not read `slot`)
    int blocks = 0;                   // 0: no plan (not profitable / not possible)
    int stage_lines = 0;              // LDS stage: most lines any block lists, in steps of 32
    long long lines_listed = 0;       // line ids the blocks list ...
    long long lines_stored = 0;       // ... and those `lines` holds: fewer once equal lists are shared
    long long lists_stored = 0;       // the distinct lists then; 0: every block has its own
    long long slots = 0;              // entries `slot` was allocated for

    std::array<void **, 6> arrays() {
        return {(void **)&ldesc4, (void **)&ldesc, (void **)&lines, (void **)&lbase, (void **)&slot, (void **)&row_seg};
    }
    void release() {
        for (void **p : arrays()) (void)hipFree(*p);
        pat.release();
        *this = XWindowPlan();
    }
    // what the plan holds on the device, with the pads it was allocated with (rows: the handle's)
    size_t bytes(long long rows) const {
        if (!ldesc4) return 0;
        return (size_t)blocks * (16 + sizeof(Desc) + (lbase ? 4 : 0)) + ((size_t)lines_stored + kLocalLinesMax) * 4 +
               ((size_t)slots + kPad) * 2 + (row_seg ? (size_t)rows * 4 : 0) + pat.bytes(rows, blocks);
    }
    // a host-built plan to the device; -1: HIP error (what is allocated by then goes with the handle)
    int upload(const LocalPlan<Desc> &p) {
        if (upload_array(&ldesc4, p.desc.data(), p.desc.size(), 1) || upload_array(&ldesc, p.ldesc.data(), p.ldesc.size(), 1) ||
            upload_array(&lines, p.lines.data(), p.lines.size(), 0) || upload_array(&slot, p.lcol.data(), p.lcol.size(), 0))
            return -1;
        blocks = (int)p.desc.size();
        stage_lines = p.stage_lines;
        lines_listed = lines_stored = (long long)p.lines.size() - kLocalLinesMax;
        slots = (long long)p.lcol.size() - kPad;
        return 0;
    }
    // the launch over `count` of the blocks, at a stage of `cap` entries of value_bytes each; entries: the handle's
    XWindowLaunch launch_shape(int count, int cap, int value_bytes, long long entries) const {
        XWindowLaunch L;
        // runs of 16 neighbouring blocks per XCD: each L2 keeps its own window of x lines
        // (measured flat from 8 to 128 on three matrices); stream_xcd overrides
        L.chunk = g_stream_xcd < 0 ? (count + 7) / 8 : (g_stream_xcd ? g_stream_xcd : 16);
        const int round = 8 * L.chunk;
        L.grid = round > 0 ? (count + round - 1) / round * round : count;
        L.lds = std::max((size_t)cap * (size_t)value_bytes, (size_t)stage_lines * kLineBytes);
        // a pattern plan: the slots are rebuilt in LDS (behind the stage) from the block's segment or table, not read
        // entry by entry
        L.patterns = pat.ptab && g_local_patterns != 0;
        L.pat_lds = L.lds + ((size_t)cap + 8) * sizeof(unsigned short) + (size_t)pat.seg_max * sizeof(uint4);
        // streamed-once hint only when the matrix cannot live in the 256 MiB Infinity Cache anyway
        // (cant-like, 53 MB: 10.9 us without it, 11.7 us with; fem-large: 160 vs 151 us)
        L.nt = g_local_nt < 0 ? entries * (value_bytes + 2LL) > (128LL << 20) : g_local_nt != 0;
        return L;
    }
};
// The tile plans of a handle (csr_tile, tile_kernels.hpp): up to three tiers of the same kind of plan, launched by the
// same kernel.  TileTier is what every tier has; each tier lists its device arrays ONCE, in arrays(): release() frees
// that list and the digest (csr_tile_digest) hashes it, so an array cannot be in one and not in the other.
struct TileArr {
    void *p;
    size_t count, elem;  // elements and bytes per element for the digest; elem 0: scratch or derived, freed but not digested
};
struct TileTier {
    int *tcol = nullptr;              // [padded + kTileChunkMax]
    unsigned short *tkey = nullptr;
    void *tval = nullptr;
    int4 *pass = nullptr;             // [passes] (the ordinary tiles: in stream order)
    int *block_row = nullptr;         // [blocks + 1] first row of every block
    int *block_pass = nullptr;        // [blocks + 1] (the ordinary tiles: [streams + 1], first pass of every stream)
    int blocks = 0;                   // 0: no tiles
    int rows_per_block = 0;
    int passes = 0;
    int max_win = 0;                  // widest staged window (columns)
    long long entries = 0, padded = 0, staged = 0, staged_cols = 0;
    bool packed = false;              // stageable passes hold packed column words (kernel instantiation with the decode)

    // the entry arrays and the pass descriptors, as every tier's digest begins (live: the tier exists; vb: bytes per value)
    std::vector<TileArr> entry_arrays(bool live, size_t vb) const {
        const size_t pad = live ? (size_t)padded + kTileChunkMax : 0;
        // (a packed plan's keys: padding only)
        return {{tcol, pad, 4}, {tkey, packed ? (pad ? (size_t)kTileChunkMax : 0) : pad, 2}, {tval, pad, vb}, {pass, (size_t)passes, 16}};
    }
    static void free_all(const std::vector<TileArr> &arrs) {
        for (const TileArr &a : arrs) (void)hipFree(a.p);
    }
};
// the ordinary tiles: 2-D tiles (row-block accumulators in LDS x column passes), for matrices without an x-window plan
struct OwnTiles : TileTier {
    int lds_min = 0;                  // LDS bytes to ask for at least (scattered matrices: one workgroup per CU)
    int rem_rows = 0;                 // rows with remainder entries (windows too sparse for a pass), tile_remainder
    long long rem_entries = 0;
    int *rem_row = nullptr, *rem_ptr = nullptr, *rem_col = nullptr;  // [rows], [rows + 1], [entries]
    void *rem_val = nullptr;
    int streams = 0;                  // workgroups of the csr_tile launch: each walks the blocks of one stream
    int *stream_block = nullptr;      // [streams + 1] first block (in sblock_rows) of every stream
    int2 *sblock_rows = nullptr;      // [blocks] {first row, rows} in stream order
    // the expansion of x for a plan with gather passes (round 3; tile_kernels.hpp, XE): x value per tile entry, written
    // by tile_expand ahead of every csr_tile launch of this handle, and what tile_expand walks
    void *xe = nullptr;               // [padded + kTileChunkMax]
    spmv::TileExpansion *expansion = nullptr;
    int4 *long_rows = nullptr;        // rows beyond the tile limit {row, first slot, pieces, 0} ...
    int4 *pieces = nullptr;           // ... and their pieces, cut at column stripes, stripe by stripe
    int num_long = 0, num_pieces = 0;

    std::vector<TileArr> arrays(size_t vb = 0) const {
        std::vector<TileArr> a = entry_arrays(blocks > 0, vb);
        const size_t per_stream = blocks > 0 ? (size_t)streams + 1 : 0;
        a.insert(a.end(), {{block_pass, per_stream, 4}, {block_row, blocks > 0 ? (size_t)blocks + 1 : 0, 4}, {stream_block, per_stream, 4},
                           {sblock_rows, (size_t)blocks, 8}, {rem_row, (size_t)rem_rows, 4}, {rem_ptr, rem_rows > 0 ? (size_t)rem_rows + 1 : 0, 4},
                           {rem_col, (size_t)rem_entries, 4}, {rem_val, (size_t)rem_entries, vb}, {xe, 0, 0}, {long_rows, 0, 0}, {pieces, 0, 0}});
        return a;
    }
    void release();  // spmv_csr.hip (the expansion is a complete type there)
};
// a compacted tier: rows picked out of the matrix into row blocks of their own; a block's passes are dealt out to
// several workgroups (work items), each leaves its accumulators in a slab
struct CompactTiles : TileTier {
    int rows = 0, items = 0;
    int4 *work = nullptr;
    int *item_first = nullptr, *row_map = nullptr, *block_of_row = nullptr;
    void *slab = nullptr;

    std::vector<TileArr> arrays(size_t vb = 0) const {
        std::vector<TileArr> a = entry_arrays(items > 0, vb);
        const size_t per_block = items > 0 ? (size_t)blocks + 1 : 0;
        a.insert(a.end(), {{block_row, per_block, 4}, {block_pass, per_block, 4}, {work, (size_t)items, 16}, {item_first, per_block, 4},
                           {row_map, (size_t)rows, 4}, {block_of_row, (size_t)rows, 4}, {slab, 0, 0}});
        return a;
    }
    void release() {
        free_all(arrays());
        *this = CompactTiles();
    }
};
// What a handle keeps from its first spmv_hip_csr_update_values on (spmv_update.hip): for each of the four arrays that
// hold matrix values in the tile plans' order -- tile.tval, tile.rem_val, lt.tval, mt.tval -- the source map, one int per
// slot: the entry of `val` the slot holds, -1 for a padding slot.  A handle that is never updated has none.
struct UpdateState {
    int *src[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t slots[4] = {0, 0, 0, 0};  // a tier's `padded` (a multiple of 4: passes start on multiples of 4), the remainder's entries
    bool mapped = false;             // the analysis has run (a handle without tile plans: nothing to map)
    long long updates = 0;
    size_t map_bytes = 0;
    float map_build_us = 0, last_us = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;  // around the last update's device work; read by spmv_hip_csr_update_info
    bool timed = false;
    ~UpdateState() {
        for (int *p : src) (void)hipFree(p);
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};
struct spmv_csr_dev {
    UpdateState *upd = nullptr;  // spmv_hip_csr_update_values' state; nullptr until the first update
    int value_bytes = 8;
    int M_local = 0, M_total = 0, N = 0, row0 = 0;
    long long nz = 0;
    int *row_ptr = nullptr;  // [M_local + 1], rebased to 0
    int *col = nullptr;
    void *val = nullptr;
    void *x = nullptr;  // [N]
    void *y = nullptr;  // [M_total]
    // stream kernel
    int4 *desc = nullptr;
    int num_blocks = 0;
    int4 *long_rows = nullptr;
    int num_long = 0;
    int4 *pieces = nullptr;
    void *partial = nullptr;
    int num_partial = 0;
    void *spmm_partial = nullptr;  // the k-wide partial sums of the pieces for SpMM (spmv_spmm.hip): grows only
    size_t spmm_partial_bytes = 0;
    int stream_cap = 2048;
    // stream kernel with the x window in LDS (csr_stream_local): own blocks, 16-bit local columns
    XWindowPlan<int2> xw;
    int local_cap = 2048;
    // N4 overlap: x-window blocks whose listed x lines all lie in this handle's own range of x (interior) / the rest
    int *interior_ids = nullptr, *boundary_ids = nullptr;
    int num_interior = 0, num_boundary = 0;
    bool have_split = false;
    // N4 overlap below block granularity (round 3): the handle's entries split by COLUMN -- own_part holds those whose
    // column lies in the rank's own range of x (it can run before the halo has arrived), halo_part the rest; two
    // sub-handles over the same rows, launched on this handle's vectors (spmv_hip_csr_split_columns)
    spmv_csr_dev *own_part = nullptr, *halo_part = nullptr;
    long long own_entries = 0, halo_entries = 0;
    bool tiles_only = false;  // a handle made of tile plans alone (the tile side of an HLL handle): STREAM only
    OwnTiles tile;     // csr_tile plan of a handle without an x-window plan
    CompactTiles lt;   // rows beyond tile_lmax (2048 compacted rows per block)
    CompactTiles mt;   // (round 3) the MIDDLE tier of a scattered matrix, rows of tile_mid_lo < entries <= tile_lmax in blocks
                       // as tall as the LDS takes, so that their column ranges hold enough entries to be staged as well
    // heuristics
    int lanes_per_row = 16;
    int auto_variant = SPMV_CSR_STREAM;
    int max_row = 0;
    size_t rest_bytes = 0;  // device memory but the x-window plan's (csr_device_bytes)
    int place_tries = 0;  // placement tuning at upload (tune_placement): placements timed, first / kept time
    float place_first_us = 0, place_best_us = 0;
    // arrays moved to a chosen address (spmv_hip_csr_relocate): the field points INTO `raw`, which is what gets freed
    // (vmm: the memory came from hipMemCreate + hipMemAddressReserve + hipMemMap, `raw` is the reserved range)
    struct relocated { void **field; void *raw; size_t size; bool vmm = false; hipMemGenericAllocationHandle_t phys = {}; size_t mapped = 0; };
    std::vector<relocated> relocs;
};

// what info() reports as device_bytes: the x-window plan's bytes and the rest of the handle's
inline size_t csr_device_bytes(const spmv_csr_dev *m) { return m->rest_bytes + m->xw.bytes(m->M_local); }

struct spmv_hll_dev {
    int M = 0, N = 0, hacks = 0;  // rows / hacks HELD by this handle
    int M_total = 0, row0 = 0;    // rows of the whole matrix (length of y), first global row (multiple of 32)
    long long nz_hint = 0;
    long long slots = 0;
    long long *hack_off = nullptr;  // [hacks + 1]
    int *maxnz = nullptr;           // [hacks]
    int *JA = nullptr;
    double *AS = nullptr;
    int4 *hdesc = nullptr;  // [num_blocks] {first row, rows, first slot lo, first slot hi}
    int num_blocks = 0;
    int stage_slots = kHllCap;  // LDS stage of hll_lds: the largest workgroup, <= kHllCap
    int *long_windows = nullptr;  // [num_long_windows] hdesc windows of one row longer than the stage (SpMM: hll_spmm_row)
    int num_long_windows = 0;
    // hll_lds_local (x window in LDS): own windows, 16-bit local JA; row_seg is filled, the pattern plan has tables only
    XWindowPlan<int4> xw;
    spmv_csr_dev *tiles = nullptr; // csr_tile over the slab's rows (padding slots included), when the slab gets no x-window plan
    double *x = nullptr;
    double *y = nullptr;
    int lanes_per_row = 8;
    int auto_variant = SPMV_HLL_LDS;
    size_t rest_bytes = 0;  // device memory but the x-window plan's and the tile handle's (hll_device_bytes)
    int place_tries = 0;  // placement tuning at upload (tune_placement)
    float place_first_us = 0, place_best_us = 0;
};

inline size_t hll_device_bytes(const spmv_hll_dev *m) {
    return m->rest_bytes + m->xw.bytes(m->M) + (m->tiles ? csr_device_bytes(m->tiles) : 0);
}

// spmv_csr.hip: a handle around device arrays that already hold the matrix (ownership passes to the handle
// on success only); col / val carry kPad zeroed entries behind the last one
int csr_adopt_f64(int M, int N, const int *row_ptr_host, int *d_col, double *d_val, spmv_csr_dev **out);
int csr_adopt_f32(int M, int N, const int *row_ptr_host, int *d_col, float *d_val, spmv_csr_dev **out);
// ... by the value type
template <typename T>
int csr_adopt(int M, int N, const int *row_ptr_host, int *d_col, T *d_val, spmv_csr_dev **out) {
    if constexpr (sizeof(T) == 8) return csr_adopt_f64(M, N, row_ptr_host, d_col, d_val, out);
    else return csr_adopt_f32(M, N, row_ptr_host, d_col, d_val, out);
}
// device memory freed on every way out of a function
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
    template <typename U> U *as() const { return static_cast<U *>(p); }
};
// Bare CSR arrays on the device, not a handle (no plans, no vectors), in two roles.  CsrView looks at arrays that belong
// to someone else -- a handle (csr_view) or a DevCsr (view()): what the product, sum and transpose cores take.  DevCsr
// owns its arrays and frees them when it goes: what the cores hand back, and what the AMG device setup
// (spmv_amg_setup.hip) keeps of a level.
struct CsrView {
    int rows = 0, cols = 0;
    long long nz = 0;
    const int *rp = nullptr, *col = nullptr;  // [rows + 1], [nz]
    const void *val = nullptr;
};
inline CsrView csr_view(const spmv_csr_dev *m) { return {m->M_total, m->N, m->nz, m->row_ptr, m->col, m->val}; }
// does the handle hold the arrays csr_view shows?  (a handle made of tile plans alone does not)
inline bool csr_holds_arrays(const spmv_csr_dev *m) {
    return !m->tiles_only && m->row_ptr && (m->nz == 0 || (m->col && m->val));
}
// what the triangular and the preconditioner builds ask of a handle; else -1 with a message naming `what`
inline int handle_ok(const spmv_csr_dev *m, const char *what) {
    if (m->M_total != m->N) return fail("%s: needs a square matrix (%d x %d)", what, m->M_total, m->N);
    if (!csr_holds_arrays(m)) return fail("%s: the handle does not hold its CSR arrays", what);
    return 0;
}
struct DevCsr {
    int rows = 0, cols = 0;
    long long nz = 0;
    int *rp = nullptr, *col = nullptr;  // [rows + 1], [nz + the pad they were allocated with]
    void *val = nullptr;
    DevCsr() = default;
    DevCsr(int rows_, int cols_) : rows(rows_), cols(cols_) {}
    DevCsr(DevCsr &&o) noexcept { *this = std::move(o); }
    DevCsr &operator=(DevCsr &&o) noexcept {  // (a swap: what this held goes with o)
        std::swap(rows, o.rows), std::swap(cols, o.cols), std::swap(nz, o.nz);
        std::swap(rp, o.rp), std::swap(col, o.col), std::swap(val, o.val);
        return *this;
    }
    ~DevCsr() { (void)hipFree(rp), (void)hipFree(col), (void)hipFree(val); }
    CsrView view() const { return {rows, cols, nz, rp, col, val}; }
    hipError_t alloc_rp() { return hipMalloc((void **)&rp, std::max<size_t>(((size_t)rows + 1) * sizeof(int), 16)); }
    // col and val for n entries of type T at their exact size, with `pad` zeroed entries behind (kPad: ready for csr_adopt)
    template <typename T>
    hipError_t alloc_entries(long long n_entries, size_t pad, hipStream_t s) {
        const size_t n = (size_t)n_entries;
        nz = n_entries;
        hipError_t e = hipMalloc((void **)&col, std::max<size_t>((n + pad) * sizeof(int), 16));
        if (e == hipSuccess) e = hipMalloc(&val, std::max<size_t>((n + pad) * sizeof(T), 16));
        if (e == hipSuccess && pad) e = hipMemsetAsync(col + n, 0, pad * sizeof(int), s);
        if (e == hipSuccess && pad) e = hipMemsetAsync(static_cast<T *>(val) + n, 0, pad * sizeof(T), s);
        return e;
    }
    void entries_adopted() { col = nullptr, val = nullptr; }  // a handle owns them now (csr_adopt succeeded)
};
// A build's way out: a failed allocation in it is reported by rc, not by the next launch.  Declared ahead of what the
// build allocates, so that it runs behind their frees.
struct ClearHipError {
    ~ClearHipError() { (void)hipGetLastError(); }
};
// spmv_spgemm.hip: C = A B on bare arrays (values of value_bytes bytes; the definition of spmv_hip_csr_spgemm).  On
// success C holds the product (col / val with kPad zeroed entries behind, ready for csr_adopt), rp_host is C's
// row_ptr, stats[8] the stats of spmv_hip_csr_spgemm and ms[0..2] count / symbolic / numeric; on -1 C is as it was.
int spgemm_core(int value_bytes, const CsrView &A, const CsrView &B, int block_products, long long chunk_products, DevCsr &C,
                std::vector<int> &rp_host, long long *stats, double *ms);
int spgemm_max_block_products();  // the cap of the on-chip tier (spgemm_kernels.hpp: kSgMaxProducts)
// block_products as spmv_hip_csr_spgemm takes it: 0 (auto), -1 (no on-chip tier) or a power of two in [64, cap]
inline bool spgemm_block_products_ok(int bp) {
    return bp == 0 || bp == -1 || (bp >= 64 && bp <= spgemm_max_block_products() && (bp & (bp - 1)) == 0);
}
// spmv_transpose.hip: At = A^T on bare arrays, the same way
int transpose_core(int value_bytes, const CsrView &A, DevCsr &At, std::vector<int> &rp_host);
// spmv_spadd.hip: C = alpha a + beta b on bare arrays, the same way (b NULL: alpha canon(a); the arguments, stats[6] and
// ms[0..3] -- check / canonical / symbolic / numeric -- of spmv_hip_csr_add)
int spadd_core(int value_bytes, const CsrView *a, double alpha, const CsrView *b, double beta, int method, int lanes,
               int long_row, DevCsr &C, std::vector<int> &rp_host, long long *stats, double *ms);
// spmv_csr.hip: the line lists of the handle's x-window plan on the host: ld[b] = {first id in `lines`, ids}, base[b] =
// what block b adds to its ids (shared lists count from the block's first line; 0 otherwise)
int csr_lines_to_host(const spmv_csr_dev *m, std::vector<int2> &ld, std::vector<int> &lines, std::vector<int> &base);
int csr_tile_digest(const spmv_csr_dev *m, unsigned long long *out);  // spmv_csr.hip: see spmv_hip_csr_tile_digest
// launchers the timing / exchange code calls across translation units
int csr_launch_any(const spmv_csr_dev *m, int variant, const void *x, void *y, hipStream_t s);
// part 0: the interior x-window blocks only; part 1: everything else (boundary blocks, split rows)
int csr_launch_part(const spmv_csr_dev *m, int part, const void *x, void *y, hipStream_t s);
// column split: part 0: y = A_own x (own range of x only); part 1: y += A_halo x (after the halo has arrived)
int csr_launch_split(const spmv_csr_dev *m, int part, const void *x, void *y, hipStream_t s);
int hll_launch(const spmv_hll_dev *m, int variant, const double *x, double *y_full, hipStream_t s);

// ------------------------------------------------------------------ timing loops
// events around each launch on the stream the kernel runs on
template <typename Launch, typename Zero>
int time_loop(int warmup, int iters, float *ms_each, Launch launch, Zero zero_y) {
    // zero_y() is a no-op when the caller did not ask for the reference's memset
    if (iters <= 0 || !ms_each) return fail("time: iters must be > 0 and ms_each non-NULL");
    // the events are kept from call to call (per device): creating and destroying 2 x iters of them costs ~0.2 ms, which a
    // caller that brackets 20 launches with a wall clock -- bench.py on the driver's command -- sees as 10 us per step
    static std::vector<hipEvent_t> pool;
    static int pool_device = -1;
    int rc = 0;
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !rc) rc = fail("time: %s failed: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    if (pool_device != g_device) {  // (events of another device's context: let them go with it)
        pool.clear();
        pool_device = g_device;
    }
    while (pool.size() < (size_t)iters * 2) {
        hipEvent_t e = nullptr;
        if (!hip_ok(hipEventCreate(&e), "hipEventCreate")) return rc;
        pool.push_back(e);
    }
    hipEvent_t *ev = pool.data();
    for (int i = 0; i < warmup && !rc; ++i) {
        rc = zero_y();
        if (!rc) rc = launch();
    }
    for (int i = 0; i < iters && !rc; ++i) {
        rc = zero_y();
        if (rc) break;
        if (!hip_ok(hipEventRecord(ev[2 * i], g_stream), "hipEventRecord")) break;
        rc = launch();
        if (rc) break;
        if (!hip_ok(hipEventRecord(ev[2 * i + 1], g_stream), "hipEventRecord")) break;
    }
    if (!rc && hip_ok(hipStreamSynchronize(g_stream), "hipStreamSynchronize"))
        for (int i = 0; i < iters; ++i)
            if (!hip_ok(hipEventElapsedTime(&ms_each[i], ev[2 * i], ev[2 * i + 1]), "hipEventElapsedTime")) break;
    return rc;
}

// `iters` back-to-back launches captured once into a hipGraph and replayed `replays` times:
// what a launch-bound loop (small matrices: an 11 us kernel against ~6 us of per-launch host
// work) costs per SpMV when the host is out of the way.  ms_per_iter = mean over the replays.
template <typename Launch>
int graph_loop(int iters, int replays, float *ms_per_iter, Launch launch) {
    if (iters <= 0 || replays <= 0 || !ms_per_iter) return fail("time_graph: bad arguments");
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    hipError_t e = hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return fail("hipStreamBeginCapture failed: %s", hipGetErrorString(e));
    for (int i = 0; i < iters && !rc; ++i) rc = launch();
    e = hipStreamEndCapture(g_stream, &graph);
    if (!rc && e != hipSuccess) rc = fail("hipStreamEndCapture failed: %s", hipGetErrorString(e));
    if (!rc) {
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) rc = fail("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    if (!rc) {
        e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = hipGraphLaunch(exec, g_stream);  // warm-up replay
        if (e == hipSuccess) e = hipEventRecord(e0, g_stream);
        for (int r = 0; r < replays && e == hipSuccess; ++r) e = hipGraphLaunch(exec, g_stream);
        if (e == hipSuccess) e = hipEventRecord(e1, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = fail("graph replay failed: %s", hipGetErrorString(e));
        else *ms_per_iter = ms / ((float)replays * (float)iters);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
}

// one step = this rank's kernel, then the all-gatherv of y (when a communicator exists)
template <typename Launch>
int step_loop(void *y, int value_bytes, const int *bounds, int warmup, int iters, float *ms_kernel,
              float *ms_exchange, Launch launch) {
    if (iters <= 0) return fail("step_time: iters must be > 0");
    // (events kept from call to call, per device: see time_loop)
    static std::vector<hipEvent_t> pool;
    static int pool_device = -1;
    int rc = 0;
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !rc) rc = fail("step_time: %s failed: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    if (pool_device != g_device) {
        pool.clear();
        pool_device = g_device;
    }
    while (pool.size() < (size_t)iters * 3) {
        hipEvent_t e = nullptr;
        if (!hip_ok(hipEventCreate(&e), "hipEventCreate")) return rc;
        pool.push_back(e);
    }
    hipEvent_t *ev = pool.data();
    for (int i = -warmup; i < iters && !rc; ++i) {
        if (i >= 0 && !hip_ok(hipEventRecord(ev[3 * i], g_stream), "hipEventRecord")) break;
        rc = launch();
        if (rc) break;
        if (i >= 0 && !hip_ok(hipEventRecord(ev[3 * i + 1], g_stream), "hipEventRecord")) break;
        if (g_comm) rc = spmv_hip_comm_allgatherv(y, bounds, value_bytes, g_stream);
        if (rc) break;
        if (i >= 0 && !hip_ok(hipEventRecord(ev[3 * i + 2], g_stream), "hipEventRecord")) break;
    }
    if (!rc && hip_ok(hipStreamSynchronize(g_stream), "hipStreamSynchronize")) {
        for (int i = 0; i < iters && !rc; ++i) {
            float a = 0, b = 0;
            if (!hip_ok(hipEventElapsedTime(&a, ev[3 * i], ev[3 * i + 1]), "hipEventElapsedTime")) break;
            if (!hip_ok(hipEventElapsedTime(&b, ev[3 * i + 1], ev[3 * i + 2]), "hipEventElapsedTime")) break;
            if (ms_kernel) ms_kernel[i] = a;
            if (ms_exchange) ms_exchange[i] = b;
        }
    }
    return rc;
}
