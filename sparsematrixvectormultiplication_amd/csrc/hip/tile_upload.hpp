// tile_upload.hpp -- the csr_tile plans of a handle between the matrix and the device: which tiers a matrix gets and how
// they are cut (tile_plan_all over tile_plan.hpp / tile_plan_device.hpp), and how the finished plans reach the handle
// (tile_upload_all).  Included by spmv_csr.hip alone: tile_allow_lds sets an attribute on the csr_tile instantiations of
// that translation unit, the ones launch_csr_tile launches.
#pragma once
#include "spmv_internal.hpp"

#include "tile_plan.hpp"
#include "tile_plan_device.hpp"

namespace {

// Pieces of the rows marked in `split` for a tiled handle: cut where the column crosses a stripe of
// `stripe_cols` columns (and every kLongPiece entries), slots numbered row by row (csr_long_finish adds a
// row's slots in that order), but the pieces themselves ordered stripe by stripe: the launch then sweeps
// x one L2-sized stripe at a time instead of gathering from all of it at once.
void build_striped_pieces(int M, const int *rp, const int *col, const std::vector<unsigned char> &split,
                          int stripe_cols, std::vector<int4> &pieces, std::vector<int4> &long_rows) {
    struct Tagged {
        int stripe;
        int4 d;
    };
    std::vector<Tagged> tmp;
    long_rows.clear();
    for (int r = 0; r < M; ++r) {
        if (!split[r]) continue;
        const int first_slot = (int)tmp.size();
        int e = rp[r];
        const int end = rp[r + 1];
        while (e < end) {
            const int s = col[e] / stripe_cols;
            int f = e + 1;
            while (f < end && f - e < kLongPiece && col[f] / stripe_cols == s) ++f;
            tmp.push_back(Tagged{s, int4{r, e, f, (int)tmp.size()}});
            e = f;
        }
        long_rows.push_back(int4{r, first_slot, (int)tmp.size() - first_slot, 0});
    }
    std::stable_sort(tmp.begin(), tmp.end(), [](const Tagged &a, const Tagged &b) { return a.stripe < b.stripe; });
    pieces.resize(tmp.size());
    for (size_t k = 0; k < tmp.size(); ++k) pieces[k] = tmp[k].d;
}

// One tier of a handle's tile plans on the host, between planning and upload.
template <typename T>
struct TierBuild {
    TilePlan<T> plan;
    // a plan built on the device (tile_plan_device.hpp) keeps its entry arrays there: the handle adopts them
    std::shared_ptr<TileDevArrays<T>> dev;
    bool have = false;
    bool packed = false;  // a packed plan: every pass staged (the ordinary tiles: never for scattered matrices)
    // compacted tiers only: rows[v] = the v-th row of the tier, the work items, the first item of every block
    std::vector<int> rows, item_first;
    std::vector<int4> work;
};

// Everything the tile plans of one handle consist of on the host, between planning and upload.
template <typename T>
struct TileBuild {
    TierBuild<T> tiles;  // the ordinary tiles
    TierBuild<T> lt;     // the long rows' tiles
    TierBuild<T> mt;     // the middle tier of a scattered matrix (rows of g_tile_mid_lo < entries <= tile_lmax): the same kind of plan
    bool scattered = false;
    std::vector<int4> tile_pieces, tile_long;
    std::string dev_error;  // a device build that failed with a HIP error (the host builder took over)
};

// Long-row tile plan.  In: `split` marks the rows the ordinary tiles left out.  Those of them shorter than 2^21
// entries are compacted (rows[v] = the v-th such row) and given a tile plan of their own with pos_bits = 21;
// `split` keeps only what this plan does not take.  A block's passes are cut into work items of about equal pass
// counts, a few thousand in all.  false: nothing to do (fewer than 2^20 entries in such rows).
// build(rows, begin, len, rows per block, lmax, pos_bits, pack): tile_build over the compacted rows into tier.plan /
// tier.dev -- on the host or on the device
// (len_lo, len_hi]: which of the marked rows this plan takes; kPosBits / kRowsPerBlock: 21 / 2048 for the long rows
// (up to 2^21 - 1 entries each), 17 / as tall as the LDS takes for the middle tier of a scattered matrix
template <typename T, typename Build>
bool build_long_tiles(int M, int N, const int *rp, const int *row_len, int chunk, std::vector<unsigned char> &split,
                      TierBuild<T> &tier, Build build, int len_lo, int len_hi, int kPosBits, int kRowsPerBlock,
                      int items) {
    std::vector<int> &rows = tier.rows;
    const TilePlan<T> &plan = tier.plan;
    if (items <= 0) items = g_tile_items;
    rows.clear();
    long long entries = 0;
    for (int r = 0; r < M; ++r)
        if (split[(size_t)r] && row_len[r] > len_lo && row_len[r] <= len_hi) {
            rows.push_back(r);
            entries += row_len[r];
        }
    if (rows.empty() || (entries < (1LL << 20) && g_tile_long < 2)) return false;  // (2: whatever the size, tests)
    std::vector<int> vbegin(rows.size()), vlen(rows.size());
    for (size_t v = 0; v < rows.size(); ++v) {
        vbegin[v] = rp[rows[v]];
        vlen[v] = row_len[rows[v]];
    }
    // packed (every pass staged) unless that leaves passes of a few entries each
    tier.packed = g_tile_pack != 0;
    if (!build((int)rows.size(), vbegin.data(), vlen.data(), kRowsPerBlock, len_hi, kPosBits, tier.packed)) return false;
    if (tier.packed && plan.entries < (long long)plan.pass_desc.size() * (chunk / 8)) {
        tier.packed = false;
        if (!build((int)rows.size(), vbegin.data(), vlen.data(), kRowsPerBlock, len_hi, kPosBits, false)) return false;
    }
    for (int r : rows) split[(size_t)r] = 0;
    // work items: ~tile_items (1008: two rounds of the 512 places) of them over all blocks, at least 4 passes each
    const long long passes = (long long)plan.pass_desc.size();
    const int per_item = (int)std::max<long long>(4, (passes + items - 1) / items);
    tier.work.clear();
    tier.item_first.assign(1, 0);
    for (int b = 0; b < plan.num_blocks; ++b) {
        for (int p = plan.block_pass[(size_t)b]; p < plan.block_pass[(size_t)b + 1]; p += per_item)
            tier.work.push_back(int4{b, p, std::min(p + per_item, plan.block_pass[(size_t)b + 1]), (int)tier.work.size()});
        tier.item_first.push_back((int)tier.work.size());
    }
    return true;
}

// The tile plans for rows given as (first entry, length) pairs over host arrays col / val -- a CSR matrix's rows, or
// the rows of an HLL slab (spmv_hll.hip).  rp: the CSR row pointer when the rows ARE a CSR matrix's (then rows that
// neither plan takes go to stripe-cut split-row pieces), nullptr otherwise (then such rows veto the plan).
//
// Rows per block (auto): two regimes, told apart on a sample of the rows.
//  * banded (most entries in passes that can be staged): 32 KiB of accumulators (4096 fp64 / 8192 fp32 rows), so
//    that two workgroups with their 32 KiB x slices share a CU (road-like, wide band: measured best of 2048 / 4096 /
//    8192);
//  * scattered (gather passes): what matters is that a pass spans little of x (the band all blocks gather from
//    together must fit L2), that the blocks run in few rounds (a new round starts again at column 0) and that not
//    too many of them are on the way at once: the tallest blocks (up to 16384 rows) that still leave ~2 per CU, ONE
//    workgroup per CU.  Power-law matrix (fp32, 2^24 rows): 2.90 ms at 8192 rows, 1.97 ms at 16384 with one
//    workgroup per CU, 2.39 ms with two.
constexpr int kTileGatherMinCols = 800000;  // (auto) columns from which a tile plan with gather passes is built

// din (optional): the same rows on the device (row_begin / row_len / col / val there): the plans are then built by
// tile_build_device -- byte for byte what tile_build makes of the host arrays, which remain the fallback when a
// device build fails with a HIP error (hcol / hval may be NULL when there is a din: then such a failure vetoes the plan).
template <typename T>
void tile_plan_all(int Ml, int N, const int *row_begin, const int *row_len, const int *rp, long long nz, const int *hcol,
                   const T *hval, TileBuild<T> &tb, const TileDevInput<T> *din = nullptr) {
    const int chunk = 2048;
    UploadTrace trace("tile_plan_all");
    bool dev_ok = din != nullptr;
    std::vector<void *> dev_tmp;  // device copies of compacted row lists (long rows' plan), freed on return
    struct FreeAll {
        std::vector<void *> &v;
        ~FreeAll() {
            for (void *p : v) (void)hipFree(p);
        }
    } free_all{dev_tmp};
    // one tile_build, wherever: rows [s0, s0 + rows) of the handle's row arrays (begin_h / len_h point at row s0), or --
    // own_rows -- a row list of its own that exists on the host only
    auto build_at = [&](int rows, const int *begin_h, const int *len_h, const int *begin_d, const int *len_d, int rpb, int lmax,
                        int pos_bits, bool pack, long long target, int min_pass, TilePlan<T> &plan,
                        std::shared_ptr<TileDevArrays<T>> &arrays) -> bool {
        arrays.reset();
        if (dev_ok) {
            TileDevInput<T> in = *din;
            in.row_begin = begin_d;
            in.row_len = len_d;
            const int rc = tile_build_device<T>(rows, N, in, len_h, rpb, lmax, g_tile_density, chunk, g_tile_balance != 0 || pos_bits != 17,
                                                pos_bits, plan, arrays, pack, target, min_pass, tb.dev_error);
            if (rc >= 0) return rc == 1;
            dev_ok = false;  // a HIP error: everything from here on on the host
            arrays.reset();
        }
        if (!hcol || !hval) return false;
        return tile_build<T>(rows, N, begin_h, len_h, hcol, hval, rpb, lmax, g_tile_density, chunk, g_tile_balance != 0 || pos_bits != 17,
                             pos_bits, plan, pack, target, min_pass);
    };
    std::shared_ptr<TileDevArrays<T>> probe_arrays;
    int lmax_eff = g_tile_lmax;  // longest row of the ordinary tiles (g_tile_mid_lo once a middle tier is decided on)
    auto build_rows = [&](int rows, int s0, int rpb, bool pack, long long target, int min_pass, TilePlan<T> &plan,
                          std::shared_ptr<TileDevArrays<T>> &arrays) {
        return build_at(rows, row_begin + s0, row_len + s0, din ? din->row_begin + s0 : nullptr, din ? din->row_len + s0 : nullptr, rpb,
                        lmax_eff, 17, pack, target, min_pass, plan, arrays);
    };
    int rb = g_tile_rows;
    // Which kernel: a banded matrix is built PACKED -- every pass cut at the window and staged, the sparse tails too
    // (tile_plan.hpp) -- for the kernel instantiation without gather code, unless that leaves passes of a few entries
    // each (entries far from the band: one window, i.e. one pass, per stray entry); anything else keeps gather passes.
    const int banded_rows = 32768 / (int)sizeof(T);
    // the tallest blocks a CU's LDS takes (tile_kernels.hpp): the packed kernel is built for the banded limit
    constexpr int banded_rows_max = tile_banded_rows_max<T>();
    constexpr int scattered_rows_max = tile_scattered_rows_max<T>();
    bool want_pack = g_tile_pack != 0;
    // (... or slices several times the size of the entries they serve: 32 KiB of x out of L2 for a few hundred entries
    // costs as much as gathering them, measured on 30 uniformly random columns per row of a 1 M-column matrix)
    auto pack_pays = [&](const TilePlan<T> &p) {
        return p.entries >= (long long)p.pass_desc.size() * (chunk / 8) &&
               p.staged_cols * (long long)sizeof(T) <= 2 * p.entries * (long long)(4 + sizeof(T));
    };
    {
        // a slice of the matrix from its middle (rows keep their global columns)
        const int srows = rb ? rb : banded_rows;
        const int sample = std::min(Ml, 8 * srows), s0 = (Ml - sample) / 2;
        TilePlan<T> probe;
        const bool ok = build_rows(sample, s0, srows, false, 0, 0, probe, probe_arrays);
        const bool banded = ok && probe.staged_entries * 2 >= probe.entries;
        if (!rb) {
            if (banded) {
                rb = banded_rows;
            } else {
                rb = 16384;
                while (rb > 2048 && (long long)Ml < 448LL * rb) rb >>= 1;  // at least ~1.75 blocks per CU
                rb = std::min(rb, scattered_rows_max);
                tb.scattered = true;
            }
        }
        want_pack = want_pack && banded && rb <= banded_rows_max;
        if (want_pack) {  // the same slice as a packed plan
            const bool pok = build_rows(sample, s0, srows, true, 0, 0, probe, probe_arrays);
            want_pack = pok && pack_pays(probe);
        }
        probe_arrays.reset();
    }
    trace.mark("sample probes");
    tb.tiles.packed = want_pack && !tb.scattered;
    // The middle tier (round 3).  In a scattered plan every entry is a gathered value, and the gathers are what the
    // kernel waits for (config 5: 0.91 of 1.19 ms for the rows of up to 1024 entries).  Rows of more than mid_lo
    // entries, compacted into blocks as tall as the LDS takes (16384 fp32 rows), put enough entries into every
    // 32 KiB column range for the PACKED kernel: their x look-ups move to LDS like the long rows' -- when there are
    // enough of them (2^22 entries) for the extra launch and its slabs to pay.
    bool want_mid = false;
    // where the tier starts: the taller the blocks (fp32: 32512 rows, fp64: 16128), the shorter the rows that still fill
    // a column range -- config 5 (fp32): 1051 us from 128 entries on, 1031 from 96, 1023 from 64, 1014 from 48, 1046 from
    // 32 (profiles/r3_sweep_mid_lo.txt)
    const int mid_lo = g_tile_mid_lo > 0 ? g_tile_mid_lo : sizeof(T) == 4 ? 48 : 128;
    if (tb.scattered && g_tile_mid && g_tile_long && !g_tile_rows && g_tile_lmax > mid_lo && g_tile_pack) {
        long long mid_entries = 0;
        for (int r = 0; r < Ml; ++r)
            if (row_len[r] > mid_lo && row_len[r] <= g_tile_lmax) mid_entries += row_len[r];
        want_mid = mid_entries >= (4LL << 20);
        if (want_mid) lmax_eff = mid_lo;
    }
    // Mid-size matrices (fewer rows than kTileMinRows, but entries for four full passes on every place): only a
    // band of dense rows pays -- the packed plan, with blocks thin enough to give every place one (their slices stay
    // small next to their entries: 33 per row, 503 625 rows: 48.6 us in 493 blocks of 1024 rows against 68.3 us for the
    // gather kernel and 59.5 us in 247 blocks of 2048; 50 per row, 161 070 rows: 30.8 against 39.9 us).
    const bool mid = g_stream_tile < 0 && (long long)Ml < kTileMinRows;
    if (mid && !tb.tiles.packed) return;
    // (auto) tile plans pay from about 800 000 rows / columns on (kTileMinRows, kTileGatherMinCols): 5 uniformly random
    // columns per row tie with the gather kernel at 750 000 rows (37.4 vs 37.9 us) and lose at 500 000 (28 vs 23 us); at
    // 1.09 M rows 3 per row win 37 vs 44 us, power-law fp32 74 vs 107 us, a road-like band 24 vs 29 us.  (Before the block
    // count was fitted to rounds the break-even was 1.5 M columns: 2 x 256 short blocks on 256 places.)
    if (g_stream_tile < 0 && !tb.tiles.packed && N < kTileGatherMinCols) return;
    // How many blocks: equal-work blocks finish together, so the kernel runs in ROUNDS of as many blocks as the chip
    // holds at once (2 per CU banded, 1 scattered) and a last round of a few blocks costs a whole one -- 530 blocks on
    // 512 places took 2 x 215 us on a dense band, 1040 on 256 five rounds instead of four on the power-law matrix.
    // So (auto): the smallest number of rounds k for which blocks of up to the tallest height the LDS takes, closed
    // at in_tiles / (98.5 % of k rounds' places) entries, come out as at most k rounds' worth.
    long long target = 0;
    if (!g_tile_rows && g_tile_balance && g_tile_fit) {
        const int places = g_tile_places ? g_tile_places : (tb.scattered ? 1 : 2) * g_num_cus;
        const int rows_max = tb.scattered ? scattered_rows_max : banded_rows_max;
        long long in_tiles = 0;
        for (int r = 0; r < Ml; ++r)
            if (row_len[r] <= lmax_eff) in_tiles += row_len[r];
        const long long full = std::max(1, (Ml + rb - 1) / rb);
        const int b0 = (int)tile_cut_rows(Ml, row_len, lmax_eff, rb, std::max<long long>(chunk, (in_tiles + full - 1) / full)).size() - 1;
        // (a matrix whose blocks fill less than 90 % of one round keeps them: thinner blocks would each read more of x)
        const int kmax = mid ? 1 : b0 * 10LL > places * 9LL ? (b0 + places - 1) / places : 0;
        for (int k = 1; k <= kmax; ++k) {
            const long long want = (long long)k * places * 197 / 200;
            const long long t = std::max<long long>(chunk, (in_tiles + want - 1) / want);
            const int b = (int)tile_cut_rows(Ml, row_len, lmax_eff, rows_max, t).size() - 1;
            if (b <= k * places) {
                rb = rows_max;
                target = t;
                break;
            }
        }
    }
    trace.mark("block count fit");
    TierBuild<T> &own = tb.tiles;
    own.have = build_rows(Ml, 0, rb, own.packed, target,
                          // (its extra launch costs ~2 us: not for matrices whose whole product takes 25)
                          nz >= (16LL << 20) || g_stream_tile == 1 ? g_tile_min_pass : 0, own.plan, own.dev);
    // (the remainder is for a few per cent of far-out entries: more than 4 % and the plan is rebuilt without one)
    if (own.have && own.packed && (long long)own.plan.rem_row.size() * 25 > own.plan.entries)
        own.have = build_rows(Ml, 0, rb, own.packed, target, 0, own.plan, own.dev);
    // (the whole matrix may differ from the sample)
    if (own.have && own.packed && !pack_pays(own.plan)) {
        own.packed = false;
        if (g_stream_tile < 0 && N < kTileGatherMinCols) {
            own.have = false;
            return;
        }
        own.have = build_rows(Ml, 0, rb, false, target, 0, own.plan, own.dev);
    }
    // (auto) a matrix made mostly of rows beyond the tile limit gains nothing without the long rows' plan
    if (own.have && g_stream_tile < 0 && !g_tile_long && own.plan.entries * 2 < nz) own.have = false;
    if (!own.have) return;
    trace.mark("ordinary tiles");
    // one workgroup per place of the chip walks several blocks back to back (tile_streams 0: one workgroup per block)
    // (tile_places: tests walk long streams on small matrices)
    tile_make_streams(own.plan, !g_tile_streams ? 0x3fffffff : g_tile_places ? g_tile_places : (tb.scattered ? 1 : 2) * g_num_cus);
    // The rows beyond the tile limit, compacted: their own row blocks (<= 2048 of them each), same passes -- so many
    // entries per column range that every pass is staged: the long rows' x lookups happen in LDS at the HBM streaming
    // rate instead of going through the gather path -- and a block's passes dealt out to many workgroups.
    std::vector<unsigned char> leftover = own.plan.split;
    // one compacted tier out of `leftover` (packed_only: the middle tier's rule)
    auto build_compact = [&](TierBuild<T> &tier, bool packed_only, int len_lo, int len_hi, int pos_bits, int tier_rows, int items) {
        return build_long_tiles<T>(
            Ml, N, row_begin, row_len, chunk, leftover, tier,
            [&](int rows, const int *begin_h, const int *len_h, int rpb, int lmax, int bits, bool pack) {
                if (packed_only && !pack) return false;  // (a middle tier with gather passes would be the ordinary tiles again, plus slabs)
                int *d_begin = nullptr, *d_len = nullptr;
                if (dev_ok) {  // the compacted row list exists on the host only: a device copy for this build
                    if (upload_array(&d_begin, begin_h, (size_t)rows, 1) == 0) dev_tmp.push_back(d_begin);
                    else dev_ok = false;
                    if (dev_ok && upload_array(&d_len, len_h, (size_t)rows, 1) == 0) dev_tmp.push_back(d_len);
                    else dev_ok = false;
                }
                return build_at(rows, begin_h, len_h, d_begin, d_len, rpb, lmax, bits, pack, 0, 0, tier.plan, tier.dev);
            },
            len_lo, len_hi, pos_bits, tier_rows, items);
    };
    // (with a middle tier the long rows' plan starts behind it)
    if (g_tile_long) tb.lt.have = build_compact(tb.lt, false, want_mid ? g_tile_lmax : 0, (1 << 21) - 1, 21, 2048, 0);
    // the middle tier: what the ordinary tiles left out up to tile_lmax (the long rows' plan has taken the rest)
    if (want_mid)
        tb.mt.have = build_compact(tb.mt, true, mid_lo, g_tile_lmax, 17, scattered_rows_max,
                                   // (its blocks fill a CU's LDS: one workgroup per CU, so whole rounds of the CUs -- three of them: config 5
                                   // 1008 / 954 / 898 / 918 / 943 / 996 us at 256 / 512 / 768 / 1008 / 1280 / 2016 items, profiles/r3_sweep_mid_items.txt)
                                   g_tile_mid_items ? g_tile_mid_items : 3 * std::max(g_num_cus, 1));
    if (want_mid && (!tb.mt.have || !tb.mt.packed)) {
        // the tier did not come about (its passes would average fewer than 256 entries, or its build failed): the plan
        // without one, from the start -- the ordinary tiles then take the rows up to tile_lmax again
        const int keep = g_tile_mid;
        g_tile_mid = 0;
        tb = TileBuild<T>();
        tile_plan_all<T>(Ml, N, row_begin, row_len, rp, nz, hcol, hval, tb, din);
        g_tile_mid = keep;
        return;
    }
    trace.mark("streams, long rows' tiles");
    bool any_left = false;
    for (unsigned char f : leftover) any_left |= f != 0;
    if (!any_left) return;
    if (!rp) {  // no CSR arrays on the device to fall back on
        own.have = tb.lt.have = false;
        return;
    }
    // whatever is left (rows of 2^21 entries and more, or all long rows with tile_long = 0) stays with the split-row
    // kernels, pieces cut at stripes of 1 MiB of x: a quarter of an XCD's L2
    const int stripe_cols = (1 << 20) / (int)sizeof(T);
    build_striped_pieces(Ml, rp, hcol, leftover, stripe_cols, tb.tile_pieces, tb.tile_long);
}

// csr_tile asks for up to a CU's whole LDS as dynamic shared memory; HIP wants that allowed per kernel beyond
// 64 KiB.  Done once per value type, at upload (not at launch: a launch may sit inside a graph capture).
template <typename T>
int tile_allow_lds() {
    // the attribute belongs to (function, device): spmv_hip_init may have switched devices since the last upload
    static int done_for_device = -1;
    const bool done = done_for_device == g_device;
    if (done) return 0;
    constexpr int kXpTrips = 2048 * (int)sizeof(T) / kTileTripBytes;  // the expanded plans' instantiation
    const void *fns[8] = {(const void *)csr_tile<T, false, 2048, kXpTrips, true>, (const void *)csr_tile<T, true, 2048, kXpTrips, true>,
                          (const void *)csr_tile<T, false, 2048, kTileTrips, false>, (const void *)csr_tile<T, true, 2048, kTileTrips, false>,
                          (const void *)csr_tile<T, false, 2048, kTileTrips, true>, (const void *)csr_tile<T, true, 2048, kTileTrips, true>,
                          (const void *)csr_tile<T, false, 2048, kTileTrips, false, true>,
                          (const void *)csr_tile<T, true, 2048, kTileTrips, false, true>};
    for (const void *fn : fns) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done_for_device = g_device;
    return 0;
}

// One array of a plan on its way to the handle: the device builder's moves in (and leaves nullptr behind: its owner no
// longer frees it), the host builder's is uploaded.  built: where the device builder keeps it, nullptr for a host plan.
template <typename P, typename E>
int adopt_or_upload(P **dst, E **built, const std::vector<E> &host) {
    if (!built) return upload_array((E **)dst, host.data(), host.size(), 0);
    *dst = *built;
    *built = nullptr;
    return 0;
}

// What every tier takes from its plan: the entry arrays (tcol_count / tkey_count: their elements, from whichever side built
// them) and the counters.
template <typename T>
int take_entries(TileTier &t, const TierBuild<T> &b, size_t &tcol_count, size_t &tkey_count) {
    const TilePlan<T> &plan = b.plan;
    TileDevArrays<T> *dev = b.dev.get();  // built on the device: the entry arrays are there already
    tcol_count = dev ? dev->tcol_count : plan.tcol.size();
    tkey_count = dev ? dev->tkey_count : plan.tkey.size();
    if (adopt_or_upload(&t.tcol, dev ? &dev->tcol : nullptr, plan.tcol)) return -1;
    if (adopt_or_upload(&t.tkey, dev ? &dev->tkey : nullptr, plan.tkey)) return -1;
    if (adopt_or_upload(&t.tval, dev ? &dev->tval : nullptr, plan.tval)) return -1;
    t.blocks = plan.num_blocks;
    t.rows_per_block = plan.rows_per_block;
    t.passes = (int)plan.pass_desc.size();
    t.max_win = plan.max_win;
    t.entries = plan.entries;
    t.padded = (long long)tcol_count - kTileChunkMax;
    t.staged = plan.staged_entries;
    t.staged_cols = plan.staged_cols;
    t.packed = b.packed;
    return 0;
}

// the ordinary tiles -> the handle
template <typename T>
int upload_own_tiles(spmv_csr_dev *m, const TileBuild<T> &tb) {
    OwnTiles &t = m->tile;
    const TilePlan<T> &tiles = tb.tiles.plan;
    TileDevArrays<T> *dev = tb.tiles.dev.get();
    // (the kernel walks STREAMS: descriptors in stream order, the passes / blocks of every stream, the blocks' rows)
    if (upload_array(&t.block_pass, tiles.stream_pass.data(), tiles.stream_pass.size(), 1)) return -1;
    if (upload_array(&t.block_row, tiles.block_row.data(), tiles.block_row.size(), 1)) return -1;
    if (upload_array(&t.pass, tiles.spass.data(), tiles.spass.size(), 1)) return -1;
    if (!tiles.rem_row.empty()) {  // remainder: rows that have any, their entry ranges
        std::vector<int> rrow, rptr;
        for (size_t k = 0; k < tiles.rem_row.size(); ++k) {
            if (rrow.empty() || rrow.back() != tiles.rem_row[k]) {
                rrow.push_back(tiles.rem_row[k]);
                rptr.push_back((int)k);
            }
        }
        rptr.push_back((int)tiles.rem_row.size());
        if (upload_array(&t.rem_row, rrow.data(), rrow.size(), 0)) return -1;
        if (upload_array(&t.rem_ptr, rptr.data(), rptr.size(), 0)) return -1;
        if (adopt_or_upload(&t.rem_col, dev ? &dev->rem_col : nullptr, tiles.rem_col)) return -1;
        if (adopt_or_upload(&t.rem_val, dev ? &dev->rem_val : nullptr, tiles.rem_val)) return -1;
        t.rem_rows = (int)rrow.size();
        t.rem_entries = (long long)tiles.rem_row.size();
        m->rest_bytes += rrow.size() * 8 + tiles.rem_row.size() * (4 + sizeof(T));
    }
    if (upload_array(&t.stream_block, tiles.stream_block.data(), tiles.stream_block.size(), 1)) return -1;
    if (upload_array(&t.sblock_rows, tiles.sblock_rows.data(), tiles.sblock_rows.size(), 1)) return -1;
    size_t tcol_count = 0, tkey_count = 0;
    if (take_entries(t, tb.tiles, tcol_count, tkey_count)) return -1;
    if (!tb.tile_long.empty() && upload_array(&t.long_rows, tb.tile_long.data(), tb.tile_long.size(), 0)) return -1;
    if (!tb.tile_pieces.empty() && upload_array(&t.pieces, tb.tile_pieces.data(), tb.tile_pieces.size(), 0)) return -1;
    t.streams = tiles.num_streams;
    t.lds_min = tb.scattered ? 84 * 1024 : 0;  // more than half a CU's LDS: one workgroup per CU
    t.num_long = (int)tb.tile_long.size();
    t.num_pieces = (int)tb.tile_pieces.size();
    m->rest_bytes += tcol_count * (4 + sizeof(T)) + tkey_count * 2 + tiles.pass_desc.size() * 16 + tiles.block_pass.size() * 4 +
                       (tb.tile_pieces.size() + tb.tile_long.size()) * 16;
    return 0;
}

// a compacted tier (the long rows' plan, the middle tier) -> the handle: block tables, work items, entry arrays, slabs
template <typename T>
int upload_compact_tiles(spmv_csr_dev *m, const TierBuild<T> &b, CompactTiles &L) {
    const TilePlan<T> &ltiles = b.plan;
    std::vector<int> block_of_row(b.rows.size());
    for (int k = 0; k < ltiles.num_blocks; ++k)
        for (int v = ltiles.block_row[(size_t)k]; v < ltiles.block_row[(size_t)k + 1]; ++v) block_of_row[(size_t)v] = k;
    if (upload_array(&L.block_row, ltiles.block_row.data(), ltiles.block_row.size(), 1)) return -1;
    if (upload_array(&L.block_pass, ltiles.block_pass.data(), ltiles.block_pass.size(), 1)) return -1;
    if (upload_array(&L.block_of_row, block_of_row.data(), block_of_row.size(), 1)) return -1;
    if (upload_array(&L.item_first, b.item_first.data(), b.item_first.size(), 1)) return -1;
    if (upload_array(&L.row_map, b.rows.data(), b.rows.size(), 1)) return -1;
    if (upload_array(&L.pass, ltiles.pass_desc.data(), ltiles.pass_desc.size(), 1)) return -1;
    if (upload_array(&L.work, b.work.data(), b.work.size(), 1)) return -1;
    size_t ltcol_count = 0, ltkey_count = 0;
    if (take_entries(L, b, ltcol_count, ltkey_count)) return -1;
    const size_t slab_bytes = std::max<size_t>(1, b.work.size()) * (size_t)ltiles.rows_per_block * sizeof(T);
    hipError_t e = hipMalloc(&L.slab, slab_bytes);
    if (e != hipSuccess) return fail("hipMalloc(slabs) failed: %s", hipGetErrorString(e));
    m->rest_bytes += slab_bytes;
    L.rows = (int)b.rows.size();
    L.items = (int)b.work.size();
    m->rest_bytes += ltcol_count * (4 + sizeof(T)) + ltkey_count * 2 + ltiles.pass_desc.size() * 16 + b.work.size() * 16 +
                       b.rows.size() * 8;
    return 0;
}

// the plans' arrays -> the handle (on a failure the handle keeps what was allocated: its owner frees it)
template <typename T>
int tile_upload_all(spmv_csr_dev *m, const TileBuild<T> &tb) {
    // the kernels need more than 64 KiB of dynamic LDS: where the device will not allow that the handle simply gets
    // no tiles and keeps its gather kernels (return 1; the message stays in spmv_hip_last_error)
    if ((tb.tiles.have || tb.lt.have || tb.mt.have) && tile_allow_lds<T>()) return 1;
    if (tb.tiles.have && upload_own_tiles<T>(m, tb)) return -1;
    OwnTiles &t = m->tile;
    // a plan whose passes gather (scattered columns: next to none of them dense enough to stage) runs on an expanded x:
    // tile_expand walks the entries slice by slice of x and writes every entry's value into its pass's segment of x',
    // which csr_tile<.., PACK> stages as that pass's window (tile_kernels.hpp).  The same products in the same order:
    // the same bits as the gather passes.
    // auto: plans from 2^22 entries on with fewer than a tenth of them in staged passes -- fp32 always (uniformly random
    // columns, 2 M x 10 ... 16 M x 8: -17 ... -37 %; config 5's short rows 491 -> 141 + 180 us), fp64 when x is beyond
    // 100 MB: an fp64 gather brings twice the bytes per line and the expansion moves twice the bytes per entry -- 4 M x
    // 20: 518 -> 539 us, 12 M x 4: 462 -> 454, 16 M x 8: 1095 -> 939 (profiles/r3_ab_expand.txt)
    // ("tile_expand" 0: never, 1: always)
    const bool expand_pays = sizeof(T) == 4 || (long long)m->N * (long long)sizeof(T) >= (100LL << 20);
    if (tb.tiles.have && !tb.tiles.packed && t.tcol && t.padded > 0 &&
        (g_tile_expand > 0 || (g_tile_expand < 0 && expand_pays && t.entries >= (1 << 22) && t.staged * 10 <= t.entries))) {
        const size_t slots = (size_t)t.padded;
        t.expansion = new (std::nothrow) TileExpansion();
        if (!t.expansion) return fail("csr_upload: out of host memory");
        std::string err;
        if (tile_build_expansion<T>(m->N, t.tcol, t.tkey, slots, t.pass, (int)tb.tiles.plan.spass.size(), g_stream, *t.expansion, err) < 0)
            return fail("%s", err.c_str());
        const size_t xe_bytes = (slots + kTileChunkMax) * sizeof(T);
        hipError_t e = hipMalloc(&t.xe, xe_bytes);
        if (e == hipSuccess) e = hipMemsetAsync(t.xe, 0, xe_bytes, g_stream);
        if (e != hipSuccess) return fail("hipMalloc(expanded x) failed: %s", hipGetErrorString(e));
        m->rest_bytes += xe_bytes + (slots + 64) * 2 + (slots + kTileChunkMax) * 4 + tb.tiles.plan.spass.size() * 16 +
                           (size_t)t.expansion->chunks * 24 + (t.expansion->runs + t.expansion->groups) * 4;
    }
    if (tb.lt.have && upload_compact_tiles<T>(m, tb.lt, m->lt)) return -1;
    if (tb.mt.have && upload_compact_tiles<T>(m, tb.mt, m->mt)) return -1;
    return 0;
}

}  // namespace
