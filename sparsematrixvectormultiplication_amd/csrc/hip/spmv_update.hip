// spmv_update.hip -- spmv_hip_csr_update_values: new numbers on a handle's pattern, under the plan it has
// (include/spmv_hip.h).
//
// Nothing an upload decides reads a value, and only five arrays of a handle hold matrix values: `val`, which the gather
// kernels, the x-window plan, the pattern plan, the split rows and the long rows read in CSR order, and the four arrays
// of the tile plans that hold the values in the plans' order (tile.tval, tile.rem_val, lt.tval, mt.tval).  An update is
// one copy into `val` -- into the allocation, which stays where the placement search put it -- and, for a handle with
// tile plans, one upd_gather (update_kernels.hpp) per such array through its source map.
//
// The source maps are made by the handle's FIRST update, from the plan the handle holds and nothing else (no knob is
// read: the knobs of the upload may be gone by then).  A slot of a pass is (local row of its block, column); the pass's
// block gives the row, and the slot holds the row's entry with that column -- for a (row, column) pair that repeats,
// the builders keep entry order inside a pass, from pass to pass of a block (passes go up the columns, a cut inside a
// run of repeats leaves the earlier entries in the earlier pass) and put a remainder window's repeats, all of them,
// behind whatever an earlier pass took (tile_plan.hpp, build_range): so the k-th slot of a pair, passes in block order
// first and the remainder then, is the pair's k-th entry.  An upload that is never followed by an update keeps, allocates
// and runs nothing of this.
#include "spmv_internal.hpp"

#include <atomic>
#include <chrono>
#include <thread>

#include "tile_plan.hpp"  // tile_detail::run_threads
#include "update_kernels.hpp"

namespace {

// The analysis runs on the builder's threads: blocks hold disjoint rows, so the threads that take different blocks (or
// different rows) touch different slots of the maps and different counters of the lookup.
int map_threads() { return (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u); }

template <typename E>
int to_host(std::vector<E> &out, const void *dev, size_t count) {
    out.resize(count);
    if (count) HIP_TRY(hipMemcpy(out.data(), dev, count * sizeof(E), hipMemcpyDeviceToHost));
    return 0;
}

// The entries of the handle's rows by (row, column), repeats in entry order, and how many of each pair's entries the
// maps have handed out so far.
struct EntryLookup {
    int rows = 0;
    std::vector<int> rp, col;  // the handle's arrays
    std::vector<int> order;    // entries by (row, column), stable; empty: every row ascends already (order[e] = e)
    std::vector<int> scol;     // col[order[.]] then
    std::vector<int> taken;    // at a pair's first place in that order: entries of the pair handed out

    int load(const spmv_csr_dev *m) {
        if (to_host(rp, m->row_ptr, (size_t)m->M_local + 1) || to_host(col, m->col, (size_t)m->nz)) return -1;
        prepare();
        return 0;
    }
    // rp and col are there
    void prepare() {
        rows = (int)rp.size() - 1;
        taken.assign(col.size(), 0);
        const int threads = map_threads();
        std::atomic<bool> ascending(true);
        spmv::tile_detail::run_threads(threads, [&](int th) {  // (rows th, th + threads, ...)
            for (int r = th; r < rows && ascending.load(std::memory_order_relaxed); r += threads)
                for (int e = rp[(size_t)r] + 1; e < rp[(size_t)r + 1]; ++e)
                    if (col[(size_t)e - 1] > col[(size_t)e]) {
                        ascending.store(false, std::memory_order_relaxed);
                        break;
                    }
        });
        if (ascending.load()) return;
        order.resize(col.size());
        scol.resize(col.size());
        spmv::tile_detail::run_threads(threads, [&](int th) {
            for (int r = th; r < rows; r += threads) {
                const int e0 = rp[(size_t)r], e1 = rp[(size_t)r + 1];
                for (int e = e0; e < e1; ++e) order[(size_t)e] = e;
                std::stable_sort(order.begin() + e0, order.begin() + e1, [&](int a, int b) { return col[(size_t)a] < col[(size_t)b]; });
                for (int e = e0; e < e1; ++e) scol[(size_t)e] = col[(size_t)order[(size_t)e]];
            }
        });
    }
    // the next entry of (row, c) not handed out yet; -1: the row holds no such entry (any more)
    int next(int row, int c) {
        if (row < 0 || row >= rows) return -1;
        const std::vector<int> &sc = order.empty() ? col : scol;
        const int *lo = sc.data() + rp[(size_t)row], *hi = sc.data() + rp[(size_t)row + 1];
        const int *first = std::lower_bound(lo, hi, c);
        if (first == hi || *first != c) return -1;
        const size_t at = (size_t)(first - sc.data());
        const size_t e = at + (size_t)taken[at];
        if (e >= (size_t)rp[(size_t)row + 1] || sc[e] != c) return -1;
        ++taken[at];
        return order.empty() ? (int)e : order[e];
    }
};

int bad_plan(const char *what) { return fail("csr_update_values: the %s do not lead back to the handle's entries", what); }

// the slots of one pass: d = {first slot, entries, window base, flags}, r0 the first row of its block in the tier's row
// space, row_of the tier's rows in the handle's (nullptr: the same).  1: the pass does not lead back to the handle's
// entries (no message from here: the passes run on threads)
int map_pass(const int4 d, int r0, const std::vector<int> *row_of, const std::vector<int> &tcol, const std::vector<unsigned short> &tkey,
             EntryLookup &look, std::vector<int> &map) {
    if (d.y < 0 || d.x < 0 || (size_t)d.x + (size_t)d.y > map.size()) return 1;
    const bool packed = (d.w & kTilePassPacked) != 0;
    if (!packed && tkey.size() < map.size()) return 1;
    for (int k = 0; k < d.y; ++k) {
        const size_t slot = (size_t)d.x + (size_t)k;
        const unsigned word = (unsigned)tcol[slot];
        const int lrow = packed ? (int)((word & 0x7fffffffu) >> kTilePackShift) : (int)(tkey[slot] & kTileRowMask);
        const int c = packed ? d.z + (int)(word & kTilePackColMask) : (int)word;
        int row = r0 + lrow;
        if (row_of) {
            if (row < 0 || (size_t)row >= row_of->size()) return 1;
            row = (*row_of)[(size_t)row];
        }
        const int e = look.next(row, c);
        if (e < 0) return 1;
        map[slot] = e;
    }
    return 0;
}

// One tier's plan on the host, as far as the maps need it.  The ordinary tiles: descriptors in stream order, block_pass
// and stream_block per stream, block_first the blocks' first rows in stream order, a block's passes back to back with
// kTilePassLast on the last.  A compacted tier: descriptors in block order, block_pass and block_first per block, row_of
// the tier's rows in the handle's.
struct TierHost {
    std::vector<int4> pass;
    std::vector<int> block_pass, stream_block, block_first, row_of, tcol;
    std::vector<unsigned short> tkey;
    std::vector<int> rem_row, rem_ptr, rem_col;  // the ordinary tiles' remainder
    size_t padded = 0;
};

int map_own_tiles(const TierHost &t, EntryLookup &look, std::vector<int> &map, std::vector<int> &rem_map) {
    const char *what = "ordinary tiles";
    const int streams = (int)t.block_pass.size() - 1, blocks = (int)t.block_first.size(), passes = (int)t.pass.size();
    map.assign(t.padded, -1);
    const int threads = map_threads();
    std::atomic<bool> bad(false);
    spmv::tile_detail::run_threads(threads, [&](int th) {  // (streams th, th + threads, ...: their blocks are disjoint)
        for (int s = th; s < streams && !bad.load(std::memory_order_relaxed); s += threads) {
            int blk = t.stream_block[(size_t)s];
            bool ok = t.block_pass[(size_t)s] >= 0 && t.block_pass[(size_t)s + 1] <= passes;
            for (int p = ok ? t.block_pass[(size_t)s] : 0; ok && p < t.block_pass[(size_t)s + 1]; ++p) {
                ok = blk >= 0 && blk < blocks &&
                     !map_pass(t.pass[(size_t)p], t.block_first[(size_t)blk], nullptr, t.tcol, t.tkey, look, map);
                if (ok && (t.pass[(size_t)p].w & kTilePassLast)) ++blk;
            }
            if (!ok) bad.store(true, std::memory_order_relaxed);
        }
    });
    if (bad.load()) return bad_plan(what);
    // the remainder, by (row, column): behind the passes
    const int rem_rows = (int)t.rem_row.size(), rem_entries = (int)t.rem_col.size();
    rem_map.assign((size_t)rem_entries, -1);
    for (int i = 0; i < rem_rows; ++i) {
        if (t.rem_ptr[(size_t)i] < 0 || t.rem_ptr[(size_t)i + 1] > rem_entries) return bad_plan("remainder");
        for (int k = t.rem_ptr[(size_t)i]; k < t.rem_ptr[(size_t)i + 1]; ++k)
            if ((rem_map[(size_t)k] = look.next(t.rem_row[(size_t)i], t.rem_col[(size_t)k])) < 0) return bad_plan("remainder");
    }
    return 0;
}

int map_compact_tiles(const TierHost &t, EntryLookup &look, std::vector<int> &map, const char *what) {
    const int blocks = (int)t.block_first.size() - 1, passes = (int)t.pass.size();
    map.assign(t.padded, -1);
    const int threads = map_threads();
    std::atomic<bool> bad(false);
    spmv::tile_detail::run_threads(threads, [&](int th) {  // (blocks th, th + threads, ...: their rows are disjoint)
        for (int b = th; b < blocks && !bad.load(std::memory_order_relaxed); b += threads) {
            bool ok = t.block_pass[(size_t)b] >= 0 && t.block_pass[(size_t)b + 1] <= passes;
            for (int p = ok ? t.block_pass[(size_t)b] : 0; ok && p < t.block_pass[(size_t)b + 1]; ++p)
                ok = !map_pass(t.pass[(size_t)p], t.block_first[(size_t)b], &t.row_of, t.tcol, t.tkey, look, map);
            if (!ok) bad.store(true, std::memory_order_relaxed);
        }
    });
    return bad.load() ? bad_plan(what) : 0;
}

int fetch_entries(const TileTier &t, TierHost &h) {
    h.padded = (size_t)t.padded;
    return to_host(h.pass, t.pass, (size_t)t.passes) || to_host(h.tcol, t.tcol, h.padded) || (!t.packed && to_host(h.tkey, t.tkey, h.padded));
}

int fetch_own_tiles(const OwnTiles &t, TierHost &h) {
    const size_t per_stream = (size_t)t.streams + 1;
    std::vector<int2> sblock_rows;
    if (fetch_entries(t, h) || to_host(h.block_pass, t.block_pass, per_stream) || to_host(h.stream_block, t.stream_block, per_stream) ||
        to_host(sblock_rows, t.sblock_rows, (size_t)t.blocks))
        return -1;
    for (const int2 &b : sblock_rows) h.block_first.push_back(b.x);
    if (t.rem_entries <= 0) return 0;
    return to_host(h.rem_row, t.rem_row, (size_t)t.rem_rows) || to_host(h.rem_ptr, t.rem_ptr, (size_t)t.rem_rows + 1) ||
           to_host(h.rem_col, t.rem_col, (size_t)t.rem_entries);
}

int fetch_compact_tiles(const CompactTiles &L, TierHost &h) {
    const size_t per_block = (size_t)L.blocks + 1;
    return fetch_entries(L, h) || to_host(h.block_pass, L.block_pass, per_block) || to_host(h.block_first, L.block_row, per_block) ||
           to_host(h.row_of, L.row_map, (size_t)L.rows);
}

// The handle's source maps, once.  On -1 the state holds no map and the handle is as it was.
int build_maps(const spmv_csr_dev *m, UpdateState &u) {
    const bool own = m->tile.blocks > 0 && m->tile.tval, lt = m->lt.items > 0 && m->lt.tval, mt = m->mt.items > 0 && m->mt.tval;
    if (!own && !lt && !mt) {
        u.mapped = true;
        return 0;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    HIP_TRY(hipStreamSynchronize(g_stream));
    EntryLookup look;
    if (look.load(m)) return -1;
    std::vector<int> maps[4];
    {
        TierHost t;
        if (own && (fetch_own_tiles(m->tile, t) || map_own_tiles(t, look, maps[0], maps[1]))) return -1;
    }
    for (int k = 2; k < 4; ++k) {
        TierHost t;
        const CompactTiles &L = k == 2 ? m->lt : m->mt;
        if (k == 2 ? !lt : !mt) continue;
        if (fetch_compact_tiles(L, t) || map_compact_tiles(t, look, maps[k], k == 2 ? "long rows' tiles" : "middle tier's tiles")) return -1;
    }
    int *d[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int k = 0; k < 4 && !rc; ++k)
        if (!maps[k].empty()) rc = upload_array(&d[k], maps[k].data(), maps[k].size(), 0);
    if (rc) {
        for (int *p : d) (void)hipFree(p);
        (void)hipGetLastError();
        return -1;
    }
    for (int k = 0; k < 4; ++k) {
        u.src[k] = d[k];
        u.slots[k] = maps[k].size();
        u.map_bytes += maps[k].size() * sizeof(int);
    }
    u.map_build_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t_begin).count();
    u.mapped = true;
    return 0;
}

template <typename T>
int gather_all(const spmv_csr_dev *m, const UpdateState &u, hipStream_t s) {
    void *dst[4] = {m->tile.tval, m->tile.rem_val, m->lt.tval, m->mt.tval};
    for (int k = 0; k < 4; ++k) {
        if (!u.slots[k]) continue;
        const long long n = (long long)u.slots[k];
        const int grid = (int)std::max<long long>(1, std::min<long long>(kUpdBlocks, ((n + 3) / 4 + kBlock - 1) / kBlock));
        hipLaunchKernelGGL((upd_gather<T>), dim3(grid), dim3(kBlock), 0, s, n, (const int *)u.src[k], (const T *)m->val, (T *)dst[k]);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// values: the handle's nz new values in its dtype and entry order, on the host or (on_device) on the device
int update_values(spmv_csr_dev *m, const void *values, bool on_device, hipStream_t s) {
    if (need_device()) return -1;
    if (!m || !values) return fail("csr_update_values: NULL argument");
    if (m->tiles_only || !csr_holds_arrays(m))
        return fail("csr_update_values: a handle made of tile plans alone holds no CSR arrays to update");
    if (m->own_part || m->halo_part)
        return fail("csr_update_values: the handle holds a column split, whose parts keep values of their own: drop it "
                    "(split_columns over all %d columns), and split the columns again after the update", m->N);
    if (!m->upd) {
        m->upd = new (std::nothrow) UpdateState();
        if (!m->upd) return fail("csr_update_values: out of host memory");
    }
    UpdateState &u = *m->upd;
    if (!u.mapped && build_maps(m, u)) return -1;  // (nothing of the handle has been written yet)
    if (!u.t0) HIP_TRY(hipEventCreate(&u.t0));
    if (!u.t1) HIP_TRY(hipEventCreate(&u.t1));
    u.timed = false;
    HIP_TRY(hipEventRecord(u.t0, s));
    const size_t bytes = (size_t)m->nz * (size_t)m->value_bytes;  // (the kPad entries behind stay zero)
    if (bytes) HIP_TRY(hipMemcpyAsync(m->val, values, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (m->value_bytes == 8 ? gather_all<double>(m, u, s) : gather_all<float>(m, u, s)) return -1;
    HIP_TRY(hipEventRecord(u.t1, s));
    u.timed = true;
    ++u.updates;
    if (!on_device) HIP_TRY(hipStreamSynchronize(s));  // the caller's array is free again
    return 0;
}

}  // namespace

extern "C" int spmv_hip_csr_update_values(spmv_csr_dev *m, const void *val_host) {
    return guarded("csr_update_values", [&] { return update_values(m, val_host, false, g_stream); });
}

extern "C" int spmv_hip_csr_update_values_on(spmv_csr_dev *m, const void *d_val, void *stream) {
    return guarded("csr_update_values_on", [&] { return update_values(m, d_val, true, stream ? (hipStream_t)stream : g_stream); });
}

extern "C" int spmv_hip_csr_update_info(const spmv_csr_dev *m, long long *counts, double *us) {
    if (!m || !counts || !us) return fail("csr_update_info: NULL argument");
    counts[0] = counts[1] = 0;
    us[0] = us[1] = 0.0;
    UpdateState *u = m->upd;
    if (!u) return 0;
    if (u->timed) {  // the last update's device work: waits for it
        HIP_TRY(hipEventSynchronize(u->t1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, u->t0, u->t1));
        u->last_us = ms * 1e3f;
        u->timed = false;
    }
    counts[0] = u->updates;
    counts[1] = (long long)u->map_bytes;
    us[0] = u->map_build_us;
    us[1] = u->last_us;
    return 0;
}
