// launch_dispatch.hpp -- what csr_launch (spmv_csr.hip) and hll_launch (spmv_hll.hip) share: run-time flags and sizes
// turned into template arguments, and the one place that decides which plan a STREAM launch runs.
#pragma once
#include <cstdint>
#include <type_traits>

#include "spmv_internal.hpp"

namespace spmv {

template <int V>
constexpr std::integral_constant<int, V> int_c{};

// body(std::true_type()) or body(std::false_type()): a generic lambda reads the flag as decltype(flag)::value
template <typename F>
void with_flag(bool flag, F body) {
    if (flag) body(std::true_type());
    else body(std::false_type());
}

// body(int_c<V>) for the V of the list that equals `value`; the LAST of the list when none does
template <int V, int... Rest, typename F>
void with_value(int value, F body) {
    if constexpr (sizeof...(Rest) == 0) body(int_c<V>);
    else if (value == V) body(int_c<V>);
    else with_value<Rest...>(value, body);
}

// ---- which plan a STREAM launch runs: the only readers of g_stream_kind and of x's alignment rules
// the x-window kernels read whole aligned lines of x
inline bool x_window_runs(int local_blocks, const void *x) {
    return (g_stream_kind == -1 || g_stream_kind == 5) && local_blocks > 0 && ((uintptr_t)x & (kLineBytes - 1)) == 0;
}

// a PACKED tile plan copies its x slices as 16-byte pieces and has no gather code to fall back on: with an x that is
// not 16-byte aligned the clamp of the last piece no longer keeps the loads inside x
inline bool tiles_take_x(const spmv_csr_dev *m, const void *x) { return !m->tile.packed || ((uintptr_t)x & 15) == 0; }

// (forced: a tiles-only handle has nothing else, whatever the knob says)
inline bool tiles_run(const spmv_csr_dev *m, const void *x, bool forced) {
    return (forced || g_stream_kind == -1 || g_stream_kind == 6) && tiles_take_x(m, x);
}

enum class stream_route { x_window, tiles, gather, nothing_else, unaligned_x };  // the last two: a tiles-only handle's errors

// part < 0: the whole product; 0 / 1: the interior / boundary sub-lists, which only an x-window launch of a handle
// that has the split can run (anything else: csr_launch_part runs everything as part 1)
inline stream_route csr_stream_route(const spmv_csr_dev *m, const void *x, int part) {
    const bool local = x_window_runs(m->xw.blocks, x) && (part < 0 || m->have_split);
    const bool tiled = !local && m->tile.blocks > 0 && tiles_run(m, x, m->tiles_only);
    if (m->tiles_only && !tiled) return tiles_take_x(m, x) ? stream_route::nothing_else : stream_route::unaligned_x;
    return tiled ? stream_route::tiles : local ? stream_route::x_window : stream_route::gather;
}

// the gather stream's short-row kernel (csr_stream_short): the mean row is shorter than stage / 256, so most blocks are
// cut by the row cap and not by the stage
inline bool csr_short_rows(const spmv_csr_dev *m) {
    return (m->stream_cap == 4096 || m->stream_cap == 2048) && m->M_local > 0 &&
           m->nz < (long long)m->M_local * (m->stream_cap / kBlock);
}

}  // namespace spmv
