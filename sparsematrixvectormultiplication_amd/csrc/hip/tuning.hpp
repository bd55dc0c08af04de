// tuning.hpp -- the kernel tuning knobs: each one declared ONCE here, with its default (the measured best) and its
// meaning.  Its key, its legal values and its refusal text are its row of kKnobs in spmv_device.hip, which
// spmv_hip_set_tuning, spmv_hip_get_tuning and SPMV_TUNING go through; include/spmv_hip.h documents the keys.
#pragma once

inline int g_stream_cap = 0;        // nnz staged per stream workgroup (fixed at upload); 0 = by matrix size
inline int g_stream_block = 256;    // threads per csr_stream workgroup
inline int g_stream_nt = 1;         // non-temporal loads for col/val in the gather stream kernels
inline int g_stream_xcd = 0;        // blocks per XCD run (xcd_chunked); 0 = default, -1 = one contiguous eighth per XCD
inline int g_stream_kind = -1;      // -1 = auto (x-window kernel or tiles when the handle has that plan, else csr_stream), 5 = x-window,
                                    // 6 = tiles, 0 = csr_stream
inline int g_stream_tile = -1;      // csr_tile plan at upload: -1 = auto (no x-window plan, enough rows), 0 = never, 1 = whenever no x-window plan
inline int g_tile_lmax = 1536;      // rows longer than this stay with the split-row kernels (1024 until round 3: config 5 1016 us at 1024,
                                    // 1000 at 1536, 1001 at 2048; with the expanded short rows 942 / 927 / 930)
inline int g_tile_rows = 0;         // rows per block: 0 = auto, else a multiple of 256 in 256..kTileRowsMax
inline int g_halo_split = 1;        // halo setup splits the handle by columns (1) or by blocks only (0); read by spmv_hip_comm_halo_setup
inline int g_halo_overlap = 1;      // power iteration with halo: exchange beside the interior blocks (1) or strictly in order (0)
inline int g_tile_pack = 1;         // 1: passes that can be staged store head | row | column offset in one 32-bit word (no key read)
inline int g_tile_long = 1;         // 1: the rows beyond the tile limit get a tile plan of their own (compacted rows, work items, slabs) when
                                    // they hold >= 2^20 entries together, 2: always, 0: never
inline int g_tile_balance = 1;      // 1: row blocks of about equal entry counts (keeps the workgroups in step), 0: equal row counts
inline int g_tile_min_pass = 256;   // windows of a packed plan with fewer entries than this (and sparser than 1 per 16 columns) go to the remainder; 0: none
inline int g_tile_places = 0;       // 0: the chip's (2 or 1 workgroups per CU) | the number of workgroup places the streams / the block count are made for
inline int g_tile_items = 1008;     // work items the long rows' passes are dealt out to (about); two rounds of the 512 places: 1.222 ms on the
                                    // power-law matrix against 1.248 with 4096, 1.231 with 504
inline int g_local_patterns = -1;   // x-window plans: -1 auto (a pattern plan where it holds a quarter of the slots at most), 0 never, 1 always;
                                    // read at upload (the plan) and at launch (0: the slot stream)
inline int g_local_share = -1;      // x-window plans: equal segments / relative line lists stored once: -1 auto (on), 0 off, 1 on, 2 on with a
                                    // hash of the length only; takes effect at the next upload
inline int g_local_segment_cap = 0; // pattern plans of CSR handles: no segment wider than this many bytes; 0: the LDS budget's cap; next upload
inline int g_tile_mid_items = 0;    // work items of the middle tier (0: three rounds of the CUs)
inline int g_tile_streams = 1;      // 1: one csr_tile workgroup per place of the chip walks several row blocks back to back
inline int g_tile_fit = 1;          // 1: (auto rows) the number of row blocks is fitted to whole rounds of the chip's workgroup places
inline int g_skew_rows = 1;         // 1: gather-kernel handles hand rows far longer than the average to the split-row kernels
inline int g_tile_probe = 0;        // measurement only: bit 0 loads, staging and barriers only, bit 1 no gathers, bit 2 no run sums (y is then wrong), bit 3 one workgroup per CU
inline int g_probe_depth = 4;       // loads in flight per lane of the stream probe (4 | 16)
inline int g_tile_gather_ahead = 0; // 1: plans with gather passes run the csr_tile instantiation that gathers one pass early; read at launch;
                                    // measured: no gain (profiles/r3_ab_gather_ahead.txt)
inline int g_tile_expand = -1;      // plans with gather passes: -1 auto, 0 never, 1 always: x expanded into entry order ahead of csr_tile
                                    // (tile_expand + csr_tile<.., XE>); read at upload (the plan) and at launch (0: the gather passes)
inline int g_tile_mid_lo = 0;       // a scattered matrix's rows longer than this (up to tile_lmax) form the middle tier; 0: auto (48 entries
                                    // for fp32, 128 for fp64); next upload
inline int g_tile_mid = 1;          // 1: scattered plans get that tier (when it holds >= 2^22 entries), 0: never; next upload
inline int g_place_tries = 12;      // other placements of the value array upload tries for large handles (0: none); next upload
inline int g_tile_plan_on_device = 1;  // 1: the csr_tile plan is built by kernels (tile_plan_device.hpp), 0: by host threads (tile_plan.hpp); next upload
inline int g_tile_density = 4;      // a pass is staged when it holds at least one entry per this many columns of its window; 0: never
inline int g_gather_mode = 0;       // all-gatherv: 0 = one ncclBroadcast per owner in a group, 1 = padded ncclAllGather + scatter
inline int g_local_nt = -1;         // non-temporal loads in the x-window kernels: -1 = auto (off while the matrix fits the Infinity Cache)
inline int g_local_cap = 0;         // stage of the x-window plan: 0 = auto, 1024, 2048 or 3072; next upload
inline int g_stream_local = 1;      // build the x-window plan at upload when it pays; next upload
inline int g_plan_on_device = 1;    // ... with the device kernels where they apply (0: always on the host); next upload
