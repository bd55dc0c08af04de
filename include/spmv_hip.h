/*
 * spmv_hip.h -- C-ABI of the MI355X (gfx950) SpMV device layer.
 *
 * This is the one NEW seam the build adds to the reference's header surface.
 * It sits where the reference's CUDA driver talks to the device
 * (/root/reference/main_cuda.cu): device allocation + upload (:135-145 CSR,
 * :369-402 HLL), the six kernel launch sites (:166, :238, :317 CSR; :454,
 * :568, :637 HLL), the per-iteration result copy-back (e.g. :183) and the
 * frees (:682-685, :731-744).  The shape is the one that driver dictates:
 * upload once -> run many -> fetch y.
 *
 * Conventions (the reference's own, libs/csr_matrix.h / src/csr_matrix.c:74-78):
 *   - plain C: pointers and sizes only, no C++/torch types;
 *   - every call returns 0 on success and -1 on failure; nothing in the
 *     library calls exit(); the message of the last failure is available from
 *     spmv_hip_last_error();
 *   - host arrays are borrowed for the duration of the call only; device
 *     handles are opaque and owned by the library;
 *   - one host thread, one device per process (multi-GPU = one process per
 *     GPU; see spmv_hip_comm_* below);
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with -1.
 *
 * Reference-side binding: see INTEGRATION.md.
 */
#ifndef SPMV_AMD_SPMV_HIP_H
#define SPMV_AMD_SPMV_HIP_H

#include <stddef.h>

#include "csr_matrix.h"
#include "hll_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmv_csr_dev spmv_csr_dev; /* a CSR matrix (or a row block of one) resident in HBM */
typedef struct spmv_hll_dev spmv_hll_dev; /* an HLL matrix resident in HBM as one flat slab */

/* CSR kernel selection.  1..3 answer the reference's three CUDA CSR kernels
 * (cuda_src/csr_matrix_cuda.cu:122-241); 4 has no reference counterpart. */
enum {
    SPMV_CSR_AUTO = 0,       /* pick from the matrix' row-length statistics */
    SPMV_CSR_THREAD_ROW = 1, /* one lane per row            (replaces spmv_csr_naive_kernel) */
    SPMV_CSR_WAVE_ROW = 2,   /* one 64-lane wavefront per row, 2-wide vector loads
                                (replaces spmv_csr_warp_kernel) */
    SPMV_CSR_SUBWAVE = 3,    /* 2..32 lanes per row, picked from mean nnz/row
                                (replaces spmv_csr_warp_shared_memory_kernel's slot:
                                the x-cache idea is dropped) */
    SPMV_CSR_STREAM = 4      /* nnz-balanced row blocks streamed through LDS: csr_stream_local (x lines of
                                the block staged in LDS, 16-bit local columns) when upload found an x-window
                                plan for the matrix; csr_tile (row-block accumulators in LDS, column passes
                                that keep the gathered band of x in L2, dense passes staged in LDS) for large
                                matrices with scattered columns; else csr_stream (gathers); what AUTO resolves to */
};

/* HLL kernel selection.  1..3 answer cuda_src/hll_matrix.cu:346-479. */
enum {
    SPMV_HLL_AUTO = 0,
    SPMV_HLL_THREAD_ROW = 1, /* one lane per row over the row-major slab (spmv_hll_naive_kernel) */
    SPMV_HLL_SUBWAVE = 2,    /* a lane group per row                     (spmv_hll_warp_kernel) */
    SPMV_HLL_LDS = 3         /* row-aligned slab windows staged through LDS (spmv_hll_warp_shared_kernel_v1's
                                slot): hll_lds_local with an x-window plan; for a large slab with scattered columns
                                the 2-D tile kernel over the slab's rows; else hll_lds; what AUTO resolves to */
};

typedef struct {
    int M_local;           /* rows held by this handle                          */
    int M_total;           /* rows of the whole matrix (length of y)            */
    int N;                 /* columns (length of x)                             */
    int row0;              /* first global row of this handle's block           */
    long long nz;          /* stored entries held by this handle                */
    int value_bytes;       /* 8 = fp64, 4 = fp32                                */
    int auto_variant;      /* what SPMV_*_AUTO resolves to                      */
    int lanes_per_row;     /* SUBWAVE group width chosen at upload              */
    int stream_blocks;     /* workgroups of the STREAM / LDS kernel             */
    int long_rows;         /* rows split over several workgroups                */
    long long slots;       /* HLL only: padded slots S                          */
    int hacks;             /* HLL only: number of hacks                         */
    long long algo_bytes;  /* algorithmic HBM bytes of one SpMV  */
    long long device_bytes;/* HBM held by the handle                            */
    int local_blocks;      /* CSR: workgroups of the x-window stream kernel, 0 = matrix has no plan */
    int local_stage_lines; /* CSR: x lines (128 B) its widest block stages in LDS */
    long long local_lines; /* CSR: x lines listed over all blocks                 */
    long long stream_bytes;/* CSR: bytes the x-window kernel really streams from HBM:
                              nz (val + 2) + 4 lines + 24 blocks + 4 (M + 1) + val (M + N);
                              0 without a plan (then algo_bytes is what moves)    */
    int stream_kernel;     /* which kernel STREAM / LDS (and AUTO) launches with default tuning:
                              CSR 0 csr_stream, 1 csr_stream_local, 2 csr_stream_short, 3 csr_tile;
                              HLL 0 hll_lds, 1 hll_lds_local, 2 csr_tile over the slab's rows (padding slots included) */
    int tile_blocks;       /* CSR: row blocks (workgroups) of csr_tile, 0 = no tile plan */
    int tile_passes;       /* CSR: column passes over all blocks */
    int tile_split_rows;   /* CSR: rows beyond the tile limit (split-row kernels, stripe-ordered pieces) */
    long long tile_entries;        /* CSR: entries held by the tiles */
    long long tile_staged_entries; /* CSR: ... of which in passes whose x slice is staged in LDS */
    int tile_long_rows;            /* CSR: rows beyond the tile limit that got the long-row tile plan (compacted rows,
                                      a block's passes dealt out to many workgroups, slabs added in order) */
    int tile_long_items;           /* CSR: workgroups of that plan */
    long long tile_long_entries;   /* CSR: entries it holds */
    long long tile_staged_cols;    /* CSR: x values the staged passes copy to LDS per SpMV (all tile plans): traffic served by L2 */
    long long tile_remainder_entries; /* CSR: ... of tile_entries, in windows too sparse for a pass: added to y by tile_remainder behind the tiles */
    int tile_mid_rows;             /* CSR: rows of the MIDDLE tier of a scattered plan (128 < entries <= tile_lmax, compacted into
                                      blocks as tall as the LDS takes, packed plan, work items + slabs like the long rows) */
    int tile_mid_items;            /* CSR: workgroups of that plan */
    long long tile_mid_entries;    /* CSR: entries it holds */
    int place_tries;       /* placements of the value array that upload timed (0: not tuned -- small handle, or "place_tries" 0) */
    float place_first_us;  /* kernel time at the placement hipMalloc gave first */
    float place_best_us;   /* ... at the placement the handle kept */
    unsigned long long val_address; /* where the value array lies now (placement record of a bench line) */
    long long tile_expanded_entries; /* CSR: entry slots of a tile plan with gather passes that run on an expanded x (tile_expand
                                        writes every entry's x value in entry order, csr_tile streams it: "tile_expand") */
    long long pattern_slots; /* CSR: slots held by the pattern tables of an x-window plan (0: the kernel reads the 16-bit slot of
                                every entry) -- where most rows of a block are their predecessor shifted by a constant the
                                kernel rebuilds the slots from one segment per block: its pattern table and 6 bytes per row
                                ("local_patterns"); the slots counted are the tables' */
    float pattern_with_us;    /* (auto) what upload measured for its kernel with the pattern plan ... */
    float pattern_without_us; /* ... and without (0 / 0: no plan was built); the plan stays where it is at least 2 % faster */
    int pattern_segment_max;  /* CSR: bytes of the widest segment kept: the LDS the kernel adds per workgroup */
    int pattern_segment_cap;  /* CSR: ... and the widest the LDS budget allowed (7 resident workgroups per CU) */
    long long pattern_table_rows; /* CSR: rows of the blocks whose segment was wider: they rebuild their slots from their
                                     pattern table (rinfo, row_ptr and the table in memory) */
    long long pattern_segments_stored; /* CSR: segments held in memory: equal segments are stored once and shared by their
                                          blocks ("local_share"; 0: no segments) */
    long long local_lists_stored;   /* CSR: line lists held in memory: lists that are equal relative to their first line are
                                       stored once, each block adds its own first line (0: every block holds absolute ids) */
    long long local_lines_stored;   /* CSR: line ids the handle's list array holds (local_lines where every block keeps its own
                                       list; fewer once equal lists are shared), without the kernel's zeroed tail */
} spmv_dev_info;

/* ---- device ------------------------------------------------------------ */
int spmv_hip_device_count(void);               /* -1 when HIP itself is unusable */
int spmv_hip_init(int device);                 /* select device, create the library stream */
int spmv_hip_shutdown(void);
int spmv_hip_sync(void);                       /* wait for the library stream */
void *spmv_hip_stream(void);                   /* the hipStream_t kernels are launched on */
const char *spmv_hip_last_error(void);
int spmv_hip_device_name(char *buf, size_t len, int *compute_units, long long *hbm_bytes);
/* Evict L2 + Infinity Cache by streaming through a scratch buffer of `bytes`
 * (answers clear_gpu_cache / clear_cache_kernel, cuda_src/utility.cu:140-175;
 * the reference's 64 MiB is far below MI355X's 256 MiB Infinity Cache). */
int spmv_hip_flush_cache(size_t bytes);
/* Box state for bench records (round 3: the same code runs 180 or 200 us on the headline matrix depending on the box):
 * "key=value;..." with pci (bus id, to find the card under /sys/class/drm), arch, cus, sclk_khz / mclk_khz (HIP clock
 * attributes), mem_bus_bits, l2_bytes, hbm_bytes, xcds (from the chip's CU count: 32 per XCD).  Needs spmv_hip_init. */
int spmv_hip_device_state(char *buf, size_t len);
/* Read-only streaming probe: `iters` launches that each read `bytes` (a scratch buffer the library keeps) with 16-byte
 * non-temporal loads, 2048-thread-blocks grid-stride; mean / min event time per launch in ms.  What this box's HBM
 * gives a pure stream right now: the yardstick beside every kernel time in a bench line. */
int spmv_hip_stream_probe(size_t bytes, int warmup, int iters, float *ms_mean, float *ms_min);
/* the same read-only stream over device memory the caller names (16-byte aligned) */
int spmv_hip_stream_probe_at(const void *dptr, size_t bytes, int warmup, int iters, float *ms_mean, float *ms_min);
/* Gather probe: values per second the chip delivers when every lane of every gather wave-instruction reads a different
 * random line of a table of `table_bytes` (rounded down to a power of two of elements; <= 2 MiB: L2 resident on every
 * XCD), `waves_per_cu` wavefronts per CU with 8 independent gathers in flight each.  The ceiling of a gather-bound
 * kernel (csr_tile's gather passes, the gather stream kernels on scattered columns), as the stream probe is the
 * ceiling of a streaming one. */
int spmv_hip_gather_probe(int value_bytes, size_t table_bytes, int waves_per_cu, double *values_per_s);
/* Kernel tuning knobs, for A/B measurements.  Every key is listed here with its default, the measured best, in
 * parentheses.  Also settable through the environment, SPMV_TUNING="key=value,...", read by spmv_hip_init (items
 * without '=' are skipped, the first refused one fails the init).  A refused value leaves the knob as it was; booleans
 * (1 | 0) store value != 0.  None of the three entry points below needs a device.
 *   read at upload
 *     "stream_cap" (0)  0 (auto) | 1024 | 2048 | 3072 | 4096 | 8192 entries staged per workgroup of the gather stream
 *                     kernel; a value other than the x-window stage skips the x-window plan
 *     "stream_local" (1)  1 | 0   build the x-window plan (16-bit local columns + line lists) when the matrix allows
 *     "plan_on_device" (1)  1 | 0  build that plan with the device kernels where they apply (every block within the
 *                     line limit), else / otherwise on the host
 *     "local_cap" (0)  0 (auto = 2048) | 1024 | 2048 | 3072   stage of the x-window kernels (3072: +0.5..3 % on the
 *                     nlpkkt-like matrix depending on the box, -8 % on the cant-like one)
 *     "skew_rows" (1)  1 | 0   handles that run the gather kernels give rows longer than max(128, 16 x the average
 *                     row) to the split-row kernels (one workgroup per row piece) instead of leaving each to one lane
 *     "stream_tile" (-1)  -1 (auto) | 0 | 1   build the 2-D tile plan (csr_tile) when the matrix gets no x-window plan;
 *                     "tile_rows" (0) 0 (auto: 32 KiB of accumulators for banded matrices, as many rows as the LDS takes for
 *                     scattered ones: 16128 fp64 / 32512 fp32) | a multiple of 256 in 256..32768 rows per block;
 *                     "tile_lmax" (1536) 1..65536 longest row kept in the ordinary tiles;
 *                     "tile_density" (4) 0..4096 columns per entry up to which a pass is staged in LDS (0: never);
 *                     "tile_balance" (1) 1 | 0 row blocks of equal entry / row counts; "tile_long" (1) 1 | 0 | 2 a tile plan of
 *                     their own for the rows beyond tile_lmax (0: split-row kernels, 2: however few they are);
 *                     "tile_fit" (1) 1 | 0 (with tile_rows 0) the number of row blocks is fitted to whole rounds of the
 *                     workgroups the chip holds at once (512 banded / 256 scattered), blocks up to the tallest the LDS takes;
 *                     "tile_streams" (1) 1 | 0 one csr_tile workgroup per place of the chip walks several row blocks back to
 *                     back (0: one workgroup per block); "tile_places" (0) 0 (the chip's: 2 or 1 per CU) | a multiple of 8 up
 *                     to 4096: how many workgroups the streams and the block count are made for (tests);
 *                     "tile_items" (1008) 8..65536 work items the long rows' passes are dealt out to;
 *                     "tile_min_pass" (256) 0..2048 a packed plan's windows with fewer entries than this, and fewer than one per
 *                     16 columns, go to the remainder kernel instead of being a pass (0: no remainder);
 *                     "local_patterns" (-1) -1 | 0 | 1 (read at upload and at launch; a value below -1 stores -1, above 1
 *                         stores 1) x-window plans: the kernel rebuilds a block's
 *                         slots from a pattern table instead of reading them -- auto: built for streamed matrices of at least
 *                         12 entries per row whose tables hold at most a quarter of the slots, then kept only if upload
 *                         measures its kernel at least 2 % faster with it on this handle; 0 never; 1 always
 *                     "local_share" (-1) -1 | 0 | 1 | 2 (read at upload) x-window plans of CSR handles: every distinct pattern segment
 *                         and every distinct line list (relative to its first line) is stored once and shared by the blocks
 *                         that repeat it -- auto: on; 0 off (every block its own copy); 1 on; 2 on, with a hash of the
 *                         span's length alone, so that every group has to be told apart word by word (tests)
 *                     "local_segment_cap" (0) 0 | bytes (read at upload) pattern plans of CSR handles: segments wider than this
 *                         stay tables even where the LDS budget would take them (tests: both kinds of blocks on a small
 *                         matrix; 1: no segments at all); 0: the LDS budget alone (spmv_hip_csr_pattern_segment_cap)
 *                     "tile_mid_items" (0) 0 (three rounds of the CUs) .. 65536 work items of the middle tier
 *                     "tile_expand" (-1) -1 | 0 | 1 (read at upload and at launch; normalised like local_patterns) a tile plan
 *                         with gather passes runs on an
 *                         expanded x -- auto: from 2^22 entries on when under a tenth of them are staged, fp32 always, fp64
 *                         when x is beyond 100 MB; 0 never; 1 always
 *                     "tile_gather_ahead" (0) 0 | 1 (read at launch) plans with gather passes send a pass's gathers out one pass
 *                     early (twice as many in flight per CU) -- measured to buy nothing (1113 vs 1108 us on config 5, 514.9 vs
 *                     514.8 on uniformly random columns: profiles/r3_ab_gather_ahead.txt), hence off;
 *                     "tile_mid" (1) 1 | 0 a scattered plan gives its rows of more than "tile_mid_lo" (0) entries (0 = auto: 48 for
 *                     fp32, 128 for fp64; else 8..1024; up to tile_lmax) a tier of their own -- compacted, blocks as tall as the
 *                     LDS takes, every pass staged -- when they hold >= 2^22 entries;
 *                     "tile_plan_on_device" (1) 1 | 0 the plan is built by kernels from the CSR arrays in HBM (round 3) or by host
 *                     threads; the two builders give the same bytes;
 *                     "tile_pack" (1) 1 | 0 banded matrices get the PACKED plan (every pass cut at the 32 KiB window and
 *                     staged, keys in the column words, kernel instantiation without gather code) unless its passes
 *                     would average fewer than 256 entries; 0: always the plan with gather passes
 *     "place_tries" (12)  0..16: how many other placements of the value array a handle that streams >= 128 MiB of
 *                     values tries (a fresh allocation each, the kernel timed 2 + 6 launches on it), keeping the fastest.
 *                     Round 3 found the x-window kernel's time on the headline matrix to depend on WHERE the values lie:
 *                     the same matrix runs in 182-187 or in 199-205 us, deterministically per address
 *                     (profiles/r3_placement_*.txt); 0 keeps what hipMalloc gave first
 *   read at launch
 *     "stream_kind" (-1)  -1 (auto: x-window kernel when the handle has a plan, csr_tile when it has tiles, else
 *                     csr_stream) | 5 x-window | 6 csr_tile |
 *                     0 csr_stream; any other value is an error
 *     "stream_nt" (1) 1 | 0, "local_nt" (-1) -1 (auto) | 0 | 1   non-temporal hint on the streamed arrays
 *     "stream_xcd" (0)  blocks per XCD run: 0 default (16 for the x-window kernels, dispatch order otherwise),
 *                     -1 one contiguous eighth per XCD, n > 0 runs of n
 *     "stream_block" (256)  256 | 512 | 1024 threads (csr_stream at 4096 / 8192)
 *     "gather_mode" (0)  all-gatherv: 0 grouped broadcasts | 1 padded all-gather + scatter (see spmv_hip_comm_autotune)
 *   read by the multi-rank halo code
 *     "halo_split" (1)  1 | 0   spmv_hip_comm_halo_setup splits the handle by columns (1) or by whole blocks only (0)
 *     "halo_overlap" (1)  1 | 0   the power iteration with halo exchanges beside the interior blocks (1) or strictly in order (0)
 *   measurement only
 *     "tile_probe" (0)  stores value & 15: bit 0 csr_tile does loads, staging and barriers only, bit 1 no gathers, bit 2 no
 *                     run sums (y is then wrong), bit 3 one workgroup per CU
 *     "probe_depth" (4)  4 | 16 loads in flight per lane of spmv_hip_stream_probe */
int spmv_hip_set_tuning(const char *key, int value);
/* the value a knob holds now; -1 for an unknown key or a NULL argument */
int spmv_hip_get_tuning(const char *key, int *value);
/* the key of knob `index` (0, 1, ...: every key set_tuning takes, once), NULL past the last */
const char *spmv_hip_tuning_key(int index);

/* raw device buffers, for callers that keep x / y on the device themselves */
int spmv_hip_malloc(void **dptr, size_t bytes);
int spmv_hip_free(void *dptr);
int spmv_hip_memcpy_h2d(void *dptr, const void *hptr, size_t bytes);
int spmv_hip_memcpy_d2h(void *hptr, const void *dptr, size_t bytes);
int spmv_hip_memset(void *dptr, int byte, size_t bytes);

/* ---- CSR --------------------------------------------------------------- */
/* Upload rows [row0, row1) of a host CSR matrix (row_ptr has M+1 entries and
 * is NOT rebased by the caller).  row0 = 0, row1 = M uploads everything.
 * x and y buffers of full length (N, M) are allocated with the handle. */
int spmv_hip_csr_upload(int M, int N, const int *row_ptr, const int *col_idx,
                        const double *values, int row0, int row1, spmv_csr_dev **out);
int spmv_hip_csr_upload_f32(int M, int N, const int *row_ptr, const int *col_idx,
                            const float *values, int row0, int row1, spmv_csr_dev **out);
/* Host-only self-check of what upload precomputes (workgroup blocks, split rows, the x-window plan: 16-bit
 * local columns + per-block line lists) for a CSR structure; needs no device.  0 when every invariant holds;
 * stats[6] (optional): gather blocks, x-window blocks (0 = no plan), listed lines, widest block's lines, long
 * rows, rows handed to the split-row kernels because they alone touch too many lines. */
int spmv_hip_csr_plan_check(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes, int *stats);
/* The same for the csr_tile plan (row blocks x column passes, see spmv_dev_info.tile_*): builds it as upload
 * would with the given parameters (rows per block: multiple of 256 in 256..32768; lmax: longest row kept in the
 * tiles; density: columns per entry up to which a pass is staged; chunk: 2048 entries per pass; balance: 1 = row blocks of about equal entry counts) and replays the kernel's bookkeeping with
 * integer checksums; needs no device.  Both kinds of plan are built and checked: the one with gather passes, then
 * the PACKED one (every pass cut at the window and staged, column words carry the keys: what upload builds for
 * banded matrices, run by the kernel instantiation without gather code).  stats[12] (optional), six per kind in
 * that order: row blocks, passes, entries in tiles, entries in staged passes, rows left to the split-row
 * kernels, widest staged window (columns). */
int spmv_hip_csr_tile_plan_check(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes,
                                 int rows_per_block, int lmax, int density, int chunk, int balance, long long *stats);
/* What upload WOULD decide for a CSR structure under the current tunings (host only, values taken as 1): stats[10] =
 * a tile plan is built (0: the gather kernels keep the matrix), packed plan, scattered geometry (one workgroup per
 * CU), rows per block the kernel is launched for, row blocks, streams (workgroups), passes, rows of the tallest
 * block, work items of the long rows' plan, entries in the ordinary tiles. */
int spmv_hip_csr_tile_auto_plan(int M, int N, const int *row_ptr, const int *col_idx, int value_bytes, long long *stats);
/* Digests of the arrays of a handle's csr_tile plans (the tests' way of saying "the plan built on the device is the plan
 * the host builder makes"): digest[2 k] = elements, digest[2 k + 1] = a hash of the bytes of array k, 32 arrays (entry
 * arrays, pass descriptors, stream tables, remainder, the long rows' plan, the middle tier); digest has 64 entries. */
int spmv_hip_csr_tile_digest(const spmv_csr_dev *m, unsigned long long *digest);
int spmv_hip_hll_tile_digest(const spmv_hll_dev *m, unsigned long long *digest);
/* COO triplets (0-based, any order) -> a CSR handle, built ON THE DEVICE (upload of the
 * triplets, one stable radix sort by (row, column), row pointers and the x-window plan by kernels).  Same
 * matrix as convert_in_csr + spmv_hip_csr_upload_matrix; entries that repeat one (row, column) keep file
 * order here (the reference's quicksort leaves them in its own order), which only reorders equal-column
 * terms of a row's sum. */
int spmv_hip_csr_from_coo(int M, int N, long long nz, const int *I, const int *J, const double *val,
                          spmv_csr_dev **out);
/* the handle's CSR arrays back to the host: row_ptr[M_local + 1] rebased to 0, col[nz], val[nz] (handle's
 * dtype); any pointer may be NULL */
int spmv_hip_csr_download(const spmv_csr_dev *m, int *row_ptr, int *col, void *val);
/* New numbers on the handle's pattern: the handle's own nz values (a row-range handle: its own rows' entries), in the
 * handle's dtype and in its own entry order -- the order spmv_hip_csr_download returns -- from a host array, or (_on)
 * from a device array on `stream` (NULL: the library's), without synchronising with the host once the handle's first
 * update has been made.
 * After the call the handle IS the upload of (its pattern, the new values) under the plan it already has: every launch
 * (each variant, SpMM, run_part, the solvers) gives that upload's bytes, spmv_hip_csr_download returns the new values and
 * spmv_hip_csr_tile_digest is that upload's digest under the same knobs.  Nothing an upload decides reads a value, so
 * spmv_hip_csr_info and spmv_hip_csr_addresses do not change: the value array is written in place, where the placement
 * search put it; the zero entries behind it and every padding slot of a tile tier stay zero.  Non-finite values are
 * copied like any other.  Rows may be unsorted and may repeat a (row, column) pair.
 * Cost: one copy of nz values; a handle with tile plans also regathers the tiers' value arrays (ordinary tiles, their
 * remainder, the long rows' and the middle tier) through source maps, one int per slot, which the handle's FIRST update
 * builds on the host from the plan it holds (one analysis: the pattern and the plans' columns and keys come back once)
 * and the handle keeps.  An upload that is never followed by an update allocates and runs nothing for this.
 * Objects built FROM the handle -- a transpose, an HLL conversion, a preconditioner, a column split -- hold values of
 * their own and do not follow.
 * A HIP error in the middle of an update (a failed copy or launch, not a refusal) leaves `val` and the tile tiers'
 * value arrays in an undefined mix of old and new values: upload again.
 * -1 with the handle untouched: a NULL argument; a handle made of tile plans alone; a handle that holds a column split
 * (spmv_hip_csr_split_columns: its parts hold values of their own.  Drop it with a split over all N columns and split
 * again after the update). */
int spmv_hip_csr_update_values(spmv_csr_dev *m, const void *val_host);
int spmv_hip_csr_update_values_on(spmv_csr_dev *m, const void *d_val, void *stream);
/* counts[2] = updates made so far, bytes of the source maps on the device (0: none needed, or no update yet);
 * us[2] = the host time of the first update's analysis, the device time of the last update (copy and gathers; waits
 * for it), both in microseconds. */
int spmv_hip_csr_update_info(const spmv_csr_dev *m, long long *counts, double *us);
/* A^T of a whole CSR handle, built on the device, as a new handle of N rows and M columns with the same dtype.
 * Row j of the result holds the entries of column j of A in ascending row order.  Entries that repeat a (row, column)
 * pair keep their order in A.  Values are moved, never combined, so the arrays are a permutation of A's: bit-exact.
 * The build is one stable radix sort of the entries by column on the device; only the N + 1 row pointers of A^T cross
 * to the host.  The result is an ordinary handle: upload's plans and searches apply to it, and it owns its arrays
 * (freeing either handle leaves the other usable).
 * -1: NULL argument, a row-range handle (row0 != 0 or M_local != M_total), a handle without its CSR arrays
 * (tiles-only), M * value_bytes (the transpose's x) beyond the kernels' 32-bit gather range.  *out stays NULL on
 * failure. */
int spmv_hip_csr_transpose(const spmv_csr_dev *m, spmv_csr_dev **out);
/* C = A B of two whole CSR handles of the same dtype (A: M x K, B: K x N), built on the device, as a new M x N handle.
 * The rows of A and B may be unsorted and may repeat a (row, column) pair.  C has canonical rows (columns ascending, no
 * repeats) and a structural pattern: (i, c) is present exactly when some entry a_ij and some entry b_jc exist; a sum
 * that cancels to 0.0 stays.  The value is that of the serial loop
 *     for e in row i of A, in entry order:  j = colA[e], a = (double)valA[e]
 *         for f in row j of B, in entry order:  c = colB[f], p = a * (double)valB[f]      (one rounded product)
 *             acc[c] = p if c is new in row i, else acc[c] + p                              (one rounded sum)
 * rounded once to the handle's dtype: the same additions in the same order, never a fused multiply-add, no atomics,
 * so two calls give the same bytes and the result is what the AMG setup's host product (host/amg_plan.c) computes.
 * Non-finite values reach exactly the entries whose sums contain them.
 *   block_products   the on-chip tier's cap: rows are cut into blocks of at most this many products (and 4096 rows)
 *                    that one workgroup expands, sorts and compresses in LDS.  0: auto (4096); a power of two in
 *                    [64, 4096]; -1: no on-chip tier.  A row with more products (with -1: with any) is a long row
 *   chunk_products   long rows go through HBM (expansion, one stable radix sort, compress) in chunks of whole rows of
 *                    at most this many products (a row larger than that is a chunk of its own).  0: auto (2^23), else >= 64
 * Both passes run twice, once for the rows' entry counts (keys only) and once for columns and values, so C's arrays are
 * allocated at their exact size and the workspace is the counts, the block list and one chunk.
 * C is an ordinary handle (upload's plans, its own arrays, independent of A and B, which are not modified).
 *   stats (8, may be NULL)  products, entries of C, on-chip blocks with products, rows in them, long rows, chunks, the
 *                           largest row's products, the largest row's entries
 *   ms (4, may be NULL)     host milliseconds of count, symbolic, numeric, adopt
 * -1 with a message (*out NULL, A and B usable): NULL argument, A's columns != B's rows, different dtypes, a row-range
 * or tiles-only handle, block_products / chunk_products outside the above, more entries in C than a handle indexes,
 * N * value_bytes beyond the kernels' 32-bit gather range, a failed allocation. */
int spmv_hip_csr_spgemm(const spmv_csr_dev *a, const spmv_csr_dev *b, int block_products, long long chunk_products,
                        spmv_csr_dev **out, long long *stats, double *ms);
/* The row plan of that product (host only; no device needed) from the rows' product counts.  The rows are cut in order
 * into n_blocks contiguous blocks [block_row[k], block_row[k + 1]) that partition [0, M).  A row with more than
 * block_products products (0: 4096; -1: any product at all) is a long row: it is the last row of its block, is listed
 * in long_row (ascending) and is left to the global tier.  The other rows of a block hold at most block_products products
 * together, and a block has at most max_rows rows (1 .. 4096), its long row included.  block_row has M + 1 entries and
 * long_row M.  -1: NULL argument, M < 0, a negative count, block_products not 0, -1 or a power of two in [64, 4096],
 * max_rows outside [1, 4096]. */
int spmv_spgemm_plan(int M, const long long *products, int block_products, int max_rows, int *block_row, int *n_blocks,
                     int *long_row, int *n_long);
/* C = alpha A + beta B of two whole M x N CSR handles of the same dtype T, built on the device, as a new M x N handle;
 * with b = NULL, C = alpha canon(A).  a == b is allowed.
 *   canon(X)   X with canonical rows (columns ascending, no repeats): the value at (i, c) is the serial sum in double of
 *              row i's entries with column c, in entry order (the first entry starts the sum, every addition one rounded
 *              operation), rounded once to T.  It is the product X I of spmv_hip_csr_spgemm, byte for byte.
 *   C          canonical rows on the union of the patterns of canon(A) and canon(B).  The pattern is structural: A - A
 *              keeps A's pattern with zero values, beta = 0 keeps B's entries.  With a' and b' the values of canon(A) and
 *              canon(B):  both present: T(fl(fl(alpha a') + fl(beta b')));  A alone: T(fl(alpha a'));  B alone:
 *              T(fl(beta b')).  Every product and sum is one rounded double operation, never a fused multiply-add, and
 *              there are no atomics in the values: two calls give the same bytes.  Non-finite values reach exactly the
 *              entries whose formula contains them; alpha = 0 gets no shortcut (0 * inf is NaN at that entry alone).
 *   method     0: auto (an operand whose rows are not canonical goes through the product's tiers as X I first, then the
 *              merge); 1: merge only (an operand that is not canonical is refused); 2: both operands through X I first
 *   lanes      lanes per row of the merge kernels: 0 = auto (from the mean of len A_i + len B_i), else a power of two
 *              in [1, 64]
 *   long_row   the combined length len A_i + len B_i from which a row gets a whole workgroup: 0 = auto (32 trips of the
 *              row's lanes, between 256 and 2048), else >= 1
 * The canonical check (one pass over row_ptr and col of each operand) runs on every call.  The merge runs twice, once for
 * the rows' entry counts (every entry of A looks its column up in B's row) and once for columns and values (every entry
 * computes its own final position), so C's arrays are allocated at their exact size.
 * C is an ordinary handle (upload's plans, its own arrays, independent of A and B, which are not modified).
 *   stats (6, may be NULL)  entries of C, entries present in both operands, A found canonical (0 / 1), B found canonical
 *                           (1 when absent), long rows, the largest row's entries
 *   ms (5, may be NULL)     host milliseconds of check, canonical, symbolic, numeric, adopt
 * -1 with a message (*out NULL, A and B usable): a or out NULL, different shapes, different dtypes, a row-range or
 * tiles-only handle, alpha or beta not finite, method / lanes / long_row outside the above, method 1 on an operand that is
 * not canonical (the message names it and its first offending row), more entries in C than a handle indexes, a failed
 * allocation. */
int spmv_hip_csr_add(const spmv_csr_dev *a, double alpha, const spmv_csr_dev *b /* may be NULL */, double beta,
                     int method, int lanes, int long_row, spmv_csr_dev **out, long long *stats, double *ms);
/* C = P A Q^T of a whole M x N CSR handle, built on the device, as a new M x N handle of the same dtype.  row_perm (M
 * entries) and col_perm (N entries) are host arrays; either may be NULL, the identity.  The gather convention:
 *     C[i, j] = A[row_perm[i], col_perm[j]]
 * Row i of C is row row_perm[i] of A.  Entry e of that row keeps its place in the row and its value bit for bit and gets
 * the column j with col_perm[j] == col[e].  Nothing is sorted or combined: repeated pairs stay repeated and C's rows are
 * unsorted in general (upload's plans take that; spmv_hip_csr_add with b = NULL sorts them).  Permuting C by the inverse
 * permutations gives A's arrays exactly.  With one symmetric permutation p (C = A permuted by p, p), a system A x = b
 * becomes C y = b[p] with x[p] = y.
 * Each permutation is checked on the device: the first position whose value lies outside the range or repeats an
 * earlier position is refused by name, position and value.  Only the row lengths (4 bytes per row) cross to the host.
 * C is an ordinary handle (upload's plans, its own arrays, independent of A, which is not modified).
 * -1 with a message (*out NULL, A usable): m or out NULL, a row-range or tiles-only handle, an array that is not a
 * permutation, a failed allocation. */
int spmv_hip_csr_permute(const spmv_csr_dev *m, const int *row_perm /* may be NULL */, const int *col_perm /* may be NULL */,
                         spmv_csr_dev **out);
/* ms[2]: host milliseconds of the device build and of the adopt of this thread's last successful spmv_hip_csr_permute */
int spmv_hip_csr_permute_ms(double *ms);
/* The reverse Cuthill-McKee ordering of a square matrix of n rows.  G is the graph with u ~ v iff u != v and the matrix
 * stores an entry at (u, v) or (v, u): stored zeros count, repeats count once, the diagonal is ignored.  deg(v) is the
 * number of neighbours of v; "smallest" means smallest (deg, index).
 *     seq = [];  visited = {}
 *     while some node is unvisited:
 *         s = the smallest unvisited node
 *         if peripheral > 0 and deg(s) > 0:
 *             repeat at most `peripheral` times:
 *                 t = the smallest node of the last level of a breadth-first search from s
 *                 if depth(t) > depth(s):  s = t   else: stop
 *                 (depth = the number of levels of the search from that node; a search reaches unvisited nodes only,
 *                  which are s's component)
 *         append s, mark it;  for every node v of seq from s on, in order:
 *             append v's unvisited neighbours in ascending (deg, index), mark them
 *     perm[i] = seq[n - 1 - i]                           new row i is old row perm[i]
 * Isolated nodes are the smallest nodes: they come first in seq in index order and last in perm.  The reordered matrix
 * is spmv_hip_csr_permute(m, perm, perm).
 *   peripheral   passes of the search for a start node far from the rest, 0 .. SPMV_RCM_MAX_PERIPHERAL
 *   stats (SPMV_RCM_STATS, may be NULL)  components (isolated nodes included), isolated nodes, levels (the expansions of
 *                the ordering: one per level of every component that is not an isolated node), chained levels, wide levels,
 *                launches of the searches and levels, searches run, the bandwidth max |i - j| over the stored entries
 *                before, and max |inv[i] - inv[j]| after
 * spmv_rcm_plan_build is the definition itself, one host thread, no device (chained levels, wide levels and launches
 * are 0).  -1: a NULL array, n < 0, row_ptr that does not start at 0 or descends, a column outside [0, n), peripheral
 * outside its range; -2: out of memory. */
#define SPMV_RCM_STATS 9
#define SPMV_RCM_MAX_PERIPHERAL 8
int spmv_rcm_plan_build(int n, const int *row_ptr, const int *col, int peripheral, int *perm, long long *stats);
/* The same perm, byte for byte, built on the device from a whole square handle.  The pattern of A + A^T comes from the
 * cores of spmv_hip_csr_transpose and spmv_hip_csr_add (no handle is made).  One sort of all nodes by (deg, index) gives
 * every node its rank, which stands for (deg, index) in all later keys, the start nodes (a cursor over the sorted list
 * that skips visited nodes) and the isolated nodes (one pass).  Inside one search the next level in seq order is the set
 * of unvisited neighbours of the frontier sorted by (place in seq of the earliest frontier parent, deg, index):
 *   wide level     a kernel gives lane groups to the frontier's rows and takes an integer atomicMin of the parent's place
 *                  into every unvisited neighbour (the result does not depend on arrival order); one radix sort of
 *                  (parent, rank) on the bits in use; a kernel writes the places.  Four bytes cross to the host: the next
 *                  frontier's size
 *   chained levels a run of levels whose frontier and next frontier hold at most chain_nodes nodes is one launch of one
 *                  workgroup: candidates in LDS, a bitonic sort, a barrier, the next level.  It stops when the frontier is
 *                  empty or the next one is too wide, and the wide tier goes on.  chain_nodes: 0 = auto (1024), -1 = never
 *                  chain, else a power of two in the range spmv_hip_rcm_chain_nodes reports (64 .. 4096: 8 bytes of LDS
 *                  per node)
 *   searches       the peripheral passes run the same expansion without the sort
 *   ms (3, may be NULL)   host milliseconds of graph, peripheral, order
 * Two calls give the same bytes.  -1 with a message: m NULL, perm NULL, a matrix that is not square, a row-range or
 * tiles-only handle, peripheral or chain_nodes outside the above, a failed allocation. */
int spmv_hip_csr_rcm(const spmv_csr_dev *m, int peripheral, int chain_nodes, int *perm, long long *stats, double *ms);
/* the chain_nodes spmv_hip_csr_rcm takes: the smallest and largest power of two and what 0 stands for (no device needed;
 * any pointer may be NULL) */
int spmv_hip_rcm_chain_nodes(int *smallest, int *largest, int *automatic);
/* convenience over the kept struct */
int spmv_hip_csr_upload_matrix(const CSRMatrix *csr, spmv_csr_dev **out);
void spmv_hip_csr_free(spmv_csr_dev *m);
int spmv_hip_csr_info(const spmv_csr_dev *m, spmv_dev_info *out);
/* device addresses of the handle's arrays (placement studies): out[8] = row_ptr, col, val, x, y, lcol, lines, ldesc4
 * (0 where the handle has none) */
int spmv_hip_csr_addresses(const spmv_csr_dev *m, unsigned long long *out);
/* Measurement only: one launch of the x-window kernel (fp64, 2048-entry stage) with per-workgroup time stamps behind
 * `warm` ordinary launches: stamps[3 * b + {0, 1, 2}] = start, end (ticks of the constant 100 MHz clock), dispatch id << 8
 * | XCD of block b; stamps has 3 * local_blocks entries.  warm + 1000: the stamped launch reads no slots (y is wrong);
 * warm + 2000: the second word is the time the block's records were back -- the end of its head -- instead of its end. */
int spmv_hip_csr_stamp_blocks(spmv_csr_dev *m, int warm, unsigned long long *stamps);
/* The widest pattern-plan segment (bytes) upload lets an x-window plan keep: its LDS copy beside the stage of
   max(local_cap * value_bytes, stage_lines * 128) bytes and the (local_cap + 8) 16-bit slots must not cost a resident
   workgroup of csr_stream_local per CU (at most the 7 its registers allow).  -1 on bad arguments.  No device needed. */
int spmv_hip_csr_pattern_segment_cap(int value_bytes, int local_cap, int stage_lines);
/* Move one array of the handle (same numbering) to an address of the form (multiple of `align`) + offset; align a
 * power of two >= 256, offset a multiple of 256 below it.  Round 3 found the x-window kernel's time on the headline
 * matrix to depend on where its arrays lie (profiles/r3_placement_*.txt); this is the tool that study used. */
int spmv_hip_csr_relocate(spmv_csr_dev *m, int which, unsigned long long align, unsigned long long offset);
/* the same with memory from HIP's virtual-memory API (hipMemCreate / hipMemAddressReserve / hipMemMap): the virtual
 * address is aligned to `align` exactly as asked, whatever hipMalloc would have chosen */
int spmv_hip_csr_relocate_vmm(spmv_csr_dev *m, int which, unsigned long long align, unsigned long long offset);

/* library-owned vectors: host -> x, run, y -> host (y has M_total entries;
 * this handle writes rows [row0, row0 + M_local) of it) */
int spmv_hip_csr_set_x(spmv_csr_dev *m, const void *x_host);   /* N values of the handle's dtype */
int spmv_hip_csr_run(spmv_csr_dev *m, int variant);             /* asynchronous on the library stream */
int spmv_hip_csr_get_y(spmv_csr_dev *m, void *y_host);          /* syncs, copies M_total values */
void *spmv_hip_csr_x_ptr(spmv_csr_dev *m);                      /* device pointers of those vectors */
void *spmv_hip_csr_y_ptr(spmv_csr_dev *m);

/* caller-owned device vectors (d_y points at element 0 of the FULL y) and
 * caller's stream (NULL = library stream) */
int spmv_hip_csr_run_on(spmv_csr_dev *m, int variant, const void *d_x, void *d_y, void *stream);

/* ---- CSR: several vectors per pass over the matrix (SpMM) ----------------- */
/* Y = A X for k vectors at once.  X: N x k, Y: M_total x k, both row-major (element (i, j) at i * k + j), values of the
 * handle's dtype.  The handle writes rows [row0, row0 + M_local) of Y and no other row.  Each row of a handle is read
 * from HBM once per call, whatever k is.  k = 1 is exactly spmv_hip_csr_run_on(m, SPMV_CSR_AUTO, ...) (same bits).
 * -1 for k < 1, NULL arguments, pointers not aligned to the element size, or a tiles-only handle. */
int spmv_hip_csr_spmm_on(spmv_csr_dev *m, int k, const void *d_X, void *d_Y, void *stream); /* NULL stream = library's */
int spmv_hip_csr_spmm(spmv_csr_dev *m, int k, const void *X_host, void *Y_host);  /* host arrays; syncs */
/* the reference timing protocol of spmv_hip_csr_time, for the k-vector product on library-owned scratch X / Y */
int spmv_hip_csr_spmm_time(spmv_csr_dev *m, int k, int warmup, int iters, float *ms_each);

/* The reference's timing protocol (main_cuda.cu:159-200): per iteration
 * [zero y if zero_y], record an event, launch, record an event; `warmup`
 * untimed iterations first.  ms_each receives `iters` kernel durations in
 * milliseconds.  The kernels overwrite every row of y, so zero_y only matters
 * for protocol fidelity (the memset sits outside the event pair either way). */
int spmv_hip_csr_time(spmv_csr_dev *m, int variant, int warmup, int iters, int zero_y,
                      float *ms_each);

/* ---- HLL --------------------------------------------------------------- */
/* total_rows = the matrix' M (the last hack may hold fewer than 32 rows). */
int spmv_hip_hll_upload(const HLLMatrix *hll, int total_rows, int N, spmv_hll_dev **out);
/* Host-only self-check of what HLL upload precomputes (slab offsets, workgroup windows, x-window plan); needs no
 * device.  stats[4] (optional): gather windows, x-window windows (0 = no plan), listed lines, widest window's lines. */
int spmv_hip_hll_plan_check(const HLLMatrix *hll, int total_rows, int N, int *stats);
/* One rank's share: hacks [hack0, hack1) = rows [32 hack0, min(32 hack1, total_rows)).  y keeps the
 * full length; the kernels write this handle's rows (HLL is split on hack boundaries). */
int spmv_hip_hll_upload_part(const HLLMatrix *hll, int total_rows, int N, int hack0, int hack1,
                             spmv_hll_dev **out);
/* `iters` launches captured once into a hipGraph and replayed `replays` times (after one warm-up
 * replay): mean time per SpMV with the per-launch host work out of the way -- the number that
 * matters for launch-bound matrices (cant: ~11 us kernel).  Also for HLL below. */
int spmv_hip_csr_time_graph(spmv_csr_dev *m, int variant, int iters, int replays, float *ms_per_iter);
int spmv_hip_hll_time_graph(spmv_hll_dev *m, int variant, int iters, int replays, float *ms_per_iter);

/* build the HLL slab ON THE DEVICE from a resident whole fp64 CSR matrix
 * (per-hack maximum, H-sized offset scan on the host, fill kernel); same slab as
 * convert_to_hll + spmv_hip_hll_upload give when no column repeats inside a row. */
int spmv_hip_hll_from_csr(const spmv_csr_dev *csr, spmv_hll_dev **out);
/* flat slab back to the host: hack_off[hacks + 1] (slot offsets, each hack starts on an even
 * slot), maxnz[hacks], JA / AS [hack_off[hacks]]; any pointer may be NULL */
void *spmv_hip_hll_x_ptr(spmv_hll_dev *m); /* device pointers of the handle's x [N] and y [M] */
void *spmv_hip_hll_y_ptr(spmv_hll_dev *m);
int spmv_hip_hll_download(const spmv_hll_dev *m, long long *hack_off, int *maxnz, int *JA, double *AS);
void spmv_hip_hll_free(spmv_hll_dev *m);
int spmv_hip_hll_info(const spmv_hll_dev *m, spmv_dev_info *out);
int spmv_hip_hll_set_x(spmv_hll_dev *m, const double *x_host);
int spmv_hip_hll_run(spmv_hll_dev *m, int variant);
int spmv_hip_hll_get_y(spmv_hll_dev *m, double *y_host);
int spmv_hip_hll_run_on(spmv_hll_dev *m, int variant, const void *d_x, void *d_y, void *stream);
int spmv_hip_hll_time(spmv_hll_dev *m, int variant, int warmup, int iters, int zero_y,
                      float *ms_each);

/* ---- HLL: several vectors per pass over the slab (SpMM) ------------------- */
/* Y = A X for k vectors at once, fp64.  X: N x k, Y: M_total x k, both row-major (element (i, j) at i * k + j).  The
 * handle writes rows [row0, row0 + M_local) of Y and no other row (hack-range handles and device-built slabs alike).
 * Each slot of the slab is read from HBM once per call, whatever k is; padding slots are multiplied like real ones, as
 * in every HLL SpMV kernel.  k = 1 is exactly spmv_hip_hll_run_on(m, SPMV_HLL_AUTO, ...) (same bits).  Results are a
 * fixed sequence of adds that depends on the slab and k only (no atomics; 16-byte and element loads of X / Y add in
 * the same order).  -1 for k < 1, NULL arguments or X / Y not aligned to 8 bytes (the HIP error state stays clean). */
int spmv_hip_hll_spmm_on(spmv_hll_dev *m, int k, const void *d_X, void *d_Y, void *stream); /* NULL stream = library's */
/* host arrays; syncs; copies back only the handle's rows of Y_host */
int spmv_hip_hll_spmm(spmv_hll_dev *m, int k, const double *X_host, double *Y_host);
/* the reference timing protocol of spmv_hip_hll_time, for the k-vector product on library-owned scratch X / Y */
int spmv_hip_hll_spmm_time(spmv_hll_dev *m, int k, int warmup, int iters, float *ms_each);

/* ---- multi-GPU: one process per GPU, rows split by nnz ------------------ */
/* Contiguous nnz-balanced row split for `parts` GPUs: the reference's greedy
 * (prepare_thread_distribution, src/csr_matrix.c:167-266) with fixed-size
 * output: bounds[0..parts] with bounds[0] = 0, bounds[parts] = M; a part may
 * be empty (bounds[p] == bounds[p+1]).  Pure host code, no device needed. */
int spmv_hip_partition_rows(int M, const int *row_ptr, int parts, int *bounds);
/* The same for HLL with the reference's hack partitioner (prepare_thread_distribution_hll,
 * src/hll_matrix.c:410-540, weight = padded slots): bounds[parts + 1] are HACK indices. */
int spmv_hip_partition_hacks(const HLLMatrix *hll, int parts, int *bounds);

/* RCCL communicator over the GPUs of one node.  Rank 0 creates the id
 * (SPMV_COMM_ID_BYTES opaque bytes) and hands it to the other processes by
 * any means (the Python host uses torch.distributed's store). */
#define SPMV_COMM_ID_BYTES 128
int spmv_hip_comm_get_id(void *id_bytes);
int spmv_hip_comm_init(const void *id_bytes, int rank, int nranks);
int spmv_hip_comm_destroy(void);
/* what RCCL reports for the communicator (ncclCommUserRank / ncclCommCount) */
int spmv_hip_comm_info(int *rank, int *nranks);
/* In-place all-gatherv of y over xGMI: rank r contributes
 * d_y[bounds[r] .. bounds[r+1]) and receives everybody else's rows, as one
 * grouped set of ncclBroadcast calls on `stream` (NULL = library stream).
 * value_bytes is 8 (fp64) or 4 (fp32). */
int spmv_hip_comm_allgatherv(void *d_y, const int *bounds, int value_bytes, void *stream);
/* The scatter half of the padded all-gather on its own: slice p of `d_stage` (at p * widest slice
 * values) -> rows [bounds[p], bounds[p+1]) of d_y, for every p but skip_rank (-1: all). */
int spmv_hip_comm_scatter_staged(const void *d_stage, void *d_y, const int *bounds, int ranks, int skip_rank,
                                 int value_bytes, void *stream);
/* Collective.  Times the two implementations of the all-gatherv on this node -- (0) one
 * ncclBroadcast per owner inside a group, in place; (1) a single ncclAllGather of slices padded to the
 * widest one into a staging buffer + one scatter kernel -- takes the maximum over ranks, checks that (1)
 * reproduces (0) bit for bit, and makes the faster one the mode spmv_hip_comm_allgatherv uses from
 * then on (also settable: spmv_hip_set_tuning("gather_mode", 0 | 1)).  d_y must already hold a
 * gathered vector.  ms_modes[2] (optional) receives the two times, ms_modes[1] < 0 if (1) was rejected. */
int spmv_hip_comm_autotune(void *d_y, const int *bounds, int value_bytes, int iters, int *mode_out,
                           float *ms_modes);
/* One multi-GPU step, timed: SpMV on this rank's rows then the all-gatherv of
 * the library-owned y, both on the library stream, events around each part.
 * ms_kernel / ms_exchange receive `iters` values (either may be NULL). */
int spmv_hip_csr_step_time(spmv_csr_dev *m, int variant, const int *bounds, int warmup, int iters,
                           float *ms_kernel, float *ms_exchange);
/* HLL twin; bounds are ROW bounds (32 x the hack bounds of spmv_hip_partition_hacks, last = M) */
int spmv_hip_hll_step_time(spmv_hll_dev *m, int variant, const int *bounds, int warmup, int iters,
                           float *ms_kernel, float *ms_exchange);

/* SURVEY 8(f) N4 -- iterated SpMV (power iteration as the skeleton): `iters` steps of
 * x <- A x / ||A x||_2 from the handle's current x; y = A x on this rank's rows, all-gatherv(y) when a
 * communicator exists (bounds = the row partition, else NULL), the 2-norm by a fixed-order device
 * reduction that every rank repeats over the gathered y (same bits everywhere, no extra collective).
 * No host synchronisation inside the loop; with one GPU and use_graph != 0 the loop is one hipGraph.
 * Out: x normalised iterate, y last A x, *lambda last ||A x||_2, *ms_total device time of the loop. */
int spmv_hip_csr_power_iterate(spmv_csr_dev *m, int variant, int iters, const int *bounds, int use_graph,
                               double *lambda, float *ms_total);

/* N4, second half -- the halo exchange of an iterated method: a rank needs only the entries of x its rows'
 * columns touch (its own range plus a halo on banded matrices), not the whole all-gathered vector.
 *   spmv_hip_csr_needed_ranges   those entries as at most max_ranges ascending ranges [lo, hi) (ranges[2 * max]),
 *                                from the handle's x-window plan; the whole vector when it has none
 *   spmv_hip_halo_plan           pure host logic, identical on every rank: from every rank's ranges (counts[ranks],
 *                                ranges[ranks * 2 * stride]) and the ownership bounds, the (peer, lo, hi) triples
 *                                this rank sends and receives (send / recv [3 * max_segments])
 *   spmv_hip_comm_halo_setup     collective: all-gathers the ranks' needs, runs the plan, keeps the segments
 *   spmv_hip_comm_halo_exchange  one group of ncclSend / ncclRecv on those segments, in place in d_vec
 *   spmv_hip_comm_halo_info      values sent / received per exchange, peers talked to
 *   spmv_hip_csr_power_iterate_halo   the power iteration with that exchange: partial norms + one all-reduce,
 *                                every rank scales its own range of x, halo segments of x travel */
/* N4, overlap of the exchange with the product.  A rank's x-window blocks are split into INTERIOR blocks (every
 * x line they list lies in the rank's own range [row0, row0 + M_local) of x: they can run before the halo has
 * arrived) and BOUNDARY blocks (the rest, plus rows outside the plan).
 *   spmv_hip_csr_split_interior   computes the split from the handle's plan (spmv_hip_comm_halo_setup calls it);
 *                                 counts[4] (optional): interior blocks, boundary blocks, entries in interior
 *                                 blocks, entries elsewhere.  A handle without an x-window plan has no interior.
 *   spmv_hip_csr_run_part         part 0 = interior blocks only, part 1 = everything else; 0 then 1 = one
 *                                 spmv_hip_csr_run_on(STREAM), bit for bit (d_x / d_y / stream NULL = the handle's)
 *   spmv_hip_csr_power_iterate_halo   uses it when a communicator exists: the halo exchange runs on a second
 *                                 stream beside the interior blocks, the boundary blocks wait for its event
 *                                 ("halo_overlap" tuning knob 1 | 0) */
/* N4, the second skeleton: `iters` steps of plain conjugate gradients for a symmetric positive definite A, from
 * x0 = 0: p is the handle's x (gathered / halo-exchanged every step exactly as in the power iteration: bounds = the
 * row partition when a communicator exists; use_halo != 0 after spmv_hip_comm_halo_setup), q = A p its y, every rank
 * keeps its rows of x and r.  Dot products are fixed-order device reductions; across ranks the partial sums are
 * all-gathered and added in rank order by every rank (same bits everywhere).  No host synchronisation in the loop.
 * b_host: the right-hand side, M_total values of the handle's dtype (a rank reads its own rows).  Out: x_host
 * (optional) the iterate after `iters` steps, M_total values; rr_hist (optional) [iters + 1] the squared residual
 * norm r.r before the first step and after every step; *ms_total device time of the loop. */
int spmv_hip_csr_cg(spmv_csr_dev *m, int variant, int iters, const int *bounds, int use_halo, const void *b_host,
                    void *x_host, double *rr_hist, float *ms_total);
/* k independent CG recurrences for a symmetric positive definite A, x0 = 0, sharing one SpMM per step (the loop of
 * spmv_hip_csr_cg with one alpha and one beta per column: not block CG).  The product is spmv_hip_csr_spmm_on on
 * library-owned P (N x k) and Q (M_total x k); k = 1 is the handle's AUTO SpMV and gives spmv_hip_csr_cg's bits
 * (variant SPMV_CSR_AUTO).  Column j's dot products add in an order that does not depend on j: permuting the columns
 * of B permutes the results bit for bit.  With a communicator every rank keeps its rows of X and R, P is all-gathered
 * with the row bounds scaled by k and the k dot products are all-gathered and added in rank order; there is no halo
 * exchange variant.
 * B_host: M_total x k row-major, values of the handle's dtype (a rank reads its own rows).
 * tol: column j freezes at the first step t with rs_j(t) <= tol^2 * rs_j(0) (tol = 0: only when rs_j = 0 exactly).
 *   A frozen column's x, r, p no longer change and its history repeats its last value.  It still rides in the SpMM.
 * tol = 0: exactly `iters` steps, no host synchronisation inside the loop.
 * tol > 0: the host reads one device word every 16 steps and stops once every column is frozen.
 * Out: X_host (optional) M_total x k; rr_hist (optional) (iters + 1) x k, r.r per column before step 1 and
 * after every step; iters_done (optional) [k] steps each column took; *ms_total device time of the loop.
 * -1: k < 1 or k > 64, non-square, tiles-only handle, n*k beyond int range, a communicator without bounds. */
int spmv_hip_csr_cg_multi(spmv_csr_dev *m, int k, int iters, double tol, const int *bounds,
                          const void *B_host, void *X_host, double *rr_hist, int *iters_done, float *ms_total);
/* BiCGSTAB (van der Vorst 1992) for a square, possibly nonsymmetric A: x0 = 0, shadow residual r^ = r0 = b.  Two
 * SpMVs per step (v = A p, t = A s) through the handle's launch for `variant` (SPMV_CSR_AUTO: whatever plan upload
 * picked), on library-owned p and s; fixed-order device reductions in double, fp64 scalars that stay on the device.
 * With a communicator every rank keeps its rows of x, r, r^, s, p all-gathered with `bounds` (two exchanges per step),
 * the partial sums all-gathered and added in rank order: every rank holds the same bits and stops at the same step.
 * There is no halo exchange variant.
 * Stops: s.s <= tol^2 rr0 (a half step: x += alpha p, r = s), r.r <= tol^2 rr0 (tol = 0: only at exactly 0),
 *   r^.v = 0 or r^.r' = 0 (BREAKDOWN_RHO), t.s = 0 or t.t = 0 (BREAKDOWN_OMEGA), a non-finite value counting as
 *   a breakdown.  A breakdown leaves x at the last full iterate.  After a stop x and r no longer change and the
 *   history repeats its last value.
 * tol = 0: exactly `iters` steps are launched, no host synchronisation inside the loop.
 * tol > 0: the host reads one device word every 16 steps and ends the loop once the solve has stopped.
 * b_host: M_total values of the handle's dtype (a rank reads its own rows).  Out: x_host (optional) M_total values;
 * rr_hist (optional) [iters + 1] r.r before step 1 and after every step (s.s at a converged half step);
 * info (optional) [3]: steps taken (a converged half step counts, a step that broke down before its update does
 * not), the status (SPMV_BICG_*), 1 when the solve stopped at a half step; *ms_total device time of the loop.
 * -1: non-square, iters < 0, tol < 0 or not finite, a communicator without bounds, a row-range handle without a
 * communicator, more ranks than the library supports. */
enum { SPMV_BICG_RAN_ALL = 0, SPMV_BICG_CONVERGED = 1, SPMV_BICG_BREAKDOWN_RHO = 2, SPMV_BICG_BREAKDOWN_OMEGA = 3 };
int spmv_hip_csr_bicgstab(spmv_csr_dev *m, int variant, int iters, double tol, const int *bounds,
                          const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total);
/* CGLS (conjugate gradients on the normal equations, the stable form of Bjorck, Elfving and Strakos 1998) for
 * min ||A x - b||_2^2 + damp^2 ||x||_2^2, A of any shape (M x N), x0 = 0.  mt must be a transpose of m
 * (spmv_hip_csr_transpose): same dtype, N x M, the same nz.  Only those properties are checked.
 *   r = b, s = A^T r, p = s, gamma = s.s
 *   each step: q = A p (m's AUTO launch), delta = q.q + damp^2 p.p, alpha = gamma / delta,
 *              x += alpha p, r -= alpha q, s = A^T r - damp^2 x (mt's AUTO launch), gamma' = s.s,
 *              stop if gamma' <= tol^2 gamma0, beta = gamma' / gamma, p = s + beta p
 * From x0 = 0 it converges to the minimum-norm least-squares solution when damp = 0.
 * Scalars are fp64 on the device.  Dots are accumulated in double in a fixed order: two calls give the same bits.
 * tol = 0: exactly `iters` steps, no host synchronisation.  tol > 0: one device word is read every 16 steps.
 * Breakdown: delta == 0 while gamma > 0, or any non-finite scalar.  It stops with x at the last full iterate and
 * never writes a NaN into x.  gamma0 == 0 (A^T b = 0): converged at step 0, x = 0.
 * After a stop x and r no longer change and both histories repeat their last value.
 * Single device: no communicator, no row bounds.
 * b_host: M values of the handle's dtype.  Out (all optional): x_host N values; ss_hist [iters + 1] s.s;
 * rr_hist [iters + 1] r.r (the recurrence's ||b - A x||^2); info[2] = {steps, status}; *ms_total device time.
 * -1: NULL m / mt / b_host, mt not N x M or nz / dtype differ, a row-range or tiles-only handle, iters < 0,
 * tol or damp negative or not finite. */
enum { SPMV_CGLS_RAN_ALL = 0, SPMV_CGLS_CONVERGED = 1, SPMV_CGLS_BREAKDOWN = 2 };
int spmv_hip_csr_cgls(spmv_csr_dev *m, spmv_csr_dev *mt, int iters, double tol, double damp, const void *b_host,
                      void *x_host, double *ss_hist, double *rr_hist, int *info, float *ms_total);
/* Preconditioners of a square CSR handle, built on the device: M = the diagonal (JACOBI, block = 1) or the block
 * diagonal of `block` x `block` blocks (BLOCK_JACOBI, block in [1, 32]) of the handle's own rows [row0, row0 + M_local).
 * Blocks start at row0; the last one may be shorter.  Entries that repeat a (row, column) pair are added in entry order
 * (block = 1: the diagonal is their left-to-right fp64 sum).  Each block is inverted in fp64 (Gauss-Jordan with partial
 * pivoting, the first largest |pivot| wins; JACOBI: 1.0 / d, correctly rounded) and stored once rounded to the
 * handle's dtype.  BLOCK_JACOBI with block = 1 gives JACOBI's bytes.  P owns its arrays: P and the handle may be freed
 * in either order.  Two builds give the same bytes.
 * -1 (*out stays NULL, the HIP error state stays clean): a missing, zero or non-finite diagonal, a zero or non-finite
 * pivot or inverse (the message names the first bad row or block), a bad kind or block, a non-square matrix, a
 * tiles-only handle.
 *   spmv_hip_precond_info      info[5] = kind, block, rows, row0, value_bytes
 *   spmv_hip_precond_apply     z = M^-1 r on P's rows: r_host, z_host hold `rows` values (element i = row row0 + i); syncs
 *   spmv_hip_precond_apply_on  the same on device vectors, asynchronous on `stream` (NULL = the library's)
 * The apply accumulates each row's sum in double and rounds it once. */
typedef struct spmv_precond spmv_precond;
enum { SPMV_PRECOND_JACOBI = 1, SPMV_PRECOND_BLOCK_JACOBI = 2 };
int spmv_hip_csr_precond_build(const spmv_csr_dev *m, int kind, int block, spmv_precond **out);
void spmv_hip_precond_free(spmv_precond *P);
int spmv_hip_precond_info(const spmv_precond *P, int *info);
int spmv_hip_precond_apply(const spmv_precond *P, const void *r_host, void *z_host);
int spmv_hip_precond_apply_on(const spmv_precond *P, const void *d_r, void *d_z, void *stream);
/* Sparse triangular solves on a square CSR handle.  T is the lower (upper) triangle of the handle's own diagonal block
 * A[row0:row1, row0:row1]: entries on the other side of the diagonal and entries in columns outside [row0, row1) are
 * ignored, with SPMV_TRSV_UNIT the stored diagonal as well.  Rows may be unsorted and may repeat a (row, column) pair:
 * repeats are added in entry order in fp64.  The solver owns a private copy of its triangle, stored in level order
 * (row i's level = 1 + the largest level among the rows it reads) with the off-diagonal values rounded to the handle's
 * dtype and the diagonal kept as its inverse (1.0 / d in fp64, rounded once); it never changes the handle and may
 * outlive it.  A solve is one launch per wide level and one launch per run of consecutive narrow levels (one
 * workgroup, a barrier between levels); no kernel waits for another workgroup.  Every row's sum is accumulated in
 * double in a fixed order and rounded once: two solves, and two builds, give the same bits.
 * ordering: SPMV_ORDER_NATURAL only (SPMV_ORDER_MULTICOLOR changes which matrix a preconditioner factors, below).
 * -1 (*out stays NULL, the HIP error state stays clean, the handle still works): a missing, zero or non-finite diagonal
 * with SPMV_TRSV_NONUNIT (the message names the first bad row), a bad uplo / diag / ordering, a non-square matrix, a
 * tiles-only handle.
 *   spmv_hip_trsv_solve     x with T x = b; b_host, x_host hold `rows` values (element i = row row0 + i); syncs
 *   spmv_hip_trsv_solve_on  the same on device vectors (b and x must not overlap), asynchronous on `stream` (NULL =
 *                           the library's), no host synchronisation
 *   spmv_hip_trsv_info      info[SPMV_TRSV_INFO_WORDS] = rows, row0, value_bytes, off-diagonal entries, levels, launches,
 *                           rows of the widest level, colours (0), rows of the median level, lanes per short row,
 *                           microseconds of the analysis (download, canonical rows, levels) and of the upload */
typedef struct spmv_trsv spmv_trsv;
enum { SPMV_TRSV_LOWER = 0, SPMV_TRSV_UPPER = 1 };
enum { SPMV_TRSV_NONUNIT = 0, SPMV_TRSV_UNIT = 1 };
enum { SPMV_ORDER_NATURAL = 0, SPMV_ORDER_MULTICOLOR = 1 };
enum { SPMV_TRSV_INFO_WORDS = 12, SPMV_PRECOND_TRI_INFO_WORDS = 14 };
int spmv_hip_csr_trsv_build(const spmv_csr_dev *m, int uplo, int diag, int ordering, spmv_trsv **out);
int spmv_hip_trsv_solve(const spmv_trsv *T, const void *b_host, void *x_host);
int spmv_hip_trsv_solve_on(const spmv_trsv *T, const void *d_b, void *d_x, void *stream);
int spmv_hip_trsv_info(const spmv_trsv *T, int *info);
void spmv_hip_trsv_free(spmv_trsv *T);
/* New values, the symbolic work kept.  m is a handle of the object's dtype, rows and row0 with the pattern the object was
 * built from -- normally the same handle after spmv_hip_csr_update_values.  After the call the object is, byte for byte,
 * the one a fresh build with the same arguments on a fresh upload of m's arrays gives: spmv_hip_precond_factors, every
 * apply and solve, the infos apart from their times, and so every solver step with it.
 *   spmv_hip_precond_refresh  JACOBI, BLOCK_JACOBI: the device build once more into an array of its own, copied over P's
 *                             only when no row or block was refused.  SSOR, ILU0 (either ordering): no host analysis
 *                             and no value crosses to the host but the diagonal -- the first refresh builds, once, from
 *                             the downloaded PATTERN the map from every entry of the canonical (and permuted) diagonal
 *                             block to the handle entries that feed it (a repeated pair: in entry order) and from there
 *                             to the triangles' level order, and keeps the block's pattern on the device; from then on
 *                             a refresh gathers in fp64 (repeats added in entry order), runs the build's own ILU(0)
 *                             launches, checks the pivots and the diagonal, and scatters with one rounding to the dtype.
 *                             FSAI, AMG, CHEBYSHEV: refused -- their pattern, hierarchy or interval is a function of
 *                             the values: build them again.
 *   spmv_hip_trsv_refresh     a triangular solver, lower or upper, unit or not, the same way
 * All or nothing: the numbers are made in scratch arrays and published only behind the checks; a zero pivot, a zero or
 * non-finite diagonal or a singular block is refused in the words of the build's refusal, with its row, and leaves the
 * object applying exactly as before.  The pattern is checked on every call: a 64-bit digest of m's row_ptr and col is
 * taken on the device at the object's first refresh (which, for the kinds with maps, also holds m's pattern to the
 * triangles the object stores) and compared from then on.  -1 also: a NULL argument, a handle of other rows, row0 or
 * dtype, a tiles-only handle.  An object that is never refreshed keeps nothing more than before. */
int spmv_hip_precond_refresh(spmv_precond *P, const spmv_csr_dev *m);
int spmv_hip_trsv_refresh(spmv_trsv *T, const spmv_csr_dev *m);
/* The host analysis behind them (no device needed), on an n x n CSR pattern with local columns; columns outside [0, n)
 * are ignored, rows may be unsorted.
 *   spmv_trsv_colour  greedy first-fit colouring in natural order over the pattern of A + A^T; colour[n], order[n] =
 *                     the rows by (colour, row); returns the number of colours (-1: out of memory or bad arguments)
 *   spmv_trsv_levels  the level schedule of the strict lower / upper triangle: level[n] (from 1), perm[n] = the rows
 *                     level by level, inside a level first the rows with fewer than long_len entries on that side, then
 *                     the others, each in ascending order; level_ptr[levels + 1], level_split[levels] (a level's first
 *                     long row) index perm; plan[3 k] = {1, first, end} for a run of narrow levels (at most chain_rows
 *                     rows and chain_entries entries each), {0, l, l + 1} for a wide one; counts[4] = levels, launches,
 *                     widest level, entries.  The caller allocates level_ptr[n + 1], level_split[n], plan[3 n]. */
int spmv_trsv_colour(int n, const int *row_ptr, const int *col, int *colour, int *order);
int spmv_trsv_levels(int n, const int *row_ptr, const int *col, int uplo, int long_len, int chain_rows,
                     int chain_entries, int *level, int *perm, int *level_ptr, int *level_split, int *plan,
                     long long *counts);
/* Preconditioners made of two triangular solves, of the handle's own diagonal block A = L + D + U (the same
 * spmv_precond type: info (block = 1), apply, apply_on, free, spmv_hip_csr_pcg and spmv_hip_csr_pbicgstab take them):
 *   SPMV_PRECOND_SSOR   M = w / (2 - w) (D/w + L) (D/w)^-1 (D/w + U), 0 < w = omega < 2; no factorisation; w = 1 is
 *                       symmetric Gauss-Seidel.  M is symmetric when A is.
 *   SPMV_PRECOND_ILU0   M = L U, L unit lower, U upper, both with A's pattern, (L U)_ij = a_ij on it (omega unused).
 *                       Factored on the device level by level, one wavefront per row, a row's updates in ascending
 *                       pivot order in fp64, the factors rounded once to the handle's dtype.  For SPD A, U = D L^T.
 * SPMV_ORDER_MULTICOLOR builds them of Q A Q^T, Q ordering the rows by (colour, row) of spmv_trsv_colour; the apply
 * reads r and writes z through Q inside its first and last kernel.  One P serves one stream at a time (the two
 * solves share a vector of P's).  P keeps only the diagonal on the host; spmv_hip_precond_factors reads the rest back.
 * -1 as spmv_hip_csr_precond_build, and for a zero or non-finite ILU(0) pivot (its row in the message).
 *   spmv_hip_precond_tri_info  info[SPMV_PRECOND_TRI_INFO_WORDS] = forward solve: levels, launches, widest, median
 *                              level; backward solve: the same four; colours (0: natural order); entries of L and of
 *                              U (each with its diagonal); microseconds of analysis, factorisation, upload
 *   spmv_hip_precond_factors   L (which = SPMV_FACTOR_L) or U in the handle's row numbering, columns ascending, values
 *                              of the handle's dtype, both with their diagonal (ILU(0): L's is exactly 1; SSOR: the
 *                              triangles of A).  With the multicolour order they are Q^T L Q and Q^T U Q.  First call:
 *                              col = val = NULL fills row_ptr[rows + 1]; second call: all three. */
enum { SPMV_PRECOND_SSOR = 3, SPMV_PRECOND_ILU0 = 4 };
enum { SPMV_FACTOR_L = 0, SPMV_FACTOR_U = 1 };
int spmv_hip_csr_precond_build_tri(const spmv_csr_dev *m, int kind, int ordering, double omega, spmv_precond **out);
int spmv_hip_precond_tri_info(const spmv_precond *P, int *info);
int spmv_hip_precond_factors(const spmv_precond *P, int which, int *row_ptr, int *col, void *val);
/* FSAI, a factorised sparse approximate inverse (Kolotilina and Yeremin) of the handle's own diagonal block (the same
 * spmv_precond type: info (block = 1), apply, apply_on, free, spmv_hip_csr_pcg and spmv_hip_csr_pbicgstab take it): a
 * sparse lower-triangular G with G^T G ~ A^-1, applied as z = G^T (G r), two SpMVs and no triangular solve.
 * The block is made canonical as for the triangular solves (local columns, sorted rows, repeats added in entry order in
 * fp64) and only its lower triangle is read: A~ is the symmetric matrix with that lower triangle (A itself when A is
 * symmetric; for a nonsymmetric A the preconditioner is the FSAI of A~, still a valid right preconditioner).
 * Row i of G has the pattern S_i = {i} and the stored columns j < i of row i; with more than cap - 1 of those the
 * cap - 1 of largest |a_ij| stay, ties to the larger column (cap in [1, 32]; an explicit zero is a stored column).  With
 * S_i ascending, i last, row i of G solves C^T g = e_last, C C^T = A~[S_i, S_i] the Cholesky factorisation (an entry
 * A~[a, b], a >= b, is read from canonical row a and is 0 when the row does not store it): diag(G A~ G^T) = 1 and
 * (G A~)_ij = 0 for j in S_i, j != i.  cap = 1 gives G = diag(a_ii^-1/2).  G^T G is symmetric positive definite
 * whatever A is.  No powers of A enlarge the pattern and G is not filtered afterwards.
 * The rows are built on the device, each by the smallest power of two >= |S_i| (at least 4) of lanes, in fp64 in a
 * fixed order without atomics, and rounded once to the handle's dtype: two builds give the same bytes.  G is an
 * ordinary whole rows x rows CSR handle with whatever plan upload picks, G^T is spmv_hip_csr_transpose of it (the
 * bit-exact transpose of the rounded G).  P owns both and the vector between the products: it may outlive the handle
 * it was built from, and one P serves one stream at a time.  On a row-range handle this is FSAI of the diagonal block:
 * across ranks, block-Jacobi of FSAI.  CSR handles only, one right-hand side.
 * The apply runs the two handles' own launches; r and z hold `rows` values at local row 0 and must not overlap (an r
 * or z that is not 128-byte aligned takes the gather kernels; an aligned r is read as spmv_hip_csr_run_on reads its x,
 * in whole 128-byte lines, so up to the end of the line that holds its last value).  Its rounding is that of the SpMV kernels, twice: the
 * sentence "accumulated in double, rounded once" of the other kinds does not describe this one -- t = G r is rounded to
 * the handle's dtype before G^T multiplies it.  The launches do not look at a solver's stop state: after a stop they
 * rewrite z with the bits it holds.
 * -1 (*out stays NULL, the HIP error state stays clean, the handle still works): a row without a diagonal entry (named),
 * a Cholesky pivot that is not positive or not finite (A~[S_i, S_i] is not positive definite; the first such row is
 * named), an entry of G that is not finite in the handle's dtype, a cap outside [1, 32], a non-square matrix, a
 * tiles-only handle.
 *   spmv_hip_precond_fsai_info  info[SPMV_PRECOND_FSAI_INFO_WORDS] = cap, entries of G, rows that lost entries to the
 *                               cap, the largest |S_i|, the plan of G and of G^T (0 gather kernels, 1 x-window, 2
 *                               x-window with a pattern plan, 3 csr_tile), microseconds of analysis (download,
 *                               canonical rows, patterns), of the device build, and of the two uploads with the
 *                               transpose
 *   spmv_hip_precond_factors    G for SPMV_FACTOR_L, G^T for SPMV_FACTOR_U, as their handles hold them
 *   spmv_fsai_plan              the host pass (no device needed) on an n x n CSR matrix with local columns (columns
 *                               outside [0, n) are ignored; rows may be unsorted and repeat a column, repeats are added
 *                               in entry order): g_ptr[n + 1] and g_col (room for min(n cap, row_ptr[n] + n) entries)
 *                               = the patterns S_i; width_ptr[5] and width_rows[n] = the rows of 4 << k lanes are
 *                               width_rows[width_ptr[k] .. width_ptr[k + 1]), ascending; counts[4] = entries of G,
 *                               rows that lost entries to the cap, the largest |S_i|, the first row that stores no
 *                               diagonal entry (-1: none).  -1: bad arguments or out of memory. */
enum { SPMV_PRECOND_FSAI = 5 };
enum { SPMV_PRECOND_FSAI_INFO_WORDS = 9 };
int spmv_hip_csr_precond_build_fsai(const spmv_csr_dev *m, int cap, spmv_precond **out);
int spmv_hip_precond_fsai_info(const spmv_precond *P, int *info);
int spmv_fsai_plan(int n, const int *row_ptr, const int *col, const double *val, int cap, int *g_ptr, int *g_col,
                   int *width_ptr, int *width_rows, long long *counts);
/* Smoothed-aggregation algebraic multigrid (Vanek, Mandel and Brezina) of the handle's own diagonal block, one V(1,1)
 * cycle per apply (the same spmv_precond type: info (block = 1), apply, apply_on, apply_multi, apply_multi_on, free;
 * spmv_hip_csr_pcg, _pbicgstab, _minres, _pcg_multi and _lobpcg take it).  On a row-range handle this is the AMG of the
 * diagonal block: across ranks, block-Jacobi of AMG.  fp64 and fp32 CSR handles.
 * The setup runs on the host in fp64 on the canonical block (local columns, sorted rows, repeats added in entry order):
 * level l holds A_l with n_l rows and d_i = a_ii, A_0 is the block.
 *   1. every d_i must be present, finite and > 0 (else -1; level 0 names the row, deeper levels the level)
 *   2. rho_l = max_i (sum_j |a_ij|) / d_i, the Gershgorin bound of D^-1 A, in stored order; w_l = 4 / (3 rho_l): the
 *      damped Jacobi sweep x += w D^-1 (b - A x) converges for SPD A without an eigenvalue estimate
 *   3. n_l <= coarse_rows: the DIRECT coarsest level, its dense inverse by Gauss-Jordan with partial pivoting in fp64
 *      (a zero or non-finite pivot: -1 with the level)
 *   4. l + 1 == max_levels: the SMOOTH coarsest level
 *   5. an off-diagonal (i, j) is strong when a_ij != 0 and |a_ij| >= theta sqrt(d_i d_j); the strength graph has an
 *      edge when either direction is strong; neighbours in ascending order
 *   6. aggregation in three passes in row order: (a) a row with a neighbour, itself and all neighbours unaggregated,
 *      starts an aggregate of itself and them; (b) a row still unaggregated joins the aggregate, as it stood after (a),
 *      of its first neighbour that had one; (c) a row still unaggregated with a neighbour starts an aggregate and takes
 *      its unaggregated neighbours along.  Rows without neighbours are in no aggregate: they are only smoothed.
 *   7. na aggregates; na == 0 or 10 na > 9 n_l (a stall): the SMOOTH coarsest level
 *   8. T (n_l x na) has T[i, agg(i)] = 1; P_l = T - diag(w_l / d_i) A_l T on the pattern of A_l T (entries that cancel
 *      stay); R_l = P_l^T; A_{l+1} = R_l (A_l P_l); every sum in fp64 in ascending column order
 * theta in [0, 1), coarse_rows in [1, 256], max_levels in [1, 16].
 * The apply, with b the right-hand side of level l and g = w_l / d (d as the device holds it, g kept in fp64):
 *   not coarsest:  x = g.b;  r = b - A x;  b' = R r;  e = cycle(l + 1, b');  x = x + P e;  x' = x + g.(b - A x)
 *   DIRECT:        x = Ainv b
 *   SMOOTH:        x = g.b;  x' = x + g.(b - A x)
 * Every row's value is accumulated in double in a fixed order and rounded once to the handle's dtype on store; level
 * vectors are of the handle's dtype; no atomics; the second sweep writes a second vector.  Two applies, and two builds,
 * give the same bits.  M is symmetric positive definite for SPD A up to that rounding.
 * On the device level 0 is P's own upload of the canonical block (an ordinary handle: A_0 x runs through its AUTO launch,
 * for k vectors through spmv_hip_csr_spmm_on) plus three fused vector passes; every P_l, R_l, A_l (l > 0) and Ainv is a
 * plain CSR array of P's, rounded once to the handle's dtype, run by one row kernel (amg_kernels.hpp: G lanes per row, G a
 * power of two <= 32 from the operator's mean row).  With chain != 0 everything from the first level l > 0 with at most
 * 256 rows and 4096 entries of A_l down to the coarsest and back is ONE launch of one workgroup (a single-level DIRECT
 * hierarchy is that one launch); chain = 0 launches every pass on its own and gives the same bits.  No kernel waits for
 * another workgroup.  P owns its level vectors for one right-hand side, so one P serves one stream at a time; it may
 * outlive the handle.  r and z must not overlap.  The launches do not look at a solver's stop state: after a stop they
 * rewrite z with the bits it holds.
 * For k right-hand sides the same kernels walk row-major n_l x k arrays, a group keeping 4 columns in registers per
 * walk of the row; column j's sums do not depend on j or k.  The level vectors then live in the caller's d_work:
 *   spmv_hip_precond_work_bytes      *bytes = what spmv_hip_precond_apply_multi_on needs in d_work for k columns: 0 for
 *                                    Jacobi and block-Jacobi, rows x k values (at least 16 bytes) and a 128-byte line
 *                                    for FSAI, the sum of the level vectors for AMG (every vector n_l rounded up to 32 rows
 *                                    plus 32 rows, times k values; the part behind a vector's values should be zero:
 *                                    the x-window kernels read whole 128-byte lines), the three arrays of
 *                                    CHEBYSHEV (below); -1 for SSOR and ILU(0)
 *   spmv_hip_csr_precond_build_amg   -1 (*out stays NULL, the HIP error state stays clean, the handle still works): the
 *                                    refusals above, a parameter out of range, a non-square or tiles-only handle
 *   spmv_hip_precond_amg_info        info[SPMV_PRECOND_AMG_INFO_WORDS] = levels, the first chained level (-1: none),
 *                                    launches per apply, the coarsest kind (SPMV_AMG_DIRECT / _SMOOTH), operator
 *                                    complexity x 1000 (sum of entries of A_l / entries of A_0), microseconds of
 *                                    download with canonical rows, of the host setup, of the uploads, chain, then
 *                                    rows[16] and entries of A_l[16] per level (0 beyond the last)
 *   spmv_hip_precond_amg_level       what the device holds of level `level`: which = SPMV_AMG_A, _P, _R or _INV (the
 *                                    dense inverse of a DIRECT level as n_l rows of n_l entries), values of the handle's
 *                                    dtype; scalars[5] = w_l, rho_l, the kind (SPMV_AMG_NOT_COARSEST, _DIRECT, _SMOOTH),
 *                                    n_l, the aggregates.  row_ptr = NULL: scalars alone; col = val = NULL: row_ptr
 *                                    (n_l + 1 entries; R: aggregates + 1) and scalars; else all.
 *   spmv_amg_plan_build / _levels / _level / _free / _error   the host setup alone (no device needed) on canonical rows
 *                                    (ascending columns in [0, n) without repeats, else -1): the same reader in fp64,
 *                                    with which = SPMV_AMG_T as well; _error is the message of this thread's last -1.
 * The setup on the device (opt-in; the host setup above is the definition and stays the default):
 *   spmv_hip_csr_precond_build_amg_device   the same preconditioner, byte for byte: for every handle, dtype and argument
 *                                    set on which spmv_hip_csr_precond_build_amg succeeds it holds the same row_ptr, col
 *                                    and val of every A_l, P_l and R_l, the same dense inverse, w, rho, kinds, rows,
 *                                    aggregates and g; where that refuses, this refuses with the same message (*out
 *                                    stays NULL, the HIP error state clean, the handle working).  The hierarchy is made in
 *                                    fp64 on the device from the canonical block (an fp32 handle's values widened) and
 *                                    rounded once at the end.  Per level: row statistics (d, rho, the lowest bad
 *                                    diagonal); the strength graph by a filter, a radix sort of both directions of every
 *                                    strong entry and a pass that drops repeats; the aggregation on the host (serial by
 *                                    definition, about 1 % of the host setup); P = T - diag(w / d) A T, R = P^T and
 *                                    A_{l+1} = R (A P) by the cores of spmv_hip_csr_spgemm and spmv_hip_csr_transpose,
 *                                    which are defined as the host setup's sums and order; the dense inverse of a DIRECT
 *                                    level on the host.  block_products goes to all three products of a level: 0 (auto),
 *                                    -1 (global tier only) or a power of two in [64, 4096], as in spmv_hip_csr_spgemm;
 *                                    the other arguments are refused as spmv_hip_csr_precond_build_amg refuses them.
 *                                    Of spmv_hip_precond_amg_info's three times the first is the download, the second the
 *                                    device setup, the third level 0's upload and the workspace.
 *   spmv_hip_precond_amg_setup_info  info[SPMV_PRECOND_AMG_SETUP_INFO_WORDS] = the setup (0 host, 1 device), then
 *                                    microseconds of the device setup's phases over all levels: row statistics, strength
 *                                    graph, aggregation (host), A T with the smoothing of P, transpose, A P, R (A P),
 *                                    coarsest inverse (host), rounding to the dtype.  A host-built P: 0 and zeros. */
enum { SPMV_PRECOND_AMG = 6 };
enum { SPMV_PRECOND_AMG_INFO_WORDS = 41 };
enum { SPMV_PRECOND_AMG_SETUP_INFO_WORDS = 10 };
enum { SPMV_AMG_A = 0, SPMV_AMG_P = 1, SPMV_AMG_R = 2, SPMV_AMG_INV = 3, SPMV_AMG_T = 4 };
enum { SPMV_AMG_NOT_COARSEST = 0, SPMV_AMG_DIRECT = 1, SPMV_AMG_SMOOTH = 2 };
typedef struct spmv_amg_plan spmv_amg_plan;
int spmv_amg_plan_build(int n, const int *row_ptr, const int *col, const double *val, double theta, int coarse_rows,
                        int max_levels, spmv_amg_plan **out);
int spmv_amg_plan_levels(const spmv_amg_plan *plan);
int spmv_amg_plan_level(const spmv_amg_plan *plan, int level, int which, int *row_ptr, int *col, double *val,
                        double *scalars);
void spmv_amg_plan_free(spmv_amg_plan *plan);
const char *spmv_amg_plan_error(void);
int spmv_hip_csr_precond_build_amg(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels, int chain,
                                   spmv_precond **out);
int spmv_hip_csr_precond_build_amg_device(const spmv_csr_dev *m, double theta, int coarse_rows, int max_levels,
                                          int chain, int block_products, spmv_precond **out);
int spmv_hip_precond_amg_info(const spmv_precond *P, int *info);
int spmv_hip_precond_amg_setup_info(const spmv_precond *P, int *info);
int spmv_hip_precond_amg_level(const spmv_precond *P, int level, int which, int *row_ptr, int *col, void *val,
                               double *scalars);
int spmv_hip_precond_work_bytes(const spmv_precond *P, int k, long long *bytes);
/* A Chebyshev polynomial in the Jacobi-scaled matrix (the same spmv_precond type: info (block = 1), apply, apply_on,
 * apply_multi, apply_multi_on, free; spmv_hip_csr_pcg, _pbicgstab, _minres, _pcg_multi and _lobpcg take it): m = degree
 * steps of Jacobi-preconditioned Chebyshev iteration on A z = r from z = 0, A the handle's own diagonal block made
 * canonical as for the triangular, FSAI and AMG builds (local columns, sorted rows, repeats added in entry order in
 * fp64).  With T the handle's dtype, g_i = T(1 / a_ii) and [lmin, lmax] the interval of D^-1 A the polynomial is fitted to:
 *   theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta
 *   rho_0 = 1 / sigma;  a_0 = 0;  b_0 = 1 / theta
 *   for j = 1 .. m-1:  rho_j = 1 / (2 sigma - rho_{j-1});  a_j = rho_j rho_{j-1};  b_j = 2 rho_j / delta
 *   step 0:        d = b_0 g.r;                          z = d
 *   step j >= 1:   q = A z;   d = a_j d + b_j g.(r - q);  z = z + d
 * The coefficients are computed on the host in double, each line one rounded operation in the order written, none
 * fused.  The vector passes compute in double from the stored values and round once to T for every value they store; z
 * takes the rounded d.  1 - t p(t) = T_m((theta - t) / delta) / T_m(sigma), so M^-1 = p(D^-1 A) D^-1 is symmetric for a
 * symmetric A and positive definite whenever the spectrum of D^-1 A lies in (0, lmax]; an lmax that is too small can make
 * it indefinite at even degree, and spmv_hip_csr_pcg then reports SPMV_PCG_BREAKDOWN as for any indefinite M.  Degree 1 is
 * Jacobi times 1 / theta.  For a nonsymmetric A the same formula is used (an interval, no ellipse) and serves
 * spmv_hip_csr_pbicgstab from the right.
 * lmax = 0: the Gershgorin bound max_i sum_j |a_ij| / a_ii of the canonical block in fp64, the sums in stored order (the
 * rho_0 of the AMG setup, computed by the same function): a true upper bound, so M stays positive definite.  lmin = 0:
 * lmax / ratio.  Explicit values are taken as given.
 * On the device A is P's own upload of the canonical block rounded to T (an ordinary whole rows x rows handle with
 * whatever plan upload picks: A z runs through its AUTO launch, for k vectors through spmv_hip_csr_spmm_on), so P may
 * outlive the handle it was built from, and on a row-range handle it is the polynomial of the diagonal block.  P owns
 * z, d and q, each with the 128-byte tail the x-window kernels read: one P serves one stream at a time.  No product
 * reads a caller's buffer: the iterate lives in P's z and the last pass writes the caller's z (with degree 1 it is the
 * only pass).  An apply is m - 1 products and m element-wise launches (16-byte pieces when r and z are 16-byte aligned,
 * single values otherwise: the same bits); no LDS, no atomics, no reduction: two applies give the same bits.  r and z
 * must not overlap.  The launches do not look at a solver's stop state: after a stop they rewrite z with the bits it
 * holds.  For k right-hand sides the three vectors live in the caller's d_work (spmv_hip_precond_work_bytes: three
 * arrays of rows x k values rounded up to whole 128-byte lines plus one line each); column j's values do not depend on
 * j or k, and k = 1 runs the launches of the one-wide apply.
 *   spmv_chebyshev_coefficients            a[degree], b[degree] of the loop above (no device needed); -1: a NULL array,
 *                                          degree outside [1, SPMV_CHEBYSHEV_MAX_DEGREE], lmin or lmax not finite,
 *                                          lmin <= 0 or lmin >= lmax
 *   spmv_hip_csr_precond_build_chebyshev   -1 (*out stays NULL, the HIP error state stays clean, the handle still works):
 *                                          a row without a diagonal entry, or whose diagonal is not positive or not finite
 *                                          (the first such row, local and global, is named), a non-square or tiles-only
 *                                          handle; degree outside [1, 32], ratio <= 1 or not finite, lmax < 0 or not
 *                                          finite, lmin < 0 or not finite, lmin >= lmax after the defaults (the value and
 *                                          the allowed range are named)
 *   spmv_hip_precond_cheb_info             info[SPMV_PRECOND_CHEB_INFO_WORDS] = degree, lmin, lmax, the Gershgorin bound
 *                                          (also when lmax was given), products per apply (degree - 1), the plan of P's
 *                                          upload (0 gather kernels, 1 x-window, 2 x-window with a pattern plan, 3
 *                                          csr_tile), microseconds of download with canonical rows and the bound, and of
 *                                          the upload with the vectors
 * Not here: eigenvalue estimates (power iteration, Lanczos), Chebyshev smoothing inside the AMG cycle, a product fused
 * with the recurrence, the solvers' dots fused into the last pass, HLL handles, an ellipse for nonsymmetric spectra, a
 * halo exchange. */
enum { SPMV_PRECOND_CHEBYSHEV = 7 };
enum { SPMV_PRECOND_CHEB_INFO_WORDS = 8, SPMV_CHEBYSHEV_MAX_DEGREE = 32 };
int spmv_chebyshev_coefficients(int degree, double lmin, double lmax, double *a, double *b);
int spmv_hip_csr_precond_build_chebyshev(const spmv_csr_dev *m, int degree, double lmin, double lmax, double ratio,
                                         spmv_precond **out);
int spmv_hip_precond_cheb_info(const spmv_precond *P, double *info);
/* Preconditioned CG for a symmetric positive definite A and M, x0 = 0 (P = NULL: M = I, z is r itself):
 *   r = b, z = M^-1 r, p = z, rz = r.z, rr0 = r.r
 *   each step: q = A p, alpha = rz / p.q, x += alpha p, r -= alpha q, z = M^-1 r, rz' = r.z, rr = r.r,
 *              stop (CONVERGED) if rr <= tol^2 rr0, beta = rz' / rz, p = z + beta p
 * The product, the communicator, the bounds and the all-gatherv of p are those of spmv_hip_csr_cg (no halo variant).
 * Jacobi is fused into the x / r update with both dots; a block-Jacobi apply is a pass of its own that makes the dots;
 * an SSOR or ILU(0) apply is its two solves, an FSAI apply its two SpMVs, then one pass for the two dots.
 * P = NULL, or Jacobi on a matrix whose diagonal is exactly 1, with tol = 0 and no breakdown gives spmv_hip_csr_cg's
 * x and rr_hist bit for bit.
 * Breakdown: p.q <= 0, rz' <= 0 while rr > 0, or any non-finite scalar (A or M not SPD); x stays at the last full
 * iterate, no NaN is written into it.  rr0 = 0: converged at step 0 with x = 0.  After a stop x no longer changes and
 * both histories repeat their last value.  tol = 0: exactly `iters` steps, no host synchronisation; tol > 0: the host
 * reads one device word every 16 steps.
 * Out (all optional): x_host M_total values; rr_hist, rz_hist [iters + 1] r.r and r.z before step 1 and after every
 * step; info[2] = {steps, status (SPMV_PCG_*)}; *ms_total device time of the loop.
 * -1: as spmv_hip_csr_bicgstab, and a P whose rows, row0 or dtype differ from the handle's. */
enum { SPMV_PCG_RAN_ALL = 0, SPMV_PCG_CONVERGED = 1, SPMV_PCG_BREAKDOWN = 2 };
int spmv_hip_csr_pcg(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, const int *bounds,
                     const void *b_host, void *x_host, double *rr_hist, double *rz_hist, int *info, float *ms_total);
/* k independent preconditioned CG recurrences for a symmetric positive definite A and M, x0 = 0, sharing one SpMM per
 * step: the loop of spmv_hip_csr_pcg with one alpha, one beta, one stop state and one status per column (not block CG),
 * in the layout of spmv_hip_csr_cg_multi.  B, X and every loop vector are row-major n x k; the product is
 * spmv_hip_csr_spmm_on on library-owned P (N x k) and Q (M_total x k).  The communicator, the bounds scaled by k, the
 * all-gatherv of P and the dot products added in rank order are those of spmv_hip_csr_cg_multi.
 * P: NULL, JACOBI, BLOCK_JACOBI, FSAI, AMG or CHEBYSHEV.  Jacobi is fused into the x / r update with both dots; a block-Jacobi apply is
 * a pass of its own that makes the dots; an FSAI apply is Z = G^T (G R), two SpMMs through P's handles, an AMG apply its
 * V-cycle on k columns, then one pass for the dots.  SSOR and ILU0 are refused: their triangular solves take one right-hand side.
 * Column j's sums add in an order that does not depend on j: permuting the columns of B permutes X, both histories,
 * steps and status bit for bit, and two calls give the same bits.  k = 1 gives spmv_hip_csr_pcg's bits (variant
 * SPMV_CSR_AUTO); P = NULL gives spmv_hip_csr_cg_multi's X and history while no column breaks down.
 * Per column, the rules of spmv_hip_csr_pcg: rr0 = 0 converges at step 0 with x = 0; before step t's update p.q <= 0 or a
 * non-finite scalar is a breakdown with steps = t - 1; after it a non-finite rr or rz is a breakdown, then rr <= tol^2 rr0
 * converges, then rz <= 0 is a breakdown.  A stopped column keeps its x, r, z and p, its histories repeat their last
 * value, it still rides in the SpMM and it never receives a NaN in X, whatever the other columns hold.
 * tol = 0: exactly `iters` steps, no host synchronisation; tol > 0: the host reads one device word every 16 steps and
 * ends the loop once no column is active.
 * Out (all optional): X_host M_total x k; rr_hist, rz_hist (iters + 1) x k, r.r and r.z per column before step 1 and
 * after every step; steps[k]; status[k] (SPMV_PCG_*); *ms_total device time of the loop.
 * -1 (the HIP error state stays clean, the handle still works): k < 1 or k > 64, a non-square matrix, a tiles-only
 * handle, n*k beyond int range, iters < 0, tol < 0 or not finite, a communicator without bounds, a row-range handle
 * without a communicator, a P whose rows, row0 or dtype differ from the handle's, a P of kind SSOR or ILU0.
 *   spmv_hip_precond_apply_multi_on  Z = M^-1 R for row-major rows x k device arrays (element (i, j) at i k + j, row i =
 *                                    row row0 + i), asynchronous on `stream` (NULL = the library's).  Jacobi and
 *                                    block-Jacobi ignore d_work; a row's sum is pc_apply's: in double, the block's
 *                                    columns ascending, rounded once.  FSAI needs d_work, rows x k values plus one
 *                                    128-byte line: work = G R, then Z = G^T work, by spmv_hip_csr_spmm_on on P's two
 *                                    handles (R, with the same tail, is read as that call reads its X); P's own vector
 *                                    is not touched.  The Jacobi and block-Jacobi kernels move 16-byte pieces of a
 *                                    row when k values are whole pieces AND d_R and d_Z are 16-byte aligned; else they
 *                                    move single elements (the same bits, more instructions).  -1: k outside [1, 64],
 *                                    arrays not aligned to the element size, FSAI, AMG or CHEBYSHEV without d_work, SSOR or ILU0.
 *   spmv_hip_precond_apply_multi     the same on host arrays of rows x k values: allocates, copies, syncs */
int spmv_hip_csr_pcg_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol, const int *bounds,
                           const void *B_host, void *X_host, double *rr_hist, double *rz_hist, int *steps, int *status,
                           float *ms_total);
int spmv_hip_precond_apply_multi_on(const spmv_precond *P, int k, const void *d_R, void *d_Z, void *d_work,
                                    void *stream);
int spmv_hip_precond_apply_multi(const spmv_precond *P, int k, const void *R_host, void *Z_host);
/* Right-preconditioned BiCGSTAB: the loop of spmv_hip_csr_bicgstab on A M^-1 with x = M^-1 y, so r stays the true
 * residual and tol, the half step, the breakdown rules, rr_hist and info mean what they mean there:
 *   p^ = M^-1 p, v = A p^, ..., s^ = M^-1 s, t = A s^, x += alpha p^ + omega s^ (a half step: x += alpha p^)
 * With a communicator p^ and s^ (the products' inputs) are all-gathered.  Jacobi is fused into the s and p updates;
 * block-Jacobi, SSOR, ILU(0) and FSAI are applied after them.
 * P = NULL gives spmv_hip_csr_bicgstab's bits.  -1: as spmv_hip_csr_bicgstab, and a P that does not fit the handle. */
int spmv_hip_csr_pbicgstab(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol,
                           const int *bounds, const void *b_host, void *x_host, double *rr_hist, int *info,
                           float *ms_total);
/* k independent right-preconditioned BiCGSTAB recurrences for a square, possibly nonsymmetric A, x0 = 0, r^_j = b_j,
 * sharing the two SpMMs of a step and the k-wide apply: the loop of spmv_hip_csr_pbicgstab with one alpha, omega, beta,
 * rho, stop state, status, half-step flag and step count per column (not block BiCGSTAB: no k x k coefficient
 * matrices), in the layout of spmv_hip_csr_cg_multi.  B, X and every loop vector are row-major n x k:
 *   X = 0;  R = R^ = P = B;  P^ = M^-1 P;  rho_j = rr0_j = r_j.r_j
 *   each step:  V = A P^ (one SpMM);  alpha_j = rho_j / r^_j.v_j;  s_j = r_j - alpha_j v_j;  S^ = M^-1 S
 *               (s_j.s_j <= tol^2 rr0_j: x_j += alpha_j p^_j, r_j = s_j, column j stops at the half step)
 *               T = A S^ (one SpMM);  omega_j = t_j.s_j / t_j.t_j;  x_j += alpha_j p^_j + omega_j s^_j
 *               r_j = s_j - omega_j t_j;  rho'_j = r^_j.r_j;  rr_j = r_j.r_j
 *               beta_j = (rho'_j / rho_j) (alpha_j / omega_j);  rho_j = rho'_j
 *               p_j = r_j + beta_j (p_j - omega_j v_j);  P^ = M^-1 P
 * The products are spmv_hip_csr_spmm_on on library-owned P^ and S^ (N x k); there is no `variant`: the SpMM has none
 * and k = 1 is the handle's AUTO launch.  With a communicator P^ and S^ are all-gathered with the row bounds scaled by
 * k (two exchanges per step) and every dot product is all-gathered and added in rank order, as in
 * spmv_hip_csr_cg_multi; there is no halo exchange variant.
 * P: NULL (P^ is P and S^ is S), JACOBI (fused into the s and p updates), BLOCK_JACOBI, FSAI, AMG or CHEBYSHEV (the
 * k-wide apply of spmv_hip_precond_apply_multi_on after them).  SSOR and ILU0 are refused: their triangular solves take
 * one right-hand side.
 * Column j's sums add in an order that does not depend on j: permuting the columns of B permutes X, the history, steps,
 * status and half_step bit for bit, and two calls give the same bits.  k = 1 agrees with spmv_hip_csr_pbicgstab to
 * rounding, not bit for bit: that solver sums 16-byte pieces of rows, this one row by row.
 * Per column, the rules of spmv_hip_csr_bicgstab: b_j = 0 converges at step 0 with x_j = 0; s_j.s_j <= tol^2 rr0_j is a
 * converged half step (the history holds s.s, half_step[j] = 1); r_j.r_j <= tol^2 rr0_j converges; r^.v = 0, r^.r' = 0
 * or a non-finite value is BREAKDOWN_RHO; t.s = 0, t.t = 0 or a non-finite value is BREAKDOWN_OMEGA.  A breakdown
 * before the update leaves x_j at the last full iterate and does not count the step.  A stopped column keeps its x, r,
 * s and p, its history repeats its last value, it still rides in the SpMMs and the applies, and nothing it holds, a NaN
 * included, reaches another column.
 * tol = 0: exactly `iters` steps, no host synchronisation; tol > 0: the host reads one device word every 16 steps and
 * ends the loop once no column is active.
 * B_host: M_total x k row-major, values of the handle's dtype (a rank reads its own rows).
 * Out (all optional but ms_total): X_host M_total x k; rr_hist (iters + 1) x k, r.r per column before step 1 and after
 * every step; steps[k]; status[k] (SPMV_BICG_*); half_step[k]; *ms_total device time of the loop.
 * -1 (the HIP error state stays clean, the handle still works): k < 1 or k > 64, a non-square matrix, a tiles-only
 * handle, n*k beyond int range, iters < 0, tol < 0 or not finite, a communicator without bounds, a row-range handle
 * without a communicator, a P whose rows, row0 or dtype differ from the handle's, a P of kind SSOR or ILU0. */
int spmv_hip_csr_bicgstab_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol, const int *bounds,
                                const void *B_host, void *X_host, double *rr_hist, int *steps, int *status,
                                int *half_step, float *ms_total);
/* MINRES (Paige and Saunders 1975) for (A - shift I) x = b with a symmetric, possibly indefinite A and an optional
 * symmetric positive definite preconditioner M (P = NULL: y is r2 itself), x0 = 0.  One SpMV per step through the
 * handle's launch for `variant` on library-owned v, short recurrences, fixed-order device reductions in double, fp64
 * scalars that stay on the device.  The shift goes to A alone; M is used as built.
 *   r1 = r2 = b;  y = M^-1 r2;  bb0 = r2.y;  beta = sqrt(bb0);  phibar = beta
 *   oldb = dbar = epsln = 0;  cs = -1;  sn = 0;  w = w2 = 0;  hist[0] = bb0
 *   step k:  v = y / beta
 *            t = A v - shift v;  if k >= 2: t -= (beta / oldb) r1
 *            alfa = v.t;  t -= (alfa / beta) r2
 *            r1 = r2;  r2 = t;  y = M^-1 r2;  oldb = beta;  bb = r2.y;  beta = sqrt(bb)
 *            oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta
 *            gamma = sqrt(gbar^2 + beta^2);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar
 *            w1 = w2;  w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  x += phi w
 *            hist[k] = phibar^2;  converged when phibar^2 <= tol^2 bb0
 * (cs, sn, dbar, phibar on the right-hand sides of one line are the values before the step.)  hist[k] is the
 * recurrence's r.r of (A - shift I) x_k = b; with M it is r.M^-1 r.  It never grows.
 * Converged: bb0 == 0 at step 0 with x = 0; else the first step with phibar^2 <= tol^2 bb0 (tol = 0: only at exactly
 *   0), which still does its x += phi w.
 * Breakdown (x stays at the last full iterate, no NaN is written into it; the step is not counted): at the start bb0
 *   < 0 or not finite (steps = 0); in step k alfa or alfa / beta not finite; bb < 0 (M is not positive definite);
 *   gamma == 0; or bb, delta, epsln, dbar, gamma, phi, phibar, the new beta / oldb or phibar^2 not finite.
 * After a stop x no longer changes and the history repeats its last value.
 * tol = 0: exactly `iters` steps are launched, no host synchronisation inside the loop.
 * tol > 0: the host reads one device word every 16 steps and ends the loop once the solve has stopped.
 * With a communicator every rank keeps its rows; the next v is all-gathered with `bounds` (one exchange per step), the
 * partial sums are all-gathered and added in rank order: every rank holds the same bits and stops at the same step.
 * There is no halo exchange variant.  With P the apply follows the Lanczos update as launches of its own (a pass for
 * Jacobi and block-Jacobi, two triangular solves for SSOR and ILU(0), two SpMVs for FSAI), then one pass for r2.y.
 * b_host: M_total values of the handle's dtype (a rank reads its own rows).  Out (all optional): x_host M_total
 * values; rr_hist [iters + 1]; info[2] = {steps, status (SPMV_MINRES_*)}; *ms_total device time of the loop.
 * -1: NULL m or b_host, a non-square or tiles-only handle, iters < 0, tol < 0 or not finite, shift not finite, a
 * communicator without bounds, a row-range handle without a communicator, more ranks than the library supports, a P
 * whose rows, row0 or dtype differ from the handle's. */
enum { SPMV_MINRES_RAN_ALL = 0, SPMV_MINRES_CONVERGED = 1, SPMV_MINRES_BREAKDOWN = 2 };
int spmv_hip_csr_minres(spmv_csr_dev *m, const spmv_precond *P, int variant, int iters, double tol, double shift,
                        const int *bounds, const void *b_host, void *x_host, double *rr_hist, int *info,
                        float *ms_total);
/* k independent MINRES recurrences for (A - shift_j I) x_j = b_j with a symmetric, possibly indefinite A and an
 * optional symmetric positive definite M, x0 = 0, sharing the one SpMM of a step and the k-wide apply: the loop of
 * spmv_hip_csr_minres with one shift, one set of Lanczos scalars, one Givens rotation, one phibar, stop state, status
 * and step count per column (not block MINRES: no k x k coefficient matrices), in the layout of spmv_hip_csr_cg_multi.
 * B, X and every loop vector are row-major n x k:
 *   R1 = R2 = B;  Y = M^-1 R2;  bb0_j = r2_j.y_j;  beta_j = sqrt(bb0_j);  phibar_j = beta_j
 *   oldb_j = dbar_j = epsln_j = 0;  cs_j = -1;  sn_j = 0;  W = W2 = 0;  hist[0][j] = bb0_j
 *   step t:  v_j = y_j / beta_j;  A_V = A V (one SpMM)
 *            t_j = a_j - shift_j v_j;  if t >= 2: t_j -= (beta_j / oldb_j) r1_j
 *            alfa_j = v_j.t_j;  t_j -= (alfa_j / beta_j) r2_j
 *            r1_j = r2_j;  r2_j = t_j;  Y = M^-1 R2;  oldb_j = beta_j;  bb_j = r2_j.y_j;  beta_j = sqrt(bb_j)
 *            oldeps_j = epsln_j;  delta_j = cs_j dbar_j + sn_j alfa_j;  gbar_j = sn_j dbar_j - cs_j alfa_j
 *            epsln_j = sn_j beta_j;  dbar_j = -cs_j beta_j;  gamma_j = sqrt(gbar_j^2 + beta_j^2)
 *            cs_j = gbar_j / gamma_j;  sn_j = beta_j / gamma_j;  phi_j = cs_j phibar_j;  phibar_j = sn_j phibar_j
 *            w1_j = w2_j;  w2_j = w_j;  w_j = (v_j - oldeps_j w1_j - delta_j w2_j) / gamma_j;  x_j += phi_j w_j
 *            hist[t][j] = phibar_j^2;  column j has converged when phibar_j^2 <= tol^2 bb0_j
 * (cs, sn, dbar, phibar on the right-hand sides of one line are the values before the step.)  The product is
 * spmv_hip_csr_spmm_on on library-owned V (N x k, with the 128-byte line tail); there is no `variant`: the SpMM has none
 * and k = 1 is the handle's AUTO launch.  With a communicator the next V is all-gathered with the row bounds scaled by
 * k (one exchange per step) and every dot product is all-gathered and added in rank order, as in
 * spmv_hip_csr_cg_multi; there is no halo exchange variant.
 * shift: k values, or NULL for all 0.  The shifts go to A alone; M is used as built.
 * P: NULL (y is r2 and t.t is bb), JACOBI (y = D^-1 t and t.y fused into the second Lanczos pass), BLOCK_JACOBI, FSAI,
 * AMG or CHEBYSHEV (the k-wide apply of spmv_hip_precond_apply_multi_on after it, then one pass for r2.y).  SSOR and
 * ILU0 are refused: their triangular solves take one right-hand side.
 * Column j's sums add in an order that does not depend on j: permuting the columns of B together with the shifts
 * permutes X, the history, steps and status bit for bit, and two calls give the same bits.  k = 1 agrees with
 * spmv_hip_csr_minres to rounding, not bit for bit: that solver sums 16-byte pieces of rows, this one row by row.
 * Per column, the rules of spmv_hip_csr_minres: b_j = 0 converges at step 0 with x_j = 0; the step that converges
 * still does its x_j += phi_j w_j (and forms no v_j: beta_j may be 0); a breakdown (bb0_j < 0 or not finite at the
 * start; alfa_j or alfa_j / beta_j not finite; bb_j < 0, which is how an M that is not positive definite is refused;
 * gamma_j = 0; any scalar of the rotation not finite) leaves x_j at the last full iterate and does not count the step;
 * no NaN is written into X.  A stopped column keeps its x, r1, r2, w and v, its history repeats its last value, it
 * still rides in the SpMMs and the applies, and nothing it holds, a NaN or Inf included, reaches another column.
 * tol = 0: exactly `iters` steps, no host synchronisation; tol > 0: the host reads one device word every 16 steps and
 * ends the loop once no column is active.
 * B_host: M_total x k row-major, values of the handle's dtype (a rank reads its own rows).
 * Out (all optional): X_host M_total x k; rr_hist (iters + 1) x k, the recurrence's r.r (with M: r.M^-1 r) per column
 * before step 1 and after every step; steps[k]; status[k] (SPMV_MINRES_*); *ms_total device time of the loop.
 * -1 (the HIP error state stays clean, the handle still works): k < 1 or k > 64, a non-square matrix, a tiles-only
 * handle, n*k beyond int range, iters < 0, tol < 0 or not finite, a shift_j that is not finite, a communicator without
 * bounds, a row-range handle without a communicator, a P whose rows, row0 or dtype differ from the handle's, a P of
 * kind SSOR or ILU0. */
int spmv_hip_csr_minres_multi(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol, const double *shift,
                              const int *bounds, const void *B_host, void *X_host, double *rr_hist, int *steps,
                              int *status, float *ms_total);
/* LOBPCG (Knyazev 2001) for the k smallest (largest = 0) or largest eigenpairs of a symmetric A held by an fp64 CSR
 * handle, with an optional symmetric positive definite preconditioner (Jacobi, block-Jacobi, FSAI, AMG or Chebyshev; smallest
 * only).
 * Six row-major n x k arrays X, W, P, AX, AW, AP (element (i, j) at i k + j, the SpMM's layout).  Per step one SpMM
 * (spmv_hip_csr_spmm_on), one k-wide apply (spmv_hip_precond_apply_multi_on), a Gram pass and an update pass over the
 * basis S = [X | W | P], AS = [AX | AW | AP] (lobpcg_kernels.hpp), and a Rayleigh-Ritz step on the host.
 *   anorm = ||A||_inf (row sums of |a| in entry order, then the maximum)
 *   step 0:  X = X0;  AX = A X;  G_B = X^T X, G_A = X^T AX;  (theta, C) = rr(G_B, G_A);  X = X C;  AX = AX C
 *   step t = 0, 1, ...:
 *            W = AX - X diag(theta);  res_hist[t, j] = ||w_j||_2;  theta_hist[t, j] = theta_j
 *            CONVERGED when tol > 0 and every ||w_j|| <= tol anorm;  RAN_ALL when t == iters
 *            W = M^-1 W (with P);  AW = A W
 *            G_B = S^T S, G_A = S^T AS  (nb = 2 blocks at t = 0, where there is no P yet, 3 afterwards)
 *            (theta, C, Cp) = rr(G_B, G_A);  X = S C;  P = S Cp;  AX = AS C;  AP = AS Cp
 *   after the loop:  AW = A X;  resid[j] = ||A x_j - theta_j x_j||_2;  w = theta
 * rr is spmv_lobpcg_rr below.  There is no explicit projection of W on X and no locking: a converged column keeps
 * riding.  The host reads the Gram matrices in every step: there is no sync-free mode, and tol = 0 means exactly
 * `iters` steps.
 * BREAKDOWN: at step 0 when a Gram entry is not finite or X0 has fewer than k independent columns (w and X are then
 * zeros, steps = 0); in step t when a residual norm or a Gram entry is not finite or fewer than k basis directions
 * are kept: X stays at the last full iterate.  After a stop both histories repeat their last row.
 * Sums: a Gram entry adds its rows 4 at a time (one fp64 MFMA per 16 x 16 tile), a wave its row groups in grid-stride
 * order, the waves of a workgroup in wave order, the workgroups in workgroup order; the residual norms as
 * spmv_hip_csr_cg_multi's dots.  No atomics: two calls give the same bits.
 * X0_host: n x k.  Out (all optional): w[k]; X_host n x k; theta_hist, res_hist (iters + 1) x k; resid[k]; *anorm;
 * info[4] = {steps, status (SPMV_LOBPCG_*), restarts (steps that dropped P), the smallest basis size kept in any
 * step}; *ms device time of the whole solve; *host_ms wall time inside spmv_lobpcg_rr.
 * -1: NULL m or X0_host, an fp32 handle, a non-square, row-range or tiles-only handle, an active communicator, k
 * outside [1, 16], n < 4 k, iters < 0, tol < 0 or not finite, a P of kind SSOR or ILU0 (no k-wide apply), a P whose
 * rows, row0 or dtype differ from the handle's, any P together with largest.
 *   spmv_lobpcg_rr          host only (csrc/host/lobpcg_rr.c).  GB = S^T S, GA = S^T AS, both m x m row-major, m = nb k,
 *                           nb in [1, 3], k in [1, 16].  Both are symmetrised; D = diag(GB)^-1/2 (0 where the diagonal
 *                           is <= 1e-290); D GB D = V L V^T; the directions with L_i > drop max L are kept.  When some
 *                           were dropped and nb == 3 the same is done on the leading 2k x 2k blocks (*restarted = 1, the
 *                           P rows of C are 0).  T = D V_keep L_keep^-1/2; T^T GA T = Z diag(ritz) Z^T; theta = the k
 *                           smallest ascending (largest: the k largest descending); C = T Z_k (m x k row-major);
 *                           Cp = C with its first k rows 0, each column scaled to Cp_j^T GB Cp_j = 1 (a zero column
 *                           stays 0).  *kept = directions kept.  The eigenproblems are solved by Householder
 *                           tridiagonalisation and implicit QL.  Returns 0; SPMV_LOBPCG_RR_BREAKDOWN when an entry is
 *                           not finite or kept < k (theta, C, Cp are then not to be used); -1 for bad arguments.
 *   spmv_hip_lobpcg_gram    the Gram pass alone on device arrays: d_S[nb], d_AS[nb] row-major n x k fp64 (entries from nb
 *                           on are not read and may be NULL) -> GB_host, GA_host (m x m).  Synchronous.
 *   spmv_hip_lobpcg_update  the update pass alone: X = S C, P = S Cp, AX = AS C, AP = AS Cp with C_host, Cp_host m x k;
 *                           the outputs may be the S / AS blocks themselves (a row is read completely before it is
 *                           written).  Synchronous.  Both: -1 for n < 0, k outside [1, 16], nb outside [1, 3], n k
 *                           beyond int range, a NULL or misaligned array. */
enum { SPMV_LOBPCG_RAN_ALL = 0, SPMV_LOBPCG_CONVERGED = 1, SPMV_LOBPCG_BREAKDOWN = 2 };
enum { SPMV_LOBPCG_RR_BREAKDOWN = 1 };
int spmv_hip_csr_lobpcg(spmv_csr_dev *m, const spmv_precond *P, int k, int iters, double tol, int largest,
                        const double *X0_host, double *w, double *X_host, double *theta_hist, double *res_hist,
                        double *resid, double *anorm, int *info, float *ms, float *host_ms);
int spmv_lobpcg_rr(int nb, int k, const double *GB, const double *GA, int largest, double drop, double *theta,
                   double *C, double *Cp, int *kept, int *restarted);
int spmv_hip_lobpcg_gram(long long n, int k, int nb, const void *const *d_S, const void *const *d_AS,
                         double *GB_host, double *GA_host);
int spmv_hip_lobpcg_update(long long n, int k, int nb, const void *const *d_S, const void *const *d_AS,
                           const double *C_host, const double *Cp_host, void *d_X, void *d_P, void *d_AX, void *d_AP);
/* Restarted GMRES(m) (Saad and Schultz 1986) for a square, possibly nonsymmetric A, right-preconditioned, x0 = 0.  It
 * minimises the residual over the Krylov space of a cycle, so the residual estimate never grows inside a cycle, and it
 * cannot break down on a nonsingular matrix.  One SpMV per step through the handle's launch for `variant`, one apply of
 * P (any kind; NULL: none), classical Gram-Schmidt done twice (CGS2), always: no modified Gram-Schmidt, no switch.
 *   x = 0;  rr0 = b.b;  hist[0] = rr0;  t = 0
 *   rr0 == 0: CONVERGED at step 0.  rr0 not finite: BREAKDOWN at step 0.  (x = 0 either way, no cycle starts)
 *   cycle:
 *     r = b - A x  (the first cycle: r = b, no product);  beta = sqrt(r.r)
 *     beta not finite: BREAKDOWN.  beta == 0: CONVERGED.
 *     v_0 = r / beta;  g = (beta, 0, ..., 0)
 *     for j = 0 .. restart - 1 while t < iters:
 *        z = M^-1 v_j  (P = NULL: z is v_j itself, no copy);  w = A z
 *        h  = V_j^T w;  w = w - V_j h            (V_j = [v_0 .. v_j])
 *        h' = V_j^T w;  w = w - V_j h';  ww = w.w  (in the same pass);  h = h + h'
 *        eta = sqrt(ww)
 *        the rotations 0 .. j - 1 applied to the column (h_0 .. h_j, eta):
 *           (h_i, h_{i+1}) = (c_i h_i + s_i h_{i+1}, -s_i h_i + c_i h_{i+1});  d = hypot(h_j, eta)
 *        d == 0 or anything not finite: BREAKDOWN, the step is not counted
 *        c_j = h_j / d;  s_j = eta / d;  h_j = d;  g_{j+1} = -s_j g_j;  g_j = c_j g_j;  t = t + 1;  hist[t] = g_{j+1}^2
 *        hist[t] <= tol^2 rr0: CONVERGED  (tol = 0: only at exactly 0)
 *        v_{j+1} = w / eta  (eta == 0 gives g_{j+1} == 0, which has converged: no division by zero)
 *     the close of the cycle with its J counted columns (J = 0: nothing):
 *        R y = g by back substitution in double;  u = V_{J-1} y;  x = x + M^-1 u  (P = NULL: x = x + u)
 *     stop on CONVERGED, BREAKDOWN or t == iters (RAN_ALL); else the next cycle
 * Vectors have the handle's dtype (fp64 or fp32); every sum and scalar is fp64.  The Hessenberg column, the rotations,
 * g and the stop state live on the device.  An update w - V h adds its terms in index order in double and rounds each
 * value once; a dot product adds in the fixed order of the other solvers, which depends on n alone and not on
 * restart or on the column: two calls give the same bits, and so do two values of restart that both cover iters.
 * hist[t] is the recurrence's ||b - A x_t||^2 (the true residual's also with P: the preconditioner is on the right).
 * After a stop the history repeats its last value.  x only ever receives the update of fully counted columns: a
 * breakdown leaves it at the iterate of the last counted step and no NaN is written into it.
 * The host reads the stop state once per cycle, after the cycle's last step; nothing synchronises inside a cycle, and a
 * stopped solve's remaining steps of that cycle return at once.  tol = 0 reads as often.
 * The basis (restart + 1 vectors, or iters + 1 when that is fewer) is allocated per call.
 * b_host: M_total values of the handle's dtype.  Out (all optional): x_host M_total values; rr_hist [iters + 1];
 * info[3] = {steps counted, status (SPMV_GMRES_*), cycles started}; *ms_total device time of the solve, its reads
 * included.
 * -1 (the HIP error state stays clean, the handle still works): NULL m or b_host, restart outside [1, 64], iters < 0,
 * tol < 0 or not finite, a non-square, row-range or tiles-only handle, an active communicator, a P whose rows, row0
 * or dtype differ from the handle's, a failed allocation.
 *   spmv_hip_gmres_dots    the dot-product pass alone on device arrays: basis vector i at d_V + i ld elements, n values
 *                          each (the ld - n elements behind them are not read) -> h_out_host[i] = v_i.w.  Synchronous.
 *   spmv_hip_gmres_update  the update pass alone: w = w - sum_i h_host[i] v_i in place; *ww_out_host (optional) = w.w of
 *                          what was stored.  Synchronous.  Both: -1 for a NULL array, value_bytes not 4 or 8, n < 0,
 *                          nvec outside [1, 64], ld < n, ld * value_bytes not a multiple of 16, an array not aligned
 *                          to 16 bytes, an active communicator. */
enum { SPMV_GMRES_RAN_ALL = 0, SPMV_GMRES_CONVERGED = 1, SPMV_GMRES_BREAKDOWN = 2 };
int spmv_hip_csr_gmres(spmv_csr_dev *m, const spmv_precond *P, int variant, int restart, int iters, double tol,
                       const void *b_host, void *x_host, double *rr_hist, int *info, float *ms_total);
int spmv_hip_gmres_dots(const void *d_V, long long ld, int nvec, const void *d_w, long long n, int value_bytes,
                        double *h_out_host);
int spmv_hip_gmres_update(const void *d_V, long long ld, int nvec, const double *h_host, void *d_w, long long n,
                          int value_bytes, double *ww_out_host);
int spmv_hip_csr_split_interior(spmv_csr_dev *m, long long *counts);
/* N4 overlap below block granularity (round 3).  On a KKT-coupled cut every block also lists lines of the coupling block,
 * which another rank owns: no interior BLOCKS -- but 13 of a row's 28 entries have their column in the rank's own range.
 *   spmv_hip_csr_split_columns   splits the handle's entries by column into two sub-handles over the same rows: [col_lo,
 *                                col_hi) = the rank's own range of x; counts[2] (optional): entries inside / outside
 *                                (spmv_hip_comm_halo_setup calls it with the rank's bounds; "halo_split" 0: not)
 *   spmv_hip_csr_run_split       part 0: y = A_own x (reads nothing of x outside the range: it can run while the halo
 *                                travels); part 1: y += A_halo x.  0 then 1 = the handle's product up to the order in
 *                                which a row's two partial sums are added (a fixed order: reproducible)
 * spmv_hip_csr_power_iterate_halo uses the column split where halo setup made one. */
int spmv_hip_csr_split_columns(spmv_csr_dev *m, int col_lo, int col_hi, long long *counts);
int spmv_hip_csr_run_split(spmv_csr_dev *m, int part, const void *d_x, void *d_y, void *stream);
int spmv_hip_csr_run_part(spmv_csr_dev *m, int part, const void *d_x, void *d_y, void *stream);
int spmv_hip_csr_needed_ranges(const spmv_csr_dev *m, int max_ranges, int *ranges, int *count);
int spmv_hip_halo_plan(int ranks, int rank, const int *bounds, const int *counts, const int *ranges, int stride,
                       int max_segments, int *send, int *nsend, int *recv, int *nrecv);
int spmv_hip_comm_halo_setup(spmv_csr_dev *m, const int *bounds);
int spmv_hip_comm_halo_exchange(void *d_vec, int value_bytes, void *stream);
int spmv_hip_comm_halo_info(long long *send_values, long long *recv_values, int *peers);
int spmv_hip_csr_power_iterate_halo(spmv_csr_dev *m, int variant, int iters, double *lambda, float *ms_total);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_AMD_SPMV_HIP_H */
