"""Shared x-window plans ("local_share"): every distinct pattern segment and every distinct line list (relative to its
first line) is stored once, the blocks that repeat it point at the one copy.  Sharing changes where a block finds its
plan, never what the plan says: y must be the bits of the unshared plan (local_share 0), of the plan shared under a
hash that tells nothing apart (2: the byte comparison has to split every group), and of the slot-stream kernel."""
import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import synth

pytestmark = pytest.mark.gpu

CAP, ROWS_CAP, SKEW = 2048, 1024, 64   # csr_build_blocks: entries and rows per block, entries per lane of a row sum
# The kkt-like grid: 16 128 rows, 200 blocks.  Blocks repeat with the period of (row start mod 16, position in the grid
# line), so short grid lines repeat soonest: 52 (fp64) / 70 (fp32) distinct block patterns and 32 / 38 distinct line lists
# by count_distinct below -- a 20 x 20 x 20 grid of the same size has 202 blocks and not two alike.
KKT = (12, 12, 56)


@pytest.fixture
def forced():
    with sp.tuning(local_patterns=1, local_cap=CAP):
        yield


def cut_blocks(rp):
    """[(first row, end row)] as csr_build_blocks cuts rows none of which is long."""
    def lanes(nrows):
        return 1 if nrows > 128 else min(64, 1 << ((256 // nrows).bit_length() - 1))
    M, out, r = len(rp) - 1, [], 0
    assert np.max(np.diff(rp)) <= CAP - 3
    while r < M:
        base, r1, longest = int(rp[r]) & ~3, r, 0
        while r1 < M and r1 - r < ROWS_CAP and int(rp[r1 + 1]) - base <= CAP:
            n = int(rp[r1 + 1] - rp[r1])
            if r1 > r and max(longest, n) // lanes(r1 - r + 1) > SKEW:
                break
            longest, r1 = max(longest, n), r1 + 1
        out.append((r, r1))
        r = r1
    return out


def count_distinct(rp, col, itemsize):
    """(blocks, distinct block patterns, distinct relative line lists): a block's pattern is its rows' lengths, its
    first entry's offset from the multiple of 4 it is staged from, and its slots (rank of the x line in the block's list
    x elements per line + column within the line) -- what its segment is made from."""
    shift = 4 if itemsize == 8 else 5
    patterns, lists, blocks = set(), set(), cut_blocks(rp)
    for r0, r1 in blocks:
        c = col[rp[r0]:rp[r1]].astype(np.int64)
        lines = np.unique(c >> shift)
        slots = (np.searchsorted(lines, c >> shift) << shift) | (c & ((1 << shift) - 1))
        patterns.add((int(rp[r0]) & 3, np.diff(rp[r0:r1 + 1]).tobytes(), slots.tobytes()))
        lists.add((lines - lines[0]).tobytes() if len(lines) else b"")
    return len(blocks), len(patterns), len(lists)


def stencil_1d(n, offsets, rng, dtype):
    """Row i holds columns i + o (o in offsets, inside [0, n)): every row its predecessor shifted by one."""
    offs = np.array(sorted(offsets))
    rows = np.repeat(np.arange(n), len(offs))
    cols = rows + np.tile(offs, n)
    keep = (cols >= 0) & (cols < n)
    rows, cols = rows[keep], cols[keep]
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, rows + 1, 1)
    return n, np.cumsum(rp).astype(np.int32), cols.astype(np.int32), rng.uniform(-1, 1, len(cols)).astype(dtype)


def concat(parts):
    """Block-diagonal stack of (n, rp, col, val) matrices."""
    rps, cols, vals, c_off, e_off = [np.zeros(1, np.int32)], [], [], 0, 0
    for m, rp, col, val in parts:
        rps.append(rp[1:] + e_off)
        cols.append(col + c_off)
        vals.append(val)
        c_off += m
        e_off += int(rp[-1])
    return c_off, np.concatenate(rps).astype(np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def gapped_band(M, per_row, half_width, rng):
    """Random columns within half_width of the diagonal, drawn only from a random half of the 128-byte lines of x: the
    gaps in every block's line list, its row lengths and its slots are its own."""
    kept = np.flatnonzero(np.repeat(rng.random((M + 15) // 16) < 0.5, 16)[:M])
    i = np.arange(M)
    lo, hi = np.searchsorted(kept, i - half_width), np.searchsorted(kept, i + half_width)
    assert np.all(hi > lo)
    cols = np.sort(kept[lo[:, None] + (rng.random((M, per_row)) * (hi - lo)[:, None]).astype(np.int64)], axis=1)
    fresh = np.ones_like(cols, dtype=bool)
    fresh[:, 1:] = cols[:, 1:] != cols[:, :-1]
    rp = np.concatenate([[0], np.cumsum(fresh.sum(axis=1))]).astype(np.int32)
    col = cols[fresh].astype(np.int32)
    return M, rp, col, rng.uniform(-1, 1, len(col))


def uploads(M, rp, col, val, x, lo=0, hi=None, run=None):
    """{local_share: (info, y of the pattern kernel, y of the slot stream)} of fresh uploads of rows [lo, hi)."""
    hi, out = M if hi is None else hi, {}
    for share in (1, 0, 2):
        with sp.tuning(local_share=share), sp.CsrDevice(M, M, rp, col, val, row0=lo, row1=hi) as dev:
            info, ys = dev.info(), []
            assert info["local_blocks"] > 0 and info["pattern_slots"] > 0, info
            for patterns in (1, 0):
                with sp.tuning(local_patterns=patterns):
                    sp.lib().spmv_hip_memset(dev.y_ptr, 0xFF, dev.M * x.itemsize)
                    if run is None:
                        ys.append(dev.spmv(x, sp.CSR_STREAM)[lo:hi].copy())
                    else:
                        dev.set_x(x)
                        run(dev)
                        sp.hip_sync()
                        ys.append(dev.get_y()[lo:hi].copy())
            out[share] = (info, ys[0], ys[1])
    return out


def assert_same_bits(got):
    want = got[0][2].tobytes()   # the unshared plan's slot stream
    for share, (_, y, y0) in got.items():
        assert y.tobytes() == want and y0.tobytes() == want, f"local_share {share}"


def assert_close(y, ref, dtype):
    tol = 1e-10 if dtype == np.float64 else 1e-5
    assert np.max(np.abs(y.astype(np.float64) - ref)) <= tol * max(np.max(np.abs(ref)), 1e-300)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shared_plan_gives_the_unshared_bits_in_fewer_bytes(gpu, oracle, forced, dtype):
    rng = np.random.default_rng(3001)
    M, rp, col, val = synth.kkt_like(KKT, 5)
    val = val.astype(dtype)
    blocks, patterns, lists = count_distinct(rp, col, np.dtype(dtype).itemsize)
    assert blocks >= 150 and 2 * patterns < blocks and 2 * lists < blocks, (blocks, patterns, lists)
    x = rng.uniform(-1, 1, M).astype(dtype)
    got = uploads(M, rp, col, val, x)
    assert_same_bits(got)
    assert_close(got[1][1], (oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64)(rp, col, val, x), dtype)
    on, off, weak = got[1][0], got[0][0], got[2][0]
    assert on["local_blocks"] == off["local_blocks"] == blocks and on["local_lines"] == off["local_lines"]
    assert on["stream_bytes"] < off["stream_bytes"] and on["device_bytes"] < off["device_bytes"], (on, off)
    # what sharing found is what the count above found (a segment holds nothing but its block's pattern)
    assert on["local_lists_stored"] == lists and 0 < on["pattern_segments_stored"] <= patterns, (on, patterns, lists)
    assert off["local_lists_stored"] == 0 and off["pattern_segments_stored"] == blocks  # (every block's segment fits)
    # the hash of the length alone: the byte comparison keeps apart what the hash did not
    assert on["stream_bytes"] <= weak["stream_bytes"] <= off["stream_bytes"] + 4 * blocks


def test_shared_plan_on_row_ranges_and_their_sub_lists(gpu, forced):
    """Two ranks' worth of rows, each handle through its interior / boundary sub-lists (the second has row0 > 0: its
    blocks' first lines lie far from line 0)."""
    rng = np.random.default_rng(3002)
    M, rp, col, val = synth.kkt_like(KKT, 5)
    x = rng.uniform(-1, 1, M)
    for lo, hi in ((0, M // 2), (M // 2, M)):
        whole = uploads(M, rp, col, val, x, lo, hi)
        assert_same_bits(whole)
        assert whole[1][0]["stream_bytes"] < whole[0][0]["stream_bytes"]

        seen = []

        def parts(dev):
            counts = dev.split_interior()   # (from the line lists, on the host: the blocks' first lines added back)
            assert counts["interior_blocks"] + counts["boundary_blocks"] == dev.info()["local_blocks"], counts
            seen.append(counts)
            dev.run_part(0)
            dev.run_part(1)
        split = uploads(M, rp, col, val, x, lo, hi, run=parts)
        assert_same_bits(split)
        assert seen[0]["boundary_blocks"] > 0 and all(c == seen[0] for c in seen), seen
        assert split[1][1].tobytes() == whole[0][2].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shared_plan_with_short_blocks_and_table_blocks(gpu, oracle, forced, dtype):
    """A last block cut short (the plain loops), and blocks of 2-entry rows whose segments are wider than the LDS budget
    (they keep {0, 0} and their tables) between blocks that share theirs."""
    rng = np.random.default_rng(3003)
    wide = stencil_1d(30000, range(-13, 14), rng, dtype)
    short = stencil_1d(60000, (0, 1), rng, dtype)
    for matrix, tables in ((stencil_1d(9001, range(-13, 14), rng, dtype), False), (concat([wide, short, wide]), True)):
        M, rp, col, val = matrix
        x = rng.uniform(-1, 1, M).astype(dtype)
        got = uploads(M, rp, col, val, x)
        assert_same_bits(got)
        assert_close(got[1][1], (oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64)(rp, col, val, x), dtype)
        on, off = got[1][0], got[0][0]
        assert (0 < on["pattern_table_rows"] < M) == tables and on["pattern_table_rows"] == off["pattern_table_rows"], on
        assert on["stream_bytes"] < off["stream_bytes"]


def test_nothing_shared_where_no_two_blocks_are_alike(gpu, oracle, forced):
    rng = np.random.default_rng(3004)
    M, rp, col, val = gapped_band(8000, 16, 600, rng)
    blocks, patterns, lists = count_distinct(rp, col, 8)
    assert blocks >= 40 and patterns == blocks and lists == blocks, (blocks, patterns, lists)
    x = rng.uniform(-1, 1, M)
    got = uploads(M, rp, col, val, x)
    assert_same_bits(got)
    assert_close(got[1][1], oracle.csr_serial(rp, col, val, x), np.float64)
    on, off, weak = got[1][0], got[0][0], got[2][0]
    assert on["local_blocks"] == blocks and on["local_lists_stored"] == blocks
    # every list and every segment still there, plus the blocks' first lines
    assert on["stream_bytes"] == weak["stream_bytes"] == off["stream_bytes"] + 4 * blocks
    assert on["device_bytes"] == weak["device_bytes"] == off["device_bytes"] + 4 * blocks


def test_hll_x_window_handles_are_unchanged(gpu, oracle, forced):
    """hll_lds_local uses the same staging helpers with lists of absolute ids: the knob does not reach it."""
    rng = np.random.default_rng(3005)
    M, rp, col, val = synth.kkt_like(KKT, 5)
    x = rng.uniform(-1, 1, M)
    hll = sp.convert_to_hll(sp.PreMatrix.from_arrays(M, M, np.repeat(np.arange(M, dtype=np.int32), np.diff(rp)), col, val))
    got = {}
    for share in (1, 0):
        with sp.tuning(local_share=share), sp.HllDevice(hll) as dev:
            info = dev.info()
            assert info["local_blocks"] > 0 and info["pattern_slots"] > 0
            got[share] = (info["device_bytes"], info["stream_bytes"], dev.spmv(x, sp.HLL_LDS).tobytes())
    assert got[1] == got[0]
    ref = oracle.csr_serial(rp, col, val, x)
    assert np.max(np.abs(np.frombuffer(got[1][2]) - ref)) <= 1e-10 * np.max(np.abs(ref))
