"""The head of an x-window block (csr_stream_local): the block's records -- desc, ldesc, sdesc, lbase, pdesc -- are
fetched back to back behind one wait, and what a plan has (shared line lists, segments) picks the body of the kernel
that runs instead of being a pointer the kernel tests.  Nothing of the arithmetic changed, so every body -- {slot stream,
pattern plan} x {own, shared line lists} x {segments, segments and tables, tables only} -- must give the same bits on
one matrix, in whole launches, in part launches (ids) and at every edge of the rounded grid, and those bits must pass the
row gates against the oracle."""
import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import synth
from _util import assert_parity, assert_parity_f32
from test_gpu_plan_sharing import cut_blocks

pytestmark = pytest.mark.gpu

CAP, UNIT = 2048, 512   # a block's stage; a block of more than CAP - UNIT entries (from its base) is staged straight-line
MATRICES = {"kkt 8x8x8": lambda: synth.kkt_like((8, 8, 8), 5),
            "kkt 12x10x9": lambda: synth.kkt_like((12, 10, 9), 5),
            "fem 4x4x5": lambda: synth.fem_like((4, 4, 5), 1)}


@pytest.fixture
def forced():
    """local_cap CAP for the test; the knobs the tests set themselves are as they were after it, also when a failed test
    leaves combinations() unfinished."""
    others = ("local_patterns", "local_share", "local_segment_cap", "stream_xcd")
    with sp.tuning(local_cap=CAP, **{k: sp.get_tuning(k) for k in others}):
        yield


def blocks_of(rp, lo, hi):
    """[(first row, end row)] of the handle of rows [lo, hi), as upload cuts them (its row_ptr counts from its first entry)."""
    return cut_blocks(np.asarray(rp[lo:hi + 1], dtype=np.int64) - int(rp[lo]))


def last_block_is_short(rp, lo, hi):
    own = np.asarray(rp[lo:hi + 1], dtype=np.int64) - int(rp[lo])
    r0, r1 = blocks_of(rp, lo, hi)[-1]
    return int(own[r1]) - (int(own[r0]) & ~3) <= CAP - UNIT


def gate(y, ref, rp, col, val, x, lo, hi, what):
    """The row gate of the dtype on the handle's rows."""
    e0, e1 = int(rp[lo]), int(rp[hi])
    own_rp = (np.asarray(rp[lo:hi + 1], dtype=np.int64) - e0).astype(np.int32)
    if val.dtype == np.float64:
        assert_parity(y, ref[lo:hi], own_rp, col[e0:e1], val[e0:e1], x, what=what)
    else:
        assert_parity_f32(y, ref[lo:hi], own_rp, col[e0:e1], val[e0:e1], x, what=what)


def product(dev, x, lo, hi, parts=False):
    """y of the handle's rows: one whole launch, or part 0 then part 1 of its split; y filled with 0xFF before."""
    sp.lib().spmv_hip_memset(dev.y_ptr, 0xFF, dev.M * x.itemsize)
    if not parts:
        return dev.spmv(x, sp.CSR_STREAM)[lo:hi].copy()
    dev.set_x(x)
    dev.run_part(0)
    dev.run_part(1)
    sp.hip_sync()
    return dev.get_y()[lo:hi].copy()


def combinations(M, rp, col, val, lo, hi):
    """(name, info, handle) of fresh uploads of rows [lo, hi) under every knob combination: local_patterns 0 / 1 and
    local_share 0 / 1 at upload; with a pattern plan, the segment cap as the LDS budget sets it (every block a segment),
    one uint4 below the widest segment (those blocks keep {0, 0} and their tables) and below any (tables only)."""
    widest = None
    for patterns in (1, 0):
        for share in (0, 1):
            for cap in (("budget", "below widest", "none") if patterns else ("budget",)):
                segment_cap = {"budget": 0, "none": 1}.get(cap) if cap != "below widest" else widest - 16
                with sp.tuning(local_patterns=patterns, local_share=share, local_segment_cap=segment_cap), \
                        sp.CsrDevice(M, M, rp, col, val, row0=lo, row1=hi) as dev:
                    info = dev.info()
                    name = f"patterns {patterns} share {share} segments {cap}"
                    assert info["local_blocks"] == len(blocks_of(rp, lo, hi)), (name, info["local_blocks"])
                    assert (info["pattern_slots"] > 0) == bool(patterns), (name, info)
                    assert (info["local_lists_stored"] > 0) == bool(share), (name, info)
                    if patterns:
                        rows = info["pattern_table_rows"]
                        if cap == "budget":
                            # (rows may be > 0 already: a block of many short rows is wider than the LDS budget)
                            assert rows < hi - lo and info["pattern_segment_max"] > 16, (name, info)
                            widest = info["pattern_segment_max"] if widest is None else widest
                        elif cap == "none":
                            assert rows == hi - lo and info["pattern_segment_max"] == 0, (name, info)
                        elif len(blocks_of(rp, lo, hi)) > 1:
                            assert 0 < rows <= hi - lo and info["pattern_segment_max"] < widest, (name, info)
                    yield name, info, dev


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("matrix", sorted(MATRICES))
def test_every_instantiation_gives_the_same_bits(gpu, oracle, forced, matrix, dtype):
    rng = np.random.default_rng(4101)
    M, rp, col, val = MATRICES[matrix]()
    val = val.astype(dtype)
    x = rng.uniform(-1, 1, M).astype(dtype)
    ref = (oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64)(rp, col, val, x)
    # the whole matrix (its split has no boundary block: part 1 is an empty launch), and a row range in the middle, whose
    # x lines lie on both sides of its own range (both parts have blocks; its first line is far from line 0)
    mixed_tables = 0
    for lo, hi in ((0, M), (M // 3 + 1, 2 * M // 3 + 7)):
        want = None
        for name, info, dev in combinations(M, rp, col, val, lo, hi):
            what = f"{matrix} {np.dtype(dtype).name} rows [{lo}, {hi}) {name}"
            y = product(dev, x, lo, hi)
            gate(y, ref, rp, col, val, x, lo, hi, what)
            want = y.tobytes() if want is None else want
            assert y.tobytes() == want, what
            counts = dev.split_interior()
            assert counts["interior_blocks"] + counts["boundary_blocks"] == info["local_blocks"], (what, counts)
            assert (counts["boundary_blocks"] == 0) == (lo == 0 and hi == M), (what, counts)
            assert product(dev, x, lo, hi, parts=True).tobytes() == want, what + " part 0 then part 1"
            mixed_tables += 0 < info.get("pattern_table_rows", 0) < hi - lo
    assert mixed_tables > 0   # some handle had both kinds of blocks: segments and {0, 0}


def rows_for_blocks(rp, want, short_last):
    """hi such that rows [0, hi) are cut into `want` blocks, the last of them cut short (or not)."""
    whole = blocks_of(rp, 0, len(rp) - 1)   # (cut greedily from row 0: a prefix of the rows has a prefix of the blocks)
    assert len(whole) > want, (len(whole), want)
    hi = whole[want - 1][0] + 10 if short_last else whole[want - 1][1]
    assert len(blocks_of(rp, 0, hi)) == want and last_block_is_short(rp, 0, hi) == short_last, (want, hi)
    return hi


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", ["one block", "8 run - 1", "8 run + 1", "8 run", "short last block"])
def test_grid_edges(gpu, oracle, forced, shape, dtype):
    """The grid is rounded to whole runs on all 8 XCDs; workgroups past the last block return at once.  One block in a
    grid of 128; at a run length of 2 (stream_xcd) 15, 16 and 17 blocks in grids of 16, 16 and 32; a last block cut
    short (the plain loops) behind full ones."""
    rng = np.random.default_rng(4102)
    M, rp, col, val = synth.kkt_like((12, 10, 9), 5)
    val = val.astype(dtype)
    x = rng.uniform(-1, 1, M).astype(dtype)
    ref = (oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64)(rp, col, val, x)
    run = 2
    blocks, short = {"one block": (1, True), "8 run - 1": (8 * run - 1, False), "8 run + 1": (8 * run + 1, False),
                     "8 run": (8 * run, False), "short last block": (5, True)}[shape]
    hi = rows_for_blocks(rp, blocks, short)
    want = None
    with sp.tuning(stream_xcd=0 if shape == "one block" else run):
        for name, info, dev in combinations(M, rp, col, val, 0, hi):
            what = f"{shape} {np.dtype(dtype).name} rows [0, {hi}) {name}"
            assert info["local_blocks"] == blocks, (what, info["local_blocks"])
            y = product(dev, x, 0, hi)
            gate(y, ref, rp, col, val, x, 0, hi, what)
            want = y.tobytes() if want is None else want
            assert y.tobytes() == want, what


def test_stamps_of_the_head(gpu, forced):
    """The stamped launch with probe 2: the second word is the time the block's records were back, between the block's
    start and its end; y is the product's (the probe changes no arithmetic)."""
    rng = np.random.default_rng(4103)
    M, rp, col, val = synth.kkt_like((12, 10, 9), 5)
    x = rng.uniform(-1, 1, M)
    for share in (0, 1):
        with sp.tuning(local_patterns=1, local_share=share), sp.CsrDevice(M, M, rp, col, val) as dev:
            want = dev.spmv(x, sp.CSR_STREAM).tobytes()
            start, end, _, _ = dev.stamp_blocks(1)
            start2, head, _, xcd = dev.stamp_blocks(2001)
            assert dev.get_y().tobytes() == want
            assert np.all(start > 0) and np.all(end >= start)
            # (a head is two scalar round trips: far below a millisecond of the 100 MHz clock)
            assert np.all(head >= start2) and np.all(head - start2 < 100000), (head - start2).max()
            assert np.all((xcd >= 0) & (xcd < 8))
