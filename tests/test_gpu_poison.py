"""GPU: non-finite inputs and buffer edges on every product path -- what `0 x something` hides from finite data.

The kernels lean on discarded products in many places: zero padding behind col / val whose column is 0, products past
a block's end parked in LDS slots no row reads, whole 128-byte lines of x whose tail lies behind x[N-1], masked entries
behind a pass's end, clamped last pieces, HLL padding slots.  With finite data a multiply by a 0/1 mask in place of a
select, a lane that sums a padding product or a read past x all give the same bits.  With a NaN or an infinity they do
not, so here:

  poisoned x       a NaN (or +-Inf) in x reaches exactly the rows that store an entry in that column; every other row
                   keeps the bits of the clean launch (assert_poison_x: exact, judged by the structure and the oracle)
  poisoned values  a dozen NaN stored values make exactly their rows NaN (assert_poison_values)
  guard bands      x and y inside larger allocations, NaN around x, 0xA5 around y: finite results, untouched guards
  SpMM             a NaN column of X stays in its column of Y; a NaN element reaches the rows that read it

Values and x are uniform in [-1, 1] (the class of a poisoned row then does not depend on the order of its adds).
Every case first asserts through info() that the intended path was taken; local_patterns is pinned.  The HLL
expectation comes from the slab as downloaded: a row reads every slot it stores, padding included (an empty row of a
hack with slots reads x[0])."""
import contextlib

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import (assert_guard_bands, assert_parity, assert_parity_f32, assert_poison_values, assert_poison_x,
                   rows_reading)
from test_gpu_scaling import (DTYPES, F32, F64, TILE_IDS, DeviceBuffer, band, gather_rows, hll_of, plan, run, scattered,
                              short_rows, skewed, tile_cases)

pytestmark = pytest.mark.gpu

GUARD = 256


def reference(oracle, dtype):
    return oracle.csr_serial if np.dtype(dtype) == F64 else oracle.csr_f32_accum64


def uniform(rng, n, dtype):
    return rng.uniform(-1, 1, n).astype(dtype)


def rows_of(rp, lo, hi, col, val):
    """Rows [lo, hi) as a CSR of their own (global columns)."""
    e0, e1 = int(rp[lo]), int(rp[hi])
    return (np.asarray(rp[lo:hi + 1]) - rp[lo]).astype(np.int32), col[e0:e1], val[e0:e1]


def slab_rows(dev):
    """What a slab handle's rows store, padding slots included, as CSR: (rp, col, val) of its M_local rows (slot (i, j)
    of hack h at hack_off[h] + i * maxnz[h] + j)."""
    off, mz, ja, as_ = dev.download()
    M = dev.info()["M_local"]
    r = np.arange(M)
    lens = mz[r // 32].astype(np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    at = np.repeat(off[r // 32] + (r % 32) * lens - rp[:-1], lens) + np.arange(rp[-1])
    assert rp[-1] < 2 ** 31
    return rp.astype(np.int32), ja[at], as_[at]


# ------------------------------------------------------------------ poisoned x
def poison_set(rng, rp, col, N, share=0.3):
    """N - 1, then seeded random columns until the share of rows that read one of them first reaches `share`."""
    M = len(rp) - 1
    need = int(np.ceil(share * M))
    nonempty = np.flatnonzero(np.diff(rp) > 0)
    assert len(nonempty) >= need, "too many empty rows for a poisoned set"
    # (about -ln(0.7) N / (entries per row) columns are needed: the first draw usually holds them)
    seq, more = np.array([N - 1], dtype=np.int64), 1024 + N * len(nonempty) // (2 * max(len(col), 1))
    while True:
        seq = np.concatenate([seq, rng.integers(0, N, more)])
        u, first = np.unique(seq, return_index=True)          # the draw at which a column joins the set
        at = np.minimum(np.searchsorted(u, col), len(u) - 1)
        t = np.where(u[at] == col, first[at], len(seq))
        t_row = np.full(M, len(seq), dtype=np.int64)
        t_row[nonempty] = np.minimum.reduceat(t, np.asarray(rp, dtype=np.int64)[nonempty])
        reached = np.sort(t_row)[need - 1]
        if reached < len(seq):
            return np.unique(seq[:reached + 1])
        assert len(seq) < 64 * N, "the columns of the structure cannot reach the share"
        more = 3 * len(seq)


SHARES = {}


def check_poisoned_x(oracle, rng, stored, x, launch, what):
    """launch(x) -> the rows of `stored` = (rp, col, val).  Six single columns (0, N - 1 and the two sides of the fp64
    and of the fp32 line edge), then a set touching 20 .. 80 % of the rows with NaN, then the set half +Inf half -Inf."""
    rp, col, val = stored
    N, ref = len(x), reference(oracle, x.dtype)
    y_clean = launch(x)
    assert np.isfinite(y_clean).all(), f"{what}: clean launch"

    def one(cols, values, tag):
        xp = x.copy()
        xp[cols] = values
        assert_poison_x(y_clean, launch(xp), rp, col, val, xp, ref(rp, col, val, xp), f"{what}, {tag}")
        return xp

    for c in (0, N - 1, 15, 16, 31, 32):
        one([c], np.nan, f"NaN in column {c}")
    cols = poison_set(rng, rp, col, N)
    mask = np.zeros(N, dtype=bool)
    mask[cols] = True
    share = rows_reading(rp, col, mask).mean()
    assert 0.2 <= share <= 0.8, f"{what}: the poisoned set touches {share:.1%} of the rows"
    SHARES[what] = share
    print(f"poisoned set, {what}: {len(cols)} columns touch {share:.1%} of the rows")
    one(cols, np.nan, "NaN set")
    one(cols, np.where(np.arange(len(cols)) % 2 == 0, np.inf, -np.inf), "+-Inf set")
    assert launch(x).tobytes() == y_clean.tobytes(), f"{what}: the clean launch after the poisoned ones"


class Data:
    """Uniform values and x on a structure."""

    def __init__(self, rng, M, N, rp, col, dtype):
        self.M, self.N, self.rp, self.col = M, N, np.asarray(rp, np.int32), np.asarray(col, np.int32)
        self.dtype, self.val, self.x = dtype, uniform(rng, self.rp[-1], dtype), uniform(rng, N, dtype)


@contextlib.contextmanager
def csr_handle(data, knobs, fingerprint, what, rows=(0, None), val=None):
    knobs = {"local_patterns": 0, **knobs}
    assert knobs["local_patterns"] in (0, 1)
    with sp.tuning(**knobs):
        with sp.CsrDevice(data.M, data.N, data.rp, data.col, data.val if val is None else val, *rows) as dev:
            info = dev.info()
            assert info["value_bytes"] == np.dtype(data.dtype).itemsize
            assert fingerprint(info), f"{what}: path not taken: {plan(info)}"
            yield dev, info


@contextlib.contextmanager
def hll_handle(data, knobs, fingerprint, what, hacks=(0, None), val=None):
    knobs = {"local_patterns": 0, **knobs}
    with sp.tuning(**knobs):
        with sp.HllDevice(hll_of(data.M, data.N, data.rp, data.col, data.val if val is None else val), *hacks) as dev:
            info = dev.info()
            assert fingerprint(info), f"{what}: path not taken: {plan(info)}"
            yield dev, info


def csr_x_case(oracle, rng, data, knobs, fingerprint, variant, what, rows=None):
    lo, hi = rows or (0, data.M)
    with csr_handle(data, knobs, fingerprint, what, (lo, hi)) as (dev, _):
        check_poisoned_x(oracle, rng, rows_of(data.rp, lo, hi, data.col, data.val), data.x,
                         lambda x: run(dev, x, variant)[lo:hi], what)


def hll_x_case(oracle, rng, data, knobs, fingerprint, variant, what, hacks=(0, None)):
    with hll_handle(data, knobs, fingerprint, what, hacks) as (dev, info):
        lo, hi = info["row0"], info["row0"] + info["M_local"]
        check_poisoned_x(oracle, rng, slab_rows(dev), data.x, lambda x: run(dev, x, variant)[lo:hi], what)


@DTYPES
@pytest.mark.parametrize("vname", sorted(sp.CSR_VARIANTS))
def test_x_csr_explicit_variants(gpu, oracle, dtype, vname):
    rng = np.random.default_rng(201)
    data = Data(rng, *gather_rows(rng), dtype)
    csr_x_case(oracle, rng, data, {}, lambda i: i["lanes_per_row"] >= 2 and i["long_rows"] > 0, sp.CSR_VARIANTS[vname],
               f"csr {vname} {np.dtype(dtype).name}")


@DTYPES
@pytest.mark.parametrize("cap", [2048, 4096, 8192])
def test_x_csr_stream_with_long_row_pieces(gpu, oracle, dtype, cap):
    rng = np.random.default_rng(202)
    data = Data(rng, *gather_rows(rng), dtype)
    pieces = int((np.diff(data.rp) > cap - 3).sum())
    csr_x_case(oracle, rng, data, {"stream_cap": cap, "stream_local": 0, "stream_tile": 0},
               lambda i: i["stream_kernel"] == 0 and i["long_rows"] == pieces > 0, sp.CSR_STREAM,
               f"csr_stream cap={cap} {np.dtype(dtype).name}")


@DTYPES
def test_x_csr_stream_short(gpu, oracle, dtype):
    rng = np.random.default_rng(203)
    data = Data(rng, *short_rows(rng), dtype)
    csr_x_case(oracle, rng, data, {"stream_cap": 2048, "stream_local": 0, "stream_tile": 0},
               lambda i: i["stream_kernel"] == 2 and i["local_blocks"] == 0, sp.CSR_STREAM,
               f"csr_stream_short {np.dtype(dtype).name}")


def local_ok(patterns):
    return lambda i: i["stream_kernel"] == 1 and i["local_blocks"] > 0 and (i["pattern_slots"] > 0) == bool(patterns)


@DTYPES
@pytest.mark.parametrize("patterns", [0, 1])
@pytest.mark.parametrize("lcap", [1024, 2048, 3072])
def test_x_csr_stream_local(gpu, oracle, dtype, lcap, patterns):
    rng = np.random.default_rng(204 + lcap)
    data = Data(rng, *band(rng, far=0.05), dtype)
    csr_x_case(oracle, rng, data, {"local_cap": lcap, "local_patterns": patterns}, local_ok(patterns), sp.CSR_STREAM,
               f"csr_stream_local cap={lcap} patterns={patterns} {np.dtype(dtype).name}")


def skew_split(rng):
    M, N = 200_000, 1_000_000
    lens = rng.poisson(5.5, M).astype(np.int64)
    lens[rng.choice(M, 60, replace=False)] = 1000
    rp, col = scattered(rng, M, N, lens=lens)
    limit = max(128, 16 * (int(rp[-1]) // M))
    return (M, N, rp, col), np.flatnonzero(lens > limit)


SKEW_KNOBS = {"skew_rows": 1, "stream_local": 0, "stream_tile": 0}


def skew_ok(split):
    return lambda i: i["local_blocks"] == 0 and i["tile_blocks"] == 0 and i["long_rows"] == len(split) > 0


@DTYPES
def test_x_csr_skew_row_split(gpu, oracle, dtype):
    rng = np.random.default_rng(206)
    structure, split = skew_split(rng)
    csr_x_case(oracle, rng, Data(rng, *structure, dtype), SKEW_KNOBS, skew_ok(split), sp.CSR_STREAM,
               f"skew row split {np.dtype(dtype).name}")


@DTYPES
def test_x_csr_row_block_handle(gpu, oracle, dtype):
    rng = np.random.default_rng(207)
    data = Data(rng, *gather_rows(rng), dtype)
    csr_x_case(oracle, rng, data, {"stream_local": 0, "stream_tile": 0},
               lambda i: (i["row0"], i["M_local"]) == (1000, 1999) and i["long_rows"] > 0, sp.CSR_STREAM,
               f"row block {np.dtype(dtype).name}", rows=(1000, 2999))


@DTYPES
def test_x_csr_run_part_and_run_split(gpu, oracle, dtype):
    """Each part on its own: the expectation for a part holds the entries of that part only (run_part: the rows of its
    blocks; run_split: the entries inside / outside the handle's own column range, part 1 added to a zeroed y)."""
    rng = np.random.default_rng(208)
    n = 30000
    data = Data(rng, *band(rng, n, n, 22, 150), dtype)
    bounds = sp.partition_rows(data.rp, 3)
    lo, hi = int(bounds[1]), int(bounds[2])
    rp, col, val = rows_of(data.rp, lo, hi, data.col, data.val)
    item = np.dtype(dtype).itemsize
    with csr_handle(data, {}, lambda i: i["local_blocks"] > 0, "run_part", (lo, hi)) as (dev, _):
        counts = dev.split_interior()
        assert counts["interior_blocks"] > 0 and counts["boundary_blocks"] > 0
        assert dev.split_columns(lo, hi)["halo_entries"] > 0

        def part(call, p, fill):
            def launch(x):
                dev.set_x(x)
                assert sp.lib().spmv_hip_memset(dev.y_ptr, fill, n * item) == 0
                call(p)
                sp.hip_sync()
                return dev.get_y()[lo:hi]
            return launch

        name = np.dtype(dtype).name
        outside = data.x.copy()
        outside[:lo], outside[hi:] = np.nan, np.nan          # NaN in every column outside the handle's own range
        inside = data.x.copy()
        inside[lo:hi] = np.nan
        # run_part: which rows a part owns shows in the clean launch (the others keep the 0xFF fill)
        written = [~np.isnan(part(dev.run_part, p, 0xFF)(data.x)) for p in (0, 1)]
        lens = np.diff(rp)
        assert np.array_equal(written[0], ~written[1]) and written[0].any() and written[1].any()
        for p in (0, 1):
            sel, keep = np.flatnonzero(written[p]), np.repeat(written[p], lens)
            rp_p = np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.int32)
            launch = part(dev.run_part, p, 0xFF)
            check_poisoned_x(oracle, rng, (rp_p, col[keep], val[keep]), data.x, lambda x: launch(x)[sel],
                             f"run_part({p}) {name}")
            y = launch(inside)                                 # the other part's rows keep the fill
            assert (np.ascontiguousarray(y[~written[p]]).view(np.uint8) == 0xFF).all(), f"run_part({p}) wrote foreign rows"
        launch = part(dev.run_part, 0, 0xFF)                   # interior blocks read the own range of x only
        assert launch(outside).tobytes() == launch(data.x).tobytes(), "run_part(0) read x outside the own range"
        # run_split: the rows that store an entry of the part, as a CSR of that part's entries
        own = (col >= lo) & (col < hi)
        rows = np.repeat(np.arange(hi - lo), lens)
        for p, keep, other in ((0, own, outside), (1, ~own, inside)):
            n_p = np.bincount(rows[keep], minlength=hi - lo)
            sel = np.flatnonzero(n_p)
            rp_p = np.concatenate([[0], np.cumsum(n_p[sel])]).astype(np.int32)
            launch = part(dev.run_split, p, 0xFF if p == 0 else 0)
            check_poisoned_x(oracle, rng, (rp_p, col[keep], val[keep]), data.x, lambda x: launch(x)[sel],
                             f"run_split({p}) {name}")
            assert launch(other).tobytes() == launch(data.x).tobytes(), f"run_split({p}) read the other part's columns"


# (every plan of tile_cases but the middle tier: that tier exists from 2^22 entries scattered over 2^25 columns only, and
# building, uploading and poisoning a case of that size eight times takes far longer than a few seconds)
TILE_PLANS = [w for w in TILE_IDS if w != "mid tier"]


@DTYPES
@pytest.mark.parametrize("which", TILE_PLANS + ["gather passes, tile_gather_ahead=1"])
def test_x_csr_tile_plans(gpu, oracle, dtype, which):
    rng = np.random.default_rng(205)
    name, _, ahead = which.partition(", tile_gather_ahead=")
    for what, structure, knobs, fingerprint, _ in tile_cases(rng, dtype):
        if what != name:
            continue
        if ahead:
            knobs = dict(knobs, tile_gather_ahead=int(ahead))
        csr_x_case(oracle, rng, Data(rng, *structure, dtype), knobs, fingerprint, sp.CSR_STREAM,
                   f"csr_tile {which} {np.dtype(dtype).name}")
        return
    raise AssertionError(which)


@pytest.mark.parametrize("vname", sorted(sp.HLL_VARIANTS))
def test_x_hll_explicit_variants(gpu, oracle, vname):
    rng = np.random.default_rng(209)
    data = Data(rng, *gather_rows(rng), F64)
    hll_x_case(oracle, rng, data, {}, lambda i: i["hacks"] == (data.M + 31) // 32, sp.HLL_VARIANTS[vname], f"hll {vname}")


def test_x_hll_lds(gpu, oracle):
    rng = np.random.default_rng(210)
    data = Data(rng, *gather_rows(rng), F64)
    hll_x_case(oracle, rng, data, {"stream_local": 0, "stream_tile": 0},
               lambda i: i["stream_kernel"] == 0 and i["local_blocks"] == 0 and i["tile_blocks"] == 0, sp.HLL_LDS, "hll_lds")


@pytest.mark.parametrize("patterns", [0, 1])
def test_x_hll_lds_local(gpu, oracle, patterns):
    rng = np.random.default_rng(211)
    data = Data(rng, *band(rng, 4099, 4500, 27, 200), F64)
    hll_x_case(oracle, rng, data, {"local_patterns": patterns}, local_ok(patterns), sp.HLL_LDS,
               f"hll_lds_local patterns={patterns}")


HLL_TILE_KNOBS = {"stream_tile": 1, "tile_rows": 1024, "stream_local": 0}


def hll_tile_ok(i):
    return i["stream_kernel"] == 2 and i["tile_entries"] + i["tile_long_entries"] == i["slots"]


def hll_tile_structure(rng):
    M, N = 9001, 1_500_000
    return (M, N) + scattered(rng, M, N, 16)


def test_x_hll_tile_kernel_over_the_slab(gpu, oracle):
    rng = np.random.default_rng(212)
    data = Data(rng, *hll_tile_structure(rng), F64)
    hll_x_case(oracle, rng, data, HLL_TILE_KNOBS, hll_tile_ok, sp.HLL_LDS, "hll tiles")


def hack_range(data):
    hb = sp.partition_hacks(hll_of(data.M, data.N, data.rp, data.col, data.val), 3)
    rb = sp.hack_bounds_to_rows(hb, data.M)
    return (int(hb[1]), int(hb[2])), (int(rb[1]), int(rb[2]))


def test_x_hll_hack_range_and_device_built_slab(gpu, oracle):
    rng = np.random.default_rng(213)
    data = Data(rng, *band(rng, 4099, 4500, 27, 200, far=0.05), F64)
    hacks, (lo, hi) = hack_range(data)
    hll_x_case(oracle, rng, data, {}, lambda i: (i["row0"], i["M_local"]) == (lo, hi - lo), sp.HLL_AUTO, "hll hack range",
               hacks)
    with sp.tuning(local_patterns=0):
        with sp.CsrDevice(data.M, data.N, data.rp, data.col, data.val) as c, sp.HllDevice.from_csr_device(c) as dev:
            info = dev.info()
            assert info["hacks"] == (data.M + 31) // 32 and info["local_blocks"] > 0, plan(info)
            check_poisoned_x(oracle, rng, slab_rows(dev), data.x, lambda x: run(dev, x, sp.HLL_AUTO), "hll device-built slab")


def test_x_hll_empty_rows_read_x0_and_csr_rows_do_not(gpu, oracle):
    """The one documented difference between the formats: an empty row of a hack with slots is NaN when x[0] is."""
    rng = np.random.default_rng(214)
    data = Data(rng, *gather_rows(rng), F64)
    empty = np.flatnonzero(np.diff(data.rp) == 0)
    assert len(empty) > 10
    xp = data.x.copy()
    xp[0] = np.nan
    with hll_handle(data, {}, lambda i: True, "hll") as (dev, _):
        rp, col, val = slab_rows(dev)
        padded = empty[np.diff(rp)[empty] > 0]
        assert len(padded) > 10 and not col[rp[padded]].any() and not val[rp[padded]].any()
        assert np.isnan(run(dev, xp, sp.HLL_AUTO)[padded]).all()
    with csr_handle(data, {}, lambda i: True, "csr") as (dev, _):
        assert not run(dev, xp, sp.CSR_AUTO)[empty].any()


@DTYPES
def test_x_transposed_handle(gpu, oracle, dtype):
    rng = np.random.default_rng(215)
    data = Data(rng, *band(rng), dtype)
    assert data.M != data.N
    with csr_handle(data, {}, lambda i: True, "A") as (dev, _), sp.tuning(local_patterns=0), dev.transpose() as dt:
        info = dt.info()
        assert (info["M_total"], info["N"], info["nz"]) == (data.N, data.M, data.rp[-1]) and info["local_blocks"] > 0
        check_poisoned_x(oracle, rng, dt.download(), uniform(rng, data.M, dtype), lambda x: run(dt, x, sp.CSR_AUTO),
                         f"transposed handle {np.dtype(dtype).name}")


# ------------------------------------------------------------------ poisoned values
def value_positions(rng, rp, split_rows=()):
    """{what: (entry, row)}: about a dozen stored entries, each in a row of its own."""
    rp = np.asarray(rp, dtype=np.int64)
    lens, nz, M = np.diff(rp), int(rp[-1]), len(rp) - 1
    out, used = {}, set()

    def pick(what, entries):
        for e in entries:
            r = int(np.searchsorted(rp, e, side="right")) - 1
            if r not in used:
                used.add(r)
                out[what] = (int(e), r)
                return

    pick("first entry of the matrix", [0])
    pick("last entry of the matrix", [nz - 1])
    inner = M // 2 + np.flatnonzero(lens[M // 2:M - 1] >= 3)
    pick("first entry of an interior row", rp[inner[:1]])
    pick("last entry of an interior row", rp[inner[1:2] + 1] - 1)
    empty = np.flatnonzero(lens == 0)
    before = empty[(empty > 1) & (lens[np.maximum(empty - 1, 0)] > 0)]
    after = empty[(empty < M - 2) & (lens[np.minimum(empty + 1, M - 1)] > 0)]
    pick("last entry of the row before an empty row", rp[before[len(before) // 3:]] - 1)
    pick("first entry of the row after an empty row", rp[after[2 * len(after) // 3:] + 1])
    longest = np.argsort(-lens, kind="stable")[:4]
    pick("middle of the longest row", rp[longest] + lens[longest] // 2)
    rows = np.asarray(split_rows, dtype=np.int64)
    pick("middle of a row of the skew split", rp[rows] + lens[rows] // 2)
    for k in range(4):
        pick(f"random entry {k}", rng.integers(0, nz, 64))
    assert len(out) >= 9, out
    return out


def check_poisoned_values(rng, data, make, launch, what, split_rows=(), need=()):
    """make(val) -> a handle context; launch(dev) -> y.  One clean and one poisoned handle, the same plan."""
    picks = value_positions(rng, data.rp, split_rows)
    for label in need:
        assert label in picks, f"{what}: the structure has no {label}"
    val = data.val.copy()
    val[[e for e, _ in picks.values()]] = np.nan
    with make(None) as (d0, i0), make(val) as (d1, i1):
        assert plan(i0) == plan(i1), f"{what}: a NaN value changed the plan"
        assert_poison_values(launch(d0), launch(d1), [r for _, r in picks.values()], what)


EMPTY = ("last entry of the row before an empty row", "first entry of the row after an empty row")


@DTYPES
@pytest.mark.parametrize("path", ["csr_stream pieces", "csr_stream skew split", "csr_stream_local patterns",
                                  "csr_tile gather passes", "csr_tile packed", "csr_tile long-row tier"])
def test_values_csr(gpu, oracle, dtype, path):
    rng = np.random.default_rng(220)
    split, need = (), ()
    if path == "csr_stream pieces":
        structure, need = gather_rows(rng), EMPTY
        knobs = {"stream_cap": 2048, "stream_local": 0, "stream_tile": 0}
        ok = lambda i: i["stream_kernel"] == 0 and i["long_rows"] >= 5
    elif path == "csr_stream skew split":
        (structure, split), knobs, need = skew_split(rng), SKEW_KNOBS, ("middle of a row of the skew split",)
        ok = skew_ok(split)
    elif path == "csr_stream_local patterns":
        structure, knobs, ok, need = band(rng, far=0.05), {"local_patterns": 1}, local_ok(1), EMPTY
    else:
        structure, knobs, ok = next((s, k, f) for w, s, k, f, _ in tile_cases(rng, dtype) if "csr_tile " + w == path)
        need = EMPTY if path == "csr_tile long-row tier" else ()
    data = Data(rng, *structure, dtype)
    check_poisoned_values(rng, data, lambda val: csr_handle(data, knobs, ok, path, val=val),
                          lambda dev: run(dev, data.x, sp.CSR_STREAM), f"values, {path} {np.dtype(dtype).name}", split, need)


@pytest.mark.parametrize("path", ["hll_lds_local", "hll tiles"])
def test_values_hll(gpu, oracle, path):
    rng = np.random.default_rng(221)
    if path == "hll_lds_local":
        structure, knobs, ok, need = band(rng, 4099, 4500, 27, 200), {"local_patterns": 0}, local_ok(0), EMPTY
    else:
        structure, knobs, ok, need = hll_tile_structure(rng), HLL_TILE_KNOBS, hll_tile_ok, ()
    data = Data(rng, *structure, F64)
    check_poisoned_values(rng, data, lambda val: hll_handle(data, knobs, ok, path, val=val),
                          lambda dev: run(dev, data.x, sp.HLL_LDS), f"values, {path}", need=need)


# ------------------------------------------------------------------ guard bands on caller buffers
def guarded_product(dev, X, M, offset, k):
    """run_on (k = 0) or spmm_on with X at `offset` bytes from a 128-byte boundary between 256-byte bands of NaN, Y
    (0xFF) between bands of 0xA5: (Y, the bands before, the bands after)."""
    dtype, item = X.dtype, X.dtype.itemsize
    assert offset % item == 0
    front = (GUARD + offset) // item
    image_x = np.full(front + X.size + GUARD // item, np.nan, dtype=dtype)
    image_x[front:front + X.size] = X.reshape(-1)
    ybytes = M * max(k, 1) * item
    image_y = np.concatenate([np.full(GUARD, 0xA5, np.uint8), np.full(ybytes, 0xFF, np.uint8), np.full(GUARD, 0xA5, np.uint8)])
    with DeviceBuffer(image_x.nbytes) as dx, DeviceBuffer(image_y.nbytes) as dy:
        assert dx.p.value % 128 == 0 and dy.p.value % 128 == 0
        dx.upload(image_x, 0)
        dy.upload(image_y, 0)
        px, py = dx.p.value + GUARD + offset, dy.p.value + GUARD
        if k:
            dev.spmm_on(px, py, k)
        else:
            dev.run_on(px, py)
        got = dy.download(image_y.shape, np.uint8, 0)
    bands = lambda a: np.concatenate([a[:GUARD], a[-GUARD:]])
    return got[GUARD:-GUARD].view(dtype).reshape((M, k) if k else (M,)), bands(image_y), bands(got)


def check_guarded(oracle, rng, dev, stored, M, N, dtype, rows, what):
    """Every offset of x, SpMV and SpMM (k = 3): the row gate, finite rows, the bands, the rows outside the handle's."""
    lo, hi = rows
    rp, col, val = stored
    ref = reference(oracle, dtype)
    gate = assert_parity if np.dtype(dtype) == F64 else assert_parity_f32
    item = np.dtype(dtype).itemsize
    for k in (0, 3):
        X = uniform(rng, N * max(k, 1), dtype).reshape((N, k) if k else (N,))
        for offset in (0, 16, item):
            tag = f"{what}, x at +{offset}, " + (f"spmm_on k={k}" if k else "run_on")
            Y, before, after = guarded_product(dev, X, M, offset, k)
            assert_guard_bands(before, after, tag)
            outside = np.concatenate([Y[:lo], Y[hi:]]).view(np.uint8)
            assert (outside == 0xFF).all(), f"{tag}: rows outside [{lo}, {hi}) were written"
            for j in range(max(k, 1)):
                xj, yj = (np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y[lo:hi, j])) if k else (X, Y[lo:hi])
                assert np.isfinite(yj).all(), f"{tag}: non-finite row {np.flatnonzero(~np.isfinite(yj))[0]} of column {j}"
                gate(yj, ref(rp, col, val, xj), rp, col, val, xj, what=f"{tag} column {j}")


def tile_any(i):
    return i["stream_kernel"] == 3 and i["tile_blocks"] > 0


def guard_cases(rng, tail):
    """(what, structure, knobs, fingerprint, rows): N % 16 == tail, M no multiple of 32."""
    N = 5600 + tail
    yield "x-window", band(rng, 5003, N, far=0.05), {}, local_ok(0), None
    yield "x-window row block", band(rng, 5003, N, far=0.05), {}, local_ok(0), (1001, 4002)
    M, N = 40_003, 40_000 + tail
    yield ("staged tiles", (M, N) + scattered(rng, M, N, 12, sigma=200),
           dict(stream_tile=1, tile_rows=2048, tile_pack=0, stream_local=0),
           lambda i: tile_any(i) and i["local_blocks"] == 0 and i["tile_staged_entries"] > 0.5 * i["tile_entries"], None)
    M, N = 60_003, 60_000 + tail
    yield ("packed tiles", (M, N) + scattered(rng, M, N, 9, sigma=2500), dict(stream_tile=1, tile_rows=2048),
           lambda i: tile_any(i) and i["tile_staged_entries"] + i["tile_remainder_entries"] == i["tile_entries"]
           and i["tile_staged_cols"] > 0, None)
    M, N = 9001, 2_000_000 + tail
    lens = rng.poisson(14, M)
    lens[::997] = 3000
    yield ("expanded x", (M, N) + scattered(rng, M, N, lens=lens),
           dict(stream_tile=1, tile_rows=1024, tile_expand=1, tile_lmax=4096, tile_density=0, tile_pack=0, stream_local=0),
           lambda i: tile_any(i) and i["tile_expanded_entries"] >= i["tile_entries"] > 0, None)


GUARD_IDS = ["x-window", "x-window row block", "staged tiles", "packed tiles", "expanded x"]


@DTYPES
@pytest.mark.parametrize("tail", [1, 15])
@pytest.mark.parametrize("which", GUARD_IDS)
def test_guard_bands_csr(gpu, oracle, dtype, which, tail):
    rng = np.random.default_rng(230 + tail)
    for what, (M, N, rp, col), knobs, fingerprint, rows in guard_cases(rng, tail):
        if what != which:
            continue
        assert N % 16 == tail and all(M % m for m in (32, 64, 256))
        data = Data(rng, M, N, rp, col, dtype)
        lo, hi = rows or (0, M)
        with csr_handle(data, knobs, fingerprint, what, (lo, hi)) as (dev, _):
            check_guarded(oracle, rng, dev, rows_of(data.rp, lo, hi, data.col, data.val), M, N, dtype, (lo, hi),
                          f"guards, {what} N%16={tail} {np.dtype(dtype).name}")
        return
    raise AssertionError(which)


@pytest.mark.parametrize("tail", [1, 15])
@pytest.mark.parametrize("part", ["whole", "hack range"])
def test_guard_bands_hll_lds_local(gpu, oracle, tail, part):
    rng = np.random.default_rng(240 + tail)
    M, N = 4099, 4496 + tail
    assert N % 16 == tail and all(M % m for m in (32, 64, 256))
    data = Data(rng, *band(rng, M, N, 27, 200, far=0.05), F64)
    hacks, rows = hack_range(data) if part == "hack range" else ((0, None), (0, M))
    with hll_handle(data, {}, local_ok(0), "hll_lds_local", hacks) as (dev, info):
        assert (info["row0"], info["row0"] + info["M_local"]) == rows
        check_guarded(oracle, rng, dev, rows_of(data.rp, *rows, data.col, data.val), M, N, F64, rows,
                      f"guards, hll_lds_local {part} N%16={tail}")


# ------------------------------------------------------------------ SpMM column isolation
def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bad = np.flatnonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} elements changed bits; first at flat index {bad[0]}"


def check_spmm_isolation(rng, spmm, stored, N, dtype, what, empty_rows=True):
    rp, col, _ = stored
    stores = np.diff(rp) > 0
    assert stores.any() and (not empty_rows or not stores.all())
    for k in (3, 8, 17):
        X = uniform(rng, N * k, dtype).reshape(N, k)
        Y = spmm(X)
        assert np.isfinite(Y).all() and not Y[~stores].any()
        for j in (0, k // 2, k - 1):                      # (a) a whole column of X
            Xp = X.copy()
            Xp[:, j] = np.nan
            Yp = spmm(Xp)
            others = np.arange(k) != j
            same_bits(Yp[:, others], Y[:, others], f"{what} k={k}: NaN column {j} of X, the other columns of Y")
            assert np.isnan(Yp[stores, j]).all(), f"{what} k={k}: column {j} is not NaN on every row that stores an entry"
            assert not Yp[~stores, j].any() and not np.isnan(Yp[~stores, j]).any(), f"{what} k={k}: an empty row of column {j}"
        for j, c in zip((0, k // 2, k - 1), (0, N - 1, int(col[rng.integers(0, len(col))]))):   # (b) one element
            Xp = X.copy()
            Xp[c, j] = np.nan
            Yp = spmm(Xp)
            mask = np.zeros(N, dtype=bool)
            mask[c] = True
            reads = rows_reading(rp, col, mask)
            hit = np.zeros(Y.shape, dtype=bool)
            hit[reads, j] = True
            assert np.isnan(Yp[hit]).all(), f"{what} k={k}: X[{c}, {j}] = NaN does not reach a row that reads column {c}"
            same_bits(Yp[~hit], Y[~hit], f"{what} k={k}: X[{c}, {j}] = NaN, every other element of Y")


@DTYPES
def test_spmm_csr_column_isolation(gpu, oracle, dtype):
    rng = np.random.default_rng(250)
    data = Data(rng, *gather_rows(rng), dtype)
    with csr_handle(data, {}, lambda i: i["long_rows"] > 0, "csr spmm") as (dev, _):
        check_spmm_isolation(rng, dev.spmm, (data.rp, data.col, data.val), data.N, dtype, f"csr spmm {np.dtype(dtype).name}")


def test_spmm_hll_column_isolation(gpu, oracle):
    rng = np.random.default_rng(251)
    data = Data(rng, *gather_rows(rng), F64)
    with hll_handle(data, {}, lambda i: i["hacks"] == (data.M + 31) // 32, "hll spmm") as (dev, _):
        assert dev.download()[1].max() > 2048            # one-row windows longer than the stage
        # (every row of a hack with slots stores slots: an empty row of the matrix reads x[0] through its padding)
        check_spmm_isolation(rng, dev.spmm, slab_rows(dev), data.N, F64, "hll spmm", empty_rows=False)
