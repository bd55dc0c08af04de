"""GPU: every kernel path on wide-range data, row by row and through the power-of-two scaling identity.

Data: values and x with random signs and magnitudes over [2^-8, 1]; the scaled copy (D_r A D_c^-1, D_c x) with D_r,
D_c diagonal matrices of +-2^e (|e| <= 40 for fp32, 300 for fp64).  No kernel has atomics and no upload decision reads
values, so each result is a fixed sequence of adds set by the structure (and k) alone, and power-of-two scaling is
exact in IEEE arithmetic whatever that sequence is:

    y(D_r A D_c^-1, D_c x) == D_r y(A, x)   bit for bit (compared as numbers: +0 == -0, no NaN).

A term from the wrong row, a stale LDS slot or the wrong x column breaks that however small it is.  For every path:
(a) info() shows the path was taken, (b) the scaled handle passes the row gate against the oracle (assert_parity for
fp64, assert_parity_f32 for fp32), (c) the identity holds against an unscaled handle of the same structure, which
reports the same plan.  local_patterns is pinned (0 or 1) throughout: under auto, upload keeps or drops the pattern
plan by timing, and two handles could then report different plans.  Launch-time knobs (stream_xcd, stream_nt,
local_nt, tile_gather_ahead) must reproduce the default launch's bits; upload-time ones (skew_rows, tile_items,
local_cap) change the plan and are gated by the oracle."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import (assert_parity, assert_parity_f32, assert_same_numbers, banded_csr, coo_from_csr, random_csr,
                   scale_rows, scaled_copy, scaling, wide_range)

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


PLAN_KEYS = ("stream_kernel", "local_blocks", "local_lines", "local_stage_lines", "long_rows", "stream_blocks", "slots",
             "hacks", "pattern_slots", "auto_variant", "lanes_per_row", "nz")


def plan(info):
    return {k: v for k, v in info.items() if k in PLAN_KEYS or k.startswith("tile_")}


class Case:
    """Wide-range values and x on a structure, and the scaled copy."""

    def __init__(self, rng, M, N, rp, col, dtype):
        self.M, self.N, self.rp, self.col, self.dtype = M, N, np.asarray(rp, np.int32), np.asarray(col, np.int32), dtype
        self.val, self.x = wide_range(rng, self.rp[-1], dtype), wide_range(rng, N, dtype)
        self.dr, self.dc = scaling(rng, M, N, dtype)
        self.vs, self.xs = scaled_copy(self.rp, self.col, self.val, self.x, self.dr, self.dc)

    def gate(self, oracle, y, x, rows=None, what=""):
        """Rows [lo, hi) of y, the scaled matrix times x, row by row against the oracle."""
        lo, hi = rows if rows is not None else (0, self.M)
        rp, e0, e1 = self.rp[lo:hi + 1] - self.rp[lo], self.rp[lo], self.rp[hi]
        col, val = self.col[e0:e1], self.vs[e0:e1]
        if self.dtype == F64:
            assert_parity(y[lo:hi], oracle.csr_serial(rp, col, val, x), rp, col, val, x, what=what)
        else:
            assert_parity_f32(y[lo:hi], oracle.csr_f32_accum64(rp, col, val, x), rp, col, val, x, what=what)

    def identity(self, y_scaled, y_plain, rows=None, what=""):
        lo, hi = rows if rows is not None else (0, self.M)
        assert_same_numbers(y_scaled[lo:hi], scale_rows(y_plain[lo:hi], self.dr[lo:hi]), what)


def csr_maker(case, row0=0, row1=None):
    return lambda vals: sp.CsrDevice(case.M, case.N, case.rp, case.col, vals, row0, row1)


def hll_of(M, N, rp, col, val):
    r, c, v = coo_from_csr(rp, col, val)
    return sp.convert_to_hll(sp.PreMatrix.from_arrays(M, N, r, c, v))


def hll_maker(case, hack0=0, hack1=None):
    return lambda vals: sp.HllDevice(hll_of(case.M, case.N, case.rp, case.col, vals), hack0, hack1)


@contextlib.contextmanager
def pair(make, knobs):
    """(unscaled handle, scaled handle) under knobs; local_patterns pinned to 0 unless the knobs say 1."""
    knobs = dict(knobs)
    knobs.setdefault("local_patterns", 0)
    assert knobs["local_patterns"] in (0, 1)
    with sp.tuning(**knobs):
        with make("plain") as d0, make("scaled") as d1:
            i0, i1 = d0.info(), d1.info()
            assert plan(i0) == plan(i1), "the two handles of one structure report different plans"
            yield d0, d1, i1


def run(dev, x, variant):
    """One launch into a poisoned y (every row must be written)."""
    dev.set_x(x)
    item = 4 if getattr(dev, "dtype", F64) == F32 else 8
    sp.lib().spmv_hip_memset(dev.y_ptr, 0xFF, dev.M * item)
    dev.run(variant)
    return dev.get_y()


def check_spmv(oracle, case, make, knobs, fingerprint, variant, what, rows=None, launch_knobs=()):
    """(a) fingerprint, (b) row gate of the scaled handle, (c) identity against the unscaled handle; then every
    launch-time setting in launch_knobs must give the default launch's bits on the scaled handle."""
    vals = {"plain": case.val, "scaled": case.vs}
    with pair(lambda which: make(vals[which]), knobs) as (d0, d1, info):
        assert fingerprint(info), f"{what}: path not taken: {plan(info)}"
        y0, y1 = run(d0, case.x, variant), run(d1, case.xs, variant)
        case.gate(oracle, y1, case.xs, rows, what)
        case.identity(y1, y0, rows, what)
        for kv in launch_knobs:
            with sp.tuning(**kv):
                assert_same_numbers(run(d1, case.xs, variant)[slice(*(rows or (0, case.M)))],
                                    y1[slice(*(rows or (0, case.M)))], f"{what} {kv}")
        return info


# ------------------------------------------------------------------ structures
def with_rows(rng, rp, col, N, where, lengths):
    """Rows `where` replaced by rows of `lengths` distinct sorted columns."""
    lens = np.diff(rp).astype(np.int64)
    rows = [col[rp[r]:rp[r + 1]] for r in range(len(lens))]
    for r, n in zip(where, lengths):
        rows[r] = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
        lens[r] = n
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate(rows).astype(np.int32)


def scattered(rng, M, N, mean=None, sigma=None, lens=None):
    lens = rng.poisson(mean, M).astype(np.int64) if lens is None else np.asarray(lens, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.repeat(np.arange(M), lens)
    if sigma is None:
        col = rng.integers(0, N, rp[-1])
    else:
        col = np.clip(rows * (N - 1) // max(M - 1, 1) + np.rint(rng.normal(0, sigma, rp[-1])).astype(np.int64), 0, N - 1)
    return rp, col[np.lexsort((col, rows))].astype(np.int32)


def gather_rows(rng):
    """Scattered columns, rows longer than every stage (long-row pieces at every cap)."""
    M, N = 3000, 50000
    rp, col, _ = random_csr(rng, M, N, 30, 120, 0.05)
    rp, col = with_rows(rng, rp, col, N, [0, 7, 1500, 2998, 2999], [2047, 2049, 8193, 30000, 4097])
    return M, N, rp, col


def short_rows(rng):
    M, N = 20011, 300_000
    rp, col, _ = random_csr(rng, M, N, 3, 12, 0.1)
    return M, N, rp, col


def band(rng, M=5003, N=5600, mean=27, width=200, far=0.0):
    rp, col, _ = banded_csr(rng, M, N, mean, width, 0.02, far_frac=far)
    return M, N, rp, col


def skewed(rng):
    M, N = 6500, 3_000_000
    lens = np.minimum((1.08 / rng.random(M)).astype(np.int64), 60000)
    lens[rng.random(M) < 0.1] = 0
    lens[[11, 3000, 6499]] = [50000, 5000, 900]
    return (M, N) + scattered(rng, M, N, lens=lens)


def stray(rng, rp, col, N, frac):
    col = col.copy()
    s = rng.random(len(col)) < frac
    col[s] = rng.integers(0, N, int(s.sum()))
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return col[np.lexsort((col, rows))]


XCD = [{"stream_xcd": c} for c in (-1, 1, 3, 64)]


def xcd_blocks_ok(blocks):
    """The remap is exercised off the grid: a block count that is no multiple of 8 x chunk."""
    return all(blocks % (8 * c) for c in (1, 3, 64))


# ------------------------------------------------------------------ CSR explicit variants
@DTYPES
@pytest.mark.parametrize("vname", ["thread_row", "wave_row", "subwave"])
def test_csr_explicit_variants(gpu, oracle, dtype, vname):
    rng = np.random.default_rng(101)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, dtype)
    variant = sp.CSR_VARIANTS[vname]
    # (the explicit variants are launched by request; the handle is what the planner made of the matrix)
    check_spmv(oracle, case, csr_maker(case), {}, lambda i: i["value_bytes"] == np.dtype(dtype).itemsize and
               i["lanes_per_row"] >= 2 and i["long_rows"] > 0, variant, f"csr {vname}")


# ------------------------------------------------------------------ CSR stream kernels
@DTYPES
@pytest.mark.parametrize("cap", [2048, 4096, 8192])
def test_csr_stream_with_long_row_pieces(gpu, oracle, dtype, cap):
    rng = np.random.default_rng(102)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, dtype)
    lens = np.diff(rp)
    info = check_spmv(oracle, case, csr_maker(case), {"stream_cap": cap, "stream_local": 0, "stream_tile": 0},
                      lambda i: i["stream_kernel"] == 0 and i["long_rows"] == int((lens > cap - 3).sum()) > 0,
                      sp.CSR_STREAM, f"csr_stream cap={cap}",
                      launch_knobs=XCD + [{"stream_nt": 0}] if cap == 2048 else [{"stream_nt": 0}])
    if cap == 2048:
        assert xcd_blocks_ok(info["stream_blocks"]), info["stream_blocks"]


@DTYPES
def test_csr_stream_short(gpu, oracle, dtype):
    rng = np.random.default_rng(103)
    M, N, rp, col = short_rows(rng)
    case = Case(rng, M, N, rp, col, dtype)
    for cap in (2048, 4096):  # (the kernel's two stages)
        info = check_spmv(oracle, case, csr_maker(case), {"stream_cap": cap, "stream_local": 0, "stream_tile": 0},
                          lambda i: i["stream_kernel"] == 2 and i["local_blocks"] == 0, sp.CSR_STREAM,
                          f"csr_stream_short cap={cap}", launch_knobs=XCD + [{"stream_nt": 0}])
        if cap == 2048:
            assert xcd_blocks_ok(info["stream_blocks"]), info["stream_blocks"]


@DTYPES
@pytest.mark.parametrize("patterns", [0, 1])
@pytest.mark.parametrize("lcap", [1024, 2048, 3072])
def test_csr_stream_local(gpu, oracle, dtype, lcap, patterns):
    rng = np.random.default_rng(104 + lcap)
    M, N, rp, col = band(rng, far=0.05)
    case = Case(rng, M, N, rp, col, dtype)
    info = check_spmv(oracle, case, csr_maker(case), {"local_cap": lcap, "local_patterns": patterns},
                      lambda i: i["stream_kernel"] == 1 and i["local_blocks"] > 0 and (i["pattern_slots"] > 0) == bool(patterns),
                      sp.CSR_STREAM, f"csr_stream_local cap={lcap} patterns={patterns}",
                      launch_knobs=XCD + [{"local_nt": 0}, {"local_nt": 1}])
    if lcap == 2048:
        assert xcd_blocks_ok(info["local_blocks"]), info["local_blocks"]


# ------------------------------------------------------------------ csr_tile plans
def tile_cases(rng, dtype):
    M, N = 7001, 2_000_003
    yield ("gather passes", (M, N) + scattered(rng, M, N, 18), dict(stream_tile=1, tile_rows=1024, tile_expand=0),
           lambda i: i["stream_kernel"] == 3 and i["tile_staged_entries"] == 0 and i["tile_expanded_entries"] == 0,
           [{"tile_gather_ahead": 1}])
    M = 9001
    lens = rng.poisson(14, M)
    lens[::997] = 3000
    yield ("expanded x", (M, N) + scattered(rng, M, N, lens=lens),
           dict(stream_tile=1, tile_rows=1024, tile_expand=1, tile_lmax=4096, tile_density=0, tile_pack=0, stream_local=0),
           lambda i: i["stream_kernel"] == 3 and i["tile_expanded_entries"] >= i["tile_entries"] > 0, [])
    M = N = 60_000
    rp, col = scattered(rng, M, N, 9, sigma=2500)
    # (a packed plan stages every entry of its tiles; what sat in windows too sparse for a pass is its remainder)
    yield ("packed", (M, N, rp, col), dict(stream_tile=1, tile_rows=2048),
           lambda i: i["stream_kernel"] == 3 and i["tile_staged_entries"] + i["tile_remainder_entries"] == i["tile_entries"]
           and i["tile_staged_cols"] > 0 and i["tile_remainder_entries"] <= 0.01 * i["tile_entries"], [])
    yield ("remainder", (M, N, rp, stray(rng, rp, col, N, 0.004)), dict(stream_tile=1, tile_rows=2048),
           lambda i: i["stream_kernel"] == 3 and i["tile_remainder_entries"] > 0 and
           i["tile_staged_entries"] + i["tile_remainder_entries"] == i["tile_entries"], [])
    sk = skewed(rng)
    long_ok = lambda i: i["stream_kernel"] == 3 and i["tile_long_rows"] > 0 and i["tile_long_items"] > 0 and i["tile_split_rows"] == 0
    yield ("long-row tier", sk, dict(stream_tile=1, tile_rows=512, tile_lmax=700, tile_long=2), long_ok, [])
    for items in (8, 64):
        yield (f"long-row tier tile_items={items}", sk, dict(stream_tile=1, tile_rows=512, tile_lmax=700, tile_long=2,
                                                               tile_items=items), long_ok, [])
    yield ("split rows", sk, dict(stream_tile=1, tile_rows=512, tile_lmax=700, tile_long=0),
           lambda i: i["stream_kernel"] == 3 and i["tile_split_rows"] > 0 and i["tile_long_rows"] == 0, [])
    # the middle tier: 2^22 entries and more in rows of (48 | 128) < entries <= tile_lmax, scattered over 2^25 columns
    # (over 2 M columns the same rows fill their column slices: a packed plan, no tier)
    M, mean, N = (70_000, 80, 1 << 25) if dtype == F32 else (60_000, 150, 1 << 25)
    yield ("mid tier", (M, N) + scattered(rng, M, N, mean), dict(stream_tile=1),
           lambda i: i["stream_kernel"] == 3 and i["tile_mid_rows"] > 0 and i["tile_mid_entries"] >= 4 << 20, [])


TILE_IDS = ["gather passes", "expanded x", "packed", "remainder", "long-row tier", "long-row tier tile_items=8",
            "long-row tier tile_items=64", "split rows", "mid tier"]


@DTYPES
@pytest.mark.parametrize("which", TILE_IDS)
def test_csr_tile_plans(gpu, oracle, dtype, which):
    rng = np.random.default_rng(105)
    for what, (M, N, rp, col), knobs, fingerprint, launch in tile_cases(rng, dtype):
        if what != which:
            continue
        case = Case(rng, M, N, rp, col, dtype)
        check_spmv(oracle, case, csr_maker(case), knobs, fingerprint, sp.CSR_STREAM, f"csr_tile {what}",
                   launch_knobs=launch)
        return
    raise AssertionError(which)


# ------------------------------------------------------------------ CSR handle shapes
@DTYPES
@pytest.mark.parametrize("skew", [1, 0])
def test_csr_skew_row_split(gpu, oracle, dtype, skew):
    rng = np.random.default_rng(106)
    M, N = 200_000, 1_000_000
    lens = rng.poisson(5.5, M).astype(np.int64)
    lens[rng.choice(M, 60, replace=False)] = 1000
    rp, col = scattered(rng, M, N, lens=lens)
    assert rp[-1] >= 1 << 20
    case = Case(rng, M, N, rp, col, dtype)
    limit = max(128, 16 * (int(rp[-1]) // M))
    expect = int((lens > limit).sum()) if skew else 0
    check_spmv(oracle, case, csr_maker(case), {"skew_rows": skew, "stream_local": 0, "stream_tile": 0},
               lambda i: i["local_blocks"] == 0 and i["tile_blocks"] == 0 and i["long_rows"] == expect,
               sp.CSR_STREAM, f"skew_rows={skew}")


@DTYPES
def test_csr_row_block_handle(gpu, oracle, dtype):
    rng = np.random.default_rng(107)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, dtype)
    check_spmv(oracle, case, csr_maker(case, 1000, 2999), {"stream_local": 0, "stream_tile": 0},
               lambda i: (i["row0"], i["M_local"]) == (1000, 1999) and i["long_rows"] > 0, sp.CSR_STREAM,
               "row block", rows=(1000, 2999))


@DTYPES
def test_csr_run_part_and_run_split(gpu, oracle, dtype):
    rng = np.random.default_rng(108)
    n = 30000
    _, _, rp, col = band(rng, n, n, 22, 150)
    case = Case(rng, n, n, rp, col, dtype)
    bounds = sp.partition_rows(rp, 3)
    lo, hi = int(bounds[1]), int(bounds[2])
    vals = {"plain": case.val, "scaled": case.vs}
    with pair(lambda which: sp.CsrDevice(n, n, rp, col, vals[which], lo, hi), {}) as (d0, d1, info):
        assert info["local_blocks"] > 0
        counts = [d.split_interior() for d in (d0, d1)]
        assert counts[0] == counts[1] and counts[1]["interior_blocks"] > 0 and counts[1]["boundary_blocks"] > 0
        splits = [d.split_columns(lo, hi) for d in (d0, d1)]
        assert splits[0] == splits[1] and splits[1]["halo_entries"] > 0
        ys = {}
        for name, parts in (("run_part", lambda d: (d.run_part(0), d.run_part(1))),
                            ("run_split", lambda d: (d.run_split(0), d.run_split(1)))):
            for d, x, key in ((d0, case.x, "plain"), (d1, case.xs, "scaled")):
                d.set_x(x)
                sp.lib().spmv_hip_memset(d.y_ptr, 0xFF, n * np.dtype(dtype).itemsize)
                parts(d)
                sp.hip_sync()
                ys[key] = d.get_y()
            case.gate(oracle, ys["scaled"], case.xs, (lo, hi), name)
            case.identity(ys["scaled"], ys["plain"], (lo, hi), name)


# ------------------------------------------------------------------ HLL (fp64)
@pytest.mark.parametrize("vname", ["thread_row", "subwave"])
def test_hll_explicit_variants(gpu, oracle, vname):
    rng = np.random.default_rng(109)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, F64)
    check_spmv(oracle, case, hll_maker(case), {}, lambda i: i["hacks"] == (M + 31) // 32,
               sp.HLL_VARIANTS[vname], f"hll {vname}")


def test_hll_lds(gpu, oracle):
    rng = np.random.default_rng(110)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, F64)
    check_spmv(oracle, case, hll_maker(case), {"stream_local": 0, "stream_tile": 0},
               lambda i: i["stream_kernel"] == 0 and i["local_blocks"] == 0 and i["tile_blocks"] == 0, sp.HLL_LDS, "hll_lds")


@pytest.mark.parametrize("patterns", [0, 1])
def test_hll_lds_local(gpu, oracle, patterns):
    rng = np.random.default_rng(111)
    M, N, rp, col = band(rng, 4099, 4500, 27, 200)
    case = Case(rng, M, N, rp, col, F64)
    info = check_spmv(oracle, case, hll_maker(case), {"local_patterns": patterns},
                      lambda i: i["stream_kernel"] == 1 and i["local_blocks"] > 0 and (i["pattern_slots"] > 0) == bool(patterns),
                      sp.HLL_LDS, f"hll_lds_local patterns={patterns}",
                      launch_knobs=XCD + [{"local_nt": 0}, {"local_nt": 1}])
    assert xcd_blocks_ok(info["local_blocks"]), info["local_blocks"]


def test_hll_tile_kernel_over_the_slab(gpu, oracle):
    rng = np.random.default_rng(112)
    M, N = 9001, 1_500_000
    rp, col = scattered(rng, M, N, 16)
    case = Case(rng, M, N, rp, col, F64)
    check_spmv(oracle, case, hll_maker(case), {"stream_tile": 1, "tile_rows": 1024, "stream_local": 0},
               lambda i: i["stream_kernel"] == 2 and i["tile_entries"] + i["tile_long_entries"] == i["slots"], sp.HLL_LDS,
               "hll tiles")


def test_hll_hack_range_and_device_built_slab(gpu, oracle):
    rng = np.random.default_rng(113)
    M, N, rp, col = band(rng, 4099, 4500, 27, 200, far=0.05)
    case = Case(rng, M, N, rp, col, F64)
    hb = sp.partition_hacks(hll_of(M, N, rp, col, case.val), 3)
    rb = sp.hack_bounds_to_rows(hb, M)
    lo, hi = int(rb[1]), int(rb[2])
    check_spmv(oracle, case, hll_maker(case, int(hb[1]), int(hb[2])), {},
               lambda i: (i["row0"], i["M_local"]) == (lo, hi - lo), sp.HLL_AUTO, "hll hack range", rows=(lo, hi))
    vals = {"plain": case.val, "scaled": case.vs}

    @contextlib.contextmanager
    def built(which):
        with sp.CsrDevice(M, N, rp, col, vals[which]) as c, sp.HllDevice.from_csr_device(c) as h:
            yield h

    check_spmv(oracle, case, lambda v: built("plain" if v is case.val else "scaled"), {},
               lambda i: i["hacks"] == (M + 31) // 32 and i["local_blocks"] > 0, sp.HLL_AUTO, "hll device-built slab")


# ------------------------------------------------------------------ SpMM
KS = (2, 3, 4, 5, 8, 9, 16, 17, 33, 64)


class DeviceBuffer:
    def __init__(self, nbytes):
        self.p = C.c_void_p()
        assert sp.lib().spmv_hip_malloc(C.byref(self.p), int(nbytes)) == 0
        self.nbytes = int(nbytes)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        sp.lib().spmv_hip_free(self.p)

    def upload(self, a, offset):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        assert sp.lib().spmv_hip_memcpy_h2d(C.c_void_p(self.p.value + offset), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def download(self, shape, dtype, offset):
        sp.hip_sync()
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        assert sp.lib().spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.p.value + offset), out.nbytes) == 0
        return out


def check_spmm(oracle, rng, case, make, knobs, fingerprint, ks, what, offset_path=False):
    vals = {"plain": case.val, "scaled": case.vs}
    with pair(lambda which: make(vals[which]), knobs) as (d0, d1, info):
        assert fingerprint(info), f"{what}: path not taken: {plan(info)}"
        for k in ks:
            X = wide_range(rng, case.N * k, case.dtype).reshape(case.N, k)
            Xs = (X.astype(np.float64) * case.dc[:, None]).astype(case.dtype)
            Y0, Y1 = d0.spmm(X), d1.spmm(Xs)
            for j in range(k):
                case.gate(oracle, Y1[:, j], np.ascontiguousarray(Xs[:, j]), what=f"{what} k={k} column {j}")
            case.identity(Y1, Y0, what=f"{what} k={k}")
            perm = rng.permutation(k)
            assert_same_numbers(d1.spmm(np.ascontiguousarray(Xs[:, perm])), Y1[:, perm], f"{what} k={k} permuted columns")
            Yd = d1.spmm(np.ascontiguousarray(np.repeat(Xs[:, :1], k, axis=1)))
            for j in range(k):
                assert_same_numbers(Yd[:, j], Y1[:, 0], f"{what} k={k} identical columns, column {j}")
            if offset_path:   # X and Y 8 bytes off a 16-byte boundary: the element loads, the same bits
                item = np.dtype(case.dtype).itemsize
                with DeviceBuffer(case.N * k * item + 16) as dx, DeviceBuffer(case.M * k * item + 16) as dy:
                    dx.upload(Xs, 8)
                    assert sp.lib().spmv_hip_memset(dy.p, 0xFF, dy.nbytes) == 0
                    d1.spmm_on(dx.p.value + 8, dy.p.value + 8, k)
                    assert_same_numbers(dy.download((case.M, k), case.dtype, 8), Y1, f"{what} k={k} X / Y at offset 8")


@DTYPES
def test_csr_spmm_every_k_with_long_rows(gpu, oracle, dtype):
    rng = np.random.default_rng(114)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, dtype)
    check_spmm(oracle, rng, case, csr_maker(case), {}, lambda i: i["long_rows"] > 0, KS, f"csr spmm {np.dtype(dtype).name}",
               offset_path=True)


def test_hll_spmm_every_k_with_long_windows(gpu, oracle):
    rng = np.random.default_rng(115)
    M, N, rp, col = gather_rows(rng)
    case = Case(rng, M, N, rp, col, F64)
    hll = hll_of(M, N, rp, col, case.val)
    # rows of 4097 .. 30000 entries: one-row windows longer than the 2048-slot stage, hll_spmm_row's share (the info
    # block does not list those windows: the slab's widths show they exist)
    with sp.HllDevice(hll) as h:
        _, maxnz, _, _ = h.download()
        assert maxnz.max() > 2048
    check_spmm(oracle, rng, case, hll_maker(case), {}, lambda i: i["hacks"] == (M + 31) // 32, KS, "hll spmm",
               offset_path=True)


# ------------------------------------------------------------------ full size
def test_full_size_nlpkkt_like_every_row(gpu, oracle):
    """The identity and the row gate on every row of the nlpkkt-like matrix (3.5 M rows, ~98 M entries): CSR AUTO,
    the slab built from it on the device, and one SpMM at k = 8."""
    from sparsematrixvectormultiplication_amd import synth
    M, rp, col, _ = synth.kkt_like()
    rng = np.random.default_rng(116)
    case = Case(rng, M, M, rp, col, F64)
    vals = {"plain": case.val, "scaled": case.vs}
    with pair(lambda which: sp.CsrDevice(M, M, rp, col, vals[which]), {}) as (d0, d1, info):
        assert info["stream_kernel"] == 1 and info["local_blocks"] > 0
        y0, y1 = run(d0, case.x, sp.CSR_AUTO), run(d1, case.xs, sp.CSR_AUTO)
        case.gate(oracle, y1, case.xs, what="nlpkkt-like csr")
        case.identity(y1, y0, what="nlpkkt-like csr")
        with sp.HllDevice.from_csr_device(d0) as h0, sp.HllDevice.from_csr_device(d1) as h1:
            assert plan(h0.info()) == plan(h1.info()) and h1.info()["slots"] >= rp[-1]
            yh0, yh1 = run(h0, case.x, sp.HLL_AUTO), run(h1, case.xs, sp.HLL_AUTO)
            case.gate(oracle, yh1, case.xs, what="nlpkkt-like hll")
            case.identity(yh1, yh0, what="nlpkkt-like hll")
        X = wide_range(rng, M * 8, F64).reshape(M, 8)
        Xs = X * case.dc[:, None]
        Y0, Y1 = d0.spmm(X), d1.spmm(Xs)
        case.identity(Y1, Y0, what="nlpkkt-like spmm k=8")
        for j in (0, 7):
            case.gate(oracle, Y1[:, j], np.ascontiguousarray(Xs[:, j]), what=f"nlpkkt-like spmm column {j}")


def test_full_size_powerlaw_fp32_every_row(gpu, oracle):
    """The identity and the row gate on every row of the config-5 power-law matrix (2^24 rows, 2.6e8 entries, fp32):
    long-row tier, middle tier, ordinary tiles."""
    from sparsematrixvectormultiplication_amd import synth
    n, rp, col, _ = synth.powerlaw()
    rng = np.random.default_rng(117)
    case = Case(rng, n, n, rp, col, F32)
    vals = {"plain": case.val, "scaled": case.vs}
    with pair(lambda which: sp.CsrDevice(n, n, rp, col, vals[which]), {}) as (d0, d1, info):
        assert info["stream_kernel"] == 3 and info["tile_long_rows"] > 1000 and info["tile_mid_rows"] > 1e5
        assert info["tile_entries"] + info["tile_long_entries"] + info["tile_mid_entries"] == info["nz"]
        y0, y1 = run(d0, case.x, sp.CSR_AUTO), run(d1, case.xs, sp.CSR_AUTO)
        case.identity(y1, y0, what="powerlaw fp32")
        # the same plan through its gather passes (no expanded x), plain and gathering one pass early: the same bits,
        # from the instantiations with the streamed-once hint that only a handle of this size launches
        for kv in ({"tile_expand": 0}, {"tile_expand": 0, "tile_gather_ahead": 1}):
            with sp.tuning(**kv):
                assert_same_numbers(run(d1, case.xs, sp.CSR_AUTO), y1, f"powerlaw fp32 {kv}")
    case.gate(oracle, y1, case.xs, what="powerlaw fp32")
