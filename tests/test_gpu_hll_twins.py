"""HLL handles built on the device against an upload of the same slab.

spmv_hip_hll_upload_part packs the host hacks and uploads them; spmv_hip_hll_from_csr fills the slab on the device from
a resident CSR matrix.  Both then go through hll_finish_handle (spmv_hll.hip) with a source that says where JA / AS are,
and a host builder (x-window plan, tile plan) copies the slab back only for the second.  Here, for each target,
sp.HllDevice(hll) is held to its TWIN sp.HllDevice.from_csr_device(sp.CsrDevice(...)) under the same knobs:

  1. download() -- hack offsets, row lengths, JA, AS -- is equal bit for bit;
  2. info() is equal on every key but the six that hold a time or an address, and tile_digest() is equal;
  3. every HLL variant and spmm (k = 3) on a uniform and a wide-range x, y pre-filled with 0xFF: the twin's bytes, and
     inside assert_parity against the oracle (which catches both handles being wrong alike).

All under local_patterns = 1, place_tries = 0: the only two upload decisions that are timed (upload_searches,
upload_ops.hpp) are then not taken, and nothing compared depends on a clock.

The targets, each the smallest that reaches its branch of hll_finish_handle, the branch asserted from info():
  H1 a band of 20 000 rows: the x-window plan, built on the device -- and under plan_on_device = 0 by the host builder
     (from_csr_device: on JA copied back);
  H2 a band in which 256 rows hold a dozen columns anywhere: the 2048-slot windows over them list more than 256 lines, the
     device builder declines and the host builder cuts windows by lines -- the handle then has MORE x-window windows than
     the plain cut at 2048 slots, which the device builder cannot produce (hll_plan_check, on the host);
  H3 scattered columns (test_gpu_tile.py's HLL case): the tile plan over the slab's rows, by host threads (from_csr_device:
     on JA and AS copied back) and by the device builder;
  H4 neither plan: the lane-group kernel;
  H5 a row longer than the stage: one-row windows (SpMM's long_windows), no x-window plan;
  H6 edges: no entries, 1 x 1, 33 rows (a last hack of one row), and a row block cut on hack boundaries against
     HllDevice(hll, hack0, hack1)."""
import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import assert_parity, banded_csr, coo_from_csr, random_csr, wide_range
from test_gpu_tile import scattered

pytestmark = pytest.mark.gpu

# info() keys that hold a time or an address
TIMED = ("place_tries", "place_first_us", "place_best_us", "val_address", "pattern_with_us", "pattern_without_us")
PINNED = dict(local_patterns=1, place_tries=0)
HACK = 32
VARIANTS = dict(sp.HLL_VARIANTS, auto=sp.HLL_AUTO)


# ---------------------------------------------------------------- targets
def with_rows(rp, col, val, new_rows, rng):
    """The matrix with row r replaced by the sorted columns new_rows[r]"""
    lens = np.diff(rp).astype(np.int64)
    for r, c in new_rows.items():
        lens[r] = len(c)
    out = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ncol, nval = np.empty(out[-1], dtype=np.int32), np.empty(out[-1], dtype=val.dtype)
    for r in range(len(rp) - 1):
        if r in new_rows:
            ncol[out[r]:out[r + 1]] = new_rows[r]
            nval[out[r]:out[r + 1]] = rng.uniform(-1, 1, lens[r])
        else:
            ncol[out[r]:out[r + 1]] = col[rp[r]:rp[r + 1]]
            nval[out[r]:out[r + 1]] = val[rp[r]:rp[r + 1]]
    return out, ncol, nval


def h1():
    return (20_000, 20_000) + banded_csr(np.random.default_rng(201), 20_000, 20_000, 9, 150)


H2_WIDE = range(8000, 8256)


def h2():
    rng = np.random.default_rng(202)
    M, N = 20_000, 200_000
    rp, col, val = banded_csr(rng, M, N, 9, 150)
    wide = {r: np.sort(rng.choice(N, 12, replace=False)).astype(np.int32) for r in H2_WIDE}
    return (M, N) + with_rows(rp, col, val, wide, rng)


def h3():
    return (9001, 1_500_000) + scattered(np.random.default_rng(29), 9001, 1_500_000, 16)


def h4():
    return (6000, 60_000) + random_csr(np.random.default_rng(204), 6000, 60_000, 8)


H5_LONG = 3000


def h5():
    rng = np.random.default_rng(205)
    M = N = 4000
    rp, col, val = banded_csr(rng, M, N, 9, 150)
    return (M, N) + with_rows(rp, col, val, {M // 2: np.sort(rng.choice(N, H5_LONG, replace=False)).astype(np.int32)}, rng)


def h6_empty():
    return 5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0)


def h6_one():
    return 1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([-0.75])


def h6_33_rows():
    return (33, 40) + random_csr(np.random.default_rng(206), 33, 40, 5)


def h6_rows():
    return (1000, 1000) + banded_csr(np.random.default_rng(207), 1000, 1000, 7, 40)


def x_window(info, hll):
    assert info["local_blocks"] > 0 and info["stream_kernel"] == 1 and info["pattern_slots"] > 0, info


def branch_h2(info, hll):
    x_window(info, hll)
    stats = sp.hll_plan_check(hll)
    # windows of the cut at 2048 slots; of the host builder's plan
    assert stats["local_windows"] > stats["gather_windows"] and info["local_blocks"] == stats["local_windows"], (stats, info)


def branch_h3(info, hll):
    assert info["stream_kernel"] == 2 and info["local_blocks"] == 0 and info["tile_blocks"] > 0, info


def branch_h4(info, hll):
    assert info["local_blocks"] == 0 and info["tile_blocks"] == 0 and info["auto_variant"] == sp.HLL_SUBWAVE, info


def branch_h5(info, hll):
    assert info["local_blocks"] == 0 and info["tile_blocks"] == 0 and info["auto_variant"] == sp.HLL_LDS, info
    # (the hack of the long row: 32 rows of H5_LONG slots, each a window of its own, longer than the stage of 2048 slots)
    assert H5_LONG > 2048 and info["slots"] >= HACK * H5_LONG and info["stream_blocks"] >= sp.hll_plan_check(hll)["gather_windows"], info


def branch_none(info, hll):
    assert info["tile_blocks"] == 0, info


TILES = dict(stream_tile=1, tile_rows=1024, stream_local=0)
# name: (target, the knobs that lead to its branch, the branch, hacks [hack0, hack1) of a row block or None)
CASES = {
    "H1": (h1, {}, x_window, None),
    "H1-host-plan": (h1, dict(plan_on_device=0), x_window, None),
    "H2": (h2, {}, branch_h2, None),
    "H3-host-tiles": (h3, dict(TILES, tile_plan_on_device=0), branch_h3, None),
    "H3-device-tiles": (h3, dict(TILES, tile_plan_on_device=1), branch_h3, None),
    "H4": (h4, {}, branch_h4, None),
    "H5": (h5, {}, branch_h5, None),
    "H6-empty": (h6_empty, {}, branch_none, None),
    "H6-1x1": (h6_one, {}, branch_none, None),
    "H6-33-rows": (h6_33_rows, {}, branch_none, None),
    "H6-row-block": (h6_rows, {}, branch_none, (7, 19)),
    "H6-last-rows": (h6_rows, {}, branch_none, (19, 32)),     # 1000 rows: the last hack holds 8
}

_TARGETS = {}


def target_of(case, oracle):
    """(M, N, rp, col, val, the host HLL matrix, x list, their oracle products, X of 3 columns and its products): once
    per generator"""
    make = CASES[case][0]
    if make not in _TARGETS:
        M, N, rp, col, val = make()
        rng = np.random.default_rng(7 * M + N)
        hll = sp.convert_to_hll(sp.PreMatrix.from_arrays(M, N, *coo_from_csr(rp, col, val)))
        xs = [rng.uniform(-1, 1, N), wide_range(rng, N, np.float64)]
        X3 = rng.uniform(-1, 1, (N, 3))
        _TARGETS[make] = (M, N, rp, col, val, hll, xs, [oracle.csr_serial(rp, col, val, x) for x in xs], X3,
                          [oracle.csr_serial(rp, col, val, np.ascontiguousarray(X3[:, j])) for j in range(3)])
    return _TARGETS[make]


# ---------------------------------------------------------------- the twin check
def launched(dev, x, variant):
    """y of the variant on x, every byte of y set before the launch"""
    assert sp.lib().spmv_hip_memset(dev.y_ptr, 0xFF, dev.M * 8) == 0
    dev.set_x(x)
    dev.run(variant)
    sp.hip_sync()
    return dev.get_y()


def observe(dev, xs, X3):
    """Everything that is compared between a handle and its twin"""
    seen = {"info": {k: v for k, v in dev.info().items() if k not in TIMED}, "tile_digest": dev.tile_digest()}
    for name, part in zip(("hack_off", "maxnz", "JA", "AS"), dev.download()):
        seen[name] = part
    for name, variant in VARIANTS.items():
        for k, x in enumerate(xs):
            seen[f"y {name} x{k}"] = launched(dev, x, variant)
    seen["spmm"] = dev.spmm(X3)
    return seen


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@pytest.mark.parametrize("case", list(CASES))
def test_device_built_slab_is_its_uploaded_twin(gpu, oracle, case):
    _, knobs, branch, hacks = CASES[case]
    M, N, rp, col, val, hll, xs, refs, X3, refs3 = target_of(case, oracle)
    h0, h1 = hacks or (0, hll.num_blocks)
    r0, r1 = min(h0 * HACK, M), min(h1 * HACK, M)
    with sp.tuning(**PINNED, **knobs):
        with sp.HllDevice(hll, h0, h1) as up:
            mine = observe(up, xs, X3)
            branch(mine["info"], hll)
        with sp.CsrDevice(M, N, rp, col, val, row0=r0, row1=r1) as csr:
            with sp.HllDevice.from_csr_device(csr) as built:
                twin = observe(built, xs, X3)
    assert mine.keys() == twin.keys()
    for key in mine:
        if key == "info":
            diff = {k: (mine[key][k], twin[key][k]) for k in mine[key] if mine[key][k] != twin[key][k]}
            assert not diff, f"{case}: info differs: {diff}"
        else:
            assert same(mine[key], twin[key]), f"{case}: {key} differs between the uploaded and the device-built handle"
    # ... and both right: the handle's rows against the oracle (the rest of y is as it was)
    block = (rp[r0:r1 + 1] - rp[r0], col[rp[r0]:rp[r1]], val[rp[r0]:rp[r1]])
    for name in VARIANTS:
        for k, x in enumerate(xs):
            y = mine[f"y {name} x{k}"]
            assert_parity(y[r0:r1], refs[k][r0:r1], *block, x, what=f"{case} {name} x{k}")
            assert np.all(y[:r0].view(np.uint64) == 0xFFFFFFFFFFFFFFFF) and np.all(y[r1:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF), \
                f"{case} {name} x{k}: rows outside the handle's were written"
    for j in range(3):
        yj = np.ascontiguousarray(mine["spmm"][:, j])
        assert_parity(yj[r0:r1], refs3[j][r0:r1], *block, np.ascontiguousarray(X3[:, j]), what=f"{case} spmm column {j}")
        assert not yj[:r0].any() and not yj[r1:].any(), f"{case} spmm column {j}: rows outside the handle's are not zero"
