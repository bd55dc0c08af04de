"""CsrDevice.update_values: after the call a handle is the upload of (its pattern, the new values) under the plan it has.

test_gpu_adopted_handles.py pins "a handle is the upload of its arrays" for every branch of the upload (T1 .. T9, each the
smallest that reaches its branch) and for every producer that builds a handle on the device.  Here the producer is an
UPDATE: the target's pattern is uploaded with OTHER values (a second draw, some of them exact zeros, some the target's
with the sign flipped) under the case's knobs, the branch is asserted from info(), update_values(target values) follows
-- from a host array, or from a device buffer through update_values_on -- and the handle is held to the twin with
assert_twin: download(), info(), tile_digest(), the x-window arrays, the zero pads, every variant's bytes, SpMM, the HLL
conversion, run_part and the column split.  info() and addresses() are the same before and after.

More targets, each asserted from info(): the middle tile tier (test_gpu_tile.py's generator and knobs; for its size the
plan, the arrays, the pads and every variant's bytes only); rows whose entries are shuffled and repeat (row, column)
pairs -- scattered() as it comes -- under the x-window knobs, under the tile knobs with a packed plan and with gather
passes, and a band with stray entries, whose packed plan keeps a remainder.

Then: A -> B -> A, the same update twice, two row-range handles that stitch, the transpose of an updated handle, solver
steps on one, update_info()'s counter, and the refusals, after each of which the handle still works and still updates."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import assert_parity, assert_parity_f32, wide_range
from test_gpu_adopted_handles import (CASES, DTYPES, PINNED, TIMED, assert_twin, inputs_of, launched, observe, same_results,
                                      spd_target, target_of, twin_of)
from test_gpu_tile import scattered
from test_gpu_transpose import transpose_ref

pytestmark = pytest.mark.gpu

SOURCES = ["host", "device"]


def other_values(val, seed):
    """a second draw on the same pattern: some exact zeros, some of the target's values with the sign flipped"""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-1, 1, len(val)).astype(val.dtype)
    pick = rng.random(len(val))
    out[pick < 0.05] = 0
    flip = pick > 0.8
    out[flip] = -val[flip]
    return out


@contextlib.contextmanager
def device_copy(a):
    """the address of a device buffer that holds a's bytes"""
    L, p = sp.lib(), C.c_void_p()
    a = np.ascontiguousarray(a)
    assert L.spmv_hip_malloc(C.byref(p), max(a.nbytes, 16)) == 0
    try:
        if a.nbytes:
            assert L.spmv_hip_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        yield p.value
    finally:
        sp.hip_sync()
        assert L.spmv_hip_free(p) == 0


def update(h, val, source):
    if source == "host":
        h.update_values(val)
    else:
        with device_copy(val) as d_val:
            h.update_values_on(d_val)


@contextlib.contextmanager
def updated(tgt, knobs, branch, pinned, source, seed=1):
    """The target's pattern uploaded with other values under knobs, then updated to the target's; info() and addresses()
    must not move.  The knobs stay in force for what the caller does with the handle."""
    M, N, rp, col, val = tgt
    with sp.tuning(**knobs):
        with sp.CsrDevice(M, N, rp, col, other_values(val, seed)) as h:
            info, adr = h.info(), h.addresses()
            branch(info, pinned)
            update(h, val, source)
            assert h.info() == info, "info() changed with the update"
            assert h.addresses() == adr, "addresses() changed with the update: val is written in place, never swapped"
            yield h


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_updated_handle_is_the_upload_of_the_new_values(gpu, oracle, case, dtype, source):
    tgt = target_of(case, dtype)
    xs, y_refs, X3 = inputs_of(case, dtype, oracle)
    twin_seen = twin_of(case, dtype, oracle, True)
    with updated(tgt, dict(CASES[case][1], **PINNED), CASES[case][2], True, source) as h:
        assert_twin(h, tgt, xs, f"{case} update from the {source} {np.dtype(dtype).name}", oracle, y_refs, X3, twin_seen)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_updated_handle_under_the_default_knobs(gpu, oracle, case, dtype):
    """the searches left on: the arrays, the pads and the bits only (a placement moves none, and the update keeps it)"""
    tgt = target_of(case, dtype)
    xs, y_refs, X3 = inputs_of(case, dtype, oracle)
    twin_seen = twin_of(case, dtype, oracle, False)
    with updated(tgt, CASES[case][1], CASES[case][2], False, "host") as h:
        assert_twin(h, tgt, xs, f"{case} update {np.dtype(dtype).name}, default knobs", oracle, y_refs, X3, twin_seen, full=False)


# ---------------------------------------------------------------- more targets
def shuffled_rows(rng, rp, col, val):
    """every row's entries in a random order"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    order = np.lexsort((rng.random(len(col)), rows))
    return rp, col[order], val[order]


def repeats_of(rp, col):
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return len(col) - len(np.unique(rows * (int(col.max()) + 1) + col))


def dup_band():
    """a narrow band, a dozen entries per row: two in five rows repeat a pair; rows shuffled"""
    rng = np.random.default_rng(201)
    M = N = 20_000
    tgt = (M, N) + shuffled_rows(rng, *scattered(rng, M, N, 12, sigma=40))
    assert repeats_of(tgt[2], tgt[3]) > 1000 and np.any(np.diff(tgt[3])[:2000] < 0)
    return tgt


def dup_tiles():
    rng = np.random.default_rng(202)
    M, N = 3000, 50_000
    tgt = (M, N) + shuffled_rows(rng, *scattered(rng, M, N, 12, sigma=40))
    assert repeats_of(tgt[2], tgt[3]) > 100
    return tgt


def dup_band_with_strays():
    """test_gpu_tile.py's "band + stray entries", as scattered() makes it (repeats kept) and with its rows shuffled"""
    rng = np.random.default_rng(203)
    M = N = 60_000
    rp, col, val = scattered(rng, M, N, 9, sigma=2500)
    stray = rng.random(rp[-1]) < 0.004
    col = col.copy()
    col[stray] = rng.integers(0, N, int(stray.sum()))
    return (M, N) + shuffled_rows(rng, rp, col, val)


def branch_x_window(info, pinned):
    assert info["local_blocks"] > 0 and info["stream_kernel"] == 1, info


def branch_packed_tiles(info, pinned):
    assert info["stream_kernel"] == 3 and info["tile_blocks"] > 0 and info["tile_staged_entries"] == info["tile_entries"] > 0, info


def branch_gather_tiles(info, pinned):
    assert info["stream_kernel"] == 3 and info["tile_blocks"] > 0 and info["tile_entries"] > 0, info


def branch_remainder(info, pinned):
    assert info["stream_kernel"] == 3 and info["tile_remainder_entries"] > 0, info


TILE_SMALL = dict(stream_tile=1, tile_rows=256, stream_local=0)
# name: (target, the knobs that lead to its branch, the branch)
MORE = {
    "repeats, x-window": (dup_band, {}, branch_x_window),
    "repeats, packed tiles": (dup_tiles, TILE_SMALL, branch_packed_tiles),
    "repeats, gather passes": (dup_tiles, dict(TILE_SMALL, tile_pack=0), branch_gather_tiles),
    "repeats, remainder": (dup_band_with_strays, dict(stream_tile=1, tile_rows=2048, stream_local=0), branch_remainder),
}
_MORE_TARGETS = {}


def more_target(name, dtype):
    make = MORE[name][0]
    if make not in _MORE_TARGETS:
        _MORE_TARGETS[make] = make()
    M, N, rp, col, val = _MORE_TARGETS[make]
    return M, N, rp, col, val.astype(dtype)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MORE))
def test_update_of_unsorted_rows_with_repeats(gpu, oracle, name, dtype, source):
    """Repeats keep the order the plan gave them: the sums round as the twin's do, and the digest is the twin's."""
    tgt = more_target(name, dtype)
    M, N, rp, col, val = tgt
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, N).astype(dtype), wide_range(rng, N, dtype)]
    ref = oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64
    y_refs = [ref(rp, col, val, x) for x in xs]
    _, knobs, branch = MORE[name]
    with updated(tgt, dict(knobs, **PINNED), branch, True, source) as h:
        assert_twin(h, tgt, xs, f"{name} update from the {source} {np.dtype(dtype).name}", oracle, y_refs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_update_of_the_middle_tile_tier(gpu, dtype):
    """test_gpu_tile.py's "mid tier" (the smallest that puts 2^22 entries into the tier's rows; 2^25 columns): for its
    size the plan (info, digest), the arrays, the pads and every variant's bytes on one x"""
    rng = np.random.default_rng(72)
    M, mean, N = (70_000, 80, 1 << 25) if dtype == np.float32 else (60_000, 150, 1 << 25)
    tgt = (M, N) + scattered(rng, M, N, mean, dtype=dtype)
    xs = [rng.uniform(-1, 1, N).astype(dtype)]

    def branch(info, pinned):
        assert info["stream_kernel"] == 3 and info["tile_mid_rows"] > 0 and info["tile_mid_entries"] >= 1 << 22, info

    knobs = dict(stream_tile=1, **PINNED)
    with sp.tuning(**knobs):
        with sp.CsrDevice(*tgt) as twin:
            twin_seen = observe(twin, tgt, xs, None, False)
            twin_plan = ({k: v for k, v in twin.info().items() if k not in TIMED}, twin.tile_digest())
    with updated(tgt, knobs, branch, True, "device") as h:
        assert ({k: v for k, v in h.info().items() if k not in TIMED}, h.tile_digest()) == twin_plan
        assert h.update_info()["map_bytes"] >= 4 * h.info()["tile_mid_entries"]
        assert_twin(h, tgt, xs, f"mid tier {np.dtype(dtype).name}", twin_seen=twin_seen, full=False)


# ---------------------------------------------------------------- further checks
def snapshot(h, xs):
    """what two states of ONE handle are compared by: the values, the tile plans' arrays, AUTO and STREAM on xs"""
    out = {"val": h.download()[2], "digest": h.tile_digest()}
    for k, x in enumerate(xs):
        for name in ("auto", "stream"):
            variant = sp.CSR_AUTO if name == "auto" else sp.CSR_STREAM
            out[f"y {name} x{k}"] = launched(h, x, lambda: h.run(variant))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["T1", "T3", "T4-device-tiles", "T5", "T6", "T7"])
def test_update_there_and_back_and_twice(gpu, oracle, case, dtype):
    """A -> B -> A gives the first bytes; two updates with the same values give the same bytes; val stays where it is;
    update_info() counts, and only a handle with tile plans keeps maps"""
    M, N, rp, col, A = target_of(case, dtype)
    xs = inputs_of(case, dtype, oracle)[0]
    B = other_values(A, 9)
    with sp.tuning(**CASES[case][1], **PINNED):
        with sp.CsrDevice(M, N, rp, col, A) as h:
            assert h.update_info() == {"updates": 0, "map_bytes": 0, "map_build_us": 0.0, "last_us": 0.0}
            bytes_before = h.info()["device_bytes"]
            first, where = snapshot(h, xs), h.addresses()["val"]
            h.update_values(B)
            at_b = snapshot(h, xs)
            assert at_b["val"].tobytes() == B.tobytes()
            if np.any(first["y auto x0"] != 0):
                assert at_b["y auto x0"].tobytes() != first["y auto x0"].tobytes(), "the update changed nothing"
            h.update_values(B)
            same_results(snapshot(h, xs), at_b, f"{case}: the same update twice")
            with device_copy(A) as d_a:
                h.update_values_on(d_a)
            same_results(snapshot(h, xs), first, f"{case}: A -> B -> A")
            assert h.addresses()["val"] == where
            ui, info = h.update_info(), h.info()
            assert ui["updates"] == 3 and ui["last_us"] > 0, ui
            assert info["device_bytes"] == bytes_before, "info() does not count the update's maps"
            if info["tile_blocks"] > 0:
                slots = info["tile_entries"] + info["tile_long_entries"] + info["tile_mid_entries"]
                assert ui["map_bytes"] >= 4 * slots and ui["map_build_us"] > 0, (ui, info)
            else:
                assert ui["map_bytes"] == 0 and ui["map_build_us"] == 0.0, ui


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["T1", "T4-device-tiles"])
def test_row_range_handles_update_their_own_slices_and_stitch(gpu, oracle, case, dtype):
    """two row-range handles of one matrix, each updated with its own rows' entries: each is the fresh upload of its rows
    (the twin of a row range), and the two stitch to A x within the suite's gates"""
    M, N, rp, col, val = target_of(case, dtype)
    xs, y_refs, _ = inputs_of(case, dtype, oracle)
    other = other_values(val, 4)
    cut = M // 2 + 3
    stitched, fresh = np.zeros(M, dtype=dtype), np.zeros(M, dtype=dtype)
    with sp.tuning(**CASES[case][1], **PINNED):
        for r0, r1 in ((0, cut), (cut, M)):
            e0, e1 = int(rp[r0]), int(rp[r1])
            with sp.CsrDevice(M, N, rp, col, other, r0, r1) as h, sp.CsrDevice(M, N, rp, col, val, r0, r1) as twin:
                h.update_values(val[e0:e1])
                assert h.download()[2].tobytes() == val[e0:e1].tobytes()
                assert h.tile_digest() == twin.tile_digest()
                assert {k: v for k, v in h.info().items() if k not in TIMED} == {k: v for k, v in twin.info().items() if k not in TIMED}
                for name, variant in sp.CSR_VARIANTS.items():
                    got, want = launched(h, xs[1], lambda: h.run(variant)), launched(twin, xs[1], lambda: twin.run(variant))
                    assert got[r0:r1].tobytes() == want[r0:r1].tobytes(), f"{case} rows [{r0}, {r1}) {name}"
                stitched[r0:r1] = launched(h, xs[0], lambda: h.run(sp.CSR_AUTO))[r0:r1]
                fresh[r0:r1] = launched(twin, xs[0], lambda: twin.run(sp.CSR_AUTO))[r0:r1]
    assert stitched.tobytes() == fresh.tobytes()
    gate = assert_parity if dtype == np.float64 else assert_parity_f32
    gate(stitched, y_refs[0], rp, col, val, xs[0], what=f"{case} stitched")


@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_and_solvers_after_an_update(gpu, dtype):
    """what is built from an updated handle is built from the new values: transpose().download() is the transpose of the
    new matrix, five steps of pcg with Jacobi and of bicgstab give the twin's bytes"""
    tgt = spd_target(dtype)
    M, N, rp, col, val = tgt
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, M).astype(dtype)

    def consume(dev):
        out = {}
        with dev.preconditioner("jacobi") as J:
            out["pcg"] = dev.pcg(b, 5, precond=J)[:4]             # (the last element of each result: milliseconds)
        out["bicgstab"] = dev.bicgstab(b, 5)[:3]
        with dev.transpose() as at:
            out["transpose"] = at.download()
        return out

    with sp.tuning(**PINNED):
        with sp.CsrDevice(M, N, rp, col, other_values(val, 6)) as h, sp.CsrDevice(*tgt) as twin:
            h.update_values(val)
            seen = consume(h)
            same_results(seen, consume(twin), f"fem-like {np.dtype(dtype).name}")
    for name, got, want in zip(("row_ptr", "col", "val"), seen["transpose"], transpose_ref(M, N, rp, col, val)):
        assert got.tobytes() == np.asarray(want, dtype=got.dtype).tobytes(), f"transpose after the update: {name}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["T1", "T4-device-tiles"])
def test_refusals_leave_the_handle_as_it_was(gpu, oracle, case, dtype):
    tgt = target_of(case, dtype)
    M, N, rp, col, val = tgt
    xs, _, _ = inputs_of(case, dtype, oracle)
    twin_seen = twin_of(case, dtype, oracle, True)
    other = other_values(val, 8)
    wrong_dtype = np.float32 if dtype == np.float64 else np.float64
    y_key = "y stream x0"

    def y_now(h):
        return launched(h, xs[0], lambda: h.run(sp.CSR_STREAM)).tobytes()

    with sp.tuning(**CASES[case][1], **PINNED):
        with sp.CsrDevice(M, N, rp, col, other) as h:
            h.update_values(val)
            want = twin_seen[y_key].tobytes()
            assert y_now(h) == want
            for bad in (val[:-1], np.concatenate([val, val[:1]]), val.astype(wrong_dtype), val.reshape(1, -1)):
                with pytest.raises(ValueError):
                    h.update_values(bad)
                assert y_now(h) == want and h.update_info()["updates"] == 1
            with pytest.raises(sp.SpmvHipError, match="NULL"):
                h.update_values_on(0)
            assert y_now(h) == want and h.update_info()["updates"] == 1
            h.update_values(val)                                   # a second update after the refusals
            assert y_now(h) == want and h.update_info()["updates"] == 2
            # a handle that holds a column split: refused, untouched; without the split it updates again
            counts = h.split_columns(M // 4, 3 * M // 4)
            assert counts["halo_entries"] > 0, counts
            with pytest.raises(sp.SpmvHipError, match="split"):
                h.update_values(other)
            with device_copy(other) as d_other:
                with pytest.raises(sp.SpmvHipError, match="split"):
                    h.update_values_on(d_other)
            assert y_now(h) == want and h.download()[2].tobytes() == val.tobytes() and h.update_info()["updates"] == 2
            h.split_columns(0, N)                                  # every column its own: the split is dropped
            h.update_values(other)
            h.update_values(val)
            assert h.update_info()["updates"] == 4
            assert_twin(h, tgt, xs, f"{case} after the refusals", X3=inputs_of(case, dtype, oracle)[2], twin_seen=twin_seen)
