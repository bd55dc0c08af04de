"""Host-only: the fp32 row gate (assert_parity_f32) is sound -- fp32 sums of seeded rows in any of the orders the
kernels use pass it -- and sharp -- one dropped entry fails it where the norm-wise check passes; the wide-range
generator stays in the normal range and the oracle obeys the power-of-two scaling identity bit for bit; the poison helpers (assert_poison_x, assert_poison_values,
assert_guard_bands) reject a leaked or a missing NaN, a one-ulp change, an infinity of the wrong sign and one changed
guard byte."""
import numpy as np
import pytest

from _util import (FP32_NORMWISE_RTOL, WIDE_EXP, assert_guard_bands, assert_parity, assert_parity_f32, assert_poison_values,
                   assert_poison_x, assert_same_numbers, random_csr, scale_rows, scaled_copy, scaling, wide_range)


def fp32_sequential(p):
    acc = np.float32(0)
    for v in p:
        acc = np.float32(acc + v)
    return acc


def fp32_lanes_xor_tree(p, lanes=64):
    """Lane l sums entries l, l + lanes, ... in fp32; the lanes then meet in an xor butterfly (every lane ends with the
    same sum: lane 0's is returned)."""
    acc = np.zeros(lanes, dtype=np.float32)
    for start in range(0, len(p), lanes):
        chunk = p[start:start + lanes]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    off = lanes // 2
    while off:
        acc = (acc + acc[np.arange(lanes) ^ off]).astype(np.float32)
        off //= 2
    return acc[0]


def fp32_pieces(p, piece=37):
    """The row cut into pieces, each summed on its own (lanes + tree), the pieces' sums added afterwards in order."""
    parts = [fp32_lanes_xor_tree(p[s:s + piece], 8) for s in range(0, len(p), piece)]
    return fp32_sequential(np.asarray(parts, dtype=np.float32)) if parts else np.float32(0)


ORDERS = {"sequential": fp32_sequential, "lanes+xor": fp32_lanes_xor_tree, "pieces": fp32_pieces}


def simulate(order, row_ptr, col, val, x):
    prod = (val * x[col]).astype(np.float32)          # fp32 products, rounded once
    return np.array([ORDERS[order](prod[row_ptr[r]:row_ptr[r + 1]]) for r in range(len(row_ptr) - 1)],
                    dtype=np.float32)


def seeded(rng, wide):
    M, N = 700, 5000
    lens = np.minimum(rng.poisson(20, M), 3000).astype(np.int64)
    lens[::97] = [1500, 0, 1, 2, 777, 64, 65, 3000][:len(lens[::97])]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens]).astype(np.int32)
    if wide:
        val, x = wide_range(rng, rp[-1], np.float32), wide_range(rng, N, np.float32)
        dr, dc = scaling(rng, M, N, np.float32)
        val, x = scaled_copy(rp, col, val, x, dr, dc)
    else:
        val, x = rng.uniform(-1, 1, rp[-1]).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32)
    return rp, col, val, x


@pytest.mark.parametrize("wide", [False, True], ids=["uniform", "wide-range"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_fp32_gate_passes_fp32_sums_in_every_order(oracle, order, wide):
    rng = np.random.default_rng(17 + wide)
    for trial in range(3):
        rp, col, val, x = seeded(rng, wide)
        y_ref = oracle.csr_f32_accum64(rp, col, val, x)
        y = simulate(order, rp, col, val, x)
        assert_parity_f32(y, y_ref, rp, col, val, x, what=f"{order} trial {trial}")
        # (the sums really are different: the gate is not passing bits equal to the oracle's)
        assert np.any(y.astype(np.float64) != y_ref)


def test_fp32_gate_catches_one_dropped_entry_the_normwise_check_accepts(oracle):
    rng = np.random.default_rng(4)
    rp, col, val, x = seeded(rng, wide=True)
    y_ref = oracle.csr_f32_accum64(rp, col, val, x)
    y = simulate("lanes+xor", rp, col, val, x)
    lens = np.diff(rp)
    # the smallest row with a few entries: its stray error is far below 1e-5 * max|y|
    cand = np.flatnonzero(lens >= 4)
    r = cand[np.argmin(np.abs(y_ref[cand]))]
    bad = y.copy()
    e = rp[r + 1] - 1
    bad[r] = np.float32(bad[r] - np.float32(val[e] * x[col[e]]))      # the row's last entry dropped
    err = np.max(np.abs(bad.astype(np.float64) - y_ref)) / np.max(np.abs(y_ref))
    assert err <= FP32_NORMWISE_RTOL                                   # the old check passes it ...
    with pytest.raises(AssertionError, match="beyond the fp32 summation bound"):
        assert_parity_f32(bad, y_ref, rp, col, val, x, what="dropped entry")   # ... the row gate does not
    # a stray term added to the NEXT row (a cross-row mix-up) is caught the same way
    bad = y.copy()
    nxt = r + 1 if r + 1 < len(y) else r - 1
    bad[nxt] = np.float32(bad[nxt] + np.float32(val[e] * x[col[e]]))
    if abs(float(val[e] * x[col[e]])) > 1e-3 * abs(float(y_ref[nxt])):
        with pytest.raises(AssertionError):
            assert_parity_f32(bad, y_ref, rp, col, val, x, what="stray term")


def test_fp32_gate_demands_exact_zeros_finite_results_and_normal_products(oracle):
    rp = np.array([0, 0, 2, 2], dtype=np.int32)
    col = np.array([0, 1], dtype=np.int32)
    val = np.array([1.5, -0.25], dtype=np.float32)
    x = np.array([0.5, 2.0], dtype=np.float32)
    y_ref = oracle.csr_f32_accum64(rp, col, val, x)
    assert_parity_f32(np.array([0.0, 0.25, -0.0], np.float32), y_ref, rp, col, val, x)
    with pytest.raises(AssertionError):                                  # an empty row must be exactly 0
        assert_parity_f32(np.array([1e-30, 0.25, 0.0], np.float32), y_ref, rp, col, val, x)
    with pytest.raises(AssertionError, match="non-finite"):
        assert_parity_f32(np.array([0.0, np.nan, 0.0], np.float32), y_ref, rp, col, val, x)
    tiny = np.array([2.0 ** -70, 1.0], dtype=np.float32)                 # 2^-70 * 2^-70: subnormal in fp32
    with pytest.raises(AssertionError, match="subnormal"):
        assert_parity_f32(np.zeros(3, np.float32), np.zeros(3), rp, col, tiny, np.array([2.0 ** -70, 1.0], np.float32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_range_generator_is_normal_and_the_oracle_obeys_the_identity(oracle, dtype):
    rng = np.random.default_rng(8)
    M, N = 3000, 2500
    rp, col, _ = random_csr(rng, M, N, 30, 400, 0.05)
    val, x = wide_range(rng, rp[-1], dtype), wide_range(rng, N, dtype)
    assert np.all((np.abs(val) >= 2.0 ** -8) & (np.abs(val) <= 1)) and np.all((np.abs(x) >= 2.0 ** -8) & (np.abs(x) <= 1))
    assert (val < 0).mean() > 0.4 and (val > 0).mean() > 0.4
    dr, dc = scaling(rng, M, N, dtype)
    e = WIDE_EXP[np.dtype(dtype)]
    assert np.abs(np.log2(np.abs(dr))).max() == e and np.abs(np.log2(np.abs(dc))).max() == e   # the whole range is used
    vs, xs = scaled_copy(rp, col, val, x, dr, dc)
    assert vs.dtype == dtype and xs.dtype == dtype
    if dtype == np.float64:
        y, ys = oracle.csr_serial(rp, col, val, x), oracle.csr_serial(rp, col, vs, xs)
        assert_parity(ys, ys, rp, col, vs, xs)                            # (finite, and the gate's own sums are fine)
        assert_same_numbers(ys, scale_rows(y, dr), "oracle fp64")
    else:
        y, ys = oracle.csr_f32_accum64(rp, col, val, x), oracle.csr_f32_accum64(rp, col, vs, xs)
        assert_same_numbers(ys, y * dr, "oracle fp32 data, fp64 sums")
        assert_parity_f32(ys.astype(np.float32), ys, rp, col, vs, xs)    # the data the GPU tests use passes the checks
        # the fp32 sums of the scaled data are the scaled fp32 sums (what the GPU identity relies on)
        assert_same_numbers(simulate("lanes+xor", rp, col, vs, xs), scale_rows(simulate("lanes+xor", rp, col, val, x), dr),
                            "simulated fp32 sums")


# ---- the poison helpers on a hand-made 3-row example: row 0 reads columns 0 and 2, row 1 column 1, row 2 is empty
POISON_RP = np.array([0, 2, 3, 3], dtype=np.int32)
POISON_COL = np.array([0, 2, 1], dtype=np.int32)


def poison_example(oracle, dtype, poison):
    val = np.array([0.5, -0.25, 0.75], dtype=dtype)
    x = np.array([0.5, -1.0, 0.25], dtype=dtype)
    xp = x.copy()
    xp[2] = poison                                                       # read by row 0 only
    ref = oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64
    y_clean = ref(POISON_RP, POISON_COL, val, x).astype(dtype)
    y_poisoned = ref(POISON_RP, POISON_COL, val, xp).astype(dtype)
    return val, xp, y_clean, y_poisoned, ref(POISON_RP, POISON_COL, val, xp)


def one_ulp(v):
    return np.nextafter(v, np.asarray(2, dtype=v.dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_poison_x_helper_accepts_the_oracle_and_rejects_every_kind_of_leak(oracle, dtype):
    val, xp, y_clean, y, ref = poison_example(oracle, dtype, np.nan)
    assert np.isnan(y[0]) and y[1] == y_clean[1] == -0.75 and y[2] == 0
    args = (POISON_RP, POISON_COL, val, xp, ref)
    assert_poison_x(y_clean, y, *args)
    for row in (1, 2):                                                   # a leaked NaN in an untouched row
        bad = y.copy()
        bad[row] = np.nan
        with pytest.raises(AssertionError, match="changed bits"):
            assert_poison_x(y_clean, bad, *args)
    bad = y.copy()
    bad[0] = y_clean[0]                                                  # a missing NaN in a touched row
    with pytest.raises(AssertionError, match="not NaN"):
        assert_poison_x(y_clean, bad, *args)
    bad = y.copy()
    bad[1] = one_ulp(bad[1])                                             # one ulp in an untouched row
    assert bad[1] != y[1] and abs(float(bad[1]) - float(y[1])) <= 1e-7
    with pytest.raises(AssertionError, match="changed bits"):
        assert_poison_x(y_clean, bad, *args)
    bad = y.copy()
    bad[2] = -0.0                                                        # -0 for +0: the same number, other bits
    with pytest.raises(AssertionError, match="changed bits"):
        assert_poison_x(y_clean, bad, *args)
    with pytest.raises(AssertionError, match=r"beyond \[-1, 1\]"):      # the class argument needs the bound
        assert_poison_x(y_clean, y, POISON_RP, POISON_COL, val * 4, xp, ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_poison_x_helper_tells_the_infinities_apart(oracle, dtype):
    val, xp, y_clean, y, ref = poison_example(oracle, dtype, np.inf)
    assert ref[0] == -np.inf                                             # -0.25 * +Inf
    args = (POISON_RP, POISON_COL, val, xp, ref)
    assert_poison_x(y_clean, y, *args)
    for wrong in (np.inf, np.nan, y_clean[0]):                           # +Inf where the oracle has -Inf, NaN, finite
        bad = y.copy()
        bad[0] = wrong
        with pytest.raises(AssertionError, match="oracle"):
            assert_poison_x(y_clean, bad, *args)
    xp2 = xp.copy()
    xp2[0] = np.inf                                                      # +Inf - Inf in row 0: NaN, and only NaN
    ref2 = (oracle.csr_serial if dtype == np.float64 else oracle.csr_f32_accum64)(POISON_RP, POISON_COL, val, xp2)
    assert np.isnan(ref2[0])
    y2 = ref2.astype(dtype)
    assert_poison_x(y_clean, y2, POISON_RP, POISON_COL, val, xp2, ref2)
    with pytest.raises(AssertionError, match="not NaN"):
        assert_poison_x(y_clean, y, POISON_RP, POISON_COL, val, xp2, ref2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_poison_values_helper_rejects_leaked_missing_and_one_ulp(oracle, dtype):
    _, _, y_clean, y, _ = poison_example(oracle, dtype, np.nan)          # (row 0 NaN: as if its stored value were)
    assert_poison_values(y_clean, y, [0])
    bad = y.copy()
    bad[2] = np.nan
    with pytest.raises(AssertionError, match="changed bits"):            # a leaked NaN
        assert_poison_values(y_clean, bad, [0])
    with pytest.raises(AssertionError, match="holds a NaN value"):       # a missing NaN
        assert_poison_values(y_clean, y, [0, 1])
    with pytest.raises(AssertionError, match="holds a NaN value"):       # an infinity is not the NaN a NaN value gives
        assert_poison_values(y_clean, np.where(np.isnan(y), np.inf, y).astype(dtype), [0])
    bad = y.copy()
    bad[1] = one_ulp(bad[1])
    with pytest.raises(AssertionError, match="changed bits"):            # one ulp
        assert_poison_values(y_clean, bad, [0])


def test_guard_band_helper_rejects_one_changed_byte():
    before = bytes([0xA5]) * 512
    assert_guard_bands(before, bytes(before))
    for at in (0, 255, 256, 511):
        after = bytearray(before)
        after[at] ^= 1
        with pytest.raises(AssertionError, match=f"first at byte {at}"):
            assert_guard_bands(before, after)
    with pytest.raises(AssertionError, match="guard bands of"):
        assert_guard_bands(before, before[:-1])
