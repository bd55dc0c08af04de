"""spmv_spgemm_plan (no GPU): how the rows of C = A B are dealt out to the on-chip blocks and the long rows, on hand-written
count vectors.  Every plan is checked against the rules as a whole; the cases pin the edges."""
import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp


def check_plan(products, block_products, max_rows=4096):
    """The rules of include/spmv_hip.h; returns (blocks as (first row, end row), long rows)."""
    products = np.asarray(products, dtype=np.int64)
    M = len(products)
    block_row, long_rows = sp.spgemm_plan(products, block_products, max_rows)
    cap = {0: 4096, -1: 0}.get(block_products, block_products)
    assert block_row[0] == 0 and block_row[-1] == M, block_row
    assert np.all(np.diff(block_row) >= 1), "blocks partition the rows in order, none empty"
    want_long = np.flatnonzero(products > cap)
    assert long_rows.tolist() == want_long.tolist()
    covered = []
    for r0, r1 in zip(block_row[:-1], block_row[1:]):
        assert r1 - r0 <= max_rows, (r0, r1)
        own = [r for r in range(r0, r1) if products[r] <= cap]
        assert all(r == r1 - 1 for r in range(r0, r1) if products[r] > cap), "a long row ends its block"
        assert products[own].sum() <= cap, (r0, r1)
        covered += own
    assert sorted(covered + long_rows.tolist()) == list(range(M)), "every row exactly once"
    # greedy: a block is closed only by a long row, the row cap or a row that no longer fits
    for k in range(len(block_row) - 2):
        r0, r1 = int(block_row[k]), int(block_row[k + 1])
        nxt = products[r1]
        own = products[r0:r1][products[r0:r1] <= cap].sum()
        assert products[r1 - 1] > cap or r1 - r0 == max_rows or (nxt <= cap and own + nxt > cap), (r0, r1)
    return list(zip(block_row[:-1].tolist(), block_row[1:].tolist())), long_rows.tolist()


def test_a_row_of_exactly_the_cap_is_not_long_and_one_more_is():
    blocks, long_rows = check_plan([64, 65, 3], 64)
    assert long_rows == [1] and blocks == [(0, 2), (2, 3)]
    blocks, long_rows = check_plan([4096, 4097], 0)
    assert long_rows == [1] and blocks == [(0, 2)]


def test_a_block_that_fills_the_cap_exactly():
    blocks, long_rows = check_plan([10, 54, 1, 62, 1, 2], 64)
    assert blocks == [(0, 2), (2, 5), (5, 6)] and long_rows == []
    blocks, _ = check_plan([128] * 5 + [127, 2], 256)
    assert blocks == [(0, 2), (2, 4), (4, 6), (6, 7)]


def test_runs_of_empty_rows():
    blocks, long_rows = check_plan([0, 0, 0, 5, 0, 0, 60, 0, 0], 64)
    assert blocks == [(0, 6), (6, 9)] and long_rows == []
    # more empty rows in a row than a block may hold: the row cap cuts them
    blocks, long_rows = check_plan([7] + [0] * 10 + [9], 64, max_rows=4)
    assert blocks == [(0, 4), (4, 8), (8, 12)] and long_rows == []
    blocks, _ = check_plan([1] + [0] * 5000 + [1], 64)
    assert blocks == [(0, 4096), (4096, 5002)]
    blocks, long_rows = check_plan([0, 0, 100, 0, 0, 100, 0], 64)
    assert long_rows == [2, 5] and blocks == [(0, 3), (3, 6), (6, 7)]


def test_all_rows_empty_and_a_single_row():
    assert check_plan([0] * 9, 64) == ([(0, 9)], [])
    assert check_plan([0] * 9, -1) == ([(0, 9)], [])
    assert check_plan([0], 64) == ([(0, 1)], [])
    assert check_plan([64], 64) == ([(0, 1)], [])
    assert check_plan([65], 64) == ([(0, 1)], [0])
    block_row, long_rows = sp.spgemm_plan([], 64)
    assert block_row.tolist() == [0] and long_rows.tolist() == []


def test_without_the_on_chip_tier_every_row_with_a_product_is_long():
    blocks, long_rows = check_plan([3, 0, 1, 0, 0, 5000], -1)
    assert long_rows == [0, 2, 5] and blocks == [(0, 1), (1, 3), (3, 6)]


@pytest.mark.parametrize("cap", [64, 128, 1024, 4096, 0, -1])
def test_random_counts_obey_the_rules(cap):
    rng = np.random.default_rng(cap + 5)
    for max_rows in (1, 3, 4096):
        products = rng.integers(0, 40, 300) * (rng.random(300) < 0.7)
        products[rng.integers(0, 300, 6)] = rng.integers(60, 9000, 6)
        check_plan(products, cap, max_rows)


@pytest.mark.parametrize("bad", [dict(block_products=63), dict(block_products=100), dict(block_products=8192),
                                 dict(block_products=64, max_rows=0), dict(block_products=64, max_rows=4097),
                                 dict(block_products=-2), dict(block_products=32)])
def test_refused_caps(bad):
    with pytest.raises(ValueError):
        sp.spgemm_plan([1, 2, 3], **bad)
    with pytest.raises(ValueError):
        sp.spgemm_plan([1, -2, 3], 64)
