"""The smoothed-aggregation AMG preconditioner without a device: the symbols and constants, the host setup
(spmv_amg_plan_*, sp.amg_plan) against the numpy / scipy restatement of its rules (_amg_ref.py), the ends of the
hierarchy, the restated V-cycle as a symmetric positive definite M with grid-independent step counts, and the
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import _amg_ref as ref
import sparsematrixvectormultiplication_amd as sp
from conftest import ROOT
from sparsematrixvectormultiplication_amd import _native as nat

NEW = {"spmv_amg_plan_build": 8, "spmv_amg_plan_levels": 1, "spmv_amg_plan_level": 7, "spmv_amg_plan_free": 1,
       "spmv_amg_plan_error": 0, "spmv_hip_csr_precond_build_amg": 6, "spmv_hip_precond_amg_info": 2,
       "spmv_hip_precond_amg_level": 7, "spmv_hip_precond_work_bytes": 3}
EPS = 2.0 ** -52


def plan(a, **kw):
    return sp.amg_plan(a.indptr, a.indices, a.data, **kw)


CASES = {
    "grid_24x31": lambda: ref.laplacian(24, 31),
    "grid_with_isolated_rows": lambda: ref.with_isolated_rows(ref.laplacian(24, 31), 50),
    "spd_band_500": lambda: ref.spd_band(500, 6),
    "anisotropic_32x32": lambda: ref.laplacian(32, 32, 100.0, 1.0),
}


def test_new_symbols_and_constants_are_in_step():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    L = sp.lib()
    for name, nargs in NEW.items():
        assert name in exported and name in sp.EXPORTED_SYMBOLS, name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert re.search(r"SPMV_PRECOND_AMG\s*=\s*6\b", header) and sp.PRECOND_AMG == 6
    assert sp.device.PRECOND_KINDS["amg"] == 6
    words = int(re.search(r"SPMV_PRECOND_AMG_INFO_WORDS\s*=\s*(\d+)", header).group(1))
    assert words == sp.device.PRECOND_AMG_INFO_WORDS == len(sp.device.PRECOND_AMG_INFO) + 32
    for name, value in (("A", 0), ("P", 1), ("R", 2), ("INV", 3), ("T", 4), ("NOT_COARSEST", 0), ("DIRECT", 1),
                        ("SMOOTH", 2)):
        assert re.search(rf"SPMV_AMG_{name}\s*=\s*{value}\b", header) and getattr(sp.device, "AMG_" + name) == value
    assert (ref.NOT_COARSEST, ref.DIRECT, ref.SMOOTH) == (0, 1, 2)
    kernels = open(os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "csrc", "hip", "amg_kernels.hpp")).read()
    assert int(re.search(r"kAmgChainRows\s*=\s*(\d+)", kernels).group(1)) == sp.device.AMG_CHAIN_ROWS == 256
    assert int(re.search(r"kAmgChainEntries\s*=\s*(\d+)", kernels).group(1)) == sp.device.AMG_CHAIN_ENTRIES == 4096
    assert int(re.search(r"kAmgMaxLevels\s*=\s*(\d+)", kernels).group(1)) == sp.device.AMG_MAX_LEVELS == 16


def test_python_arguments_are_checked_before_the_library_is_asked():
    dev = sp.CsrDevice.__new__(sp.CsrDevice)
    sp.device._Handle.__init__(dev)      # a NULL handle: any device call would fail, not raise ValueError
    dev.M, dev.N, dev.dtype = 5, 5, np.float64
    for kw in ({"theta": -0.1}, {"theta": 1.0}, {"theta": np.nan}, {"coarse_rows": 0}, {"coarse_rows": 257},
               {"coarse_rows": 2.5}, {"max_levels": 0}, {"max_levels": 17}, {"max_levels": True}, {"block": 2},
               {"ordering": "multicolor"}):
        with pytest.raises((ValueError, TypeError)):
            dev.preconditioner("amg", **kw)
    a = ref.laplacian(3, 3)
    for kw in ({"theta": 1.0}, {"coarse_rows": 257}, {"max_levels": 0}):
        with pytest.raises(ValueError):
            plan(a, **kw)


def entry_terms(r, a, p):
    """the largest number of products a_rj a_jk p_kc in one entry of R A P"""
    return int((ref.ones_of(r) @ ref.ones_of(a) @ ref.ones_of(p)).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_the_restatement_level_by_level(name):
    """Every level of the plan against one step of the restatement ON THE PLAN'S OWN A_l (level 0: the input), so that a
    last-bit difference of a coarse matrix cannot flip a strength decision between the two: the aggregates exactly, w
    and rho to 4 ulp, P within (k + 2) 2^-52 (T + g |A| T) with k the longest row of A, and A_{l+1} within
    t 2^-52 (|R| |A| |P|) with t the largest number of products in one entry."""
    a = CASES[name]()
    levels = plan(a)
    mats = ref.from_reader(levels)
    assert len(levels) >= 2 and abs(mats[0]["A"] - a).max() == 0
    assert np.array_equal(levels[0]["A"][0], a.indptr) and np.array_equal(levels[0]["A"][1], a.indices)
    for l, (lv, m) in enumerate(zip(levels, mats)):
        n = lv["rows"]
        w, rho = ref.level_step_scalars(m["A"])
        assert abs(lv["w"] - w) <= 4 * EPS * w and abs(lv["rho"] - rho) <= 4 * EPS * rho, (name, l)
        if lv["kind"] != ref.NOT_COARSEST:
            assert l == len(levels) - 1
            continue
        s = ref.level_step(m["A"], 0.08)
        t_rp, t_col, t_val = lv["T"]
        agg = np.full(n, -1, dtype=np.int64)
        agg[np.nonzero(np.diff(t_rp))[0]] = t_col
        assert np.all(np.diff(t_rp) <= 1) and np.all(t_val == 1.0)
        assert np.array_equal(agg, s["agg"]) and lv["aggregates"] == s["na"], (name, l)
        for key, got in (("P", m["P"]), ("R", m["R"]), ("next", mats[l + 1]["A"])):
            want = s[key]
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), (name, l, key)
        g = s["w"] / s["d"]
        pb = ref.structural_product(abs(m["A"]), s["T"])  # (its pattern holds T's: every aggregated row has its diagonal)
        pb.data = (pb.indices == s["agg"][np.repeat(np.arange(n), np.diff(pb.indptr))]) + np.repeat(g, np.diff(pb.indptr)) * pb.data
        assert np.array_equal(pb.indices, m["P"].indices)
        bound = (ref.longest(m["A"]) + 2) * EPS * pb.data
        assert np.all(np.abs(m["P"].data - s["P"].data) <= bound), (name, l, "P")
        assert abs(m["R"] - m["P"].T).max() == 0, (name, l, "R is the exact transpose")
        rap = ref.structural_product(abs(s["R"]), ref.structural_product(abs(m["A"]), abs(s["P"])))
        assert np.array_equal(rap.indices, mats[l + 1]["A"].indices)
        t = entry_terms(s["R"], m["A"], s["P"])
        want = ref.structural_product(m["R"], ref.structural_product(m["A"], m["P"]))  # from the plan's own P: P's last
        # bits are held above and do not enter this bound
        assert np.array_equal(want.indices, mats[l + 1]["A"].indices)
        diff = np.abs(mats[l + 1]["A"].data - want.data)
        print(f"{name} level {l}: n = {n}, aggregates = {s['na']}, t = {t}, max diff / bound = "
              f"{np.max(diff / (t * EPS * rap.data)):.3f}")
        assert np.all(diff <= t * EPS * rap.data), (name, l, "A next")
    # the independent restatement of the whole hierarchy has the same shape
    whole = ref.build(a)
    assert [lv["rows"] for lv in levels] == [lv["A"].shape[0] for lv in whole]
    assert [lv["kind"] for lv in levels] == [lv["kind"] for lv in whole]


def test_structure_of_the_aggregates_and_two_builds():
    a = CASES["grid_with_isolated_rows"]()
    first, second = plan(a), plan(a)
    for lv, lv2 in zip(first, second):
        for key in ("A", "P", "R", "T", "inv"):
            if key in lv:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(lv[key], lv2[key])), key
        assert (lv["w"], lv["rho"], lv["kind"], lv["rows"], lv["aggregates"]) == \
               (lv2["w"], lv2["rho"], lv2["kind"], lv2["rows"], lv2["aggregates"])
    lv = first[0]
    n = lv["rows"]
    nb = ref.strength_neighbours(a, a.diagonal(), 0.08)
    t = ref.csr_of(lv["T"], (n, lv["aggregates"]))
    counts = np.diff(t.indptr)
    isolated = np.array([len(s) == 0 for s in nb])
    assert isolated.sum() == 50
    assert np.all(counts[~isolated] == 1) and np.all(counts[isolated] == 0)
    assert np.all(np.asarray(t.sum(axis=1)).ravel()[~isolated] == 1.0)
    assert np.all(np.diff(ref.csr_of(lv["T"], (n, lv["aggregates"])).tocsc().indptr) >= 1)  # no empty aggregate
    # an isolated row is only smoothed: its row of P holds no entry (its only entry is its diagonal)
    assert np.all(np.diff(lv["P"][0])[isolated] == 0)


def test_ends_of_the_hierarchy():
    small = plan(ref.laplacian(6, 7))                       # 42 rows <= coarse_rows
    assert len(small) == 1 and small[0]["kind"] == ref.DIRECT and "P" not in small[0]
    inv = ref.csr_of(small[0]["inv"], (42, 42)).toarray()
    assert np.max(np.abs(inv @ ref.laplacian(6, 7).toarray() - np.eye(42))) <= 1e-13
    one = plan(sps.csr_matrix(np.array([[2.5]])))
    assert len(one) == 1 and one[0]["kind"] == ref.DIRECT and one[0]["inv"][2][0] == 0.4
    diag = plan(sps.diags(np.linspace(1.0, 9.0, 300), format="csr"))
    assert len(diag) == 1 and diag[0]["kind"] == ref.SMOOTH and diag[0]["rho"] == 1.0 and diag[0]["w"] == 4.0 / 3.0
    two = plan(ref.laplacian(24, 31), max_levels=2)
    assert [lv["kind"] for lv in two] == [ref.NOT_COARSEST, ref.SMOOTH] and two[1]["rows"] > 64
    one_level = plan(ref.laplacian(24, 31), max_levels=1)
    assert len(one_level) == 1 and one_level[0]["kind"] == ref.SMOOTH
    deep = plan(ref.laplacian(24, 31), coarse_rows=1)
    assert deep[-1]["kind"] in (ref.DIRECT, ref.SMOOTH) and len(deep) <= 16
    full = plan(ref.laplacian(64, 64))
    sizes = [lv["rows"] for lv in full]
    print("64 x 64: level sizes", sizes, "operator complexity",
          sum(len(lv["A"][1]) for lv in full) / len(full[0]["A"][1]))
    assert sizes[0] == 4096 and sizes == sorted(sizes, reverse=True) and sizes[-1] <= 64 and full[-1]["kind"] == ref.DIRECT


def test_restated_cycle_is_symmetric_positive_definite():
    a = ref.laplacian(16, 17)
    levels = ref.from_reader(plan(a))
    assert len(levels) >= 2
    m = ref.dense_m(levels, a.shape[0])
    assert np.max(np.abs(m - m.T)) <= 1e-12 * np.max(np.abs(m))
    assert np.min(np.linalg.eigvalsh((m + m.T) / 2)) > 0


def test_restated_pcg_step_counts_hardly_move_with_the_grid():
    """numpy PCG to 1e-8 with the restated cycle on the plan's levels, 5-point Laplacian on g x g, b = ones:
    steps(64) <= jacobi_steps(64) / 4 and steps(128) <= 1.5 steps(32)."""
    steps = {}
    for g in (32, 64, 128):
        a = ref.laplacian(g, g)
        levels = ref.from_reader(plan(a))
        b = np.random.default_rng(g).standard_normal(g * g)
        steps[g], x = ref.pcg_steps(a, b, lambda r: ref.cycle(levels, r), 1e-8)
        assert np.linalg.norm(b - a @ x) <= 1e-7 * np.linalg.norm(b)
    dinv = 1.0 / ref.laplacian(64, 64).diagonal()
    a = ref.laplacian(64, 64)
    b = np.random.default_rng(64).standard_normal(64 * 64)
    jacobi, _ = ref.pcg_steps(a, b, lambda r: dinv * r, 1e-8)
    print("pcg steps with the restated cycle", steps, "jacobi on 64 x 64", jacobi)
    assert steps[64] <= jacobi / 4 and steps[128] <= 1.5 * steps[32], (steps, jacobi)


def raw_build(n, rp, col, val, theta=0.08, coarse_rows=64, max_levels=16):
    L = sp.lib()
    out = C.c_void_p()
    rp, col = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(col, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    rc = L.spmv_amg_plan_build(n, rp.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p),
                               val.ctypes.data_as(nat.c_double_p), theta, coarse_rows, max_levels, C.byref(out))
    msg = L.spmv_amg_plan_error().decode()
    if rc == 0:
        L.spmv_amg_plan_free(out)
    else:
        assert not out.value
    return rc, msg


def test_refusals_name_the_row_or_the_level():
    a = ref.laplacian(9, 9)
    n = a.shape[0]
    for bad, word in ((0.0, "row 37"), (-4.0, "row 37"), (np.nan, "row 37"), (np.inf, "row 37")):
        b = a.copy()
        b[37, 37] = bad
        if bad == 0.0:
            assert b.indices[b.indptr[37]:b.indptr[38]].tolist().count(37) == 1  # a stored zero, not a missing entry
        rc, msg = raw_build(n, b.indptr, b.indices, b.data)
        assert rc == -1 and word in msg, (bad, msg)
        with pytest.raises(sp.SpmvHipError, match=word):
            plan(b)
    lil = a.tolil()
    lil[37, 37] = 0.0
    missing = sps.csr_matrix(lil)
    missing.eliminate_zeros()
    missing.sort_indices()
    rc, msg = raw_build(n, missing.indptr, missing.indices, missing.data)
    assert rc == -1 and "row 37" in msg and "no diagonal" in msg, msg
    for kw, word in (({"theta": 1.0}, "theta"), ({"theta": -0.5}, "theta"), ({"theta": float("nan")}, "theta"),
                     ({"coarse_rows": 0}, "coarse_rows"), ({"coarse_rows": 257}, "coarse_rows"),
                     ({"max_levels": 0}, "max_levels"), ({"max_levels": 17}, "max_levels")):
        rc, msg = raw_build(n, a.indptr, a.indices, a.data, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    # rows that are not canonical
    rc, msg = raw_build(2, [0, 2, 3], [1, 0, 1], [1.0, 2.0, 2.0])
    assert rc == -1 and "row 0" in msg and "canonical" in msg, msg
    # a singular coarsest matrix: the 1-D Neumann Laplacian of 40 rows (integers: the last pivot is exactly 0)
    neumann = sps.diags([-np.ones(39), np.r_[1.0, 2 * np.ones(38), 1.0], -np.ones(39)], [-1, 0, 1], format="csr")
    rc, msg = raw_build(40, neumann.indptr, neumann.indices, neumann.data)
    assert rc == -1 and "level 0" in msg and "pivot" in msg, msg
    # after every refusal the library still builds
    assert raw_build(n, a.indptr, a.indices, a.data)[0] == 0
    assert raw_build(0, [0], [], [])[0] == 0
