"""The AMG setup on the device (CsrDevice.preconditioner("amg", setup="device")) against the host setup, which defines
it: the same hierarchy byte for byte -- every row_ptr, col and val of every A_l, P_l and R_l, the dense inverse, w, rho,
the kinds, rows and aggregates, and (through apply's bits) g -- over matrices that put the strength test exactly on its
threshold, store strong entries in one direction only and have sums that are not exact; through both tiers of the
products; for shuffled rows with repeats, row ranges, fp32, every argument; the same refusals word for word; the same
solver steps."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import _amg_ref as ref
import sparsematrixvectormultiplication_amd as sp
from test_gpu_amg import CASES as BASE_CASES, device_of, shuffled_with_repeats
from test_gpu_precond import csr

pytestmark = pytest.mark.gpu

TIMES = ("download_us", "setup_us", "upload_us")


def tridiag(n):
    return sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])


def upwind(gx, gy):
    """one-sided in x: every (i, i - 1) of a line of gx has no stored (i - 1, i)"""
    bidiag = sps.diags([-np.ones(gx - 1), np.ones(gx)], [-1, 0])
    return sps.kron(sps.identity(gy), bidiag) + sps.kron(tridiag(gy), sps.identity(gx))


def weak_upper(gx, gy):
    a = ref.laplacian(gx, gy)
    return sps.tril(a) + 0.01 * sps.triu(a, 1)


def weighted(gx, gy, seed=5):
    """graph Laplacian of the gx x gy grid (x edges, then y edges) with random weights, + 0.01 I"""
    idx = np.arange(gx * gy).reshape(gx, gy)
    lo = np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()])
    hi = np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()])
    w = np.random.default_rng(seed).uniform(0.01, 1, lo.size)
    adj = sps.coo_matrix((w, (lo, hi)), shape=(gx * gy, gx * gy))
    adj = adj + adj.T
    return sps.diags(np.asarray(adj.sum(axis=1)).ravel() + 0.01) - adj


def laplacian_3d(g):
    t, eye = tridiag(g), sps.identity(g)
    return sps.kron(sps.kron(t, eye), eye) + sps.kron(sps.kron(eye, t), eye) + sps.kron(sps.kron(eye, eye), t)


def sorted_csr(a):
    a = sps.csr_matrix(a)
    a.sort_indices()
    return a


# name -> (matrix, arguments, what the host plan must give: rows per level or the number of levels, the kinds or None)
N, D, S = ref.NOT_COARSEST, ref.DIRECT, ref.SMOOTH
CASES = {name: (make, {}, None, None) for name, make in BASE_CASES.items()}
CASES["grid_64x64"] = (BASE_CASES["grid_64x64"], {}, [4096, 704, 101, 19], [N, N, N, D])
CASES.update({
    "tie_quarter": (lambda: ref.laplacian(24, 31), {"theta": 0.25}, 2, [N, S]),   # 0.25 sqrt(16) = 1 = |a_ij| exactly
    "tie_quarter_nudged": (lambda: ref.laplacian(24, 31), {"theta": 0.2500001}, 1, [S]),
    "upwind_20x17": (lambda: upwind(20, 17), {}, [340, 63], [N, D]),
    "weak_upper": (lambda: weak_upper(20, 17), {}, 2, [N, D]),
    "weighted_30x23": (lambda: weighted(30, 23), {}, 3, [N, N, D]),
    "weighted_30x23_theta_0.3": (lambda: weighted(30, 23), {"theta": 0.3}, 3, [N, N, D]),
    "lap3_14": (lambda: laplacian_3d(14), {}, [2744, 364, 13], [N, N, D]),
})
FP32 = ("grid_24x31", "grid_with_isolated_rows", "weighted_30x23", "upwind_20x17", "direct_40")
RUNS = [(name, np.float64) for name in CASES] + [(name, np.float32) for name in FP32]


def same_bytes(got, want, what):
    """two preconditioners' levels() and amg_info() (without its times)"""
    lg, lw = got.levels(), want.levels()
    assert len(lg) == len(lw), what
    for l, (g, w) in enumerate(zip(lg, lw)):
        assert sorted(g) == sorted(w), (what, l)
        for key in w:
            if key in ("A", "P", "R", "inv"):
                for part, u, v in zip(("row_ptr", "col", "val"), g[key], w[key]):
                    assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), (what, l, key, part)
            else:
                assert np.array(g[key]).tobytes() == np.array(w[key]).tobytes(), (what, l, key)   # w, rho: the bits
    ig, iw = got.amg_info(), want.amg_info()
    assert {k: v for k, v in ig.items() if k not in TIMES} == {k: v for k, v in iw.items() if k not in TIMES}, what
    return lw


def same_apply(got, want, n, dtype, what, seed=11):
    b = np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
    z = want.apply(b)
    assert np.all(np.isfinite(z)) and got.apply(b).tobytes() == z.tobytes(), what


@pytest.mark.parametrize("name,dtype", RUNS, ids=[f"{n}-{np.dtype(d)}" for n, d in RUNS])
def test_device_setup_gives_the_host_setup_s_bytes(gpu, name, dtype):
    make, kw, shape, kinds = CASES[name]
    a = sorted_csr(make())
    n = a.shape[0]
    with device_of(a, dtype) as dev, dev.preconditioner("amg", **kw) as Ph, \
            dev.preconditioner("amg", setup="device", **kw) as Pd, dev.preconditioner("amg", setup="device", **kw) as Pd2:
        levels = same_bytes(Pd, Ph, name)
        same_bytes(Pd2, Pd, name + ", two device builds")
        rows = [lv["rows"] for lv in levels]
        print(f"{name} {np.dtype(dtype)}: rows {rows}, kinds {[lv['kind'] for lv in levels]}")
        if kinds is not None and dtype == np.float64:            # the case reaches the levels it is here for
            assert [lv["kind"] for lv in levels] == kinds, (name, rows)
            assert rows == shape if isinstance(shape, list) else len(rows) == shape, (name, rows)
        assert Pd.info() == Ph.info() and Pd.work_bytes(3) == Ph.work_bytes(3)
        same_apply(Pd, Ph, n, dtype, name)
        same_apply(Pd2, Ph, n, dtype, name)
        R = np.random.default_rng(4).uniform(-1, 1, (n, 3)).astype(dtype)
        assert Pd.apply_multi(R).tobytes() == Ph.apply_multi(R).tobytes(), name


@pytest.mark.parametrize("name", ["grid_64x64", "lap3_14"])
def test_both_tiers_of_the_products(gpu, name):
    make, kw, _, _ = CASES[name]
    a = sorted_csr(make())
    with device_of(a) as dev, dev.preconditioner("amg", setup="device", **kw) as auto:
        for bp in (64, -1):
            with dev.preconditioner("amg", setup="device", block_products=bp, **kw) as P:
                same_bytes(P, auto, f"{name}, block_products = {bp}")
                same_apply(P, auto, a.shape[0], np.float64, f"{name}, block_products = {bp}")


def test_shuffled_rows_with_repeats(gpu):
    a = ref.laplacian(24, 31)
    rp, col, val = shuffled_with_repeats(a)
    n = a.shape[0]
    with sp.CsrDevice(n, n, rp, col, val) as dev, dev.preconditioner("amg") as Ph, \
            dev.preconditioner("amg", setup="device") as Pd:
        levels = same_bytes(Pd, Ph, "shuffled rows")
        assert len(levels) >= 2
        same_apply(Pd, Ph, n, np.float64, "shuffled rows")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_range_handle_and_lifetime(gpu, dtype):
    a = ref.laplacian(40, 40)
    m, rp, col, val = csr(a)
    val = val.astype(dtype)
    r0, r1 = 333, 1333
    with sp.CsrDevice(m, m, rp, col, val, r0, r1) as part, part.preconditioner("amg") as Ph, \
            part.preconditioner("amg", setup="device") as Pd:
        assert Pd.info() == Ph.info() and Pd.info()["row0"] == r0 and Pd.rows == r1 - r0
        assert len(same_bytes(Pd, Ph, "row range")) >= 2
        same_apply(Pd, Ph, r1 - r0, dtype, "row range")
    dev = sp.CsrDevice(m, m, rp, col, val)
    P = dev.preconditioner("amg", setup="device")
    r = np.random.default_rng(9).uniform(-1, 1, m).astype(dtype)
    z, lv = P.apply(r), P.levels()
    dev.close()                                                  # P outlives its handle
    assert P.apply(r).tobytes() == z.tobytes()
    assert all(u.tobytes() == v.tobytes() for g, h in zip(P.levels(), lv) for u, v in zip(g["A"], h["A"]))
    P.close()


@pytest.mark.parametrize("kw", [{"coarse_rows": 1}, {"coarse_rows": 256}, {"max_levels": 1}, {"max_levels": 2},
                                {"chain": False}], ids=lambda kw: "-".join(f"{k}_{v}" for k, v in kw.items()))
def test_arguments(gpu, kw):
    a = ref.laplacian(24, 31)
    with device_of(a) as dev, dev.preconditioner("amg", **kw) as Ph, dev.preconditioner("amg", setup="device", **kw) as Pd:
        levels = same_bytes(Pd, Ph, str(kw))
        if "max_levels" in kw:
            assert len(levels) == kw["max_levels"]
        if kw.get("coarse_rows") == 256:
            assert levels[-1]["kind"] == D and levels[-1]["rows"] > 64
        if "chain" in kw:
            assert Pd.amg_info()["chain"] == 0 and Pd.amg_info()["first_chained"] == -1
        same_apply(Pd, Ph, a.shape[0], np.float64, str(kw))


def grid_with(change):
    lil = ref.laplacian(24, 31).tolil()
    change(lil)
    out = sps.csr_matrix(lil)
    out.eliminate_zeros()
    out.sort_indices()
    return out


def set_entry(i, j, v):
    def change(lil):
        lil[i, j] = v
    return change


REFUSALS = {
    "missing_diagonal": (lambda: grid_with(set_entry(17, 17, 0.0)), "row 17 has no diagonal entry"),
    "negative_diagonal": (lambda: grid_with(set_entry(17, 17, -4.0)), "row 17 has a diagonal that is not finite and > 0"),
    "infinite_off_diagonal": (lambda: grid_with(set_entry(40, 41, np.inf)), "an entry of the matrix is not finite"),
}


def refusal_of(dev, **kw):
    with pytest.raises(sp.SpmvHipError) as err:
        dev.preconditioner("amg", **kw)
    return str(err.value).split(": ", 1)[1]                     # without the name of the entry point


@pytest.mark.parametrize("name", sorted(REFUSALS) + ["non_square"])
def test_refusals_in_the_host_setup_s_words(gpu, name):
    rng = np.random.default_rng(5)
    if name == "non_square":
        m, rp = 10, np.arange(0, 4 * 10 + 1, 4, dtype=np.int32)
        dev = sp.CsrDevice(m, 12, rp, rng.integers(0, 12, 40).astype(np.int32), rng.uniform(1, 2, 40))
        word, ncols = "square", 12
    else:
        make, word = REFUSALS[name]
        bad = make()
        if name == "missing_diagonal":
            assert 17 not in bad.indices[bad.indptr[17]:bad.indptr[18]]
        dev, ncols = device_of(bad), bad.shape[1]
    with dev:
        x = rng.uniform(-1, 1, ncols)
        if name == "infinite_off_diagonal":
            x[41] = 0.0                                          # 0 * inf aside, the other rows stay finite
        on_host, on_device = refusal_of(dev), refusal_of(dev, setup="device")
        assert word in on_host and on_device == on_host, (on_host, on_device)
        if name != "non_square":
            assert "local rows; the handle's first row is global row 0" in on_device
        out = C.c_void_p()
        assert sp.lib().spmv_hip_csr_precond_build_amg_device(dev.h, 0.08, 64, 16, 1, 0, C.byref(out)) == -1 and not out
        y = dev.spmv(x)                                          # the handle works and no stale HIP error is reported
        assert np.all(np.isfinite(np.delete(y, 40) if name == "infinite_off_diagonal" else y))
        sp.hip_sync()
        assert np.array_equal(dev.spmv(x), y, equal_nan=True)


def test_a_coarse_entry_beyond_fp32_is_refused_as_on_the_host(gpu):
    """4 * 8e37 is finite in fp32 and level 1's 4.56 * 8e37 is not: the rounding at the end refuses, after the whole
    hierarchy was made in fp64"""
    a = ref.laplacian(24, 31) * 8e37
    with device_of(a, np.float32) as dev:
        on_host, on_device = refusal_of(dev), refusal_of(dev, setup="device")
        assert "level 1: an entry of A is not finite in the handle's dtype" in on_host and on_device == on_host
    with device_of(a) as dev, dev.preconditioner("amg") as Ph, dev.preconditioner("amg", setup="device") as Pd:
        same_bytes(Pd, Ph, "8e37 in fp64")


def test_refused_arguments(gpu):
    L = sp.lib()
    with device_of(ref.laplacian(9, 9)) as dev:
        for args, word in (((1.0, 64, 16, 1, 0), "theta"), ((0.08, 0, 16, 1, 0), "coarse_rows"),
                           ((0.08, 64, 17, 1, 0), "max_levels"), ((0.08, 64, 16, 1, 3), "block_products"),
                           ((0.08, 64, 16, 1, 8192), "block_products")):
            out = C.c_void_p()
            assert L.spmv_hip_csr_precond_build_amg_device(dev.h, *args, C.byref(out)) == -1 and not out
            got = L.spmv_hip_last_error().decode()
            assert word in got, got
            if word != "block_products":                         # ... as the host entry refuses them
                assert L.spmv_hip_csr_precond_build_amg(dev.h, *args[:4], C.byref(out)) == -1
                assert L.spmv_hip_last_error().decode() == got
        with dev.preconditioner("amg", setup="device") as P:
            assert P.amg_info()["levels"] >= 1


def test_solvers_take_the_same_steps(gpu):
    a = ref.laplacian(64, 64)
    n = a.shape[0]
    b = np.random.default_rng(64).standard_normal(n)
    B = np.random.default_rng(3).uniform(-1, 1, (n, 3))
    with device_of(a) as dev, dev.preconditioner("amg") as Ph, dev.preconditioner("amg", setup="device") as Pd:
        xh, rrh, rzh, infoh, _ = dev.pcg(b, 200, tol=1e-8, precond=Ph)
        xd, rrd, rzd, infod, _ = dev.pcg(b, 200, tol=1e-8, precond=Pd)
        assert infoh["status"] == sp.PCG_CONVERGED and infod == infoh
        assert xd.tobytes() == xh.tobytes() and rrd.tobytes() == rrh.tobytes() and rzd.tobytes() == rzh.tobytes()
        Xh, _, _, ih, _ = dev.pcg_multi(B, 40, tol=1e-6, precond=Ph)
        Xd, _, _, idv, _ = dev.pcg_multi(B, 40, tol=1e-6, precond=Pd)
        assert Xd.tobytes() == Xh.tobytes() and np.array_equal(idv["steps"], ih["steps"])
        assert np.array_equal(idv["status"], ih["status"])


def test_setup_info(gpu):
    a = ref.laplacian(64, 64)
    with device_of(a) as dev, dev.preconditioner("amg") as Ph, dev.preconditioner("amg", setup="device") as Pd:
        host, device = Ph.amg_setup_info(), Pd.amg_setup_info()
        assert list(host) == list(device) == list(sp.device.PRECOND_AMG_SETUP_INFO)
        assert host["setup"] == 0 and all(v == 0 for v in host.values())
        assert device["setup"] == 1
        phases = [v for k, v in device.items() if k != "setup"]
        print("device setup of grid_64x64:", device, "amg_info", {k: Pd.amg_info()[k] for k in TIMES})
        assert all(v >= 0 for v in phases) and sum(phases) <= Pd.amg_info()["setup_us"] + 1000
        assert device["ap_us"] > 0 and device["rap_us"] > 0      # four levels: the products ran
    with device_of(BASE_CASES["diagonal_300"]()) as dev, dev.preconditioner("amg", setup="device") as P:
        info = P.amg_setup_info()                                # one SMOOTH level: no product, no inverse
        assert info["setup"] == 1 and info["ap_us"] == info["rap_us"] == info["transpose_us"] == info["inverse_us"] == 0
