"""The smoothed-aggregation AMG preconditioner on the GPU (CsrDevice.preconditioner("amg")): the levels the device holds
against the host setup, the apply against the restated V-cycle on those levels within an entry-wise running bound
(_amg_ref.cycle_with_bound), the bit identities (chain on and off, two applies, k = 1, column permutations, NaN
columns, the device form), refusals, and every solver that takes it."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import _amg_ref as ref
import sparsematrixvectormultiplication_amd as sp
from test_gpu_lobpcg import assert_eigenpairs
from test_gpu_pcg_multi import DeviceBuffer, assert_matches_pcg_columns
from test_gpu_precond import csr, pbicgstab_ref, pcg_ref
from test_trsv_host import canonical

pytestmark = pytest.mark.gpu


def device_of(a, dtype=np.float64, row0=0, row1=None):
    m, rp, col, val = csr(a)
    return sp.CsrDevice(m, m, rp, col, val.astype(dtype), row0, m if row1 is None else row1)


def shuffled_with_repeats(a, seed=3):
    """(rp, col, val) of a with every diagonal entry stored as two halves and every row's entries shuffled"""
    rng = np.random.default_rng(seed)
    rp, col, val = [0], [], []
    for i in range(a.shape[0]):
        c = list(a.indices[a.indptr[i]:a.indptr[i + 1]])
        v = list(a.data[a.indptr[i]:a.indptr[i + 1]])
        k = c.index(i)
        v[k] *= 0.5
        c.append(i)
        v.append(v[k])
        order = rng.permutation(len(c))
        col += [c[q] for q in order]
        val += [v[q] for q in order]
        rp.append(len(col))
    return np.array(rp, np.int32), np.array(col, np.int32), np.array(val)


def dirichlet_1d(n):
    return sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


CASES = {
    "grid_24x31": lambda: ref.laplacian(24, 31),
    "grid_64x64": lambda: ref.laplacian(64, 64),
    "one_row": lambda: sps.csr_matrix(np.array([[2.5]])),
    "direct_40": lambda: dirichlet_1d(40),
    "diagonal_300": lambda: sps.diags(np.linspace(1.0, 9.0, 300), format="csr"),
    "grid_with_isolated_rows": lambda: ref.with_isolated_rows(ref.laplacian(24, 31), 50),
}
RUNS = [(name, np.float64) for name in CASES] + [("grid_24x31", np.float32), ("grid_with_isolated_rows", np.float32)]
COVERED = {}  # case -> amg_info(), for test_the_cases_cover_every_path


def assert_levels_are_the_plan_rounded_once(P, a, dtype, what):
    """levels() against sp.amg_plan on the canonical block: the same bytes after one rounding to dtype"""
    want = sp.amg_plan(a.indptr, a.indices, a.data)
    got = P.levels()
    assert len(got) == len(want) == P.amg_info()["levels"], what
    for l, (g, w) in enumerate(zip(got, want)):
        assert (g["w"], g["rho"], g["kind"], g["rows"], g["aggregates"]) == \
               (w["w"], w["rho"], w["kind"], w["rows"], w["aggregates"]), (what, l)
        keys = [k for k in ("A", "P", "R", "inv") if k in w]
        assert sorted(k for k in g if k in ("A", "P", "R", "inv")) == sorted(keys), (what, l)
        for key in keys:
            assert g[key][2].dtype == dtype
            assert g[key][0].tobytes() == w[key][0].tobytes() and g[key][1].tobytes() == w[key][1].tobytes(), (what, l, key)
            assert g[key][2].tobytes() == w[key][2].astype(dtype).tobytes(), (what, l, key)
    return got


def assert_apply_within_the_running_bound(P, levels, b, dtype, what):
    z = P.apply(b)
    z_ref, bound = ref.cycle_with_bound(ref.from_reader(levels), b.astype(np.float64), dtype)
    err = np.abs(z.astype(np.float64) - z_ref)
    print(f"{what}: max |z - ref| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, max bound / max |z| = "
          f"{np.max(bound) / np.max(np.abs(z_ref)):.2e}")
    assert np.all(np.isfinite(z)) and np.all(err <= bound), (what, int(np.argmax(err - bound)))
    return z


@pytest.mark.parametrize("name,dtype", RUNS, ids=[f"{n}-{np.dtype(d)}" for n, d in RUNS])
def test_levels_and_apply(gpu, name, dtype):
    a = CASES[name]()
    n = a.shape[0]
    rng = np.random.default_rng(11)
    b = rng.uniform(-1, 1, n).astype(dtype)
    with device_of(a, dtype) as dev, dev.preconditioner("amg") as P, dev.preconditioner("amg") as P2:
        assert P.info() == {"kind": sp.PRECOND_AMG, "block": 1, "rows": n, "row0": 0,
                            "value_bytes": np.dtype(dtype).itemsize}
        a_held = sps.csr_matrix((a.data.astype(dtype).astype(np.float64), a.indices, a.indptr), shape=a.shape)
        levels = assert_levels_are_the_plan_rounded_once(P, a_held, dtype, name)
        for g, h in zip(levels, P2.levels()):                         # two builds: the same bytes
            for key in ("A", "P", "R", "inv"):
                if key in g:
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(g[key], h[key])), (name, key)
        info = P.amg_info()
        COVERED[name] = info
        assert info["rows"] == [lv["rows"] for lv in levels] and info["entries"] == [len(lv["A"][1]) for lv in levels]
        z = assert_apply_within_the_running_bound(P, levels, b, dtype, f"{name} {np.dtype(dtype)}")
        assert P.apply(b).tobytes() == z.tobytes() and P2.apply(b).tobytes() == z.tobytes()
        if name == "direct_40":
            assert info["levels"] == 1 and info["coarsest"] == sp.device.AMG_DIRECT and info["first_chained"] == 0
            assert info["launches"] == 1
            x = rng.uniform(-1, 1, n)
            ax = a @ x
            got = P.apply(ax)
            lv = ref.from_reader(levels)
            _, bound = ref.cycle_with_bound(lv, ax, dtype)
            slack = np.abs(lv[0]["inv"] @ a.toarray() - np.eye(n)) @ np.abs(x)   # what the stored inverse itself is off by
            assert np.all(np.abs(got - x) <= bound + slack), np.max(np.abs(got - x) / (bound + slack))
        if name == "diagonal_300":
            assert info["levels"] == 1 and info["coarsest"] == sp.device.AMG_SMOOTH and info["first_chained"] == -1
            w = 4.0 / 3.0
            want = w * (2.0 - w) * b / a.diagonal()
            assert np.all(np.abs(z - want) <= 8 * np.finfo(dtype).eps * np.abs(want))
        if name == "one_row":
            assert abs(z[0] - b[0] / 2.5) <= 4 * np.finfo(dtype).eps * abs(z[0])


def test_the_cases_cover_every_path(gpu):
    """from amg_info(): a chained tail of at least 2 levels, an unchained level below 0, both coarsest kinds, a level
    whose row count is no multiple of 64"""
    missing = [name for name in CASES if name not in COVERED]
    for name in missing:
        with device_of(CASES[name]()) as dev, dev.preconditioner("amg") as P:
            COVERED[name] = P.amg_info()
    infos = COVERED
    assert any(i["first_chained"] >= 1 and i["levels"] - i["first_chained"] >= 2 for i in infos.values())
    big = infos["grid_64x64"]
    assert big["rows"][:2] == [4096, 704] and big["first_chained"] == 2, big
    assert {i["coarsest"] for i in infos.values()} == {sp.device.AMG_DIRECT, sp.device.AMG_SMOOTH}
    assert any(r % 64 for i in infos.values() for r in i["rows"])
    for i in infos.values():
        assert 1000 <= i["complexity_x1000"] < 2000 and i["chain"] == 1 and i["launches"] >= 1


def test_unsorted_rows_with_repeats(gpu):
    a = ref.laplacian(24, 31)
    rp, col, val = shuffled_with_repeats(a)
    n = a.shape[0]
    b = np.random.default_rng(2).uniform(-1, 1, n)
    with sp.CsrDevice(n, n, rp, col, val) as dev, dev.preconditioner("amg") as P, \
            device_of(a) as clean, clean.preconditioner("amg") as Pc:
        block = canonical(rp, col, val, 0, n)
        assert abs(block - a).max() == 0                         # halves of the diagonal add back exactly
        levels = assert_levels_are_the_plan_rounded_once(P, block, np.float64, "shuffled rows")
        z = assert_apply_within_the_running_bound(P, levels, b, np.float64, "shuffled rows")
        assert z.tobytes() == Pc.apply(b).tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lifetime_and_row_ranges(gpu, dtype):
    a = ref.laplacian(40, 40)
    m, rp, col, val = csr(a)
    val = val.astype(dtype)
    r = np.random.default_rng(9).uniform(-1, 1, m).astype(dtype)
    dev = sp.CsrDevice(m, m, rp, col, val)
    P = dev.preconditioner("amg")
    z, lv = P.apply(r), P.levels()
    dev.close()                                                  # P outlives its handle
    assert P.apply(r).tobytes() == z.tobytes()
    assert all(u.tobytes() == v.tobytes() for g, h in zip(P.levels(), lv) for u, v in zip(g["A"], h["A"]))
    P.close()
    # a row-range handle builds the AMG of its own diagonal block: the bytes of that block uploaded on its own
    r0, r1 = 333, 1333
    mb, rpb, colb, valb = csr(canonical(rp, col, val, r0, r1 - r0))
    with sp.CsrDevice(m, m, rp, col, val, r0, r1) as part, part.preconditioner("amg") as Pp, \
            sp.CsrDevice(mb, mb, rpb, colb, valb.astype(dtype)) as own, own.preconditioner("amg") as Po:
        assert Pp.info()["row0"] == r0 and Pp.rows == r1 - r0 and Pp.amg_info()["levels"] >= 2
        for g, h in zip(Pp.levels(), Po.levels()):
            for key in ("A", "P", "R", "inv"):
                if key in g:
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(g[key], h[key])), key
        assert Pp.apply(r[r0:r1]).tobytes() == Po.apply(r[r0:r1]).tobytes()


def apply_on_device(P, R, k, with_work=True):
    L = sp.lib()
    Z = np.zeros_like(R)
    wb = P.work_bytes(k)
    with DeviceBuffer(R.nbytes + 128) as d_r, DeviceBuffer(R.nbytes + 128) as d_z, DeviceBuffer(max(wb, 16)) as d_w:
        assert L.spmv_hip_memset(C.c_void_p(d_w), 0, max(wb, 16)) == 0
        assert L.spmv_hip_memcpy_h2d(C.c_void_p(d_r), R.ctypes.data_as(C.c_void_p), R.nbytes) == 0
        P.apply_multi_on(d_r, d_z, k, d_work=d_w if with_work else 0)
        sp.hip_sync()
        assert L.spmv_hip_memcpy_d2h(Z.ctypes.data_as(C.c_void_p), C.c_void_p(d_z), Z.nbytes) == 0
    return Z


@pytest.mark.parametrize("name,dtype", [("grid_24x31", np.float64), ("grid_64x64", np.float64), ("grid_64x64", np.float32),
                                        ("direct_40", np.float64), ("diagonal_300", np.float32)])
def test_bit_identities(gpu, name, dtype):
    a = CASES[name]()
    n = a.shape[0]
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, n).astype(dtype)
    with device_of(a, dtype) as dev, dev.preconditioner("amg") as P, dev.preconditioner("amg", chain=False) as Pu:
        iu, ic = Pu.amg_info(), P.amg_info()
        assert iu["chain"] == 0 and iu["first_chained"] == -1 and iu["launches"] >= ic["launches"]
        z = P.apply(b)
        assert Pu.apply(b).tobytes() == z.tobytes()                       # chain off: the same bits
        assert P.apply(b).tobytes() == z.tobytes()                        # two applies
        assert P.apply_multi(b.reshape(n, 1)).tobytes() == z.tobytes()    # k = 1
        levels = ref.from_reader(P.levels())
        for k in (2, 3, 8, 64):
            R = rng.uniform(-1, 1, (n, k)).astype(dtype)
            Z = P.apply_multi(R)
            Zr, bound = ref.cycle_with_bound(levels, R.astype(np.float64), dtype)
            assert np.all(np.abs(Z - Zr) <= bound), (name, k)
            perm = rng.permutation(k)
            assert P.apply_multi(np.ascontiguousarray(R[:, perm])).tobytes() == np.ascontiguousarray(Z[:, perm]).tobytes()
            assert Pu.apply_multi(R).tobytes() == Z.tobytes()
            assert apply_on_device(P, R, k).tobytes() == Z.tobytes()      # the device form
            bad = R.copy()
            bad[n // 2, k // 2] = np.nan                                   # a NaN in one column reaches no other
            Zb = P.apply_multi(bad)
            keep = np.arange(k) != k // 2
            assert Zb[:, keep].tobytes() == Z[:, keep].tobytes() and np.isnan(Zb[:, k // 2]).any()
    dev = device_of(a, dtype)
    P = dev.preconditioner("amg")
    R = rng.uniform(-1, 1, (n, 3)).astype(dtype)
    Z = P.apply_multi(R)
    dev.close()                                                           # P works after the handle is closed
    assert P.apply_multi(R).tobytes() == Z.tobytes()
    P.close()


def test_refusals_leave_the_handle_working(gpu, oracle):
    a = ref.laplacian(24, 31)
    n, rp, col, val = csr(a)
    rng = np.random.default_rng(5)
    b, x = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    y_ref = oracle.csr_serial(rp, col, val, x)
    L = sp.lib()
    with device_of(a) as dev, dev.preconditioner("amg") as P:
        good = dev.pcg(b, 8, precond=P)

        def still_works(after):
            assert np.max(np.abs(dev.spmv(x) - y_ref)) <= 1e-10 * np.max(np.abs(y_ref)), after
            again = dev.pcg(b, 8, precond=P)
            assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes(), after

        R = rng.uniform(-1, 1, (n, 3))
        with DeviceBuffer(R.nbytes + 128) as d_r, DeviceBuffer(R.nbytes + 128) as d_z:
            with pytest.raises(sp.SpmvHipError, match="d_work"):
                P.apply_multi_on(d_r, d_z, 3)
        still_works("AMG without d_work")
        with device_of(ref.laplacian(20, 20)) as small, small.preconditioner("amg") as Ps, \
                device_of(a, np.float32) as d32, d32.preconditioner("amg") as P32:
            for other, what in ((Ps, "another size"), (P32, "another dtype")):
                for method in (dev.pcg, dev.bicgstab, dev.minres):
                    with pytest.raises(ValueError):
                        method(b, 2, precond=other)
                out = np.zeros(n)
                assert L.spmv_hip_csr_pcg(dev.h, other.h, 0, 2, 0.0, None, b.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p), None, None, None, None) == -1
                assert b"the preconditioner covers rows" in L.spmv_hip_last_error()
                still_works(what)
        for kw, word in (({"theta": 1.0}, "theta"), ({"coarse_rows": 0}, "coarse_rows"), ({"max_levels": 17}, "max_levels")):
            args = dict(theta=0.08, coarse_rows=64, max_levels=16)
            args.update(kw)
            out = C.c_void_p()
            assert L.spmv_hip_csr_precond_build_amg(dev.h, args["theta"], args["coarse_rows"], args["max_levels"], 1,
                                                    C.byref(out)) == -1
            assert not out and word.encode() in L.spmv_hip_last_error()
            still_works(word)
        with pytest.raises(sp.SpmvHipError, match="factors"):
            P.factors()
        for kind in ("ssor", "ilu0"):
            with dev.preconditioner(kind) as tri:
                with pytest.raises(sp.SpmvHipError, match="one right-hand side"):
                    tri.work_bytes(3)
        with dev.preconditioner("jacobi") as J, dev.preconditioner("fsai") as F:
            assert J.work_bytes(3) == 0 and F.work_bytes(3) == n * 3 * 8 + 128 and P.work_bytes(3) == 3 * P.work_bytes(1)
        still_works("the other kinds' work_bytes")
    bad = a.tolil()
    bad[17, 17] = -4.0
    with device_of(sps.csr_matrix(bad)) as dev:
        with pytest.raises(sp.SpmvHipError, match="row 17"):
            dev.preconditioner("amg")
        assert np.all(np.isfinite(dev.spmv(x)))
    neumann = sps.diags([-np.ones(39), np.r_[1.0, 2 * np.ones(38), 1.0], -np.ones(39)], [-1, 0, 1], format="csr")
    with device_of(neumann) as dev:
        with pytest.raises(sp.SpmvHipError, match="level 0"):
            dev.preconditioner("amg")
    m, rp2 = 10, np.arange(0, 4 * 10 + 1, 4, dtype=np.int32)
    with sp.CsrDevice(m, 12, rp2, rng.integers(0, 12, 40).astype(np.int32), rng.uniform(1, 2, 40)) as rect:
        with pytest.raises(sp.SpmvHipError, match="square"):
            rect.preconditioner("amg")


@pytest.fixture(scope="module")
def grid64():
    a = ref.laplacian(64, 64)
    return a, np.random.default_rng(64).standard_normal(a.shape[0])


def test_pcg_steps_follow_the_restatement_and_beat_jacobi(gpu, grid64):
    a, b = grid64
    tol = 1e-8
    with device_of(a) as dev, dev.preconditioner("amg") as P, dev.preconditioner("jacobi") as J:
        levels = ref.from_reader(P.levels())
        x, hrr, hrz, info, ms = dev.pcg(b, 500, tol=tol, precond=P)
        _, _, _, info_ref = pcg_ref(lambda v: a @ v, lambda r: ref.cycle(levels, r), b, 500, tol)
        jacobi = dev.pcg(b, 2000, tol=tol, precond=J)[3]
        print("pcg steps: amg", info, "restated", info_ref, "jacobi", jacobi)
        assert info["status"] == info_ref["status"] == jacobi["status"] == sp.PCG_CONVERGED
        assert abs(info["steps"] - info_ref["steps"]) <= 1 and 4 * info["steps"] <= jacobi["steps"]
        assert np.linalg.norm(b - a @ x) <= 10 * tol * np.linalg.norm(b)
        # minres converges with it on the SPD grid
        xm, hm, infom, _ = dev.minres(b, 500, tol=tol, precond=P)
        assert infom["status"] == sp.MINRES_CONVERGED and infom["steps"] <= 2 * info["steps"], infom
        assert np.linalg.norm(b - a @ xm) <= 100 * tol * np.linalg.norm(b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pcg_multi_with_amg(gpu, grid64, dtype):
    a, b = grid64
    n = a.shape[0]
    b = b.astype(dtype)
    B = np.random.default_rng(3).uniform(-1, 1, (n, 3)).astype(dtype)
    with device_of(a, dtype) as dev, dev.preconditioner("amg") as P:
        x, hrr, hrz, info, _ = dev.pcg(b, 6, precond=P)
        X, rr, rz, infom, _ = dev.pcg_multi(b.reshape(n, 1), 6, precond=P)      # k = 1: pcg bit for bit
        assert X[:, 0].tobytes() == x.tobytes() and rr[:, 0].tobytes() == hrr.tobytes() and rz[:, 0].tobytes() == hrz.tobytes()
        assert infom["steps"][0] == info["steps"] and infom["status"][0] == info["status"]
        if dtype == np.float64:
            assert_matches_pcg_columns(dev, B, 5, P, "amg k = 3")
        X3, _, _, info3, _ = dev.pcg_multi(B, 200, tol=1e-5, precond=P)
        assert np.all(info3["status"] == sp.PCG_CONVERGED) and np.all(info3["steps"] <= 30), info3
        res = np.linalg.norm(B.astype(np.float64) - a @ X3.astype(np.float64), axis=0)
        assert np.all(res <= 1e-4 * np.linalg.norm(B, axis=0))


def test_bicgstab_on_convection_diffusion(gpu):
    a = ref.convection_diffusion(40)
    b = np.random.default_rng(40).standard_normal(a.shape[0])
    tol = 1e-8
    with device_of(a) as dev, dev.preconditioner("amg") as P, dev.preconditioner("jacobi") as J:
        levels = ref.from_reader(P.levels())
        x, hist, info, _ = dev.bicgstab(b, 1000, tol=tol, precond=P)
        _, _, info_ref = pbicgstab_ref(lambda v: a @ v, lambda r: ref.cycle(levels, r), b, 1000, tol)
        jacobi = dev.bicgstab(b, 2000, tol=tol, precond=J)[2]
        print("bicgstab steps: amg", info, "restated", info_ref, "jacobi", jacobi)
        assert info["status"] == sp.BICG_CONVERGED and jacobi["status"] == sp.BICG_CONVERGED
        assert info["steps"] < jacobi["steps"]
        assert np.linalg.norm(b - a @ x) <= 100 * tol * np.linalg.norm(b)


def test_lobpcg_with_amg(gpu):
    a = ref.laplacian(48, 48)
    ev = np.linalg.eigvalsh(a.toarray())
    tol, k = 1e-8, 4
    with device_of(a) as dev, dev.preconditioner("amg") as P, dev.preconditioner("jacobi") as J:
        w, X, th, rh, info, ms = dev.lobpcg(k, 200, tol=tol, precond=P)
        assert info["status"] == sp.LOBPCG_CONVERGED, info
        assert_eigenpairs(a, ev, w, X, info, tol)
        jacobi = dev.lobpcg(k, 2000, tol=tol, precond=J)[4]
        print("lobpcg steps: amg", info["steps"], "jacobi", jacobi["steps"])
        assert jacobi["status"] == sp.LOBPCG_CONVERGED and 4 * info["steps"] <= jacobi["steps"]
