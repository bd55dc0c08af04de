"""One contract for every preconditioner kind (CsrDevice.preconditioner), run from one list: a new kind is one more line
in KINDS.  What is held here is what the kinds share -- the device apply, the k-wide apply at k = 1, the workspace, the
refusals of the kinds without a k-wide apply, the readers of another kind's payload, the lifetime -- on a symmetric
positive definite band of 67 rows (more than one wave; no multiple of 64, of 3 or of 4) and on the matrix of one row, in
both dtypes.  What each kind computes is held by its own test file."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import _amg_ref
import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd import _native as nat
from test_gpu_amg import apply_on_device as apply_multi_on_device
from test_gpu_amg import device_of
from test_gpu_pcg_multi import DeviceBuffer

pytestmark = pytest.mark.gpu

ONE_WIDE = "an SSOR or ILU(0) preconditioner is two triangular solves, and those take one right-hand side"
# name: (arguments, the reader of its own payload or None, what apply_multi_on says of a missing d_work: None where the
# kind needs none, ONE_WIDE where it has no k-wide apply)
KINDS = {
    "jacobi": ({}, None, None),
    "block_jacobi": ({"block": 3}, None, None),
    "ssor": ({}, "tri_info", ONE_WIDE),
    "ilu0": ({}, "tri_info", ONE_WIDE),
    "fsai": ({"cap": 4}, "fsai_info", "an FSAI apply needs d_work (rows x k values and one 128-byte line)"),
    "amg": ({"coarse_rows": 8}, "amg_info",  # 67 rows: more than one level
            "an AMG apply needs d_work (spmv_hip_precond_work_bytes: its level vectors)"),
    "chebyshev": ({"degree": 3}, "cheb_info",
                  "a CHEBYSHEV apply needs d_work (spmv_hip_precond_work_bytes: its three arrays)"),
}
WITH_FACTORS = ("ssor", "ilu0", "fsai")
# a reader and the end of its refusal of another kind's object
READERS = {"tri_info": "is not made of triangular solves", "fsai_info": "is not FSAI", "amg_info": "is not AMG",
           "amg_setup_info": "is not AMG", "cheb_info": "is not CHEBYSHEV"}

EVERY_KIND = pytest.mark.parametrize("kind", list(KINDS))
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
SIZES = pytest.mark.parametrize("n", [67, 1])

_MATRICES = {}


def matrix(n):
    if n not in _MATRICES:
        _MATRICES[n] = _amg_ref.spd_band(n, 2, 5) if n > 1 else sps.csr_matrix(np.array([[2.5]]))
    return _MATRICES[n]


def built(kind, n, dtype):
    """(the handle, its preconditioner of `kind`, a right-hand side)"""
    dev = device_of(matrix(n), dtype)
    P = dev.preconditioner(kind, **KINDS[kind][0])
    return dev, P, np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)


def refusal(call):
    with pytest.raises(sp.SpmvHipError) as e:
        call()
    return str(e.value)


@EVERY_KIND
@SIZES
@DTYPES
def test_apply_on_gives_the_bytes_of_apply(gpu, kind, n, dtype):
    dev, P, r = built(kind, n, dtype)
    with dev, P:
        assert P.info() == {"kind": sp.PRECOND_KINDS[kind], "block": KINDS[kind][0].get("block", 1), "rows": n,
                            "row0": 0, "value_bytes": np.dtype(dtype).itemsize}
        if kind == "amg":
            assert (P.amg_info()["levels"] > 1) == (n > 1)
        z = P.apply(r)
        assert np.all(np.isfinite(z)) and np.any(z != 0)
        on = np.zeros_like(r)
        with DeviceBuffer(r.nbytes + 128) as d_r, DeviceBuffer(r.nbytes + 128) as d_z:
            assert sp.lib().spmv_hip_memcpy_h2d(C.c_void_p(d_r), r.ctypes.data_as(C.c_void_p), r.nbytes) == 0
            P.apply_on(d_r, d_z)
            sp.hip_sync()
            assert sp.lib().spmv_hip_memcpy_d2h(on.ctypes.data_as(C.c_void_p), C.c_void_p(d_z), on.nbytes) == 0
        assert on.tobytes() == z.tobytes()


@pytest.mark.parametrize("kind", [k for k in KINDS if KINDS[k][2] != ONE_WIDE])
@SIZES
@DTYPES
def test_the_k_wide_apply_at_one_column(gpu, kind, n, dtype):
    dev, P, r = built(kind, n, dtype)
    sentence = KINDS[kind][2]
    with dev, P:
        z = P.apply(r)
        R = np.ascontiguousarray(r.reshape(n, 1))
        assert P.apply_multi(R).tobytes() == z.tobytes()
        w1, w4 = P.work_bytes(1), P.work_bytes(4)
        if sentence is None:
            assert w1 == 0 and w4 == 0
            assert apply_multi_on_device(P, R, 1, with_work=False).tobytes() == z.tobytes()
        else:
            assert 0 < w1 <= w4
            assert refusal(lambda: apply_multi_on_device(P, R, 1, with_work=False)) == \
                f"spmv_hip_precond_apply_multi_on: precond_apply_multi_on: {sentence}"
            assert apply_multi_on_device(P, R, 1).tobytes() == z.tobytes()
        assert P.apply(r).tobytes() == z.tobytes()


def raw_lobpcg(dev, P, k):
    """past the Python checks, into the library"""
    n = P.rows
    X0, w, X, resid = np.ones((n, k)), np.zeros(k), np.zeros((n, k)), np.zeros(k)
    th, rh = np.zeros((2, k)), np.zeros((2, k))
    words = np.zeros(4, dtype=np.int32)
    anorm, ms, host_ms = C.c_double(0), C.c_float(0), C.c_float(0)
    dp = nat.c_double_p
    rc = sp.lib().spmv_hip_csr_lobpcg(dev.h, P.h, k, 1, 0.0, 0, X0.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                      X.ctypes.data_as(dp), th.ctypes.data_as(dp), rh.ctypes.data_as(dp),
                                      resid.ctypes.data_as(dp), C.byref(anorm), words.ctypes.data_as(nat.c_int_p),
                                      C.byref(ms), C.byref(host_ms))
    sp.device._check(rc, "spmv_hip_csr_lobpcg")


@pytest.mark.parametrize("kind", [k for k in KINDS if KINDS[k][2] == ONE_WIDE])
@SIZES
@DTYPES
def test_the_one_wide_kinds_refuse_every_k_wide_call(gpu, kind, n, dtype):
    dev, P, r = built(kind, n, dtype)
    with dev, P:
        z = P.apply(r)
        R = np.ascontiguousarray(r.reshape(n, 1))

        def on_device():
            with DeviceBuffer(R.nbytes + 128) as d_r, DeviceBuffer(R.nbytes + 128) as d_z, DeviceBuffer(256) as d_w:
                P.apply_multi_on(d_r, d_z, 1, d_work=d_w)

        calls = {"spmv_hip_precond_work_bytes: precond_work_bytes": lambda: P.work_bytes(1),
                 "spmv_hip_precond_apply_multi: precond_apply_multi": lambda: P.apply_multi(R),
                 "spmv_hip_precond_apply_multi_on: precond_apply_multi_on": on_device,
                 "spmv_hip_csr_pcg_multi: csr_pcg_multi": lambda: dev.pcg_multi(R, 2, precond=P)}
        # csr_lobpcg asks for fp64 and for n >= 4 k before it looks at the preconditioner
        if dtype == np.float64 and n >= 8:
            calls["spmv_hip_csr_lobpcg: csr_lobpcg"] = lambda: raw_lobpcg(dev, P, 2)
        for prefix, call in calls.items():
            assert refusal(call) == f"{prefix}: {ONE_WIDE}"
            assert P.apply(r).tobytes() == z.tobytes(), prefix


def raw_amg_level(P):
    rc = sp.lib().spmv_hip_precond_amg_level(P.h, 0, 0, None, None, None, None)
    return rc, sp.lib().spmv_hip_last_error().decode()


@EVERY_KIND
@SIZES
@DTYPES
def test_the_readers_of_another_kind_are_refused(gpu, kind, n, dtype):
    dev, P, r = built(kind, n, dtype)
    number = sp.PRECOND_KINDS[kind]
    own = KINDS[kind][1]
    with dev, P:
        z = P.apply(r)
        for reader, tail in READERS.items():
            if reader == own or (reader == "amg_setup_info" and own == "amg_info"):
                assert getattr(P, reader)()
            else:
                name = f"precond_{reader}"
                assert refusal(getattr(P, reader)) == f"spmv_hip_{name}: {name}: kind {number} {tail}"
        rc, msg = raw_amg_level(P)
        if kind == "amg":
            assert rc == 0
        else:
            assert (rc, msg) == (-1, f"precond_amg_level: kind {number} is not AMG")
        if kind in WITH_FACTORS:
            factors = P.factors()
            assert len(factors) == 2
            for rp, col, val in factors:
                assert rp.shape == (n + 1,) and rp[0] == 0 and np.all(np.diff(rp) >= 1)  # both hold their diagonal
                assert col.shape == val.shape == (rp[-1],) and val.dtype == dtype
        else:
            assert refusal(P.factors) == f"spmv_hip_precond_factors: precond_factors: kind {number} has no factors"
        assert P.apply(r).tobytes() == z.tobytes()


@EVERY_KIND
@SIZES
@DTYPES
def test_the_preconditioner_outlives_its_handle(gpu, kind, n, dtype):
    dev, P, r = built(kind, n, dtype)
    with P:
        z = P.apply(r)
        dev.close()
        assert P.apply(r).tobytes() == z.tobytes()
