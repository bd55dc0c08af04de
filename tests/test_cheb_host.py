"""The Chebyshev polynomial preconditioner without a GPU: the coefficient loop against its restatement bit for bit, the
Python checks before any device call, the polynomial identity of the restatement, the step counts it predicts, and the
resources of the new passes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _amg_ref
import _cheb_ref as ref
import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels
from conftest import ROOT
from test_precond_host import _handle_without_device

INTERVALS = [(2.0 / 30.0, 2.0), (0.37, 1.9371)]


@pytest.mark.parametrize("degree", [1, 2, 5, 32])
@pytest.mark.parametrize("lmin,lmax", INTERVALS)
def test_coefficients_equal_the_numpy_loop_bit_for_bit(degree, lmin, lmax):
    a, b = sp.chebyshev_coefficients(degree, lmin, lmax)
    ra, rb = ref.coefficients(degree, lmin, lmax)
    assert a.shape == b.shape == (degree,) and a.dtype == b.dtype == np.float64
    assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes()
    assert a[0] == 0.0 and b[0] == 1.0 / ((lmax + lmin) / 2.0)
    assert np.all(a[1:] > 0.0) and np.all(a[1:] < 1.0) and np.all(b > 0.0)


def test_coefficients_refuse_bad_arguments():
    for args in ((0, 0.1, 2.0), (33, 0.1, 2.0), (2.5, 0.1, 2.0), (True, 0.1, 2.0), (3, 0.0, 2.0), (3, -0.1, 2.0),
                 (3, 2.0, 2.0), (3, 2.5, 2.0), (3, 0.1, float("inf")), (3, float("nan"), 2.0), (3, None, 2.0),
                 (3, 0.1, None)):
        with pytest.raises(ValueError):
            sp.chebyshev_coefficients(*args)
    L = sp.lib()
    buf = (C.c_double * 40)()
    for degree, lmin, lmax in ((0, 0.1, 2.0), (33, 0.1, 2.0), (3, 0.0, 2.0), (3, 2.0, 2.0), (3, 0.1, float("inf")),
                               (3, float("nan"), 2.0)):
        assert L.spmv_chebyshev_coefficients(degree, lmin, lmax, buf, buf) == -1
    assert L.spmv_chebyshev_coefficients(3, 0.1, 2.0, None, buf) == -1
    assert L.spmv_chebyshev_coefficients(3, 0.1, 2.0, buf, None) == -1


def test_kind_and_symbols():
    assert sp.device.PRECOND_KINDS["chebyshev"] == 7 == sp.PRECOND_CHEBYSHEV
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert re.search(r"SPMV_PRECOND_CHEBYSHEV\s*=\s*7\b", text)
    assert re.search(rf"SPMV_PRECOND_CHEB_INFO_WORDS\s*=\s*{len(sp.device.PRECOND_CHEB_INFO)}\b", text)
    assert re.search(rf"SPMV_CHEBYSHEV_MAX_DEGREE\s*=\s*{sp.device.CHEBYSHEV_MAX_DEGREE}\b", text)
    for name in ("spmv_chebyshev_coefficients", "spmv_hip_csr_precond_build_chebyshev", "spmv_hip_precond_cheb_info"):
        assert name in sp.EXPORTED_SYMBOLS
    build = sp.lib().spmv_hip_csr_precond_build_chebyshev
    assert build.restype is C.c_int and len(build.argtypes) == 6
    assert build.argtypes[1] is C.c_int and all(t is C.c_double for t in build.argtypes[2:5])


@pytest.mark.parametrize("kw", [
    {"degree": 0}, {"degree": 33}, {"degree": 2.5}, {"degree": True}, {"degree": "4"}, {"degree": None}, {"degree": float("nan")},
    {"lmax": -1.0}, {"lmax": float("inf")}, {"lmax": float("nan")}, {"lmin": -0.1}, {"lmin": float("inf")},
    {"lmin": float("nan")}, {"lmin": 2.0, "lmax": 2.0}, {"lmin": 2.5, "lmax": 2.0},
    {"ratio": 1.0}, {"ratio": 0.5}, {"ratio": float("nan")}, {"ratio": float("inf")},
    {"block": 2}, {"ordering": "multicolor"}])
def test_preconditioner_rejects_bad_arguments_before_any_device_call(kw):
    with pytest.raises(ValueError):
        _handle_without_device().preconditioner("chebyshev", **kw)


def test_good_arguments_reach_the_library():
    """the same NULL handle with arguments that pass: the call gets as far as the library, which refuses the handle"""
    for kw in ({}, {"degree": 1}, {"degree": 32, "lmax": 2.0, "lmin": 0.1}, {"lmin": 0.1}, {"lmax": 1.5, "ratio": 1.5},
               {"degree": np.int64(3)}):
        with pytest.raises(sp.SpmvHipError):
            _handle_without_device().preconditioner("chebyshev", **kw)


def test_the_new_keywords_end_the_signature():
    import inspect
    names = list(inspect.signature(sp.CsrDevice.preconditioner).parameters)
    assert names[-4:] == ["degree", "lmax", "lmin", "ratio"]
    defaults = inspect.signature(sp.CsrDevice.preconditioner).parameters
    assert (defaults["degree"].default, defaults["lmax"].default, defaults["lmin"].default, defaults["ratio"].default) == \
           (4, None, None, 30.0)


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 7, 8, 32])
def test_the_restatement_is_the_scaled_chebyshev_polynomial(degree):
    """1 - t p(t) = T_m((theta - t) / delta) / T_m(sigma) on 1 x 1 matrices, inside and outside the interval"""
    for lmin, lmax in INTERVALS:
        theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
        for t in (0.5 * lmin, lmin, theta, 0.9 * lmax, lmax):
            want = ref.chebyshev_t(degree, (theta - t) / delta) / ref.chebyshev_t(degree, theta / delta)
            assert abs(ref.residual_polynomial(t, degree, lmin, lmax) - want) <= 1e-12, (degree, lmin, lmax, t)


def test_degree_one_is_jacobi_over_theta():
    a = _amg_ref.spd_band(300, 4, 1)
    r = np.random.default_rng(1).uniform(-1, 1, 300)
    g = ref.inverse_diagonal(a, np.float64)
    lmin, lmax = ref.interval(a)
    assert ref.apply(a, g, r, 1, lmin, lmax).tobytes() == ((1.0 / ((lmax + lmin) / 2.0)) * (g * r)).tobytes()


def test_the_bound_of_the_restatement_covers_its_rounded_form():
    a = _amg_ref.spd_band(300, 4, 1)
    r = np.random.default_rng(2).uniform(-1, 1, (300, 3))
    lmin, lmax = ref.interval(a)
    for dtype in (np.float64, np.float32):
        a_held = a.astype(dtype).astype(np.float64)
        g = ref.inverse_diagonal(a_held, dtype)
        rr = r.astype(dtype).astype(np.float64)
        for degree in (1, 2, 4, 7):
            z, bound = ref.apply_with_bound(a_held, g, rr, degree, lmin, lmax, dtype)
            err = np.abs(ref.apply(a_held, g, rr, degree, lmin, lmax, dtype) - z)
            assert np.all(err <= bound), (dtype, degree)
            off = np.abs(ref.apply(a_held, g, rr, degree, lmin, 1.01 * lmax, dtype) - z)
            assert np.any(off > bound), (dtype, degree)      # the bound tells a 1 % larger lmax apart


def test_step_counts_of_the_restatement():
    """the counts the issue's table states: PCG to 1e-8 with the Gershgorin bound and ratio 30"""
    a = _amg_ref.laplacian(64, 64)
    b = np.random.default_rng(0).uniform(-1, 1, a.shape[0])
    assert ref.gershgorin(a) == 2.0
    assert [ref.pcg_steps(a, b, d, 1e-8) for d in (0, 2, 3, 4, 8)] == [193, 99, 68, 52, 31]
    band = _amg_ref.spd_band(300, 4, 1)
    bb = np.random.default_rng(0).uniform(-1, 1, 300)
    assert [ref.pcg_steps(band, bb, d, 1e-8) for d in (0, 2, 3, 4, 8)] == [42, 22, 18, 13, 7]


def test_step_counts_of_the_other_solvers():
    """the table's other rows: right-preconditioned BiCGSTAB on the stencil, LOBPCG with k = 4 on the 48 x 48 grid"""
    import _lobpcg_ref
    from test_gpu_precond import pbicgstab_ref
    a = _amg_ref.convection_diffusion(40)
    b = np.random.default_rng(0).uniform(-1, 1, a.shape[0])
    g, (lmin, lmax) = ref.inverse_diagonal(a, np.float64), ref.interval(a)
    steps = [pbicgstab_ref(lambda v: a @ v, minv, b, 2000, 1e-8)[-1]["steps"]
             for minv in (lambda v: g * v, lambda v: ref.apply(a, g, v, 4, lmin, lmax))]
    assert steps == [63, 17]
    a = _amg_ref.laplacian(48, 48)
    X0 = np.random.default_rng(0).standard_normal((a.shape[0], 4))
    g, (lmin, lmax) = ref.inverse_diagonal(a, np.float64), ref.interval(a)
    steps = [_lobpcg_ref.lobpcg_ref(a, X0, 2000, 1e-8, minv=minv)[-1]["steps"]
             for minv in (lambda R: g[:, None] * R, lambda R: ref.apply(a, g, R, 4, lmin, lmax))]
    assert steps == [320, 68]


def test_gershgorin_is_the_amg_plans_rho():
    """the bound the build takes lmax from is the rho of level 0 of the AMG host setup, bit for bit"""
    for a in (_amg_ref.laplacian(33, 31), _amg_ref.spd_band(300, 4, 1), _amg_ref.convection_diffusion(12)):
        assert sp.amg_plan(a.indptr, a.indices, a.data, max_levels=1)[0]["rho"] == ref.gershgorin(a)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chebyshev_passes_compile_for_gfx950_without_scratch():
    k = {n: v for n, v in compile_kernels("spmv_cheb.hip").items() if "cheb_" in n}
    for stem in ("cheb_first", "cheb_step", "mcheb_first", "mcheb_step"):
        for sig in ("IdLi1ELb0E", "IdLi1ELb1E", "IdLi2ELb0E", "IdLi2ELb1E", "IfLi1ELb0E", "IfLi1ELb1E", "IfLi4ELb0E",
                    "IfLi4ELb1E"):
            assert any(re.search(rf"\d+{stem}{sig}", n) for n in k), (stem, sig, sorted(k))
    for name, v in k.items():
        assert v.scratch == 0 and v.lds == 0, (name, v)
        assert v.vgprs <= 64, (name, v.vgprs)     # the bound the solver kernels sit under (test_bicgstab_host.py)
