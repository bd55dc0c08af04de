"""The numpy restatement of spmv_hip_csr_gmres's loop (tests/_gmres_ref.py) against cases whose answers are known, so
that the GPU tests compare the device against something known to be right.  No GPU."""
import numpy as np
import pytest

from _gmres_ref import BREAKDOWN, CONVERGED, RAN_ALL, forward_dot, gmres_ref, reversed_dot
from test_gpu_bicgstab import convection_diffusion, nonsym_banded

PERMUTATION = np.array([[0.0, 1.0], [1.0, 0.0]])
# test_gpu_bicgstab.py::test_bicgstab_breakdowns: BiCGSTAB ends at step 1 with BREAKDOWN_OMEGA
OMEGA_A = np.array([[-1.0, 0.0, 2.0], [-1.0, -1.0, 2.0], [0.0, 0.0, 1.0]])
OMEGA_B = np.array([0.0, 1.0, 1.0])
SHIFT = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])

# the banded comparisons of tests/test_gpu_gmres.py: (iters, restart, bound on x, absolute and relative bound on hist)
BANDED_RUNS = ((5, 30, 1e-10, 0.0, 1e-10), (25, 10, 1e-7, 1e-8, 1e-4))


def mat(a):
    return lambda v: a @ v


def scipy_csr(row_ptr, col, val):
    import scipy.sparse as sps
    n = len(row_ptr) - 1
    return sps.csr_matrix((val, col, row_ptr), shape=(n, n))


def test_permutation_bicgstab_cannot_solve():
    x, h, info = gmres_ref(mat(PERMUTATION), np.array([1.0, 0.0]), 6, restart=4)
    assert info == {"steps": 2, "status": CONVERGED, "cycles": 1}
    assert np.array_equal(x, [0.0, 1.0])
    assert np.array_equal(h, [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def test_omega_matrix_bicgstab_cannot_solve():
    x, h, info = gmres_ref(mat(OMEGA_A), OMEGA_B, 6, tol=1e-12, restart=3)
    assert info == {"steps": 3, "status": CONVERGED, "cycles": 1}
    assert np.max(np.abs(x - [2.0, -1.0, 1.0])) <= 1e-12
    assert np.max(np.abs(OMEGA_A @ x - OMEGA_B)) <= 1e-12


def test_scaled_identity_and_zero_right_hand_side():
    b = np.ones(4)
    x, h, info = gmres_ref(mat(4.0 * np.eye(4)), b, 3, restart=5)
    assert info == {"steps": 1, "status": CONVERGED, "cycles": 1}
    assert h[0] == 4.0 and np.all(h[1:] == 0.0) and np.array_equal(x, b / 4)
    x, h, info = gmres_ref(mat(4.0 * np.eye(4)), np.zeros(4), 3)
    assert info == {"steps": 0, "status": CONVERGED, "cycles": 0}
    assert np.all(x == 0.0) and np.all(h == 0.0)
    x, h, info = gmres_ref(mat(4.0 * np.eye(4)), b, 0)
    assert info == {"steps": 0, "status": RAN_ALL, "cycles": 1} and np.all(x == 0.0) and np.array_equal(h, [4.0])
    x, h, info = gmres_ref(mat(4.0 * np.eye(4)), np.array([1.0, np.nan, 0.0, 0.0]), 3)
    assert info == {"steps": 0, "status": BREAKDOWN, "cycles": 0} and np.all(x == 0.0)


def test_nilpotent_shift_breaks_down_without_touching_x():
    x, h, info = gmres_ref(mat(SHIFT), np.array([1.0, 0.0, 0.0]), 5, restart=4)
    assert info == {"steps": 0, "status": BREAKDOWN, "cycles": 1}
    assert np.all(x == 0.0) and np.all(h == 1.0)
    x, h, info = gmres_ref(mat(SHIFT), np.array([0.0, 0.0, 1.0]), 5, restart=4)
    assert info == {"steps": 2, "status": BREAKDOWN, "cycles": 1}
    assert np.all(x == 0.0) and np.all(h == 1.0)


def test_skew_tridiagonal_needs_every_step_and_never_grows():
    n = 64
    a = np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    b = np.random.default_rng(64).uniform(-1, 1, n)
    x, h, info = gmres_ref(mat(a), b, 80, tol=1e-10, restart=64)
    assert info == {"steps": 64, "status": CONVERGED, "cycles": 1}
    # |s| <= 1 exactly, so the estimate never grows from step 1 on; hist[0] is b.b itself and hist[1] = (s sqrt(b.b))^2,
    # which with s = 1 (the diagonal is 0) is b.b up to the rounding of the root and the square
    assert np.all(h[2:] <= h[1:-1]) and h[1] <= h[0] * (1.0 + 2.0 ** -51)
    r = b - a @ x
    assert np.sqrt(r @ r) <= 1e-13 * np.sqrt(b @ b)


@pytest.mark.parametrize("restart, steps", [(5, 54), (10, 76), (30, 46)])
def test_convection_diffusion_steps(restart, steps):
    """Central differences at cell Peclet numbers 0.6 and 0.3, tol 1e-8.  The counts are those of this b (they move by
    tens with the right-hand side: 47 to 70, 49 to 88 and 41 to 49 steps over a dozen seeds); within 2 because numpy's
    dot product may add in another order on another machine."""
    a = scipy_csr(*convection_diffusion(13, 11, 0.6, 0.3, 0.0))
    b = np.random.default_rng(1311).uniform(-1, 1, a.shape[0])
    x, h, info = gmres_ref(lambda v: a @ v, b, 200, tol=1e-8, restart=restart)
    assert info["status"] == CONVERGED and abs(info["steps"] - steps) <= 2, info
    assert info["cycles"] == -(-info["steps"] // restart)
    r = b - a @ x
    assert r @ r <= 1e-16 * (b @ b)
    assert h[info["steps"]] <= 1e-16 * h[0] < h[info["steps"] - 1]
    inside = np.arange(len(h) - 1) % restart != 0
    assert np.all(h[1:][inside[: len(h) - 1]] <= h[:-1][inside[: len(h) - 1]])


def test_power_of_two_scaling_is_exact():
    a = scipy_csr(*convection_diffusion(13, 11, 0.6, 0.3, 0.0))
    b = np.random.default_rng(7).uniform(-1, 1, a.shape[0])
    x, h, info = gmres_ref(lambda v: a @ v, b, 25, restart=10)
    xs, hs, infos = gmres_ref(lambda v: a @ v, b * 2.0 ** 7, 25, restart=10)
    assert info == infos == {"steps": 25, "status": RAN_ALL, "cycles": 3}
    assert np.array_equal(xs, x * 2.0 ** 7) and np.array_equal(hs, h * 4.0 ** 7)


def test_jacobi_from_the_right_is_the_column_scaled_system():
    a = scipy_csr(*convection_diffusion(9, 7, 0.6, 0.3, 0.5)).toarray()
    dinv = 1.0 / (np.arange(a.shape[0]) % 5 + 1.0)
    b = np.random.default_rng(8).uniform(-1, 1, a.shape[0])
    x, h, info = gmres_ref(mat(a), b, 12, restart=5, minv=lambda v: dinv * v)
    y, hy, infoy = gmres_ref(mat(a * dinv[None, :]), b, 12, restart=5)
    assert info == infoy
    assert np.max(np.abs(x - dinv * y)) <= 1e-13 * np.max(np.abs(x)) and np.all(np.abs(h - hy) <= 1e-12 * hy)


def banded_spread():
    """(x spread / max |x|, largest relative history spread, largest absolute history spread / hist[0]) per run of
    BANDED_RUNS between the dot products summed forwards and in reversed row order."""
    n = 6000
    rng = np.random.default_rng(909)
    a = scipy_csr(*nonsym_banded(rng, n, 7, 60, 0.5))
    b = a @ rng.uniform(-1, 1, n)
    out = []
    for iters, restart, _, _, _ in BANDED_RUNS:
        xf, hf, _ = gmres_ref(lambda v: a @ v, b, iters, restart=restart, dot=forward_dot)
        xr, hr, _ = gmres_ref(lambda v: a @ v, b, iters, restart=restart, dot=reversed_dot)
        out.append((np.max(np.abs(xf - xr)) / np.max(np.abs(xf)), np.max(np.abs(hf - hr) / hf),
                    np.max(np.abs(hf - hr)) / hf[0]))
    return out


def test_gpu_tolerances_are_a_hundred_times_the_summation_spread():
    """The bounds tests/test_gpu_gmres.py holds the device to on the banded fixture, against what the order of the
    dot products alone moves in the restated loop.  Measured: 5 steps at restart 30 move x by 1.0e-15 of max |x| and
    the history by 7.9e-15 relative (bounds 1e-10 and 1e-10); 25 steps at restart 10 move x by 6.7e-16 and the history
    by 2.9e-12 relative, 7.9e-15 of hist[0] (bounds 1e-7, and 1e-8 hist[0] + 1e-4 relative)."""
    for (iters, restart, x_tol, h_abs, h_rel), (dx, dh_rel, dh_abs) in zip(BANDED_RUNS, banded_spread()):
        print(f"gmres spread, {iters} steps at restart {restart}: x {dx:.3e}, hist relative {dh_rel:.3e}, "
              f"hist / hist[0] {dh_abs:.3e}")
        assert 100.0 * dx <= x_tol
        assert 100.0 * dh_rel <= h_rel or 100.0 * dh_abs <= h_abs
