"""Every solver's steps on every SpMV route of csr_launch and spmm_launch, not on a band's x-window plan alone.

The other solver tests run banded and tridiagonal matrices under default knobs.  Here each route of ROUTES is forced as
test_gpu_scaling.py forces it for the bare product -- upload knobs, launch knobs, and a fingerprint from info() that
fails with "path not taken" -- on the matrices of test_solver_routes_host.py (a band with arrow rows at the long-row
limits, short scattered rows, tile matrices with stray entries and with arrow rows), and one handle per route, dtype and
kind of values serves every solver that kind is for:
    spd     cg, pcg (none and Jacobi), minres, cg_multi (k = 2, then 8, then 3 on the one handle, so the long rows'
            k-wide scratch grows and is then reused), Jacobi pcg_multi (k = 8), the Chebyshev apply of degree 3 (k = 1, 4)
    indef   minres
    nonsym  bicgstab, Jacobi pbicgstab, cgls with at = dev.transpose() built under the same upload knobs (its
            fingerprint is asserted too); the rect matrix is one more cgls case of its own
    lap     the exact gate
The k-wide solvers and the k = 4 apply see only the blocks and the long-row pieces: they run on xw-slots, gather-2048,
short and tile-packed.  cgls and the k = 1 apply always launch AUTO: they are skipped on the routes where AUTO is not the
route named -- "short" under STREAM (AUTO is the lane-group kernel there: the route "short-auto" runs everything through
it) and the three explicit variants, which serve the four solvers that take `variant` (cg, pcg, minres, bicgstab).

Checks.  (1) The exact gate: on lap with b = 3 x 1 every route must give q = 4 b exactly whatever its order of addition
(every partial sum is an integer below 2^24), so cg and pcg give the history [9 n, 0, 0], x = b / 4 bit for bit and
CONVERGED after one step, bicgstab stops at its half step with x = b / 4, cgls has alpha = 1 / 16 and x = b / 4,
cg_multi is exact in every column c_j x 1: a row dropped, counted twice, left unzeroed or short of a long-row piece
changes an integer.  MINRES multiplies b / |b|, which is no representable number: its first entry is exact, its x is held
to b / 4 within the measured tolerance below ("minres_lap").  (2) x and every history after 1, 2 and 3 steps against the
long-double loops of the other solver tests, within max(16 x MEASURED, 4 eps): test_gpu_solver_sizes.py's convention, with
MEASURED taken on the CPU against a reference that sums every row in the handle's dtype (test_solver_routes_host.py;
`python tests/test_gpu_solver_routes.py` prints the table, a CPU test recomputes its fp32 entries).  The Chebyshev apply
is held to _cheb_ref.apply_with_bound's own entry-wise bound.  (3) The same solve twice gives the same bits on every
route; xw-as-gather (the x-window handle launched with stream_kind = 0) gives xw-slots' bits and tile_gather_ahead = 1
gives tile-gather's, for every solver.  (4) After the solves the handle still multiplies: spmv passes the row gate under
the route's knobs."""
import contextlib
import functools
import os
import sys

if __name__ == "__main__":      # (run as a script, for the table: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import scipy.sparse as sps

import _cheb_ref
import sparsematrixvectormultiplication_amd as sp
import test_solver_routes_host as H
from _util import assert_parity, assert_parity_f32
from test_gpu_bicgstab import bicgstab_ref
from test_gpu_scaling import plan
from test_gpu_solver_sizes import differences

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
STEPS = H.STEPS
STREAM, AUTO = sp.CSR_STREAM, sp.CSR_AUTO
SUBWAVE = sp.CSR_VARIANTS["subwave"]
GATHER = dict(stream_local=0, stream_tile=0)


def long_rows_beyond(cap):
    return lambda i, lens: i["long_rows"] == int((lens > cap - 3).sum()) == {2048: 2, 8192: 1}[cap]


def x_window(i, lens):
    return i["stream_kernel"] == 1 and i["local_blocks"] > 0 and i["long_rows"] > 0


def gather(i, lens):
    return i["stream_kernel"] == 0 and i["local_blocks"] == 0 and i["tile_blocks"] == 0


def tiles(i, lens):
    return i["stream_kernel"] == 3 and i["tile_blocks"] > 0


def packed(i, lens):
    return (tiles(i, lens) and i["tile_staged_entries"] + i["tile_remainder_entries"] == i["tile_entries"]
            and i["tile_staged_cols"] > 0)


def gather_passes(i, lens):
    return tiles(i, lens) and i["tile_staged_entries"] == 0 and i["tile_expanded_entries"] == 0


def route(matrix, upload, fingerprint, variant=STREAM, launch=None, auto=True, wide=False):
    """auto: AUTO is this route (cgls and the k = 1 apply run); wide: the k-wide solvers run"""
    return dict(matrix=matrix, upload=upload, launch=launch or {}, fingerprint=fingerprint, variant=variant, auto=auto, wide=wide)


TILE = {k: v[1] for k, v in H.TILE_KNOBS.items()}
ROUTES = {
    "xw-pattern": route("band+arrow", dict(local_patterns=1), lambda i, n: x_window(i, n) and i["pattern_slots"] > 0),
    "xw-slots": route("band+arrow", dict(local_patterns=0), lambda i, n: x_window(i, n) and i["pattern_slots"] == 0, wide=True),
    "xw-as-gather": route("band+arrow", dict(local_patterns=0), lambda i, n: x_window(i, n) and i["pattern_slots"] == 0,
                          launch=dict(stream_kind=0)),
    "gather-2048": route("band+arrow", dict(stream_cap=2048, **GATHER),
                         lambda i, n: gather(i, n) and long_rows_beyond(2048)(i, n), wide=True),
    "gather-8192": route("band+arrow", dict(stream_cap=8192, **GATHER),
                         lambda i, n: gather(i, n) and long_rows_beyond(8192)(i, n)),
    "short": route("short", dict(stream_cap=2048, **GATHER),
                   lambda i, n: i["stream_kernel"] == 2 and i["auto_variant"] == SUBWAVE, auto=False, wide=True),
    "short-auto": route("short", dict(stream_cap=2048, **GATHER),
                        lambda i, n: i["stream_kernel"] == 2 and i["auto_variant"] == SUBWAVE, variant=AUTO),
    "tile-packed": route("tile", TILE["tile-packed"], packed, wide=True),
    "tile-remainder": route("tile+stray", TILE["tile-remainder"], lambda i, n: packed(i, n) and i["tile_remainder_entries"] > 0),
    "tile-gather": route("tile", TILE["tile-gather"], gather_passes),
    "tile-gather-ahead": route("tile", TILE["tile-gather"], gather_passes, launch=dict(tile_gather_ahead=1)),
    "tile-expanded": route("tile", TILE["tile-expanded"],
                           lambda i, n: tiles(i, n) and i["tile_expanded_entries"] >= i["tile_entries"] > 0),
    "tile-long": route("tile+arrow", TILE["tile-long"],
                       lambda i, n: tiles(i, n) and i["tile_long_rows"] > 0 and i["tile_long_items"] > 0),
    "tile-split": route("tile+arrow", TILE["tile-split"], lambda i, n: tiles(i, n) and i["tile_split_rows"] > 0),
}
for _name in ("thread_row", "wave_row", "subwave"):
    ROUTES["explicit-" + _name] = route("band+arrow", {}, lambda i, n: i["lanes_per_row"] >= 2 and i["long_rows"] > 0,
                                        variant=sp.CSR_VARIANTS[_name], auto=False)
SAME_BITS = [("xw-as-gather", "xw-slots"), ("tile-gather-ahead", "tile-gather")]
RECT_KNOBS = dict(stream_tile=1, tile_rows=1024, tile_expand=0)      # tile_cases' "gather passes"

BY_AUTO = ("cgls",)           # (no `variant` argument: launched through AUTO)
WIDE = ("cg_multi", "pcg_multi")
CG_MULTI_KS = (2, 8, 3)       # in this order: the long rows' scratch grows at 8 and is reused at 3
CHEB_DEGREE, CHEB_K = 3, 4

# Largest difference between the long-double loop and the same recurrence in the handle's dtype with every product
# rounded and every row summed in that dtype, in entry order and in reverse entry order (the larger of the two), over 1,
# 2 and 3 steps; x relative to max |x|, history entries relative to the first one.  Taken on the CPU by
# test_solver_routes_host.measure; `python tests/test_gpu_solver_routes.py` prints this table.  The tolerance is 16 times
# the figure and at least 4 eps.
MEASURED = {
    ('cg', 'float64', 'band+arrow'): 5.506e-15,   # 2 steps, reverse order (x 5.506e-15, history 4.065e-17) -> tolerance 8.810e-14
    ('pcg', 'float64', 'band+arrow'): 5.530e-15,   # 2 steps, reverse order (x 5.530e-15, history 4.065e-17) -> tolerance 8.848e-14
    ('pcg_jacobi', 'float64', 'band+arrow'): 5.149e-16,   # 3 steps, reverse order (x 5.149e-16, history 2.391e-18) -> tolerance 8.238e-15
    ('minres', 'float64', 'band+arrow'): 3.445e-15,   # 3 steps, entry order (x 3.445e-15, history 2.391e-18) -> tolerance 5.513e-14
    ('minres_indef', 'float64', 'band+arrow'): 4.882e-15,   # 2 steps, reverse order (x 4.882e-15, history 6.887e-16) -> tolerance 7.811e-14
    ('bicgstab', 'float64', 'band+arrow'): 2.091e-15,   # 2 steps, entry order (x 2.091e-15, history 1.794e-18) -> tolerance 3.345e-14
    ('pbicgstab', 'float64', 'band+arrow'): 6.436e-16,   # 3 steps, entry order (x 6.436e-16, history 2.335e-21) -> tolerance 1.030e-14
    ('cgls', 'float64', 'band+arrow'): 1.081e-14,   # 3 steps, reverse order (x 1.081e-14, history 2.866e-15) -> tolerance 1.729e-13
    ('cg_multi', 'float64', 'band+arrow'): 6.015e-15,   # 3 steps, reverse order (x 6.015e-15, history 3.061e-16) -> tolerance 9.624e-14
    ('pcg_multi', 'float64', 'band+arrow'): 5.446e-16,   # 2 steps, reverse order (x 5.446e-16, history 1.858e-16) -> tolerance 8.713e-15
    ('minres_lap', 'float64', 'band+arrow'): 3.656e-14,   # 1 steps, reverse order (x 3.656e-14, history 1.017e-23) -> tolerance 5.850e-13
    ('cg', 'float64', 'short'): 3.687e-16,   # 2 steps, reverse order (x 3.687e-16, history 8.571e-18) -> tolerance 5.899e-15
    ('pcg', 'float64', 'short'): 3.906e-16,   # 3 steps, entry order (x 3.906e-16, history 8.571e-18) -> tolerance 6.249e-15
    ('pcg_jacobi', 'float64', 'short'): 3.645e-16,   # 3 steps, reverse order (x 3.645e-16, history 2.562e-18) -> tolerance 5.832e-15
    ('minres', 'float64', 'short'): 4.501e-16,   # 2 steps, reverse order (x 4.501e-16, history 2.679e-19) -> tolerance 7.202e-15
    ('minres_indef', 'float64', 'short'): 1.720e-14,   # 1 steps, entry order (x 1.720e-14, history 0.000e+00) -> tolerance 2.752e-13
    ('bicgstab', 'float64', 'short'): 4.541e-16,   # 3 steps, reverse order (x 4.541e-16, history 1.339e-19) -> tolerance 7.266e-15
    ('pbicgstab', 'float64', 'short'): 3.302e-16,   # 3 steps, reverse order (x 3.302e-16, history 6.696e-20) -> tolerance 5.283e-15
    ('cgls', 'float64', 'short'): 6.410e-16,   # 2 steps, entry order (x 6.410e-16, history 1.813e-16) -> tolerance 1.026e-14
    ('cg_multi', 'float64', 'short'): 4.764e-16,   # 2 steps, entry order (x 4.764e-16, history 1.375e-16) -> tolerance 7.623e-15
    ('pcg_multi', 'float64', 'short'): 5.158e-16,   # 1 steps, entry order (x 5.158e-16, history 3.289e-16) -> tolerance 8.253e-15
    ('minres_lap', 'float64', 'short'): 1.480e-15,   # 1 steps, entry order (x 1.480e-15, history 1.175e-30) -> tolerance 2.368e-14
    ('cg', 'float64', 'tile'): 5.493e-16,   # 2 steps, reverse order (x 5.493e-16, history 1.814e-16) -> tolerance 8.789e-15
    ('pcg', 'float64', 'tile'): 5.825e-16,   # 2 steps, reverse order (x 5.825e-16, history 7.087e-18) -> tolerance 9.320e-15
    ('pcg_jacobi', 'float64', 'tile'): 5.352e-16,   # 3 steps, reverse order (x 5.352e-16, history 1.121e-16) -> tolerance 8.564e-15
    ('minres', 'float64', 'tile'): 5.631e-16,   # 2 steps, reverse order (x 5.631e-16, history 0.000e+00) -> tolerance 9.010e-15
    ('minres_indef', 'float64', 'tile'): 6.970e-15,   # 1 steps, entry order (x 6.970e-15, history 0.000e+00) -> tolerance 1.115e-13
    ('bicgstab', 'float64', 'tile'): 4.876e-16,   # 3 steps, reverse order (x 4.876e-16, history 1.081e-23) -> tolerance 7.801e-15
    ('pbicgstab', 'float64', 'tile'): 4.566e-16,   # 2 steps, entry order (x 4.566e-16, history 1.365e-20) -> tolerance 7.305e-15
    ('cgls', 'float64', 'tile'): 7.664e-16,   # 1 steps, entry order (x 7.664e-16, history 1.823e-17) -> tolerance 1.226e-14
    ('cg_multi', 'float64', 'tile'): 6.433e-16,   # 3 steps, entry order (x 6.433e-16, history 1.829e-16) -> tolerance 1.029e-14
    ('pcg_multi', 'float64', 'tile'): 5.494e-16,   # 3 steps, reverse order (x 5.494e-16, history 1.131e-16) -> tolerance 8.791e-15
    ('minres_lap', 'float64', 'tile'): 4.737e-15,   # 1 steps, entry order (x 4.737e-15, history 2.084e-29) -> tolerance 7.579e-14
    ('cg', 'float64', 'tile+stray'): 5.498e-16,   # 3 steps, reverse order (x 5.498e-16, history 1.814e-16) -> tolerance 8.797e-15
    ('pcg', 'float64', 'tile+stray'): 5.338e-16,   # 3 steps, reverse order (x 5.338e-16, history 2.835e-18) -> tolerance 8.541e-15
    ('pcg_jacobi', 'float64', 'tile+stray'): 4.660e-16,   # 3 steps, entry order (x 4.660e-16, history 1.123e-16) -> tolerance 7.457e-15
    ('minres', 'float64', 'tile+stray'): 6.158e-16,   # 3 steps, entry order (x 6.158e-16, history 9.922e-18) -> tolerance 9.853e-15
    ('minres_indef', 'float64', 'tile+stray'): 4.456e-15,   # 1 steps, entry order (x 4.456e-15, history 0.000e+00) -> tolerance 7.130e-14
    ('bicgstab', 'float64', 'tile+stray'): 5.511e-16,   # 3 steps, reverse order (x 5.511e-16, history 1.081e-23) -> tolerance 8.818e-15
    ('pbicgstab', 'float64', 'tile+stray'): 4.585e-16,   # 3 steps, entry order (x 4.585e-16, history 1.107e-20) -> tolerance 7.336e-15
    ('cgls', 'float64', 'tile+stray'): 6.610e-16,   # 2 steps, reverse order (x 6.610e-16, history 1.167e-16) -> tolerance 1.058e-14
    ('cg_multi', 'float64', 'tile+stray'): 6.585e-16,   # 2 steps, reverse order (x 6.585e-16, history 1.829e-16) -> tolerance 1.054e-14
    ('pcg_multi', 'float64', 'tile+stray'): 5.242e-16,   # 3 steps, entry order (x 5.242e-16, history 2.263e-16) -> tolerance 8.388e-15
    ('minres_lap', 'float64', 'tile+stray'): 4.737e-15,   # 1 steps, entry order (x 4.737e-15, history 2.084e-29) -> tolerance 7.579e-14
    ('cg', 'float64', 'tile+arrow'): 1.300e-14,   # 3 steps, reverse order (x 1.300e-14, history 1.814e-16) -> tolerance 2.081e-13
    ('pcg', 'float64', 'tile+arrow'): 1.304e-14,   # 3 steps, reverse order (x 1.304e-14, history 4.110e-17) -> tolerance 2.086e-13
    ('pcg_jacobi', 'float64', 'tile+arrow'): 4.436e-16,   # 3 steps, reverse order (x 4.436e-16, history 6.809e-21) -> tolerance 7.097e-15
    ('minres', 'float64', 'tile+arrow'): 2.340e-14,   # 3 steps, entry order (x 2.340e-14, history 1.347e-17) -> tolerance 3.744e-13
    ('minres_indef', 'float64', 'tile+arrow'): 3.011e-14,   # 1 steps, entry order (x 3.011e-14, history 0.000e+00) -> tolerance 4.818e-13
    ('bicgstab', 'float64', 'tile+arrow'): 4.007e-14,   # 3 steps, reverse order (x 4.007e-14, history 1.967e-17) -> tolerance 6.411e-13
    ('pbicgstab', 'float64', 'tile+arrow'): 9.020e-16,   # 2 steps, reverse order (x 9.020e-16, history 1.092e-19) -> tolerance 1.443e-14
    ('cgls', 'float64', 'tile+arrow'): 1.409e-13,   # 3 steps, entry order (x 1.409e-13, history 2.906e-14) -> tolerance 2.254e-12
    ('cg_multi', 'float64', 'tile+arrow'): 1.393e-14,   # 3 steps, reverse order (x 1.393e-14, history 1.829e-16) -> tolerance 2.229e-13
    ('pcg_multi', 'float64', 'tile+arrow'): 8.386e-16,   # 3 steps, reverse order (x 8.386e-16, history 1.127e-16) -> tolerance 1.342e-14
    ('minres_lap', 'float64', 'tile+arrow'): 8.290e-15,   # 1 steps, entry order (x 8.290e-15, history 3.810e-25) -> tolerance 1.326e-13
    ('cgls', 'float64', 'rect'): 4.132e-16,   # 3 steps, entry order (x 4.132e-16, history 1.268e-16) -> tolerance 6.611e-15
    ('cg', 'float32', 'band+arrow'): 4.991e-07,   # 2 steps, reverse order (x 4.991e-07, history 4.416e-09) -> tolerance 7.986e-06
    ('pcg', 'float32', 'band+arrow'): 4.991e-07,   # 2 steps, reverse order (x 4.991e-07, history 4.416e-09) -> tolerance 7.986e-06
    ('pcg_jacobi', 'float32', 'band+arrow'): 2.242e-07,   # 3 steps, reverse order (x 2.242e-07, history 1.707e-10) -> tolerance 3.587e-06
    ('minres', 'float32', 'band+arrow'): 3.790e-06,   # 3 steps, reverse order (x 3.790e-06, history 1.207e-08) -> tolerance 6.064e-05
    ('minres_indef', 'float32', 'band+arrow'): 3.996e-06,   # 3 steps, reverse order (x 3.996e-06, history 5.356e-07) -> tolerance 6.393e-05
    ('bicgstab', 'float32', 'band+arrow'): 1.650e-06,   # 1 steps, reverse order (x 1.650e-06, history 8.021e-09) -> tolerance 2.640e-05
    ('pbicgstab', 'float32', 'band+arrow'): 3.190e-07,   # 1 steps, entry order (x 3.190e-07, history 4.807e-13) -> tolerance 5.105e-06
    ('cgls', 'float32', 'band+arrow'): 1.564e-05,   # 1 steps, reverse order (x 2.561e-07, history 1.564e-05) -> tolerance 2.503e-04
    ('cg_multi', 'float32', 'band+arrow'): 2.715e-06,   # 2 steps, reverse order (x 2.715e-06, history 3.424e-08) -> tolerance 4.344e-05
    ('pcg_multi', 'float32', 'band+arrow'): 3.463e-07,   # 2 steps, entry order (x 3.463e-07, history 7.571e-10) -> tolerance 5.541e-06
    ('minres_lap', 'float32', 'band+arrow'): 1.113e-05,   # 1 steps, entry order (x 1.113e-05, history 1.989e-06) -> tolerance 1.780e-04
    ('cg', 'float32', 'short'): 1.957e-07,   # 3 steps, reverse order (x 1.957e-07, history 1.083e-10) -> tolerance 3.131e-06
    ('pcg', 'float32', 'short'): 1.957e-07,   # 3 steps, reverse order (x 1.957e-07, history 1.083e-10) -> tolerance 3.131e-06
    ('pcg_jacobi', 'float32', 'short'): 2.003e-07,   # 3 steps, reverse order (x 2.003e-07, history 3.562e-11) -> tolerance 3.204e-06
    ('minres', 'float32', 'short'): 2.469e-07,   # 2 steps, reverse order (x 2.469e-07, history 2.306e-10) -> tolerance 3.950e-06
    ('minres_indef', 'float32', 'short'): 3.173e-07,   # 1 steps, entry order (x 3.173e-07, history 2.242e-12) -> tolerance 5.077e-06
    ('bicgstab', 'float32', 'short'): 1.804e-07,   # 3 steps, reverse order (x 1.804e-07, history 8.548e-12) -> tolerance 2.887e-06
    ('pbicgstab', 'float32', 'short'): 1.718e-07,   # 3 steps, entry order (x 1.718e-07, history 3.756e-12) -> tolerance 2.748e-06
    ('cgls', 'float32', 'short'): 2.535e-07,   # 3 steps, reverse order (x 2.535e-07, history 5.775e-10) -> tolerance 4.056e-06
    ('cg_multi', 'float32', 'short'): 2.112e-07,   # 3 steps, reverse order (x 2.112e-07, history 2.731e-10) -> tolerance 3.379e-06
    ('pcg_multi', 'float32', 'short'): 2.043e-07,   # 3 steps, entry order (x 2.043e-07, history 2.993e-10) -> tolerance 3.269e-06
    ('minres_lap', 'float32', 'short'): 7.947e-08,   # 1 steps, entry order (x 7.947e-08, history 1.081e-14) -> tolerance 1.272e-06
    ('cg', 'float32', 'tile'): 2.772e-07,   # 3 steps, reverse order (x 2.772e-07, history 4.489e-11) -> tolerance 4.435e-06
    ('pcg', 'float32', 'tile'): 2.772e-07,   # 3 steps, reverse order (x 2.772e-07, history 4.489e-11) -> tolerance 4.435e-06
    ('pcg_jacobi', 'float32', 'tile'): 2.748e-07,   # 3 steps, entry order (x 2.748e-07, history 9.146e-11) -> tolerance 4.396e-06
    ('minres', 'float32', 'tile'): 3.126e-07,   # 3 steps, entry order (x 3.126e-07, history 7.793e-11) -> tolerance 5.002e-06
    ('minres_indef', 'float32', 'tile'): 3.280e-07,   # 3 steps, reverse order (x 3.280e-07, history 3.849e-12) -> tolerance 5.248e-06
    ('bicgstab', 'float32', 'tile'): 2.635e-07,   # 2 steps, reverse order (x 2.635e-07, history 1.440e-12) -> tolerance 4.217e-06
    ('pbicgstab', 'float32', 'tile'): 2.570e-07,   # 3 steps, entry order (x 2.570e-07, history 5.247e-13) -> tolerance 4.111e-06
    ('cgls', 'float32', 'tile'): 3.166e-07,   # 2 steps, reverse order (x 3.166e-07, history 2.787e-10) -> tolerance 5.065e-06
    ('cg_multi', 'float32', 'tile'): 2.851e-07,   # 3 steps, entry order (x 2.851e-07, history 1.521e-10) -> tolerance 4.561e-06
    ('pcg_multi', 'float32', 'tile'): 3.091e-07,   # 3 steps, reverse order (x 3.091e-07, history 1.568e-10) -> tolerance 4.946e-06
    ('minres_lap', 'float32', 'tile'): 1.589e-07,   # 1 steps, entry order (x 1.589e-07, history 2.029e-14) -> tolerance 2.543e-06
    ('cg', 'float32', 'tile+stray'): 3.139e-07,   # 3 steps, reverse order (x 3.139e-07, history 1.447e-10) -> tolerance 5.023e-06
    ('pcg', 'float32', 'tile+stray'): 3.139e-07,   # 3 steps, reverse order (x 3.139e-07, history 1.447e-10) -> tolerance 5.023e-06
    ('pcg_jacobi', 'float32', 'tile+stray'): 2.518e-07,   # 3 steps, entry order (x 2.518e-07, history 1.672e-10) -> tolerance 4.029e-06
    ('minres', 'float32', 'tile+stray'): 3.173e-07,   # 2 steps, entry order (x 3.173e-07, history 2.146e-11) -> tolerance 5.076e-06
    ('minres_indef', 'float32', 'tile+stray'): 3.193e-07,   # 1 steps, reverse order (x 3.193e-07, history 4.550e-12) -> tolerance 5.108e-06
    ('bicgstab', 'float32', 'tile+stray'): 2.494e-07,   # 3 steps, entry order (x 2.494e-07, history 2.554e-13) -> tolerance 3.990e-06
    ('pbicgstab', 'float32', 'tile+stray'): 2.554e-07,   # 3 steps, entry order (x 2.554e-07, history 5.312e-13) -> tolerance 4.086e-06
    ('cgls', 'float32', 'tile+stray'): 2.719e-07,   # 2 steps, reverse order (x 2.719e-07, history 6.302e-10) -> tolerance 4.350e-06
    ('cg_multi', 'float32', 'tile+stray'): 3.038e-07,   # 2 steps, entry order (x 3.038e-07, history 1.358e-10) -> tolerance 4.861e-06
    ('pcg_multi', 'float32', 'tile+stray'): 2.919e-07,   # 3 steps, reverse order (x 2.919e-07, history 2.836e-10) -> tolerance 4.670e-06
    ('minres_lap', 'float32', 'tile+stray'): 1.589e-07,   # 1 steps, entry order (x 1.589e-07, history 2.029e-14) -> tolerance 2.543e-06
    ('cg', 'float32', 'tile+arrow'): 2.056e-06,   # 2 steps, entry order (x 2.056e-06, history 6.467e-09) -> tolerance 3.290e-05
    ('pcg', 'float32', 'tile+arrow'): 2.056e-06,   # 2 steps, entry order (x 2.056e-06, history 6.467e-09) -> tolerance 3.290e-05
    ('pcg_jacobi', 'float32', 'tile+arrow'): 2.586e-07,   # 3 steps, entry order (x 2.586e-07, history 1.817e-10) -> tolerance 4.137e-06
    ('minres', 'float32', 'tile+arrow'): 6.681e-06,   # 3 steps, reverse order (x 6.681e-06, history 4.649e-09) -> tolerance 1.069e-04
    ('minres_indef', 'float32', 'tile+arrow'): 1.978e-06,   # 3 steps, entry order (x 1.978e-06, history 9.461e-08) -> tolerance 3.165e-05
    ('bicgstab', 'float32', 'tile+arrow'): 2.577e-06,   # 3 steps, entry order (x 2.577e-06, history 1.652e-09) -> tolerance 4.123e-05
    ('pbicgstab', 'float32', 'tile+arrow'): 2.945e-07,   # 3 steps, reverse order (x 2.945e-07, history 3.582e-12) -> tolerance 4.712e-06
    ('cgls', 'float32', 'tile+arrow'): 8.261e-05,   # 3 steps, entry order (x 8.261e-05, history 1.775e-05) -> tolerance 1.322e-03
    ('cg_multi', 'float32', 'tile+arrow'): 8.803e-06,   # 3 steps, reverse order (x 8.803e-06, history 3.941e-08) -> tolerance 1.409e-04
    ('pcg_multi', 'float32', 'tile+arrow'): 4.754e-07,   # 3 steps, reverse order (x 4.754e-07, history 1.089e-10) -> tolerance 7.607e-06
    ('minres_lap', 'float32', 'tile+arrow'): 1.589e-07,   # 1 steps, entry order (x 1.589e-07, history 2.729e-08) -> tolerance 2.543e-06
    ('cgls', 'float32', 'rect'): 1.936e-07,   # 2 steps, entry order (x 1.936e-07, history 7.341e-10) -> tolerance 3.097e-06
}


def tolerance(solver, dtype, name):
    return max(16.0 * MEASURED[(solver, np.dtype(dtype).name, name)], 4.0 * float(np.finfo(dtype).eps))


# ---------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def reference_runs(solver, name, dtype):
    """iters -> (x, the histories) of the long-double loop; shared by the routes of a matrix, never written to"""
    prob = H.problem(solver, name, dtype)
    return {iters: H.loop(solver, prob, iters) for iters in STEPS}


@functools.lru_cache(maxsize=None)
def cheb_setup(name, dtype):
    M, N, rp, col = H.matrix(name)
    a = sps.csr_matrix((H.held(name, "spd", dtype).astype(np.float64), col, rp), shape=(M, N))
    return a, _cheb_ref.inverse_diagonal(a, dtype), _cheb_ref.interval(a)


# ---------------------------------------------------------------- handles
@contextlib.contextmanager
def handles(route_id, kind, dtype, transpose=False, jacobi=False, cheb=False, name=None, knobs=None):
    """(dev, at, Jacobi, Chebyshev) of one route: uploaded and built under the route's upload knobs, fingerprints
    asserted, then the route's launch knobs for the body"""
    r = ROUTES[route_id] if route_id else dict(matrix=name, upload=knobs, launch={}, fingerprint=gather_passes)
    name = r["matrix"]
    M, N, rp, col = H.matrix(name)
    lens = np.diff(rp)
    made = []
    try:
        with sp.tuning(**r["upload"]):
            dev = sp.CsrDevice(M, N, rp, col, H.held(name, kind, dtype))
            made.append(dev)
            info = dev.info()
            assert r["fingerprint"](info, lens), f"{route_id or name}: path not taken: {plan(info)}"
            at = J = P = None
            if transpose:
                at = dev.transpose()
                made.append(at)
                if M == N:   # (the pattern is symmetric: the transpose is the same route)
                    assert r["fingerprint"](at.info(), lens), f"{route_id} transpose: path not taken: {plan(at.info())}"
            if jacobi:
                J = dev.preconditioner("jacobi")
                made.append(J)
            if cheb:
                P = dev.preconditioner("chebyshev", degree=CHEB_DEGREE)
                made.append(P)
        with sp.tuning(**r["launch"]):
            yield dev, at, J, P
    finally:
        for obj in reversed(made):
            obj.close()


def solve(solver, dev, at, J, b, iters, variant):
    """(x, the histories) of one device solve"""
    if solver == "cg":
        x, h, _ = dev.cg(b, iters, variant)
        return x, [h]
    if solver in ("pcg", "pcg_jacobi"):
        x, rr, rz, _, _ = dev.pcg(b, iters, precond=J if solver == "pcg_jacobi" else None, variant=variant)
        return x, [rr, rz]
    if solver in ("minres", "minres_indef"):
        x, h, _, _ = dev.minres(b, iters, variant=variant)
        return x, [h]
    if solver in ("bicgstab", "pbicgstab"):
        x, h, _, _ = dev.bicgstab(b, iters, variant=variant, precond=J if solver == "pbicgstab" else None)
        return x, [h]
    if solver == "cgls":
        x, ss, rr, _, _ = dev.cgls(b, iters, at=at)
        return x, [ss, rr]
    if solver == "cg_multi":
        X, h, _, _ = dev.cg_multi(b, iters)
        return X, [h]
    assert solver == "pcg_multi"
    X, rr, rz, _, _ = dev.pcg_multi(b, iters, precond=J)
    return X, [rr, rz]


def bits(got):
    return [got[0].tobytes()] + [h.tobytes() for h in got[1]]


def first_columns(run, k):
    return run[0][:, :k], [h[:, :k] for h in run[1]]


def check_solver(solver, route_id, dev, at, J, dtype, out):
    """1, 2 and 3 steps against the long-double loop within tolerance(), and the last solve again: the same bits.
    out[solver...] keeps the bits of the 3-step solve for the identities between routes."""
    r = ROUTES[route_id] if route_id else dict(matrix="rect", variant=AUTO)
    name = r["matrix"]
    tol = tolerance(solver, dtype, name)
    refs = reference_runs(solver, name, dtype)
    b = H.problem(solver, name, dtype)[5]
    for k in (CG_MULTI_KS if solver == "cg_multi" else (None,)):
        bk = b if k is None else np.ascontiguousarray(b[:, :k])
        for iters in STEPS:
            got = solve(solver, dev, at, J, bk, iters, r["variant"])
            assert got[0].dtype == dtype and got[0].shape == bk.shape[:0] + (dev.N,) + bk.shape[1:]
            ref = refs[iters] if k is None else first_columns(refs[iters], k)
            dx, dh = differences(got, ref)
            print(f"{route_id or name} {solver} {np.dtype(dtype).name} k={k} {iters} steps: x {dx:.3e} hist {dh:.3e} "
                  f"(tolerance {tol:.3e})")
            assert dx <= tol and dh <= tol, (route_id, solver, k, iters, dx, dh, tol)
        again = solve(solver, dev, at, J, bk, STEPS[-1], r["variant"])
        assert bits(again) == bits(got), (route_id, solver, k, "the same solve twice")
        out[(solver, k)] = bits(got)


def check_cheb(route_id, dev, P, dtype, ks, out):
    name = ROUTES[route_id]["matrix"]
    a, g, (lo, hi) = cheb_setup(name, dtype)
    for k in ks:
        r = H.rhs(dev.M, dtype, 40 + k, None if k == 1 else k)
        z = P.apply(r) if k == 1 else P.apply_multi(r)
        z_ref, bound = _cheb_ref.apply_with_bound(a, g, r.astype(np.float64), CHEB_DEGREE, lo, hi, dtype)
        err = np.abs(z.astype(np.float64) - z_ref)
        print(f"{route_id} chebyshev k={k} {np.dtype(dtype).name}: max |z - ref| / bound = "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert z.dtype == dtype and np.all(np.isfinite(z)) and np.all(err <= bound), (route_id, k, int(np.argmax(err - bound)))
        assert (P.apply(r) if k == 1 else P.apply_multi(r)).tobytes() == z.tobytes(), (route_id, k, "the same apply twice")
        out[("chebyshev", k)] = [z.tobytes()]


def still_multiplies(oracle, route_id, dev, kind, dtype):
    """(4) the handle after its solves: one product under the route's knobs, row by row against the oracle"""
    r = ROUTES[route_id]
    M, N, rp, col = H.matrix(r["matrix"])
    val = H.held(r["matrix"], kind, dtype)
    x = H.rhs(N, dtype, 77)
    y = dev.spmv(x, r["variant"])
    what = f"{route_id} {kind} {np.dtype(dtype).name}: spmv after the solves"
    if dtype == np.float64:
        assert_parity(y, oracle.csr_serial(rp, col, val, x), rp, col, val, x, what=what)
    else:
        assert_parity_f32(y, oracle.csr_f32_accum64(rp, col, val, x), rp, col, val, x, what=what)


def run_route(oracle, route_id, dtype):
    """every solver of the route on its three handles -> {(solver, k): the bits of its 3-step solve}"""
    r = ROUTES[route_id]
    out = {}
    with handles(route_id, "spd", dtype, jacobi=True, cheb=True) as (dev, _, J, P):
        for solver in ("cg", "pcg", "pcg_jacobi", "minres") + (WIDE if r["wide"] else ()):
            check_solver(solver, route_id, dev, None, J, dtype, out)
        check_cheb(route_id, dev, P, dtype, ((1,) if r["auto"] else ()) + ((CHEB_K,) if r["wide"] else ()), out)
        still_multiplies(oracle, route_id, dev, "spd", dtype)
    with handles(route_id, "indef", dtype) as (dev, _, _, _):
        check_solver("minres_indef", route_id, dev, None, None, dtype, out)
        still_multiplies(oracle, route_id, dev, "indef", dtype)
    with handles(route_id, "nonsym", dtype, transpose=r["auto"], jacobi=True) as (dev, at, J, _):
        for solver in ("bicgstab", "pbicgstab") + (BY_AUTO if r["auto"] else ()):
            check_solver(solver, route_id, dev, at, J, dtype, out)
        still_multiplies(oracle, route_id, dev, "nonsym", dtype)
    return out


# ---------------------------------------------------------------- (1) the exact gate
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("route_id", sorted(ROUTES))
def test_exact_gate(gpu, route_id, dtype):
    """lap, b = 3 x 1: q = 4 b exactly on every route, so one step closes every solver in integers (module docstring).
    MINRES: first entry exact, x = b / 4 within tolerance("minres_lap"): at most 5.9e-13 (fp64) and 1.8e-4 (fp32), both
    on band+arrow -- the rounding of (4 + d) v - d v in rows of up to 8193 entries."""
    r = ROUTES[route_id]
    M = H.matrix(r["matrix"])[0]
    c = H.C_EXACT
    b = np.full(M, c, dtype)
    quarter = np.full(M, c / 4.0, dtype).tobytes()
    rr0 = float(M * c * c)
    with handles(route_id, "lap", dtype, transpose=r["auto"]) as (dev, at, _, _):
        for _ in range(2):       # (the second round: nothing left over from the first)
            x, h, _ = dev.cg(b, 2, r["variant"])
            assert h.tolist() == [rr0, 0.0, 0.0] and x.tobytes() == quarter, (route_id, "cg", h.tolist())
            x, rr, rz, info, _ = dev.pcg(b, 2, variant=r["variant"])
            assert rr.tolist() == [rr0, 0.0, 0.0] and rz.tolist() == [rr0, 0.0, 0.0], (route_id, "pcg", rr.tolist(), rz.tolist())
            assert info == {"steps": 1, "status": sp.PCG_CONVERGED} and x.tobytes() == quarter, (route_id, "pcg", info)
            x, h, info, _ = dev.bicgstab(b, 2, variant=r["variant"])
            x_ref, h_ref, info_ref = bicgstab_ref(lambda v: 4.0 * v, b.astype(np.float64), 2)
            assert info == info_ref == {"steps": 1, "status": sp.BICG_CONVERGED, "half_step": 1}, (route_id, "bicgstab", info)
            assert h.tobytes() == h_ref.tobytes() and h[0] == rr0 and x.tobytes() == quarter, (route_id, "bicgstab", h.tolist())
            x, h, info, _ = dev.minres(b, 1, variant=r["variant"])
            tol = tolerance("minres_lap", dtype, r["matrix"])
            dx = float(np.max(np.abs(x.astype(np.float64) - c / 4.0)) / (c / 4.0))
            print(f"{route_id} minres on lap {np.dtype(dtype).name}: x {dx:.3e} hist {h[1] / h[0]:.3e} (tolerance {tol:.3e})")
            assert h[0] == rr0 and dx <= tol and 0.0 <= h[1] <= tol * rr0, (route_id, "minres", dx, h.tolist(), tol)
            if r["auto"]:
                x, ss, rr, info, _ = dev.cgls(b, 2, at=at)
                assert ss.tolist() == [16.0 * rr0, 0.0, 0.0] and rr.tolist() == [rr0, 0.0, 0.0], (route_id, "cgls", ss, rr)
                assert info == {"steps": 1, "status": sp.CGLS_CONVERGED} and x.tobytes() == quarter, (route_id, "cgls", info)
            if r["wide"]:
                for k in CG_MULTI_KS:
                    cs = np.array(H.C_COLUMNS[:k], dtype=np.float64)
                    B = np.ascontiguousarray(np.tile(cs, (M, 1)).astype(dtype))
                    X, h, done, _ = dev.cg_multi(B, 2)
                    assert h[0].tolist() == (M * cs * cs).tolist() and np.all(h[1:] == 0.0), (route_id, "cg_multi", k, h.tolist())
                    assert done.tolist() == [1] * k and X.tobytes() == (B / dtype(4)).tobytes(), (route_id, "cg_multi", k, done)


# ---------------------------------------------------------------- (2), (3), (4) on every route
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("route_id", sorted(ROUTES))
def test_steps_match_the_long_double_loops(gpu, oracle, route_id, dtype):
    """1, 2 and 3 steps of every solver of the route against the long-double loops within tolerance(); every solve and
    every apply twice: the same bits; the Chebyshev apply within its running bound; the handle's spmv after the solves
    through the row gate."""
    run_route(oracle, route_id, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("route_id,base", SAME_BITS)
def test_routes_that_must_give_the_same_bits(gpu, oracle, route_id, base, dtype):
    """the x-window kernels give the gather kernels' bits, so the x-window handle launched with
    stream_kind = 0 gives xw-slots' bits for every solver; gathering one pass early (tile_gather_ahead = 1) changes
    no bit of tile-gather's."""
    one, two = run_route(oracle, route_id, dtype), run_route(oracle, base, dtype)
    assert set(one) <= set(two)
    for key in one:
        assert one[key] == two[key], (route_id, base, key)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_cgls_on_the_rect_matrix_through_gather_passes(gpu, dtype):
    """CGLS on the 7001 x 2 000 003 "gather passes" matrix of test_gpu_scaling.tile_cases: A through the tile kernel's
    gather passes, its transpose (2 000 003 rows) as dev.transpose() builds it under the same knobs."""
    with handles(None, "nonsym", dtype, transpose=True, name="rect", knobs=RECT_KNOBS) as (dev, at, _, _):
        print("rect transpose:", plan(at.info()))
        check_solver("cgls", None, dev, at, None, dtype, {})


# ---------------------------------------------------------------- the CPU measurement behind MEASURED
def print_measured():
    for dtype in DTYPES:
        for solver, name in H.measured_cases():
            w, iters, order, dx, dh = H.measure(solver, name, dtype)
            key = (solver, np.dtype(dtype).name, name)
            print(f"    {key!r}: {w:.3e},   # {iters} steps, {order} order (x {dx:.3e}, history {dh:.3e}) -> tolerance "
                  f"{max(16 * w, 4 * float(np.finfo(dtype).eps)):.3e}", flush=True)


if __name__ == "__main__":
    print_measured()
