"""GPU: Y = A X for k vectors per pass over an HLL slab (spmv_hip_hll_spmm*), column by column against the reference's
goldens and the oracle (column j of A X is A X[:, j]; fp64 gate 1e-10, assert_parity)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import assert_parity, banded_csr, coo_from_csr, random_csr
from conftest import GOLDEN_CASES, ROOT, golden_path, load_golden

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 7, 8, 9, 16, 33, 64)


class DeviceBuffer:
    """spmv_hip_malloc'd bytes, freed on exit."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        assert sp.lib().spmv_hip_malloc(C.byref(self.p), int(nbytes)) == 0
        self.nbytes = int(nbytes)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        sp.lib().spmv_hip_free(self.p)

    def at(self, offset=0):
        return self.p.value + offset

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        assert sp.lib().spmv_hip_memcpy_h2d(C.c_void_p(self.at(offset)), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def poison(self):
        assert sp.lib().spmv_hip_memset(self.p, 0xFF, self.nbytes) == 0  # NaN everywhere

    def download(self, shape, offset=0):
        sp.hip_sync()
        out = np.empty(shape)
        assert offset + out.nbytes <= self.nbytes
        assert sp.lib().spmv_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.at(offset)), out.nbytes) == 0
        return out


def hll_of(M, N, rp, col, val):
    r, c, v = coo_from_csr(rp, col, val)
    return sp.convert_to_hll(sp.PreMatrix.from_arrays(M, N, r, c, v))


def check_columns(oracle, Y, X, rp, col, val, what, rows=None):
    """Every column of Y against the oracle on the same column of X (rows: the handle's row range)."""
    lo, hi = rows if rows is not None else (0, len(rp) - 1)
    for j in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, j])
        ref = oracle.csr_serial(rp, col, val, x)
        assert_parity(Y[lo:hi, j], ref[lo:hi], rp[lo:hi + 1] - rp[lo], col[rp[lo]:rp[hi]], val[rp[lo]:rp[hi]], x,
                      what=f"{what} column {j}")


def with_long_rows(rng, rp, col, val, N, where, lengths):
    """The CSR with rows `where` replaced by rows of `lengths` distinct sorted columns (0: an empty row)."""
    lens = np.diff(rp).astype(np.int64)
    rows = [col[rp[r]:rp[r + 1]] for r in range(len(lens))]
    vals = [val[rp[r]:rp[r + 1]] for r in range(len(lens))]
    for r, n in zip(where, lengths):
        rows[r] = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
        vals[r] = rng.uniform(-1, 1, n)
        lens[r] = n
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rp2, np.concatenate(rows).astype(np.int32), np.concatenate(vals)


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_hll_spmm_matches_reference_golden(gpu, oracle, name):
    """X = [ones, x_rand, 2 x_rand - 1]: columns 0 and 1 are the compiled reference's y_ones / y_rand."""
    g = load_golden(name)
    pre = sp.read_matrix_market(golden_path(name))
    csr = sp.convert_in_csr(pre)
    xr = np.asarray(g["x_rand"], dtype=np.float64)
    X = np.column_stack([np.ones(csr.N), xr, 2.0 * xr - 1.0])
    with sp.HllDevice(sp.convert_to_hll(pre)) as dev:
        Y = dev.spmm(X)
    assert Y.shape == (csr.M, 3)
    for j, key in ((0, "y_ones"), (1, "y_rand")):
        assert_parity(Y[:, j], g[key], csr.row_ptr, csr.col_idx, csr.values, X[:, j], what=f"{name}/{key}")
    check_columns(oracle, Y, X, np.asarray(csr.row_ptr), np.asarray(csr.col_idx), np.asarray(csr.values), name)


# ------------------------------------------------------------------ seeded slabs
def _seeded_cases():
    rng = np.random.default_rng(31)
    M, N = 3000, 30000
    rp, col, val = random_csr(rng, M, N, 14, 60, 0.05)
    # a hack of empty rows; hacks whose rows are wider than the stage (2500 of at most 2048 slots): each row of them a
    # one-row window for hll_spmm_row
    rp, col, val = with_long_rows(rng, rp, col, val, N, list(range(64, 96)) + [5, 1700, 2999],
                                  [0] * 32 + [2500, 9000, 20000])
    yield "random", M, N, rp, col, val
    M = N = 8000
    rp, col, val = banded_csr(rng, M, N, 20, 150, empty_frac=0.1, far_frac=0.05)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [0, 4000], [2100, 7999])
    yield "banded", M, N, rp, col, val
    # a row of more than 65535 slots: its window's descriptor holds span 0
    M, N = 200, 100_000
    rp, col, val = random_csr(rng, M, N, 9, 30, 0.2)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [77], [70_000])
    yield "row > 65535", M, N, rp, col, val


def test_hll_spmm_seeded_slabs_every_k(gpu, oracle):
    rng = np.random.default_rng(7)
    for what, M, N, rp, col, val in _seeded_cases():
        with sp.HllDevice(hll_of(M, N, rp, col, val)) as dev:
            for k in KS:
                X = rng.uniform(-1, 1, (N, k))
                check_columns(oracle, dev.spmm(X), X, rp, col, val, f"{what} k={k}")


# ------------------------------------------------------------------ every plan kind of a handle
def _plan_cases():
    from sparsematrixvectormultiplication_amd import synth
    rng = np.random.default_rng(17)
    M, N = 3000, 30000
    rp, col, val = random_csr(rng, M, N, 14, 60, 0.05)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [40], [3000])
    yield ("hll_lds", M, N, rp, col, val, {"stream_local": 0, "stream_tile": 0},
           lambda i: i["stream_kernel"] == 0 and i["local_blocks"] == 0 and i["tile_blocks"] == 0)
    M = N = 20000
    rp, col, val = banded_csr(rng, M, N, 22, 150)
    yield "x-window", M, N, rp, col, val, {}, lambda i: i["stream_kernel"] == 1 and i["local_blocks"] > 0
    M, rp, col, val = synth.kkt_like((24, 24, 25), 5)
    yield ("pattern", M, M, rp, col, val, {"local_patterns": 1},
           lambda i: i["stream_kernel"] == 1 and i["pattern_slots"] > 0)
    M, N = 9001, 1_500_000
    lens = rng.poisson(12, M).astype(np.int64)
    rows = np.repeat(np.arange(M), lens)
    c = rng.integers(0, N, int(lens.sum()))
    order = np.lexsort((c, rows))
    c, rows = c[order], rows[order]
    keep = np.ones(len(c), bool)
    keep[1:] = (rows[1:] != rows[:-1]) | (c[1:] != c[:-1])  # distinct columns per row
    lens = np.bincount(rows[keep], minlength=M)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    yield ("tiles", M, N, rp, c[keep].astype(np.int32), rng.uniform(-1, 1, rp[-1]),
           {"stream_tile": 1, "tile_rows": 1024, "stream_local": 0},
           lambda i: i["stream_kernel"] == 2 and i["local_blocks"] == 0)


def test_hll_spmm_on_handles_with_every_plan_kind(gpu, oracle):
    rng = np.random.default_rng(3)
    for what, M, N, rp, col, val, knobs, has_plan in _plan_cases():
        hll = hll_of(M, N, rp, col, val)
        with sp.tuning(**knobs):
            dev = sp.HllDevice(hll)
        with dev:
            info = dev.info()
            assert has_plan(info), (what, {k: info[k] for k in ("stream_kernel", "local_blocks", "pattern_slots",
                                                                 "tile_blocks")})
            for k in (1, 3, 8, 12):
                X = rng.uniform(-1, 1, (N, k))
                check_columns(oracle, dev.spmm(X), X, rp, col, val, f"{what} k={k}")
            x = np.ascontiguousarray(X[:, 0])
            assert dev.spmm(x).ravel().tobytes() == dev.spmv(x, sp.HLL_AUTO).tobytes(), what


# ------------------------------------------------------------------ k = 1, determinism, load paths
def test_hll_spmm_k1_is_the_handles_spmv(gpu, oracle):
    rng = np.random.default_rng(21)
    M, N = 5000, 5200
    rp, col, val = random_csr(rng, M, N, 25, 80, 0.02)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [100], [5000])
    x = rng.uniform(-1, 1, N)
    with sp.HllDevice(hll_of(M, N, rp, col, val)) as dev, DeviceBuffer(N * 8 + 128) as dx, \
            DeviceBuffer(M * 8) as dy1, DeviceBuffer(M * 8) as dy2:
        dx.upload(x)
        dev.run_on(dx.at(), dy1.at(), sp.HLL_AUTO)
        dev.spmm_on(dx.at(), dy2.at(), 1)
        y_spmv = dy1.download(M)
        assert dy2.download(M).tobytes() == y_spmv.tobytes()
        assert dev.spmm(x).shape == (M, 1)
        assert dev.spmm(x).ravel().tobytes() == y_spmv.tobytes()
        assert dev.spmm(x[:, None]).ravel().tobytes() == y_spmv.tobytes()
        check_columns(oracle, y_spmv[:, None], x[:, None], rp, col, val, "k=1")


def test_hll_spmm_is_bit_reproducible_on_both_load_paths(gpu, oracle):
    rng = np.random.default_rng(22)
    M, N = 5000, 5200
    rp, col, val = random_csr(rng, M, N, 25, 80, 0.02)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [100, 4000], [5000, 3000])
    with sp.HllDevice(hll_of(M, N, rp, col, val)) as dev:
        for k in (2, 3, 8, 33, 40):
            X = rng.uniform(-1, 1, (N, k))
            Y = dev.spmm(X)
            assert dev.spmm(X).tobytes() == Y.tobytes(), f"k={k}: result changed between calls"
            assert dev.spmm(np.asfortranarray(X)).tobytes() == Y.tobytes()
            check_columns(oracle, Y, X, rp, col, val, f"k={k}")
            # X / Y 16-byte aligned (16-byte loads when k is even) and 8 bytes off (element loads): the same bits
            with DeviceBuffer(N * k * 8 + 16) as dx, DeviceBuffer(M * k * 8 + 16) as dy:
                for off in (0, 8):
                    dx.upload(X, off)
                    dy.poison()
                    dev.spmm_on(dx.at(off), dy.at(off), k)
                    assert dy.download((M, k), off).tobytes() == Y.tobytes(), f"k={k}, X / Y offset {off}"
        ms = dev.time_spmm(8, warmup=2, iters=5)
        assert ms.shape == (5,) and np.all(ms > 0) and np.all(ms < 1e3)


# ------------------------------------------------------------------ hack ranges, device-built slabs
def test_hll_spmm_hack_ranges_fill_one_shared_y(gpu, oracle):
    rng = np.random.default_rng(8)
    M, N, k = 6000, 6000, 6
    rp, col, val = random_csr(rng, M, N, 20, 50, 0.05)
    rp, col, val = with_long_rows(rng, rp, col, val, N, [10, 3333], [3000, 4500])
    X = rng.uniform(-1, 1, (N, k))
    hll = hll_of(M, N, rp, col, val)
    with sp.HllDevice(hll) as whole:
        Y_ref = whole.spmm(X)
    hb = sp.partition_hacks(hll, 3)
    rb = sp.hack_bounds_to_rows(hb, M)
    assert hb[0] == 0 and hb[-1] == hll.num_blocks
    with DeviceBuffer(N * k * 8) as dx, DeviceBuffer(M * k * 8) as dy:
        dx.upload(X)
        dy.poison()
        for p in range(3):
            lo, hi = int(rb[p]), int(rb[p + 1])
            with sp.HllDevice(hll, int(hb[p]), int(hb[p + 1])) as part:
                assert (part.info()["row0"], part.info()["M_local"]) == (lo, hi - lo)
                before = dy.download((M, k))
                part.spmm_on(dx.at(), dy.at(), k)
                after = dy.download((M, k))
                outside = np.ones(M, bool)
                outside[lo:hi] = False
                assert after[outside].tobytes() == before[outside].tobytes(), f"range {p} wrote outside its rows"
                assert np.all(np.isnan(after[hi:])) and np.all(np.isfinite(after[lo:hi]))
                Yh = part.spmm(X)  # the host entry point writes only the handle's rows of Y_host
                assert np.all(Yh[outside] == 0)
                assert Yh[lo:hi].tobytes() == after[lo:hi].tobytes()
                if hi > lo:  # the same range built on the device from a 32-aligned CSR row block
                    with sp.CsrDevice(M, N, rp, col, val, row0=lo, row1=hi) as cpart, \
                            sp.HllDevice.from_csr_device(cpart) as built:
                        assert built.info()["row0"] == lo and built.info()["slots"] == part.info()["slots"]
                        assert built.spmm(X).tobytes() == Yh.tobytes(), f"range {p}: device-built slab"
        Y = dy.download((M, k))
    assert np.all(np.isfinite(Y))
    # (a range's windows are cut from its own first row, so its sums may be grouped otherwise than the whole slab's)
    for j in range(k):
        assert_parity(Y[:, j], Y_ref[:, j], rp, col, val, X[:, j], what=f"hack ranges vs whole slab, column {j}")
    check_columns(oracle, Y, X, rp, col, val, "hack ranges")


def test_hll_spmm_device_built_slab_gives_the_host_built_bits(gpu, oracle):
    rng = np.random.default_rng(9)
    for what, M, N, rp, col, val in _seeded_cases():
        hll = hll_of(M, N, rp, col, val)
        with sp.HllDevice(hll) as host_built, sp.CsrDevice(M, N, rp, col, val) as cdev, \
                sp.HllDevice.from_csr_device(cdev) as dev_built:
            for k in (2, 5, 8, 20):
                X = rng.uniform(-1, 1, (N, k))
                Y = host_built.spmm(X)
                assert dev_built.spmm(X).tobytes() == Y.tobytes(), f"{what} k={k}"
            check_columns(oracle, Y, X, rp, col, val, f"{what} k={k}")


# ------------------------------------------------------------------ caller stream, torch buffers
_TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first: one HIP runtime serves torch and the library (as in bench.py)
sys.path.insert(0, sys.argv[1])
import sparsematrixvectormultiplication_amd as sp
sys.path.insert(0, sys.argv[2])
from _util import random_csr, coo_from_csr

assert torch.cuda.is_available()
torch.cuda.set_device(0)
sp.hip_init(0)
rng = np.random.default_rng(12)
M, N, k = 4000, 4100, 8
rp, col, val = random_csr(rng, M, N, 18, 60, 0.05)
r, c, v = coo_from_csr(rp, col, val)
X = rng.uniform(-1, 1, (N, k))
with sp.HllDevice(sp.convert_to_hll(sp.PreMatrix.from_arrays(M, N, r, c, v))) as dev:
    Y_host = dev.spmm(X)
    X_t = torch.from_numpy(X).to("cuda")
    Y_t = torch.full((M, k), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev.spmm_on(X_t.data_ptr(), Y_t.data_ptr(), k, stream=s.cuda_stream)
    s.synchronize()
    Y_s = Y_t.cpu().numpy()
np.savez(sys.argv[3], rp=rp, col=col, val=val, X=X, Y_host=Y_host, Y_stream=Y_s)
"""


def test_hll_spmm_on_a_caller_stream_with_torch_buffers(gpu, oracle):
    """spmm_on with torch tensors' data_ptr() and a torch stream.  In a fresh child process that imports torch before
    the library, so that both use one HIP runtime."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "r.npz")
        proc = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT, os.path.join(ROOT, "tests"), out],
                              capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr[-3000:]
        r = np.load(out)
        rp, col, val, X = r["rp"], r["col"], r["val"], r["X"]
        Y_host, Y_stream = r["Y_host"], r["Y_stream"]
    assert Y_stream.tobytes() == Y_host.tobytes()
    check_columns(oracle, Y_stream, X, rp, col, val, "torch stream")


# ------------------------------------------------------------------ full size
def test_hll_spmm_full_size_nlpkkt_like(gpu, oracle):
    from sparsematrixvectormultiplication_amd import synth
    M, rp, col, val = synth.kkt_like()
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (M, 8))
    with sp.CsrDevice(M, M, rp, col, val) as cdev:
        with sp.HllDevice.from_csr_device(cdev) as dev:
            # the slab's AS is above 128 MiB: upload searched its placement, and the handle runs after the search
            info = dev.info()
            assert info["place_tries"] >= 1 and 0 < info["place_best_us"] <= info["place_first_us"], info
            dev.run()
            Y = dev.spmm(X)
    check_columns(oracle, Y, X, rp, col, val, "nlpkkt-like k=8")


# ------------------------------------------------------------------ errors
def test_hll_spmm_errors_leave_the_handle_usable(gpu, oracle):
    rng = np.random.default_rng(2)
    M, N = 2000, 2100
    rp, col, val = random_csr(rng, M, N, 12, 40, 0.0)
    lib = sp.lib()
    with sp.HllDevice(hll_of(M, N, rp, col, val)) as dev, DeviceBuffer(N * 8 * 4 + 64) as dx, \
            DeviceBuffer(M * 8 * 4 + 64) as dy:
        for k, X_ptr, Y_ptr, msg in ((0, dx.at(), dy.at(), b"k = 0"), (4, None, dy.at(), b"NULL"),
                                     (4, dx.at(4), dy.at(), b"aligned"), (4, dx.at(), dy.at(4), b"aligned")):
            assert lib.spmv_hip_hll_spmm_on(dev.h, k, X_ptr, Y_ptr, None) == -1
            assert msg in lib.spmv_hip_last_error()
        assert lib.spmv_hip_hll_spmm(dev.h, 4, None, None) == -1
        assert b"NULL" in lib.spmv_hip_last_error()
        with pytest.raises(sp.SpmvHipError, match="k = 0"):
            dev.spmm_on(dx.at(), dy.at(), 0)
        with pytest.raises(sp.SpmvHipError):
            dev.time_spmm(0)
        X = rng.uniform(-1, 1, (N, 4))
        check_columns(oracle, dev.spmm(X), X, rp, col, val, "SpMM after the refused calls")
