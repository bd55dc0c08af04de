"""GPU side of the path: thin objects over the C-ABI of include/spmv_hip.h.

Shape dictated by the reference's CUDA driver (main_cuda.cu): upload once
(:135-145, :369-402) -> run many (:166, :238, :317, :454, :568, :637) ->
fetch y (:183).  No CPU fallback anywhere: a failed C call raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _native as nat
from .host import CsrHost, HllHost

CSR_AUTO, CSR_THREAD_ROW, CSR_WAVE_ROW, CSR_SUBWAVE, CSR_STREAM = 0, 1, 2, 3, 4
HLL_AUTO, HLL_THREAD_ROW, HLL_SUBWAVE, HLL_LDS = 0, 1, 2, 3
# CsrDevice.bicgstab: info["status"] (SPMV_BICG_* of include/spmv_hip.h)
BICG_RAN_ALL, BICG_CONVERGED, BICG_BREAKDOWN_RHO, BICG_BREAKDOWN_OMEGA = 0, 1, 2, 3
# CsrDevice.cgls: info["status"] (SPMV_CGLS_* of include/spmv_hip.h)
CGLS_RAN_ALL, CGLS_CONVERGED, CGLS_BREAKDOWN = 0, 1, 2
# CsrDevice.pcg: info["status"] (SPMV_PCG_*); CsrDevice.preconditioner kinds (SPMV_PRECOND_*)
PCG_RAN_ALL, PCG_CONVERGED, PCG_BREAKDOWN = 0, 1, 2
# CsrDevice.minres: info["status"] (SPMV_MINRES_* of include/spmv_hip.h)
MINRES_RAN_ALL, MINRES_CONVERGED, MINRES_BREAKDOWN = 0, 1, 2
# CsrDevice.lobpcg: info["status"] (SPMV_LOBPCG_* of include/spmv_hip.h); its limits
LOBPCG_RAN_ALL, LOBPCG_CONVERGED, LOBPCG_BREAKDOWN = 0, 1, 2
LOBPCG_MAX_K, LOBPCG_DROP = 16, 1e-10
# CsrDevice.gmres: info["status"] (SPMV_GMRES_* of include/spmv_hip.h); the widest restart
GMRES_RAN_ALL, GMRES_CONVERGED, GMRES_BREAKDOWN = 0, 1, 2
GMRES_MAX_RESTART = 64
PRECOND_JACOBI, PRECOND_BLOCK_JACOBI, PRECOND_SSOR, PRECOND_ILU0, PRECOND_FSAI, PRECOND_AMG = 1, 2, 3, 4, 5, 6
PRECOND_CHEBYSHEV = 7
PRECOND_KINDS = {"jacobi": PRECOND_JACOBI, "block_jacobi": PRECOND_BLOCK_JACOBI, "ssor": PRECOND_SSOR,
                 "ilu0": PRECOND_ILU0, "fsai": PRECOND_FSAI, "amg": PRECOND_AMG, "chebyshev": PRECOND_CHEBYSHEV}
# the Chebyshev polynomial preconditioner: its largest degree, what spmv_hip_precond_cheb_info returns (doubles)
CHEBYSHEV_MAX_DEGREE = 32
PRECOND_CHEB_INFO = ("degree", "lmin", "lmax", "gershgorin", "products", "plan", "download_us", "upload_us")
# the AMG hierarchy (SPMV_AMG_*): what a level reader returns, a level's kind, the limits of the setup
AMG_A, AMG_P, AMG_R, AMG_INV, AMG_T = 0, 1, 2, 3, 4
AMG_NOT_COARSEST, AMG_DIRECT, AMG_SMOOTH = 0, 1, 2
AMG_MAX_LEVELS, AMG_MAX_COARSE_ROWS, AMG_CHAIN_ROWS, AMG_CHAIN_ENTRIES = 16, 256, 256, 4096
PRECOND_AMG_INFO = ("levels", "first_chained", "launches", "coarsest", "complexity_x1000", "download_us", "setup_us",
                    "upload_us", "chain")  # then rows[16] and entries[16] per level
PRECOND_AMG_INFO_WORDS = len(PRECOND_AMG_INFO) + 2 * AMG_MAX_LEVELS
# the AMG setups, and what spmv_hip_precond_amg_setup_info returns: the setup, then the device setup's phases
AMG_SETUPS = {"host": 0, "device": 1}
PRECOND_AMG_SETUP_INFO = ("setup", "stats_us", "strength_us", "aggregate_us", "tentative_us", "transpose_us", "ap_us",
                          "rap_us", "inverse_us", "round_us")
PRECOND_AMG_SETUP_INFO_WORDS = len(PRECOND_AMG_SETUP_INFO)
SPGEMM_MAX_BLOCK_PRODUCTS = 4096
# CsrDevice.triangular / the SSOR and ILU(0) preconditioners (SPMV_TRSV_*, SPMV_ORDER_*)
TRSV_LOWER, TRSV_UPPER, TRSV_NONUNIT, TRSV_UNIT = 0, 1, 0, 1
ORDER_NATURAL, ORDER_MULTICOLOR = 0, 1
ORDERINGS = {"natural": ORDER_NATURAL, "multicolor": ORDER_MULTICOLOR}
TRSV_INFO = ("rows", "row0", "value_bytes", "entries", "levels", "launches", "widest", "colours", "median",
             "lanes_per_row", "analysis_us", "upload_us")
PRECOND_TRI_INFO = ("forward_levels", "forward_launches", "forward_widest", "forward_median", "backward_levels",
                    "backward_launches", "backward_widest", "backward_median", "colours", "entries_l", "entries_u",
                    "analysis_us", "factor_us", "upload_us")
PRECOND_FSAI_INFO = ("cap", "entries", "truncated_rows", "widest", "plan_g", "plan_gt", "analysis_us", "build_us",
                     "upload_us")
FSAI_PLANS = ("gather", "x_window", "x_window_pattern", "csr_tile")  # fsai_info()["plan_g"], ["plan_gt"]
# CsrDevice.matmul: the result's matmul_info (the stats and the time split of spmv_hip_csr_spgemm)
MATMUL_STATS = ("products", "nz", "blocks", "block_rows", "long_rows", "chunks", "max_row_products", "max_row_nz")
MATMUL_MS = ("count", "symbolic", "numeric", "adopt")
SPGEMM_MAX_ROWS = 4096
# CsrDevice.add: the result's add_info (the stats and the time split of spmv_hip_csr_add)
ADD_STATS = ("nz", "matches", "a_canonical", "b_canonical", "long_rows", "max_row_nz")
ADD_MS = ("check", "canonical", "symbolic", "numeric", "adopt")
ADD_METHODS = {"auto": 0, "merge": 1, "canonical": 2}
# CsrDevice.rcm / rcm_plan: the info (the stats of spmv_hip_csr_rcm and spmv_rcm_plan_build) and the time split
RCM_STATS = ("components", "isolated", "levels", "chained_levels", "wide_levels", "launches", "peripheral_searches",
             "bandwidth_before", "bandwidth_after")
RCM_MS = ("graph", "peripheral", "order")
RCM_MAX_PERIPHERAL = 8
PERMUTE_MS = ("device_build", "adopt")
CSR_STREAM_KERNELS = ("csr_stream", "csr_stream_local", "csr_stream_short", "csr_tile")
HLL_LDS_KERNELS = ("hll_lds", "hll_lds_local", "csr_tile (HLL slab rows)")
CSR_VARIANTS = {"thread_row": CSR_THREAD_ROW, "wave_row": CSR_WAVE_ROW, "subwave": CSR_SUBWAVE,
                "stream": CSR_STREAM}
HLL_VARIANTS = {"thread_row": HLL_THREAD_ROW, "subwave": HLL_SUBWAVE, "lds": HLL_LDS}


class SpmvHipError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        msg = nat.lib().spmv_hip_last_error()
        raise SpmvHipError(f"{what}: {msg.decode(errors='replace') if msg else 'failed (-1)'}")


def device_count() -> int:
    return nat.lib().spmv_hip_device_count()


def hip_init(device: int = 0) -> None:
    _check(nat.lib().spmv_hip_init(int(device)), "spmv_hip_init")


def hip_sync() -> None:
    _check(nat.lib().spmv_hip_sync(), "spmv_hip_sync")


def hip_stream() -> int:
    return nat.lib().spmv_hip_stream() or 0


def device_name():
    buf = C.create_string_buffer(256)
    cus, mem = C.c_int(), C.c_longlong()
    _check(nat.lib().spmv_hip_device_name(buf, 256, C.byref(cus), C.byref(mem)), "device_name")
    return buf.value.decode(), cus.value, mem.value


def flush_cache(nbytes: int = 1 << 30) -> None:
    """Refill L2 + the 256 MiB Infinity Cache with scratch data."""
    _check(nat.lib().spmv_hip_flush_cache(int(nbytes)), "spmv_hip_flush_cache")


def stream_probe(nbytes: int = 1 << 30, warmup: int = 3, iters: int = 10):
    """(mean, min) ms of a read-only 16-byte-per-lane stream over `nbytes` of HBM (spmv_hip_stream_probe)."""
    mean, mn = C.c_float(0), C.c_float(0)
    _check(nat.lib().spmv_hip_stream_probe(int(nbytes), int(warmup), int(iters), C.byref(mean), C.byref(mn)),
           "spmv_hip_stream_probe")
    return float(mean.value), float(mn.value)


def stream_probe_at(dptr: int, nbytes: int, warmup: int = 2, iters: int = 8):
    """(mean, min) ms of the read-only stream over [dptr, dptr + nbytes) (spmv_hip_stream_probe_at)."""
    mean, mn = C.c_float(0), C.c_float(0)
    _check(nat.lib().spmv_hip_stream_probe_at(C.c_void_p(dptr), int(nbytes), int(warmup), int(iters), C.byref(mean),
                                              C.byref(mn)), "spmv_hip_stream_probe_at")
    return float(mean.value), float(mn.value)


def gather_probe(value_bytes: int = 4, table_bytes: int = 2 << 20, waves_per_cu: int = 16) -> float:
    """values / s of 64-different-lines gathers from an L2-resident table (spmv_hip_gather_probe)."""
    out = C.c_double(0)
    _check(nat.lib().spmv_hip_gather_probe(int(value_bytes), int(table_bytes), int(waves_per_cu), C.byref(out)),
           "spmv_hip_gather_probe")
    return float(out.value)


def _read(path, limit=400):
    try:
        with open(path) as fh:
            return fh.read(limit).strip()
    except OSError:
        return None


def box_state(probe_bytes: int = 1 << 30) -> dict:
    """What distinguishes one GPU box of the pool from another, for bench records: the HIP attributes
    (spmv_hip_device_state), the card's sysfs state (partition modes, DPM clock tables with the active level,
    power cap, VBIOS) found through its PCI bus id, and the time of a read-only stream over 1 GiB."""
    import glob
    import os
    buf = C.create_string_buffer(512)
    _check(nat.lib().spmv_hip_device_state(buf, 512), "spmv_hip_device_state")
    out = dict(item.split("=", 1) for item in buf.value.decode().split(";") if "=" in item)
    for k in ("cus", "xcds", "sclk_khz", "mclk_khz", "mem_bus_bits", "l2_bytes", "hbm_bytes", "hbm_free_bytes"):
        if k in out:
            out[k] = int(out[k])
    pci = out.get("pci", "").lower()
    card = None
    for dev in sorted(glob.glob("/sys/class/drm/card*/device")):
        if pci and os.path.basename(os.path.realpath(dev)).lower() == pci:
            card = dev
            break
    sysfs = {}
    if card:
        for name in ("current_compute_partition", "current_memory_partition", "pp_dpm_sclk", "pp_dpm_mclk",
                     "pp_dpm_fclk", "pp_dpm_socclk", "power_dpm_force_performance_level", "vbios_version",
                     "mem_info_vram_used", "unique_id"):
            v = _read(os.path.join(card, name))
            if v is not None:
                # DPM tables: keep the active level ("*") only
                if name.startswith("pp_dpm_"):
                    act = [ln for ln in v.splitlines() if ln.rstrip().endswith("*")]
                    v = {"active": act[0].rstrip(" *") if act else None, "levels": len(v.splitlines())}
                sysfs[name] = v
        for hw in sorted(glob.glob(os.path.join(card, "hwmon", "hwmon*"))):
            for name in ("power1_cap", "power1_average", "power1_input", "temp1_input", "freq1_input", "freq2_input"):
                v = _read(os.path.join(hw, name))
                if v is not None:
                    sysfs[name] = v
    out["sysfs_card"] = card
    out["sysfs"] = sysfs
    if probe_bytes:
        mean, mn = stream_probe(probe_bytes, 3, 10)
        out["stream_probe"] = {"bytes": int(probe_bytes), "ms_mean": round(mean, 5), "ms_min": round(mn, 5),
                               "gbps_mean": round(probe_bytes / (mean * 1e-3) / 1e9, 1)}
    return out


def set_tuning(key: str, value: int) -> None:
    """Set one tuning knob (the keys, their values and defaults: include/spmv_hip.h).  A refused value raises and
    leaves the knob as it was.  Code that should put the knob back afterwards uses tuning()."""
    _check(nat.lib().spmv_hip_set_tuning(key.encode(), int(value)), "spmv_hip_set_tuning")


def get_tuning(key: str) -> int:
    """The value a tuning knob holds now."""
    value = C.c_int()
    _check(nat.lib().spmv_hip_get_tuning(key.encode(), C.byref(value)), "spmv_hip_get_tuning")
    return value.value


def tuning_values() -> dict:
    """{key: current value} of every tuning knob, in the library's order."""
    out, index = {}, 0
    while (key := nat.lib().spmv_hip_tuning_key(index)) is not None:
        out[key.decode()] = get_tuning(key.decode())
        index += 1
    return out


@contextlib.contextmanager
def tuning(**knobs):
    """with tuning(tile_rows=256, stream_kind=6): ... -- the knobs set in the order given; on the way out, also by an
    exception or a refused knob, those that were set get the values they held before (not the defaults), last first."""
    saved = []
    try:
        for key, value in knobs.items():
            before = get_tuning(key)
            set_tuning(key, value)
            saved.append((key, before))
        yield
    finally:
        for key, before in reversed(saved):
            set_tuning(key, before)


class _Handle:
    _free = None

    def __init__(self):
        self.h = C.c_void_p()

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            getattr(nat.lib(), self._free)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class CsrDevice(_Handle):
    """A CSR matrix, or rows [row0, row1) of one, resident in HBM."""

    _free = "spmv_hip_csr_free"

    def __init__(self, M, N, row_ptr, col_idx, values, row0=0, row1=None):
        super().__init__()
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.int32)
        if values.dtype == np.float32:
            values = np.ascontiguousarray(values)
            fn, vp, self.dtype = nat.lib().spmv_hip_csr_upload_f32, nat.c_float_p, np.float32
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            fn, vp, self.dtype = nat.lib().spmv_hip_csr_upload, nat.c_double_p, np.float64
        if len(row_ptr) != M + 1:
            raise ValueError("row_ptr must have M + 1 entries")
        row1 = M if row1 is None else row1
        _check(fn(int(M), int(N), row_ptr.ctypes.data_as(nat.c_int_p),
                  col_idx.ctypes.data_as(nat.c_int_p), values.ctypes.data_as(vp), int(row0),
                  int(row1), C.byref(self.h)), "spmv_hip_csr_upload")
        self.M, self.N = int(M), int(N)
        self.row0, self.row1 = int(row0), int(row1)

    def _own_rows(self):
        """(row0, row1): the rows this handle holds (the whole matrix unless uploaded as a row range)."""
        return getattr(self, "row0", 0), getattr(self, "row1", self.M)

    @classmethod
    def _built(cls, M, N, dtype, what, build):
        """A whole M x N handle the library builds on the device: build(out) is the C call, out its handle argument."""
        self = cls.__new__(cls)
        _Handle.__init__(self)
        _check(build(C.byref(self.h)), what)
        self.M, self.N, self.dtype = int(M), int(N), dtype
        return self

    @classmethod
    def from_coo(cls, M, N, I, J, val):
        """CSR built on the device from COO triplets (spmv_hip_csr_from_coo); fp64."""
        I = np.ascontiguousarray(I, dtype=np.int32)
        J = np.ascontiguousarray(J, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        return cls._built(M, N, np.float64, "spmv_hip_csr_from_coo", lambda out: nat.lib().spmv_hip_csr_from_coo(
            int(M), int(N), len(I), I.ctypes.data_as(nat.c_int_p), J.ctypes.data_as(nat.c_int_p),
            val.ctypes.data_as(nat.c_double_p), out))

    def transpose(self) -> "CsrDevice":
        """A^T as a new handle (spmv_hip_csr_transpose): built on the device from this handle's arrays, N x M, the same
        dtype, bit-exact values; it gets the plans an upload of A^T would get and owns its arrays."""
        return CsrDevice._built(self.N, self.M, self.dtype, "spmv_hip_csr_transpose",
                                lambda out: nat.lib().spmv_hip_csr_transpose(self.h, out))

    def matmul(self, other: "CsrDevice", block_products: int = 0, chunk_products: int = 0) -> "CsrDevice":
        """C = self @ other as a new handle (spmv_hip_csr_spgemm): both whole matrices of one dtype.  C has canonical rows
        (ascending columns, no repeats), a structural pattern (a sum that cancels to 0.0 stays) and, bit for bit, the
        values of the serial loop in include/spmv_hip.h: every product and sum a separate rounded double operation in
        entry order, rounded once to the dtype.  block_products: the on-chip tier's cap (0 = auto = 4096, a power of two
        in [64, 4096], -1 = every row through the global tier); chunk_products: the global tier's workspace in products
        (0 = auto, else >= 64).  C.matmul_info holds the stats (MATMUL_STATS) and "ms" (MATMUL_MS) of this product."""
        if not isinstance(other, CsrDevice):
            raise TypeError("matmul takes a CsrDevice")
        stats, ms = (C.c_longlong * len(MATMUL_STATS))(), (C.c_double * len(MATMUL_MS))()
        out = CsrDevice._built(self.M, other.N, self.dtype, "spmv_hip_csr_spgemm", lambda out: nat.lib().spmv_hip_csr_spgemm(
            self.h, other.h, int(block_products), int(chunk_products), out, stats, ms))
        out.matmul_info = dict(zip(MATMUL_STATS, (int(v) for v in stats)))
        out.matmul_info["ms"] = dict(zip(MATMUL_MS, (float(v) for v in ms)))
        return out

    def __matmul__(self, other):
        return self.matmul(other) if isinstance(other, CsrDevice) else NotImplemented

    def add(self, other: "CsrDevice" = None, alpha: float = 1.0, beta: float = 1.0, method: str = "auto", lanes: int = 0,
            long_row: int = 0) -> "CsrDevice":
        """C = alpha * self + beta * other as a new handle (spmv_hip_csr_add): both whole matrices of one shape and dtype;
        other = None gives alpha * canon(self).  C has canonical rows (ascending columns, no repeats) on the union of the
        two patterns (structural: a sum that cancels to 0.0 stays) and, bit for bit, the values of the definition in
        include/spmv_hip.h: repeated pairs added in entry order first, then every product and sum a separate rounded
        double operation, rounded once to the dtype.  method: "auto" (operands with unsorted rows or repeats go through
        the product's tiers first), "merge" (canonical operands only) or "canonical" (both through the product first);
        lanes: lanes per row of the merge (0 = auto, else a power of two in [1, 64]); long_row: the combined row length
        from which a row gets a workgroup (0 = auto).  C.add_info holds the stats (ADD_STATS) and "ms" (ADD_MS)."""
        if other is not None and not isinstance(other, CsrDevice):
            raise TypeError("add takes a CsrDevice or None")
        for name, m in (("self", self), ("other", other)):
            if m is not None and m._own_rows() != (0, m.M):
                raise ValueError(f"add: {name} holds rows {m._own_rows()} of {m.M}; only whole matrices add")
        if other is not None and (other.M, other.N) != (self.M, self.N):
            raise ValueError(f"add: self is {self.M} x {self.N} and other is {other.M} x {other.N}")
        if other is not None and np.dtype(other.dtype) != np.dtype(self.dtype):
            raise ValueError(f"add: self holds {np.dtype(self.dtype)} and other {np.dtype(other.dtype)}")
        alpha, beta = float(alpha), float(beta)
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError(f"add: alpha = {alpha}, beta = {beta}; both must be finite")
        if method not in ADD_METHODS:
            raise ValueError(f"add: method = {method!r}; one of {sorted(ADD_METHODS)}")
        lanes, long_row = int(lanes), int(long_row)
        if lanes != 0 and (lanes < 1 or lanes > 64 or lanes & (lanes - 1)):
            raise ValueError(f"add: lanes = {lanes}; 0 (auto) or a power of two in [1, 64]")
        if long_row < 0 or long_row > 0x7fffffff:
            raise ValueError(f"add: long_row = {long_row}; 0 (auto) or a positive row length")
        stats, ms = (C.c_longlong * len(ADD_STATS))(), (C.c_double * len(ADD_MS))()
        out = CsrDevice._built(self.M, self.N, self.dtype, "spmv_hip_csr_add", lambda out: nat.lib().spmv_hip_csr_add(
            self.h, alpha, other.h if other is not None else None, beta, ADD_METHODS[method], lanes, long_row, out, stats, ms))
        out.add_info = dict(zip(ADD_STATS, (int(v) for v in stats)))
        out.add_info["ms"] = dict(zip(ADD_MS, (float(v) for v in ms)))
        return out

    def canonical(self) -> "CsrDevice":
        """canon(self) as a new handle: sorted rows, repeated (row, column) pairs added in entry order (add(None))."""
        return self.add(None)

    def permute(self, row_perm=None, col_perm=None) -> "CsrDevice":
        """C = P A Q^T as a new handle (spmv_hip_csr_permute): C[i, j] = A[row_perm[i], col_perm[j]].  Row i of C is row
        row_perm[i] of this matrix, entry by entry: each keeps its place in the row and its value bit for bit and gets
        the column j with col_perm[j] == its column.  None is the identity.  Nothing is sorted or combined (canonical()
        sorts the rows); permuting C by the inverse permutations gives this handle's arrays exactly.  C gets the plans an
        upload would get, owns its arrays and outlives this handle.  C.permute_info["ms"] holds PERMUTE_MS."""
        perms = []
        for name, perm, n in (("row_perm", row_perm, self.M), ("col_perm", col_perm, self.N)):
            if perm is not None:
                perm = np.asarray(perm)
                if perm.ndim != 1 or perm.size != n:
                    raise ValueError(f"permute: {name} has shape {perm.shape}; {n} entries are needed")
                if not np.issubdtype(perm.dtype, np.integer):
                    raise ValueError(f"permute: {name} holds {perm.dtype}; integers are needed")
                if perm.size and (perm.min() < -2 ** 31 or perm.max() >= 2 ** 31):
                    raise ValueError(f"permute: {name} holds values beyond 32 bits")
                perm = np.ascontiguousarray(perm, dtype=np.int32)
            perms.append(perm)
        if self._own_rows() != (0, self.M):
            raise SpmvHipError(f"csr_permute: a handle of rows {self._own_rows()} of {self.M}; only whole matrices permute")
        ptr = [q.ctypes.data_as(nat.c_int_p) if q is not None else None for q in perms]
        out = CsrDevice._built(self.M, self.N, self.dtype, "spmv_hip_csr_permute",
                               lambda out: nat.lib().spmv_hip_csr_permute(self.h, ptr[0], ptr[1], out))
        ms = (C.c_double * len(PERMUTE_MS))()
        _check(nat.lib().spmv_hip_csr_permute_ms(ms), "spmv_hip_csr_permute_ms")
        out.permute_info = {"ms": dict(zip(PERMUTE_MS, (float(v) for v in ms)))}
        return out

    def rcm(self, peripheral: int = 2, chain_nodes: int = 0):
        """(perm, info): the reverse Cuthill-McKee ordering of this square matrix, built on the device
        (spmv_hip_csr_rcm); perm is what rcm_plan gives on the downloaded arrays, byte for byte.  New row i is old row
        perm[i]: the reordered matrix is permute(perm, perm).  peripheral: passes of the start-node search, 0 .. 8;
        chain_nodes: levels of at most this many nodes run chained in one workgroup (0 = auto, -1 = never, else a power
        of two in rcm_chain_nodes()).  info holds RCM_STATS and "ms" (RCM_MS)."""
        peripheral, chain_nodes = int(peripheral), int(chain_nodes)
        perm = np.zeros(self.M, dtype=np.int32)
        stats, ms = (C.c_longlong * len(RCM_STATS))(), (C.c_double * len(RCM_MS))()
        _check(nat.lib().spmv_hip_csr_rcm(self.h, peripheral, chain_nodes, perm.ctypes.data_as(nat.c_int_p), stats, ms),
               "spmv_hip_csr_rcm")
        info = dict(zip(RCM_STATS, (int(v) for v in stats)))
        info["ms"] = dict(zip(RCM_MS, (float(v) for v in ms)))
        return perm, info

    def reordered(self, method: str = "rcm", **kw):
        """(B, perm) with B = self.permute(perm, perm) for the ordering `method` ("rcm": perm of self.rcm(**kw)).
        Vectors: to solve A x = b, solve B y = b[perm]; then x[perm] = y.  B.reorder_info is the ordering's info."""
        if method != "rcm":
            raise ValueError(f"reordered: method = {method!r}; \"rcm\" is the ordering there is")
        perm, info = self.rcm(**kw)
        out = self.permute(perm, perm)
        out.reorder_info = info
        return out, perm

    def __add__(self, other):
        return self.add(other) if isinstance(other, CsrDevice) else NotImplemented

    def __sub__(self, other):
        return self.add(other, 1.0, -1.0) if isinstance(other, CsrDevice) else NotImplemented

    def __neg__(self):
        return self.add(None, -1.0)

    def download(self):
        """(row_ptr, col_idx, values) of the handle's rows, from the device."""
        info = self.info()
        rp = np.zeros(info["M_local"] + 1, dtype=np.int32)
        col = np.zeros(max(info["nz"], 1), dtype=np.int32)
        val = np.zeros(max(info["nz"], 1), dtype=self.dtype)
        _check(nat.lib().spmv_hip_csr_download(self.h, rp.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p),
                                               val.ctypes.data_as(C.c_void_p)), "spmv_hip_csr_download")
        return rp, col[:info["nz"]], val[:info["nz"]]

    def update_values(self, values):
        """New numbers on the handle's pattern (spmv_hip_csr_update_values): the handle's own nz values, of its dtype and
        in its own entry order -- the order download() returns.  The handle is then the upload of (its pattern, values)
        under the plan it has; info() and addresses() stay as they are.  The first update of a handle with tile plans
        pays one analysis (update_info()["map_build_us"]); a handle holding a column split is refused."""
        values = np.asarray(values)
        nz = self.info()["nz"]
        if values.ndim != 1 or values.size != nz:
            raise ValueError(f"update_values: values has shape {values.shape}; the handle holds {nz} entries")
        if values.dtype != np.dtype(self.dtype):
            raise ValueError(f"update_values: values holds {values.dtype}, the handle {np.dtype(self.dtype)}")
        values = np.ascontiguousarray(values)
        if nz == 0:     # (an empty array need not have an address)
            values = np.zeros(1, dtype=self.dtype)
        _check(nat.lib().spmv_hip_csr_update_values(self.h, values.ctypes.data_as(C.c_void_p)), "spmv_hip_csr_update_values")

    def update_values_on(self, d_val, stream=0):
        """update_values from a device array (its address) of the handle's nz values in the handle's dtype, on `stream`
        (0: the library's); does not wait for the device once the handle's first update has been made."""
        _check(nat.lib().spmv_hip_csr_update_values_on(self.h, C.c_void_p(int(getattr(d_val, "value", d_val) or 0)),
                                                       C.c_void_p(int(stream)) if stream else None),
               "spmv_hip_csr_update_values_on")

    def update_info(self) -> dict:
        """{"updates": made so far, "map_bytes": the source maps on the device, "map_build_us": the first update's
        analysis, "last_us": the last update's device time (waits for it)} (spmv_hip_csr_update_info)."""
        counts, us = (C.c_longlong * 2)(), (C.c_double * 2)()
        _check(nat.lib().spmv_hip_csr_update_info(self.h, counts, us), "spmv_hip_csr_update_info")
        return {"updates": int(counts[0]), "map_bytes": int(counts[1]), "map_build_us": float(us[0]), "last_us": float(us[1])}

    @classmethod
    def from_host(cls, csr: CsrHost, row0=0, row1=None):
        return cls(csr.M, csr.N, csr.row_ptr, csr.col_idx, csr.values, row0, row1)

    def info(self) -> dict:
        out = nat.DevInfo()
        _check(nat.lib().spmv_hip_csr_info(self.h, C.byref(out)), "spmv_hip_csr_info")
        return out.as_dict()

    def addresses(self) -> dict:
        out = (C.c_ulonglong * 8)()
        _check(nat.lib().spmv_hip_csr_addresses(self.h, out), "spmv_hip_csr_addresses")
        return dict(zip(("row_ptr", "col", "val", "x", "y", "lcol", "lines", "ldesc4"), (int(v) for v in out)))

    ARRAYS = ("row_ptr", "col", "val", "x", "y", "lcol", "lines", "ldesc4")

    def tile_digest(self):
        """(elements, hash) of each of the 32 arrays of the handle's tile plans (spmv_hip_csr_tile_digest)."""
        out = (C.c_ulonglong * 64)()
        _check(nat.lib().spmv_hip_csr_tile_digest(self.h, out), "spmv_hip_csr_tile_digest")
        return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(32)]

    def stamp_blocks(self, warm: int = 3):
        """(start, end, dispatch id, xcd) per x-window block of one stamped launch; times in ticks of 10 ns."""
        n = self.info()["local_blocks"]
        buf = np.zeros(3 * n, dtype=np.uint64)
        _check(nat.lib().spmv_hip_csr_stamp_blocks(self.h, int(warm), buf.ctypes.data_as(C.POINTER(C.c_ulonglong))),
               "spmv_hip_csr_stamp_blocks")
        buf = buf.reshape(n, 3)
        return buf[:, 0].astype(np.int64), buf[:, 1].astype(np.int64), (buf[:, 2] >> np.uint64(8)).astype(np.int64), \
            (buf[:, 2] & np.uint64(0xf)).astype(np.int64)

    def relocate(self, which: str, align: int, offset: int, vmm: bool = False):
        fn = nat.lib().spmv_hip_csr_relocate_vmm if vmm else nat.lib().spmv_hip_csr_relocate
        _check(fn(self.h, self.ARRAYS.index(which), int(align), int(offset)), "spmv_hip_csr_relocate")

    def set_x(self, x):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if len(x) != self.N:
            raise ValueError(f"x has {len(x)} entries, matrix has {self.N} columns")
        _check(nat.lib().spmv_hip_csr_set_x(self.h, x.ctypes.data_as(C.c_void_p)), "csr_set_x")

    def run(self, variant=CSR_AUTO):
        _check(nat.lib().spmv_hip_csr_run(self.h, int(variant)), "spmv_hip_csr_run")

    def get_y(self):
        y = np.empty(self.M, dtype=self.dtype)
        _check(nat.lib().spmv_hip_csr_get_y(self.h, y.ctypes.data_as(C.c_void_p)), "csr_get_y")
        return y

    def spmv(self, x, variant=CSR_AUTO):
        self.set_x(x)
        self.run(variant)
        return self.get_y()

    def run_on(self, d_x: int, d_y: int, variant=CSR_AUTO, stream: int = 0):
        _check(nat.lib().spmv_hip_csr_run_on(self.h, int(variant), C.c_void_p(d_x),
                                             C.c_void_p(d_y), C.c_void_p(stream)), "csr_run_on")

    x_ptr = property(lambda s: nat.lib().spmv_hip_csr_x_ptr(s.h) or 0)
    y_ptr = property(lambda s: nat.lib().spmv_hip_csr_y_ptr(s.h) or 0)

    def time(self, variant=CSR_AUTO, warmup=5, iters=95, zero_y=True):
        """Per-launch kernel milliseconds, reference protocol (main_cuda.cu:159-200)."""
        ms = np.zeros(iters, dtype=np.float32)
        _check(nat.lib().spmv_hip_csr_time(self.h, int(variant), int(warmup), int(iters),
                                           int(bool(zero_y)), ms.ctypes.data_as(nat.c_float_p)),
               "csr_time")
        return ms

    def time_graph(self, variant=CSR_AUTO, iters=20, replays=10) -> float:
        """ms per SpMV when `iters` launches are replayed from one hipGraph."""
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_time_graph(self.h, int(variant), int(iters), int(replays), C.byref(ms)),
               "csr_time_graph")
        return float(ms.value)

    def spmm(self, X):
        """Y = A X for the k columns of X (N x k, or a vector of N: k = 1) in one pass over the matrix
        (spmv_hip_csr_spmm).  Returns an (M_total, k) array; rows outside the handle's are zero."""
        X = np.asarray(X)
        if X.dtype != self.dtype:
            raise ValueError(f"X has dtype {X.dtype}, the handle holds {np.dtype(self.dtype)}")
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] != self.N or X.shape[1] < 1:
            raise ValueError(f"X must be {self.N} x k with k >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X)
        Y = np.zeros((self.M, X.shape[1]), dtype=self.dtype)
        _check(nat.lib().spmv_hip_csr_spmm(self.h, int(X.shape[1]), X.ctypes.data_as(C.c_void_p),
                                           Y.ctypes.data_as(C.c_void_p)), "spmv_hip_csr_spmm")
        return Y

    def spmm_on(self, d_X: int, d_Y: int, k: int, stream: int = 0):
        """Y = A X on device buffers (row-major N x k and M_total x k, e.g. spmv_hip_malloc or a torch tensor's
        data_ptr()), asynchronous on `stream` (0 = the library's)."""
        _check(nat.lib().spmv_hip_csr_spmm_on(self.h, int(k), C.c_void_p(d_X), C.c_void_p(d_Y), C.c_void_p(stream)),
               "spmv_hip_csr_spmm_on")

    def time_spmm(self, k, warmup=5, iters=95):
        """Per-launch milliseconds of the k-vector product on library-owned X / Y (spmv_hip_csr_spmm_time)."""
        ms = np.zeros(iters, dtype=np.float32)
        _check(nat.lib().spmv_hip_csr_spmm_time(self.h, int(k), int(warmup), int(iters),
                                                ms.ctypes.data_as(nat.c_float_p)), "csr_spmm_time")
        return ms

    def power_iterate(self, iters, variant=CSR_AUTO, bounds=None, use_graph=True):
        """iters steps of x <- A x / ||A x||_2 on the device; returns (lambda, ms_total)."""
        lam, ms = C.c_double(0), C.c_float(0)
        _check(nat.lib().spmv_hip_csr_power_iterate(self.h, int(variant), int(iters), _bounds_arg(bounds),
                                                    int(bool(use_graph)), C.byref(lam), C.byref(ms)),
               "csr_power_iterate")
        return float(lam.value), float(ms.value)

    def cg(self, b, iters, variant=CSR_AUTO, bounds=None, use_halo=False):
        """iters steps of conjugate gradients from x0 = 0 (spmv_hip_csr_cg); returns (x, r.r history, ms)."""
        b = np.ascontiguousarray(b, dtype=self.dtype)
        if len(b) != self.M:
            raise ValueError("b must have M entries")
        x = np.zeros(self.M, dtype=self.dtype)
        hist = np.zeros(iters + 1)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_cg(self.h, int(variant), int(iters), _bounds_arg(bounds), int(bool(use_halo)),
                                         b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                         hist.ctypes.data_as(nat.c_double_p), C.byref(ms)), "spmv_hip_csr_cg")
        return x, hist, float(ms.value)

    def cg_multi(self, B, iters, tol=0.0, bounds=None):
        """k independent CG recurrences from x0 = 0 that share one SpMM per step (spmv_hip_csr_cg_multi), for the k
        columns of B (M x k, or a vector of M: k = 1).  Column j freezes once its r.r <= tol^2 times its initial r.r
        (tol = 0: only at r.r = 0; tol > 0 also ends the loop early once every column is frozen).  Returns
        (X (M, k), r.r history (iters + 1, k), steps each column took [k], ms)."""
        B = np.asarray(B)
        if B.dtype != self.dtype:
            raise ValueError(f"B has dtype {B.dtype}, the handle holds {np.dtype(self.dtype)}")
        if B.ndim == 1:
            B = B.reshape(-1, 1)
        if B.ndim != 2 or B.shape[0] != self.M or not 1 <= B.shape[1] <= 64:
            raise ValueError(f"B must be {self.M} x k with 1 <= k <= 64, got shape {B.shape}")
        _check_iters_tol(iters, tol, finite=False)
        B = np.ascontiguousarray(B)
        k = B.shape[1]
        X = np.zeros((self.M, k), dtype=self.dtype)
        hist = np.zeros((int(iters) + 1, k))
        done = np.zeros(k, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_cg_multi(self.h, int(k), int(iters), float(tol), _bounds_arg(bounds),
                                               B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                               hist.ctypes.data_as(nat.c_double_p), done.ctypes.data_as(nat.c_int_p),
                                               C.byref(ms)), "spmv_hip_csr_cg_multi")
        return X, hist, done, float(ms.value)

    def _check_solve_args(self, b, iters, tol, precond):
        b = _check_vector(b, self.M, self.dtype, "b", "handle")
        _check_iters_tol(iters, tol)
        if precond is not None:
            self._check_precond(precond)
        return b

    def _check_precond(self, precond):
        if not isinstance(precond, Preconditioner):
            raise ValueError("precond must be a Preconditioner (CsrDevice.preconditioner) or None")
        if np.dtype(precond.dtype) != np.dtype(self.dtype):
            raise ValueError(f"the preconditioner holds {np.dtype(precond.dtype)}, the handle "
                             f"{np.dtype(self.dtype)}")
        row0, row1 = self._own_rows()
        if (precond.row0, precond.row0 + precond.rows) != (row0, row1):
            raise ValueError(f"the preconditioner covers rows [{precond.row0}, {precond.row0 + precond.rows}), "
                             f"the handle rows [{row0}, {row1})")

    def preconditioner(self, kind="jacobi", block=1, omega=1.0, ordering="natural", cap=32, theta=0.08, coarse_rows=64,
                       max_levels=16, chain=True, setup="host", block_products=0, degree=4, lmax=None, lmin=None,
                       ratio=30.0) -> "Preconditioner":
        """A preconditioner of this handle's rows; it owns its arrays.  kind "jacobi" (block 1) or "block_jacobi"
        (block in [1, 32]): built on the device (spmv_hip_csr_precond_build).  kind "ssor" (0 < omega < 2; 1 is
        symmetric Gauss-Seidel) or "ilu0": two sparse triangular solves (spmv_hip_csr_precond_build_tri), block 1;
        ordering "natural", or "multicolor": of the rows reordered by a greedy colouring (few dependency levels, more
        steps).  kind "fsai": a sparse lower-triangular G with G^T G ~ A^-1 on the pattern of the lower triangle, at
        most cap (in [1, 32]) entries per row, applied as two SpMVs (spmv_hip_csr_precond_build_fsai); block 1,
        ordering "natural".  kind "amg": smoothed-aggregation multigrid, one V(1,1) cycle per apply
        (spmv_hip_csr_precond_build_amg): strength threshold theta in [0, 1), a coarsest level of at most coarse_rows
        (in [1, 256]) rows solved by its dense inverse, at most max_levels (in [1, 16]) levels, chain: the small
        levels in one launch (the same bits either way); block 1, ordering "natural".  setup "host" (the default) makes
        the hierarchy on the host, "device" on the device (spmv_hip_csr_precond_build_amg_device): the same
        preconditioner byte for byte; block_products (device setup only) goes to its sparse products as in matmul: 0,
        -1 or a power of two in [64, 4096].  kind "chebyshev": a polynomial of `degree` (in [1, 32]) in the
        Jacobi-scaled matrix, degree - 1 SpMVs and degree element-wise passes per apply
        (spmv_hip_csr_precond_build_chebyshev), fitted to the interval [lmin, lmax] of D^-1 A: lmax None is the
        Gershgorin bound of the block, lmin None is lmax / ratio (ratio > 1); block 1, ordering "natural"."""
        if kind not in PRECOND_KINDS:
            raise ValueError(f"kind must be one of {sorted(PRECOND_KINDS)}, got {kind!r}")
        if isinstance(block, bool) or int(block) != block or not 1 <= int(block) <= 32:
            raise ValueError(f"block must be an integer in [1, 32], got {block!r}")
        if kind != "block_jacobi" and int(block) != 1:
            raise ValueError(f"{kind} takes block = 1, got {block}")
        if ordering not in ORDERINGS:
            raise ValueError(f"ordering must be one of {sorted(ORDERINGS)}, got {ordering!r}")
        if kind in ("ssor", "ilu0"):
            if not np.isfinite(float(omega)) or not 0.0 < float(omega) < 2.0:
                raise ValueError(f"omega must lie in (0, 2), got {omega!r}")
            return Preconditioner(self, "spmv_hip_csr_precond_build_tri", PRECOND_KINDS[kind], ORDERINGS[ordering],
                                  float(omega))
        if ordering != "natural":
            raise ValueError(f"{kind} takes ordering = 'natural', got {ordering!r}")
        if kind == "fsai":
            if isinstance(cap, bool) or int(cap) != cap or not 1 <= int(cap) <= 32:
                raise ValueError(f"cap must be an integer in [1, 32], got {cap!r}")
            return Preconditioner(self, "spmv_hip_csr_precond_build_fsai", int(cap))
        if kind == "amg":
            _check_amg_args(theta, coarse_rows, max_levels)
            _check_amg_setup(setup, block_products)
            args = (float(theta), int(coarse_rows), int(max_levels), int(bool(chain)))
            if AMG_SETUPS[setup]:
                return Preconditioner(self, "spmv_hip_csr_precond_build_amg_device", *args, int(block_products))
            return Preconditioner(self, "spmv_hip_csr_precond_build_amg", *args)
        if kind == "chebyshev":
            return Preconditioner(self, "spmv_hip_csr_precond_build_chebyshev",
                                  *_check_chebyshev_args(degree, lmax, lmin, ratio))
        return Preconditioner(self, "spmv_hip_csr_precond_build", PRECOND_KINDS[kind], int(block))

    def triangular(self, lower=True, unit_diagonal=False, ordering="natural") -> "TriangularSolver":
        """The lower (upper) triangle of this handle's diagonal block as a solver of T x = b on the device
        (spmv_hip_csr_trsv_build); it owns a copy of the triangle.  ordering: "natural" only."""
        if ordering not in ORDERINGS:
            raise ValueError(f"ordering must be one of {sorted(ORDERINGS)}, got {ordering!r}")
        if ordering != "natural":
            raise ValueError("a bare triangular solve takes ordering = 'natural': the multicolour order changes which "
                             "matrix a preconditioner factors")
        return TriangularSolver(self, bool(lower), bool(unit_diagonal))

    def pcg(self, b, iters, tol=0.0, precond=None, variant=CSR_AUTO, bounds=None):
        """Preconditioned CG from x0 = 0 (spmv_hip_csr_pcg) for a symmetric positive definite A; precond: a
        Preconditioner of this handle, or None (no preconditioning: csr_cg's bits).  Stops once r.r <= tol^2 times
        the initial r.r (tol = 0: only at exactly 0; tol > 0 also ends the loop early), or at a breakdown.  Returns
        (x, r.r history (iters + 1), r.z history (iters + 1), info {"steps", "status" (PCG_*)}, ms)."""
        b = self._check_solve_args(b, iters, tol, precond)
        x = np.zeros(self.M, dtype=self.dtype)
        rr = np.zeros(int(iters) + 1)
        rz = np.zeros(int(iters) + 1)
        info = np.zeros(2, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_pcg(self.h, None if precond is None else precond.h, int(variant), int(iters),
                                          float(tol), _bounds_arg(bounds),
                                          b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                          rr.ctypes.data_as(nat.c_double_p), rz.ctypes.data_as(nat.c_double_p),
                                          info.ctypes.data_as(nat.c_int_p), C.byref(ms)), "spmv_hip_csr_pcg")
        return x, rr, rz, {"steps": int(info[0]), "status": int(info[1])}, float(ms.value)

    def pcg_multi(self, B, iters, tol=0.0, precond=None, bounds=None):
        """k independent preconditioned CG recurrences from x0 = 0 that share one SpMM per step
        (spmv_hip_csr_pcg_multi), for the k columns of a C-contiguous B (M x k, 1 <= k <= 64) of the handle's dtype.
        precond: a Jacobi, block-Jacobi, FSAI, AMG or Chebyshev Preconditioner of this handle, or None (cg_multi's
        bits); SSOR and ILU(0) take one right-hand side and are refused.  Every column stops on its own, by the rules
        of pcg; tol > 0
        also ends the loop early once every column has stopped.  Returns (X (M, k), r.r history (iters + 1, k), r.z
        history (iters + 1, k), info {"steps": int array [k], "status": int array [k] (PCG_*)}, ms)."""
        B = _check_columns(B, self.M, self.dtype, "B", "handle")
        _check_iters_tol(iters, tol)
        if precond is not None:
            self._check_precond(precond)
        k = B.shape[1]
        X = np.zeros((self.M, k), dtype=self.dtype)
        rr = np.zeros((int(iters) + 1, k))
        rz = np.zeros((int(iters) + 1, k))
        steps = np.zeros(k, dtype=np.int32)
        status = np.zeros(k, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_pcg_multi(self.h, None if precond is None else precond.h, int(k), int(iters),
                                                float(tol), _bounds_arg(bounds),
                                                B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                                rr.ctypes.data_as(nat.c_double_p), rz.ctypes.data_as(nat.c_double_p),
                                                steps.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p),
                                                C.byref(ms)), "spmv_hip_csr_pcg_multi")
        return X, rr, rz, {"steps": steps, "status": status}, float(ms.value)

    def bicgstab(self, b, iters, tol=0.0, variant=CSR_AUTO, bounds=None, precond=None):
        """BiCGSTAB from x0 = 0 with shadow residual r^ = b (spmv_hip_csr_bicgstab), for a square, possibly
        nonsymmetric A.  Stops once r.r (or s.s at a half step) <= tol^2 times the initial r.r (tol = 0: only at
        exactly 0; tol > 0 also ends the loop early), or at a breakdown.  precond: a Preconditioner of this handle
        applied from the right (spmv_hip_csr_pbicgstab; r stays the true residual), or None.  Returns (x, r.r history
        (iters + 1), info {"steps", "status" (BICG_*), "half_step"}, ms)."""
        b = self._check_solve_args(b, iters, tol, precond)
        x = np.zeros(self.M, dtype=self.dtype)
        hist = np.zeros(int(iters) + 1)
        info = np.zeros(3, dtype=np.int32)
        ms = C.c_float(0)
        args = (int(variant), int(iters), float(tol), _bounds_arg(bounds), b.ctypes.data_as(C.c_void_p),
                x.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                info.ctypes.data_as(nat.c_int_p), C.byref(ms))
        if precond is None:
            _check(nat.lib().spmv_hip_csr_bicgstab(self.h, *args), "spmv_hip_csr_bicgstab")
        else:
            _check(nat.lib().spmv_hip_csr_pbicgstab(self.h, precond.h, *args), "spmv_hip_csr_pbicgstab")
        return x, hist, {"steps": int(info[0]), "status": int(info[1]), "half_step": int(info[2])}, float(ms.value)

    def bicgstab_multi(self, B, iters, tol=0.0, precond=None, bounds=None):
        """k independent right-preconditioned BiCGSTAB recurrences from x0 = 0 that share the two SpMMs of a step
        (spmv_hip_csr_bicgstab_multi), for the k columns of a C-contiguous B (M x k, 1 <= k <= 64) of the handle's
        dtype and a square, possibly nonsymmetric A.  precond: a Jacobi, block-Jacobi, FSAI, AMG or Chebyshev
        Preconditioner of this handle, or None; SSOR and ILU(0) take one right-hand side and are refused.  Every
        column stops on its own, by the rules of bicgstab; tol > 0 also ends the loop early once every column has
        stopped.  Returns (X (M, k), r.r history (iters + 1, k), info {"steps", "status" (BICG_*), "half_step"}: int
        arrays [k], ms)."""
        B = _check_columns(B, self.M, self.dtype, "B", "handle")
        _check_iters_tol(iters, tol)
        if precond is not None:
            self._check_precond(precond)
        k = B.shape[1]
        X = np.zeros((self.M, k), dtype=self.dtype)
        hist = np.zeros((int(iters) + 1, k))
        steps = np.zeros(k, dtype=np.int32)
        status = np.zeros(k, dtype=np.int32)
        half = np.zeros(k, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_bicgstab_multi(self.h, None if precond is None else precond.h, int(k), int(iters),
                                                     float(tol), _bounds_arg(bounds),
                                                     B.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                                     hist.ctypes.data_as(nat.c_double_p),
                                                     steps.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p),
                                                     half.ctypes.data_as(nat.c_int_p), C.byref(ms)),
               "spmv_hip_csr_bicgstab_multi")
        return X, hist, {"steps": steps, "status": status, "half_step": half}, float(ms.value)

    def minres(self, b, iters, tol=0.0, shift=0.0, precond=None, variant=CSR_AUTO, bounds=None):
        """MINRES from x0 = 0 (spmv_hip_csr_minres) for (A - shift I) x = b with a symmetric, possibly indefinite A:
        one SpMV per step, a residual norm that never grows.  precond: a Preconditioner of this handle that is
        symmetric positive definite (it is used as built, the shift goes to A alone), or None.  Stops once the
        recurrence's r.r (r.M^-1 r with a preconditioner) <= tol^2 times its initial value (tol = 0: only at exactly
        0; tol > 0 also ends the loop early), or at a breakdown.  Returns (x, that r.r history (iters + 1), info
        {"steps", "status" (MINRES_*)}, ms)."""
        if not np.isfinite(float(shift)):
            raise ValueError(f"shift must be finite, got {shift}")
        b = self._check_solve_args(b, iters, tol, precond)
        x = np.zeros(self.M, dtype=self.dtype)
        hist = np.zeros(int(iters) + 1)
        info = np.zeros(2, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_minres(self.h, None if precond is None else precond.h, int(variant), int(iters),
                                             float(tol), float(shift), _bounds_arg(bounds),
                                             b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                             hist.ctypes.data_as(nat.c_double_p), info.ctypes.data_as(nat.c_int_p),
                                             C.byref(ms)), "spmv_hip_csr_minres")
        return x, hist, {"steps": int(info[0]), "status": int(info[1])}, float(ms.value)

    def minres_multi(self, B, iters, tol=0.0, shift=0.0, precond=None, bounds=None):
        """k independent MINRES recurrences from x0 = 0 that share one SpMM per step (spmv_hip_csr_minres_multi), for
        (A - shift_j I) x_j = b_j with the k columns of a C-contiguous B (M x k, 1 <= k <= 64) of the handle's dtype
        and a symmetric, possibly indefinite A.  shift: one value for every column, or k values.  precond: a Jacobi,
        block-Jacobi, FSAI, AMG or Chebyshev Preconditioner of this handle that is symmetric positive definite, or
        None; SSOR and ILU(0) take one right-hand side and are refused.  Every column stops on its own, by the rules
        of minres; tol > 0 also ends the loop early once every column has stopped.  Returns (X (M, k), the
        recurrence's r.r history (iters + 1, k), info {"steps", "status" (MINRES_*)}: int arrays [k], ms)."""
        B = _check_columns(B, self.M, self.dtype, "B", "handle")
        _check_iters_tol(iters, tol)
        k = B.shape[1]
        shifts = np.asarray(shift, dtype=np.float64)
        if shifts.ndim == 0:
            shifts = np.full(k, float(shifts))
        if shifts.shape != (k,):
            raise ValueError(f"shift must be a scalar or {k} values, got shape {shifts.shape}")
        if not np.all(np.isfinite(shifts)):
            raise ValueError(f"shift must be finite, got {shift}")
        shifts = np.ascontiguousarray(shifts)
        if precond is not None:
            self._check_precond(precond)
        X = np.zeros((self.M, k), dtype=self.dtype)
        hist = np.zeros((int(iters) + 1, k))
        steps = np.zeros(k, dtype=np.int32)
        status = np.zeros(k, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_minres_multi(self.h, None if precond is None else precond.h, int(k), int(iters),
                                                   float(tol), shifts.ctypes.data_as(nat.c_double_p),
                                                   _bounds_arg(bounds), B.ctypes.data_as(C.c_void_p),
                                                   X.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                                   steps.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p),
                                                   C.byref(ms)), "spmv_hip_csr_minres_multi")
        return X, hist, {"steps": steps, "status": status}, float(ms.value)

    def gmres(self, b, iters, tol=0.0, restart=30, precond=None, variant=CSR_AUTO):
        """Restarted GMRES(restart) from x0 = 0 (spmv_hip_csr_gmres) for a square, possibly nonsymmetric A held whole
        by this handle: one SpMV per step, classical Gram-Schmidt done twice, a residual estimate that never grows
        inside a cycle.  restart in [1, 64].  precond: a Preconditioner of this handle of any kind, applied from the
        right (the history stays that of the true residual), or None.  Stops once the estimate <= tol^2 times b.b
        (tol = 0: only at exactly 0), or at a breakdown; the host reads the stop state once per cycle.  Returns (x,
        squared residual estimate history (iters + 1), info {"steps", "status" (GMRES_*), "cycles"}, ms)."""
        b = self._check_solve_args(b, iters, tol, precond)
        if isinstance(restart, bool) or int(restart) != restart or not 1 <= int(restart) <= GMRES_MAX_RESTART:
            raise ValueError(f"restart must be an integer in [1, {GMRES_MAX_RESTART}], got {restart!r}")
        x = np.zeros(self.M, dtype=self.dtype)
        hist = np.zeros(int(iters) + 1)
        info = np.zeros(3, dtype=np.int32)
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_csr_gmres(self.h, None if precond is None else precond.h, int(variant), int(restart),
                                            int(iters), float(tol), b.ctypes.data_as(C.c_void_p),
                                            x.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(nat.c_double_p),
                                            info.ctypes.data_as(nat.c_int_p), C.byref(ms)), "spmv_hip_csr_gmres")
        return x, hist, {"steps": int(info[0]), "status": int(info[1]), "cycles": int(info[2])}, float(ms.value)

    def lobpcg(self, k, iters, tol=0.0, precond=None, X0=None, largest=False, seed=0):
        """LOBPCG (spmv_hip_csr_lobpcg) for the k smallest (largest=True: largest) eigenpairs of a symmetric fp64 A,
        1 <= k <= 16, n >= 4 k.  precond: a Jacobi, block-Jacobi, FSAI, AMG or Chebyshev Preconditioner of this handle
        (smallest only), or None.  X0: n x k starting block (None:
        np.random.default_rng(seed).standard_normal((n, k))).  Stops as
        converged once tol > 0 and every residual norm <= tol ||A||_inf; tol = 0 runs exactly `iters` steps (the host
        reads the Gram matrices in every step either way).  Returns (w [k] ascending (largest: descending), X (n, k),
        theta history (iters + 1, k), residual-norm history (iters + 1, k), info {"steps", "status" (LOBPCG_*),
        "restarts", "min_basis", "resid" [k] (the true ||A x - w x||), "anorm", "host_ms"}, ms)."""
        if np.dtype(self.dtype) != np.dtype(np.float64):
            raise ValueError(f"lobpcg needs an fp64 handle, this one holds {np.dtype(self.dtype)}")
        if self.M != self.N:
            raise ValueError(f"lobpcg needs a square matrix, got {self.M} x {self.N}")
        if self._own_rows() != (0, self.M):
            raise ValueError(f"lobpcg needs the whole matrix, the handle holds rows {self._own_rows()}")
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= LOBPCG_MAX_K:
            raise ValueError(f"k must be an integer in [1, {LOBPCG_MAX_K}], got {k!r}")
        k = int(k)
        if self.M < 4 * k:
            raise ValueError(f"lobpcg needs n >= 4 k = {4 * k}, got n = {self.M}")
        _check_iters_tol(iters, tol)
        if precond is not None:
            self._check_precond(precond)
            if precond.kind in (PRECOND_SSOR, PRECOND_ILU0):
                raise ValueError("lobpcg: SSOR and ILU(0) take one right-hand side, they have no k-wide apply")
            if largest:
                raise ValueError("lobpcg: a preconditioner serves the smallest eigenvalues only")
        from .distributed import NativeComm  # (distributed imports this module)
        if NativeComm.active:
            raise ValueError("lobpcg runs on one device, a communicator is active (NativeComm.close() first)")
        if X0 is None:
            X0 = np.random.default_rng(seed).standard_normal((self.M, k))
        X0 = np.asarray(X0)
        if X0.dtype != np.float64 or X0.shape != (self.M, k):
            raise ValueError(f"X0 must be a float64 array of shape ({self.M}, {k}), got {X0.dtype} {X0.shape}")
        X0 = np.ascontiguousarray(X0)
        iters = int(iters)
        w, X, resid = np.zeros(k), np.zeros((self.M, k)), np.zeros(k)
        th, rh = np.zeros((iters + 1, k)), np.zeros((iters + 1, k))
        words = np.zeros(4, dtype=np.int32)
        anorm, ms, host_ms = C.c_double(0), C.c_float(0), C.c_float(0)
        dp = nat.c_double_p
        _check(nat.lib().spmv_hip_csr_lobpcg(self.h, None if precond is None else precond.h, k, iters, float(tol),
                                             int(bool(largest)), X0.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                             X.ctypes.data_as(dp), th.ctypes.data_as(dp), rh.ctypes.data_as(dp),
                                             resid.ctypes.data_as(dp), C.byref(anorm), words.ctypes.data_as(nat.c_int_p),
                                             C.byref(ms), C.byref(host_ms)), "spmv_hip_csr_lobpcg")
        info = {"steps": int(words[0]), "status": int(words[1]), "restarts": int(words[2]), "min_basis": int(words[3]),
                "resid": resid, "anorm": float(anorm.value), "host_ms": float(host_ms.value)}
        return w, X, th, rh, info, float(ms.value)

    def cgls(self, b, iters, tol=0.0, damp=0.0, at=None):
        """CGLS from x0 = 0 for min ||A x - b||^2 + damp^2 ||x||^2, A of any shape (spmv_hip_csr_cgls).  at: a
        transpose of this handle (CsrDevice.transpose); None: one is built for the call and freed after it (its build
        is not part of ms).  Stops once s.s <= tol^2 times the initial s.s (tol = 0: only at exactly 0; tol > 0 also
        ends the loop early), or at a breakdown.  Returns (x (N), s.s history (iters + 1), r.r history (iters + 1),
        info {"steps", "status" (CGLS_*)}, ms)."""
        b = _check_vector(b, self.M, self.dtype, "b", "handle")
        _check_iters_tol(iters, tol)
        if not float(damp) >= 0.0 or not np.isfinite(float(damp)):
            raise ValueError(f"damp must be finite and >= 0, got {damp}")
        if at is not None and not isinstance(at, CsrDevice):
            raise ValueError("at must be a CsrDevice holding the transpose")
        own = at is None
        if own:
            at = self.transpose()
        try:
            x = np.zeros(self.N, dtype=self.dtype)
            ss = np.zeros(int(iters) + 1)
            rr = np.zeros(int(iters) + 1)
            info = np.zeros(2, dtype=np.int32)
            ms = C.c_float(0)
            _check(nat.lib().spmv_hip_csr_cgls(self.h, at.h, int(iters), float(tol), float(damp),
                                               b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                               ss.ctypes.data_as(nat.c_double_p), rr.ctypes.data_as(nat.c_double_p),
                                               info.ctypes.data_as(nat.c_int_p), C.byref(ms)), "spmv_hip_csr_cgls")
        finally:
            if own:
                at.close()
        return x, ss, rr, {"steps": int(info[0]), "status": int(info[1])}, float(ms.value)

    def split_interior(self) -> dict:
        """Split the x-window blocks into interior (own range of x only) and boundary ones
        (spmv_hip_csr_split_interior); returns the block and entry counts."""
        counts = (C.c_longlong * 4)()
        _check(nat.lib().spmv_hip_csr_split_interior(self.h, counts), "spmv_hip_csr_split_interior")
        return dict(zip(("interior_blocks", "boundary_blocks", "interior_entries", "boundary_entries"),
                        (int(v) for v in counts)))

    def split_columns(self, col_lo: int, col_hi: int) -> dict:
        """Split the handle's entries by column ([col_lo, col_hi) = the rank's own range of x) into two sub-handles
        (spmv_hip_csr_split_columns); returns the entry counts inside / outside the range."""
        counts = (C.c_longlong * 2)()
        _check(nat.lib().spmv_hip_csr_split_columns(self.h, int(col_lo), int(col_hi), counts), "spmv_hip_csr_split_columns")
        return {"own_entries": int(counts[0]), "halo_entries": int(counts[1])}

    def run_split(self, part: int):
        """part 0: y = A_own x (own range of x only); part 1: y += A_halo x (asynchronous on the library stream)."""
        _check(nat.lib().spmv_hip_csr_run_split(self.h, int(part), None, None, None), "spmv_hip_csr_run_split")

    def run_part(self, part: int):
        """part 0: interior blocks only; part 1: the rest (asynchronous on the library stream)."""
        _check(nat.lib().spmv_hip_csr_run_part(self.h, int(part), None, None, None), "spmv_hip_csr_run_part")

    def power_iterate_halo(self, iters, variant=CSR_AUTO):
        """power_iterate with the halo exchange (NativeComm.halo_setup first when a communicator exists)."""
        lam, ms = C.c_double(0), C.c_float(0)
        _check(nat.lib().spmv_hip_csr_power_iterate_halo(self.h, int(variant), int(iters), C.byref(lam), C.byref(ms)),
               "csr_power_iterate_halo")
        return float(lam.value), float(ms.value)

    def get_x(self):
        x = np.empty(self.N, dtype=self.dtype)
        _check(nat.lib().spmv_hip_memcpy_d2h(x.ctypes.data_as(C.c_void_p), C.c_void_p(self.x_ptr), x.nbytes),
               "memcpy_d2h")
        return x

    def step_time(self, bounds, variant=CSR_AUTO, warmup=5, iters=95):
        """Multi-GPU step (SpMV + all-gatherv of y): per-step kernel and exchange ms."""
        b = np.ascontiguousarray(bounds, dtype=np.int32)
        mk, mx = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
        _check(nat.lib().spmv_hip_csr_step_time(self.h, int(variant), b.ctypes.data_as(nat.c_int_p),
                                                int(warmup), int(iters),
                                                mk.ctypes.data_as(nat.c_float_p),
                                                mx.ctypes.data_as(nat.c_float_p)), "csr_step_time")
        return mk, mx


def lobpcg_rr(GB, GA, nb, k, largest=False, drop=LOBPCG_DROP):
    """The Rayleigh-Ritz step of lobpcg on the host (spmv_lobpcg_rr): GB = S^T S, GA = S^T AS, both (nb k) x (nb k).
    Returns (rc (0, or 1: breakdown), theta [k], C (nb k, k), Cp (nb k, k), kept, restarted)."""
    m = int(nb) * int(k)
    GB = np.ascontiguousarray(GB, dtype=np.float64)
    GA = np.ascontiguousarray(GA, dtype=np.float64)
    if GB.shape != (m, m) or GA.shape != (m, m):
        raise ValueError(f"GB and GA must be {m} x {m}, got {GB.shape} and {GA.shape}")
    theta, Cm, Cp = np.zeros(int(k)), np.zeros((m, int(k))), np.zeros((m, int(k)))
    kept, restarted = C.c_int(0), C.c_int(0)
    dp = nat.c_double_p
    rc = nat.lib().spmv_lobpcg_rr(int(nb), int(k), GB.ctypes.data_as(dp), GA.ctypes.data_as(dp), int(bool(largest)),
                                  float(drop), theta.ctypes.data_as(dp), Cm.ctypes.data_as(dp), Cp.ctypes.data_as(dp),
                                  C.byref(kept), C.byref(restarted))
    if rc < 0:
        raise ValueError(f"spmv_lobpcg_rr refused nb = {nb}, k = {k}, drop = {drop}")
    return rc, theta, Cm, Cp, int(kept.value), int(restarted.value)


def _block_pointers(blocks):
    arr = (C.c_void_p * 3)()
    for i, p in enumerate(blocks):
        arr[i] = C.c_void_p(p) if p else None
    return arr


def lobpcg_gram(n, k, nb, d_S, d_AS):
    """The Gram pass of lobpcg alone (spmv_hip_lobpcg_gram) on device arrays: d_S, d_AS are up to 3 device addresses
    of row-major n x k fp64 blocks (those from nb on may be 0).  Returns (S^T S, S^T AS), each (nb k) x (nb k)."""
    m = int(nb) * int(k)
    GB, GA = np.zeros((m, m)), np.zeros((m, m))
    _check(nat.lib().spmv_hip_lobpcg_gram(int(n), int(k), int(nb), _block_pointers(d_S), _block_pointers(d_AS),
                                          GB.ctypes.data_as(nat.c_double_p), GA.ctypes.data_as(nat.c_double_p)),
           "spmv_hip_lobpcg_gram")
    return GB, GA


def lobpcg_update(n, k, nb, d_S, d_AS, Cm, Cp, d_X, d_P, d_AX, d_AP):
    """The update pass of lobpcg alone (spmv_hip_lobpcg_update): X = S C, P = S Cp, AX = AS C, AP = AS Cp on device
    arrays; the outputs may be blocks of S / AS."""
    m = int(nb) * int(k)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    Cp = np.ascontiguousarray(Cp, dtype=np.float64)
    if Cm.shape != (m, int(k)) or Cp.shape != (m, int(k)):
        raise ValueError(f"C and Cp must be {m} x {k}, got {Cm.shape} and {Cp.shape}")
    _check(nat.lib().spmv_hip_lobpcg_update(int(n), int(k), int(nb), _block_pointers(d_S), _block_pointers(d_AS),
                                            Cm.ctypes.data_as(nat.c_double_p), Cp.ctypes.data_as(nat.c_double_p),
                                            C.c_void_p(d_X), C.c_void_p(d_P), C.c_void_p(d_AX), C.c_void_p(d_AP)),
           "spmv_hip_lobpcg_update")


def gmres_dots(d_V, ld, nvec, d_w, n, value_bytes):
    """The dot-product pass of gmres alone (spmv_hip_gmres_dots) on device arrays: d_V the address of nvec basis
    vectors of n values, ld elements apart (ld * value_bytes a multiple of 16), d_w that of w.  Returns V^T w [nvec]."""
    h = np.zeros(max(int(nvec), 1))
    _check(nat.lib().spmv_hip_gmres_dots(C.c_void_p(d_V), int(ld), int(nvec), C.c_void_p(d_w), int(n),
                                         int(value_bytes), h.ctypes.data_as(nat.c_double_p)), "spmv_hip_gmres_dots")
    return h[:int(nvec)]


def gmres_update(d_V, ld, nvec, h, d_w, n, value_bytes, want_ww=True):
    """The update pass of gmres alone (spmv_hip_gmres_update): w <- w - V h on device arrays, each value rounded once.
    Returns w.w of what was stored (None when not wanted)."""
    h = np.ascontiguousarray(h, dtype=np.float64)
    if h.shape != (int(nvec),):
        raise ValueError(f"h must hold {nvec} values, got shape {h.shape}")
    ww = C.c_double(0)
    _check(nat.lib().spmv_hip_gmres_update(C.c_void_p(d_V), int(ld), int(nvec), h.ctypes.data_as(nat.c_double_p),
                                           C.c_void_p(d_w), int(n), int(value_bytes),
                                           C.byref(ww) if want_ww else None), "spmv_hip_gmres_update")
    return float(ww.value) if want_ww else None


def _bounds_arg(bounds):
    """The row bounds of the ranks as the int pointer a solver entry takes; None (no communicator) stays None"""
    if bounds is None:
        return None
    return np.ascontiguousarray(bounds, dtype=np.int32).ctypes.data_as(nat.c_int_p)  # (the pointer keeps the array)


def _check_iters_tol(iters, tol, finite=True):
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    if not float(tol) >= 0.0 or finite and not np.isfinite(float(tol)):
        raise ValueError(f"tol must be {'finite and ' if finite else ''}>= 0, got {tol}")


def _check_vector(v, rows, dtype, name, owner):
    v = np.asarray(v)
    if v.dtype != dtype:
        raise ValueError(f"{name} has dtype {v.dtype}, the {owner} holds {np.dtype(dtype)}")
    if v.ndim != 1 or v.shape[0] != rows:
        raise ValueError(f"{name} must be a vector of {rows} values, got shape {v.shape}")
    return np.ascontiguousarray(v)


def _check_columns(A, rows, dtype, name, owner):
    """A as it is when it is a C-contiguous rows x k array of dtype with 1 <= k <= 64; else ValueError"""
    A = np.asarray(A)
    if A.dtype != dtype:
        raise ValueError(f"{name} has dtype {A.dtype}, the {owner} holds {np.dtype(dtype)}")
    if A.ndim != 2 or A.shape[0] != rows or not 1 <= A.shape[1] <= 64:
        raise ValueError(f"{name} must be {rows} x k with 1 <= k <= 64, got shape {A.shape}")
    if not A.flags.c_contiguous:
        raise ValueError(f"{name} must be C-contiguous (row-major {rows} x k)")
    return A


class TriangularSolver(_Handle):
    """x with T x = b for a triangle of a CsrDevice's diagonal block, resident in HBM in level order
    (CsrDevice.triangular).  It owns its arrays: the handle it was built from may be freed first."""

    _free = "spmv_hip_trsv_free"

    def __init__(self, dev: CsrDevice, lower: bool, unit_diagonal: bool):
        super().__init__()
        _check(nat.lib().spmv_hip_csr_trsv_build(dev.h, TRSV_LOWER if lower else TRSV_UPPER,
                                                 TRSV_UNIT if unit_diagonal else TRSV_NONUNIT, ORDER_NATURAL,
                                                 C.byref(self.h)), "spmv_hip_csr_trsv_build")
        info = self.info()
        self.rows, self.row0 = info["rows"], info["row0"]
        self.dtype = np.float64 if info["value_bytes"] == 8 else np.float32

    def info(self) -> dict:
        out = (C.c_int * len(TRSV_INFO))()
        _check(nat.lib().spmv_hip_trsv_info(self.h, out), "spmv_hip_trsv_info")
        return dict(zip(TRSV_INFO, (int(v) for v in out)))

    def solve(self, b):
        """x with T x = b for b of `rows` values (element i = row row0 + i) of the handle's dtype."""
        b = _check_vector(b, self.rows, self.dtype, "b", "solver")
        x = np.zeros(self.rows, dtype=self.dtype)
        _check(nat.lib().spmv_hip_trsv_solve(self.h, b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)),
               "spmv_hip_trsv_solve")
        return x

    def refresh(self, dev: CsrDevice):
        """The solver from the values dev holds now (spmv_hip_trsv_refresh): dev is a handle of the solver's dtype, rows
        and row0 with the pattern it was built from, normally the same handle after update_values.  The level order and
        the launch plan stay; the solver then is, byte for byte, a fresh build on a fresh upload of dev's arrays.  All or
        nothing: a refusal (the build's words, with its row) leaves the solver as it was."""
        _check(nat.lib().spmv_hip_trsv_refresh(self.h, dev.h), "spmv_hip_trsv_refresh")

    def solve_on(self, d_b: int, d_x: int, stream: int = 0):
        """The same on device vectors (b and x must not overlap), asynchronous on `stream` (0 = the library's)."""
        _check(nat.lib().spmv_hip_trsv_solve_on(self.h, C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(stream)),
               "spmv_hip_trsv_solve_on")


def identity(n, dtype=np.float64) -> CsrDevice:
    """I_n as a handle (a plain upload), for A + sigma I: A.add(sp.identity(n), beta=sigma)."""
    n = int(n)
    if n < 0:
        raise ValueError(f"identity: n = {n}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"identity: dtype {np.dtype(dtype)}; float64 or float32")
    return CsrDevice(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, dtype=dtype))


def spgemm_plan(products, block_products, max_rows=SPGEMM_MAX_ROWS):
    """The row plan of CsrDevice.matmul (spmv_spgemm_plan; no device needed) from the rows' product counts:
    (block_row, long_rows).  Blocks k = rows [block_row[k], block_row[k + 1]) partition the rows in order; a long row
    (more than block_products products; with -1 any product) is the last row of its block and is listed in long_rows;
    the other rows of a block hold at most block_products products (0 = 4096) and a block at most max_rows rows."""
    products = np.ascontiguousarray(products, dtype=np.int64)
    if products.ndim != 1:
        raise ValueError("products must be one-dimensional")
    M = products.size
    block_row, long_row = np.zeros(M + 1, dtype=np.int32), np.zeros(max(M, 1), dtype=np.int32)
    nb, nl = C.c_int(), C.c_int()
    rc = nat.lib().spmv_spgemm_plan(M, products.ctypes.data_as(C.POINTER(C.c_longlong)), int(block_products), int(max_rows),
                                    block_row.ctypes.data_as(nat.c_int_p), C.byref(nb), long_row.ctypes.data_as(nat.c_int_p),
                                    C.byref(nl))
    if rc != 0:
        raise ValueError(f"spgemm_plan refused block_products = {block_products}, max_rows = {max_rows} "
                         f"(0, -1 or a power of two in [64, 4096]; 1 .. 4096 rows; counts >= 0)")
    return block_row[:nb.value + 1].copy(), long_row[:nl.value].copy()


def rcm_chain_nodes():
    """(smallest, largest, auto): the chain_nodes CsrDevice.rcm takes beside 0 and -1 (spmv_hip_rcm_chain_nodes)."""
    lo, hi, auto = C.c_int(), C.c_int(), C.c_int()
    nat.lib().spmv_hip_rcm_chain_nodes(C.byref(lo), C.byref(hi), C.byref(auto))
    return lo.value, hi.value, auto.value


def rcm_plan(row_ptr, col, n, peripheral=2):
    """(perm, info): the reverse Cuthill-McKee ordering of an n x n CSR pattern on one host thread (spmv_rcm_plan_build;
    no device needed): the serial loop of include/spmv_hip.h, which CsrDevice.rcm reproduces.  New row i is old row
    perm[i].  info holds RCM_STATS (the device's counters are 0)."""
    n, peripheral = int(n), int(peripheral)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    if n < 0 or row_ptr.ndim != 1 or row_ptr.size != n + 1:
        raise ValueError(f"rcm_plan: row_ptr needs n + 1 = {n + 1} entries")
    if col.ndim != 1 or col.size < int(row_ptr[-1]):
        raise ValueError(f"rcm_plan: col holds {col.size} entries, row_ptr ends at {int(row_ptr[-1])}")
    if not 0 <= peripheral <= RCM_MAX_PERIPHERAL:
        raise ValueError(f"rcm_plan: peripheral = {peripheral}; 0 .. {RCM_MAX_PERIPHERAL}")
    perm = np.zeros(n, dtype=np.int32)
    stats = (C.c_longlong * len(RCM_STATS))()
    rc = nat.lib().spmv_rcm_plan_build(n, row_ptr.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p), peripheral,
                                       perm.ctypes.data_as(nat.c_int_p), stats)
    if rc == -2:
        raise MemoryError("rcm_plan: out of memory")
    if rc != 0:
        raise ValueError("rcm_plan: row_ptr must start at 0 and ascend, and every column must lie in [0, n)")
    return perm, dict(zip(RCM_STATS, (int(v) for v in stats)))


def _check_amg_args(theta, coarse_rows, max_levels):
    if not np.isfinite(float(theta)) or not 0.0 <= float(theta) < 1.0:
        raise ValueError(f"theta must lie in [0, 1), got {theta!r}")
    if isinstance(coarse_rows, bool) or int(coarse_rows) != coarse_rows or not 1 <= int(coarse_rows) <= AMG_MAX_COARSE_ROWS:
        raise ValueError(f"coarse_rows must be an integer in [1, {AMG_MAX_COARSE_ROWS}], got {coarse_rows!r}")
    if isinstance(max_levels, bool) or int(max_levels) != max_levels or not 1 <= int(max_levels) <= AMG_MAX_LEVELS:
        raise ValueError(f"max_levels must be an integer in [1, {AMG_MAX_LEVELS}], got {max_levels!r}")


def _check_amg_setup(setup, block_products):
    if not isinstance(setup, str) or setup not in AMG_SETUPS:
        raise ValueError(f"setup must be one of {sorted(AMG_SETUPS)}, got {setup!r}")
    bp = block_products
    if isinstance(bp, bool) or int(bp) != bp or not (bp in (0, -1) or (64 <= bp <= SPGEMM_MAX_BLOCK_PRODUCTS
                                                                         and int(bp) & (int(bp) - 1) == 0)):
        raise ValueError(f"block_products must be 0 (auto), -1 (global tier only) or a power of two in "
                         f"[64, {SPGEMM_MAX_BLOCK_PRODUCTS}], got {bp!r}")
    if setup == "host" and int(bp) != 0:
        raise ValueError(f"block_products belongs to setup='device'; the host setup forms no device products, got {bp!r}")


def _amg_levels(read, levels, dtype, with_t):
    """The levels of an AMG hierarchy through a reader read(level, which, row_ptr, col, val, scalars) (the plan's on
    the host, a Preconditioner's on the device)."""
    out = []
    for lv in range(levels):
        sc = np.zeros(5)
        dp = sc.ctypes.data_as(nat.c_double_p)
        read(lv, AMG_A, None, None, None, dp)
        entry = {"w": float(sc[0]), "rho": float(sc[1]), "kind": int(sc[2]), "rows": int(sc[3]), "aggregates": int(sc[4])}
        names = [("A", AMG_A, entry["rows"])]
        if entry["kind"] == AMG_NOT_COARSEST:
            names += [("P", AMG_P, entry["rows"]), ("R", AMG_R, entry["aggregates"])]
            if with_t:
                names.append(("T", AMG_T, entry["rows"]))
        elif entry["kind"] == AMG_DIRECT:
            names.append(("inv", AMG_INV, entry["rows"]))
        for name, which, rows in names:
            rp = np.zeros(rows + 1, dtype=np.int32)
            read(lv, which, rp.ctypes.data_as(nat.c_int_p), None, None, None)
            col = np.zeros(max(int(rp[-1]), 1), dtype=np.int32)
            val = np.zeros(max(int(rp[-1]), 1), dtype=dtype)
            read(lv, which, rp.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p),
                 val.ctypes.data_as(nat.c_double_p if with_t else C.c_void_p), None)
            entry[name] = (rp, col[:rp[-1]], val[:rp[-1]])
        out.append(entry)
    return out


def _check_chebyshev_args(degree, lmax, lmin, ratio):
    """(degree, lmin, lmax, ratio) as the library takes them (None: 0.0, the default), or ValueError"""
    if isinstance(degree, bool) or not isinstance(degree, (int, float, np.integer, np.floating)) or \
            not np.isfinite(float(degree)) or int(degree) != degree or not 1 <= int(degree) <= CHEBYSHEV_MAX_DEGREE:
        raise ValueError(f"degree must be an integer in [1, {CHEBYSHEV_MAX_DEGREE}], got {degree!r}")
    bounds = {}
    for name, v in (("lmax", lmax), ("lmin", lmin)):
        v = 0.0 if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not np.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError(f"{name} must be None or finite and >= 0, got {v!r}")
        bounds[name] = float(v)
    if bounds["lmax"] > 0.0 and bounds["lmin"] > 0.0 and bounds["lmin"] >= bounds["lmax"]:
        raise ValueError(f"lmin must be below lmax, got lmin = {lmin!r}, lmax = {lmax!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or \
            not np.isfinite(float(ratio)) or not float(ratio) > 1.0:
        raise ValueError(f"ratio must be finite and > 1, got {ratio!r}")
    return int(degree), bounds["lmin"], bounds["lmax"], float(ratio)


def chebyshev_coefficients(degree, lmin, lmax):
    """(a, b): the coefficients of the Chebyshev polynomial preconditioner of `degree` on [lmin, lmax]
    (spmv_chebyshev_coefficients; no device needed), 0 < lmin < lmax:
    theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma, a_0 = 0,
    b_0 = 1 / theta, then rho_j = 1 / (2 sigma - rho_{j-1}), a_j = rho_j rho_{j-1}, b_j = 2 rho_j / delta."""
    degree, lmin, lmax, _ = _check_chebyshev_args(degree, lmax, lmin, 2.0)
    if not 0.0 < lmin < lmax:
        raise ValueError(f"the interval must satisfy 0 < lmin < lmax, got [{lmin!r}, {lmax!r}]")
    a, b = np.zeros(degree), np.zeros(degree)
    if nat.lib().spmv_chebyshev_coefficients(degree, lmin, lmax, a.ctypes.data_as(nat.c_double_p),
                                             b.ctypes.data_as(nat.c_double_p)) != 0:
        raise ValueError(f"no coefficients for degree {degree} on [{lmin!r}, {lmax!r}]")
    return a, b


def amg_plan(row_ptr, col, val, theta=0.08, coarse_rows=64, max_levels=16) -> list:
    """The host setup of the AMG preconditioner alone (spmv_amg_plan_build; no device needed) on an n x n CSR matrix
    with canonical rows (ascending columns, no repeats): the levels as Preconditioner.levels() returns them, in fp64,
    with "T" (the aggregates: T[i, agg(i)] = 1) beside "P" and "R".  A refusal raises SpmvHipError with the setup's
    message (the row at level 0, the level below it)."""
    _check_amg_args(theta, coarse_rows, max_levels)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    if rp.ndim != 1 or rp.size < 1 or col.shape != val.shape or col.ndim != 1 or col.size < int(rp[-1]):
        raise ValueError("row_ptr (n + 1), col and val (row_ptr[n] each) do not fit together")
    L = nat.lib()
    plan = C.c_void_p()

    def check(rc):
        if rc != 0:
            raise SpmvHipError(L.spmv_amg_plan_error().decode())

    check(L.spmv_amg_plan_build(rp.size - 1, rp.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p),
                                val.ctypes.data_as(nat.c_double_p), float(theta), int(coarse_rows), int(max_levels),
                                C.byref(plan)))
    try:
        return _amg_levels(lambda *a: check(L.spmv_amg_plan_level(plan, *a)), L.spmv_amg_plan_levels(plan), np.float64,
                           True)
    finally:
        L.spmv_amg_plan_free(plan)


class Preconditioner(_Handle):
    """M^-1 of a Jacobi, block-Jacobi, SSOR, ILU(0), FSAI, AMG or Chebyshev preconditioner of a CsrDevice's rows,
    resident in HBM (CsrDevice.preconditioner).  It owns its arrays: the handle it was built from may be freed first."""

    _free = "spmv_hip_precond_free"

    def __init__(self, dev: CsrDevice, entry_point: str, *args):
        """The build entry point `entry_point` of the library on dev's handle, with the arguments that stand between
        the handle and the result in its prototype (CsrDevice.preconditioner has checked them)."""
        super().__init__()
        _check(getattr(nat.lib(), entry_point)(dev.h, *args, C.byref(self.h)), entry_point)
        info = self.info()
        self.kind, self.block, self.rows, self.row0 = info["kind"], info["block"], info["rows"], info["row0"]
        self.dtype = np.float64 if info["value_bytes"] == 8 else np.float32

    def info(self) -> dict:
        out = (C.c_int * 5)()
        _check(nat.lib().spmv_hip_precond_info(self.h, out), "spmv_hip_precond_info")
        return dict(zip(("kind", "block", "rows", "row0", "value_bytes"), (int(v) for v in out)))

    def refresh(self, dev: CsrDevice):
        """The preconditioner from the values dev holds now (spmv_hip_precond_refresh): dev is a handle of P's dtype,
        rows and row0 with the pattern P was built from, normally the same handle after update_values.  Jacobi and
        block-Jacobi rerun their device build; SSOR, ILU(0) (either ordering) keep their colouring, levels and launch
        plans and redo the numbers on the device.  P then is, byte for byte, the fresh build with the same arguments on a
        fresh upload of dev's arrays.  All or nothing: a refusal (the build's words, with its row) leaves P applying as
        before.  FSAI, AMG and Chebyshev depend on the values beyond their numbers and are refused: build them again."""
        _check(nat.lib().spmv_hip_precond_refresh(self.h, dev.h), "spmv_hip_precond_refresh")

    def apply(self, r):
        """z = M^-1 r for r of `rows` values (element i = row row0 + i) of the handle's dtype."""
        r = np.asarray(r)
        if r.dtype != self.dtype:
            raise ValueError(f"r has dtype {r.dtype}, the preconditioner holds {np.dtype(self.dtype)}")
        if r.ndim != 1 or r.shape[0] != self.rows:
            raise ValueError(f"r must be a vector of {self.rows} values, got shape {r.shape}")
        r = np.ascontiguousarray(r)
        z = np.zeros(self.rows, dtype=self.dtype)
        _check(nat.lib().spmv_hip_precond_apply(self.h, r.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)),
               "spmv_hip_precond_apply")
        return z

    def apply_multi(self, R):
        """Z = M^-1 R for the k columns of a C-contiguous R (rows x k, 1 <= k <= 64) of the handle's dtype
        (spmv_hip_precond_apply_multi); Jacobi, block-Jacobi, FSAI, AMG and Chebyshev."""
        R = _check_columns(R, self.rows, self.dtype, "R", "preconditioner")
        Z = np.zeros(R.shape, dtype=self.dtype)
        _check(nat.lib().spmv_hip_precond_apply_multi(self.h, int(R.shape[1]), R.ctypes.data_as(C.c_void_p),
                                                      Z.ctypes.data_as(C.c_void_p)), "spmv_hip_precond_apply_multi")
        return Z

    def apply_multi_on(self, d_R: int, d_Z: int, k: int, d_work: int = 0, stream: int = 0):
        """The same on row-major rows x k device arrays, asynchronous on `stream` (0 = the library's).  FSAI needs
        d_work, rows x k values and one 128-byte line, AMG its level vectors (work_bytes(k), zeroed once), Chebyshev
        its three arrays (work_bytes(k)); the other kinds ignore it.  Jacobi and block-Jacobi move 16-byte
        pieces when a row of k values is whole pieces and d_R, d_Z are 16-byte aligned, single elements otherwise (the
        same bits)."""
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 64:
            raise ValueError(f"k must be an integer in [1, 64], got {k!r}")
        _check(nat.lib().spmv_hip_precond_apply_multi_on(self.h, int(k), C.c_void_p(d_R), C.c_void_p(d_Z),
                                                         C.c_void_p(d_work), C.c_void_p(stream)),
               "spmv_hip_precond_apply_multi_on")

    def work_bytes(self, k: int) -> int:
        """Bytes of d_work that apply_multi_on needs for k columns (spmv_hip_precond_work_bytes): 0 for Jacobi and
        block-Jacobi; SSOR and ILU(0) have no k-wide apply and are refused."""
        out = C.c_longlong(0)
        _check(nat.lib().spmv_hip_precond_work_bytes(self.h, int(k), C.byref(out)), "spmv_hip_precond_work_bytes")
        return int(out.value)

    def amg_info(self) -> dict:
        """AMG: levels, the first level of the chained tail (-1: none), launches per apply, the coarsest kind (AMG_DIRECT
        or AMG_SMOOTH), operator complexity x 1000, microseconds of download, host setup and upload, chain, and the
        rows and the entries of A_l per level."""
        out = (C.c_int * PRECOND_AMG_INFO_WORDS)()
        _check(nat.lib().spmv_hip_precond_amg_info(self.h, out), "spmv_hip_precond_amg_info")
        info = dict(zip(PRECOND_AMG_INFO, (int(v) for v in out)))
        n, base = info["levels"], len(PRECOND_AMG_INFO)
        info["rows"] = [int(v) for v in out[base:base + n]]
        info["entries"] = [int(v) for v in out[base + AMG_MAX_LEVELS:base + AMG_MAX_LEVELS + n]]
        return info

    def amg_setup_info(self) -> dict:
        """AMG: "setup" (0: the host setup, 1: the device setup) and the microseconds of the device setup's phases over
        all levels: row statistics, strength graph, aggregation (host), A T with the smoothing, transpose, A P,
        R (A P), coarsest inverse (host), rounding to the dtype; zeros for a host-built preconditioner."""
        out = (C.c_int * PRECOND_AMG_SETUP_INFO_WORDS)()
        _check(nat.lib().spmv_hip_precond_amg_setup_info(self.h, out), "spmv_hip_precond_amg_setup_info")
        return dict(zip(PRECOND_AMG_SETUP_INFO, (int(v) for v in out)))

    def levels(self) -> list:
        """AMG: what the device holds, level by level: {"w", "rho", "kind" (AMG_*), "rows", "aggregates", "A", and "P",
        "R" (not on the coarsest level) or "inv" (a DIRECT coarsest level: its dense inverse, row by row)}, every
        operator a (row_ptr, col, val) triple with values of the handle's dtype."""
        fn = nat.lib().spmv_hip_precond_amg_level
        return _amg_levels(lambda *a: _check(fn(self.h, *a), "spmv_hip_precond_amg_level"), self.amg_info()["levels"],
                           self.dtype, False)

    def cheb_info(self) -> dict:
        """Chebyshev: the degree, lmin and lmax as used, the Gershgorin bound of the block (also when lmax was given),
        the products per apply (degree - 1), the plan of the preconditioner's own upload (an index into FSAI_PLANS),
        microseconds of download with the canonical rows and the bound, and of the upload with the vectors."""
        out = (C.c_double * len(PRECOND_CHEB_INFO))()
        _check(nat.lib().spmv_hip_precond_cheb_info(self.h, out), "spmv_hip_precond_cheb_info")
        info = dict(zip(PRECOND_CHEB_INFO, (float(v) for v in out)))
        for key in ("degree", "products", "plan", "download_us", "upload_us"):
            info[key] = int(info[key])
        return info

    def tri_info(self) -> dict:
        """SSOR / ILU(0): levels, launches, widest and median level of the forward and the backward solve, colours
        (0: natural order), entries of L and of U, microseconds of analysis, factorisation and upload."""
        out = (C.c_int * len(PRECOND_TRI_INFO))()
        _check(nat.lib().spmv_hip_precond_tri_info(self.h, out), "spmv_hip_precond_tri_info")
        return dict(zip(PRECOND_TRI_INFO, (int(v) for v in out)))

    def fsai_info(self) -> dict:
        """FSAI: the cap, the entries of G, the rows that lost entries to the cap, the largest pattern, the plans of
        the handles of G and G^T (an index into FSAI_PLANS), microseconds of analysis, device build, and the two
        uploads with the transpose."""
        out = (C.c_int * len(PRECOND_FSAI_INFO))()
        _check(nat.lib().spmv_hip_precond_fsai_info(self.h, out), "spmv_hip_precond_fsai_info")
        return dict(zip(PRECOND_FSAI_INFO, (int(v) for v in out)))

    def factors(self):
        """SSOR / ILU(0): (L, U), each a (row_ptr, col, val) triple in the handle's row numbering with ascending
        columns, both with their diagonal (ILU(0): L's is exactly 1; SSOR: the triangles of A).  With the multicolour
        order they are Q^T L Q and Q^T U Q, triangular after the rows are put in (colour, row) order.  FSAI: (G, G^T),
        M^-1 = G^T G."""
        out = []
        for which in (0, 1):
            rp = np.zeros(self.rows + 1, dtype=np.int32)
            fn = nat.lib().spmv_hip_precond_factors
            _check(fn(self.h, which, rp.ctypes.data_as(nat.c_int_p), None, None), "spmv_hip_precond_factors")
            col = np.zeros(max(int(rp[-1]), 1), dtype=np.int32)
            val = np.zeros(max(int(rp[-1]), 1), dtype=self.dtype)
            _check(fn(self.h, which, rp.ctypes.data_as(nat.c_int_p), col.ctypes.data_as(nat.c_int_p),
                      val.ctypes.data_as(C.c_void_p)), "spmv_hip_precond_factors")
            out.append((rp, col[:rp[-1]], val[:rp[-1]]))
        return tuple(out)

    def apply_on(self, d_r: int, d_z: int, stream: int = 0):
        """z = M^-1 r on device vectors, asynchronous on `stream` (0 = the library's)."""
        _check(nat.lib().spmv_hip_precond_apply_on(self.h, C.c_void_p(d_r), C.c_void_p(d_z), C.c_void_p(stream)),
               "spmv_hip_precond_apply_on")


class HllDevice(_Handle):
    """An HLL matrix resident in HBM as one flat slab."""

    _free = "spmv_hip_hll_free"

    def __init__(self, hll: HllHost = None, hack0=0, hack1=None):
        """The whole matrix, or hacks [hack0, hack1) of it (one rank's share)."""
        super().__init__()
        if hll is not None:
            hack1 = hll.num_blocks if hack1 is None else hack1
            _check(nat.lib().spmv_hip_hll_upload_part(C.byref(hll.c), int(hll.M), int(hll.N), int(hack0),
                                                      int(hack1), C.byref(self.h)), "spmv_hip_hll_upload_part")
            self.M, self.N = hll.M, hll.N

    def time_graph(self, variant=HLL_AUTO, iters=20, replays=10) -> float:
        ms = C.c_float(0)
        _check(nat.lib().spmv_hip_hll_time_graph(self.h, int(variant), int(iters), int(replays), C.byref(ms)),
               "hll_time_graph")
        return float(ms.value)

    def step_time(self, row_bounds, variant=HLL_AUTO, warmup=5, iters=95):
        """Multi-GPU step (SpMV on this rank's hacks + all-gatherv of y): kernel and exchange ms."""
        b = np.ascontiguousarray(row_bounds, dtype=np.int32)
        mk, mx = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
        _check(nat.lib().spmv_hip_hll_step_time(self.h, int(variant), b.ctypes.data_as(nat.c_int_p),
                                                int(warmup), int(iters), mk.ctypes.data_as(nat.c_float_p),
                                                mx.ctypes.data_as(nat.c_float_p)), "hll_step_time")
        return mk, mx

    @classmethod
    def from_csr_device(cls, csr: "CsrDevice"):
        """HLL built on the GPU from a resident CSR matrix (spmv_hip_hll_from_csr)."""
        self = cls()
        _check(nat.lib().spmv_hip_hll_from_csr(csr.h, C.byref(self.h)), "spmv_hip_hll_from_csr")
        self.M, self.N = csr.info()["M_total"], csr.N
        return self

    def run_on(self, d_x: int, d_y: int, variant=HLL_AUTO, stream: int = 0):
        _check(nat.lib().spmv_hip_hll_run_on(self.h, int(variant), C.c_void_p(d_x), C.c_void_p(d_y),
                                             C.c_void_p(stream)), "hll_run_on")

    x_ptr = property(lambda s: nat.lib().spmv_hip_hll_x_ptr(s.h) or 0)
    y_ptr = property(lambda s: nat.lib().spmv_hip_hll_y_ptr(s.h) or 0)

    def tile_digest(self):
        out = (C.c_ulonglong * 64)()
        _check(nat.lib().spmv_hip_hll_tile_digest(self.h, out), "spmv_hip_hll_tile_digest")
        return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(32)]

    def download(self):
        """(hack_off, maxnz, JA, AS) of the flat device slab."""
        info = self.info()
        H = info["hacks"]
        off = np.zeros(H + 1, dtype=np.int64)
        mz = np.zeros(max(H, 1), dtype=np.int32)
        _check(nat.lib().spmv_hip_hll_download(self.h, off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                               mz.ctypes.data_as(nat.c_int_p), None, None), "hll_download")
        S = int(off[H])
        ja, as_ = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.float64)
        _check(nat.lib().spmv_hip_hll_download(self.h, None, None, ja.ctypes.data_as(nat.c_int_p),
                                               as_.ctypes.data_as(nat.c_double_p)), "hll_download")
        return off, mz[:H], ja[:S], as_[:S]

    def info(self) -> dict:
        out = nat.DevInfo()
        _check(nat.lib().spmv_hip_hll_info(self.h, C.byref(out)), "spmv_hip_hll_info")
        return out.as_dict()

    def set_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if len(x) != self.N:
            raise ValueError(f"x has {len(x)} entries, matrix has {self.N} columns")
        _check(nat.lib().spmv_hip_hll_set_x(self.h, x.ctypes.data_as(nat.c_double_p)), "hll_set_x")

    def run(self, variant=HLL_AUTO):
        _check(nat.lib().spmv_hip_hll_run(self.h, int(variant)), "spmv_hip_hll_run")

    def get_y(self):
        y = np.empty(self.M, dtype=np.float64)
        _check(nat.lib().spmv_hip_hll_get_y(self.h, y.ctypes.data_as(nat.c_double_p)), "hll_get_y")
        return y

    def spmv(self, x, variant=HLL_AUTO):
        self.set_x(x)
        self.run(variant)
        return self.get_y()

    def time(self, variant=HLL_AUTO, warmup=5, iters=95, zero_y=True):
        ms = np.zeros(iters, dtype=np.float32)
        _check(nat.lib().spmv_hip_hll_time(self.h, int(variant), int(warmup), int(iters),
                                           int(bool(zero_y)), ms.ctypes.data_as(nat.c_float_p)),
               "hll_time")
        return ms

    def spmm(self, X):
        """Y = A X for the k columns of X (N x k float64, or a vector of N: k = 1) in one pass over the slab
        (spmv_hip_hll_spmm).  Returns an (M_total, k) array; rows outside the handle's are zero."""
        X = np.asarray(X)
        if X.dtype != np.float64:
            raise ValueError(f"X has dtype {X.dtype}, HLL handles hold float64")
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] != self.N or X.shape[1] < 1:
            raise ValueError(f"X must be {self.N} x k with k >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X)
        Y = np.zeros((self.M, X.shape[1]), dtype=np.float64)
        _check(nat.lib().spmv_hip_hll_spmm(self.h, int(X.shape[1]), X.ctypes.data_as(nat.c_double_p),
                                           Y.ctypes.data_as(nat.c_double_p)), "spmv_hip_hll_spmm")
        return Y

    def spmm_on(self, d_X: int, d_Y: int, k: int, stream: int = 0):
        """Y = A X on device buffers (row-major N x k and M_total x k float64, e.g. spmv_hip_malloc or a torch
        tensor's data_ptr()), asynchronous on `stream` (0 = the library's)."""
        _check(nat.lib().spmv_hip_hll_spmm_on(self.h, int(k), C.c_void_p(d_X), C.c_void_p(d_Y), C.c_void_p(stream)),
               "spmv_hip_hll_spmm_on")

    def time_spmm(self, k, warmup=5, iters=95):
        """Per-launch milliseconds of the k-vector product on library-owned X / Y (spmv_hip_hll_spmm_time)."""
        ms = np.zeros(iters, dtype=np.float32)
        _check(nat.lib().spmv_hip_hll_spmm_time(self.h, int(k), int(warmup), int(iters),
                                                ms.ctypes.data_as(nat.c_float_p)), "hll_spmm_time")
        return ms
