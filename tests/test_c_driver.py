"""The C driver (csrc/driver/spmv_bench.c): a plain-C host over the C-ABI, reference protocol."""
import csv
import os
import subprocess

import pytest

from conftest import GOLDEN, GOLDEN_CASES, ROOT

DRIVER = os.path.join(ROOT, "sparsematrixvectormultiplication_amd", "spmv_bench")
ORACLE = os.path.join(ROOT, "oracle", "liboracle_spmv.so")


@pytest.mark.gpu
def test_c_driver_runs_reference_protocol_on_golden_matrices(tmp_path, gpu):
    out = tmp_path / "result"
    proc = subprocess.run([DRIVER, "--oracle", ORACLE, "--out", str(out), "--iters", "10", GOLDEN],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = list(csv.DictReader(open(out / "spmv_results_hip.csv")))
    assert sorted(r["matrix_name"] for r in rows) == sorted(n + ".mtx" for n in GOLDEN_CASES)
    # the reference's GPU CSV schema (cuda_src/utility.cu:115-123), unchanged
    assert list(rows[0])[:8] == ["matrix_name", "rows", "cols", "nonzeros", "time_serial",
                                 "time_serial_hll", "time_row_csr", "time_warp_csr"]
    for r in rows:
        for key in ("relative_error_row_csr", "relative_error_warp_csr", "relative_error_warp_shared_csr",
                    "relative_error_row_hll", "relative_error_warp_hll", "relative_error_warp_shared_hll"):
            assert float(r[key]) < 1e-10, (r["matrix_name"], key, r[key])
        if int(r["nonzeros"]) > 0:
            assert float(r["time_warp_csr"]) > 0 and float(r["flops_warp_csr"]) > 0
    roof = list(csv.DictReader(open(out / "spmv_results_hip_roofline.csv")))
    assert len(roof) == len(rows) and all(float(r["rel_err_stream_csr"]) < 1e-10 for r in roof)
    # launch shapes: the reference's block-size schema (cuda_src/utility.cu:236-261, written at
    # main_cuda.cu:728) plus what really varies here (lanes per row, stage, workgroups, kernel)
    dims = list(csv.DictReader(open(out / "spmv_results_hip_block_dim.csv")))
    assert len(dims) == len(rows)
    assert list(dims[0]) == ["matrix_name", "nonzeros", "block_size_csr_row", "block_size_csr_warp",
                             "block_size_csr_shared", "block_size_hll_row", "block_size_hll_warp",
                             "block_size_hll_shared"]
    assert all(int(d["block_size_csr_warp"]) % 64 == 0 for d in dims)
    shapes = list(csv.DictReader(open(out / "spmv_results_hip_launch_shape.csv")))
    assert len(shapes) == len(rows)
    assert all(sh["csr_stream_kernel"] in ("csr_stream", "csr_stream_local", "csr_stream_short", "csr_tile") for sh in shapes)
    # running again appends, never wipes (the reference deletes the result directory)
    subprocess.run([DRIVER, "--out", str(out), "--iters", "6", os.path.join(GOLDEN, "general_matrix.mtx")],
                   check=True, capture_output=True, timeout=120)
    assert len(list(csv.DictReader(open(out / "spmv_results_hip.csv")))) == len(rows) + 1
    # --hll-on-device: HLL built by the GPU from the resident CSR, same checks
    out2 = tmp_path / "result_dev"
    proc = subprocess.run([DRIVER, "--oracle", ORACLE, "--out", str(out2), "--iters", "6", "--hll-on-device",
                           GOLDEN], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    for r in csv.DictReader(open(out2 / "spmv_results_hip.csv")):
        for key in ("relative_error_row_hll", "relative_error_warp_hll", "relative_error_warp_shared_hll"):
            assert float(r[key]) < 1e-10, (r["matrix_name"], key, r[key])
    # --csr-on-device --hll-on-device: nothing but the parser runs on the host; the reference value for the
    # error columns is then the thread-per-row GPU kernel (no oracle in this mode), so compare the streams
    out3 = tmp_path / "result_dev2"
    proc = subprocess.run([DRIVER, "--out", str(out3), "--iters", "6", "--hll-on-device", "--csr-on-device", GOLDEN],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    roof3 = list(csv.DictReader(open(out3 / "spmv_results_hip_roofline.csv")))
    assert len(roof3) == len(rows) and all(float(r["rel_err_stream_csr"]) < 1e-10 for r in roof3)


def test_c_driver_fails_loudly_without_a_gpu(tmp_path):
    import sparsematrixvectormultiplication_amd as sp
    if sp.device_count() > 0:
        pytest.skip("a HIP device is present")
    proc = subprocess.run([DRIVER, "--out", str(tmp_path / "r"), GOLDEN], capture_output=True, text=True)
    assert proc.returncode == 1 and "no usable HIP device" in proc.stderr


@pytest.mark.gpu
def test_bench_row_partitioned_two_ranks_sharing_the_gpu(gpu):
    """The N > 1 host path of bench.py on real kernels: two ranks (both on this box's one
    GPU -- RCCL refuses that, so the exchange goes through host memory with gloo), each
    uploads only its nnz-balanced row block, and every rank checks the gathered y against
    the oracle.  Everything except the RCCL transport itself is what the 8-GPU run executes."""
    import json
    import socket
    import sys
    # the driver's own command shape: no outer launcher, bench.py starts its ranks as child processes
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
           "--grid", "24,24,24", "--exchange", "gloo-host", "--check", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), proc.stdout[-2000:]   # ONE JSON line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["rows_per_rank"][0] > 0
    assert sum(out["config"]["rows_per_rank"]) == out["config"]["rows"]
    assert proc.stderr.count("check: max|y - y_ref|") == 2
    # the same through an outer torch.distributed.run, as the task statement's launcher does
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "1", "--grid", "24,24,24", "--exchange", "gloo-host",
           "--check", "--no-cpu-baseline"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    assert out["config"]["parallelism"] == "row-block x2"
    assert proc.stderr.count("check: max|y - y_ref|") == 2
    # the HLL workload on two ranks: hack-aligned shares (reference's hack partitioner)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "1", "--workload", "cant_hll", "--grid", "5,5,40",
           "--exchange", "gloo-host", "--check", "--no-cpu-baseline"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and "HLL" in out["config"]["workload"] and out["value"] > 0
    assert proc.stderr.count("check: max|y - y_ref|") == 2


@pytest.mark.gpu
def test_bench_powerlaw_two_ranks_checked_against_the_oracle(gpu):
    """BASELINE configs[4]'s workload (power-law rows, fp32) through the N > 1 host path at a size the oracle
    finishes in seconds: nnz-balanced split of very unequal rows, fp32 exchange, every rank checks the gathered
    y against K1's loop with a double accumulator (fp32 has no reference counterpart: norm-wise 1e-5)."""
    import json
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--workload", "powerlaw", "--powerlaw-n", "262144", "--exchange", "gloo-host", "--check",
           "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["dtype"] == "f32" and out["value"] > 0
    assert sum(out["config"]["rows_per_rank"]) == 262144
    assert out["config"]["nnz_imbalance_max_over_mean"] < 1.2
    assert proc.stderr.count("check: max|y - y_ref|") == 2


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_and_full_adds_the_rest(gpu):
    """A plain run prints the headline with no box record, CPU baseline, parity gate or side measurements; --full
    adds the box record and the CPU baseline with its parity gate (`also` belongs to the default workload only)."""
    import json
    import sys
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--workload", "cant", "--grid", "5,5,40", "--settle-ms", "0"]
    outs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-sweep", "--cpu-iters", "5"])):
        proc = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert proc.returncode == 0, proc.stderr[-3000:]
        outs[mode] = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = outs["plain"], outs["full"]
    for out in (plain, full):
        assert out["value"] > 0 and out["unit"] == "GFLOP/s" and out["dtype"] == "f64" and out["ms_per_step"] > 0
        assert out["steps"] == 3 and out["warmup"] == 1 and out["roofline"]["kernel_ms_mean"] > 0
    assert not {"box", "cpu_baseline", "parity_vs_cpu_reference", "also"} & set(plain)
    assert "box" in full and full["cpu_baseline"]["value"] > 0 and "thread_sweep" not in full["cpu_baseline"]
    assert full["parity_vs_cpu_reference"]["parity_ok"]


@pytest.mark.gpu
def test_bench_dumps_what_the_last_timed_step_computed(tmp_path, gpu, oracle):
    """--dump-outputs DIR: after the --steps timed steps, the y of the last one lands in DIR/y.npy in the workload's
    dtype and equals the oracle's; the result line reports the steps asked for and the time of one of them."""
    import json
    import sys

    import numpy as np
    from _util import assert_parity
    from sparsematrixvectormultiplication_amd import synth
    grid = (24, 24, 24)
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--grid", ",".join(map(str, grid)), "--settle-ms", "0", "--no-cpu-baseline", "--no-also", "--no-box-state",
           "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert sorted(os.listdir(out_dir)) == ["y.npy"]
    y = np.load(out_dir / "y.npy")
    _, rp, col, val = synth.kkt_like(grid, 2)
    x = np.ones(len(rp) - 1)
    assert y.dtype == np.float64 and y.shape == x.shape
    assert_parity(y, oracle.csr_serial(rp, col, val, x), rp, col, val, x, what="bench --dump-outputs")


@pytest.mark.gpu
def test_bench_job_ends_nonzero_when_one_rank_fails(gpu):
    """An unattended multi-rank run must not hang on a dead rank: rank 1 raises before the timed region while
    rank 0 goes on into its first collective; the job has to end with a non-zero code well inside a minute."""
    import sys
    import time
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--grid", "24,24,24", "--exchange", "gloo-host", "--no-cpu-baseline", "--fail-rank", "1",
           "--dist-timeout", "30"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    t = time.time()
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    took = time.time() - t
    assert proc.returncode != 0, proc.stdout[-1000:]
    assert "--fail-rank" in proc.stderr
    assert not [ln for ln in proc.stdout.splitlines() if ln.startswith("{")], "a failed job printed a result line"
    assert took < 60, f"the job took {took:.0f} s to notice the dead rank"


@pytest.mark.gpu
def test_native_communicator_under_torch_first_load_order(gpu):
    """bench.py imports torch before libspmv_amd.so, so the C-ABI's RCCL calls bind to the
    librccl that torch ships, not /opt/rocm's.  Same single-rank exchange in that load order."""
    import sys
    code = r'''
import numpy as np, torch
import sparsematrixvectormultiplication_amd as sp
from sparsematrixvectormultiplication_amd.distributed import NativeComm
assert torch.cuda.is_available()
torch.cuda.set_device(0)
sp.hip_init(0)
comm = NativeComm(0, 1, lambda ident: ident)
rp = np.arange(0, 3 * 600 + 1, 3, dtype=np.int32)
col = (np.arange(1800) * 7 % 600).astype(np.int32)
col = np.sort(col.reshape(600, 3), axis=1).ravel().astype(np.int32)
val = np.linspace(-1, 1, 1800)
with sp.CsrDevice(600, 600, rp, col, val) as dev:
    dev.set_x(np.ones(600))
    mk, mx = dev.step_time(np.array([0, 600], np.int32), sp.CSR_AUTO, 1, 3)
    y = dev.get_y()
    assert np.allclose(y, val.reshape(600, 3).sum(axis=1)) and mk.shape == (3,)
comm.close()
t = torch.ones(4, device="cuda") * 2
assert float(t.sum()) == 8.0      # torch's own runtime still works next to the library
print("ok")
'''
    proc = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert proc.returncode == 0 and "ok" in proc.stdout, proc.stderr[-3000:]


@pytest.mark.gpu
def test_randomised_parity_sweep(gpu):
    """tests/fuzz_parity.py: 150 random small matrices (banded / scattered / mixed, empty and long
    rows, unsorted and repeated columns, fp64 / fp32, row blocks) through the fast path of both
    formats against the oracle."""
    import sys
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_parity.py"), "150", "11"],
                          capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stdout[-1500:] + proc.stderr[-3000:]
    assert "all 150 cases passed" in proc.stdout


@pytest.mark.gpu
def test_tuning_through_the_environment(gpu):
    """SPMV_TUNING="key=value,..." is read by spmv_hip_init: forcing the gather kernel through the environment
    changes which kernel runs (same result), an unknown key makes init fail loudly."""
    import sys
    code = r'''
import numpy as np, sys
import sparsematrixvectormultiplication_amd as sp
sys.path.insert(0, "tests")
from _util import banded_csr
sp.hip_init(0)
rng = np.random.default_rng(1)
rp, col, val = banded_csr(rng, 3000, 3000, 20, 100)
with sp.CsrDevice(3000, 3000, rp, col, val) as d:
    print("BLOCKS", d.info()["local_blocks"], "SUM", repr(float(np.sum(d.spmv(np.ones(3000))))))
'''
    outs = {}
    for tag, env in (("default", {}), ("no_plan", {"SPMV_TUNING": "stream_local=0,stream_cap=4096"})):
        proc = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                              env={**os.environ, **env})
        assert proc.returncode == 0, proc.stderr[-2000:]
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("BLOCKS")][-1].split()
        outs[tag] = (int(line[1]), float(line[3]))
    assert outs["default"][0] > 0 and outs["no_plan"][0] == 0
    assert abs(outs["default"][1] - outs["no_plan"][1]) <= 1e-9 * max(1.0, abs(outs["default"][1]))
    proc = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                          env={**os.environ, "SPMV_TUNING": "no_such_knob=1"})
    assert proc.returncode != 0 and "unknown key" in (proc.stderr + proc.stdout)
