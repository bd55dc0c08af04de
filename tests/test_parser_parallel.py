"""the OpenMP tokenising parser must give exactly what the serial reader
(and the reference's fscanf loop) gives, for any thread count and odd layouts."""
import os
import time

import numpy as np
import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import PARSER_CASES, digest, parser_case_key, reference_digests, write_parser_case
from _util import write_free_form_mtx as _write


def _load(path, threads=None):
    old = os.environ.pop("SPMV_PARSE_THREADS", None)
    if threads is not None:
        os.environ["SPMV_PARSE_THREADS"] = str(threads)
    try:
        t = time.perf_counter()
        pre = sp.read_matrix_market(path)
        dt = time.perf_counter() - t
        return (pre.M, pre.N, pre.nz, np.array(pre.I), np.array(pre.J), np.array(pre.val)), dt
    finally:
        os.environ.pop("SPMV_PARSE_THREADS", None)
        if old is not None:
            os.environ["SPMV_PARSE_THREADS"] = old


@pytest.mark.parametrize("field,symmetry,ragged", PARSER_CASES)
def test_parallel_parser_equals_serial_and_reference(tmp_path, field, symmetry, ragged):
    path = tmp_path / "big.mtx"
    write_parser_case(path, field, symmetry, ragged)
    assert os.path.getsize(path) > (1 << 20)          # large enough for the parallel path
    par, t_par = _load(path)
    ser, t_ser = _load(path, threads=1)
    assert par[:3] == ser[:3]
    for a, b in zip(par[3:], ser[3:]):
        assert a.tobytes() == b.tobytes()
    # what the reference's own reader made of the same file (tests/golden/reference_digests.json)
    ref = reference_digests("parser")[parser_case_key(field, symmetry, ragged)]
    assert (ref["M"], ref["N"], ref["nz"]) == par[:3]
    assert (digest(par[3]), digest(par[4]), digest(par[5])) == (ref["I"], ref["J"], ref["val"])


def test_parallel_parser_reports_errors(tmp_path):
    rng = np.random.default_rng(3)
    M = N = 40000
    nnz = 120000
    rows, cols, vals = rng.integers(0, M, nnz), rng.integers(0, N, nnz), rng.uniform(-1, 1, nnz)
    path = tmp_path / "short.mtx"
    _write(path, M, N, rows, cols, vals, "real", "general")
    text = open(path).read().splitlines(keepends=True)
    open(path, "w").write("".join(text[:-5]))                         # fewer entries than announced
    with pytest.raises(ValueError):
        sp.read_matrix_market(path)
    bad = text[:]
    bad[60000] = f"{M + 7} 1 0.5\n"                                   # row index out of range
    open(path, "w").write("".join(bad))
    with pytest.raises(ValueError):
        sp.read_matrix_market(path)
    bad = text[:]
    bad[70000] = "12 x7 0.5\n"                                        # not a number
    open(path, "w").write("".join(bad))
    with pytest.raises(ValueError):
        sp.read_matrix_market(path)


@pytest.mark.parametrize("env", [{"OMP_NUM_THREADS": "8", "OMP_THREAD_LIMIT": "2"},
                                 {"OMP_NUM_THREADS": "64", "OMP_DYNAMIC": "true"},
                                 {"OMP_NUM_THREADS": "1"}])
@pytest.mark.parametrize("name", ["sym_empty_rows", "sym_pattern"])
def test_symmetric_expansion_when_the_runtime_delivers_fewer_threads(name, env):
    """The symmetric mirror pass sizes its per-thread table with omp_get_max_threads() but the team
    may be smaller (OMP_THREAD_LIMIT, OMP_DYNAMIC, nested regions): nz and the triplets must equal
    the golden ones produced by the compiled reference whatever team the runtime hands out."""
    import subprocess
    import sys

    from conftest import ROOT, golden_path, load_golden
    code = ("import numpy as np, sparsematrixvectormultiplication_amd as sp\n"
            f"pre = sp.read_matrix_market({golden_path(name)!r})\n"
            "csr = sp.convert_in_csr(pre)\n"
            "np.savez(__import__('sys').argv[1], nz=pre.nz, row_ptr=np.array(csr.row_ptr), "
            "col=np.array(csr.col_idx), val=np.array(csr.values))\n")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "o.npz")
        proc = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, cwd=ROOT,
                              env={**os.environ, **env}, timeout=120)
        assert proc.returncode == 0, proc.stderr[-2000:]
        got = np.load(out)
        g = load_golden(name)
        assert int(got["nz"]) == int(g["row_ptr"][-1]) > 0
        assert np.array_equal(got["row_ptr"], g["row_ptr"])
        assert np.array_equal(got["col"], g["col_idx"])
        assert np.array_equal(got["val"], g["values"])
