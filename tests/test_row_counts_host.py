"""counts_to_row_ptr (csrc/hip/row_counts.hpp), the step from the per-row counts of a symbolic pass to the row_ptr of the
new handle, which the product and the sum share.  Its refusal -- a C of more than 0x7fffffff - kPad entries -- cannot be
reached through the public entry points without 2^31 entries on a device, but the function is host code in a header that
includes no HIP header: tests/row_counts_check.cpp calls it on its own, compiled by the host C++ compiler with
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded).

The cases (kPad is the header's): no rows; one empty row; counts {3, 0, 5}; three rows of 2^30 entries, refused at row 1;
a sum of exactly 0x7fffffff - kPad, accepted; one entry more, refused at the last row."""
import os
import shutil
import subprocess

import pytest

_TESTS = os.path.dirname(os.path.abspath(__file__))
_HIP_SRC = os.path.join(os.path.dirname(_TESTS), "sparsematrixvectormultiplication_amd", "csrc", "hip")


def test_counts_to_row_ptr_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "row_counts_check")
    # the sanitizers' runtimes inside the program where the compiler can do that: no order of shared libraries to get right
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", *runtime, "-I" + _HIP_SRC,
                                os.path.join(_TESTS, "row_counts_check.cpp"), "-o", exe],
                               capture_output=True, text=True, timeout=120)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
