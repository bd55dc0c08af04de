"""What hipcc makes of the reordering kernels for gfx950 (no GPU needed).  The row copy and the expansions are
bandwidth and latency bound and live on occupancy: nothing may spill, and none of them uses LDS.  The ordering chain keeps
what its cap promises in LDS: 8 bytes per node at the largest cap (4096 64-bit keys) and two counters; the search chain
keeps its lists in global memory and only the counters in LDS; rcm_next_start keeps one word."""
import os
import re

import pytest

import sparsematrixvectormultiplication_amd as sp
from _util import HIPCC, compile_kernels

VGPR_BOUND = 64  # eight waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_reorder_kernels_do_not_spill_and_the_chain_keeps_its_lds_promise():
    kernels = compile_kernels("spmv_reorder.hip")
    ours = {k: v for k, v in kernels.items() if re.search(r"4spmv\d+(ro|rcm)_", k)}   # (rocPRIM's sort kernels are there too)
    names = ("ro_first_position", "ro_repeats", "ro_row_lengths", "ro_copy_rows", "rcm_degrees", "rcm_ranks", "rcm_isolated",
             "rcm_next_start", "rcm_seed", "rcm_expand", "rcm_keys", "rcm_place", "rcm_min_rank", "rcm_chain",
             "rcm_bandwidth")
    for name in names:
        assert any(name in k for k in ours), (name, sorted(kernels))
    for name, count in (("ro_copy_rows", 2), ("rcm_expand", 2), ("rcm_chain", 2), ("rcm_seed", 2)):
        assert len([k for k in ours if name in k]) == count, (name, sorted(ours))   # {fp64, fp32} or {order, search}
    assert len(ours) == len(names) + 4, sorted(ours)
    for name, k in ours.items():
        assert k.scratch == 0, f"{name} spills {k.scratch} bytes of scratch ({k.vgprs} VGPRs)"
        assert k.vgprs <= VGPR_BOUND, f"{name}: {k.vgprs} VGPRs > {VGPR_BOUND}"
    largest = sp.rcm_chain_nodes()[1]
    for name, k in ours.items():
        if "rcm_chainILb1" in name:
            assert k.lds == 8 * largest + 8, f"{name}: {k.lds} bytes of LDS for a cap of {largest} nodes"
            assert k.lds <= 64 * 1024
        elif "rcm_chain" in name:
            assert k.lds == 8, f"{name}: {k.lds} bytes of LDS"
        elif "rcm_next_start" in name:
            assert k.lds == 4, f"{name}: {k.lds} bytes of LDS"
        else:
            assert k.lds == 0, f"{name}: {k.lds} bytes of LDS"
