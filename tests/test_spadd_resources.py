"""What hipcc makes of the sparse sum's kernels for gfx950 (no GPU needed).  The merge is bandwidth bound and lives on
occupancy: nothing may spill.  The lane-group kernels rank their matches with one ballot and use no LDS at all (0 bytes);
the long rows' workgroup rank keeps one count per wave, 4 x 4 = 16 bytes, which is all the LDS of the translation unit."""
import os

import pytest

from _util import HIPCC, compile_kernels

VGPR_BOUND = 64  # eight waves per SIMD: the searches hide each other's latency


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_spadd_kernels_do_not_spill_and_stay_out_of_lds():
    kernels = compile_kernels("spmv_spadd.hip")
    ours = {k: v for k, v in kernels.items() if "sa_" in k}
    assert not [k for k in kernels if "sg_" in k], "the product's kernels belong to spmv_spgemm.hip alone"
    rows = {k: v for k, v in ours.items() if "sa_merge_rows" in k}
    long_rows = {k: v for k, v in ours.items() if "sa_merge_long" in k}
    assert len(rows) == 4 and len(long_rows) == 4, sorted(kernels)   # {fp64, fp32} x {symbolic, numeric}
    for name in ("sa_check", "sa_long_rows", "sa_identity"):
        assert any(name in k for k in ours), (name, sorted(kernels))
    for name, k in ours.items():
        assert k.scratch == 0, f"{name} spills {k.scratch} bytes of scratch ({k.vgprs} VGPRs)"
        assert k.vgprs <= VGPR_BOUND, f"{name}: {k.vgprs} VGPRs > {VGPR_BOUND}"
    for name, k in rows.items():
        assert k.lds == 0, f"{name}: {k.lds} bytes of LDS"
    for name, k in long_rows.items():
        assert k.lds == 16, f"{name}: {k.lds} bytes of LDS"
    for name, k in ours.items():
        if name not in rows and name not in long_rows:
            assert k.lds == 0, f"{name}: {k.lds} bytes of LDS"
