"""What hipcc makes of the value update's kernels for gfx950 (no GPU needed).  upd_gather is a pure stream -- a 16-byte
load of the source map, four value loads, 16-byte stores per lane -- and lives on occupancy like every copy: nothing may
spill, and it has no use for LDS."""
import os

import pytest

from _util import HIPCC, compile_kernels

VGPR_BOUND = 64  # eight waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_update_kernels_do_not_spill_and_stay_out_of_lds():
    kernels = compile_kernels("spmv_update.hip")
    gathers = {k: v for k, v in kernels.items() if "upd_gather" in k}
    assert len(gathers) == 2, sorted(kernels)   # fp64 and fp32
    assert len(kernels) == len(gathers), f"kernels that belong to other translation units: {sorted(set(kernels) - set(gathers))}"
    for name, k in kernels.items():
        assert k.scratch == 0, f"{name} spills {k.scratch} bytes of scratch ({k.vgprs} VGPRs)"
        assert k.lds == 0, f"{name}: {k.lds} bytes of LDS"
        assert k.vgprs <= VGPR_BOUND, f"{name}: {k.vgprs} VGPRs > {VGPR_BOUND}"
