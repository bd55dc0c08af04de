"""What hipcc makes of the sparse product's kernels for gfx950 (no GPU needed): the on-chip tier sorts in LDS with 256
threads and must not spill -- scratch traffic inside the bitonic network would cost more than the tier saves -- and its
static LDS must leave room for two workgroups per CU beside the 64 KiB of keys and values of the largest block."""
import os

import pytest

from _util import HIPCC, compile_kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_spgemm_kernels_do_not_spill():
    kernels = compile_kernels("spmv_spgemm.hip")
    ours = {k: v for k, v in kernels.items() if "sg_" in k}
    block = {k: v for k, v in ours.items() if "sg_block" in k}
    assert len(block) == 4, sorted(kernels)                      # {fp64, fp32} x {symbolic, numeric}
    for name in ("sg_count", "sg_expand", "sg_row_heads", "sg_row_compress"):
        assert any(name in k for k in ours), (name, sorted(kernels))
    for name, k in ours.items():
        assert k.scratch == 0, f"{name} spills {k.scratch} bytes of scratch ({k.vgprs} VGPRs)"
    for name, k in block.items():
        # 160 KiB per CU: two workgroups of 64 KiB dynamic LDS each leave 16 KiB of static LDS for each
        assert k.lds <= 16 * 1024, f"{name}: {k.lds} bytes of static LDS"
        assert k.vgprs <= 128, f"{name}: {k.vgprs} VGPRs"
