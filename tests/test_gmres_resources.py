"""What hipcc makes of spmv_gmres.hip for gfx950 (no GPU needed): the two Gram-Schmidt passes hold eight basis pieces
and eight fp64 sums per lane in registers, and nothing in the file may spill to scratch."""
import os

import pytest

from _util import HIPCC, compile_kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gmres_kernels_do_not_spill():
    kernels = compile_kernels("spmv_gmres.hip")
    for name in ("gmres_dots", "gmres_update"):
        both = sorted(k for k in kernels if name in k)
        assert len(both) == 2, (name, sorted(kernels))            # fp64 and fp32
        assert any("IdL" in k for k in both) and any("IfL" in k for k in both), both
    for name in ("gm_residual", "gm_scale", "gm_add", "gm_start", "gm_cycle", "gm_rotate", "gm_solve", "solver_fold"):
        assert any(name in k for k in kernels), (name, sorted(kernels))
    for name, k in kernels.items():
        print(f"{name}: {k.vgprs} VGPRs, {k.lds} bytes of LDS, {k.scratch} bytes of scratch")
        assert k.scratch == 0, f"{name} spills {k.scratch} bytes of scratch ({k.vgprs} VGPRs)"
        # block_partials' wave sums (4 waves x 8 doubles) and nothing else
        assert k.lds <= 4 * 8 * 8, f"{name}: {k.lds} bytes of static LDS"
