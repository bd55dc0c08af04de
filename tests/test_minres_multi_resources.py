"""What hipcc makes of spmv_minres_multi.hip for gfx950: every kernel of spmv_hip_csr_minres_multi exists in fp64 and
fp32 and in both lane shapes, none spills, and none holds more LDS than mcg_block_partials' table.  Prints the VGPR
counts (`pytest -s`); the README section records them."""
import os
import re

import pytest

from _util import HIPCC, compile_kernels

K_BLOCK, K_MCG_MAX_K = 256, 64       # spmv_internal.hpp, cg_multi_kernels.hpp
PARTIALS_TABLE = (K_BLOCK // 64) * K_MCG_MAX_K * 8   # __shared__ double wave_sum[kBlock / 64][kMcgMaxK]
VGPR_BOUND = 64    # the bound the solver kernels sit under (test_precond_host.py): eight waves a SIMD
# mmr_update with four fp32 columns a lane holds four fp64 coefficients a column (32 registers) beside its four arrays
# and the temporaries of four fp64 divisions; forced under 64 it spills.  96 registers still leave five waves a SIMD,
# and profiles/minres_multi_step.md holds the measured rate of that pass against the fp64 one, which fits 64.
VGPR_BOUND_UPDATE_F4 = 96

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def kernels():
    return compile_kernels("spmv_minres_multi.hip")


def test_every_kernel_is_there_in_fp64_and_fp32(kernels):
    # every vector kernel in its four lane shapes: fp64 pieces of 2, fp32 pieces of 4, single elements of both
    shapes = r"I(dLi2|fLi4|dLi1|fLi1)E"
    for pattern, count in ((rf"mmr_lanczos_a{shapes}E", 4), (rf"mmr_lanczos_b{shapes}Li[012]EE", 12),
                           (rf"mmr_update{shapes}E", 4), (rf"mcg_dot_partial{shapes}E", 4)):
        found = [k for k in kernels if re.search(pattern, k)]
        assert len(found) == count, (pattern, sorted(kernels))
    for name in ("mmr_start", "mmr_set_alfa", "mmr_rotate", "solver_fold", "solver_rank_sum"):
        assert any(re.search(rf"\d{name}E", k) for k in kernels), (name, sorted(kernels))


def test_no_kernel_spills_and_none_holds_more_lds_than_the_partials_table(kernels):
    for name, v in sorted(kernels.items()):
        print(f"{v.vgprs:4d} VGPRs {v.lds:5d} B LDS {v.scratch:3d} B scratch  {name}")
    for name, v in kernels.items():
        assert v.scratch == 0, f"{name} spills {v.scratch} bytes of scratch ({v.vgprs} VGPRs)"
        assert v.lds <= PARTIALS_TABLE, f"{name}: {v.lds} bytes of LDS > {PARTIALS_TABLE}"
        bound = VGPR_BOUND_UPDATE_F4 if re.search(r"mmr_updateIfLi4E", name) else VGPR_BOUND
        assert v.vgprs <= bound, f"{name}: {v.vgprs} VGPRs > {bound}"
