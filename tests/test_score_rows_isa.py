"""CPU test of what can be read off the compiled gfx950 code of the device-rows kernels (cat_amd/csrc/k_rows.hip): the plan and merge
kernels and every instantiation of the gradient's row-strided alpha and beta stages neither spill nor use scratch.  The assembly is the
cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

STAGES = ("crf_rows_grad_alpha_kernel", "crf_rows_grad_beta_kernel", "crf_rows_grad_alpha_raw_kernel",
          "crf_rows_grad_beta_raw_kernel")
NAMES = ("crf_rows_plan_kernel", "crf_rows_merge_kernel") + STAGES


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_rows_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if any(n in k for n in NAMES)}
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for name in NAMES[:2]:
        assert any(name in k for k in mine), (name, sorted(mine))
    for name in STAGES:
        for nr in (1, 2, 4, 8):
            assert any(f"{name}ILi{nr}E" in k for k in mine), (name, nr, sorted(mine))
    assert sum("_raw_kernel" in k for k in mine) == 2 * 4 * 3     # both stages, four NR, f32 / bf16 / f16
