"""CPU test of what can be read off the compiled gfx950 code of the score gradient's kernels (cat_amd/csrc/k_score_grad.hip): no
instantiation spills or uses scratch.  The assembly is the cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAMES = ("crf_ctc_score_grad_alpha_kernel", "crf_ctc_score_grad_beta_kernel", "crf_ctc_score_grad_reduce_kernel")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_score_grad_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if any(n in k for n in NAMES)}
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for name in NAMES[:2]:
        for nr in (1, 2, 4, 8):
            assert any(f"{name}ILi{nr}EE" in k for k in mine), (name, nr, sorted(mine))
    assert any(NAMES[2] in k for k in mine)
