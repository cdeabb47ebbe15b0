"""CPU test of what can be read off the compiled gfx950 code of the edit distance's kernel (cat_amd/csrc/k_edit.hip): no instantiation
spills or uses scratch, and only the strip path touches LDS.  The assembly is the cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAME = "crf_ctc_edit_kernel"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_edit_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if NAME in k}
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for e in ("ILi1ELb0EE", "ILi2ELb0EE", "ILi4ELb0EE", "ILi8ELb0EE", "ILi8ELb1EE"):   # rows per lane 1, 2, 4, 8 in registers, and the strips
        assert sum(f"{NAME}{e}" in k for k in mine) == 1, (e, sorted(mine))
    assert len(mine) == 5, sorted(mine)
    # one wave per hypothesis with its rows in registers: two words per cell and the row's token
    for k, v in mine.items():
        assert v["vgpr_count"] <= 64, (k, v)
