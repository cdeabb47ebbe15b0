"""CPU test of what can be read off the compiled gfx950 code of the beam search's kernels (cat_amd/csrc/k_beam.hip): no instantiation
spills or uses scratch.  The assembly is the cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAMES = ("crf_beam_row_kernel", "crf_beam_search_kernel")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_beam_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if any(n in k for n in NAMES)}
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for e in ("IfEE", "INS_7AlnBf16EEE", "INS_6AlnF16EEE"):      # the row stage on fp32, bf16 and fp16 rows
        assert any(f"{NAMES[0]}{e}" in k for k in mine), (e, sorted(mine))
    assert sum(NAMES[1] in k for k in mine) == 1, sorted(mine)
    # the beam stage is one wave with its slots in registers
    (search,) = [v for k, v in mine.items() if NAMES[1] in k]
    assert search["vgpr_count"] <= 128, search
