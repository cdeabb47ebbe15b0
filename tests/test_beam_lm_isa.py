"""CPU test of what can be read off the compiled gfx950 code of the fused beam search (cat_amd/csrc/k_beam_lm.hip): it neither spills
nor uses scratch.  The assembly is the cached one of
tests/test_isa_checks.py, the helpers those of tests/test_beam_isa.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAME = "crf_beamlm_search_kernel"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_beam_lm_kernel_neither_spills_nor_uses_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if NAME in k}
    assert len(mine) == 1, sorted(mine)
    (v,) = mine.values()
    assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 128, v
    # the LM-free kernels keep their names apart from this one (tests/test_beam_isa.py counts substrings)
    assert not any(n in NAME for n in ("crf_beam_search_kernel", "crf_beam_row_kernel"))
