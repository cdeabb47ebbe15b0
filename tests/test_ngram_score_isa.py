"""CPU test of what can be read off the compiled gfx950 code of ngram_score (cat_amd/csrc/k_ngram.hip): neither instantiation spills or
uses scratch, and their names stay apart from the fused search's.  The assembly is the cached one of tests/test_isa_checks.py, the
helpers those of tests/test_beam_isa.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAME = "crf_ngram_score_kernel"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_ngram_score_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    mine = {k: v for k, v in meta.items() if NAME in k}
    assert len(mine) == 2, sorted(mine)                             # <scores> and <tokens>
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 64, (k, v)                        # eight waves per SIMD: the look-ups' load chains overlap
    # the search's kernels keep their names apart from these (tests/test_beam_lm_isa.py and tests/test_beam_isa.py count substrings)
    for other in ("crf_beamlm_search_kernel", "crf_beam_search_kernel", "crf_beam_row_kernel"):
        assert other not in NAME and NAME not in other
    assert len({k: v for k, v in meta.items() if "crf_beamlm_search_kernel" in k}) == 1
