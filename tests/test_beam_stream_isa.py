"""CPU test of what can be read off the compiled gfx950 code of the streaming beam search's kernels (cat_amd/csrc/k_beam_chunk.hip):
neither spills nor uses scratch, at no more than 128 vector registers, and their names hold none of the names that the tests of the
whole-utterance kernels count.  The assembly is the cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

NAMES = ("crf_beam_chunk_kernel", "crf_beamlm_chunk_kernel")
OLD = ("crf_beam_search_kernel", "crf_beam_row_kernel", "crf_beamlm_search_kernel")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_chunk_kernels_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    for name in NAMES:
        mine = {k: v for k, v in meta.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        (k, v), = mine.items()
        assert not any(o in k for o in OLD), k
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)
