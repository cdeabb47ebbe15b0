"""CPU test of what can be read off the compiled gfx950 code of the raw-output score gradient's kernels (cat_amd/csrc/k_score_grad.hip):
every instantiation -- the alpha and beta passes for 1, 2, 4 and 8 states per lane on fp32, bf16 and fp16 elements, and the reduce stage
on each element type -- exists and neither spills nor uses scratch.  The assembly is the cached one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.score_grad_logits_ref import core  # noqa: F401  (the feature's symbols: nothing to look for without them)
from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

ELEMS = ("f", "NS_7AlnBf16E", "NS_6AlnF16E")                              # float, crf::AlnBf16, crf::AlnF16 as the mangled names spell them
RECURSIONS = ("crf_ctc_score_grad_alpha_raw_kernel", "crf_ctc_score_grad_beta_raw_kernel")
REDUCE = "crf_ctc_score_grad_reduce_raw_kernel"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_raw_score_grad_kernels_exist_and_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    want = [f"{len(name)}{name}ILi{nr}E{e}EE" for name in RECURSIONS for nr in (1, 2, 4, 8) for e in ELEMS] + \
           [f"{len(REDUCE)}{REDUCE}I{e}EE" for e in ELEMS]
    assert len(want) == 27
    for w in want:
        hits = [k for k in meta if w in k]
        assert len(hits) == 1, (w, sorted(k for k in meta if "score_grad" in k))
        v = meta[hits[0]]
        assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (hits[0], v)
    assert len([k for k in meta if "score_grad" in k and "_raw_kernel" in k]) == 27
