"""CPU test of what can be read off the compiled gfx950 code of the CTC-Transducer loss (cat_amd/csrc/k_ctct.hip): every kernel of the
family is there, none spills or uses scratch, and each stays under the register ceiling its geometry relies on.  The assembly is the cached
one of tests/test_isa_checks.py."""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

# kernel -> (instantiations, VGPR ceiling).  The build has 13 (gather), 13 - 16 (row), 54 (lattice), 20 - 34 (grad).
#   gather, row, grad: a wave (a thread) per node with nothing but the row's loads to wait for -- 64 registers keep eight waves per SIMD
#     in flight, which is what hides the memory latency of the passes over the joiner output;
#   lattice: the workgroup form runs up to 1 024 threads, four waves per SIMD, and needs <= 128 to be launched at all; 64 lets two
#     utterances' workgroups share a compute unit.  Two staging batches of kCtctPF = 4 records of four floats are 32 of them, the two
#     running values and what a frame derives from them in fp64 the rest.
KERNELS = {"crf_ctct_gather_kernel": (1, 64), "crf_ctct_row_kernel": (3, 64), "crf_ctct_lattice_kernel": (2, 64), "crf_ctct_grad_kernel": (4, 64)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_ctct_kernels_are_there_and_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    family = {k: v for k, v in meta.items() if "crf_ctct_" in k}
    assert sum(n for n, _ in KERNELS.values()) == len(family), sorted(family)
    for name, (count, ceiling) in KERNELS.items():
        mine = {k: v for k, v in family.items() if name in k}
        assert len(mine) == count, (name, sorted(mine))
        for k, v in mine.items():
            assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
            assert v["vgpr_count"] <= ceiling, (k, v)
