"""CPU test of what can be read off the compiled gfx950 code of the join stages of rnnt_loss_simple (cat_amd/csrc/k_rnnt_join.hip): every
kernel of the family is there, none spills or uses scratch, and each stays under the register ceiling its launch geometry relies on.  The
assembly is the cached one of tests/test_isa_checks.py.  (Presence, registers, spills and scratch only: no instruction is looked for.)"""
import os
import shutil

import pytest

from tests.test_isa_checks import HIPCC, _assembly, _kernel_meta, _tool

# kernel -> (instantiations: fp32 / bf16 / fp16, VGPR ceiling).  The build has 53 (row), 127 (grad), 10 (fold).
#   row: a workgroup of 256 threads (one wave per SIMD) with 2 x 32 x 132 floats = 33 792 bytes of LDS; four of them fit the 160 KiB of a
#     compute unit, and it is the other three that cover a workgroup's staging loads and barriers -- four waves per SIMD need <= 128
#     registers each.  The 2 x 2 nodes' (maximum, sum) pairs and the four 16-byte LDS operands of a step are 24 of them.
#   grad: a thread holds 32 values of g and 32 sums of d g (64 registers) beside the frame's f, its sum and the node's four scalars; <= 128
#     keeps four workgroups (of 256 threads, 8 KiB of LDS) on a compute unit, which cover the per-frame load of f and the two barriers per
#     chunk of 16 frames.
#   fold: nothing but loads and stores to wait for -- 64 registers keep eight waves per SIMD in flight.
KERNELS = {"crf_join_row_kernel": (3, 128), "crf_join_grad_kernel": (3, 128), "crf_join_fold_kernel": (3, 64)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.timeout(900)
def test_join_kernels_are_there_and_neither_spill_nor_use_scratch():
    meta = _kernel_meta(_assembly(_tool()))
    family = {k: v for k, v in meta.items() if "crf_join_" in k}
    assert sum(n for n, _ in KERNELS.values()) == len(family), sorted(family)
    assert not any("crf_rnnt_" in k for k in family)                 # (tests/test_rnnt_isa.py counts that family by name)
    for name, (count, ceiling) in KERNELS.items():
        mine = {k: v for k, v in family.items() if name in k}
        assert len(mine) == count, (name, sorted(mine))
        for k, v in mine.items():
            print(k, v)
            assert v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0 and v["private_segment_fixed_size"] == 0, (k, v)
            assert v["vgpr_count"] <= ceiling, (k, v)
