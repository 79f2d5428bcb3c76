"""What hipcc makes of cusift_amd/csrc/sift_match8.hip for gfx950, through tools/kernel_regs.py (cross-compiled: no GPU
needed): no kernel uses scratch or spills, the match kernels run on the int8 matrix pipe, and nothing in the unit is an
fp32 MFMA."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def unit():
    import kernel_regs

    asm = kernel_regs.assembly("sift_match8.hip")
    return asm, kernel_regs.kernels(asm)


def body(asm, symbol):
    """The instructions of one kernel: from its label to its `codeLenInByte` line."""
    start = asm.index("\n%s:" % symbol)
    return asm[start:asm.index("; codeLenInByte", start)]


def test_no_scratch_and_no_spills(unit):
    _, kernels = unit
    names = [k["name"] for k in kernels]
    for needle in ("match8_kernel", "match8_batch_kernel", "match8_merge_kernel", "match8_batch_merge_kernel",
                   "quantize_kernel", "desc8_sums_kernel"):
        assert any(needle in n for n in names), needle
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_match_kernels_use_the_int8_mfma_and_nothing_uses_an_fp32_one(unit):
    asm, kernels = unit
    matchers = [k["name"] for k in kernels if re.search(r"match8_(batch_)?kernel", k["name"])]
    assert len(matchers) == 4  # pair and pair list, both distances
    for name in matchers:
        assert "v_mfma_i32_16x16x64_i8" in body(asm, name), name
    assert "v_mfma_f32" not in asm
