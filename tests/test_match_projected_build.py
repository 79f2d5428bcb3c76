"""The projected matcher's unit (cusift_amd/csrc/sift_match_project.hip, on sift_match_block.h) as hipcc builds it for
gfx950 -- kernels present, no scratch, no spills, LDS bytes, waves per SIMD and the MFMAs of a kernel's body -- from the
code object's metadata and text through tools/kernel_regs.py (cross-compiled: no GPU needed), as tests/test_match_build.py
holds sift_match.hip.  The figures are the H guide's: the same LDS tile, the same eight floats per lane behind the fp64
prologue."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "sift_match_project.hip"
FP32, INT8 = "v_mfma_f32_16x16x4_f32", "v_mfma_i32_16x16x64_i8"
# kernel: (instances, LDS bytes, waves per SIMD, MFMAs in the body)
KERNELS = {
    "match_projected_kernel": (2, 16896, 4, 64),
    "match_batch_projected_kernel": (2, 16896, 4, 64),
}


@pytest.fixture(scope="module")
def unit():
    import kernel_regs

    asm = kernel_regs.assembly(UNIT)
    return asm, kernel_regs.kernels(asm)


def family(name):
    """The kernel a mangled name instantiates: `<length><name>` is exact where a substring is not."""
    hits = [k for k in KERNELS if "%d%s" % (len(k), k) in name]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def test_both_kernels_in_two_instances_and_nothing_else(unit):
    _, kernels = unit
    count = {k: 0 for k in KERNELS}
    for d in kernels:
        count[family(d["name"])] += 1
    assert count == {k: v[0] for k, v in KERNELS.items()}
    assert len(kernels) == 4


def test_no_scratch_no_spills_and_the_lds_and_occupancy_of_the_h_guide(unit):
    import kernel_regs

    _, kernels = unit
    for d in kernels:
        _, lds, waves, _ = KERNELS[family(d["name"])]
        print(d)
        assert d["private_segment_fixed_size"] == 0, d
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, d
        assert d["group_segment_fixed_size"] == lds, d
        assert kernel_regs.waves_per_simd(d) == waves, d


def test_a_body_holds_one_tile_of_fp32_mfma_and_no_int8(unit):
    asm, kernels = unit
    for d in kernels:
        start = asm.index("\n%s:" % d["name"])
        body = asm[start:asm.index("; codeLenInByte", start)]
        assert len(re.findall(r"^\s+%s\s" % FP32, body, flags=re.M)) == KERNELS[family(d["name"])][3], d["name"]
        assert INT8 not in body, d["name"]


def test_the_unit_is_in_both_build_recipes():
    """The Makefile lists its units by name; CMakeLists.txt takes every .hip of the directory as a dependency."""
    assert re.search(r"^SOURCES :=(.|\\\n)*\bsift_match_project\b", open(os.path.join(ROOT, "Makefile")).read(), flags=re.M)
    assert "cusift_amd/csrc/*.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
