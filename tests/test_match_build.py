"""Both matcher units (cusift_amd/csrc/sift_match.hip, sift_match8.hip, on sift_match_common.h) as hipcc builds them for
gfx950 -- kernels present, no scratch, no spills, LDS bytes, waves per SIMD and the MFMAs of a main kernel's body -- from
the code object's metadata and text through tools/kernel_regs.py (cross-compiled: no GPU needed)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# unit -> {kernel: (instances, LDS bytes, waves per SIMD, MFMAs in the body)}
# fp32: one LDS tile of 32 x 132 floats, + 2 x 4 x 32 (best, second, index) triples on the column side; int8: two tiles of
# 64 x 144 bytes, + 2 x 4 x 64 word pairs on the column side.  A main kernel's body holds one tile's MFMAs, written out:
# 8 k-steps x 4 x 2 accumulators (fp32), 4 B fragments x 4 row groups x 2 k halves (int8).
FP32, INT8 = "v_mfma_f32_16x16x4_f32", "v_mfma_i32_16x16x64_i8"
UNITS = {
    "sift_match.hip": (FP32, {
        "match_kernel": (2, 16896, 4, 64),
        "match_batch_kernel": (2, 16896, 4, 64),
        "match_guided_kernel": (4, 16896, 4, 64),
        "match_batch_guided_kernel": (4, 16896, 4, 64),
        "match_mutual_kernel": (2, 19968, 4, 64),
        "match_batch_mutual_kernel": (2, 19968, 4, 64),
        "match_merge_kernel": (1, 0, 8, 0),
        "match_batch_merge_kernel": (1, 0, 8, 0),
        "match_mutual_merge_kernel": (1, 0, 8, 0),
        "match_batch_mutual_merge_kernel": (1, 0, 8, 0),
    }),
    "sift_match8.hip": (INT8, {
        "match8_kernel": (2, 18432, 2, 32),
        "match8_batch_kernel": (2, 18432, 2, 32),
        "match8_mutual_kernel": (2, 22528, 2, 32),
        "match8_batch_mutual_kernel": (2, 22528, 2, 32),
        "match8_merge_kernel": (2, 0, 8, 0),
        "match8_batch_merge_kernel": (2, 0, 8, 0),
        "match8_mutual_merge_kernel": (2, 0, 8, 0),
        "match8_batch_mutual_merge_kernel": (2, 0, 8, 0),
        "quantize_kernel": (1, 0, 8, 0),
        "desc8_sums_kernel": (1, 0, 8, 0),
    }),
}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request):
    import kernel_regs

    asm = kernel_regs.assembly(request.param)
    return request.param, asm, kernel_regs.kernels(asm)


def family(name, table):
    """The kernel a mangled name instantiates: `<length><name>` is exact where a substring is not."""
    hits = [k for k in table if "%d%s" % (len(k), k) in name]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def test_every_kernel_is_there_in_its_instances(unit):
    src, _, kernels = unit
    table = UNITS[src][1]
    count = {k: 0 for k in table}
    for d in kernels:
        count[family(d["name"], table)] += 1
    assert count == {k: v[0] for k, v in table.items()}
    assert sum(len(t) for _, t in UNITS.values()) == 20


def test_no_scratch_no_spills_and_the_lds_and_occupancy_of_each_family(unit):
    import kernel_regs

    src, _, kernels = unit
    table = UNITS[src][1]
    for d in kernels:
        _, lds, waves, _ = table[family(d["name"], table)]
        print(d)
        assert d["private_segment_fixed_size"] == 0, d
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, d
        assert d["group_segment_fixed_size"] == lds, d
        assert kernel_regs.waves_per_simd(d) == waves, d


def test_a_main_kernel_body_holds_one_tile_of_its_units_mfma_and_no_other(unit):
    src, asm, kernels = unit
    mine, table = UNITS[src]
    other = INT8 if mine == FP32 else FP32
    for d in kernels:
        start = asm.index("\n%s:" % d["name"])
        body = asm[start:asm.index("; codeLenInByte", start)]
        assert len(re.findall(r"^\s+%s\s" % mine, body, flags=re.M)) == table[family(d["name"], table)][3], d["name"]
        assert other not in body, d["name"]
