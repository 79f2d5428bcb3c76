"""The kernels of the homography, fundamental-matrix and PnP chains (cusift_amd/csrc/sift_planar.hip, sift_epipolar.hip,
sift_pnp.hip, sift_sequence.hip, on sift_ransac_chain.h) as hipcc builds them for gfx950 -- kernels present, no scratch, no
spills, LDS bytes, waves per SIMD, registers and the one atomic add of a scoring kernel -- from the code object's metadata
and text through tools/kernel_regs.py (cross-compiled: no GPU needed).

The figures are those of the build BEFORE the score, mark, gather and null-vector bodies were put on one template each:
LDS and waves per SIMD equal, VGPR + AGPR equal or lower (no kernel needs the exception for a higher count that leaves
the waves unchanged).  profiles/ransac_refactor.json has the table and the comparison of the assembly text.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# unit -> {kernel: (VGPR + AGPR, LDS bytes, waves per SIMD, global_atomic_add sites)}
UNITS = {
    "sift_planar.hip": {
        "planar_mark_kernel": (18, 16, 8, 0),
        "planar_compact_kernel": (15, 1040, 8, 0),
        "planar_score_kernel": (47, 2048, 8, 1),
        "planar_select_kernel": (159, 4296, 3, 0),
    },
    "sift_epipolar.hip": {
        "epipolar_solve_kernel": (94, 39168, 5, 0),
        "epipolar_score_kernel": (56, 2048, 8, 1),
        "epipolar_select_kernel": (372 + 116, 4952, 1, 0),
    },
    "sift_pnp.hip": {
        "pnp_mark_kernel": (24, 16, 8, 0),
        "pnp_solve_kernel": (104, 70656, 4, 0),
        "pnp_score_kernel": (68, 2560, 7, 1),
        "pnp_select_kernel": (200, 4296, 2, 0),
    },
    "sift_sequence.hip": {
        "sequence_mark_kernel": (14, 16, 8, 0),
        "sequence_pnp_mark_kernel": (18, 16, 8, 0),
        "sequence_select_kernel": (27, 16, 8, 0),
    },
}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request):
    import kernel_regs

    asm = kernel_regs.assembly(request.param)
    return request.param, kernel_regs.kernels(asm), kernel_regs.code_stats(asm)


def family(name, table):
    """The kernel a mangled name stands for: `<length><name>` is exact where a substring is not."""
    hits = [k for k in table if "%d%s" % (len(k), k) in name]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def test_every_kernel_is_there_once(unit):
    src, kernels, _ = unit
    assert sorted(family(d["name"], UNITS[src]) for d in kernels) == sorted(UNITS[src])
    assert sum(len(t) for t in UNITS.values()) == 14


def test_no_scratch_no_spills_and_the_lds_occupancy_and_registers_of_the_parent(unit):
    import kernel_regs

    src, kernels, code = unit
    for d in kernels:
        regs, lds, waves, atomics = UNITS[src][family(d["name"], UNITS[src])]
        print(d, code[d["name"]])
        assert d["private_segment_fixed_size"] == 0, d
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, d
        assert d["group_segment_fixed_size"] == lds, d
        assert kernel_regs.waves_per_simd(d) == waves, d
        assert d["vgpr_count"] + max(0, d["agpr_count"]) <= regs, d
        assert code[d["name"]]["atomic_add_sites"] == atomics, d
