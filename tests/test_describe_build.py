"""describe_given_kernel and the second-peak kernels as hipcc builds them for gfx950 -- registers, spills, scratch and
waves per SIMD from the code object's metadata (no GPU needed) -- and the C++ surface with plain g++."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_describe")
sys.path.insert(0, os.path.join(ROOT, "tools"))


_rows = {}


def keypoint_unit_rows():
    """{mangled kernel name: metadata} of sift_keypoints.hip, compiled once for the tests of this module"""
    import kernel_regs

    if not _rows:
        _rows.update({d["name"]: d for d in kernel_regs.kernels(kernel_regs.assembly("sift_keypoints.hip"))})
    return _rows


def test_describe_given_kernel_keeps_four_waves_per_simd():
    import kernel_regs

    rows = keypoint_unit_rows()
    mine = [d for name, d in rows.items() if "describe_given_kernel" in name]
    assert len(mine) == 1, sorted(rows)
    d = mine[0]
    print(d)
    assert d["vgpr_count"] + max(0, d["agpr_count"]) <= 128
    assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0  # nothing spills to memory
    assert kernel_regs.waves_per_simd(d) == 4
    # the same LDS as describe_all_kernel: KpShared and the prefix table -- the occupancy its grid is sized from
    ref = [r for name, r in rows.items() if "describe_all_kernel" in name][0]
    assert d["group_segment_fixed_size"] == ref["group_segment_fixed_size"]


def test_second_peak_kernels_fit_the_describe_grid():
    """ctx->describe_grid is sized from describe_all_kernel's occupancy and reused for both second-peak kernels: they
    must be resident in the same numbers -- nothing spilled to memory, at least 4 waves per SIMD, the same LDS."""
    import kernel_regs

    rows = keypoint_unit_rows()
    ref = [r for name, r in rows.items() if "describe_all_kernel" in name][0]
    for kernel in ("second_peak_kernel", "second_describe_kernel"):
        mine = [d for name, d in rows.items() if kernel in name]
        assert len(mine) == 1, (kernel, sorted(rows))
        d = mine[0]
        print(d)
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, kernel
        assert kernel_regs.waves_per_simd(d) >= 4, kernel
        assert d["group_segment_fixed_size"] == ref["group_segment_fixed_size"], kernel


def test_cpp_header_compiles_with_plain_gxx_with_describe_used():
    binary = os.path.join(CPP, "describe_dropin")
    if os.path.exists(binary):
        os.remove(binary)
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(binary)
    text = open(os.path.join(ROOT, "include", "cuSIFT.h")).read()
    assert re.search(r"void Describe\(cuImage &img, unsigned flags = 0, float subsampling = 1\.0f\)", text)
    assert re.search(r"inline void DescribeSift\(SiftData &siftData, cuImage &img, int numOctaves, float subsampling", text)
    src = open(os.path.join(CPP, "describe_dropin.cpp")).read()
    assert "data.Describe(img)" in src and "DescribeSift(added, img, 5" in src and "AddSiftData(added" in src
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
