"""The fused detection stays small enough for the instruction cache: the candidate block of
detect_chunk.inc holds ONE inlined CandList::refine_batch per row step -- the 20 (scale, column) cases only push -- so an
instantiation is ~30-35 KB of code with four keypoint-append sites (three row steps and the chunk's tail), not ~112 KB
with 61.  Checked on the assembly hipcc emits for the product's flags (cross-compiled here, no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ICACHE_BYTES = 65536  # assumed: AMD's public CDNA3 figure, 64 KB shared by two CUs (nothing states gfx950's)


@pytest.fixture(scope="session")
def detect_kernels():
    """{symbol: metadata + code bytes + atomic sites} of the kernels that paste detect_chunk.inc; one compile per session."""
    import kernel_regs

    asm = kernel_regs.assembly("sift_stencils.hip")  # cusift_amd.build.HIPCC_FLAGS
    code = kernel_regs.code_stats(asm)
    out = {}
    for k in kernel_regs.kernels(asm):
        if "detect_fused_kernel" in k["name"] or "detect_multi_kernel" in k["name"]:
            out[k["name"]] = dict(k, **code[k["name"]])
    return out


def test_every_instantiation_is_there(detect_kernels):
    fused = [n for n in detect_kernels if "detect_fused_kernel" in n]
    multi = [n for n in detect_kernels if "detect_multi_kernel" in n]
    assert len(fused) == 6 and len(multi) == 1, sorted(detect_kernels)


def test_fused_detection_fits_the_instruction_cache(detect_kernels):
    for n, k in detect_kernels.items():
        if "detect_fused_kernel" not in n:
            continue
        assert k["code_bytes"] < ICACHE_BYTES, (n, k["code_bytes"])
        # three row steps plus the tail of the chunk
        assert 1 <= k["atomic_add_sites"] <= 4, (n, k["atomic_add_sites"])
        assert k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 256, (n, k)


def test_multi_octave_launch_has_one_refinement_per_row_step(detect_kernels):
    n, k = next((n, k) for n, k in detect_kernels.items() if "detect_multi_kernel" in n)
    # both bodies (identity taps or not) live in this kernel: 2 x (three row steps + tail)
    assert 1 <= k["atomic_add_sites"] <= 8, (n, k["atomic_add_sites"])
    assert k["private_segment_fixed_size"] == 0, (n, k)
