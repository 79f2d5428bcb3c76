"""What the mutual 8-bit matcher and the match-bits setting add to the build: the three symbols in header, library and
binding; the new kernels in the sift_match8.hip unit for gfx950, on the int8 matrix pipe, without scratch or spills
(through tools/kernel_regs.py, cross-compiled: no GPU needed); and the C++ drop-in program of tests/cpp_match8_mutual,
plain g++, whose GPU half compares MatchSiftData8Mutual with MatchSiftData8 in both directions and SetMatchBits(8) +
RegisterPlanar with the staged route."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_match8_mutual")
BIN = os.path.join(CPP, "match8_mutual_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")
SYMBOLS = {"cusift_match8_mutual": 10, "cusift_match8_batch_mutual": 11, "cusift_ctx_set_match_bits": 2}


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_symbols_are_declared_exported_and_bound():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert re.search(r"^int %s\(cusift_ctx \*ctx" % name, extras, flags=re.M), name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    for method in ("match8_mutual", "match8_batch_mutual", "set_match_bits"):
        assert callable(getattr(capi.Context, method)), method
    assert callable(batch.BatchExtractor.match8_mutual)
    # the definition of the column side, the symmetry the tests use and both scratch formulas are in the header
    text = extras.split("int cusift_match8_mutual(")[0].rsplit("/*", 1)[1]
    for needle in ("LOWEST row", "second smallest key", "BYTE FOR BYTE", "ceil(num_pts1 / 256) x num_pts2", "no atomics"):
        assert needle in text, needle
    assert "n_pairs x ceil(max_pts / 256) x max_pts" in extras


def test_new_kernels_compile_for_gfx950_on_the_int8_pipe_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_match8.hip")
    assert "gfx950" in asm
    kernels = kernel_regs.kernels(asm)
    for needle, count, mfma in (("match8_mutual_kernel", 2, True), ("match8_batch_mutual_kernel", 2, True),
                                ("match8_mutual_merge_kernel", 2, False), ("match8_batch_mutual_merge_kernel", 2, False)):
        found = [k for k in kernels if needle in k["name"]]
        assert len(found) == count, (needle, [k["name"] for k in found])  # both distances
        for k in found:
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
            start = asm.index("\n%s:" % k["name"])
            body = asm[start:asm.index("; codeLenInByte", start)]
            assert ("v_mfma_i32_16x16x64_i8" in body) == mfma, k["name"]
            if mfma:
                assert "atomic" not in body, k["name"]


def test_cpp_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    text = open(os.path.join(ROOT, "include", "matching.h")).read()
    assert "MatchSiftData8Mutual(" in text and "inline void SetMatchBits(int bits)" in text and "#include <hip" not in text
    src = open(os.path.join(CPP, "match8_mutual_dropin.cpp")).read()
    for name in ("MatchSiftData8Mutual(", "SetMatchBits(8)", "RegisterPlanar(", "MatchSiftData8("):
        assert name in src, name


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    build()
    out = subprocess.run([BIN, GRAY1], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
