"""The Python-free build: the top-level Makefile is the one recipe (python -m cusift_amd.build and CMakeLists.txt both
drive it); an installed tree is found by find_package(cusift_amd) and a consumer links the reference's detector test
against it with its ordinary C++ compiler (the reference is a CMake project: CMakeLists.txt:45-72)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_build_is_the_makefile():
    from cusift_amd import build as b

    lib = b.build()
    assert lib == os.path.join(ROOT, "cusift_amd", "libcusift_amd.so") and os.path.exists(lib)
    assert not b.is_stale()  # `make -q all` agrees
    text = open(os.path.join(ROOT, "Makefile")).read()
    for flag in ("-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=$(ARCH)"):
        assert flag in text
    for flag in b.HIPCC_FLAGS:  # the tools' copy of the flags says what the Makefile says
        assert flag in ("-shared",) or flag.replace("gfx950", "$(ARCH)") in text, flag


def test_one_product_build_and_no_dangling_tool_paths():
    """The product sources compile one way: their only preprocessor conditionals are the phase stamps (CUSIFT_STAMPS),
    sift_math.h's header guard and its host/device switch -- no experiment switch grows back.  And every tools/ path that
    the product and its documents cite exists."""
    csrc = os.path.join(ROOT, "cusift_amd", "csrc")
    allowed = {"#ifdef CUSIFT_STAMPS": None,  # (any file)
               "#ifndef CUSIFT_SIFT_MATH_H": "sift_math.h", "#if defined(__HIPCC__) || defined(__HIP__)": "sift_math.h"}
    stray = []
    for name in sorted(os.listdir(csrc)):
        for n, line in enumerate(open(os.path.join(csrc, name), errors="replace"), 1):
            text = " ".join(line.split("//")[0].replace("# ", "#").split())
            if re.match(r"#(if|ifdef|ifndef|elif)\b", text) and allowed.get(text, "") not in (None, name):
                stray.append("%s:%d: %s" % (name, n, text))
    assert not stray, stray

    cited = {}
    paths = [os.path.join(ROOT, f) for f in ("README.md", "DESIGN.md", "INTEGRATION.md", "BASELINE.md", "bench.py")]
    for d in ("cusift_amd", "include", "bench_legs"):
        for dirpath, dirnames, files in os.walk(os.path.join(ROOT, d)):
            dirnames[:] = [x for x in dirnames if x != "__pycache__"]
            paths += [os.path.join(dirpath, f) for f in files if not f.endswith((".so", ".o", ".pyc"))]
    for path in paths:
        for ref in re.findall(r"(?<![\w/.])tools/[\w./-]*\w", open(path, errors="replace").read()):
            cited.setdefault(ref, os.path.relpath(path, ROOT))
    assert cited  # the pattern finds what the documents cite
    missing = {ref: where for ref, where in cited.items() if not os.path.exists(os.path.join(ROOT, ref))}
    assert not missing, missing


@pytest.mark.skipif(shutil.which("cmake") is None, reason="cmake not installed")
def test_install_and_find_package(tmp_path):
    prefix = tmp_path / "prefix"
    subprocess.check_call(["make", "-C", ROOT, "install", "PREFIX=%s" % prefix], stdout=subprocess.DEVNULL)
    assert (prefix / "lib" / "libcusift_amd.so").exists() and (prefix / "include" / "cusift_amd" / "cuSIFT.h").exists()
    assert (prefix / "lib" / "cmake" / "cusift_amd" / "cusift_amdConfig.cmake").exists()
    src = tmp_path / "consumer"
    src.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "cpp", "detector_dropin.cpp"), src / "detector.cpp")
    (src / "CMakeLists.txt").write_text(
        "cmake_minimum_required(VERSION 3.16)\nproject(consumer LANGUAGES CXX)\n"
        "find_package(cusift_amd REQUIRED)\nadd_executable(detector detector.cpp)\n"
        "target_compile_features(detector PRIVATE cxx_std_14)\n"
        "target_link_libraries(detector PRIVATE cusift_amd::cusift_amd)\n")
    bld = tmp_path / "build"
    subprocess.check_call(["cmake", "-S", str(src), "-B", str(bld), "-DCMAKE_PREFIX_PATH=%s" % prefix],
                          stdout=subprocess.DEVNULL)
    subprocess.check_call(["cmake", "--build", str(bld)], stdout=subprocess.DEVNULL)
    assert (bld / "detector").exists()
    out = subprocess.run(["ldd", str(bld / "detector")], capture_output=True, text=True).stdout
    assert "libcusift_amd.so" in out
