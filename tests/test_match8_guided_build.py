"""The C++ drop-in program of tests/cpp_match8_guided: plain g++, no HIP headers; its GPU half compares
MatchSiftData8Guided (include/matching.h) and MatchSiftData8Projected (include/pnp.h) with the C calls
cusift_match8_guided / cusift_match8_projected and, at a radius every pair passes, with MatchSiftData8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_match8_guided")
BIN = os.path.join(CPP, "match8_guided_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    for header, name in (("matching.h", "MatchSiftData8Guided("), ("pnp.h", "MatchSiftData8Projected(")):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert name in text and "#include <hip" not in text, header
    src = open(os.path.join(CPP, "match8_guided_dropin.cpp")).read()
    for name in ("MatchSiftData8Guided(", "MatchSiftData8Projected(", "cusift_match8_guided(", "cusift_match8_projected(",
                 "MatchSiftData8("):
        assert name in src, name


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    build()
    out = subprocess.run([BIN, GRAY1], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
