"""SiftData::secondOrientation and SecondOrientationsSift through include/cuSIFT.h: the program builds with plain g++
(no GPU needed); on the GPU it extracts gray1.pgm and checks the count the oracle gives and every duplicate against its
parent."""
import os
import re
import subprocess

import pytest

import second_orientation_model as som

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_second_orientation")
BIN = os.path.join(CPP, "second_orientation_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")


def test_cpp_header_compiles_with_plain_gxx_with_second_orientation_used():
    if os.path.exists(BIN):
        os.remove(BIN)
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)
    src = open(os.path.join(CPP, "second_orientation_dropin.cpp")).read()
    assert "data.secondOrientation = 0.8f;" in src and "SecondOrientationsSift(plain, img, 5)" in src
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    for name in ("Makefile", "CMakeLists.txt"):  # both build recipes know the program
        assert "cpp_second_orientation" in open(os.path.join(ROOT, name)).read(), name


@pytest.mark.gpu
def test_cpp_dropin_duplicates_second_orientations(oracle, gray1):
    kw = som.CASES["full-3.0"][2]
    recs, tap, _, _ = som.oracle_input(oracle, gray1, **kw)
    n, m = len(recs), int(som.parents_of(tap, som.RATIO).sum())
    assert (n, m) == (106, 20)
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([BIN, GRAY1, str(n), str(n + m)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASSED" in out.stdout, out.stdout + out.stderr
    got = re.search(r"second orientations: (\d+) keypoints, (\d+) duplicates, (\d+) head mismatches, (\d+) out of order", out.stdout)
    assert got and [int(v) for v in got.groups()] == [n, m, 0, 0], out.stdout
