"""The C++ drop-in for guided matching: MatchSiftDataGuided (include/matching.h) in tests/cpp_guided, plain g++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_guided")
BIN = os.path.join(CPP, "guided_dropin")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_guided_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: matching.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "matching.h")).read()
    assert "MatchSiftDataGuided(" in text and "cusift_match_guided(" in text and "#include <hip" not in text


@pytest.mark.gpu
def test_guided_dropin_equals_match_sift_data_and_passes_nothing_on_gpu():
    """Under a huge radius MatchSiftDataGuided is MatchSiftData -- records and pairs -- and under a zero model every
    record comes back with match == -1 (the program checks both, for both kinds of model)."""
    build()
    out = subprocess.run([BIN, os.path.join(GOLDEN, "vlfeat_sift1.bin"), os.path.join(GOLDEN, "vlfeat_sift2.bin"),
                          "999", "0.95"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and out.stdout.count("records unmatched, 0 pairs") == 2
