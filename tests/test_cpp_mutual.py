"""The C++ drop-in for mutual matching: MatchSiftDataMutual (include/matching.h) in tests/cpp_mutual, plain g++."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_mutual")
BIN = os.path.join(CPP, "mutual_dropin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
THRESHOLDS = (999.0, 0.95)


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_mutual_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: matching.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "matching.h")).read()
    assert "MatchSiftDataMutual(" in text and "#include <hip" not in text


@pytest.mark.gpu
def test_mutual_dropin_returns_the_selected_pairs_on_gpu(ctx):
    """The pairs MatchSiftDataMutual returns on the VLFeat fixture pair are the ones cusift_select_mutual's definition
    gives on the fields cusift_match_mutual writes (test_match_mutual.py), in the same order."""
    from test_match_mutual import expected_selection, fixture_pair, gpu_mutual

    build()
    out = subprocess.run([BIN, os.path.join(GOLDEN, "vlfeat_sift1.bin"), os.path.join(GOLDEN, "vlfeat_sift2.bin"),
                          "%r" % THRESHOLDS[0], "%r" % THRESHOLDS[1]], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    got = [(int(a), int(b)) for a, b in re.findall(r"^pair (\d+) (\d+)$", out.stdout, flags=re.M)]
    s1, s2 = fixture_pair()
    r1, r2 = gpu_mutual(ctx, s1, s2, 1)
    want, _ = expected_selection(r1, r2, *THRESHOLDS, False, True)
    assert 0 < len(want) < len(s1)
    assert got == [tuple(int(v) for v in row) for row in want]
