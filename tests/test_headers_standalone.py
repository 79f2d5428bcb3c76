"""Every header under include/ compiles on its own: a translation unit that includes just that header passes
g++ -std=c++14 -Wall -Wextra -fsyntax-only without a word.  A header that only compiles after another one -- because a
shared piece such as cusift_dropin::SequencePack (sequence.h) moved -- fails here and not in a caller's build."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h")))


def test_the_header_list_is_not_empty():
    assert "sequence.h" in HEADERS and "cuSIFT.h" in HEADERS and len(HEADERS) >= 17, HEADERS


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header, tmp_path):
    unit = tmp_path / "only.cpp"
    unit.write_text('#include "%s"\n' % header)
    out = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, str(unit)],
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "" and out.stderr == "", out.stdout + out.stderr
