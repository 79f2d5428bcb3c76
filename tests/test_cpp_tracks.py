"""The C++ drop-in for feature tracks: BuildTracks and TriangulateTracks (include/tracks.h) in tests/cpp_tracks, plain
g++.  The program checks its own tracks -- one keypoint of the fixture in up to four crops, at the plane's depth -- and
prints its counts."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_tracks")
BIN = os.path.join(CPP, "tracks_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_tracks_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: tracks.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "tracks.h")).read()
    for name in ("BuildTracks(", "TriangulateTracks(", "cusift_build_tracks(", "cusift_triangulate_tracks("):
        assert name in text, name
    assert "#include <hip" not in text
    assert "tests/cpp_tracks/tracks_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    assert "tests/cpp_tracks/tracks_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "sift_tracks" in make.split("SOURCES :=")[1].split("HEADERS")[0] and "cpp_tracks" in make


def test_tracks_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "tracks.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_tracks_dropin_on_gpu():
    build()
    out = subprocess.run([BIN, GRAY1], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    said = {k: [int(v) for v in re.findall(r"\d+", rest)] for k, rest in
            re.findall(r"^(tracks|views|consistent|depth) (.+)$", out.stdout, flags=re.M)}
    n_tracks, n_obs = said["tracks"][0], said["tracks"][1]
    assert sum(said["views"]) == n_tracks and sum(v * c for v, c in zip((2, 3, 4), said["views"])) == n_obs
    assert 0 < said["depth"][0] <= n_tracks and 0 < said["consistent"][0] <= n_tracks
