"""The C++ drop-in for bundle adjustment: BundleAdjust (include/tracks.h) in tests/cpp_bundle, plain g++.  The program
round-trips Scene A's poses and points and prints the summary, the history and the poses, which must be the model's."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_bundle")
BIN = os.path.join(CPP, "bundle_dropin")
ITERATIONS = 5


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_bundle_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: tracks.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "tracks.h")).read()
    for name in ("BundleAdjust(", "cusift_bundle_adjust(", "cusift_bundle_default_params("):
        assert name in text, name
    assert "#include <hip" not in text
    assert "tests/cpp_bundle/bundle_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    assert "tests/cpp_bundle/bundle_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "sift_bundle" in make.split("SOURCES :=")[1].split("HEADERS")[0] and "cpp_bundle" in make


@pytest.mark.gpu
def test_bundle_dropin_on_gpu(tmp_path):
    import bundle_model as bm

    build()
    sc = bm.scene_a()
    path = tmp_path / "scene.bin"
    with open(path, "wb") as f:
        np.asarray([sc["n"], sc["max_pts"], len(sc["offsets"]) - 1, len(sc["obs"]), ITERATIONS], "<i4").tofile(f)
        np.asarray(sc["cam"], "<f4").tofile(f)
        for arr, dt in ((sc["xy"], "<f4"), (sc["offsets"], "<i4"), (sc["obs"], "<i4"), (sc["poses"], "<f8"),
                        (sc["points"], "<f8")):
            np.ascontiguousarray(arr, dtype=dt).tofile(f)
    out = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    model = bm.run_model(sc, iterations=ITERATIONS)

    def near(got, want):
        got, want = np.asarray(got, float), np.asarray(want, float)
        return (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))).all()

    said = {k: [float(v) for v in rest.split()] for k, rest in re.findall(r"^(summary|points) (.+)$", out.stdout, flags=re.M)}
    assert near(said["summary"], model["summary"])
    history = np.array([[float(v) for v in rest.split()] for rest in re.findall(r"^history \d+ (.+)$", out.stdout, flags=re.M)])
    assert history.shape == (ITERATIONS, 4) and near(history, model["history"])
    poses = np.array([[float(v) for v in rest.split()] for rest in re.findall(r"^pose \d+ (.+)$", out.stdout, flags=re.M)])
    assert near(poses.reshape(-1, 3, 4), model["poses"])
    assert near(said["points"], [np.abs(model["points3d"][:, :3]).sum(), model["points3d"][:, 3].max()])
