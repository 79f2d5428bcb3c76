"""The C++ drop-in for matching by projection: MatchSiftDataProjected (include/pnp.h) in tests/cpp_projected, plain g++."""
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_projected")
BIN = os.path.join(CPP, "projected_dropin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
# the literals of tests/cpp_projected/projected_dropin.cpp
POSE = (0.9995, -0.015, -0.03, 0.05, 0.0152, 0.9998, 0.02, -0.03, 0.0297, -0.0204, 0.9993, 0.04)
CAM = (800.0, 790.0, 400.5, 300.5, 1.0)
RADIUS = 40.0


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def lifted(pts):
    """The program's lift(data1, true), operation by operation in float32."""
    f = np.float32
    fx, fy, cx, cy, origin = (f(v) for v in CAM)
    px, py = cx - origin, cy - origin
    i = np.arange(len(pts))
    z = np.where(i % 7 == 3, f(0), f(1) + f(0.25) * (i % 13).astype(f)).astype(f)
    u, v = (pts["coords2D"][:, 0] - px) / fx, (pts["coords2D"][:, 1] - py) / fy
    assert u.dtype == f and v.dtype == f
    out = pts.copy()
    out["coords3D"] = np.stack([u * z, v * z, z], axis=1)
    return out


def test_projected_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: pnp.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "pnp.h")).read()
    assert "MatchSiftDataProjected(" in text and "cusift_match_projected(" in text and "#include <hip" not in text
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    assert "cpp_projected" in open(os.path.join(ROOT, "Makefile")).read()
    assert "tests/cpp_projected/projected_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_the_synthetic_scene_passes_a_share_of_the_pairs():
    """The condition on the GPU test's input, where a machine without a GPU sees it too: the guide is neither empty nor
    everything, and a seventh of the rows have no depth."""
    from test_match_projected import project_mask

    s1 = lifted(read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin")))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    mask = project_mask(POSE, CAM, s1["coords3D"], s2["coords2D"], RADIUS)
    i = np.arange(len(s1))
    assert 0.001 <= mask.mean() <= 0.30, mask.mean()
    assert not mask[i % 7 == 3].any() and mask[i % 7 != 3].any(axis=1).mean() > 0.25


@pytest.mark.gpu
def test_projected_dropin_equals_the_python_calls_bytes_on_gpu(ctx, tmp_path):
    """The program's own checks pass -- a huge radius is MatchSiftData, a zero pose matches nothing -- and the five fields
    it writes under the synthetic depth and pose are the bytes of Context.match_projected on the same records."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    build()
    out_bin = str(tmp_path / "out.bin")
    out = subprocess.run([BIN, os.path.join(GOLDEN, "vlfeat_sift1.bin"), os.path.join(GOLDEN, "vlfeat_sift2.bin"),
                          "999", "0.95", out_bin], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "records unmatched, 0 pairs" in out.stdout
    s1 = lifted(read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin")))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    try:
        ctx.match_projected(d1.ptr, len(s1), d2.ptr, len(s2), POSE, capi.Camera(*CAM), RADIUS, 1)
        ctx.synchronize()
        got = d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),))
    finally:
        d1.free()
        d2.free()
    raw = open(out_bin, "rb").read()
    assert len(raw) == 20 * len(s1) + 4
    theirs = np.frombuffer(raw[:20 * len(s1)], np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4"),
                                                         ("match_xpos", "<f4"), ("match_ypos", "<f4")]))
    for f in FIELDS:
        assert theirs[f].tobytes() == np.ascontiguousarray(got[f]).tobytes(), f
    pairs = int(np.frombuffer(raw[-4:], "<i4")[0])
    assert pairs == ((got["score"] < np.float32(999.0) ** 2) & (got["ambiguity"] < np.float32(0.95) ** 2) &
                     (got["match"] >= 0)).sum() > 0
    assert (got["match"] >= 0).sum() >= 0.25 * len(s1)
