"""tests/cpp_sequence_pose/sequence_pose_dropin.cpp: RegisterEpipolarSequence (include/epipolar.h), RegisterPoseSequence
(include/pose.h) and RegisterPnPSequence (include/pnp.h) over three synthetic frames of its own, each pair against
RegisterEpipolar / RegisterPose / RegisterPnP with seed + k, byte for byte.  Plain g++, no HIP headers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_sequence_pose")
BIN = os.path.join(CPP, "sequence_pose_dropin")


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    source = open(os.path.join(CPP, "sequence_pose_dropin.cpp")).read()
    for call in ("RegisterEpipolarSequence(", "RegisterPoseSequence(", "RegisterPnPSequence(", "RegisterEpipolar(",
                 "RegisterPose(", "RegisterPnP(", "seed + k"):
        assert call in source, call
    for head in ("epipolar.h", "pose.h", "pnp.h"):
        assert "#include <hip" not in open(os.path.join(ROOT, "include", head)).read(), head


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    build_cpp()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
