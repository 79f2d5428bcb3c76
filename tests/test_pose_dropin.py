"""tests/cpp_pose/pose_dropin.cpp: include/pose.h compiles and links with plain g++, and the program passes on the GPU --
RegisterPose against the planted pose and 3-D points, EstimatePose against RegisterPose, the refusal of a NULL camera."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_pose")
BIN = os.path.join(CPP, "pose_dropin")


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_header_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    assert "#include <hip" not in open(os.path.join(ROOT, "include", "pose.h")).read()
    assert "cpp_pose" in open(os.path.join(ROOT, "Makefile")).read()


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    build_cpp()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "RegisterPose:" in out.stdout and "EstimatePose:" in out.stdout
