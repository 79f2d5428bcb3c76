"""The drop-in program of tests/cpp_describe: SiftData::Describe returns an extraction's records byte for byte, and
DescribeSift describes keypoints that AddSiftData put on the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_describe")
BIN = os.path.join(CPP, "describe_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")


@pytest.mark.gpu
def test_cpp_dropin_describes_given_records():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([BIN, GRAY1], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASSED" in out.stdout, out.stdout + out.stderr
    rows = re.findall(r"described (\d+) records( \(RootSIFT\))?: (\d+) round-trip mismatches, (\d+) from AddSiftData", out.stdout)
    assert len(rows) == 2 and rows[1][1], out.stdout
    for n, _, bad_round, bad_added in rows:
        assert int(n) == 1222 and int(bad_round) == 0 and int(bad_added) == 0, out.stdout
