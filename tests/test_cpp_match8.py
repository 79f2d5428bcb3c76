"""The C++ drop-in for the 8-bit descriptors: SiftDescriptors8, QuantizeSiftData and MatchSiftData8 (include/matching.h) in
tests/cpp_match8, plain g++.  The program prints counts and checksums; this file recomputes them in numpy
(tests/match8_model.py) from the records the program extracted."""
import os
import re
import subprocess

import numpy as np
import pytest

from match8_model import FIELDS, match8_model, quantize_model
from oracle_binding import SIFT_POINT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_match8")
BIN = os.path.join(CPP, "match8_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")
THRESHOLDS = (999.0, 0.8)


def build():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def checksum(raw):
    """sum_i (i + 1) * byte_i modulo 2^64, the program's."""
    b = np.frombuffer(np.ascontiguousarray(raw).tobytes(), np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((np.arange(1, len(b) + 1, dtype=np.uint64) * b).sum(dtype=np.uint64))


def test_match8_dropin_compiles_and_links_with_gxx():
    """No HIP headers on the include path: matching.h over cusift_amd_extras.h is self-contained C++."""
    if os.path.exists(BIN):
        os.remove(BIN)
    build()
    text = open(os.path.join(ROOT, "include", "matching.h")).read()
    for name in ("struct SiftDescriptors8", "InitSiftDescriptors8(", "FreeSiftDescriptors8(", "QuantizeSiftData(",
                 "MatchSiftData8("):
        assert name in text, name
    assert "#include <hip" not in text


@pytest.mark.gpu
def test_match8_dropin_counts_and_checksums_on_gpu(tmp_path):
    build()
    path = str(tmp_path / "records.bin")
    out = subprocess.run([BIN, GRAY1, path, "%r" % THRESHOLDS[0], "%r" % THRESHOLDS[1]], capture_output=True, text=True,
                         timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    said = {k: [int(v) for v in rest.split()] for k, rest in re.findall(r"^(counts|bytes|fields|pairs) (.+)$", out.stdout,
                                                                        flags=re.M)}
    raw = open(path, "rb").read()
    n1, n2 = (int(v) for v in np.frombuffer(raw[:8], "<i4"))
    recs = np.frombuffer(raw[8:], SIFT_POINT_DTYPE)
    assert len(recs) == n1 + n2 and n1 > n2 >= 100
    s1, s2 = recs[:n1], recs[n1:]
    q1, q2 = quantize_model(s1["data"]), quantize_model(s2["data"])
    assert said["bytes"] == [checksum(q1), checksum(q2)]
    m = match8_model(q1, q2, 1, s2["coords2D"])
    fields = np.zeros(n1, np.dtype([(f, m[f].dtype) for f in FIELDS]))
    for f in FIELDS:
        fields[f] = m[f]
    assert fields.dtype.itemsize == 20
    assert said["fields"] == [checksum(fields)]
    # MatchSiftData's filter: squared thresholds, a match inside set 2
    keep = (m["score"] < np.float32(THRESHOLDS[0]) ** 2) & (m["ambiguity"] < np.float32(THRESHOLDS[1]) ** 2)
    keep &= (m["match"] >= 0) & (m["match"] < n2)
    pairs = np.stack([np.flatnonzero(keep), m["match"][keep]], 1).astype(np.int32)
    assert said["counts"] == [n1, n2, len(pairs)] and 0 < len(pairs) < n1
    assert said["pairs"] == [checksum(pairs)]
