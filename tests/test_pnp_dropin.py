"""tests/cpp_pnp/pnp_dropin.cpp: include/pnp.h compiles and links with plain g++; on the GPU the program passes on its own
planted scene, and, given a scene of tests/test_pnp.py as record files, RegisterPnP reproduces the bytes of the Python call
for the same seed."""
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_planar import upload
from test_pnp import REFINE_THRESH, ROT_BOUND, RULE, THRESH, TRANS_BOUND, camera, case, pnp_candidates, truth_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_pnp")
BIN = os.path.join(CPP, "pnp_dropin")


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_header_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    assert "#include <hip" not in open(os.path.join(ROOT, "include", "pnp.h")).read()
    assert "cpp_pnp" in open(os.path.join(ROOT, "Makefile")).read()


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    build_cpp()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "RegisterPnP:" in out.stdout and "EstimatePnP:" in out.stdout


def with_partners(pts, seed=5):
    """(frame 1, frame 2): `pts` with a descriptor of its own per record, and a second frame whose record i sits at the
    match position of record i and carries the same descriptor, so the matcher restores the match fields of `pts`."""
    rng = np.random.default_rng(seed)
    desc = rng.uniform(0, 1, size=(len(pts), 128)) ** 4
    desc = (desc / np.sqrt((desc * desc).sum(axis=1))[:, None]).astype(np.float32)
    f1, f2 = pts.copy(), np.zeros(len(pts), dtype=SIFT_POINT_DTYPE)
    f1["data"], f2["data"] = desc, desc
    f1["match"], f1["score"], f1["ambiguity"], f1["match_xpos"], f1["match_ypos"] = -1, 0, 0, 0, 0
    f2["coords2D"][:, 0], f2["coords2D"][:, 1] = pts["match_xpos"], pts["match_ypos"]
    return f1, f2


@pytest.mark.gpu
def test_cpp_call_reproduces_the_python_calls_bytes(ctx, tmp_path):
    """One scene, one seed: the `fxfy` scene of tests/test_pnp.py (fx != fy, a 1-based origin) as two record files."""
    build_cpp()
    c = case("fxfy")
    v1, v2 = with_partners(c.pts)
    loops, seed = 300, 0xC0FFEE
    (tmp_path / "f1.bin").write_bytes(v1.tobytes())
    (tmp_path / "f2.bin").write_bytes(v2.tobytes())
    cmd = [BIN, str(tmp_path / "f1.bin"), str(tmp_path / "f2.bin")] + ["%r" % v for v in c.cam2] + \
        [str(loops), hex(seed), repr(RULE["lo"]), repr(RULE["hi"]), repr(THRESH), repr(REFINE_THRESH), str(tmp_path / "out.bin")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "PASSED" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    b1, b2 = upload(ctx, v1), upload(ctx, v2)
    res = ctx.register_pnp(b1.ptr, len(v1), b2.ptr, len(v2), camera(c.cam2), distance=0, loops=loops, seed=seed,
                           thresh=THRESH, refine_loops=5, refine_thresh=REFINE_THRESH, **RULE)
    after = b1.to_numpy(SIFT_POINT_DTYPE, (len(v1),))
    b1.free()
    b2.free()
    r, t = truth_errors(res.rt, c.R21, c.t21)
    print("%d candidates, %d inliers, %d fit; rotation %.4f degrees, translation %.4f of |t|" %
          (res.num_candidates, res.num_matches, res.num_fit, r, t))
    assert np.array_equal(after["match"], np.arange(len(v1))) and res.num_candidates == len(pnp_candidates(c.pts, **RULE))
    assert res.num_fit >= 190 and r <= ROT_BOUND and t <= TRANS_BOUND
    want = res.rt.tobytes() + res.ransac.tobytes() + \
        np.array([res.num_candidates, res.num_matches, res.num_fit], np.int32).tobytes() + after["match_error"].tobytes()
    assert raw == want
