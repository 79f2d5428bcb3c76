#!/usr/bin/env python3
"""Regenerate the RGB-D registration fixtures under tests/golden/ from the reference's own test data.

Run where the reference tree exists (needs PIL to decode the PNGs; the tests need numpy alone):

    python tests/golden/make_rgbd_fixtures.py /path/to/reference

All four are DATA the reference ships for its (commented-out) RANSACTestImage, test/test.cpp:136-184:

* rgbd_depth.npz   <- test/data/depth1.png, depth2.png   640x480 16-bit grey, the RAW samples as stored in the PNG
                      (SUN3D encoding: the depth in millimetres rotated left by 3 bits), arrays "depth1", "depth2"
                      uint16 [480, 640], numpy.savez_compressed
* rgbd_intrinsics.txt <- test/data/INTRINSICS            the 3x3 camera matrix as text, MATLAB 1-based pixel centres
* rgbd_match1_2.bin   <- test/data/match/match1_2        u32 n = 326; n x {f64 xyz of frame 1, f64 xyz of frame 2}
                                                          (extras/debug.cpp:244-280)
* rgbd_Rt1_2.bin      <- test/data/Rt/Rt1_2              f64[12], [R | t] row-major, x1 ~ R x2 + t (extras/debug.cpp:394-406)

The VLFeat dumps and match_indices1_2.bin the same test needs are written by make_fixtures.py.
"""
import os
import shutil
import sys

import numpy as np
from PIL import Image

if len(sys.argv) != 2:
    sys.exit(__doc__)
ref = sys.argv[1]
here = os.path.dirname(os.path.abspath(__file__))
src = os.path.join(ref, "test", "data")

depth = {}
for name in ("depth1", "depth2"):
    im = Image.open(os.path.join(src, name + ".png"))
    assert im.mode in ("I;16", "I;16B", "I"), im.mode
    a = np.array(im)
    assert a.shape == (480, 640) and a.min() >= 0 and a.max() <= 0xFFFF, (a.shape, a.min(), a.max())
    depth[name] = a.astype(np.uint16)
    mm = (depth[name] >> 3) | (depth[name] << 13)
    print(name, "holes %.2f %%, max depth %.3f m" % (100.0 * (mm == 0).mean(), mm.max() / 1000.0))
np.savez_compressed(os.path.join(here, "rgbd_depth.npz"), **depth)

for rel, name in (("INTRINSICS", "rgbd_intrinsics.txt"), ("match/match1_2", "rgbd_match1_2.bin"),
                  ("Rt/Rt1_2", "rgbd_Rt1_2.bin")):
    shutil.copyfile(os.path.join(src, rel), os.path.join(here, name))
    os.chmod(os.path.join(here, name), 0o644)
for name in ("rgbd_depth.npz", "rgbd_intrinsics.txt", "rgbd_match1_2.bin", "rgbd_Rt1_2.bin"):
    size = os.path.getsize(os.path.join(here, name))
    assert size < 466756, (name, size)  # below the largest fixture already committed (vlfeat_sift1.bin)
    print(name, size, "bytes")
