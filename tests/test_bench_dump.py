"""bench.py --dump-outputs (bench_legs/dump.py) on host data: a fixed image sample, files independent of the racy append
order inside an octave, and under 64 MB even when every image saturates maxPts."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_legs import dump  # noqa: E402
from cusift_amd import capi  # noqa: E402


def _batch(counts, max_pts, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((len(counts), max_pts, capi.SIFT_POINT_BYTES), np.uint8)
    for i, c in enumerate(counts):
        n = min(int(c), max_pts)
        r = np.zeros(n, capi.SIFT_POINT_DTYPE)
        # every field on a range of its own, so that a swapped or misplaced column cannot match
        r["coords2D"] = rng.integers(0, 1920, (n, 2)) + np.array([0.25, 0.5])
        r["scale"] = 2000 + rng.random(n)
        r["sharpness"] = 3000 + rng.random(n)
        r["edgeness"] = 4000 + rng.random(n)
        r["orientation"] = 5000 + rng.random(n)
        r["subsampling"] = 2.0 ** rng.integers(0, 5, n)
        r["data"] = rng.random((n, 128))
        # not written by extraction: must not reach the files
        for f in ("score", "ambiguity", "match_xpos", "match_ypos", "match_error", "empty", "coords3D"):
            r[f] = -7000 - rng.random(r[f].shape)
        r["match"] = -1
        pts[i, :n] = r.view(np.uint8).reshape(n, capi.SIFT_POINT_BYTES)
    return pts, np.asarray(counts, np.int32)


def _files(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_independent_of_the_append_order(tmp_path):
    pts, cnt = _batch(np.arange(64) * 7 + 100, 1024, seed=1)
    dump.write(str(tmp_path / "a"), dump.capture(capi, torch.from_numpy(pts), torch.from_numpy(cnt), 1024))
    rng = np.random.default_rng(2)
    for i, c in enumerate(cnt):
        pts[i, :c] = pts[i, :c][rng.permutation(c)]
    dump.write(str(tmp_path / "b"), dump.capture(capi, torch.from_numpy(pts), torch.from_numpy(cnt), 1024))
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == ["counts.npy", "descriptors.npy", "images.npy", "keypoints.npy"]
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["counts.npy"], cnt)
    assert np.array_equal(a["images.npy"], dump.sample_images(64)) and len(a["images.npy"]) == dump.SAMPLE_IMAGES
    assert len(a["keypoints.npy"]) == len(a["descriptors.npy"]) == cnt[dump.sample_images(64)].sum()
    assert np.array_equal(np.unique(a["keypoints.npy"][:, 0]), a["images.npy"])
    assert (a["keypoints.npy"] > -1000).all() and (a["descriptors.npy"] > -1000).all()


def test_dump_columns_are_the_record_fields(tmp_path):
    pts, cnt = _batch(np.arange(64) * 3 + 50, 512, seed=4)
    dump.write(str(tmp_path), dump.capture(capi, torch.from_numpy(pts), torch.from_numpy(cnt), 512))
    kp, desc = np.load(os.path.join(tmp_path, "keypoints.npy")), np.load(os.path.join(tmp_path, "descriptors.npy"))
    img = int(dump.sample_images(64)[5])
    rows = kp[:, 0] == img
    want = pts[img, : cnt[img]].view(capi.SIFT_POINT_DTYPE).reshape(-1)
    # the dump's order is canonical; match each written row to its record by the (unique) descriptor's first value
    want = want[np.argsort(want["data"][:, 0])]
    got_kp, got_desc = kp[rows], desc[rows]
    order = np.argsort(got_desc[:, 0])
    got_kp, got_desc = got_kp[order], got_desc[order]
    assert len(got_kp) == cnt[img]
    assert np.array_equal(got_kp[:, 1], want["coords2D"][:, 0]) and np.array_equal(got_kp[:, 2], want["coords2D"][:, 1])
    for c, f in enumerate(("scale", "sharpness", "edgeness", "orientation", "subsampling"), start=3):
        assert np.array_equal(got_kp[:, c], want[f]), f
    assert np.array_equal(got_desc, want["data"])


def test_dump_stays_under_64_mb_when_every_image_saturates(tmp_path):
    max_pts = 8192
    pts, cnt = _batch([max_pts + 5] * 16, max_pts, seed=3)
    dump.write(str(tmp_path), dump.capture(capi, torch.from_numpy(pts), torch.from_numpy(cnt), max_pts))
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total <= 64 << 20
    assert np.array_equal(np.load(os.path.join(tmp_path, "counts.npy")), [max_pts] * 16)
    assert len(np.load(os.path.join(tmp_path, "keypoints.npy"))) < 16 * max_pts
