"""--dump-outputs DIR: the SiftData of the last timed step, as .npy files, so that two builds can be compared output for
output.  The inputs are a fixed function of the arguments (seeded images), so the same command line gives the same
step on every run.

  counts.npy       float64 [B]       valid keypoints of every image of rank 0's batch (min(counter, maxPts))
  images.npy       float64 [S]       the sampled images' indices in the batch: a fixed, seeded choice of S = min(B, 16)
  keypoints.npy    float32 [n, 8]    image index, x, y, scale, sharpness, edgeness, orientation, subsampling
  descriptors.npy  float32 [n, 128]  the descriptors of the same rows

Rows are the sampled images' records in canonical order (the append order inside an octave is a race: it is sorted
away), image after image.  Each sampled image may fill 1/S of BUDGET_BYTES; one with more records contributes as many
as fit, evenly spaced in that order, which keeps the files under 64 MB at any maxPts.  The match fields of a SiftPoint are not written by extraction
and are left out."""
import os

import numpy as np

SAMPLE_IMAGES = 16
SAMPLE_SEED = 0
BUDGET_BYTES = 60 << 20
HEADER = ("x", "y", "scale", "sharpness", "edgeness", "orientation", "subsampling")


def sample_images(n_images):
    """The fixed, seeded choice of images (a function of the batch size only)."""
    k = min(n_images, SAMPLE_IMAGES)
    return np.sort(np.random.default_rng(SAMPLE_SEED).permutation(n_images)[:k])


def capture(capi, points, counts, max_pts):
    """Host copies of what the dump needs from one step's device tensors (points uint8 [B, max_pts, 588], counts int32
    [B]); the caller has synchronised with the step."""
    valid = np.minimum(counts.cpu().numpy().astype(np.int64), max_pts)
    idx = sample_images(len(valid))
    recs = [points[int(i), : int(valid[i])].cpu().numpy().view(capi.SIFT_POINT_DTYPE).reshape(-1) for i in idx]
    return valid, idx, recs


def _canonical(rec):
    keys = (rec["data"][:, 0], rec["edgeness"], rec["sharpness"], rec["orientation"], rec["scale"],
            rec["coords2D"][:, 0], rec["coords2D"][:, 1], rec["subsampling"])
    return rec[np.lexsort(keys)]


def write(out_dir, captured):
    valid, idx, recs = captured
    row_cap = max(1, BUDGET_BYTES // (max(1, len(idx)) * (len(HEADER) + 1 + 128) * 4))
    kps, descs = [], []
    for i, rec in zip(idx, recs):
        rec = _canonical(rec)
        if len(rec) > row_cap:
            rec = rec[np.linspace(0, len(rec) - 1, row_cap).round().astype(np.int64)]
        kp = np.empty((len(rec), len(HEADER) + 1), dtype=np.float32)
        kp[:, 0] = i
        kp[:, 1:3] = rec["coords2D"]
        for c, f in enumerate(HEADER[2:], start=3):
            kp[:, c] = rec[f]
        kps.append(kp)
        descs.append(np.asarray(rec["data"], dtype=np.float32))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "counts.npy"), valid.astype(np.float64))
    np.save(os.path.join(out_dir, "images.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "keypoints.npy"),
            np.concatenate(kps) if kps else np.zeros((0, len(HEADER) + 1), np.float32))
    np.save(os.path.join(out_dir, "descriptors.npy"), np.concatenate(descs) if descs else np.zeros((0, 128), np.float32))
