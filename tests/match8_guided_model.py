"""The definition of cusift_match8_guided / cusift_match8_projected (include/cusift_amd_extras.h), restated in numpy:
keys_model of tests/match8_model.py over the columns that pass a mask -- the lowest passing column with the smallest key,
the second smallest key of the passing multiset, the "exactly one" and "no column passes" rules.  The mask is guide_mask of
tests/test_match_guided.py or project_mask of tests/test_match_projected.py, the geometric tests restated bit for bit.
Shared by the test_match8_guided*.py files; no tolerance here."""
import numpy as np

from match8_model import INIT, SCALE, ambiguity_model, keys_model

NONE = np.int64(1) << 40  # above every key: a column that does not pass


def match8_guided_model(q1, q2, distance, xy2, mask):
    """The five fields cusift_match8_guided writes, as a dict of arrays [n1].  xy2: coords2D of set 2, float32 [n2, 2];
    mask: bool [n1, n2], column j passes against row i."""
    K = keys_model(q1, q2, distance)
    n1, n2 = K.shape
    mask = np.asarray(mask, bool)
    assert mask.shape == (n1, n2) and np.abs(K).max() < 2 ** 24
    K = np.where(mask, K, NONE)
    idx = K.argmin(1)  # the lowest column among equals
    best = K[np.arange(n1), idx]
    second_key = np.partition(K, 1, axis=1)[:, 1] if n2 > 1 else np.full(n1, NONE)  # of the passing multiset
    sign = 1 if distance == 1 else -1
    init = INIT[distance]
    passing = mask.sum(1)
    score = np.where(passing >= 1, (sign * best).astype(np.float32) * SCALE, init).astype(np.float32)
    second = np.where(passing >= 2, (sign * second_key).astype(np.float32) * SCALE, init).astype(np.float32)
    match = np.where(passing >= 1, idx, -1).astype(np.int32)
    at = np.where(passing >= 1, idx, 0)  # record 0's coordinates for a row that nothing passes
    xy2 = np.asarray(xy2, np.float32)
    return {"score": score, "ambiguity": ambiguity_model(score, second, distance), "match": match,
            "match_xpos": xy2[at, 0].copy(), "match_ypos": xy2[at, 1].copy()}


def row_categories(mask):
    """The shares of rows with no passing column, exactly one, and two or more."""
    passing = np.asarray(mask, bool).sum(1)
    return (passing == 0).mean(), (passing == 1).mean(), (passing >= 2).mean()
